// Skipping all-background windows in whole-volume prediction (additive to ABI 18; mivp_amd/inference.py WindowSkip,
// DESIGN 4.24).  Three launches around the sub-batch loop of csrc/stitch.hip and the blend inside it:
//   occupancy: foreground voxels per window (fp32 volume channel > threshold, or uint8 mask != 0), exact integers
//   compact  : the kept entries of the immutable full work list, in their original order, into the active work list the
//              gather / blend / recorded graph read; the rest of the active list is zero (invalid)
//   blend_any: the blend of a compacted sub-batch, whose union box can outgrow the launch grid of the recorded graph
//   fill     : voxels no kept window covered (wsum == 0) get the fill logits and wsum = 1, so that the unchanged finalize
//              kernels produce the fill result
// Integer atomics and an ordered block scan only: every result is bitwise reproducible.
// The window geometry (Geo, fill_geo, MAXC, TPB) is csrc/window_common.hpp's, shared with stitch.hip and window_fit.hip.
#include "window_common.hpp"

namespace {
constexpr int WAVES = TPB / 64;

MIVP_DEV int fg(float v, float thr) { return v > thr ? 1 : 0; }          // strict: NaN is not foreground
MIVP_DEV int fg(uint8_t v, float) { return v != 0 ? 1 : 0; }

// four consecutive D voxels in one load: 16 bytes of the fp32 volume, 4 bytes of the uint8 mask
MIVP_DEV int fg4(const float* p, float thr) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    return fg(v.x, thr) + fg(v.y, thr) + fg(v.z, thr) + fg(v.w, thr);
}
MIVP_DEV int fg4(const uint8_t* p, float) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    return ((v & 0xFFu) != 0) + ((v & 0xFF00u) != 0) + ((v & 0xFF0000u) != 0) + ((v & 0xFF000000u) != 0);
}

// grid (window, slab): a slab is `rows_per_slab` consecutive (i, j) rows of the window; one thread = four consecutive D
// voxels of a row at a time.  Sum in the wave, across the waves through LDS, one integer atomic per workgroup.
// src points at the channel's [H][W][D] block.  vec_ok: D % 4 == 0 and an aligned base, so every row base is aligned.
template <typename T>
__global__ __launch_bounds__(TPB) void k_window_occupancy(const T* __restrict__ src, float thr, Geo g,
                                                          const int* __restrict__ origins, int ostride, int rows_per_slab,
                                                          int vec_ok, int* __restrict__ counts) {
    __shared__ int s_part[WAVES];
    const int w = blockIdx.x;
    const int o0 = origins[(long)w * ostride + 0], o1 = origins[(long)w * ostride + 1], o2 = origins[(long)w * ostride + 2];
    // (uniform) an origin outside the padded volume counts nothing and reads nothing
    if (o0 < 0 || o1 < 0 || o2 < 0 || o0 + g.r[0] > g.p[0] || o1 + g.r[1] > g.p[1] || o2 + g.r[2] > g.p[2]) return;
    const int rows = g.r[0] * g.r[1];
    const int row_lo = blockIdx.y * rows_per_slab;
    const int row_hi = min(rows, row_lo + rows_per_slab);
    const int r2q = (g.r[2] + 3) >> 2;
    const int items = max(row_hi - row_lo, 0) * r2q;
    const int dbase = o2 - g.pad[2];                           // image coordinate of a row's element 0
    int cnt = 0;
    for (int it = threadIdx.x; it < items; it += TPB) {
        const int q = it % r2q;
        const int row = row_lo + it / r2q;
        const int i = row / g.r[1], j = row - i * g.r[1];
        const int h = o0 + i - g.pad[0], x1 = o1 + j - g.pad[1];
        if (h < 0 || h >= g.n[0] || x1 < 0 || x1 >= g.n[1]) continue;      // a row of the zero padding
        const T* rp = src + ((long)h * g.n[1] + x1) * g.n[2];
        const int d0 = dbase + 4 * q;
        const int kn = min(4, g.r[2] - 4 * q);
        if (vec_ok && kn == 4 && d0 >= 0 && d0 + 4 <= g.n[2] && (d0 & 3) == 0) {
            cnt += fg4(rp + d0, thr);
        } else {
            for (int e = 0; e < kn; ++e) {
                const int d = d0 + e;
                if (d >= 0 && d < g.n[2]) cnt += fg(rp[d], thr);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) total += s_part[k];
        if (total) atomicAdd(&counts[w], total);
    }
}

// one workgroup, chunks of TPB entries: an ordered block prefix scan (wave ballots, wave totals through LDS)
__global__ __launch_bounds__(TPB) void k_window_compact(const int4* __restrict__ full, int n_entries, int n_windows, int F,
                                                        const int* __restrict__ counts, int min_voxels,
                                                        int4* __restrict__ table, int* __restrict__ meta) {
    __shared__ int s_wave[WAVES], s_first[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int kept_entries = 0, kept_windows = 0;                    // running totals, the same in every thread
    for (int base = 0; base < n_entries; base += TPB) {
        const int e = base + threadIdx.x;
        int4 row = make_int4(0, 0, 0, 0);
        bool keep = false, first = false;
        if (e < n_entries) {
            const int w = e / F;
            row = full[e];
            keep = (row.w & 1) != 0 && w < n_windows && counts[w] >= min_voxels;
            first = keep && e - w * F == 0;
        }
        const unsigned long long m = __ballot(keep), mf = __ballot(first);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) { s_wave[wave] = __popcll(m); s_first[wave] = __popcll(mf); }
        __syncthreads();
        int off = kept_entries, tot = 0, totf = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) {
            if (k < wave) off += s_wave[k];
            tot += s_wave[k];
            totf += s_first[k];
        }
        if (keep) table[off + before] = row;                   // off + before <= e: inside the table
        kept_entries += tot;
        kept_windows += totf;
        __syncthreads();
    }
    for (int e = kept_entries + threadIdx.x; e < n_entries; e += TPB) table[e] = make_int4(0, 0, 0, 0);
    if (threadIdx.x == 0) { meta[0] = kept_windows; meta[1] = kept_entries; }
}

// The blend of a COMPACTED sub-batch.  Its union box can be any part of the padded volume (two kept windows at opposite
// corners), while the launch grid of a recorded graph is fixed: this kernel keeps the grid the unfiltered predictor
// launches (the largest union box of a sub-batch of the full list, U0 U1 U2 threads) and walks the current box with a
// grid stride, so a larger box costs more iterations, not more workgroups, and no box is ever dropped.  Per voxel it
// is k_window_blend_tta of csrc/stitch.hip statement for statement (entries staged in LDS, contributions in increasing
// entry index, COMP = the compensated sums): with the full list it computes the same bits.
template <bool COMP>
__global__ __launch_bounds__(TPB) void k_window_blend_any(const float* __restrict__ logits, int channels_last, int C, Geo g,
                                                          const int* __restrict__ table, int n_entries,
                                                          const int* __restrict__ sub_idx, int B,
                                                          const float* __restrict__ w0, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, float w_floor,
                                                          float* __restrict__ acc, float* __restrict__ wsum,
                                                          float* __restrict__ comp) {
    __shared__ int4 s_e[TPB];
    __shared__ int s_box[6];
    const long wbase = (long)sub_idx[0] * B;
    if (wbase < 0 || wbase >= n_entries) return;               // (uniform: every thread reads the same word)
    const int nb = (int)min((long)B, n_entries - wbase);
    const int4* tab = reinterpret_cast<const int4*>(table) + wbase;
    if (threadIdx.x < 3) s_box[threadIdx.x] = INT_MAX;
    else if (threadIdx.x < 6) s_box[threadIdx.x] = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += TPB) {
        const int4 e = tab[b];
        if (!(e.w & 1)) continue;
        atomicMin(&s_box[0], e.x); atomicMin(&s_box[1], e.y); atomicMin(&s_box[2], e.z);
        atomicMax(&s_box[3], e.x + g.r[0]); atomicMax(&s_box[4], e.y + g.r[1]); atomicMax(&s_box[5], e.z + g.r[2]);
    }
    __syncthreads();
    const int lo0 = s_box[0], lo1 = s_box[1], lo2 = s_box[2];
    const int hi0 = min(s_box[3], g.p[0]), hi1 = min(s_box[4], g.p[1]), hi2 = min(s_box[5], g.p[2]);
    if (lo0 >= hi0 || lo1 >= hi1 || lo2 >= hi2 || lo0 < 0 || lo1 < 0 || lo2 < 0) return;   // nothing valid (uniform)
    const int b1 = hi1 - lo1, b2 = hi2 - lo2;
    const long bvol = (long)(hi0 - lo0) * b1 * b2;             // inside the padded volume: every voxel index is in range
    const long rvol = (long)g.r[0] * g.r[1] * g.r[2];
    const long cs = channels_last ? 1 : rvol;
    const long step = (long)gridDim.x * TPB;
    for (long base = (long)blockIdx.x * TPB; base < bvol; base += step) {   // (uniform per workgroup: barriers inside)
        const long t = base + threadIdx.x;
        const bool active = t < bvol;                          // the rest stay for the barriers and touch no memory
        const long tc = active ? t : 0;
        const int p2 = lo2 + (int)(tc % b2);
        const int p1 = lo1 + (int)((tc / b2) % b1);
        const int p0 = lo0 + (int)(tc / b2 / b1);
        const long v = active ? ((long)p0 * g.p[1] + p1) * g.p[2] + p2 : 0;
        float a[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) a[c] = (active && c < C) ? acc[v * C + c] : 0.f;
        float s = active ? wsum[v] : 0.f;
        float ca[COMP ? MAXC : 1], cw = 0.f;
        if (COMP) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) ca[c] = (active && c < C) ? comp[v * (C + 1) + c] : 0.f;
            cw = active ? comp[v * (C + 1) + C] : 0.f;
        }
        bool any = false;
        for (int b0 = 0; b0 < nb; b0 += TPB) {
            const int nc = min(TPB, nb - b0);
            __syncthreads();
            if ((int)threadIdx.x < nc) s_e[threadIdx.x] = tab[b0 + threadIdx.x];
            __syncthreads();
            if (!active) continue;
            for (int b = 0; b < nc; ++b) {                     // increasing entry index
                const int4 e = s_e[b];
                if (!(e.w & 1)) continue;
                const int i = p0 - e.x, j = p1 - e.y, k = p2 - e.z;
                if (i < 0 || i >= g.r[0] || j < 0 || j >= g.r[1] || k < 0 || k >= g.r[2]) continue;
                const float wt = fmaxf(w0[i] * w1[j] * w2[k], w_floor);   // the map is indexed in volume coordinates: not flipped
                const int code = e.w >> 1;
                const int fi = (code & 1) ? g.r[0] - 1 - i : i;
                const int fj = (code & 2) ? g.r[1] - 1 - j : j;
                const int fk = (code & 4) ? g.r[2] - 1 - k : k;
                const long lv = ((long)fi * g.r[1] + fj) * g.r[2] + fk;
                const long slot = b0 + b;
                const float* src = channels_last ? logits + (slot * rvol + lv) * C : logits + slot * C * rvol + lv;
                if (COMP) {                                    // explicit roundings: nothing here may be re-associated
#pragma unroll
                    for (int c = 0; c < MAXC; ++c)
                        if (c < C) {
                            const float y = __fmaf_rn(wt, src[c * cs], -ca[c]);
                            const float tt = __fadd_rn(a[c], y);
                            ca[c] = __fsub_rn(__fsub_rn(tt, a[c]), y);
                            a[c] = tt;
                        }
                    const float y = __fsub_rn(wt, cw);
                    const float tt = __fadd_rn(s, y);
                    cw = __fsub_rn(__fsub_rn(tt, s), y);
                    s = tt;
                } else {
#pragma unroll
                    for (int c = 0; c < MAXC; ++c)
                        if (c < C) a[c] += wt * src[c * cs];
                    s += wt;
                }
                any = true;
            }
        }
        if (!any) continue;                                    // (active threads only; no barrier before the next iteration's)
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) acc[v * C + c] = a[c];
        wsum[v] = s;
        if (COMP) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) comp[v * (C + 1) + c] = ca[c];
            comp[v * (C + 1) + C] = cw;
        }
    }
}

__global__ __launch_bounds__(TPB) void k_stitch_fill(float* __restrict__ acc, float* __restrict__ wsum, int C, long nvox,
                                                     int fill_class, float fill_logit) {
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < nvox; v += (long)gridDim.x * TPB) {
        if (wsum[v] != 0.f) continue;
        for (int c = 0; c < C; ++c) acc[v * C + c] = c == fill_class ? fill_logit : -fill_logit;
        wsum[v] = 1.f;
    }
}
}  // namespace

extern "C" int mivp_window_occupancy(const float* vol, int32_t Cin, int32_t channel, float threshold, const uint8_t* mask,
                                     const int32_t* dims, const int32_t* pad, const int32_t* pdims, const int32_t* roi,
                                     const int32_t* origins, int32_t origin_stride, int32_t n_windows, int32_t* counts,
                                     mivp_stream_t stream) {
    MIVP_REQUIRE(origins && counts && dims && pad && pdims && roi);
    MIVP_REQUIRE((vol != nullptr) != (mask != nullptr));
    MIVP_REQUIRE(origin_stride == 3 || origin_stride == 4);
    MIVP_REQUIRE(n_windows >= 1 && n_windows <= (1 << 24));
    if (vol) MIVP_REQUIRE(Cin >= 1 && Cin <= 4 && channel >= 0 && channel < Cin);
    Geo g;
    MIVP_REQUIRE(fill_geo(g, dims, pad, pdims, roi));
    // slabs: enough workgroups to fill the chip when there are few large windows, never less than ~4 items per thread
    const long rows = (long)g.r[0] * g.r[1];
    const long items = rows * ((g.r[2] + 3) / 4);
    long slabs = (2048 + n_windows - 1) / n_windows;
    const long most = items / (4 * TPB) > 1 ? items / (4 * TPB) : 1;
    if (slabs > most) slabs = most;
    if (slabs > rows) slabs = rows;
    const int rows_per_slab = (int)((rows + slabs - 1) / slabs);
    slabs = (rows + rows_per_slab - 1) / rows_per_slab;
    MIVP_REQUIRE(slabs <= 65535);
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_windows, (hipStream_t)stream);
    if (e != hipSuccess) { mivp_set_error(hipGetErrorString(e)); return MIVP_ELAUNCH; }
    const dim3 grid((unsigned)n_windows, (unsigned)slabs);
    if (vol) {
        const float* src = vol + (long)channel * g.n[0] * g.n[1] * g.n[2];
        const int vec_ok = reinterpret_cast<uintptr_t>(vol) % 16 == 0 && g.n[2] % 4 == 0;
        hipLaunchKernelGGL(k_window_occupancy<float>, grid, dim3(TPB), 0, (hipStream_t)stream, src, threshold, g, origins,
                           (int)origin_stride, rows_per_slab, vec_ok, (int*)counts);
    } else {
        const int vec_ok = reinterpret_cast<uintptr_t>(mask) % 4 == 0 && g.n[2] % 4 == 0;
        hipLaunchKernelGGL(k_window_occupancy<uint8_t>, grid, dim3(TPB), 0, (hipStream_t)stream, mask, 0.f, g, origins,
                           (int)origin_stride, rows_per_slab, vec_ok, (int*)counts);
    }
    return mivp_check_launch("window_occupancy");
}

extern "C" int mivp_window_compact(const int32_t* full_table, int32_t n_entries, int32_t n_windows, int32_t n_flips,
                                   const int32_t* counts, int32_t min_voxels, int32_t* table, int32_t* meta,
                                   mivp_stream_t stream) {
    MIVP_REQUIRE(full_table && counts && table && meta && full_table != table);
    MIVP_REQUIRE(n_windows >= 1 && n_flips >= 1 && n_flips <= 8 && min_voxels >= 1);
    MIVP_REQUIRE(n_entries >= 1 && (long)n_windows * n_flips <= n_entries);
    MIVP_REQUIRE(reinterpret_cast<uintptr_t>(full_table) % 16 == 0 && reinterpret_cast<uintptr_t>(table) % 16 == 0);
    hipLaunchKernelGGL(k_window_compact, dim3(1), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(full_table), (int)n_entries, (int)n_windows, (int)n_flips, counts,
                       (int)min_voxels, reinterpret_cast<int4*>(table), (int*)meta);
    return mivp_check_launch("window_compact");
}

extern "C" int mivp_window_blend_any(const float* logits, int32_t channels_last, int32_t C, const int32_t* pdims,
                                     const int32_t* roi, const int32_t* table, int32_t n_entries, const int32_t* sub_idx,
                                     int32_t B, const int32_t* ubox, const float* w0, const float* w1, const float* w2,
                                     float w_floor, float* acc, float* wsum, float* comp, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && table && sub_idx && pdims && roi && ubox && w0 && w1 && w2 && acc && wsum);
    MIVP_REQUIRE(C >= 1 && C <= MAXC && B >= 1 && n_entries >= B && n_entries % B == 0);
    MIVP_REQUIRE(reinterpret_cast<uintptr_t>(table) % 16 == 0);
    const int32_t zero[3] = {0, 0, 0};
    Geo g;
    MIVP_REQUIRE(fill_geo(g, pdims, zero, pdims, roi));
    for (int a = 0; a < 3; ++a) MIVP_REQUIRE(ubox[a] >= g.r[a] && ubox[a] <= g.p[a]);
    const long total = (long)ubox[0] * ubox[1] * ubox[2];      // the grid only: a larger box is walked with a stride
    const auto kern = comp ? k_window_blend_any<true> : k_window_blend_any<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, logits,
                       (int)(channels_last != 0), (int)C, g, table, (int)n_entries, sub_idx, (int)B, w0, w1, w2, w_floor,
                       acc, wsum, comp);
    return mivp_check_launch("window_blend_any");
}

extern "C" int mivp_stitch_fill(float* acc, float* wsum, int32_t C, const int32_t* pdims, int32_t fill_class,
                                float fill_logit, mivp_stream_t stream) {
    MIVP_REQUIRE(acc && wsum && pdims && C >= 1 && C <= MAXC && fill_class >= 0 && fill_class < C);
    MIVP_REQUIRE(fill_logit > 0.f && fill_logit < INFINITY);
    const int32_t zero[3] = {0, 0, 0}, one[3] = {1, 1, 1};
    Geo g;
    MIVP_REQUIRE(fill_geo(g, pdims, zero, pdims, one));
    const long nvox = (long)g.p[0] * g.p[1] * g.p[2];
    const unsigned grid = (unsigned)((nvox + TPB - 1) / TPB > 2048 ? 2048 : (nvox + TPB - 1) / TPB);
    hipLaunchKernelGGL(k_stitch_fill, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, acc, wsum, (int)C, nvox, (int)fill_class,
                       fill_logit);
    return mivp_check_launch("stitch_fill");
}
