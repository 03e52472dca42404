// Whole-volume sliding-window prediction (ABI 14, mivp_amd/inference.py SlidingWindowPredictor): the windows of one
// sub-batch are cut out of the resident volume straight into the model's input tensor, the model's logits are blended
// into a whole-volume accumulator with a separable importance map, and one pass turns the accumulator into a label map
// (plus, on request, the blended logits and the whole-volume Dice / IoU counts).
//
// Every kernel reads the sub-batch index from a device word (`sub_idx`) that mivp_window_advance bumps at the end of a
// sub-batch, so gather -> model -> blend -> advance records once as a graph and replays without host work.
//
// Window table: int32 [n_entries][4] = (o0, o1, o2, valid), origins in PADDED-volume coordinates (a volume axis shorter
// than the roi is zero-padded to the roi; `pad` voxels in front).  Entry w belongs to sub-batch w / B, slot w % B.
//
// The blend is a gather over voxels, with no float atomics: one thread per voxel of the union box of the sub-batch's
// windows loads its accumulator, adds the weighted logits of the covering windows in increasing window index, and
// stores it.  Sub-batches run in stream order, so every voxel sums its contributions in global window order whatever the
// sub-batch size.
//
// Mirror test-time augmentation (ABI 18, the _tta entries): word 3 of a table entry is valid | code << 1, where bit a of the
// 3-bit code flips roi axis a.  The work list holds every window under every code, window-major; the gather hands the model
// the flipped window, the blend reads the logits through the same flip and weights them by the UNFLIPPED importance map, in
// increasing entry index.  With code 0 everywhere both kernels compute what the plain ones compute, bit for bit.
//
// The window geometry (Geo, fill_geo, MAXC, TPB) and the plain accumulation of one contribution (add_weighted) are
// csrc/window_common.hpp's, shared with window_skip.hip and window_fit.hip.
// In this file the two finalize kernels share padded_index / count_voxel and their entry points finalize_setup; the two
// gather entry points share launch_gather.
#include "window_common.hpp"

namespace {
// one thread = four consecutive D outputs of one (window, channel, i, j) row
__global__ __launch_bounds__(TPB) void k_window_gather(const float* __restrict__ vol, int Cin, Geo g,
                                                       const int* __restrict__ table, int n_entries,
                                                       const int* __restrict__ sub_idx, int B, int vec_ok,
                                                       float* __restrict__ out) {
    const int r2q = (g.r[2] + 3) >> 2;
    const long total = (long)B * Cin * g.r[0] * g.r[1] * r2q;
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % r2q);
    const long row = t / r2q;                                  // ((b * Cin + c) * r0 + i) * r1 + j
    const int j = (int)(row % g.r[1]);
    long rest = row / g.r[1];
    const int i = (int)(rest % g.r[0]);
    rest /= g.r[0];
    const int c = (int)(rest % Cin);
    const int b = (int)(rest / Cin);
    const long w = (long)sub_idx[0] * B + b;
    bool ok = w >= 0 && w < n_entries && table[w * 4 + 3] != 0;
    int h = 0, x1 = 0, d0 = 0;
    if (ok) {
        h = table[w * 4 + 0] + i - g.pad[0];
        x1 = table[w * 4 + 1] + j - g.pad[1];
        d0 = table[w * 4 + 2] + 4 * q - g.pad[2];
    }
    ok = ok && h >= 0 && h < g.n[0] && x1 >= 0 && x1 < g.n[1];
    const float* src = vol + (((long)c * g.n[0] + (ok ? h : 0)) * g.n[1] + (ok ? x1 : 0)) * g.n[2];
    float* dst = out + row * g.r[2] + 4 * q;
    if (vec_ok) {                                              // D % 4 == 0, r2 % 4 == 0, 16-byte aligned bases
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && d0 >= 0 && d0 + 4 <= g.n[2] && (d0 & 3) == 0) {
            v = *reinterpret_cast<const float4*>(src + d0);
        } else if (ok) {
            v.x = (d0 >= 0 && d0 < g.n[2]) ? src[d0] : 0.f;
            v.y = (d0 + 1 >= 0 && d0 + 1 < g.n[2]) ? src[d0 + 1] : 0.f;
            v.z = (d0 + 2 >= 0 && d0 + 2 < g.n[2]) ? src[d0 + 2] : 0.f;
            v.w = (d0 + 3 >= 0 && d0 + 3 < g.n[2]) ? src[d0 + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        const int kn = min(4, g.r[2] - 4 * q);
        for (int e = 0; e < kn; ++e) {
            const int d = d0 + e;
            dst[e] = (ok && d >= 0 && d < g.n[2]) ? src[d] : 0.f;
        }
    }
}

// one thread = one voxel of the current sub-batch's union box; the grid covers the largest union box (ubox)
__global__ __launch_bounds__(TPB) void k_window_blend(const float* __restrict__ logits, int channels_last, int C, Geo g,
                                                      const int* __restrict__ table, int n_entries,
                                                      const int* __restrict__ sub_idx, int B, int U0, int U1, int U2,
                                                      const float* __restrict__ w0, const float* __restrict__ w1,
                                                      const float* __restrict__ w2, float w_floor,
                                                      float* __restrict__ acc, float* __restrict__ wsum) {
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= (long)U0 * U1 * U2) return;
    const int u2 = (int)(t % U2);
    const long tr = t / U2;
    const int u1 = (int)(tr % U1);
    const int u0 = (int)(tr / U1);
    const long wbase = (long)sub_idx[0] * B;
    if (wbase < 0 || wbase >= n_entries) return;
    const int nb = (int)min((long)B, n_entries - wbase);
    int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = 0, hi1 = 0, hi2 = 0;
    for (int b = 0; b < nb; ++b) {
        const int* e = table + (wbase + b) * 4;
        if (!e[3]) continue;
        lo0 = min(lo0, e[0]); lo1 = min(lo1, e[1]); lo2 = min(lo2, e[2]);
        hi0 = max(hi0, e[0] + g.r[0]); hi1 = max(hi1, e[1] + g.r[1]); hi2 = max(hi2, e[2] + g.r[2]);
    }
    if (lo0 >= hi0) return;                                    // no valid window in this sub-batch
    const int p0 = lo0 + u0, p1 = lo1 + u1, p2 = lo2 + u2;
    if (p0 >= hi0 || p1 >= hi1 || p2 >= hi2) return;
    const long v = ((long)p0 * g.p[1] + p1) * g.p[2] + p2;
    const long rvol = (long)g.r[0] * g.r[1] * g.r[2];
    float a[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) a[c] = c < C ? acc[v * C + c] : 0.f;
    float s = wsum[v];
    bool any = false;
    for (int b = 0; b < nb; ++b) {                             // increasing window index
        const int* e = table + (wbase + b) * 4;
        if (!e[3]) continue;
        const int i = p0 - e[0], j = p1 - e[1], k = p2 - e[2];
        if (i < 0 || i >= g.r[0] || j < 0 || j >= g.r[1] || k < 0 || k >= g.r[2]) continue;
        const float wt = fmaxf(w0[i] * w1[j] * w2[k], w_floor);
        const long lv = ((long)i * g.r[1] + j) * g.r[2] + k;
        const float* src = channels_last ? logits + ((long)b * rvol + lv) * C : logits + (long)b * C * rvol + lv;
        const long cs = channels_last ? 1 : rvol;
        add_weighted(a, C, wt, src, cs);
        s += wt;
        any = true;
    }
    if (!any) return;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) acc[v * C + c] = a[c];
    wsum[v] = s;
}

// What k_stitch_finalize and k_stitch_finalize_probs share.  Image voxel v -> its index in the padded volume:
MIVP_DEV long padded_index(long v, const Geo& g) {
    const int d = (int)(v % g.n[2]);
    const long r = v / g.n[2];
    const int x1 = (int)(r % g.n[1]);
    const int h = (int)(r / g.n[1]);
    return ((long)(h + g.pad[0]) * g.p[1] + (x1 + g.pad[1])) * g.p[2] + (d + g.pad[2]);
}
// the workgroup's Dice / IoU counts in LDS, sm[class][intersection, predicted, target]: one voxel
MIVP_DEV void count_voxel(unsigned int* sm, int best, float tv, int C) {
    atomicAdd(&sm[best * 3 + 1], 1u);
    for (int c = 0; c < C; ++c)
        if (tv == (float)c) { atomicAdd(&sm[c * 3 + 2], 1u); if (best == c) atomicAdd(&sm[c * 3 + 0], 1u); }
}

// acc / wsum over the image (cropped out of the padded volume), first arg-max, optional logits and counts
__global__ __launch_bounds__(TPB) void k_stitch_finalize(const float* __restrict__ acc, const float* __restrict__ wsum, int C,
                                                         Geo g, uint8_t* __restrict__ labels, float* __restrict__ out,
                                                         const float* __restrict__ target,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ unsigned int sm[MAXC * 3];
    for (int i = threadIdx.x; i < MAXC * 3; i += TPB) sm[i] = 0u;
    __syncthreads();
    const long nvox = (long)g.n[0] * g.n[1] * g.n[2];
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < nvox; v += (long)gridDim.x * TPB) {
        const long pv = padded_index(v, g);
        const float s = wsum[pv];
        int best = 0;
        float bv = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c >= C) break;
            const float x = acc[pv * C + c] / s;
            if (out) out[(long)c * nvox + v] = x;
            if (c == 0 || x > bv) { bv = x; best = c; }       // first maximum, like torch.argmax
        }
        labels[v] = (uint8_t)best;
        if (target) count_voxel(sm, best, target[v], C);
    }
    if (!target) return;                                       // (uniform: the whole grid returns together)
    __syncthreads();
    for (int i = threadIdx.x; i < C * 3; i += TPB)
        if (sm[i]) atomicAdd(&counts[i], (unsigned long long)sm[i]);
}

// ABI 18.  As k_window_gather, reading each row through the entry's flip code: H / W flips change the row address, a D flip
// loads the mirrored quad (one 16-byte load where aligned) and reverses its lanes in registers.
__global__ __launch_bounds__(TPB) void k_window_gather_tta(const float* __restrict__ vol, int Cin, Geo g,
                                                           const int* __restrict__ table, int n_entries,
                                                           const int* __restrict__ sub_idx, int B, int vec_ok,
                                                           float* __restrict__ out) {
    const int r2q = (g.r[2] + 3) >> 2;
    const long total = (long)B * Cin * g.r[0] * g.r[1] * r2q;
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % r2q);
    const long row = t / r2q;                                  // ((b * Cin + c) * r0 + i) * r1 + j
    const int j = (int)(row % g.r[1]);
    long rest = row / g.r[1];
    const int i = (int)(rest % g.r[0]);
    rest /= g.r[0];
    const int c = (int)(rest % Cin);
    const int b = (int)(rest / Cin);
    const long w = (long)sub_idx[0] * B + b;
    bool ok = w >= 0 && w < n_entries && (table[w * 4 + 3] & 1) != 0;
    int h = 0, x1 = 0, dbase = 0, fd = 0;
    if (ok) {
        const int code = table[w * 4 + 3] >> 1;
        fd = (code >> 2) & 1;
        h = table[w * 4 + 0] + ((code & 1) ? g.r[0] - 1 - i : i) - g.pad[0];
        x1 = table[w * 4 + 1] + ((code & 2) ? g.r[1] - 1 - j : j) - g.pad[1];
        dbase = table[w * 4 + 2] - g.pad[2];                   // image coordinate of the row's element 0
    }
    ok = ok && h >= 0 && h < g.n[0] && x1 >= 0 && x1 < g.n[1];
    const float* src = vol + (((long)c * g.n[0] + (ok ? h : 0)) * g.n[1] + (ok ? x1 : 0)) * g.n[2];
    float* dst = out + row * g.r[2] + 4 * q;
    if (vec_ok) {                                              // D % 4 == 0, r2 % 4 == 0, 16-byte aligned bases
        const int d0 = dbase + (fd ? g.r[2] - 4 - 4 * q : 4 * q);  // lowest source index of this quad
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && d0 >= 0 && d0 + 4 <= g.n[2] && (d0 & 3) == 0) {
            v = *reinterpret_cast<const float4*>(src + d0);
        } else if (ok) {
            v.x = (d0 >= 0 && d0 < g.n[2]) ? src[d0] : 0.f;
            v.y = (d0 + 1 >= 0 && d0 + 1 < g.n[2]) ? src[d0 + 1] : 0.f;
            v.z = (d0 + 2 >= 0 && d0 + 2 < g.n[2]) ? src[d0 + 2] : 0.f;
            v.w = (d0 + 3 >= 0 && d0 + 3 < g.n[2]) ? src[d0 + 3] : 0.f;
        }
        if (fd) v = make_float4(v.w, v.z, v.y, v.x);
        *reinterpret_cast<float4*>(dst) = v;
    } else {
        const int kn = min(4, g.r[2] - 4 * q);
        for (int e = 0; e < kn; ++e) {
            const int k = 4 * q + e;
            const int d = dbase + (fd ? g.r[2] - 1 - k : k);
            dst[e] = (ok && d >= 0 && d < g.n[2]) ? src[d] : 0.f;
        }
    }
}

// ABI 18.  As k_window_blend, with the logits read through each entry's flip code.  The sub-batch's entries are staged in
// LDS once per workgroup (TPB at a time) and its union box is reduced there with integer atomics, so a thread reads the
// table from LDS instead of 2 B global words; the flips of one window sit next to each other in the work list, so one
// accumulator read serves several contributions.
// COMP: compensated (Kahan) accumulation, still in increasing entry index.  comp f32 [pdims][C + 1] carries the running
// rounding error of every accumulator word and of the weight sum from launch to launch, so the state a voxel carries is
// the same whatever the sub-batch size, and acc / wsum stay what the finalize reads.  F times as many contributions then
// round like a handful.  Without it (comp == NULL) the arithmetic is k_window_blend's.
template <bool COMP>
__global__ __launch_bounds__(TPB) void k_window_blend_tta(const float* __restrict__ logits, int channels_last, int C, Geo g,
                                                          const int* __restrict__ table, int n_entries,
                                                          const int* __restrict__ sub_idx, int B, int U0, int U1, int U2,
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
    // threads are laid over the CURRENT box, not the largest one the grid was sized for (U0 U1 U2 >= this volume): the
    // workgroups past its end leave here together, and the ones that stay have no holes
    const int b1 = hi1 - lo1, b2 = hi2 - lo2;
    const long bvol = (long)(hi0 - lo0) * b1 * b2;
    if ((long)blockIdx.x * TPB >= bvol || bvol > (long)U0 * U1 * U2) return;
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    const bool active = t < bvol;                              // the rest stay for the barriers and touch no memory
    const long tc = active ? t : 0;
    const int p2 = lo2 + (int)(tc % b2);
    const int p1 = lo1 + (int)((tc / b2) % b1);
    const int p0 = lo0 + (int)(tc / b2 / b1);
    const long v = active ? ((long)p0 * g.p[1] + p1) * g.p[2] + p2 : 0;
    const long rvol = (long)g.r[0] * g.r[1] * g.r[2];
    const long cs = channels_last ? 1 : rvol;
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
        for (int b = 0; b < nc; ++b) {                         // increasing entry index
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
            if (COMP) {                                        // explicit roundings: nothing here may be re-associated
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
                add_weighted(a, C, wt, src, cs);
                s += wt;
            }
            any = true;
        }
    }
    if (!any) return;
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

// ABI 18.  k_stitch_finalize plus the probability maps: one read of acc / wsum per voxel, the class values stay in registers.
// The labels come from the same quotients and the same comparison as k_stitch_finalize.
__global__ __launch_bounds__(TPB) void k_stitch_finalize_probs(const float* __restrict__ acc, const float* __restrict__ wsum,
                                                               int C, Geo g, uint8_t* __restrict__ labels,
                                                               float* __restrict__ out, float* __restrict__ probs,
                                                               float* __restrict__ conf, float* __restrict__ entropy,
                                                               const float* __restrict__ target,
                                                               unsigned long long* __restrict__ counts) {
    __shared__ unsigned int sm[MAXC * 3];
    for (int i = threadIdx.x; i < MAXC * 3; i += TPB) sm[i] = 0u;
    __syncthreads();
    const long nvox = (long)g.n[0] * g.n[1] * g.n[2];
    const float inv_lnc = C > 1 ? 1.f / logf((float)C) : 0.f;
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < nvox; v += (long)gridDim.x * TPB) {
        const long pv = padded_index(v, g);
        const float s = wsum[pv];
        float x[MAXC];
        int best = 0;
        float bv = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            x[c] = 0.f;
            if (c >= C) continue;
            x[c] = acc[pv * C + c] / s;
            if (out) out[(long)c * nvox + v] = x[c];
            if (c == 0 || x[c] > bv) { bv = x[c]; best = c; }  // first maximum, like torch.argmax
        }
        labels[v] = (uint8_t)best;
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) { x[c] -= bv; den += __expf(x[c]); }    // x <= 0 from here on; the maximum contributes exactly 1
        const float inv = 1.f / den;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (c >= C) continue;
            const float pc = __expf(x[c]) * inv;
            if (probs) probs[(long)c * nvox + v] = pc;
            if (pc > 0.f) dot += pc * x[c];
        }
        if (conf) conf[v] = inv;                               // the maximum probability: exp(0) / den
        // -sum p ln p = ln den - sum p (x - max)
        if (entropy) entropy[v] = fminf(fmaxf((logf(den) - dot) * inv_lnc, 0.f), 1.f);
        if (target) count_voxel(sm, best, target[v], C);
    }
    if (!target) return;                                       // (uniform: the whole grid returns together)
    __syncthreads();
    for (int i = threadIdx.x; i < C * 3; i += TPB)
        if (sm[i]) atomicAdd(&counts[i], (unsigned long long)sm[i]);
}

// a separate one-thread launch: the blend's workgroups all read the word, so none of them may bump it
__global__ void k_window_advance(int* __restrict__ sub_idx) { sub_idx[0] = sub_idx[0] + 1; }

// the one host-side launcher of the two gather kernels (they take the same arguments)
int launch_gather(decltype(&k_window_gather) kern, const char* what, const float* vol, int32_t Cin, const int32_t* dims,
                  const int32_t* pad, const int32_t* pdims, const int32_t* roi, const int32_t* table, int32_t n_entries,
                  const int32_t* sub_idx, int32_t B, float* out, mivp_stream_t stream) {
    MIVP_REQUIRE(vol && out && table && sub_idx && dims && pad && pdims && roi);
    MIVP_REQUIRE(Cin >= 1 && Cin <= 4 && B >= 1 && n_entries >= B && n_entries % B == 0);
    Geo g;
    MIVP_REQUIRE(fill_geo(g, dims, pad, pdims, roi));
    const int vec_ok = (reinterpret_cast<uintptr_t>(vol) % 16 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0) &&
                       g.n[2] % 4 == 0 && g.r[2] % 4 == 0;
    const long total = (long)B * Cin * g.r[0] * g.r[1] * ((g.r[2] + 3) / 4);
    hipLaunchKernelGGL(kern, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, vol, (int)Cin, g,
                       table, (int)n_entries, sub_idx, (int)B, vec_ok, out);
    return mivp_check_launch(what);
}

// the argument checks of the two finalize entry points, and their (grid, Geo)
int finalize_setup(const float* acc, const float* wsum, int32_t C, const int32_t* dims, const int32_t* pad,
                    const int32_t* pdims, const uint8_t* labels, const float* target, const void* counts, Geo& g,
                    unsigned& grid) {
    MIVP_REQUIRE(acc && wsum && labels && dims && pad && pdims && C >= 1 && C <= MAXC);
    MIVP_REQUIRE((target == nullptr) == (counts == nullptr));
    const int32_t one[3] = {1, 1, 1};
    MIVP_REQUIRE(fill_geo(g, dims, pad, pdims, one));
    const long nvox = (long)g.n[0] * g.n[1] * g.n[2];
    grid = (unsigned)((nvox + TPB - 1) / TPB > 2048 ? 2048 : (nvox + TPB - 1) / TPB);
    return MIVP_OK;
}
}  // namespace

extern "C" int mivp_window_gather(const float* vol, int32_t Cin, const int32_t* dims, const int32_t* pad, const int32_t* pdims,
                                  const int32_t* roi, const int32_t* table, int32_t n_entries, const int32_t* sub_idx,
                                  int32_t B, float* out, mivp_stream_t stream) {
    return launch_gather(k_window_gather, "window_gather", vol, Cin, dims, pad, pdims, roi, table, n_entries, sub_idx, B, out,
                         stream);
}

extern "C" int mivp_window_blend(const float* logits, int32_t channels_last, int32_t C, const int32_t* pdims,
                                 const int32_t* roi, const int32_t* table, int32_t n_entries, const int32_t* sub_idx,
                                 int32_t B, const int32_t* ubox, const float* w0, const float* w1, const float* w2,
                                 float w_floor, float* acc, float* wsum, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && table && sub_idx && pdims && roi && ubox && w0 && w1 && w2 && acc && wsum);
    MIVP_REQUIRE(C >= 1 && C <= MAXC && B >= 1 && n_entries >= B && n_entries % B == 0);
    const int32_t zero[3] = {0, 0, 0};
    Geo g;
    MIVP_REQUIRE(fill_geo(g, pdims, zero, pdims, roi));
    for (int a = 0; a < 3; ++a) MIVP_REQUIRE(ubox[a] >= g.r[a] && ubox[a] <= g.p[a]);
    const long total = (long)ubox[0] * ubox[1] * ubox[2];
    hipLaunchKernelGGL(k_window_blend, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, logits,
                       (int)(channels_last != 0), (int)C, g, table, (int)n_entries, sub_idx, (int)B, (int)ubox[0],
                       (int)ubox[1], (int)ubox[2], w0, w1, w2, w_floor, acc, wsum);
    return mivp_check_launch("window_blend");
}

extern "C" int mivp_stitch_finalize(const float* acc, const float* wsum, int32_t C, const int32_t* dims, const int32_t* pad,
                                    const int32_t* pdims, uint8_t* labels, float* logits, const float* target, void* counts,
                                    mivp_stream_t stream) {
    Geo g;
    unsigned grid;
    if (const int e = finalize_setup(acc, wsum, C, dims, pad, pdims, labels, target, counts, g, grid)) return e;
    hipLaunchKernelGGL(k_stitch_finalize, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, acc, wsum, (int)C, g, labels, logits,
                       target, (unsigned long long*)counts);
    return mivp_check_launch("stitch_finalize");
}

extern "C" int mivp_window_gather_tta(const float* vol, int32_t Cin, const int32_t* dims, const int32_t* pad,
                                      const int32_t* pdims, const int32_t* roi, const int32_t* table, int32_t n_entries,
                                      const int32_t* sub_idx, int32_t B, float* out, mivp_stream_t stream) {
    return launch_gather(k_window_gather_tta, "window_gather_tta", vol, Cin, dims, pad, pdims, roi, table, n_entries, sub_idx,
                         B, out, stream);
}

extern "C" int mivp_window_blend_tta(const float* logits, int32_t channels_last, int32_t C, const int32_t* pdims,
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
    const long total = (long)ubox[0] * ubox[1] * ubox[2];
    const auto kern = comp ? k_window_blend_tta<true> : k_window_blend_tta<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, logits,
                       (int)(channels_last != 0), (int)C, g, table, (int)n_entries, sub_idx, (int)B, (int)ubox[0],
                       (int)ubox[1], (int)ubox[2], w0, w1, w2, w_floor, acc, wsum, comp);
    return mivp_check_launch("window_blend_tta");
}

extern "C" int mivp_stitch_finalize_probs(const float* acc, const float* wsum, int32_t C, const int32_t* dims,
                                          const int32_t* pad, const int32_t* pdims, uint8_t* labels, float* logits,
                                          float* probs, float* confidence, float* entropy, const float* target, void* counts,
                                          mivp_stream_t stream) {
    Geo g;
    unsigned grid;
    if (const int e = finalize_setup(acc, wsum, C, dims, pad, pdims, labels, target, counts, g, grid)) return e;
    hipLaunchKernelGGL(k_stitch_finalize_probs, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, acc, wsum, (int)C, g, labels,
                       logits, probs, confidence, entropy, target, (unsigned long long*)counts);
    return mivp_check_launch("stitch_finalize_probs");
}

extern "C" int mivp_window_advance(int32_t* sub_idx, mivp_stream_t stream) {
    MIVP_REQUIRE(sub_idx);
    hipLaunchKernelGGL(k_window_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (int*)sub_idx);
    return mivp_check_launch("window_advance");
}
