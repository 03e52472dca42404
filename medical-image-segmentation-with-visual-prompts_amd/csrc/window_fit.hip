// Fitting the prediction windows to the foreground bounding box (additive to ABI 18; mivp_amd/inference.py WindowFit,
// DESIGN 4.25).  Two launches in front of the sub-batch loop of csrc/stitch.hip:
//   foreground_box : inclusive bounding box of the foreground (fp32 volume channel > threshold, or uint8 mask != 0) in
//                    image coordinates, six integer atomicMin / atomicMax per workgroup that saw foreground
//   window_fit_plan: the window tiling of that box (the placement rule of window_origins on the box, widened to the roi
//                    and clamped into the padded volume) written as the work list the gather / blend / recorded graph read
// Integers only: every result is independent of the order of the atomics and bitwise reproducible.
// The plan's geometry arguments pass the check of the other window kernels (fill_geo of csrc/window_common.hpp).
#include "window_common.hpp"

namespace {
constexpr int WAVES = TPB / 64;
constexpr int MAXF = 8;                                        // flip codes of one window (3-bit masks)

struct Dims { int n[3]; };
struct FlipCodes { int m[MAXF]; };

struct FitGeo {
    int pad[3];        // zeros in front of the image (padded volume coordinates = image coordinates + pad)
    int p[3];          // padded size, max(n, roi)
    int r[3];          // roi
    int step[3];       // max(int(r * (1 - overlap)), 1), computed by the host
    int margin[3];     // voxels added around the box
};

// bit e set = voxel e of the quad is foreground
MIVP_DEV unsigned fgbit(float v, float thr) { return v > thr ? 1u : 0u; }                  // strict: NaN is not foreground
MIVP_DEV unsigned fgbit(uint8_t v, float) { return v != 0 ? 1u : 0u; }
MIVP_DEV unsigned fgbits4(const float* p, float thr) {                                    // one 16-byte load
    const float4 v = *reinterpret_cast<const float4*>(p);
    return fgbit(v.x, thr) | fgbit(v.y, thr) << 1 | fgbit(v.z, thr) << 2 | fgbit(v.w, thr) << 3;
}
MIVP_DEV unsigned fgbits4(const uint8_t* p, float) {                                      // one 4-byte load
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    return ((v & 0xFFu) != 0) | ((v & 0xFF00u) != 0) << 1 | ((v & 0xFF0000u) != 0) << 2 | ((v & 0xFF000000u) != 0) << 3;
}

// the empty encoding: lo = dims, hi = -1 (any atomicMin / atomicMax of a foreground voxel replaces it)
__global__ void k_box_init(Dims g, int* __restrict__ box) {
    if (threadIdx.x < 3) box[threadIdx.x] = g.n[threadIdx.x];
    else if (threadIdx.x < 6) box[threadIdx.x] = -1;
}

// src: the channel's [H][W][D] block.  An item is four consecutive D voxels of one (h, w) row; the items are walked with a
// grid stride, so consecutive lanes read consecutive quads.  vec_ok: D % 4 == 0 and an aligned base, so every quad is an
// aligned load inside its row; otherwise the quad is read voxel by voxel and stops at the end of the row.
template <typename T>
__global__ __launch_bounds__(TPB) void k_foreground_box(const T* __restrict__ src, float thr, Dims g, int vec_ok,
                                                        int* __restrict__ box) {
    __shared__ int s_lo[3][WAVES], s_hi[3][WAVES];
    const int dq = (g.n[2] + 3) >> 2;
    const long items = (long)g.n[0] * g.n[1] * dq;
    int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = -1, hi1 = -1, hi2 = -1;
    for (long it = (long)blockIdx.x * TPB + threadIdx.x; it < items; it += (long)gridDim.x * TPB) {
        const int row = (int)(it / dq);
        const int d0 = 4 * (int)(it - (long)row * dq);
        const T* rp = src + (long)row * g.n[2];
        unsigned m = 0;
        if (vec_ok) {
            m = fgbits4(rp + d0, thr);
        } else {
            const int kn = min(4, g.n[2] - d0);
            for (int e = 0; e < kn; ++e) m |= fgbit(rp[d0 + e], thr) << e;
        }
        if (!m) continue;
        const int h = row / g.n[1], w = row - h * g.n[1];
        lo0 = min(lo0, h); hi0 = max(hi0, h);
        lo1 = min(lo1, w); hi1 = max(hi1, w);
        lo2 = min(lo2, d0 + __ffs((int)m) - 1);
        hi2 = max(hi2, d0 + 31 - __clz((int)m));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo0 = min(lo0, __shfl_down(lo0, off)); lo1 = min(lo1, __shfl_down(lo1, off)); lo2 = min(lo2, __shfl_down(lo2, off));
        hi0 = max(hi0, __shfl_down(hi0, off)); hi1 = max(hi1, __shfl_down(hi1, off)); hi2 = max(hi2, __shfl_down(hi2, off));
    }
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        s_lo[0][wv] = lo0; s_lo[1][wv] = lo1; s_lo[2][wv] = lo2;
        s_hi[0][wv] = hi0; s_hi[1][wv] = hi1; s_hi[2][wv] = hi2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {                                     // thread a: axis a
        int lo = INT_MAX, hi = -1;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) { lo = min(lo, s_lo[threadIdx.x][k]); hi = max(hi, s_hi[threadIdx.x][k]); }
        if (hi >= 0) {                                         // this workgroup saw foreground (then on every axis)
            atomicMin(&box[threadIdx.x], lo);
            atomicMax(&box[3 + threadIdx.x], hi);
        }
    }
}

// One workgroup.  Every thread derives the three (start, length, count) from the box, then the threads share the rows
// of the table: entry e = window e / F under codes[e % F], windows row-major over the three counts; rows past the plan
// are zero (invalid).  Nothing is written past `capacity` rows / `origin_capacity` origins whatever the box holds; a plan
// that does not fit (it cannot: a count never exceeds the full tiling's) writes meta = (-1, -1) and an all-zero table.
__global__ __launch_bounds__(TPB) void k_window_fit_plan(const int* __restrict__ box, Dims g, FitGeo f, FlipCodes codes,
                                                         int F, int4* __restrict__ table, int capacity,
                                                         int* __restrict__ origins, int origin_capacity,
                                                         int* __restrict__ meta) {
    int b0[3], len[3], cnt[3];
    bool empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int lo = box[a], hi = box[3 + a];
        empty = empty || hi < lo || lo < 0 || hi >= g.n[a];    // (a box outside the image is no box)
        const int l = min(max(lo, 0), g.n[a] - 1), h = min(max(hi, 0), g.n[a] - 1);
        int s = max(l + f.pad[a] - f.margin[a], 0);
        const int e = min(h + f.pad[a] + f.margin[a] + 1, f.p[a]);
        int n = e - s;
        if (n < f.r[a]) {                                      // widen to the roi, centred, inside the padded volume
            s = min(max(s - (f.r[a] - n) / 2, 0), f.p[a] - f.r[a]);
            n = f.r[a];
        }
        b0[a] = s; len[a] = n;
        cnt[a] = (n - f.r[a] + f.step[a] - 1) / f.step[a] + 1;
    }
    long windows = empty ? 0 : (long)cnt[0] * cnt[1] * cnt[2];
    long entries = windows * F;
    const bool fits = entries <= capacity && windows <= origin_capacity;
    if (!fits) windows = entries = 0;
    const int c12 = cnt[1] * cnt[2];
    for (int e = threadIdx.x; e < capacity; e += TPB) {
        int4 row = make_int4(0, 0, 0, 0);
        if (e < entries) {
            const int w = e / F, j = e - w * F;
            const int i0 = w / c12, rem = w - i0 * c12, i1 = rem / cnt[2], i2 = rem - i1 * cnt[2];
            row.x = b0[0] + min(i0 * f.step[0], len[0] - f.r[0]);
            row.y = b0[1] + min(i1 * f.step[1], len[1] - f.r[1]);
            row.z = b0[2] + min(i2 * f.step[2], len[2] - f.r[2]);
            row.w = 1 | codes.m[j] << 1;
            if (j == 0) { origins[3 * w + 0] = row.x; origins[3 * w + 1] = row.y; origins[3 * w + 2] = row.z; }
        }
        table[e] = row;
    }
    for (long w = windows + threadIdx.x; w < origin_capacity; w += TPB) {
        origins[3 * w + 0] = 0; origins[3 * w + 1] = 0; origins[3 * w + 2] = 0;
    }
    if (threadIdx.x == 0) { meta[0] = fits ? (int)windows : -1; meta[1] = fits ? (int)entries : -1; }
}
}  // namespace

extern "C" int mivp_foreground_box(const float* vol, int32_t Cin, int32_t channel, float threshold, const uint8_t* mask,
                                   const int32_t* dims, int32_t* box, mivp_stream_t stream) {
    MIVP_REQUIRE(dims && box);
    MIVP_REQUIRE((vol != nullptr) != (mask != nullptr));
    if (vol) MIVP_REQUIRE(Cin >= 1 && channel >= 0 && channel < Cin);
    Dims g;
    for (int a = 0; a < 3; ++a) { g.n[a] = dims[a]; MIVP_REQUIRE(g.n[a] >= 1); }
    const long nvox = (long)g.n[0] * g.n[1] * g.n[2];
    MIVP_REQUIRE(nvox < (1L << 31));
    hipLaunchKernelGGL(k_box_init, dim3(1), dim3(64), 0, (hipStream_t)stream, g, (int*)box);
    const long items = (long)g.n[0] * g.n[1] * ((g.n[2] + 3) / 4);
    const long want = (items + 4 * TPB - 1) / (4 * TPB);       // ~4 quads per thread, at most 8 workgroups per CU
    const unsigned grid = (unsigned)(want > 2048 ? 2048 : want);
    if (vol) {
        const float* src = vol + (long)channel * nvox;
        const int vec_ok = reinterpret_cast<uintptr_t>(vol) % 16 == 0 && g.n[2] % 4 == 0;
        hipLaunchKernelGGL(k_foreground_box<float>, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, src, threshold, g, vec_ok,
                           (int*)box);
    } else {
        const int vec_ok = reinterpret_cast<uintptr_t>(mask) % 4 == 0 && g.n[2] % 4 == 0;
        hipLaunchKernelGGL(k_foreground_box<uint8_t>, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, mask, 0.f, g, vec_ok,
                           (int*)box);
    }
    return mivp_check_launch("foreground_box");
}

extern "C" int mivp_window_fit_plan(const int32_t* box, const int32_t* dims, const int32_t* pad, const int32_t* pdims,
                                    const int32_t* roi, const int32_t* interval, const int32_t* margin,
                                    const int32_t* codes, int32_t n_flips, int32_t* table, int32_t n_entries,
                                    int32_t* origins, int32_t n_origins, int32_t* meta, mivp_stream_t stream) {
    MIVP_REQUIRE(box && dims && pad && pdims && roi && interval && margin && codes && table && origins && meta);
    MIVP_REQUIRE(n_flips >= 1 && n_flips <= MAXF && n_entries >= 1 && n_origins >= 1);
    MIVP_REQUIRE(n_entries <= (1 << 27) && n_origins <= (1 << 27));
    MIVP_REQUIRE(reinterpret_cast<uintptr_t>(table) % 16 == 0);
    Geo geo;
    MIVP_REQUIRE(fill_geo(geo, dims, pad, pdims, roi));
    Dims g;
    FitGeo f;
    for (int a = 0; a < 3; ++a) {
        g.n[a] = geo.n[a]; f.pad[a] = geo.pad[a]; f.p[a] = geo.p[a]; f.r[a] = geo.r[a]; f.step[a] = interval[a];
        f.margin[a] = margin[a];
        MIVP_REQUIRE(f.step[a] >= 1 && f.step[a] <= f.r[a] && f.margin[a] >= 0 && f.margin[a] <= (1 << 30));
    }
    FlipCodes c;
    for (int j = 0; j < MAXF; ++j) {
        c.m[j] = j < n_flips ? codes[j] : 0;
        MIVP_REQUIRE(c.m[j] >= 0 && c.m[j] <= 7);
    }
    hipLaunchKernelGGL(k_window_fit_plan, dim3(1), dim3(TPB), 0, (hipStream_t)stream, box, g, f, c, (int)n_flips,
                       reinterpret_cast<int4*>(table), (int)n_entries, (int*)origins, (int)n_origins, (int*)meta);
    return mivp_check_launch("window_fit_plan");
}
