// Scan statistics and data-driven intensity windows (joined ABI 18, mivp_amd/scanstats.py).
//
// k_scan_hist: the exact histogram of an integer scan raw [C][H][W][D] (int16 or uint8), one bin per value: bin = v + 32768
// for both dtypes, hist int64 [C][65536], ADDED to (the caller zeroes it, or pools scans in it).  Nothing depends on a
// voxel's coordinates, so a channel is walked flat, as calibration.hip walks its volume: the elements before the first
// 16-byte boundary of the channel's plane and those after the last whole vector are read one by one by workgroup 0, the
// rest as 16-byte vectors (8 int16 / 16 uint8 values per lane and trip, grid-strided so a wave reads 1 KiB contiguous).
//   select    per voxel: the uint8 mask [H][W][D] (shared by the channels; read as one vector where mask + index is
//             aligned, else byte by byte) is non-zero, and / or v > above.
//   count     a workgroup keeps WIN = 16384 32-bit counters in LDS (64 KiB: two workgroups per CU) for the bins
//             [wbin, wbin + WIN); a value outside that window adds to the global table directly.  Either way the result is
//             the same integers; the window only decides the speed.  Its base is a launch argument (`base`, the lowest
//             value inside): real scans sit in a few thousand consecutive values, so one fixed choice per modality covers
//             them (mivp_amd/scanstats.py has the defaults), and a pre-pass for the minimum would read the scan twice.
//             A workgroup counts fewer than 2^31 voxels, so a counter cannot wrap.
//   runs      half of a CT is air at one value and an MR background is exactly 0: 64 lanes adding to one LDS address
//             serialise.  By default a lane merges the equal consecutive selected values of its vector and adds once per
//             run; flags bit 0 adds per value instead (tools/bench_scanstats.py times both).
//   merge     one 64-bit global atomic add per (workgroup, non-empty counter).  Integer atomics only: the table is exact,
//             bitwise reproducible and independent of the launch shape.
//
// k_scan_window_plan: one workgroup per channel turns hist[c] into the slot float32 [C][8] that mivp_scan_prepare_dev
// reads: thread t sums its 256 consecutive bins (count, S1 = sum v n_v, S2 = sum v^2 n_v in int64), thread 0 forms the
// prefix of the 256 counts, N and the two ranks k = max(1, ceil(q * double(N))), the thread whose bins hold a rank walks
// them again for the k-th smallest value, and thread 0 writes the plan in float64, rounded to float32 once.  Floating-point
// contraction is off in this file: the plan's operations are the ones written, each rounded on its own, as numpy does.
#include "common.hpp"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256;
constexpr int NBINS = 65536;
constexpr int OFFSET = 32768;             // bin of value 0
constexpr int WIN = 16384;                // LDS counters per workgroup (64 KiB)
constexpr long WG_ITEMS = 1024;           // vectors per workgroup before the grid grows
constexpr long GRID_CAP = 512;            // workgroups per channel at most: two per CU
constexpr int CHUNK = NBINS / TPB;        // bins per thread of the plan kernel
typedef unsigned long long u64;

struct Select { const uint8_t* mask; int use_above, above; };

MIVP_DEV void add(unsigned* cnt, u64* g, int wbin, int v, unsigned n) {
    const int bin = v + OFFSET;
    const unsigned i = (unsigned)(bin - wbin);
    if (i < (unsigned)WIN) atomicAdd(cnt + i, n);
    else atomicAdd(g + bin, (u64)n);
}

template <typename T> MIVP_DEV int unpack(const u32x4& w, int j);
template <> MIVP_DEV int unpack<int16_t>(const u32x4& w, int j) { return (int)(int16_t)(w[j >> 1] >> (16 * (j & 1))); }
template <> MIVP_DEV int unpack<uint8_t>(const u32x4& w, int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu); }

// bit j: the mask byte of value j of the vector at element e is non-zero
template <int N>
MIVP_DEV unsigned mask_bits(const uint8_t* __restrict__ m, bool vec) {
    unsigned bits = 0u;
    if (vec) {
        unsigned w[N / 4];
        if (N == 8) {
            const u32x2 t = *reinterpret_cast<const u32x2*>(m);
            w[0] = t[0]; w[1] = t[1];
        } else {
            const u32x4 t = *reinterpret_cast<const u32x4*>(m);
#pragma unroll
            for (int i = 0; i < N / 4; ++i) w[i] = t[i];
        }
#pragma unroll
        for (int j = 0; j < N; ++j) bits |= (((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) ? 1u : 0u) << j;
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) bits |= (m[j] ? 1u : 0u) << j;
    }
    return bits;
}

template <typename T, bool MERGE>
__global__ __launch_bounds__(TPB) void k_scan_hist(const T* __restrict__ raw, long V, Select sel, int wbin,
                                                   u64* __restrict__ hist) {
    __shared__ unsigned cnt[WIN];
    constexpr int N = 16 / (int)sizeof(T);
    const int tid = (int)threadIdx.x, c = (int)blockIdx.y;
    for (int i = tid; i < WIN; i += TPB) cnt[i] = 0u;
    __syncthreads();
    const T* __restrict__ x = raw + (long)c * V;
    u64* __restrict__ g = hist + (long)c * NBINS;
    // elements before the plane's first 16-byte boundary, whole vectors, elements after them
    const long head = min(V, (long)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) / sizeof(T)));
    const long items = (V - head) / N;
    const long tail0 = head + items * N;
    const bool mvec = sel.mask && (((uintptr_t)(sel.mask + head) & (uintptr_t)(N - 1)) == 0);

    for (long it = (long)blockIdx.x * TPB + tid; it < items; it += (long)gridDim.x * TPB) {
        const long e = head + it * N;
        const u32x4 w = *reinterpret_cast<const u32x4*>(x + e);
        unsigned keep = (1u << N) - 1u;
        if (sel.mask) keep = mask_bits<N>(sel.mask + e, mvec);
        int v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            v[j] = unpack<T>(w, j);
            if (sel.use_above && !(v[j] > sel.above)) keep &= ~(1u << j);
        }
        if (MERGE) {
            int rv = 0;
            unsigned rn = 0u;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (!((keep >> j) & 1u)) continue;
                if (rn && v[j] == rv) { ++rn; continue; }
                if (rn) add(cnt, g, wbin, rv, rn);
                rv = v[j];
                rn = 1u;
            }
            if (rn) add(cnt, g, wbin, rv, rn);
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j)
                if ((keep >> j) & 1u) add(cnt, g, wbin, v[j], 1u);
        }
    }
    if (blockIdx.x == 0) {
        const long loose = head + (V - tail0);
        for (long i = tid; i < loose; i += TPB) {
            const long e = i < head ? i : tail0 + (i - head);
            const int v = (int)x[e];
            if ((!sel.mask || sel.mask[e]) && (!sel.use_above || v > sel.above)) add(cnt, g, wbin, v, 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < WIN; i += TPB) {
        const unsigned n = cnt[i];
        if (n) atomicAdd(g + wbin + i, (u64)n);
    }
}

enum { PLAN_PERCENTILE = 0, PLAN_ZSCORE = 1 };

__global__ __launch_bounds__(TPB) void k_scan_window_plan(const u64* __restrict__ hist, int mode, double q_lo, double q_hi,
                                                          double b_min, double b_max, int clip, float* __restrict__ slot) {
    __shared__ u64 pre[TPB + 1];               // counts per thread, then their exclusive prefix
    __shared__ long long s1s[TPB], s2s[TPB];
    __shared__ u64 rank[2];
    __shared__ int val[2];
    __shared__ long long tot[2];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS + (long)tid * CHUNK;
    u64 n = 0ull;
    long long s1 = 0, s2 = 0;
    for (int i = 0; i < CHUNK; ++i) {
        const u64 k = h[i];
        const long long v = (long long)(tid * CHUNK + i - OFFSET);
        n += k;
        s1 += v * (long long)k;
        s2 += v * v * (long long)k;
    }
    pre[tid + 1] = n;
    s1s[tid] = s1;
    s2s[tid] = s2;
    __syncthreads();
    if (tid == 0) {
        u64 run = 0ull;
        long long a = 0, b = 0;
        pre[0] = 0ull;
        for (int t = 0; t < TPB; ++t) {
            run += pre[t + 1];
            pre[t + 1] = run;
            a += s1s[t];
            b += s2s[t];
        }
        tot[0] = a;
        tot[1] = b;
        const double dn = (double)run;
        const double klo = ceil(q_lo * dn), khi = ceil(q_hi * dn);
        rank[0] = klo < 1.0 ? 1ull : (u64)klo;
        rank[1] = khi < 1.0 ? 1ull : (u64)khi;
        val[0] = val[1] = 0;                    // an empty histogram finds no rank
    }
    __syncthreads();
    const u64 below = pre[tid], upto = pre[tid + 1];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const u64 k = rank[r];
        if (k > below && k <= upto) {           // one thread per rank: the prefix is non-decreasing
            u64 cum = below;
            for (int i = 0; i < CHUNK; ++i) {
                cum += h[i];
                if (cum >= k) { val[r] = tid * CHUNK + i - OFFSET; break; }
            }
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const u64 N = pre[TPB];
    const double a_lo = (double)val[0], a_hi = (double)val[1];
    double mean = 0.0, sd = 0.0;
    if (N) {
        const double dn = (double)N;
        mean = (double)tot[0] / dn;
        sd = sqrt(fmax(0.0, (double)tot[1] / dn - mean * mean));
    }
    float* w = slot + 8 * c;
    if (mode == PLAN_PERCENTILE) {
        double s = 0.0, t = b_min;              // a constant scan or an empty selection
        if (a_hi != a_lo) {
            s = (b_max - b_min) / (a_hi - a_lo);
            t = b_min - a_lo * s;
        }
        w[0] = (float)s; w[1] = (float)t; w[2] = (float)b_min; w[3] = (float)b_max;
    } else {
        double s = 1.0, t = -mean;
        if (N && sd != 0.0) {
            s = 1.0 / sd;
            t = -mean / sd;
        }
        const float sf = (float)s, tf = (float)t;
        w[0] = sf; w[1] = tf;
        w[2] = clip ? fmaf((float)a_lo, sf, tf) : -FLT_MAX;
        w[3] = clip ? fmaf((float)a_hi, sf, tf) : FLT_MAX;
    }
    w[4] = (float)a_lo; w[5] = (float)a_hi; w[6] = (float)mean; w[7] = (float)sd;
}

template <typename T>
void launch_hist(bool merge, dim3 grid, hipStream_t st, const void* raw, long V, const Select& sel, int wbin, u64* hist) {
    if (merge)
        hipLaunchKernelGGL((k_scan_hist<T, true>), grid, dim3(TPB), 0, st, static_cast<const T*>(raw), V, sel, wbin, hist);
    else
        hipLaunchKernelGGL((k_scan_hist<T, false>), grid, dim3(TPB), 0, st, static_cast<const T*>(raw), V, sel, wbin, hist);
}
}  // namespace

extern "C" int mivp_scan_hist(const void* raw, int32_t dtype, int32_t C, const int32_t* dims, const uint8_t* mask,
                              int32_t use_above, int32_t above, int32_t base, int32_t flags, int64_t* hist,
                              mivp_stream_t stream) {
    MIVP_REQUIRE(raw && dims && hist && (dtype == 0 || dtype == 4) && C >= 1 && C <= 4 && (flags & ~1) == 0);
    MIVP_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long)dims[0] * dims[1] * dims[2] < (1L << 31));
    MIVP_REQUIRE(((uintptr_t)hist & 7u) == 0 && (dtype == 0 || ((uintptr_t)raw & 1u) == 0));
    const long V = (long)dims[0] * dims[1] * dims[2];
    const int n = dtype == 0 ? 16 : 8;
    long wbin = (long)base + OFFSET;                              // any base is valid: the window is moved into the table
    wbin = wbin < 0 ? 0 : (wbin > NBINS - WIN ? NBINS - WIN : wbin);
    const long want = (V / n + WG_ITEMS - 1) / WG_ITEMS;
    const dim3 grid((unsigned)(want < 1 ? 1 : (want > GRID_CAP ? GRID_CAP : want)), (unsigned)C);
    const Select sel = {mask, use_above != 0, (int)above};
    if (dtype == 0) launch_hist<uint8_t>(!(flags & 1), grid, (hipStream_t)stream, raw, V, sel, (int)wbin, (u64*)hist);
    else launch_hist<int16_t>(!(flags & 1), grid, (hipStream_t)stream, raw, V, sel, (int)wbin, (u64*)hist);
    return mivp_check_launch("scan_hist");
}

extern "C" int mivp_scan_window_plan(const int64_t* hist, int32_t C, int32_t mode, double q_lo, double q_hi, double b_min,
                                     double b_max, int32_t clip, float* slot, mivp_stream_t stream) {
    MIVP_REQUIRE(hist && slot && C >= 1 && C <= 4 && (mode == PLAN_PERCENTILE || mode == PLAN_ZSCORE));
    MIVP_REQUIRE(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0);                    // (false for a NaN)
    MIVP_REQUIRE(mode == PLAN_ZSCORE || (isfinite(b_min) && isfinite(b_max) && b_min <= b_max));
    MIVP_REQUIRE(((uintptr_t)hist & 7u) == 0 && ((uintptr_t)slot & 3u) == 0);
    hipLaunchKernelGGL(k_scan_window_plan, dim3((unsigned)C), dim3(TPB), 0, (hipStream_t)stream, (const u64*)hist, (int)mode,
                       q_lo, q_hi, b_min, b_max, (int)(clip != 0), slot);
    return mivp_check_launch("scan_window_plan");
}
