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
// With an Otsu record (below) whose valid word is set, the bins at or below its threshold read as zero, for N, S1, S2 and
// both ranks alike: the plan of the voxels above the threshold with no second pass over them.
//
// k_scan_otsu_plan: one workgroup per channel finds Otsu's threshold of hist[c] in integers.  With N = sum n_v
// and S = sum v n_v, a candidate t is a counted value that is not the largest one; n0 = sum_{v<=t} n_v, A = sum_{v<=t} v n_v,
// P = A N - S n0, q = n0 (N - n0).  The between-class variance is P^2 / (N^2 q), so the threshold maximises P^2 / q: two
// candidates compare by P_a^2 q_b against P_b^2 q_a, equal values pick the lower t.  For N < 2^33: |P| < 2^83 (__int128),
// P^2 < 2^166 (three 64-bit limbs), q < 2^64, the products below 2^230 (four limbs, __int128 partial products).  No
// floating-point operation takes part, and the comparator is a total order, so any reduction tree gives the same answer.
// Pass 1 is the window plan's (on 1024 threads of 64 bins): per-thread count and first moment, prefixed by thread 0.
// Pass 2: a thread walks its bins with running n0 and A and keeps its best candidate; a tree over the threads keeps the
// workgroup's.  The record int64 [C][4] = (t, n_le, n_gt, valid); fewer than two distinct counted values, N = 0 or
// N >= 2^33: valid = 0, t = the largest counted value (0 if none), n_le = N, n_gt = 0.
//
// k_scan_threshold_mask: out[e] = raw[channel][e] > t as uint8 on the native grid (all ones when the record is not valid),
// t read from the device record: 16-byte loads, packed byte stores, the head / tail split of k_scan_hist.
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

enum { REC_T = 0, REC_N_LE = 1, REC_N_GT = 2, REC_VALID = 3, REC_WORDS = 4 };   // the Otsu record of a channel

__global__ __launch_bounds__(TPB) void k_scan_window_plan(const u64* __restrict__ hist, int mode, double q_lo, double q_hi,
                                                          double b_min, double b_max, int clip,
                                                          const long long* __restrict__ otsu, float* __restrict__ slot) {
    __shared__ u64 pre[TPB + 1];               // counts per thread, then their exclusive prefix
    __shared__ long long s1s[TPB], s2s[TPB];
    __shared__ u64 rank[2];
    __shared__ int val[2];
    __shared__ long long tot[2];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS + (long)tid * CHUNK;
    // bins below `first` read as zero: the values at or below a valid Otsu threshold
    int first = 0;
    if (otsu && otsu[REC_WORDS * c + REC_VALID]) first = (int)otsu[REC_WORDS * c + REC_T] + OFFSET + 1 - tid * CHUNK;
    u64 n = 0ull;
    long long s1 = 0, s2 = 0;
    for (int i = 0; i < CHUNK; ++i) {
        const u64 k = i < first ? 0ull : h[i];
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
                cum += i < first ? 0ull : h[i];
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

// ---- Otsu's threshold in integers ------------------------------------------------------------------------------------
typedef unsigned __int128 u128;

struct Cand { u64 p[3]; u64 q, n0; int t; };     // P^2 in three limbs; q == 0: no candidate

MIVP_DEV void square83(__int128 P, u64* p) {      // |P| < 2^83 -> P^2 < 2^166
    const u128 u = P < 0 ? (u128)(-P) : (u128)P;
    const u64 lo = (u64)u, hi = (u64)(u >> 64);
    const u128 a = (u128)lo * lo;
    p[0] = (u64)a;
    u128 cy = (a >> 64) + 2 * ((u128)hi * lo);    // hi < 2^19: below 2^85
    p[1] = (u64)cy;
    cy = (cy >> 64) + (u128)hi * hi;
    p[2] = (u64)cy;
}

MIVP_DEV void mul3x1(const u64* p, u64 q, u64* o) {
    u128 cy = (u128)p[0] * q;
    o[0] = (u64)cy;
    cy = (cy >> 64) + (u128)p[1] * q;
    o[1] = (u64)cy;
    cy = (cy >> 64) + (u128)p[2] * q;
    o[2] = (u64)cy;
    o[3] = (u64)(cy >> 64);
}

// a total order on candidates: a comes first when P_a^2 / q_a is larger, or equal with the lower t
MIVP_DEV bool better(const Cand& a, const Cand& b) {
    if (!a.q) return false;
    if (!b.q) return true;
    u64 l[4], r[4];
    mul3x1(a.p, b.q, l);
    mul3x1(b.p, a.q, r);
#pragma unroll
    for (int i = 3; i >= 0; --i)
        if (l[i] != r[i]) return l[i] > r[i];
    return a.t < b.t;
}

// 1024 threads of 64 bins: a scan sits in a few thousand consecutive values, and only the threads whose bins are occupied
// have candidates to weigh (about 12 wide multiplies each).  With the window plan's 256 x 256 split 16 threads did all of
// it (0.25 ms on the 4096-value benchmark scan); the finer split spreads it over 64.
constexpr int OTSU_TPB = 1024;
constexpr int OTSU_CHUNK = NBINS / OTSU_TPB;

__global__ __launch_bounds__(OTSU_TPB) void k_scan_otsu_plan(const u64* __restrict__ hist, long long* __restrict__ otsu) {
    __shared__ u64 pre[OTSU_TPB + 1];               // counts per thread, then their exclusive prefix
    __shared__ long long s1s[OTSU_TPB + 1];         // first moments per thread, then their exclusive prefix
    __shared__ int top[OTSU_TPB];                   // the highest occupied bin of a thread, -1 if none
    __shared__ Cand best[OTSU_TPB / 2];             // (the upper half of the threads hands its candidates to the lower)
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS + (long)tid * OTSU_CHUNK;
    u64 n = 0ull;
    long long s1 = 0;
    int hi = -1;
    for (int i = 0; i < OTSU_CHUNK; ++i) {
        const u64 k = h[i];
        n += k;
        s1 += (long long)(tid * OTSU_CHUNK + i - OFFSET) * (long long)k;
        if (k) hi = tid * OTSU_CHUNK + i;
    }
    pre[tid + 1] = n;
    s1s[tid + 1] = s1;
    top[tid] = hi;
    __syncthreads();
    if (tid == 0) {
        u64 run = 0ull;
        long long a = 0;
        int m = -1;
        pre[0] = 0ull;
        s1s[0] = 0;
        for (int t = 0; t < OTSU_TPB; ++t) {
            run += pre[t + 1];
            pre[t + 1] = run;
            a += s1s[t + 1];
            s1s[t + 1] = a;
            m = max(m, top[t]);
        }
        top[0] = m;
    }
    __syncthreads();
    const u64 N = pre[OTSU_TPB];
    const long long S = s1s[OTSU_TPB];
    const bool exact = N < (1ull << 33);       // beyond it P and the products outgrow their limbs: no threshold
    Cand mine;
    mine.p[0] = mine.p[1] = mine.p[2] = 0ull;
    mine.q = mine.n0 = 0ull;
    mine.t = 0;
    if (exact && n) {
        u64 n0 = pre[tid];
        long long A = s1s[tid];
        for (int i = 0; i < OTSU_CHUNK; ++i) {
            const u64 k = h[i];
            if (!k) continue;
            const int v = tid * OTSU_CHUNK + i - OFFSET;
            n0 += k;
            A += (long long)v * (long long)k;
            if (n0 == N) break;                // the largest counted value is no candidate
            Cand x;
            square83((__int128)A * (__int128)N - (__int128)S * (__int128)n0, x.p);
            x.q = n0 * (N - n0);
            x.n0 = n0;
            x.t = v;
            if (better(x, mine)) mine = x;
        }
    }
    if (tid >= OTSU_TPB / 2) best[tid - OTSU_TPB / 2] = mine;
    __syncthreads();
    if (tid < OTSU_TPB / 2 && !better(best[tid], mine)) best[tid] = mine;
    __syncthreads();
    for (int s = OTSU_TPB / 4; s > 0; s >>= 1) {
        if (tid < s && better(best[tid + s], best[tid])) best[tid] = best[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    long long* w = otsu + REC_WORDS * c;
    const Cand& b = best[0];
    if (b.q) {
        w[REC_T] = b.t; w[REC_N_LE] = (long long)b.n0; w[REC_N_GT] = (long long)(N - b.n0); w[REC_VALID] = 1;
    } else {
        w[REC_T] = top[0] < 0 ? 0 : top[0] - OFFSET; w[REC_N_LE] = (long long)N; w[REC_N_GT] = 0; w[REC_VALID] = 0;
    }
}

// ---- foreground mask of a device threshold ---------------------------------------------------------------------------
constexpr long MASK_GRID_CAP = 2048;      // workgroups at most: eight per CU

template <typename T>
__global__ __launch_bounds__(TPB) void k_scan_threshold_mask(const T* __restrict__ x, long V,
                                                             const long long* __restrict__ rec, uint8_t* __restrict__ out) {
    constexpr int N = 16 / (int)sizeof(T);
    const int tid = (int)threadIdx.x;
    const bool valid = rec[REC_VALID] != 0;
    const int t = (int)rec[REC_T];
    // elements before the plane's first 16-byte boundary, whole vectors, elements after them
    const long head = min(V, (long)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) / sizeof(T)));
    const long items = (V - head) / N;
    const long tail0 = head + items * N;
    const bool ovec = ((uintptr_t)(out + head) & (uintptr_t)(N - 1)) == 0;

    for (long it = (long)blockIdx.x * TPB + tid; it < items; it += (long)gridDim.x * TPB) {
        const long e = head + it * N;
        const u32x4 w = *reinterpret_cast<const u32x4*>(x + e);
        unsigned b[N / 4];
#pragma unroll
        for (int i = 0; i < N / 4; ++i) b[i] = 0u;
#pragma unroll
        for (int j = 0; j < N; ++j) b[j >> 2] |= (unsigned)(!valid || unpack<T>(w, j) > t) << (8 * (j & 3));
        if (ovec) {
            if (N == 8) {
                u32x2 o;
                o[0] = b[0]; o[1] = b[1];
                *reinterpret_cast<u32x2*>(out + e) = o;
            } else {
                u32x4 o;
#pragma unroll
                for (int i = 0; i < N / 4; ++i) o[i] = b[i];
                *reinterpret_cast<u32x4*>(out + e) = o;
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) out[e + j] = (uint8_t)((b[j >> 2] >> (8 * (j & 3))) & 0xFFu);
        }
    }
    if (blockIdx.x == 0) {
        const long loose = head + (V - tail0);
        for (long i = tid; i < loose; i += TPB) {
            const long e = i < head ? i : tail0 + (i - head);
            out[e] = (uint8_t)(!valid || (int)x[e] > t);
        }
    }
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
                       q_lo, q_hi, b_min, b_max, (int)(clip != 0), (const long long*)nullptr, slot);
    return mivp_check_launch("scan_window_plan");
}

extern "C" int mivp_scan_otsu_plan(const int64_t* hist, int32_t C, int64_t* otsu, mivp_stream_t stream) {
    MIVP_REQUIRE(hist && otsu && C >= 1 && C <= 4);
    MIVP_REQUIRE(((uintptr_t)hist & 7u) == 0 && ((uintptr_t)otsu & 7u) == 0);
    hipLaunchKernelGGL(k_scan_otsu_plan, dim3((unsigned)C), dim3(OTSU_TPB), 0, (hipStream_t)stream, (const u64*)hist,
                       (long long*)otsu);
    return mivp_check_launch("scan_otsu_plan");
}

extern "C" int mivp_scan_window_plan_above(const int64_t* hist, int32_t C, int32_t mode, double q_lo, double q_hi,
                                           double b_min, double b_max, int32_t clip, const int64_t* otsu, float* slot,
                                           mivp_stream_t stream) {
    MIVP_REQUIRE(hist && otsu && slot && C >= 1 && C <= 4 && (mode == PLAN_PERCENTILE || mode == PLAN_ZSCORE));
    MIVP_REQUIRE(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0);                    // (false for a NaN)
    MIVP_REQUIRE(mode == PLAN_ZSCORE || (isfinite(b_min) && isfinite(b_max) && b_min <= b_max));
    MIVP_REQUIRE(((uintptr_t)hist & 7u) == 0 && ((uintptr_t)otsu & 7u) == 0 && ((uintptr_t)slot & 3u) == 0);
    hipLaunchKernelGGL(k_scan_window_plan, dim3((unsigned)C), dim3(TPB), 0, (hipStream_t)stream, (const u64*)hist, (int)mode,
                       q_lo, q_hi, b_min, b_max, (int)(clip != 0), (const long long*)otsu, slot);
    return mivp_check_launch("scan_window_plan_above");
}

extern "C" int mivp_scan_threshold_mask(const void* raw, int32_t dtype, int32_t C, const int32_t* dims, int32_t channel,
                                        const int64_t* otsu, uint8_t* out, mivp_stream_t stream) {
    MIVP_REQUIRE(raw && dims && otsu && out && (dtype == 0 || dtype == 4) && C >= 1 && C <= 4 && channel >= 0 && channel < C);
    MIVP_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long)dims[0] * dims[1] * dims[2] < (1L << 31));
    MIVP_REQUIRE(((uintptr_t)otsu & 7u) == 0 && (dtype == 0 || ((uintptr_t)raw & 1u) == 0));
    const long V = (long)dims[0] * dims[1] * dims[2];
    const int n = dtype == 0 ? 16 : 8;
    const long want = (V / n + TPB - 1) / TPB;
    const dim3 grid((unsigned)(want < 1 ? 1 : (want > MASK_GRID_CAP ? MASK_GRID_CAP : want)));
    const long long* rec = (const long long*)otsu + REC_WORDS * channel;
    if (dtype == 0)
        hipLaunchKernelGGL(k_scan_threshold_mask<uint8_t>, grid, dim3(TPB), 0, (hipStream_t)stream,
                           static_cast<const uint8_t*>(raw) + (long)channel * V, V, rec, out);
    else
        hipLaunchKernelGGL(k_scan_threshold_mask<int16_t>, grid, dim3(TPB), 0, (hipStream_t)stream,
                           static_cast<const int16_t*>(raw) + (long)channel * V, V, rec, out);
    return mivp_check_launch("scan_threshold_mask");
}
