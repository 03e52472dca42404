// Intensity transfer tables: histogram equalisation, histogram matching and Nyul-Udupa landmark standardisation of an
// integer scan (mivp_amd/transfer.py).  A table is float32 [C][65536]: table[c][v + 32768] is the model-input
// intensity of raw value v, defined for every v.  It comes with a meta record int32 [C][4] = (lowest counted value, highest
// counted value, valid, 0), both values 0 when nothing is counted.
//
// The plan kernels run one workgroup per channel over the int64 histogram of scanstats.hip, as k_scan_window_plan does:
// thread t sums its 256 consecutive bins and notes its lowest and highest counted bin, thread 0 forms the prefix of the 256
// counts, and every thread then walks its bins again with the running C(v) = sum_{w <= v} n_w and writes its 256 table
// entries.  With an Otsu record whose valid word is set, the bins at or below its threshold read as zero everywhere (the
// rule of mivp_scan_window_plan_above).  Everything is integer up to the final float64 expressions; floating-point
// contraction is off in this file, so each written operation rounds on its own and the result is rounded to float32 once.
// No atomics: equal calls give equal bits.
//   k_transfer_equalize   v0 = the lowest counted value, c0 = n_v0, d = N - c0; r = max(C(v) - c0, 0) / d (0 when d == 0);
//                         y = r * (b_max - b_min) + b_min.
//   k_transfer_match      u(v) = the smallest value u with C_ref(u) * N_src >= max(C_src(v), 1) * N_ref, compared in
//                         128-bit integers (below 2^66 for N < 2^33); u is non-decreasing in v, so a thread finds the
//                         reference chunk of its first bin by bisection of the reference's per-thread prefix and then only
//                         walks forward, bisecting again where the answer leaves the chunk.  N_src == 0 or N_ref == 0:
//                         u = v; N >= 2^33 the same with valid = 0.  Then the prepare launch's own map with the words of
//                         the reference slot: y = fmaf((float)u, s, t), clamped to [lo, hi] with clip.
//   k_scan_landmarks      the nearest-rank order statistics m_i of up to 16 quantiles (k = max(1, ceil(q * (double)N)), the
//                         rank search of k_scan_window_plan): int64 [C][17] = (valid, m_0 .. m_{n-1}, 0 ...), valid when
//                         N > 0 and m_{n-1} > m_0.
//   k_landmark_bank_add   bank float64 [C][17] = (count, sums): a valid record adds 1 and
//                         s_lo + (m_i - m_0) / (m_{n-1} - m_0) * (s_hi - s_lo); an invalid one adds nothing.
//   k_transfer_landmarks  standard landmarks S_i = sum_i / count; knots are the distinct m_i in increasing order, a knot's
//                         standard value the mean of the S_i that share it (summed in index order, divided by their number);
//                         segment j serves M_j <= v < M_{j+1}, segment 0 everything below, segment K - 2 everything from
//                         M_{K-1} on: y = T_j + (v - M_j) / (M_{j+1} - M_j) * (T_{j+1} - T_j), with clip clamped to
//                         [T_0, T_{K-1}].  K < 2: the single knot's value everywhere (0 when N == 0); an empty bank: 0
//                         everywhere and valid = 0.
//
// k_transfer_apply: out[c][e] = table[c][raw[c][e] + 32768], the streaming pass.  The scan is read as k_scan_hist reads it
// (16-byte loads of 8 int16 / 16 uint8 values, grid-strided so a wave reads 1 KiB contiguous; the elements before the first
// 16-byte boundary of the plane and after the last whole vector one by one by workgroup 0), the result written as 16-byte
// stores where the output is aligned with the input.  Two read paths for the table, the same bits from both:
//   global    every value gathers from the table in global memory (256 KB a channel: resident in L2);
//   window    a workgroup first copies the entries of up to 16384 consecutive values, from the lowest counted value of the
//             meta record up to the highest, into LDS (64 KiB: two workgroups per CU) and gathers from there; a value
//             outside the window gathers from global memory.  uint8 scans stage their 256 entries.
#include "common.hpp"
#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256;
constexpr int NBINS = 65536;
constexpr int OFFSET = 32768;             // bin of value 0
constexpr int CHUNK = NBINS / TPB;        // bins per thread of a plan kernel
constexpr int WIN = 16384;                // table entries a workgroup of the apply kernel keeps in LDS (64 KiB)
constexpr int MAXQ = 16;                  // landmarks at most
constexpr int LM_WORDS = 1 + MAXQ;        // (valid, m_0 .. m_15) and (count, sum_0 .. sum_15)
constexpr long GRID_CAP_WINDOW = 512;     // workgroups per channel at most: two per CU (LDS)
constexpr long GRID_CAP_GLOBAL = 2048;    // eight per CU
typedef unsigned long long u64;
typedef unsigned __int128 u128;

enum { REC_T = 0, REC_VALID = 3, REC_WORDS = 4 };       // the Otsu record of a channel (scanstats.hip)
enum { APPLY_GLOBAL = 1 };                              // flag bit 0 of mivp_scan_transfer_apply

struct Quantiles { double q[MAXQ]; int n; };

// the first bin that counts: the one above a valid Otsu threshold, else 0
MIVP_DEV int first_bin(const long long* __restrict__ otsu, int c) {
    if (otsu && otsu[REC_WORDS * c + REC_VALID]) return (int)otsu[REC_WORDS * c + REC_T] + OFFSET + 1;
    return 0;
}

// Pass 1 of every plan over one channel's bins h[65536]: pre[0 .. TPB] becomes the exclusive prefix of the per-thread counts
// (pre[TPB] = N) and span = (lowest counted bin, highest counted bin), -1 where nothing is counted.
MIVP_DEV void chunk_prefix(const u64* __restrict__ h, int first, u64* pre, int* los, int* his, int* span) {
    const int tid = (int)threadIdx.x;
    u64 n = 0ull;
    int lo = -1, hi = -1;
    for (int i = 0; i < CHUNK; ++i) {
        const int bin = tid * CHUNK + i;
        const u64 k = bin < first ? 0ull : h[bin];
        n += k;
        if (k) {
            if (lo < 0) lo = bin;
            hi = bin;
        }
    }
    pre[tid + 1] = n;
    los[tid] = lo;
    his[tid] = hi;
    __syncthreads();
    if (tid == 0) {
        u64 run = 0ull;
        int a = -1, b = -1;
        pre[0] = 0ull;
        for (int t = 0; t < TPB; ++t) {
            run += pre[t + 1];
            pre[t + 1] = run;
            if (los[t] >= 0) {
                if (a < 0) a = los[t];
                b = his[t];
            }
        }
        span[0] = a;
        span[1] = b;
    }
    __syncthreads();
}

MIVP_DEV void write_meta(int* __restrict__ meta, int c, const int* span, bool valid) {
    int* m = meta + 4 * c;
    m[0] = span[0] < 0 ? 0 : span[0] - OFFSET;
    m[1] = span[1] < 0 ? 0 : span[1] - OFFSET;
    m[2] = valid ? 1 : 0;
    m[3] = 0;
}

__global__ __launch_bounds__(TPB) void k_transfer_equalize(const u64* __restrict__ hist, double b_min, double b_max,
                                                           const long long* __restrict__ otsu, float* __restrict__ table,
                                                           int* __restrict__ meta) {
    __shared__ u64 pre[TPB + 1];
    __shared__ int los[TPB], his[TPB], span[2];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS;
    float* __restrict__ tab = table + (long)c * NBINS;
    const int first = first_bin(otsu, c);
    chunk_prefix(h, first, pre, los, his, span);
    const u64 N = pre[TPB];
    const u64 c0 = span[0] < 0 ? 0ull : h[span[0]];
    const u64 d = N - c0;
    const double width = b_max - b_min;
    u64 cum = pre[tid];
    for (int i = 0; i < CHUNK; ++i) {
        const int bin = tid * CHUNK + i;
        cum += bin < first ? 0ull : h[bin];
        const u64 num = cum > c0 ? cum - c0 : 0ull;
        const double r = d ? (double)num / (double)d : 0.0;
        const double y = r * width + b_min;
        tab[bin] = (float)y;
    }
    if (tid == 0) write_meta(meta, c, span, N != 0ull);
}

__global__ __launch_bounds__(TPB) void k_transfer_match(const u64* __restrict__ hist, const u64* __restrict__ ref,
                                                        const float* __restrict__ slot, int clip,
                                                        const long long* __restrict__ otsu, float* __restrict__ table,
                                                        int* __restrict__ meta) {
    __shared__ u64 pre[TPB + 1], pre_r[TPB + 1];
    __shared__ int los[TPB], his[TPB], span[2], span_r[2];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS;
    const u64* __restrict__ hr = ref + (long)c * NBINS;
    float* __restrict__ tab = table + (long)c * NBINS;
    const int first = first_bin(otsu, c);
    chunk_prefix(hr, 0, pre_r, los, his, span_r);
    chunk_prefix(h, first, pre, los, his, span);
    const u64 Ns = pre[TPB], Nr = pre_r[TPB];
    const bool exact = Ns < (1ull << 33) && Nr < (1ull << 33);     // beyond it the products outgrow 128 bits' margin
    const bool same = !exact || !Ns || !Nr;                        // u(v) = v
    const float s = slot[8 * c], t = slot[8 * c + 1], lo = slot[8 * c + 2], hi = slot[8 * c + 3];
    u64 cum = pre[tid];
    int u = -1;                                                    // the reference bin reached, and C_ref of it
    u64 cr = 0ull;
    for (int i = 0; i < CHUNK; ++i) {
        const int bin = tid * CHUNK + i;
        cum += bin < first ? 0ull : h[bin];
        int ub = bin;
        if (!same) {
            const u128 target = (u128)(cum ? cum : 1ull) * Nr;     // at most N_src N_ref, which C_ref(32767) N_src reaches
            if ((u128)cr * Ns < target) {
                int ch = (u + 1) / CHUNK;
                if ((u128)pre_r[ch + 1] * Ns < target) {           // not in this chunk: the first chunk whose end reaches it
                    int a = ch + 1, b = TPB - 1;
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if ((u128)pre_r[mid + 1] * Ns < target) a = mid + 1;
                        else b = mid;
                    }
                    u = a * CHUNK - 1;
                    cr = pre_r[a];
                }
                do {                                               // ends inside the chunk: its last bin has pre_r[ch + 1]
                    ++u;
                    cr += hr[u];
                } while ((u128)cr * Ns < target && u < NBINS - 1);
            }
            ub = u;
        }
        float y = fmaf((float)(ub - OFFSET), s, t);
        if (clip) y = y < lo ? lo : (y > hi ? hi : y);
        tab[bin] = y;
    }
    if (tid == 0) write_meta(meta, c, span, exact && Ns && Nr);
}

__global__ __launch_bounds__(TPB) void k_scan_landmarks(const u64* __restrict__ hist, Quantiles qs,
                                                        const long long* __restrict__ otsu, long long* __restrict__ rec) {
    __shared__ u64 pre[TPB + 1];
    __shared__ int los[TPB], his[TPB], span[2];
    __shared__ u64 rank[MAXQ];
    __shared__ int val[MAXQ];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS;
    const int first = first_bin(otsu, c);
    chunk_prefix(h, first, pre, los, his, span);
    if (tid < MAXQ) {
        const double k = tid < qs.n ? ceil(qs.q[tid] * (double)pre[TPB]) : 0.0;
        rank[tid] = k < 1.0 ? 1ull : (u64)k;
        val[tid] = 0;                           // an empty histogram finds no rank
    }
    __syncthreads();
    const u64 below = pre[tid], upto = pre[tid + 1];
    for (int r = 0; r < qs.n; ++r) {
        const u64 k = rank[r];
        if (k > below && k <= upto) {           // one thread per rank: the prefix is non-decreasing
            u64 cum = below;
            for (int i = 0; i < CHUNK; ++i) {
                const int bin = tid * CHUNK + i;
                cum += bin < first ? 0ull : h[bin];
                if (cum >= k) { val[r] = bin - OFFSET; break; }
            }
        }
    }
    __syncthreads();
    if (tid >= LM_WORDS) return;
    long long* w = rec + LM_WORDS * c;
    if (tid == 0) w[0] = (pre[TPB] != 0ull && val[qs.n - 1] > val[0]) ? 1 : 0;
    else w[tid] = tid - 1 < qs.n ? (long long)val[tid - 1] : 0;
}

__global__ __launch_bounds__(64) void k_landmark_bank_add(const long long* __restrict__ rec, int C, int n, double s_lo,
                                                          double s_hi, double* __restrict__ bank) {
    const int c = (int)threadIdx.x / MAXQ, i = (int)threadIdx.x % MAXQ;
    if (c >= C || i >= n) return;
    const long long* w = rec + LM_WORDS * c;
    if (!w[0]) return;
    const long long m0 = w[1], ml = w[n];
    if (ml <= m0) return;                       // (a record that says valid has m_{n-1} > m_0)
    double* b = bank + LM_WORDS * c;
    const double ratio = (double)(w[1 + i] - m0) / (double)(ml - m0);
    const double term = s_lo + ratio * (s_hi - s_lo);
    b[1 + i] = b[1 + i] + term;
    if (i == 0) b[0] = b[0] + 1.0;
}

__global__ __launch_bounds__(TPB) void k_transfer_landmarks(const u64* __restrict__ hist, const long long* __restrict__ rec,
                                                            const double* __restrict__ bank, int n, int clip,
                                                            const long long* __restrict__ otsu, float* __restrict__ table,
                                                            int* __restrict__ meta) {
    __shared__ u64 pre[TPB + 1];
    __shared__ int los[TPB], his[TPB], span[2];
    __shared__ int M[MAXQ];
    __shared__ double T[MAXQ];
    __shared__ int K;
    const int tid = (int)threadIdx.x, c = (int)blockIdx.x;
    const u64* __restrict__ h = hist + (long)c * NBINS;
    float* __restrict__ tab = table + (long)c * NBINS;
    chunk_prefix(h, first_bin(otsu, c), pre, los, his, span);
    const double count = bank[LM_WORDS * c];
    if (tid == 0) {
        const long long* w = rec + LM_WORDS * c;
        const double* b = bank + LM_WORDS * c;
        int k = 0;
        if (count > 0.0) {
            int i = 0;
            while (i < n) {                     // the indices that share one landmark value are neighbours
                const long long m = w[1 + i];
                double sum = 0.0;
                int share = 0;
                for (; i < n && w[1 + i] == m; ++i, ++share) sum = sum + b[1 + i] / count;
                M[k] = (int)m;
                T[k] = sum / (double)share;
                ++k;
            }
        }
        K = k;
    }
    __syncthreads();
    const u64 N = pre[TPB];
    const int knots = K;
    if (knots < 2) {
        const float y = (knots == 1 && N != 0ull) ? (float)T[0] : 0.0f;
        for (int i = 0; i < CHUNK; ++i) tab[tid * CHUNK + i] = y;
    } else {
        const double t_lo = T[0], t_hi = T[knots - 1];
        int j = 0;
        for (int i = 0; i < CHUNK; ++i) {
            const int bin = tid * CHUNK + i, v = bin - OFFSET;
            while (j < knots - 2 && v >= M[j + 1]) ++j;
            const double frac = (double)(v - M[j]) / (double)(M[j + 1] - M[j]);
            double y = T[j] + frac * (T[j + 1] - T[j]);
            if (clip) y = y < t_lo ? t_lo : (y > t_hi ? t_hi : y);
            tab[bin] = (float)y;
        }
    }
    if (tid == 0) write_meta(meta, c, span, count > 0.0 && knots >= 2 && N != 0ull);
}

// ---- the streaming pass ----------------------------------------------------------------------------------------------
template <typename T> MIVP_DEV int unpack(const u32x4& w, int j);
template <> MIVP_DEV int unpack<int16_t>(const u32x4& w, int j) { return (int)(int16_t)(w[j >> 1] >> (16 * (j & 1))); }
template <> MIVP_DEV int unpack<uint8_t>(const u32x4& w, int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu); }

template <typename T, bool WINDOW>
__global__ __launch_bounds__(TPB) void k_transfer_apply(const T* __restrict__ raw, long V, const float* __restrict__ table,
                                                        const int* __restrict__ meta, float* __restrict__ out) {
    constexpr int N = 16 / (int)sizeof(T);
    constexpr int LDS = !WINDOW ? 1 : (sizeof(T) == 1 ? 256 : WIN);
    __shared__ float win[LDS];
    const int tid = (int)threadIdx.x, c = (int)blockIdx.y;
    const T* __restrict__ x = raw + (long)c * V;
    const float* __restrict__ tab = table + (long)c * NBINS;
    float* __restrict__ o = out + (long)c * V;
    int wbin = 0, wlen = 0;                     // the bins [wbin, wbin + wlen) are in LDS
    if (WINDOW) {
        if (sizeof(T) == 1) {
            wbin = OFFSET;
            wlen = 256;
        } else {
            const int lo = meta[4 * c] + OFFSET, hi = meta[4 * c + 1] + OFFSET;
            wbin = lo < 0 ? 0 : (lo > NBINS - WIN ? NBINS - WIN : lo);
            wlen = hi - wbin + 1;
            wlen = wlen < 0 ? 0 : (wlen > WIN ? WIN : wlen);
        }
        for (int i = tid; i < wlen; i += TPB) win[i] = tab[wbin + i];
        __syncthreads();
    }
    auto look = [&](int v) -> float {
        const int bin = v + OFFSET;
        if (WINDOW) {
            const unsigned i = (unsigned)(bin - wbin);
            if (i < (unsigned)wlen) return win[i];
        }
        return tab[bin];
    };
    // elements before the plane's first 16-byte boundary, whole vectors, elements after them
    const long head = min(V, (long)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) / sizeof(T)));
    const long items = (V - head) / N;
    const long tail0 = head + items * N;
    const bool ovec = ((uintptr_t)(o + head) & 15u) == 0;

    for (long it = (long)blockIdx.x * TPB + tid; it < items; it += (long)gridDim.x * TPB) {
        const long e = head + it * N;
        const u32x4 w = *reinterpret_cast<const u32x4*>(x + e);
        float y[N];
#pragma unroll
        for (int j = 0; j < N; ++j) y[j] = look(unpack<T>(w, j));
        if (ovec) {
#pragma unroll
            for (int j = 0; j < N; j += 4) {
                f32x4 q;
                q[0] = y[j]; q[1] = y[j + 1]; q[2] = y[j + 2]; q[3] = y[j + 3];
                *reinterpret_cast<f32x4*>(o + e + j) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) o[e + j] = y[j];
        }
    }
    if (blockIdx.x == 0) {
        const long loose = head + (V - tail0);
        for (long i = tid; i < loose; i += TPB) {
            const long e = i < head ? i : tail0 + (i - head);
            o[e] = look((int)x[e]);
        }
    }
}

template <typename T>
void launch_apply(bool window, dim3 grid, hipStream_t st, const void* raw, long V, const float* table, const int* meta,
                  float* out) {
    if (window)
        hipLaunchKernelGGL((k_transfer_apply<T, true>), grid, dim3(TPB), 0, st, static_cast<const T*>(raw), V, table, meta, out);
    else
        hipLaunchKernelGGL((k_transfer_apply<T, false>), grid, dim3(TPB), 0, st, static_cast<const T*>(raw), V, table, meta, out);
}

bool aligned(const void* p, unsigned bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1u)) == 0; }

// 2 <= n <= 16 quantiles, strictly increasing in [0, 1] (false for a NaN)
bool quantiles_ok(const double* q, int n) {
    if (!q || n < 2 || n > MAXQ) return false;
    for (int i = 0; i < n; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0) || (i && !(q[i] > q[i - 1]))) return false;
    return true;
}
}  // namespace

extern "C" int mivp_scan_transfer_equalize(const int64_t* hist, int32_t C, double b_min, double b_max, const int64_t* otsu,
                                           float* table, int32_t* meta, mivp_stream_t stream) {
    MIVP_REQUIRE(hist && table && meta && C >= 1 && C <= 4);
    MIVP_REQUIRE(isfinite(b_min) && isfinite(b_max) && b_min <= b_max);
    MIVP_REQUIRE(aligned(hist, 8) && aligned(otsu, 8) && aligned(table, 4) && aligned(meta, 4));
    hipLaunchKernelGGL(k_transfer_equalize, dim3((unsigned)C), dim3(TPB), 0, (hipStream_t)stream, (const u64*)hist, b_min,
                       b_max, (const long long*)otsu, table, (int*)meta);
    return mivp_check_launch("scan_transfer_equalize");
}

extern "C" int mivp_scan_transfer_match(const int64_t* hist, const int64_t* ref_hist, const float* ref_slot, int32_t C,
                                        int32_t clip, const int64_t* otsu, float* table, int32_t* meta,
                                        mivp_stream_t stream) {
    MIVP_REQUIRE(hist && ref_hist && ref_slot && table && meta && C >= 1 && C <= 4);
    MIVP_REQUIRE(aligned(hist, 8) && aligned(ref_hist, 8) && aligned(otsu, 8) && aligned(ref_slot, 4) && aligned(table, 4) &&
                 aligned(meta, 4));
    hipLaunchKernelGGL(k_transfer_match, dim3((unsigned)C), dim3(TPB), 0, (hipStream_t)stream, (const u64*)hist,
                       (const u64*)ref_hist, ref_slot, (int)(clip != 0), (const long long*)otsu, table, (int*)meta);
    return mivp_check_launch("scan_transfer_match");
}

extern "C" int mivp_scan_landmarks(const int64_t* hist, int32_t C, const void* quantiles_f64, int32_t n, const int64_t* otsu,
                                   int64_t* landmarks, mivp_stream_t stream) {
    const double* quantiles = static_cast<const double*>(quantiles_f64);
    MIVP_REQUIRE(hist && landmarks && C >= 1 && C <= 4 && aligned(quantiles, 8) && quantiles_ok(quantiles, (int)n));
    MIVP_REQUIRE(aligned(hist, 8) && aligned(otsu, 8) && aligned(landmarks, 8));
    Quantiles qs;
    for (int i = 0; i < MAXQ; ++i) qs.q[i] = i < n ? quantiles[i] : 0.0;
    qs.n = (int)n;
    hipLaunchKernelGGL(k_scan_landmarks, dim3((unsigned)C), dim3(TPB), 0, (hipStream_t)stream, (const u64*)hist, qs,
                       (const long long*)otsu, (long long*)landmarks);
    return mivp_check_launch("scan_landmarks");
}

extern "C" int mivp_scan_landmark_bank_add(const int64_t* landmarks, int32_t C, int32_t n, double s_lo, double s_hi,
                                           void* bank_f64, mivp_stream_t stream) {
    double* bank = static_cast<double*>(bank_f64);
    MIVP_REQUIRE(landmarks && bank && C >= 1 && C <= 4 && n >= 2 && n <= MAXQ);
    MIVP_REQUIRE(isfinite(s_lo) && isfinite(s_hi) && s_lo <= s_hi);
    MIVP_REQUIRE(aligned(landmarks, 8) && aligned(bank, 8));
    hipLaunchKernelGGL(k_landmark_bank_add, dim3(1), dim3(64), 0, (hipStream_t)stream, (const long long*)landmarks, (int)C,
                       (int)n, s_lo, s_hi, bank);
    return mivp_check_launch("scan_landmark_bank_add");
}

extern "C" int mivp_scan_transfer_landmarks(const int64_t* hist, const int64_t* landmarks, const void* bank_f64, int32_t C,
                                            int32_t n, int32_t clip, const int64_t* otsu, float* table, int32_t* meta,
                                            mivp_stream_t stream) {
    const double* bank = static_cast<const double*>(bank_f64);
    MIVP_REQUIRE(hist && landmarks && bank && table && meta && C >= 1 && C <= 4 && n >= 2 && n <= MAXQ);
    MIVP_REQUIRE(aligned(hist, 8) && aligned(landmarks, 8) && aligned(bank, 8) && aligned(otsu, 8) && aligned(table, 4) &&
                 aligned(meta, 4));
    hipLaunchKernelGGL(k_transfer_landmarks, dim3((unsigned)C), dim3(TPB), 0, (hipStream_t)stream, (const u64*)hist,
                       (const long long*)landmarks, bank, (int)n, (int)(clip != 0), (const long long*)otsu, table, (int*)meta);
    return mivp_check_launch("scan_transfer_landmarks");
}

extern "C" int mivp_scan_transfer_apply(const void* raw, int32_t dtype, int32_t C, const int32_t* dims, const float* table,
                                        const int32_t* meta, int32_t flags, float* out, mivp_stream_t stream) {
    MIVP_REQUIRE(raw && dims && table && meta && out && (dtype == 0 || dtype == 4) && C >= 1 && C <= 4 &&
                 (flags & ~APPLY_GLOBAL) == 0);
    MIVP_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long)dims[0] * dims[1] * dims[2] < (1L << 31));
    MIVP_REQUIRE(aligned(table, 4) && aligned(meta, 4) && aligned(out, 4) && (dtype == 0 || aligned(raw, 2)));
    const long V = (long)dims[0] * dims[1] * dims[2];
    const int n = dtype == 0 ? 16 : 8;
    const bool window = !(flags & APPLY_GLOBAL);
    const long cap = window ? GRID_CAP_WINDOW : GRID_CAP_GLOBAL;
    const long want = (V / n + TPB - 1) / TPB;
    const dim3 grid((unsigned)(want < 1 ? 1 : (want > cap ? cap : want)), (unsigned)C);
    if (dtype == 0) launch_apply<uint8_t>(window, grid, (hipStream_t)stream, raw, V, table, (const int*)meta, out);
    else launch_apply<int16_t>(window, grid, (hipStream_t)stream, raw, V, table, (const int*)meta, out);
    return mivp_check_launch("scan_transfer_apply");
}
