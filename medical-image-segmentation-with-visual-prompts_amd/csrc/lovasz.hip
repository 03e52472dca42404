// Lovasz-Softmax loss term (Berman, Triki & Blaschko, CVPR 2018): the Lovasz extension of the per-class Jaccard loss, on an
// exact device-wide sort of one 32-bit key per (segment, voxel) (mivp_amd/losses.py lovasz_softmax_loss /
// LovaszSoftmaxLoss).  The sort itself is csrc/sort_common.hpp.
//
// Segments: class c >= c0 of sample b (per_image) or of the whole batch; S = (per_image ? B : 1) K segments of
// N = (per_image ? 1 : B) vol keys, K = C - c0.  Per segment, over its valid voxels, p = softmax(z), g = [y == c],
// e = g ? 1 - p_c : p_c (1 - p_y as the sum of the other exponentials over the denominator), G = sum g:
//   J(F, K) = 1 - (G - F) / (G + K), J(0, 0) = 0;   loss_seg = sum_j e_(j) (J_j - J_(j-1)) over the errors in descending order
// Launches of a call, all unconditional, their number independent of B, C and the data:
//   zero, keys   key = LV_TOP - ((bits(e) << 1) | g): ascending keys are descending errors, the foreground first inside a tie;
//                an invalid voxel gets LV_INVALID, which sorts behind every valid key.  G and the valid count per segment by
//                integer atomics (one per workgroup and segment).
//   sort         twelve launches, keys only
//   prefix       tile counts, their scan, then prefix[j] = the foreground keys among sorted positions 0 .. j
//   statistics   per tile the sum of e_(j) (J_j - J_(j-1)), each difference in closed form (no cancellation):
//                foreground 1 / (G + K_j);  background (G - F_j) / ((G + K_j - 1) (G + K_j)), or 1 when G + K_j - 1 == 0
//   finalize     one workgroup, f64, fixed order: the segments' sums, the present classes, value and the segments' factors
//   gradient     memory order; every voxel recomputes its keys, finds each key's tie group [lo, hi) in its segment by binary
//                search and applies the tie rule: with F, K the foreground / background keys in front of the group,
//                a foreground voxel gets 1 / (G + K), a background voxel of a group of b gets
//                (J(F, K + b) - J(F, K)) / b = (G - F) / ((G + K) (G + K + b)), or 1 / b when G + K == 0.
//                dz_k = w p_k (q_k - sum_c p_c q_c), q_c = factor_c s_c sgn_c, sgn = -1 on the foreground.
#include "segloss_common.hpp"
#include "sort_common.hpp"

namespace {
constexpr uint32_t LV_TOP = 0x7F000001u;                        // the key bits of e = 1 on the foreground
constexpr uint32_t LV_INVALID = 0xFFFFFFFFu;
constexpr int LV_TPB = 256;

struct LvOpt {
    int c0, has_ignore;
    float ignore;
    int per_image, all;
};

// softmax and errors of one voxel.  Both the key pass and the gradient pass build their keys here: no contraction, so the
// two see the same bits.
template <int C>
struct LvVoxel {
    float p[C], e[C];
    int cls;
    MIVP_DEV LvVoxel(const float* zz, float yv, const LvOpt& o) {
#pragma clang fp contract(off)
        cls = seg_class_rt(yv, C, o.has_ignore, o.ignore);
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, zz[c]);
        float den = 0.f, eo = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            p[c] = __expf(zz[c] - mx);
            den += p[c];
            eo += c == cls ? 0.f : p[c];
        }
        const float inv_den = __builtin_amdgcn_rcpf(den);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            p[c] *= inv_den;
            e[c] = fminf(fmaxf(c == cls ? eo * inv_den : p[c], 0.f), 1.f);     // (a NaN becomes 0: the key stays in range)
        }
    }
    MIVP_DEV uint32_t key(int c) const {
        return cls >= 0 ? LV_TOP - ((__float_as_uint(e[c]) << 1) | (c == cls ? 1u : 0u)) : LV_INVALID;
    }
};

MIVP_DEV uint32_t lv_key_fg(uint32_t key) { return key == LV_INVALID ? 0u : (LV_TOP - key) & 1u; }
MIVP_DEV float lv_key_error(uint32_t key) { return __uint_as_float((LV_TOP - key) >> 1); }

__global__ __launch_bounds__(LV_TPB) void k_lovasz_zero(uint32_t* __restrict__ counts, int n) {
    const int i = blockIdx.x * LV_TPB + threadIdx.x;
    if (i < n) counts[i] = 0u;
}

// grid (blocks of a sample, B).  keys [S][N]; counts [S][2] = (G, valid voxels)
template <int C>
__global__ __launch_bounds__(LV_TPB) void k_lovasz_keys(const float* __restrict__ z, const float* __restrict__ y, long vol, LvOpt o,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ counts) {
    __shared__ uint32_t red[LV_TPB / 64][C + 1];
    const int b = blockIdx.y, K = C - o.c0;
    const long N = o.per_image ? vol : (long)gridDim.y * vol;
    const long seg0 = o.per_image ? (long)b * K : 0L, at0 = o.per_image ? 0L : (long)b * vol;
    uint32_t cnt[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) cnt[c] = 0u;
    for (long v = (long)blockIdx.x * LV_TPB + threadIdx.x; v < vol; v += (long)gridDim.x * LV_TPB) {
        const long i = (long)b * vol + v;
        float zz[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
        const LvVoxel<C> vx(zz, y[i], o);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (c >= o.c0) keys[(seg0 + (c - o.c0)) * N + at0 + v] = vx.key(c);
            cnt[c] += c == vx.cls ? 1u : 0u;
        }
        cnt[C] += vx.cls >= 0 ? 1u : 0u;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c <= C; ++c) {
        uint32_t s = cnt[c];
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        if (lane == 0) red[wave][c] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int c = o.c0 + threadIdx.x;
        atomicAdd(&counts[2 * (seg0 + threadIdx.x)], (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]));
        atomicAdd(&counts[2 * (seg0 + threadIdx.x) + 1], (red[0][C] + red[1][C]) + (red[2][C] + red[3][C]));
    }
}

// sum of v over the workgroup on thread 0 (fixed order); red: one word per wave
MIVP_DEV uint32_t lv_block_sum(uint32_t v, uint32_t* red) {
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (nblk, S): the foreground keys of a tile
__global__ __launch_bounds__(LV_TPB) void k_lovasz_tilecount(const uint32_t* __restrict__ keys, long N, int nblk,
                                                             uint32_t* __restrict__ tcount) {
    __shared__ uint32_t red[LV_TPB / 64];
    const uint32_t* k = keys + (long)blockIdx.y * N;
    const long first = (long)blockIdx.x * SORT_TILE;
    uint32_t f = 0u;
#pragma unroll
    for (int r = 0; r < SORT_IPT; ++r) {
        const long j = first + r * LV_TPB + threadIdx.x;
        if (j < N) f += lv_key_fg(k[j]);
    }
    const uint32_t s = lv_block_sum(f, red);
    if (threadIdx.x == 0) tcount[(long)blockIdx.y * nblk + blockIdx.x] = s;
}

// exclusive scan of v over the workgroup (thread order); red: one word per wave.  total: the workgroup's sum
MIVP_DEV uint32_t lv_block_exscan(uint32_t v, uint32_t* red, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                          // red may still be read from an earlier call
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    for (int w = 0; w < wave; ++w) before += red[w];
    total = (red[0] + red[1]) + (red[2] + red[3]);
    return before + inc - v;
}

// grid S: tcount[seg][.] -> its exclusive scan, in place
__global__ __launch_bounds__(LV_TPB) void k_lovasz_tilescan(uint32_t* __restrict__ tcount, int nblk) {
    __shared__ uint32_t red[LV_TPB / 64];
    uint32_t* t = tcount + (long)blockIdx.x * nblk;
    uint32_t carry = 0u;
    for (int first = 0; first < nblk; first += LV_TPB) {
        const int i = first + threadIdx.x;
        const uint32_t v = i < nblk ? t[i] : 0u;
        uint32_t total;
        const uint32_t ex = lv_block_exscan(v, red, total);
        if (i < nblk) t[i] = carry + ex;
        carry += total;
    }
}

// grid (nblk, S): prefix[j] = foreground keys among positions 0 .. j of the segment; thread t owns SORT_IPT consecutive keys
__global__ __launch_bounds__(LV_TPB) void k_lovasz_prefix(const uint32_t* __restrict__ keys, long N, int nblk,
                                                          const uint32_t* __restrict__ tcount, uint32_t* __restrict__ prefix) {
    __shared__ uint32_t red[LV_TPB / 64];
    const uint32_t* k = keys + (long)blockIdx.y * N;
    uint32_t* p = prefix + (long)blockIdx.y * N;
    const long first = (long)blockIdx.x * SORT_TILE + (long)threadIdx.x * SORT_IPT;
    uint32_t inc[SORT_IPT], run = 0u;
#pragma unroll
    for (int r = 0; r < SORT_IPT; ++r) {
        run += first + r < N ? lv_key_fg(k[first + r]) : 0u;
        inc[r] = run;
    }
    uint32_t total;
    const uint32_t before = tcount[(long)blockIdx.y * nblk + blockIdx.x] + lv_block_exscan(run, red, total);
#pragma unroll
    for (int r = 0; r < SORT_IPT; ++r)
        if (first + r < N) p[first + r] = before + inc[r];
}

// grid (nblk, S): part[seg][tile] = sum over the tile's valid positions of e_(j) (J_j - J_(j-1))
__global__ __launch_bounds__(LV_TPB) void k_lovasz_stats(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ prefix,
                                                         const uint32_t* __restrict__ counts, long N, int nblk,
                                                         float* __restrict__ part) {
    __shared__ float red[LV_TPB / 64];
    const int seg = blockIdx.y;
    const uint32_t* k = keys + (long)seg * N;
    const uint32_t* p = prefix + (long)seg * N;
    const float G = (float)counts[2 * seg];
    const long first = (long)blockIdx.x * SORT_TILE;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < SORT_IPT; ++r) {
        const long j = first + r * LV_TPB + threadIdx.x;
        const uint32_t key = j < N ? k[j] : LV_INVALID;
        if (key != LV_INVALID) {
            const uint32_t F = p[j], Kj = (uint32_t)(j + 1) - F;   // counts with position j included
            const float e = lv_key_error(key);
            if (lv_key_fg(key)) {
                acc += e / (G + (float)Kj);
            } else {
                const float gk = G + (float)(Kj - 1u);
                acc += gk > 0.f ? e * ((G - (float)F) / (gk * (gk + 1.f))) : e;
            }
        }
    }
    for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)seg * nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup.  Groups = samples (per_image) or the batch; a group's value = the mean of its qualifying segments (0 without
// one), the value = w x the mean of the groups.  factor[seg] = 1 / (qualifying segments of the group x groups), 0 for an absent
// class.  f64, fixed order.
__global__ __launch_bounds__(256) void k_lovasz_finalize(const float* __restrict__ part, const uint32_t* __restrict__ counts,
                                                         int groups, int K, int nblk, int all, float lam,
                                                         const float* __restrict__ weight, float* __restrict__ factor,
                                                         float* __restrict__ loss) {
    __shared__ double red[256];
    double total = 0.0;
    for (int g = 0; g < groups; ++g) {
        double gsum[SEG_MAXC];
        for (int k = 0; k < K; ++k) {
            const long seg = (long)g * K + k;
            double s = 0.0;
            for (int r = threadIdx.x; r < nblk; r += 256) s += (double)part[seg * nblk + r];
            __syncthreads();
            red[threadIdx.x] = s;
            __syncthreads();
            for (int o = 128; o >= 1; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            gsum[k] = red[0];
        }
        if (threadIdx.x == 0) {
            int cnt = 0;
            double sum = 0.0;
            for (int k = 0; k < K; ++k) {
                const bool in = all || counts[2 * ((long)g * K + k)] > 0u;
                cnt += in ? 1 : 0;
                sum += in ? gsum[k] : 0.0;
            }
            total += cnt ? sum / (double)cnt : 0.0;
            for (int k = 0; k < K; ++k) {
                const bool in = all || counts[2 * ((long)g * K + k)] > 0u;
                factor[(long)g * K + k] = in ? (float)(1.0 / ((double)cnt * (double)groups)) : 0.f;
            }
        }
    }
    if (threadIdx.x == 0 && loss) {
        const double w = (double)lam * (weight ? (double)weight[0] : 1.0);
        loss[0] = (float)(w * total / (double)groups);
    }
}

// first position of a[0 .. n) that holds a value >= key (upper == false) or > key (upper == true), from position lo on
MIVP_DEV long lv_bound(const uint32_t* __restrict__ a, long lo, long n, uint32_t key, bool upper) {
    long hi = n;
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        const uint32_t v = a[mid];
        if (upper ? v <= key : v < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// dz (=, or += with ACC): one thread per voxel in memory order.  The product is rounded before the add, as in the sibling terms.
template <int C, bool ACC>
__global__ __launch_bounds__(LV_TPB) void k_lovasz_grad(const float* __restrict__ z, const float* __restrict__ y, long vol, int B,
                                                        LvOpt o, const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ counts,
                                                        const float* __restrict__ factor, float lam,
                                                        const float* __restrict__ weight, const float* __restrict__ gscale,
                                                        float* __restrict__ dz) {
    const int K = C - o.c0;
    const long total = (long)B * vol, N = o.per_image ? vol : total;
    const float coef = (gscale ? gscale[0] : 1.f) * (lam * (weight ? weight[0] : 1.f));
    for (long i = (long)blockIdx.x * LV_TPB + threadIdx.x; i < total; i += (long)gridDim.x * LV_TPB) {
        const long b = i / vol;
        float zz[C], q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
        const LvVoxel<C> vx(zz, y[i], o);
        const bool valid = vx.cls >= 0;
        float pq = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q[c] = 0.f;
            if (c >= o.c0 && valid) {
                const long seg = (o.per_image ? b * K : 0L) + (c - o.c0);
                const float fac = factor[seg];
                if (fac != 0.f) {
                    const uint32_t* a = keys + seg * N;
                    const uint32_t key = vx.key(c);
                    const float G = (float)counts[2 * seg];
                    const long lo = lv_bound(a, 0L, N, key, false);
                    const uint32_t F = lo > 0 ? prefix[seg * N + lo - 1] : 0u;
                    const float gk = G + (float)((uint32_t)lo - F);
                    if (c == vx.cls) {
                        q[c] = -fac / gk;                                  // G >= 1: this voxel is foreground
                    } else {
                        const float nb = (float)(lv_bound(a, lo, N, key, true) - lo);
                        q[c] = gk > 0.f ? fac * ((G - (float)F) / (gk * (gk + nb))) : fac / fmaxf(nb, 1.f);
                    }
                }
            }
            pq += vx.p[c] * q[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float g = valid ? coef * (vx.p[c] * (q[c] - pq)) : 0.f;
            dz[i * C + c] = ACC ? __fadd_rn(dz[i * C + c], g) : g;
        }
    }
}

// bytes of a call's workspace, every part 256-byte aligned:
// keys [S N] | the sort's (alt, hist, base) | prefix [S N] | tcount [S][nblk] | counts [S][2] | part [S][nblk] f32 | factor [S] f32
struct LvWs {
    size_t keys, sort, prefix, tcount, counts, part, factor, total;
    LvWs(long S, int64_t N) {
        const long nblk = sort_nblk(N);
        keys = 0;
        sort = keys + sort_align((size_t)S * N * 4);
        prefix = sort + SortWs(S, N).total;
        tcount = prefix + sort_align((size_t)S * N * 4);
        counts = tcount + sort_align((size_t)S * nblk * 4);
        part = counts + sort_align((size_t)S * 2 * 4);
        factor = part + sort_align((size_t)S * nblk * 4);
        total = factor + sort_align((size_t)S * 4);
    }
};

struct LvShape {
    long S, N;
    LvShape(int32_t B, int32_t C, const LvOpt& o, int64_t vol)
        : S((long)(o.per_image ? B : 1) * (C - o.c0)), N((long)(o.per_image ? 1 : B) * vol) {}
};

int lovasz_keys_run(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, const LvOpt& o, long S,
                    uint32_t* keys, uint32_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(k_lovasz_zero, dim3((unsigned)((2 * S + LV_TPB - 1) / LV_TPB)), dim3(LV_TPB), 0, st, counts, (int)(2 * S));
    const long bpb = (vol + LV_TPB - 1) / LV_TPB;
    const dim3 grid((unsigned)(bpb > 2048 ? 2048 : bpb), (unsigned)B);
#define L_KEYS(CC) hipLaunchKernelGGL((k_lovasz_keys<CC>), grid, dim3(LV_TPB), 0, st, logits, target, (long)vol, o, keys, counts)
    SEG_C_SWITCH(L_KEYS)
#undef L_KEYS
    return mivp_check_launch("lovasz_keys");
}

int lovasz_run(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, const LvOpt& o, float lam,
               const float* weight, char* ws, float* loss, const float* gscale, float* dlogits, int accumulate, bool do_loss,
               mivp_stream_t stream) {
    const LvShape sh(B, C, o, vol);
    const LvWs w(sh.S, sh.N);
    const int nblk = (int)sort_nblk(sh.N), S = (int)sh.S;
    uint32_t* keys = (uint32_t*)(ws + w.keys);
    uint32_t* prefix = (uint32_t*)(ws + w.prefix);
    uint32_t* tcount = (uint32_t*)(ws + w.tcount);
    uint32_t* counts = (uint32_t*)(ws + w.counts);
    float* part = (float*)(ws + w.part);
    float* factor = (float*)(ws + w.factor);
    hipStream_t st = (hipStream_t)stream;
    if (do_loss) {
        int rc = lovasz_keys_run(logits, target, B, vol, C, o, sh.S, keys, counts, st);
        if (rc != MIVP_OK) return rc;
        rc = sort_u32_run(keys, S, sh.N, ws + w.sort, st);
        if (rc != MIVP_OK) return rc;
        const dim3 tiles((unsigned)nblk, (unsigned)S);
        hipLaunchKernelGGL(k_lovasz_tilecount, tiles, dim3(LV_TPB), 0, st, keys, sh.N, nblk, tcount);
        hipLaunchKernelGGL(k_lovasz_tilescan, dim3((unsigned)S), dim3(LV_TPB), 0, st, tcount, nblk);
        hipLaunchKernelGGL(k_lovasz_prefix, tiles, dim3(LV_TPB), 0, st, keys, sh.N, nblk, tcount, prefix);
        rc = mivp_check_launch("lovasz_prefix");
        if (rc != MIVP_OK) return rc;
        hipLaunchKernelGGL(k_lovasz_stats, tiles, dim3(LV_TPB), 0, st, keys, prefix, counts, sh.N, nblk, part);
        hipLaunchKernelGGL(k_lovasz_finalize, dim3(1), dim3(256), 0, st, part, counts, o.per_image ? (int)B : 1, (int)(C - o.c0),
                           nblk, o.all, lam, weight, factor, loss);
        rc = mivp_check_launch("lovasz_finalize");
        if (rc != MIVP_OK) return rc;
    }
    if (!dlogits) return MIVP_OK;
    const long total = (long)B * vol;
    const unsigned grid = (unsigned)((total + LV_TPB - 1) / LV_TPB > 8192 ? 8192 : (total + LV_TPB - 1) / LV_TPB);
#define L_GRAD1(CC, AA) hipLaunchKernelGGL((k_lovasz_grad<CC, AA>), dim3(grid), dim3(LV_TPB), 0, st, logits, target, (long)vol, \
                                           (int)B, o, keys, prefix, counts, factor, lam, weight, gscale, dlogits)
#define L_GRAD(CC) do { if (accumulate) L_GRAD1(CC, true); else L_GRAD1(CC, false); } while (0)
    SEG_C_SWITCH(L_GRAD)
#undef L_GRAD
#undef L_GRAD1
    return mivp_check_launch("lovasz_grad");
}
}  // namespace

#define LV_REQUIRE_OPTIONS()                                                                                  \
    MIVP_REQUIRE(B > 0 && vol > 0 && C >= 2 && C <= SEG_MAXC);                                                \
    const LvOpt o = {include_background ? 0 : 1, has_ignore ? 1 : 0, (float)ignore_index, per_image ? 1 : 0,  \
                     classes_all ? 1 : 0};                                                                     \
    MIVP_REQUIRE(B <= 65535 && sort_fits(LvShape(B, C, o, vol).S, LvShape(B, C, o, vol).N))

extern "C" int mivp_sort_tile(void) { return SORT_TILE; }

extern "C" size_t mivp_sort_u32_ws(int32_t segments, int64_t n) {
    if (!sort_fits(segments, n)) return 0;
    return SortWs(segments, n).total;
}

extern "C" int mivp_sort_u32(uint32_t* keys, int32_t segments, int64_t n, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(segments >= 1 && segments <= 65535 && n >= 1);
    MIVP_REQUIRE(sort_fits(segments, n));                      // key counts below 2^31
    MIVP_REQUIRE(keys && workspace);
    return sort_u32_run(keys, segments, n, (char*)workspace, (hipStream_t)stream);
}

extern "C" size_t mivp_lovasz_ws(int32_t B, int32_t C, int32_t include_background, int32_t per_image, int64_t vol) {
    if (B < 1 || B > 65535 || vol < 1 || C < 2 || C > SEG_MAXC) return 0;
    const LvOpt o = {include_background ? 0 : 1, 0, 0.f, per_image ? 1 : 0, 0};
    const LvShape sh(B, C, o, vol);
    if (!sort_fits(sh.S, sh.N)) return 0;
    return LvWs(sh.S, sh.N).total;
}

extern "C" int mivp_lovasz_keys(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                                int32_t include_background, int32_t ignore_index, int32_t has_ignore, int32_t per_image,
                                uint32_t* keys, uint32_t* counts, mivp_stream_t stream) {
    const int classes_all = 0;
    LV_REQUIRE_OPTIONS();
    MIVP_REQUIRE(logits && target && keys && counts);
    return lovasz_keys_run(logits, target, B, vol, C, o, LvShape(B, C, o, vol).S, keys, counts, (hipStream_t)stream);
}

extern "C" int mivp_lovasz_loss(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                                int32_t include_background, int32_t ignore_index, int32_t has_ignore, int32_t per_image,
                                int32_t classes_all, float lambda_lovasz, const float* weight, void* workspace, float* loss,
                                float* dlogits, int32_t accumulate, mivp_stream_t stream) {
    LV_REQUIRE_OPTIONS();
    MIVP_REQUIRE(lambda_lovasz >= 0.f && lambda_lovasz <= 3.0e38f);
    MIVP_REQUIRE(logits && target && workspace && loss);
    return lovasz_run(logits, target, B, vol, C, o, lambda_lovasz, weight, (char*)workspace, loss, nullptr, dlogits, accumulate,
                      true, stream);
}

extern "C" int mivp_lovasz_loss_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                                     int32_t include_background, int32_t ignore_index, int32_t has_ignore, int32_t per_image,
                                     int32_t classes_all, float lambda_lovasz, const float* weight, const void* workspace,
                                     const float* gscale, float* dlogits, int32_t accumulate, mivp_stream_t stream) {
    LV_REQUIRE_OPTIONS();
    MIVP_REQUIRE(lambda_lovasz >= 0.f && lambda_lovasz <= 3.0e38f);
    MIVP_REQUIRE(logits && target && workspace && dlogits);
    return lovasz_run(logits, target, B, vol, C, o, lambda_lovasz, weight, (char*)const_cast<void*>(workspace), nullptr, gscale,
                      dlogits, accumulate, false, stream);
}
