// Tversky region term + top-k (hard-voxel) cross-entropy: the voxel term of csrc/segloss.hip averaged over the k hardest
// valid voxels of the batch only (nnU-Net's DC_and_topk_loss), by an exact three-level radix select.
//   u_v   = w[y_v] (1 - p_y)^gamma (-log p_y) of a valid voxel, N = valid voxels of the batch, k = max(1, floor(top_k N)) (f64)
//   key_v = the bits of u_v as this file's statistics pass computed it in f32, clamped to >= +0: 31 significant bits, monotone
//           as an unsigned integer.  Stored ONCE (one word per voxel, 0xFFFFFFFF at an invalid voxel); every later pass reads
//           the stored key, so the histograms, the sums and the gradient's selection agree on every voxel.
//   tau   = the k-th largest key, n_gt = #{key > tau}, n_eq = #{key == tau}, rho = (k - n_gt) / n_eq
//   voxel = (sum_{key > tau} u + (k - n_gt) tau) / k;  d voxel = (1 / k) sum_v s_v d u_v,  s_v = 1 | rho | 0 for key > | == | < tau
// Launches (all unconditional: k and tau are device data, a recording holds for any later content):
//   zero       the three histograms and the record
//   stats      the region rows of k_seg_loss_stats + key store + level-1 histogram (key bits 30..20; LDS bins, integer flush)
//   refine<2>  every workgroup scans histogram 1 from the top (N, k, bin b1), then counts key bits 19..10 under prefix b1
//   refine<3>  scans histogram 2 (bin b2), counts key bits 9..0 under prefix b1 b2
//   sum        scans histogram 3 (tau, n_gt, n_eq), per-workgroup partial sums of u over key > tau in a fixed order
//   finalize   one workgroup, f64: region value, voxel value, the record, loss[0]
//   grad       logits + labels + keys -> dlogits, every element once
// Only integer atomics; every float sum has a fixed order: equal calls give equal bits.
#include "segloss_common.hpp"

namespace {
constexpr int TK_REC = MIVP_SEG_TOPK_RECORD_WORDS;
constexpr int TK_NB1 = 2048, TK_NB = 1024;      // bins of level 1 (11 bits) and of levels 2, 3 (10 bits each)
constexpr int TK_MAX_BLOCKS = 1024;             // workgroups (and partial sums) of the keys-only passes
constexpr uint32_t TK_INVALID = 0xFFFFFFFFu;
static_assert(TK_REC + TK_NB1 + 2 * TK_NB + TK_MAX_BLOCKS == MIVP_SEG_TOPK_KEYS_OFFSET, "workspace layout of mivp.h");
// words of the record: the first seven are the documented ones (mivp.h), the rest carry the select from pass to pass
enum { R_N, R_K, R_TAU, R_NGT, R_NEQ, R_RHO, R_VOXEL, R_B1, R_GT1, R_B2, R_GT2 };

struct TopkWs {
    float *part, *stats, *psum;
    uint32_t *rec, *h1, *h2, *h3, *keys;
};

inline size_t topk_base(int32_t B, int64_t vol) { return (seg_region_ws(B, vol) + 3) / 4 * 4; }

inline TopkWs topk_ws(float* ws, int32_t B, int64_t vol) {
    TopkWs w;
    w.part = ws;
    w.stats = ws + (long)B * seg_bpb(vol) * SEG_K;
    uint32_t* r = reinterpret_cast<uint32_t*>(ws + topk_base(B, vol));
    w.rec = r;
    w.h1 = r + TK_REC;
    w.h2 = w.h1 + TK_NB1;
    w.h3 = w.h2 + TK_NB;
    w.psum = reinterpret_cast<float*>(w.h3 + TK_NB);
    w.keys = r + MIVP_SEG_TOPK_KEYS_OFFSET;
    return w;
}

template <int C>
MIVP_DEV uint32_t seg_topk_key(const SegVoxel<C>& v, const SegOpt& o) {
    const float u = v.wy * (seg_pow(v.om, o.gamma) * -v.logp);
    return v.cls < 0 ? TK_INVALID : (u > 0.f ? __float_as_uint(u) : 0u);       // no -0, no negative rounding residue
}

template <int C>
MIVP_DEV uint32_t seg_topk_voxel(const float* zz, float yv, const float* wt, const SegOpt& o, float* acc, uint32_t* lh) {
    const SegVoxel<C> v(zz, yv, wt, o);
    seg_voxel_region_stats<C>(v, o, acc);
    const uint32_t key = seg_topk_key<C>(v, o);
    if (key != TK_INVALID) atomicAdd(&lh[key >> 20], 1u);
    return key;
}

// LDS bins -> global bins; most bins of a workgroup are empty
template <int NB>
MIVP_DEV void topk_flush(const uint32_t* lh, uint32_t* __restrict__ h) {
    for (int i = threadIdx.x; i < NB; i += 256) {
        const uint32_t n = lh[i];
        if (n) atomicAdd(&h[i], n);
    }
}

// The whole workgroup (256 threads) walks the NB bins of h from the top: bin = the one with above < krem <= above + h[bin],
// above = the count of the bins over it; total = the count of all bins.  top_k > 0: krem is first set to
// max(1, floor(top_k total)).  Nothing found (an empty histogram): bin = above = 0.  sh: 6 words of LDS.
template <int NB>
MIVP_DEV void topk_scan(const uint32_t* __restrict__ h, double top_k, uint32_t& krem, uint32_t* sh, uint32_t& bin,
                        uint32_t& above, uint32_t& total) {
    constexpr int PER = NB / 256;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t loc[PER], s = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        loc[i] = h[NB - 1 - (t * PER + i)];
        s += loc[i];
    }
    uint32_t inc = s;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d);
        inc += lane >= d ? up : 0u;
    }
    if (lane == 63) sh[wave] = inc;
    if (t == 0) { sh[4] = 0u; sh[5] = 0u; }
    __syncthreads();
    const uint32_t w0 = sh[0], w1 = sh[1], w2 = sh[2], w3 = sh[3];
    total = (w0 + w1) + (w2 + w3);
    if (top_k > 0.0) {
        const double want = floor(top_k * (double)total);
        krem = want < 1.0 ? 1u : (uint32_t)want;
    }
    uint32_t a = (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u) + (inc - s);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (a < krem && krem - a <= loc[i]) { sh[4] = (uint32_t)(NB - 1 - (t * PER + i)); sh[5] = a; }
        a += loc[i];
    }
    __syncthreads();
    bin = sh[4];
    above = sh[5];
}
}

__global__ void k_seg_topk_zero(uint32_t* __restrict__ rec) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < TK_REC + TK_NB1 + 2 * TK_NB; i += gridDim.x * blockDim.x) rec[i] = 0u;
}

// pass 1: the partial rows of k_seg_loss_stats (voxel columns left zero), the keys, histogram 1
template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_seg_topk_stats(const float* __restrict__ z, const float* __restrict__ y, long vol,
                                                        SegOpt o, const float* __restrict__ cw, int blocks_per_b,
                                                        float* __restrict__ part, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ h1) {
    __shared__ float red[4][SEG_K];
    __shared__ uint32_t lh[TK_NB1];
    for (int i = threadIdx.x; i < TK_NB1; i += 256) lh[i] = 0u;
    __syncthreads();
    const int b = blockIdx.x / blocks_per_b, blk = blockIdx.x % blocks_per_b;
    float wt[C];
    seg_load_weights<C>(cw, wt);
    float acc[SEG_K];
#pragma unroll
    for (int i = 0; i < SEG_K; ++i) acc[i] = 0.f;
    if (VEC) {
        const long nq = vol >> 2;
        for (long q = (long)blk * 256 + threadIdx.x; q < nq; q += (long)blocks_per_b * 256) {
            const long v = (long)b * vol + 4 * q;
            float zb[4 * C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + v * C + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + v);
            uint4 k4;
            k4.x = seg_topk_voxel<C>(zb, y4.x, wt, o, acc, lh);
            k4.y = seg_topk_voxel<C>(zb + C, y4.y, wt, o, acc, lh);
            k4.z = seg_topk_voxel<C>(zb + 2 * C, y4.z, wt, o, acc, lh);
            k4.w = seg_topk_voxel<C>(zb + 3 * C, y4.w, wt, o, acc, lh);
            *reinterpret_cast<uint4*>(keys + v) = k4;
        }
    } else {
        for (long v = (long)blk * 256 + threadIdx.x; v < vol; v += (long)blocks_per_b * 256) {
            const float* zv = z + ((long)b * vol + v) * C;
            float zz[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = zv[c];
            keys[(long)b * vol + v] = seg_topk_voxel<C>(zz, y[(long)b * vol + v], wt, o, acc, lh);
        }
    }
    seg_store_partial_row<C>(acc, red, part + (long)blockIdx.x * SEG_K);       // (its barrier also ends the LDS counting)
    topk_flush<TK_NB1>(lh, h1);
}

// keys of a keys-only pass: 16-byte loads over the whole batch, the last total % 4 keys by workgroup 0
template <typename F>
MIVP_DEV void topk_for_keys(const uint32_t* __restrict__ keys, long total, F&& f) {
    const long nq = total >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const uint4 k4 = *reinterpret_cast<const uint4*>(keys + 4 * q);
        f(k4.x); f(k4.y); f(k4.z); f(k4.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(total & 3)) f(keys[4 * nq + threadIdx.x]);
}

// passes 2, 3: the bin of the previous level, then the histogram of the next 10 key bits under the prefix found so far
template <int LEVEL>
__global__ __launch_bounds__(256) void k_seg_topk_refine(const uint32_t* __restrict__ keys, long total, double top_k,
                                                         uint32_t* __restrict__ rec, const uint32_t* __restrict__ hprev,
                                                         uint32_t* __restrict__ hout) {
    __shared__ uint32_t lh[TK_NB];
    __shared__ uint32_t sh[6];
    for (int i = threadIdx.x; i < TK_NB; i += 256) lh[i] = 0u;
    uint32_t prefix, bin, above, n;
    if (LEVEL == 2) {
        uint32_t k = 0u;
        topk_scan<TK_NB1>(hprev, top_k, k, sh, bin, above, n);
        prefix = bin;
        if (blockIdx.x == 0 && threadIdx.x == 0) { rec[R_N] = n; rec[R_K] = k; rec[R_B1] = bin; rec[R_GT1] = above; }
    } else {
        const uint32_t b1 = rec[R_B1], gt1 = rec[R_GT1];
        uint32_t krem = rec[R_K] - gt1;
        topk_scan<TK_NB>(hprev, 0.0, krem, sh, bin, above, n);
        prefix = b1 << 10 | bin;
        if (blockIdx.x == 0 && threadIdx.x == 0) { rec[R_B2] = bin; rec[R_GT2] = gt1 + above; }
    }
    constexpr int SHIFT = LEVEL == 2 ? 20 : 10;                               // (an invalid key matches no prefix)
    topk_for_keys(keys, total, [&](uint32_t key) {
        if ((key >> SHIFT) == prefix) atomicAdd(&lh[(key >> (SHIFT - 10)) & (TK_NB - 1)], 1u);
    });
    __syncthreads();
    topk_flush<TK_NB>(lh, hout);
}

// pass 4: tau from histogram 3, then psum[workgroup] = sum of u over key > tau
__global__ __launch_bounds__(256) void k_seg_topk_sum(const uint32_t* __restrict__ keys, long total, uint32_t* __restrict__ rec,
                                                      const uint32_t* __restrict__ h3, float* __restrict__ psum) {
    __shared__ uint32_t sh[6];
    __shared__ float red[4];
    const uint32_t gt2 = rec[R_GT2];
    uint32_t krem = rec[R_K] - gt2, bin, above, n;
    topk_scan<TK_NB>(h3, 0.0, krem, sh, bin, above, n);
    const uint32_t tau = rec[R_B1] << 20 | rec[R_B2] << 10 | bin;
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec[R_TAU] = tau; rec[R_NGT] = gt2 + above; rec[R_NEQ] = h3[bin]; }
    float acc = 0.f;
    topk_for_keys(keys, total, [&](uint32_t key) { acc += (key != TK_INVALID && key > tau) ? __uint_as_float(key) : 0.f; });
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) psum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void k_seg_topk_finalize(const float* __restrict__ part, int B, int blocks_per_b, int C, SegOpt o,
                                    float* __restrict__ stats, const float* __restrict__ psum, int n_psum,
                                    uint32_t* __restrict__ rec, float* __restrict__ loss) {
    double above_sum = 0.0;
    if (threadIdx.x < 64) {                                                   // the first wave, fixed order; thread 0 uses it
        for (int j = threadIdx.x; j < n_psum; j += 64) above_sum += (double)psum[j];
        for (int sh = 32; sh > 0; sh >>= 1) above_sum += __shfl_xor(above_sum, sh);
    }
    const double region = seg_finalize_region(part, B, blocks_per_b, C, o, stats);
    if (threadIdx.x == 0) {
        const uint32_t N = rec[R_N], k = rec[R_K], n_gt = rec[R_NGT], n_eq = rec[R_NEQ];
        const double tau = (double)__uint_as_float(rec[R_TAU]), rest = (double)(k - n_gt);
        const double voxel = N > 0u ? (above_sum + rest * tau) / (double)k : 0.0;
        rec[R_RHO] = __float_as_uint(n_eq > 0u ? (float)(rest / (double)n_eq) : 0.f);
        rec[R_VOXEL] = __float_as_uint((float)voxel);
        loss[0] = (float)((double)o.lam_r * region + (double)o.lam_v * voxel);
    }
}

// weight of a voxel's cross-entropy term from its stored key: lambda_voxel s_v / k
MIVP_DEV float topk_weight(uint32_t key, uint32_t tau, float w_gt, float w_eq) {
    return key == TK_INVALID ? 0.f : (key > tau ? w_gt : (key == tau ? w_eq : 0.f));
}

// pass 5: dz = gscale * d loss / dz, every element stored once; as k_seg_loss_grad with a per-voxel weight from the key
template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_seg_topk_grad(const float* __restrict__ z, const float* __restrict__ y, long vol, int B,
                                                       SegOpt o, const float* __restrict__ cw, const float* __restrict__ stats,
                                                       const uint32_t* __restrict__ rec, const uint32_t* __restrict__ keys,
                                                       const float* __restrict__ gscale, float* __restrict__ dz) {
    const long total = (long)B * vol;
    const float up = gscale ? gscale[0] : 1.f;
    const float ncls = (float)(C - o.c0);
    const float wd = o.lam_r / ((o.batch ? 1.f : (float)B) * ncls);
    const uint32_t tau = rec[R_TAU];
    const float w_gt = rec[R_N] > 0u ? o.lam_v / (float)rec[R_K] : 0.f;
    const float w_eq = w_gt * __uint_as_float(rec[R_RHO]);
    float wt[C];
    seg_load_weights<C>(cw, wt);
    if (VEC) {
        const long nq = total >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
            const long i = 4 * q;
            const int b = o.batch ? B : (int)(i / vol);
            float zb[4 * C], gb[4 * C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + i * C + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + i);
            const uint4 k4 = *reinterpret_cast<const uint4*>(keys + i);
            float qa[C], qb[C];
            seg_region_consts<C>(stats + b * SEG_K, o, wd, qa, qb);
            seg_voxel_grad<C>(zb, y4.x, wt, o, topk_weight(k4.x, tau, w_gt, w_eq), up, qa, qb, gb);
            seg_voxel_grad<C>(zb + C, y4.y, wt, o, topk_weight(k4.y, tau, w_gt, w_eq), up, qa, qb, gb + C);
            seg_voxel_grad<C>(zb + 2 * C, y4.z, wt, o, topk_weight(k4.z, tau, w_gt, w_eq), up, qa, qb, gb + 2 * C);
            seg_voxel_grad<C>(zb + 3 * C, y4.w, wt, o, topk_weight(k4.w, tau, w_gt, w_eq), up, qa, qb, gb + 3 * C);
#pragma unroll
            for (int j = 0; j < C; ++j)
                *reinterpret_cast<float4*>(dz + i * C + 4 * j) = make_float4(gb[4 * j], gb[4 * j + 1], gb[4 * j + 2], gb[4 * j + 3]);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int b = o.batch ? B : (int)(i / vol);
            float zz[C], gz[C], qa[C], qb[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
            seg_region_consts<C>(stats + b * SEG_K, o, wd, qa, qb);
            seg_voxel_grad<C>(zz, y[i], wt, o, topk_weight(keys[i], tau, w_gt, w_eq), up, qa, qb, gz);
#pragma unroll
            for (int c = 0; c < C; ++c) dz[i * C + c] = gz[c];
        }
    }
}

// the region part of mivp_seg_loss_ws (rounded up to 4 words), the record, the histograms, the partial sums, the keys
extern "C" size_t mivp_seg_topk_ws(int32_t B, int64_t vol) {
    if (B <= 0 || vol <= 0) return 0;
    return topk_base(B, vol) + MIVP_SEG_TOPK_KEYS_OFFSET + ((size_t)B * (size_t)vol + 3) / 4 * 4;
}

static int seg_topk_run(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, const SegOpt& o,
                        const float* class_weights, double top_k, float* workspace, float* loss, const float* gscale,
                        float* dlogits, bool do_loss, mivp_stream_t stream) {
    const long bpb = seg_bpb(vol), total = (long)B * vol;
    const TopkWs w = topk_ws(workspace, B, vol);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vol % 4 == 0;                             // 16-byte loads of four voxels
    if (do_loss) {
        int rc;
        hipLaunchKernelGGL(k_seg_topk_zero, dim3(4), dim3(256), 0, st, w.rec);
        if ((rc = mivp_check_launch("seg_topk_zero"))) return rc;
#define T_STATS1(CC, VV) hipLaunchKernelGGL((k_seg_topk_stats<CC, VV>), dim3((unsigned)(B * bpb)), dim3(256), 0, st, logits, target, \
                                            (long)vol, o, class_weights, (int)bpb, w.part, w.keys, w.h1)
#define T_STATS(CC) do { if (vec) T_STATS1(CC, true); else T_STATS1(CC, false); } while (0)
        SEG_C_SWITCH(T_STATS)
#undef T_STATS
#undef T_STATS1
        if ((rc = mivp_check_launch("seg_topk_stats"))) return rc;
        long nkb = (total + 1023) / 1024;
        if (nkb > TK_MAX_BLOCKS) nkb = TK_MAX_BLOCKS;
        hipLaunchKernelGGL(k_seg_topk_refine<2>, dim3((unsigned)nkb), dim3(256), 0, st, w.keys, total, top_k, w.rec, w.h1, w.h2);
        if ((rc = mivp_check_launch("seg_topk_refine2"))) return rc;
        hipLaunchKernelGGL(k_seg_topk_refine<3>, dim3((unsigned)nkb), dim3(256), 0, st, w.keys, total, top_k, w.rec, w.h2, w.h3);
        if ((rc = mivp_check_launch("seg_topk_refine3"))) return rc;
        hipLaunchKernelGGL(k_seg_topk_sum, dim3((unsigned)nkb), dim3(256), 0, st, w.keys, total, w.rec, w.h3, w.psum);
        if ((rc = mivp_check_launch("seg_topk_sum"))) return rc;
        hipLaunchKernelGGL(k_seg_topk_finalize, dim3(1), dim3(1024), 0, st, w.part, (int)B, (int)bpb, (int)C, o, w.stats, w.psum,
                           (int)nkb, w.rec, loss);
        if ((rc = mivp_check_launch("seg_topk_finalize"))) return rc;
    }
    if (!dlogits) return MIVP_OK;
    const long items = vec ? total / 4 : total;
    const unsigned grid = (unsigned)((items + 255) / 256 > 8192 ? 8192 : (items + 255) / 256);
#define T_GRAD1(CC, VV) hipLaunchKernelGGL((k_seg_topk_grad<CC, VV>), dim3(grid), dim3(256), 0, st, logits, target, (long)vol, \
                                           (int)B, o, class_weights, w.stats, w.rec, w.keys, gscale, dlogits)
#define T_GRAD(CC) do { if (vec) T_GRAD1(CC, true); else T_GRAD1(CC, false); } while (0)
    SEG_C_SWITCH(T_GRAD)
#undef T_GRAD
#undef T_GRAD1
    return mivp_check_launch("seg_topk_grad");
}

#define SEG_TOPK_REQUIRE()                                                                                  \
    SEG_REQUIRE_OPTIONS();                                                                                  \
    MIVP_REQUIRE(top_k > 0.0 && top_k <= 1.0 && lambda_voxel > 0.f);                                        \
    MIVP_REQUIRE((long)B * vol < (1L << 31) && vol < (1L << 31));                                           \
    MIVP_REQUIRE(((uintptr_t)workspace & 15) == 0)

extern "C" int mivp_seg_topk(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                             int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                             const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                             float lambda_voxel, double top_k, float* workspace, float* loss, float* dlogits,
                             mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && loss);
    SEG_TOPK_REQUIRE();
    return seg_topk_run(logits, target, B, vol, C, o, class_weights, top_k, workspace, loss, nullptr, dlogits, true, stream);
}

extern "C" int mivp_seg_topk_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                                  int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                                  const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                                  float lambda_voxel, double top_k, float* workspace, const float* gscale, float* dlogits,
                                  mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && dlogits);
    SEG_TOPK_REQUIRE();
    return seg_topk_run(logits, target, B, vol, C, o, class_weights, top_k, workspace, nullptr, gscale, dlogits, false, stream);
}
