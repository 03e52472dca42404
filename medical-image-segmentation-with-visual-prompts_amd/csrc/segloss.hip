// Tversky region term + weighted (focal) softmax cross-entropy with an ignore label, forward value and gradient in two
// streaming passes over the logits.  Same operands and launch geometry as csrc/loss.hip.
//   a voxel is VALID when its label is an integer in [0, C) and not the ignore label; an invalid voxel adds to no sum and
//   gets an exactly zero gradient.  With p = softmax_c(z), t = one-hot(label), sums over the valid voxels of a sample
//   (of the whole batch when `batch`), s = 1e-5:
//   TI_c   = (2 I_c + s) / (2 I_c + 2 alpha (P_c - I_c) + 2 beta (T_c - I_c) + s),   I = sum p t, P = sum p, T = sum t
//   region = mean over (b, c >= c0) [over c >= c0 when batch] of 1 - TI_c
//   voxel  = - sum_v w[y_v] (1 - p_y)^gamma log p_y / sum_v w[y_v]                   (valid voxels of the whole batch; 0 when W = 0)
//   loss   = lambda_region region + lambda_voxel voxel
// 1 - p_y is formed as sum_{c != y} e_c / den and log p_y as z_y - max - log den: both keep their digits when the logits
// saturate.  No atomics: partial rows per workgroup, a fixed-order f64 finalize, every dz element stored exactly once.
#include "segloss_common.hpp"

namespace {
template <int C>
MIVP_DEV void seg_voxel_stats(const float* zz, float yv, const float* wt, const SegOpt& o, float* acc) {
    const SegVoxel<C> v(zz, yv, wt, o);
    seg_voxel_region_stats<C>(v, o, acc);
    if (o.lam_v > 0.f) {                                           // wy is 0 at an invalid voxel
        acc[SEG_NUM] -= v.wy * (seg_pow(v.om, o.gamma) * v.logp);
        acc[SEG_W] += v.wy;
    }
}
}

// pass 1: per-workgroup partial rows [SEG_K] for ONE sample per workgroup row; VEC: four consecutive voxels per thread and
// iteration through 16-byte loads (vol % 4 == 0), the loads of one iteration independent
template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_seg_loss_stats(const float* __restrict__ z, const float* __restrict__ y, long vol,
                                                        SegOpt o, const float* __restrict__ cw, int blocks_per_b,
                                                        float* __restrict__ part) {
    __shared__ float red[4][SEG_K];
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
            seg_voxel_stats<C>(zb, y4.x, wt, o, acc);
            seg_voxel_stats<C>(zb + C, y4.y, wt, o, acc);
            seg_voxel_stats<C>(zb + 2 * C, y4.z, wt, o, acc);
            seg_voxel_stats<C>(zb + 3 * C, y4.w, wt, o, acc);
        }
    } else {
        for (long v = (long)blk * 256 + threadIdx.x; v < vol; v += (long)blocks_per_b * 256) {
            const float* zv = z + ((long)b * vol + v) * C;
            float zz[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = zv[c];
            seg_voxel_stats<C>(zz, y[(long)b * vol + v], wt, o, acc);
        }
    }
    seg_store_partial_row<C>(acc, red, part + (long)blockIdx.x * SEG_K);
}

// partials [B][blocks_per_b][SEG_K] -> stats [B][SEG_K], then the batch-wide row stats[B][SEG_K] (the samples' rows added in
// index order), then the loss value: all in f64, fixed order
__global__ void k_seg_loss_finalize(const float* __restrict__ part, int B, int blocks_per_b, int C, SegOpt o,
                                    float* __restrict__ stats, float* __restrict__ loss) {
    const double region = seg_finalize_region(part, B, blocks_per_b, C, o, stats);
    if (threadIdx.x == 0) {
        const double W = stats[B * SEG_K + SEG_W], num = stats[B * SEG_K + SEG_NUM];
        const double voxel = W > 0.0 ? num / W : 0.0;
        loss[0] = (float)((double)o.lam_r * region + (double)o.lam_v * voxel);
    }
}

// pass 2: dz = gscale * d loss / dz (f32, same layout as z), every element stored once; VEC as in pass 1 (a group of four
// voxels never straddles two samples)
template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_seg_loss_grad(const float* __restrict__ z, const float* __restrict__ y, long vol, int B,
                                                       SegOpt o, const float* __restrict__ cw, const float* __restrict__ stats,
                                                       const float* __restrict__ gscale, float* __restrict__ dz) {
    const long total = (long)B * vol;
    const float up = gscale ? gscale[0] : 1.f;                 // the incoming d(total)/d(loss): folded in here, not a second pass
    const float ncls = (float)(C - o.c0);
    const float wd = o.lam_r / ((o.batch ? 1.f : (float)B) * ncls);
    const float W = stats[B * SEG_K + SEG_W];
    const float wv = W > 0.f ? o.lam_v / W : 0.f;
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
            float qa[C], qb[C];
            seg_region_consts<C>(stats + b * SEG_K, o, wd, qa, qb);
            seg_voxel_grad<C>(zb, y4.x, wt, o, wv, up, qa, qb, gb);
            seg_voxel_grad<C>(zb + C, y4.y, wt, o, wv, up, qa, qb, gb + C);
            seg_voxel_grad<C>(zb + 2 * C, y4.z, wt, o, wv, up, qa, qb, gb + 2 * C);
            seg_voxel_grad<C>(zb + 3 * C, y4.w, wt, o, wv, up, qa, qb, gb + 3 * C);
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
            seg_voxel_grad<C>(zz, y[i], wt, o, wv, up, qa, qb, gz);
#pragma unroll
            for (int c = 0; c < C; ++c) dz[i * C + c] = gz[c];
        }
    }
}

// partial rows [B][bpb], the samples' rows [B], the batch-wide row
extern "C" size_t mivp_seg_loss_ws(int32_t B, int64_t vol) {
    return seg_region_ws(B, vol);
}

static int seg_loss_run(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, const SegOpt& o,
                        const float* class_weights, float* workspace, float* loss, const float* gscale, float* dlogits,
                        bool do_loss, mivp_stream_t stream) {
    const long bpb = seg_bpb(vol);
    float* part = workspace;
    float* stats = workspace + (long)B * bpb * SEG_K;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vol % 4 == 0;                             // 16-byte loads of four voxels
    if (do_loss) {
#define S_STATS1(CC, VV) hipLaunchKernelGGL((k_seg_loss_stats<CC, VV>), dim3((unsigned)(B * bpb)), dim3(256), 0, st, logits, target, \
                                            (long)vol, o, class_weights, (int)bpb, part)
#define S_STATS(CC) do { if (vec) S_STATS1(CC, true); else S_STATS1(CC, false); } while (0)
        SEG_C_SWITCH(S_STATS)
#undef S_STATS
#undef S_STATS1
        int rc = mivp_check_launch("seg_loss_stats");
        if (rc) return rc;
        hipLaunchKernelGGL(k_seg_loss_finalize, dim3(1), dim3(1024), 0, st, part, (int)B, (int)bpb, (int)C, o, stats, loss);
        rc = mivp_check_launch("seg_loss_finalize");
        if (rc) return rc;
    }
    if (!dlogits) return MIVP_OK;
    const long total = vec ? (long)B * vol / 4 : (long)B * vol;
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
#define S_GRAD1(CC, VV) hipLaunchKernelGGL((k_seg_loss_grad<CC, VV>), dim3(grid), dim3(256), 0, st, logits, target, (long)vol, \
                                           (int)B, o, class_weights, stats, gscale, dlogits)
#define S_GRAD(CC) do { if (vec) S_GRAD1(CC, true); else S_GRAD1(CC, false); } while (0)
    SEG_C_SWITCH(S_GRAD)
#undef S_GRAD
#undef S_GRAD1
    return mivp_check_launch("seg_loss_grad");
}

extern "C" int mivp_seg_loss(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                             int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                             const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                             float lambda_voxel, float* workspace, float* loss, float* dlogits, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && loss);
    SEG_REQUIRE_OPTIONS();
    return seg_loss_run(logits, target, B, vol, C, o, class_weights, workspace, loss, nullptr, dlogits, true, stream);
}

extern "C" int mivp_seg_loss_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                                  int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                                  const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                                  float lambda_voxel, float* workspace, const float* gscale, float* dlogits,
                                  mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && dlogits);
    SEG_REQUIRE_OPTIONS();
    return seg_loss_run(logits, target, B, vol, C, o, class_weights, workspace, nullptr, gscale, dlogits, false, stream);
}
