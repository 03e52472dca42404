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
#include "common.hpp"

namespace {
constexpr int SEG_MAXC = 8;
constexpr int SEG_K = 3 * SEG_MAXC + 2;        // columns of a row: (I, P, T) x 8 | voxel numerator | voxel weight sum
constexpr int SEG_NUM = 3 * SEG_MAXC, SEG_W = 3 * SEG_MAXC + 1;
constexpr int SEG_MAX_BPB = 256;               // partial rows per sample (csrc/loss.hip: LOSS_MAX_BPB)
constexpr float SEG_SMOOTH = 1e-5f;

struct SegOpt {
    int c0, batch, has_ignore;
    float ignore, alpha, beta, gamma, lam_r, lam_v;
};

// class of a label, -1 for an invalid voxel (non-integer, out of range, NaN, or the ignore label)
template <int C>
MIVP_DEV int seg_class(float yv, const SegOpt& o) {
    const bool ok = yv >= 0.f && yv < (float)C && yv == floorf(yv) && !(o.has_ignore && yv == o.ignore);
    return ok ? (int)yv : -1;
}

// om^g for g == 0 or g >= 1 (om = 1 - p_y in [0, 1]); the exponents in common use take no transcendental
MIVP_DEV float seg_pow(float om, float g) {
    if (g == 0.f) return 1.f;
    if (g == 1.f) return om;
    if (g == 2.f) return om * om;
    return om > 0.f ? __expf(g * __logf(om)) : 0.f;
}

// everything the two passes need from one voxel's softmax; the selects over c never index a table with the label
template <int C>
struct SegVoxel {
    float p[C], py, om, logp, wy;
    int cls;
    MIVP_DEV SegVoxel(const float* zz, float yv, const float* wt, const SegOpt& o) {
        cls = seg_class<C>(yv, o);
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, zz[c]);
        float den = 0.f, ey = 0.f, eo = 0.f, zy = mx;
        wy = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            p[c] = __expf(zz[c] - mx);
            den += p[c];
            const bool hit = c == cls;
            ey = hit ? p[c] : ey;
            eo += hit ? 0.f : p[c];
            zy = hit ? zz[c] : zy;
            wy = hit ? wt[c] : wy;
        }
        const float inv_den = __builtin_amdgcn_rcpf(den);
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] *= inv_den;
        py = ey * inv_den;
        om = eo * inv_den;
        logp = (zy - mx) - __logf(den);
    }
};

template <int C>
MIVP_DEV void seg_voxel_stats(const float* zz, float yv, const float* wt, const SegOpt& o, float* acc) {
    const SegVoxel<C> v(zz, yv, wt, o);
    const bool valid = v.cls >= 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c >= o.c0) {
            const bool hit = c == v.cls;
            acc[3 * c] += hit ? v.p[c] : 0.f;
            acc[3 * c + 1] += valid ? v.p[c] : 0.f;
            acc[3 * c + 2] += hit ? 1.f : 0.f;
        }
    }
    if (o.lam_v > 0.f) {                                           // wy is 0 at an invalid voxel
        acc[SEG_NUM] -= v.wy * (seg_pow(v.om, o.gamma) * v.logp);
        acc[SEG_W] += v.wy;
    }
}

// per-class constants of the region gradient, lambda_region folded in: d(lambda_region region)/dp_c = qa[c] - (c == cls) qb[c]
template <int C>
MIVP_DEV void seg_region_consts(const float* __restrict__ st, const SegOpt& o, float wd, float* qa, float* qb) {
    const float gam = 1.f - o.alpha - o.beta;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        qa[c] = 0.f; qb[c] = 0.f;
        if (c >= o.c0) {
            const float I = st[3 * c], P = st[3 * c + 1], T = st[3 * c + 2];
            const float Nn = 2.f * I + SEG_SMOOTH;
            const float Dn = 2.f * I + 2.f * o.alpha * (P - I) + 2.f * o.beta * (T - I) + SEG_SMOOTH;
            const float r = Nn / (Dn * Dn);
            qa[c] = wd * (2.f * o.alpha * r);
            qb[c] = wd * (2.f / Dn - 2.f * gam * r);
        }
    }
}

// gz = up * d loss / dz of one voxel; exact zeros at an invalid voxel.  wv = lambda_voxel / W (0 when W == 0)
template <int C>
MIVP_DEV void seg_voxel_grad(const float* zz, float yv, const float* wt, const SegOpt& o, float wv, float up, const float* qa,
                             const float* qb, float* gz) {
    const SegVoxel<C> v(zz, yv, wt, o);
    float q[C], pq = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        q[c] = qa[c] - ((c == v.cls) ? qb[c] : 0.f);
        pq += v.p[c] * q[c];
    }
    // f(p) = -(1 - p)^gamma log p:  f'(p) p = gamma p (1 - p)^(gamma - 1) log p - (1 - p)^gamma
    float fp = -1.f;
    if (o.gamma != 0.f) {
        const float pm1 = seg_pow(v.om, o.gamma - 1.f);
        fp = o.gamma * v.py * pm1 * v.logp - pm1 * v.om;
    }
    const float coef = wv * v.wy * fp;
    const bool valid = v.cls >= 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float g = v.p[c] * (q[c] - pq);                                       // through the softmax
        g += coef * ((c == v.cls) ? v.om : -v.p[c]);                          // delta_cy - p_c, with 1 - p_y as a sum
        gz[c] = valid ? up * g : 0.f;
    }
}

template <int C>
MIVP_DEV void seg_load_weights(const float* __restrict__ cw, float* wt) {
#pragma unroll
    for (int c = 0; c < C; ++c) wt[c] = cw ? cw[c] : 1.f;
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < SEG_K; ++i) {
        float vsum = 0.f;
        if (i < 3 * C || i >= SEG_NUM) {                          // the other columns are never touched: they stay zero
            vsum = acc[i];
            for (int s = 32; s > 0; s >>= 1) vsum += __shfl_xor(vsum, s);
        }
        if (lane == 0) red[wave][i] = vsum;
    }
    __syncthreads();
    if (threadIdx.x < SEG_K) {
        const int i = threadIdx.x;
        part[(long)blockIdx.x * SEG_K + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// partials [B][blocks_per_b][SEG_K] -> stats [B][SEG_K], then the batch-wide row stats[B][SEG_K] (the samples' rows added in
// index order), then the loss value: all in f64, fixed order
__global__ void k_seg_loss_finalize(const float* __restrict__ part, int B, int blocks_per_b, int C, SegOpt o,
                                    float* __restrict__ stats, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    for (int ii = wv; ii < B * SEG_K; ii += nwv) {                // one wave per (b, k) sum
        const int b = ii / SEG_K, k = ii - b * SEG_K;
        double s = 0.0;
        for (int j = lane; j < blocks_per_b; j += 64) s += (double)part[((long)b * blocks_per_b + j) * SEG_K + k];
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        if (lane == 0) stats[ii] = (float)s;
    }
    __syncthreads();
    if (threadIdx.x < SEG_K) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += (double)stats[b * SEG_K + threadIdx.x];
        stats[B * SEG_K + threadIdx.x] = (float)s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sm = (double)SEG_SMOOTH, al = (double)o.alpha, be = (double)o.beta;
        const int rows = o.batch ? 1 : B;
        double d = 0.0;
        for (int r = 0; r < rows; ++r) {
            const float* st = stats + (o.batch ? B : r) * SEG_K;
            for (int c = o.c0; c < C; ++c) {
                const double I = st[3 * c], P = st[3 * c + 1], T = st[3 * c + 2];
                d += 1.0 - (2.0 * I + sm) / (2.0 * I + 2.0 * al * (P - I) + 2.0 * be * (T - I) + sm);
            }
        }
        const double region = d / ((double)rows * (double)(C - o.c0));
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

static long seg_bpb(int64_t vol) {
    long bpb = (vol + 256 * 4 - 1) / (256 * 4);
    if (bpb > SEG_MAX_BPB) bpb = SEG_MAX_BPB;
    if (bpb < 1) bpb = 1;
    return bpb;
}

// partial rows [B][bpb], the samples' rows [B], the batch-wide row
extern "C" size_t mivp_seg_loss_ws(int32_t B, int64_t vol) {
    return ((size_t)B * (seg_bpb(vol) + 1) + 1) * SEG_K;
}

static int seg_loss_run(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, const SegOpt& o,
                        const float* class_weights, float* workspace, float* loss, const float* gscale, float* dlogits,
                        bool do_loss, mivp_stream_t stream) {
    const long bpb = seg_bpb(vol);
    float* part = workspace;
    float* stats = workspace + (long)B * bpb * SEG_K;
    hipStream_t st = (hipStream_t)stream;
#define SEG_C_SWITCH(LAUNCH)                                                                         \
    switch (C) {                                                                                     \
        case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; case 5: LAUNCH(5); break; \
        case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(8); break;              \
    }
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
#undef SEG_C_SWITCH
    return mivp_check_launch("seg_loss_grad");
}

#define SEG_REQUIRE_OPTIONS()                                                                                                  \
    MIVP_REQUIRE(B > 0 && vol > 0 && C >= 2 && C <= SEG_MAXC);                                                                 \
    MIVP_REQUIRE((long)B * seg_bpb(vol) < (1L << 31) && (long)B * SEG_K < (1L << 31));                                         \
    MIVP_REQUIRE(alpha >= 0.f && beta >= 0.f && alpha <= 3.0e38f && beta <= 3.0e38f);                                         \
    MIVP_REQUIRE(focal_gamma == 0.f || (focal_gamma >= 1.f && focal_gamma <= 3.0e38f));                                        \
    MIVP_REQUIRE(lambda_region >= 0.f && lambda_voxel >= 0.f && lambda_region <= 3.0e38f && lambda_voxel <= 3.0e38f);         \
    MIVP_REQUIRE(lambda_region > 0.f || lambda_voxel > 0.f);                                                                   \
    const SegOpt o = {include_background ? 0 : 1, batch ? 1 : 0, has_ignore ? 1 : 0, (float)ignore_index, alpha, beta,         \
                      focal_gamma, lambda_region, lambda_voxel}

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
