// Multi-label targets: R overlapping label GROUPS, one sigmoid channel each (mivp_amd/multilabel.py).
//   member int32 [256]: bits 0..R-1 of entry l = the groups that contain label l, bit 8 = l is a known label
//   a voxel is VALID when its label is an integer in 0..255, known, and not the ignore label; V = the valid voxels, N = |V|
//   t_r = [label in group r], p_r = sigmoid(z_r), s = 1e-5, sums over V of a sample (of the whole batch when `batch`):
//   I_r = sum p_r t_r, P_r = sum p_r, T_r = sum t_r
//   TI_r   = (2 I + s) / (2 I + 2 alpha (P - I) + 2 beta (T - I) + s)
//   region = mean over (b, r) [over r when batch] of 1 - TI_r
//   f_r    = w_r [ t_r pi_r (1 - p_r)^gamma (-log p_r) + (1 - t_r) p_r^gamma (-log(1 - p_r)) ]
//   voxel  = sum_{v in V} sum_r f_r / (R max(N, 1))
//   loss   = lambda_region region + lambda_voxel voxel
// An invalid voxel adds to no sum and gets an exactly zero gradient in all R channels.  log p and log(1 - p) come from
// e = exp(-|z|), log1p(e) and one reciprocal: finite, and with their digits, at |z| = 30.
// The loss reuses the row layout, the partial-row store and the f64 region finalize of csrc/segloss_common.hpp (c0 = 0): no
// atomics, a fixed-order f64 finalize, every dz element stored exactly once.  Decode and the group counts are one streaming
// launch each; the counts use integer atomics only.
#include "segloss_common.hpp"

namespace {
constexpr int ML_KNOWN = 256;                                     // bit 8 of a member entry

struct MlSig { float nlp, nlq, p, q; };                           // -log p, -log(1 - p), p = sigmoid(z), q = 1 - p
MIVP_DEV MlSig ml_sig(float z) {
    const float e = __expf(-fabsf(z)), l = log1pf(e), r = __builtin_amdgcn_rcpf(1.f + e);   // v_rcp_f32: 1 ulp
    MlSig g;
    g.nlp = l - fminf(z, 0.f);
    g.nlq = l - fminf(-z, 0.f);
    g.p = z >= 0.f ? r : e * r;
    g.q = z >= 0.f ? e * r : r;
    return g;
}

// group mask of a label stored as f32, -1 for an invalid voxel (non-integer, outside 0..255, NaN, unknown, or the ignore label)
MIVP_DEV int ml_mask(float yv, const int* mem, const SegOpt& o) {
    const bool in = yv >= 0.f && yv < 256.f && yv == floorf(yv);
    const int m = mem[in ? (int)yv : 0];
    const bool ok = in && (m & ML_KNOWN) && !(o.has_ignore && yv == o.ignore);
    return ok ? (m & 255) : -1;
}

template <int R>
MIVP_DEV void ml_load_weights(const float* __restrict__ gw, const float* __restrict__ pw, float* w, float* wp) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        w[r] = gw ? gw[r] : 1.f;
        wp[r] = w[r] * (pw ? pw[r] : 1.f);                         // w_r pi_r: the weight of a positive
    }
}

template <int R>
MIVP_DEV void ml_voxel_stats(const float* zz, float yv, const int* mem, const float* w, const float* wp, const SegOpt& o,
                             float* acc) {
    const int mask = ml_mask(yv, mem, o);
    const bool valid = mask >= 0;
    float f = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const MlSig g = ml_sig(zz[r]);
        const bool t = valid && ((mask >> r) & 1);
        acc[3 * r] += t ? g.p : 0.f;
        acc[3 * r + 1] += valid ? g.p : 0.f;
        acc[3 * r + 2] += t ? 1.f : 0.f;
        if (o.lam_v > 0.f) f += t ? wp[r] * (seg_pow(g.q, o.gamma) * g.nlp) : w[r] * (seg_pow(g.p, o.gamma) * g.nlq);
    }
    acc[SEG_NUM] += valid ? f : 0.f;
    acc[SEG_W] += valid ? 1.f : 0.f;                                // N
}

// gz = up * d loss / dz of one voxel; exact zeros at an invalid voxel.  wv = lambda_voxel / (R max(N, 1))
//   t = 1: d f / dz = w pi (1 - p)^gamma (gamma p log p - (1 - p));   t = 0: d f / dz = w p^gamma (p - gamma (1 - p) log(1 - p))
template <int R>
MIVP_DEV void ml_voxel_grad(const float* zz, float yv, const int* mem, const float* w, const float* wp, const SegOpt& o, float wv,
                            float up, const float* qa, const float* qb, float* gz) {
    const int mask = ml_mask(yv, mem, o);
    const bool valid = mask >= 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const MlSig g = ml_sig(zz[r]);
        const bool t = (mask >> r) & 1;
        float d = g.p * g.q * (qa[r] - (t ? qb[r] : 0.f));          // the region term through the sigmoid
        if (o.lam_v > 0.f) {
            const float df = t ? wp[r] * (seg_pow(g.q, o.gamma) * (-o.gamma * g.p * g.nlp - g.q))
                               : w[r] * (seg_pow(g.p, o.gamma) * (g.p + o.gamma * g.q * g.nlq));
            d += wv * df;
        }
        gz[r] = valid ? up * d : 0.f;
    }
}

MIVP_DEV void ml_stage_member(const int* __restrict__ member, int* mem) {
    mem[threadIdx.x] = member[threadIdx.x];                         // 256 threads, 256 entries
    __syncthreads();
}
}

// pass 1: per-workgroup partial rows [SEG_K] for ONE sample per workgroup row; VEC: four consecutive voxels per thread and
// iteration through 16-byte loads (vol % 4 == 0)
template <int R, bool VEC>
__global__ __launch_bounds__(256) void k_ml_loss_stats(const float* __restrict__ z, const float* __restrict__ y, long vol, SegOpt o,
                                                       const int* __restrict__ member, const float* __restrict__ gw,
                                                       const float* __restrict__ pw, int blocks_per_b, float* __restrict__ part) {
    __shared__ float red[4][SEG_K];
    __shared__ int mem[256];
    ml_stage_member(member, mem);
    const int b = blockIdx.x / blocks_per_b, blk = blockIdx.x % blocks_per_b;
    float w[R], wp[R];
    ml_load_weights<R>(gw, pw, w, wp);
    float acc[SEG_K];
#pragma unroll
    for (int i = 0; i < SEG_K; ++i) acc[i] = 0.f;
    if (VEC) {
        const long nq = vol >> 2;
        for (long q = (long)blk * 256 + threadIdx.x; q < nq; q += (long)blocks_per_b * 256) {
            const long v = (long)b * vol + 4 * q;
            float zb[4 * R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + v * R + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + v);
            ml_voxel_stats<R>(zb, y4.x, mem, w, wp, o, acc);
            ml_voxel_stats<R>(zb + R, y4.y, mem, w, wp, o, acc);
            ml_voxel_stats<R>(zb + 2 * R, y4.z, mem, w, wp, o, acc);
            ml_voxel_stats<R>(zb + 3 * R, y4.w, mem, w, wp, o, acc);
        }
    } else {
        for (long v = (long)blk * 256 + threadIdx.x; v < vol; v += (long)blocks_per_b * 256) {
            const float* zv = z + ((long)b * vol + v) * R;
            float zz[R];
#pragma unroll
            for (int r = 0; r < R; ++r) zz[r] = zv[r];
            ml_voxel_stats<R>(zz, y[(long)b * vol + v], mem, w, wp, o, acc);
        }
    }
    seg_store_partial_row<R>(acc, red, part + (long)blockIdx.x * SEG_K);
}

// pass 2: partial rows -> the samples' rows, the batch-wide row and the value, all in f64 in a fixed order
__global__ void k_ml_loss_finalize(const float* __restrict__ part, int B, int blocks_per_b, int R, SegOpt o,
                                   float* __restrict__ stats, float* __restrict__ loss) {
    const double region = seg_finalize_region(part, B, blocks_per_b, R, o, stats);
    if (threadIdx.x == 0) {
        const double N = stats[B * SEG_K + SEG_W], num = stats[B * SEG_K + SEG_NUM];
        const double voxel = num / ((double)R * (N > 1.0 ? N : 1.0));
        loss[0] = (float)((double)o.lam_r * region + (double)o.lam_v * voxel);
    }
}

// pass 3: dz = gscale * d loss / dz (f32, same layout as z), every element stored once; VEC as in pass 1 (a group of four
// voxels never straddles two samples)
template <int R, bool VEC>
__global__ __launch_bounds__(256) void k_ml_loss_grad(const float* __restrict__ z, const float* __restrict__ y, long vol, int B,
                                                      SegOpt o, const int* __restrict__ member, const float* __restrict__ gw,
                                                      const float* __restrict__ pw, const float* __restrict__ stats,
                                                      const float* __restrict__ gscale, float* __restrict__ dz) {
    __shared__ int mem[256];
    ml_stage_member(member, mem);
    const long total = (long)B * vol;
    const float up = gscale ? gscale[0] : 1.f;
    const float wd = o.lam_r / ((o.batch ? 1.f : (float)B) * (float)R);
    const float N = stats[B * SEG_K + SEG_W];
    const float wv = o.lam_v / ((float)R * fmaxf(N, 1.f));
    float w[R], wp[R];
    ml_load_weights<R>(gw, pw, w, wp);
    if (VEC) {
        const long nq = total >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
            const long i = 4 * q;
            const int b = o.batch ? B : (int)(i / vol);
            float zb[4 * R], gb[4 * R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + i * R + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + i);
            float qa[R], qb[R];
            seg_region_consts<R>(stats + b * SEG_K, o, wd, qa, qb);
            ml_voxel_grad<R>(zb, y4.x, mem, w, wp, o, wv, up, qa, qb, gb);
            ml_voxel_grad<R>(zb + R, y4.y, mem, w, wp, o, wv, up, qa, qb, gb + R);
            ml_voxel_grad<R>(zb + 2 * R, y4.z, mem, w, wp, o, wv, up, qa, qb, gb + 2 * R);
            ml_voxel_grad<R>(zb + 3 * R, y4.w, mem, w, wp, o, wv, up, qa, qb, gb + 3 * R);
#pragma unroll
            for (int j = 0; j < R; ++j)
                *reinterpret_cast<float4*>(dz + i * R + 4 * j) = make_float4(gb[4 * j], gb[4 * j + 1], gb[4 * j + 2], gb[4 * j + 3]);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const int b = o.batch ? B : (int)(i / vol);
            float zz[R], gz[R], qa[R], qb[R];
#pragma unroll
            for (int r = 0; r < R; ++r) zz[r] = z[i * R + r];
            seg_region_consts<R>(stats + b * SEG_K, o, wd, qa, qb);
            ml_voxel_grad<R>(zz, y[i], mem, w, wp, o, wv, up, qa, qb, gz);
#pragma unroll
            for (int r = 0; r < R; ++r) dz[i * R + r] = gz[r];
        }
    }
}

#define ML_R_SWITCH(LAUNCH)                                                                          \
    switch (R) {                                                                                     \
        case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; \
        case 5: LAUNCH(5); break; case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(8); break; \
    }

// the checks of mivp_multilabel_loss and mivp_multilabel_loss_grad on their shared arguments, then the options as the
// kernels take them (SEG_REQUIRE_OPTIONS with 1 <= R and no background switch)
#define ML_REQUIRE_OPTIONS()                                                                                                   \
    MIVP_REQUIRE(B > 0 && vol > 0 && R >= 1 && R <= SEG_MAXC && member);                                                       \
    MIVP_REQUIRE((long)B * seg_bpb(vol) < (1L << 31) && (long)B * SEG_K < (1L << 31));                                         \
    MIVP_REQUIRE(alpha >= 0.f && beta >= 0.f && alpha <= 3.0e38f && beta <= 3.0e38f);                                         \
    MIVP_REQUIRE(focal_gamma == 0.f || (focal_gamma >= 1.f && focal_gamma <= 3.0e38f));                                        \
    MIVP_REQUIRE(lambda_region >= 0.f && lambda_voxel >= 0.f && lambda_region <= 3.0e38f && lambda_voxel <= 3.0e38f);         \
    MIVP_REQUIRE(lambda_region > 0.f || lambda_voxel > 0.f);                                                                   \
    const SegOpt o = {0, batch ? 1 : 0, has_ignore ? 1 : 0, (float)ignore_index, alpha, beta, focal_gamma, lambda_region,      \
                      lambda_voxel}

extern "C" size_t mivp_multilabel_loss_ws(int32_t B, int64_t vol) {
    return seg_region_ws(B, vol);
}

static int ml_loss_run(const float* logits, const float* target, int32_t B, int64_t vol, int32_t R, const int32_t* member,
                       const SegOpt& o, const float* gw, const float* pw, float* workspace, float* loss, const float* gscale,
                       float* dlogits, bool do_loss, mivp_stream_t stream) {
    const long bpb = seg_bpb(vol);
    float* part = workspace;
    float* stats = workspace + (long)B * bpb * SEG_K;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vol % 4 == 0;                             // 16-byte loads of four voxels
    if (do_loss) {
#define M_STATS1(RR, VV) hipLaunchKernelGGL((k_ml_loss_stats<RR, VV>), dim3((unsigned)(B * bpb)), dim3(256), 0, st, logits, target, \
                                            (long)vol, o, member, gw, pw, (int)bpb, part)
#define M_STATS(RR) do { if (vec) M_STATS1(RR, true); else M_STATS1(RR, false); } while (0)
        ML_R_SWITCH(M_STATS)
#undef M_STATS
#undef M_STATS1
        int rc = mivp_check_launch("multilabel_loss_stats");
        if (rc) return rc;
        hipLaunchKernelGGL(k_ml_loss_finalize, dim3(1), dim3(1024), 0, st, part, (int)B, (int)bpb, (int)R, o, stats, loss);
        rc = mivp_check_launch("multilabel_loss_finalize");
        if (rc) return rc;
    }
    if (!dlogits) return MIVP_OK;
    const long total = vec ? (long)B * vol / 4 : (long)B * vol;
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
#define M_GRAD1(RR, VV) hipLaunchKernelGGL((k_ml_loss_grad<RR, VV>), dim3(grid), dim3(256), 0, st, logits, target, (long)vol, \
                                           (int)B, o, member, gw, pw, stats, gscale, dlogits)
#define M_GRAD(RR) do { if (vec) M_GRAD1(RR, true); else M_GRAD1(RR, false); } while (0)
    ML_R_SWITCH(M_GRAD)
#undef M_GRAD
#undef M_GRAD1
    return mivp_check_launch("multilabel_loss_grad");
}

extern "C" int mivp_multilabel_loss(const float* logits, const float* target, int32_t B, int64_t vol, int32_t R,
                                    const int32_t* member, int32_t batch, float alpha, float beta, float focal_gamma,
                                    const float* group_weights, const float* pos_weight, int32_t ignore_index,
                                    int32_t has_ignore, float lambda_region, float lambda_voxel, float* workspace, float* loss,
                                    float* dlogits, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && loss);
    ML_REQUIRE_OPTIONS();
    return ml_loss_run(logits, target, B, vol, R, member, o, group_weights, pos_weight, workspace, loss, nullptr, dlogits, true,
                       stream);
}

extern "C" int mivp_multilabel_loss_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t R,
                                         const int32_t* member, int32_t batch, float alpha, float beta, float focal_gamma,
                                         const float* group_weights, const float* pos_weight, int32_t ignore_index,
                                         int32_t has_ignore, float lambda_region, float lambda_voxel, float* workspace,
                                         const float* gscale, float* dlogits, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && dlogits);
    ML_REQUIRE_OPTIONS();
    return ml_loss_run(logits, target, B, vol, R, member, o, group_weights, pos_weight, workspace, nullptr, gscale, dlogits,
                       false, stream);
}

// ---------------------------------------------------------------------------------------------
// decode: bits = sum_r [z_r > tau_r] << r, labels = lut[bits], probs = sigmoid(z); one launch, blockIdx.y = sample
// ---------------------------------------------------------------------------------------------
namespace {
MIVP_DEV float ml_sigmoid(float z) {                               // the map a user reads: exp and the division at full precision
    const float e = expf(-fabsf(z)), r = 1.f / (1.f + e);
    return z >= 0.f ? r : e * r;
}
}

// VEC: four consecutive voxels per thread (vol % 4 == 0 and every pointer aligned to its vector): 16-byte loads, the two
// byte maps as one 32-bit store each, the probability planes as 16-byte stores
template <int R, bool VEC>
__global__ __launch_bounds__(256) void k_ml_decode(const float* __restrict__ z, long vol, int channels_last,
                                                   const float* __restrict__ thr, const uint8_t* __restrict__ lut,
                                                   uint8_t* __restrict__ labels, uint8_t* __restrict__ bits,
                                                   float* __restrict__ probs) {
    __shared__ uint8_t slut[1 << R];
    for (int i = threadIdx.x; i < (1 << R); i += 256) slut[i] = lut[i];
    __syncthreads();
    float tau[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tau[r] = thr[r];
    const long b = blockIdx.y;
    const float* zb = z + b * R * vol;
    if (VEC) {
        const long nq = vol >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
            const long v = 4 * q;
            float zz[4][R];
            if (channels_last) {
                float buf[4 * R];
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const float4 t4 = *reinterpret_cast<const float4*>(zb + v * R + 4 * j);
                    buf[4 * j] = t4.x; buf[4 * j + 1] = t4.y; buf[4 * j + 2] = t4.z; buf[4 * j + 3] = t4.w;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int r = 0; r < R; ++r) zz[k][r] = buf[k * R + r];
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 t4 = *reinterpret_cast<const float4*>(zb + (long)r * vol + v);
                    zz[0][r] = t4.x; zz[1][r] = t4.y; zz[2][r] = t4.z; zz[3][r] = t4.w;
                }
            }
            unsigned pb = 0u, pl = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned m = 0u;
#pragma unroll
                for (int r = 0; r < R; ++r) m |= (zz[k][r] > tau[r] ? 1u : 0u) << r;
                pb |= m << (8 * k);
                pl |= (unsigned)slut[m] << (8 * k);
            }
            if (labels) *reinterpret_cast<unsigned*>(labels + b * vol + v) = pl;
            if (bits) *reinterpret_cast<unsigned*>(bits + b * vol + v) = pb;
            if (probs) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    *reinterpret_cast<float4*>(probs + (b * R + r) * vol + v) =
                        make_float4(ml_sigmoid(zz[0][r]), ml_sigmoid(zz[1][r]), ml_sigmoid(zz[2][r]), ml_sigmoid(zz[3][r]));
            }
        }
    } else {
        for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < vol; v += (long)gridDim.x * 256) {
            unsigned m = 0u;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float x = channels_last ? zb[v * R + r] : zb[(long)r * vol + v];
                m |= (x > tau[r] ? 1u : 0u) << r;
                if (probs) probs[(b * R + r) * vol + v] = ml_sigmoid(x);
            }
            if (labels) labels[b * vol + v] = slut[m];
            if (bits) bits[b * vol + v] = (uint8_t)m;
        }
    }
}

extern "C" int mivp_multilabel_decode(const float* logits, int32_t B, int64_t vol, int32_t R, int32_t channels_last,
                                      const float* thresholds, const uint8_t* lut, uint8_t* labels, uint8_t* bits, float* probs,
                                      mivp_stream_t stream) {
    MIVP_REQUIRE(logits && thresholds && lut && (labels || bits || probs));
    MIVP_REQUIRE(B > 0 && B <= 65535 && vol > 0 && R >= 1 && R <= SEG_MAXC && (long)B * vol * R < (1L << 40));
    const bool vec = vol % 4 == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)bits & 3) == 0 &&
                     ((uintptr_t)probs & 15) == 0;
    const long items = vec ? vol / 4 : vol;
    const unsigned grid = (unsigned)((items + 255) / 256 > 4096 ? 4096 : (items + 255) / 256);
#define M_DEC1(RR, VV) hipLaunchKernelGGL((k_ml_decode<RR, VV>), dim3(grid, (unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, \
                                          (long)vol, (int)channels_last, thresholds, lut, labels, bits, probs)
#define M_DEC(RR) do { if (vec) M_DEC1(RR, true); else M_DEC1(RR, false); } while (0)
    ML_R_SWITCH(M_DEC)
#undef M_DEC
#undef M_DEC1
    return mivp_check_launch("multilabel_decode");
}

// ---------------------------------------------------------------------------------------------
// group counts: counts[r] += (|pred_r & t_r|, |pred_r|, |t_r|) over the valid voxels.  Every wave ballots the three
// predicates of a group and adds the popcounts to a wave-uniform register; one lane per wave adds them into an LDS table,
// and the workgroup issues one set of 64-bit integer atomics
// ---------------------------------------------------------------------------------------------
namespace {
template <typename T> MIVP_DEV int ml_entry(T v, const int* mem);
template <> MIVP_DEV int ml_entry<uint8_t>(uint8_t v, const int* mem) { return mem[v]; }
template <> MIVP_DEV int ml_entry<float>(float v, const int* mem) {
    const bool in = v >= 0.f && v < 256.f && v == floorf(v);
    const int m = mem[in ? (int)v : 0];
    return in ? m : 0;
}

template <typename TP, typename TT>
__global__ __launch_bounds__(256) void k_group_counts(const TP* __restrict__ pred, int pred_is_labels, const TT* __restrict__ target,
                                                      long nvox, int R, const int* __restrict__ member, int has_ignore,
                                                      int ignore, unsigned long long* __restrict__ counts) {
    __shared__ int mem[256];
    __shared__ unsigned int sm[SEG_MAXC * 3];
    if (threadIdx.x < SEG_MAXC * 3) sm[threadIdx.x] = 0u;
    ml_stage_member(member, mem);                                  // ends behind a barrier
    unsigned int cnt[SEG_MAXC * 3];
#pragma unroll
    for (int i = 0; i < SEG_MAXC * 3; ++i) cnt[i] = 0u;
    // every lane of a wave runs the same number of iterations: the ballots see the whole wave
    for (long base = (long)blockIdx.x * 256; base < nvox; base += (long)gridDim.x * 256) {
        const long v = base + threadIdx.x;
        const bool in = v < nvox;
        const long vc = in ? v : nvox - 1;
        const TT tv = target[vc];
        const TP pv = pred[vc];
        const int te = ml_entry<TT>(tv, mem);
        const bool valid = in && (te & ML_KNOWN) && !(has_ignore && (float)tv == (float)ignore);
        const int tm = valid ? (te & 255) : 0;
        const int pm = valid ? ((pred_is_labels ? ml_entry<TP>(pv, mem) : (int)pv) & 255) : 0;
#pragma unroll
        for (int r = 0; r < SEG_MAXC; ++r) {
            if (r < R) {
                const bool p = (pm >> r) & 1, t = (tm >> r) & 1;
                cnt[3 * r] += (unsigned)__popcll(__ballot(p && t));
                cnt[3 * r + 1] += (unsigned)__popcll(__ballot(p));
                cnt[3 * r + 2] += (unsigned)__popcll(__ballot(t));
            }
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < SEG_MAXC * 3; ++i)
            if (i < 3 * R && cnt[i]) atomicAdd(&sm[i], cnt[i]);
    }
    __syncthreads();
    if (threadIdx.x < 3 * R && sm[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)sm[threadIdx.x]);
}
}  // namespace

extern "C" int mivp_group_counts(const void* pred, int32_t pred_dtype, int32_t pred_is_labels, const void* target,
                                 int32_t target_dtype, int64_t nvox, int32_t R, const int32_t* member, int32_t ignore_index,
                                 int32_t has_ignore, int64_t* counts, mivp_stream_t stream) {
    MIVP_REQUIRE(pred && target && member && counts && nvox > 0 && nvox < (1L << 31) && R >= 1 && R <= SEG_MAXC);
    MIVP_REQUIRE((pred_dtype == 0 || pred_dtype == 3) && (target_dtype == 0 || target_dtype == 3));
    MIVP_REQUIRE(pred_is_labels || pred_dtype == 0);               // a bits map is uint8
    const unsigned grid = (unsigned)((nvox + 255) / 256 > 2048 ? 2048 : (nvox + 255) / 256);
#define M_CNT(TP, TT) hipLaunchKernelGGL((k_group_counts<TP, TT>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const TP*)pred, \
                                         (int)pred_is_labels, (const TT*)target, (long)nvox, (int)R, member, (int)has_ignore,    \
                                         (int)ignore_index, (unsigned long long*)counts)
    if (pred_dtype == 0 && target_dtype == 0) M_CNT(uint8_t, uint8_t);
    else if (pred_dtype == 0) M_CNT(uint8_t, float);
    else if (target_dtype == 0) M_CNT(float, uint8_t);
    else M_CNT(float, float);
#undef M_CNT
    return mivp_check_launch("group_counts");
}
