// Per-voxel helpers of the fused segmentation losses: shared by csrc/segloss.hip (Tversky + weighted / focal cross-entropy,
// DESIGN 4.33) and csrc/segtopk.hip (the same region term + top-k cross-entropy).
//   a voxel is VALID when its label is an integer in [0, C) and not the ignore label; an invalid voxel adds to no sum and
//   gets an exactly zero gradient.
// 1 - p_y is formed as sum_{c != y} e_c / den and log p_y as z_y - max - log den: both keep their digits when the logits
// saturate.
#pragma once
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

// the same rule at a run-time C (csrc/distmap.hip, csrc/hausdorff.hip: one kernel for every class count)
MIVP_DEV int seg_class_rt(float yv, int C, int has_ignore, float ignore) {
    const bool ok = yv >= 0.f && yv < (float)C && yv == floorf(yv) && !(has_ignore && yv == ignore);
    return ok ? (int)yv : -1;
}

// om^g for g == 0 or g >= 1 (om = 1 - p_y in [0, 1]); the exponents in common use take no transcendental
MIVP_DEV float seg_pow(float om, float g) {
    if (g == 0.f) return 1.f;
    if (g == 1.f) return om;
    if (g == 2.f) return om * om;
    return om > 0.f ? __expf(g * __logf(om)) : 0.f;
}

// everything the passes need from one voxel's softmax; the selects over c never index a table with the label
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

// the (I, P, T) columns of one voxel
template <int C>
MIVP_DEV void seg_voxel_region_stats(const SegVoxel<C>& v, const SegOpt& o, float* acc) {
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

// gz = up * d loss / dz of one voxel; exact zeros at an invalid voxel.  wv = the weight of this voxel's cross-entropy term
// without w[y]: lambda_voxel / W for the weighted mean (0 when W == 0), lambda_voxel s_v / k for the top-k mean
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

// wave sums of the columns of a thread's row -> red[wave][SEG_K] -> one partial row, the four waves added in a fixed order
template <int C>
MIVP_DEV void seg_store_partial_row(const float* acc, float (*red)[SEG_K], float* __restrict__ row) {
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
        row[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// partials [B][blocks_per_b][SEG_K] -> stats [B][SEG_K], then the batch-wide row stats[B][SEG_K] (the samples' rows added in
// index order), then the region value on thread 0: all in f64, fixed order.  Ends behind a barrier: every thread may read stats.
MIVP_DEV double seg_finalize_region(const float* __restrict__ part, int B, int blocks_per_b, int C, const SegOpt& o,
                                    float* __restrict__ stats) {
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
    double region = 0.0;
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
        region = d / ((double)rows * (double)(C - o.c0));
    }
    return region;
}

inline long seg_bpb(int64_t vol) {
    long bpb = (vol + 256 * 4 - 1) / (256 * 4);
    if (bpb > SEG_MAX_BPB) bpb = SEG_MAX_BPB;
    if (bpb < 1) bpb = 1;
    return bpb;
}

// floats of the region part of a workspace: partial rows [B][bpb], the samples' rows [B], the batch-wide row
inline size_t seg_region_ws(int32_t B, int64_t vol) { return ((size_t)B * (seg_bpb(vol) + 1) + 1) * SEG_K; }
}

#define SEG_C_SWITCH(LAUNCH)                                                                         \
    switch (C) {                                                                                     \
        case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; case 5: LAUNCH(5); break; \
        case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(8); break;              \
    }

// the checks both families of entries make on their shared arguments, then the options as the kernels take them
#define SEG_REQUIRE_OPTIONS()                                                                                                  \
    MIVP_REQUIRE(B > 0 && vol > 0 && C >= 2 && C <= SEG_MAXC);                                                                 \
    MIVP_REQUIRE((long)B * seg_bpb(vol) < (1L << 31) && (long)B * SEG_K < (1L << 31));                                         \
    MIVP_REQUIRE(alpha >= 0.f && beta >= 0.f && alpha <= 3.0e38f && beta <= 3.0e38f);                                         \
    MIVP_REQUIRE(focal_gamma == 0.f || (focal_gamma >= 1.f && focal_gamma <= 3.0e38f));                                        \
    MIVP_REQUIRE(lambda_region >= 0.f && lambda_voxel >= 0.f && lambda_region <= 3.0e38f && lambda_voxel <= 3.0e38f);         \
    MIVP_REQUIRE(lambda_region > 0.f || lambda_voxel > 0.f);                                                                   \
    const SegOpt o = {include_background ? 0 : 1, batch ? 1 : 0, has_ignore ? 1 : 0, (float)ignore_index, alpha, beta,         \
                      focal_gamma, lambda_region, lambda_voxel}
