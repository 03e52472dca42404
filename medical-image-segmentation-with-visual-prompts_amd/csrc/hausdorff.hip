// Hausdorff distance-transform loss term (Karimi & Salcudean, IEEE TMI 2019, "HD_DT") with the distance fields of the hard
// prediction and of the labels built on the device, per step (mivp_amd/losses.py hausdorff_weight_maps /
// hausdorff_dt_loss / HausdorffDTLoss).
//
// 1. mivp_hausdorff_maps: logits f32 [B][vol][C] + target f32 [B][H][W][D] -> wmap f32 [B][K][H][W][D], K = C - c0.  Per (b, c)
//    two masks: P = {argmax_j z_j == c} (comparisons on the logits alone, the lowest index among exact maxima, at every voxel)
//    and G = {label == c} (the rule of mivp_distmap_signed: a label that is no class is in no G).  field(M)(v) = the distance
//    from v to the nearest voxel on the other side of M (to the complement inside M, to M outside), 0 everywhere in (b, c)
//    when M is empty or the whole sample;  wmap = field(P)^alpha + field(G)^alpha.  Four launches whatever B and K are:
//      seed / D   the scheme of k_distmap_d (csrc/distmap.hip), one wave per (source, b, h, w) line: source 0 classifies a
//                 voxel by the argmax of its C logits (fused: no label map of the prediction is written), source 1 by its
//                 label.  Writes the squared fields f32 [2 sources][2 sides][B][K][vol]: side 0 = distance to M, 1 = to not M.
//      W, H       edt_line of csrc/edt_common.hpp, one thread per line, the line index running across all 4 B K fields.
//      closing    per voxel and class the side each mask needs, +inf -> 0 (the side of a degenerate mask), the two squared
//                 fields added (alpha == 2: no root, no pow; exact integers at unit spacing) or powf(d2, alpha / 2) of each.
//    No atomics, nothing read back, every launch unconditional.  Limits: H, W <= 65535 and 4 B K vol < 2^31.
//
// 2. mivp_hausdorff_loss / mivp_hausdorff_loss_grad: with p = softmax_c(z), g_c = [y == c], V the valid voxels of the batch,
//    N = |V|, w = lambda_hausdorff weight[0]:
//      loss = w sum_{v in V} sum_{c >= c0} (p_c - g_c)^2 wmap_c / (K max(N, 1))
//      dz_j = w p_j sum_c p_c (q_j - q_c) / (K max(N, 1)),   q_c = 2 (p_c - g_c) wmap_c for c >= c0, else 0
//    p_y - 1 is formed as -sum_{c != y} e_c / den: it keeps its digits where p_y -> 1.  The passes, the partial rows and the
//    launch geometry are those of the boundary term (csrc/distmap.hip).
#include "edt_common.hpp"
#include "segloss_common.hpp"

namespace {
constexpr int HD_TPB = 256;

// class of the hard prediction: the first maximum of the C logits (a NaN never wins a comparison)
MIVP_DEV int hd_argmax(const float* __restrict__ zv, int C) {
    int best = 0;
    float m = zv[0];
    for (int c = 1; c < C; ++c) {
        const float t = zv[c];
        if (t > m) { m = t; best = c; }
    }
    return best;
}

// seed / D pass.  Wave line wl < 2 B H W: source = wl / (B H W) (0: prediction, 1: target), then the (b, h, w) line.  Lane
// i < 2 K owns the sweep state of pair i = 2 (c - c0) + side, as in k_distmap_d.
__global__ __launch_bounds__(HD_TPB) void k_hausdorff_d(const float* __restrict__ z, const float* __restrict__ y, int B, int C,
                                                        int c0, int has_ignore, float ignore, long lines_per_b, int D, float a,
                                                        int intp, float* __restrict__ fields) {
    const int lane = threadIdx.x & 63;
    const int nch = (D + 63) >> 6;
    const int K = C - c0;
    const long vol = lines_per_b * D;
    const long nlines = (long)B * lines_per_b;
    for (long wl = (long)blockIdx.x * (HD_TPB / 64) + (threadIdx.x >> 6); wl < 2 * nlines; wl += (long)gridDim.x * (HD_TPB / 64)) {
        const int src = wl >= nlines ? 1 : 0;                      // wave-uniform
        const long line = wl - (src ? nlines : 0L);
        const int b = (int)(line / lines_per_b);
        const long off = (line - (long)b * lines_per_b) * D;       // of the line inside its sample
        const long first = line * D;                               // voxel index of the line's start in the batch
        // class of voxel p of the line, -2 beyond its end
        auto cls_at = [&](int p) -> int {
            if (p >= D) return -2;
            return src ? seg_class_rt(y[first + p], C, has_ignore, ignore) : hd_argmax(z + (first + p) * C, C);
        };
        int prev = -EDT_NO_SEED, next = -1;
        for (int k = 0; k < nch; ++k) {
            const int p = 64 * k + lane;
            const int cls = cls_at(p);
            for (int pr = 0; pr < 2 * K; ++pr) {
                const int c = c0 + (pr >> 1), side = pr & 1;
                const unsigned long long m = __ballot(p < D && (side ? cls != c : cls == c));
                const unsigned long long ml = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
                const unsigned long long mr = m & (~0ull << lane);
                const int pv = __shfl(prev, pr);
                int nx = __shfl(next, pr);
                const int left = ml ? 64 * k + 63 - __builtin_clzll(ml) : pv;
                if (!(m >> 63) && nx <= 64 * k + 63) {             // wave-uniform: some lanes need the next seed
                    nx = EDT_NO_SEED;
                    for (int j = k + 1; j < nch; ++j) {
                        const int q = 64 * j + lane;
                        const int cq = cls_at(q);
                        const unsigned long long mm = __ballot(q < D && (side ? cq != c : cq == c));
                        if (mm) { nx = 64 * j + __builtin_ctzll(mm); break; }
                    }
                }
                const int right = mr ? 64 * k + __builtin_ctzll(mr) : nx;
                if (lane == pr) {
                    next = nx;
                    if (m) prev = 64 * k + 63 - __builtin_clzll(m);
                }
                if (p < D)
                    fields[((((long)src * 2 + side) * B + b) * K + (pr >> 1)) * vol + off + p] =
                        edt_d_value(min(p - left, right - p), a, intp);
            }
        }
    }
}

// W / H pass over all fields: line = field * lines_per_field + (outer, inner), inner = d fastest across lanes
template <bool INTP>
__global__ __launch_bounds__(HD_TPB) void k_hausdorff_line(float* __restrict__ fields, long nlines, long lines_per_field, long vol,
                                                           int inner, long outer_stride, long stride, int n, float a,
                                                           int2* __restrict__ stack) {
    const long line = (long)blockIdx.x * HD_TPB + threadIdx.x;
    if (line >= nlines) return;
    const long field = line / lines_per_field, l = line - field * lines_per_field;
    edt_line<INTP>(fields + field * vol + (l / inner) * outer_stride + (l % inner), stride, n, a, stack, nlines, line);
}

// closing: one thread per voxel of the batch, its K classes in turn.  half = alpha / 2; 1: the squared fields as they are
__global__ __launch_bounds__(HD_TPB) void k_hausdorff_close(const float* __restrict__ z, const float* __restrict__ y,
                                                            const float* __restrict__ fields, int B, int C, int c0,
                                                            int has_ignore, float ignore, long vol, float half,
                                                            float* __restrict__ wmap) {
    const int K = C - c0;
    const long total = (long)B * vol;
    const long set = total * K;                                    // floats of one (source, side) set of fields
    for (long i = (long)blockIdx.x * HD_TPB + threadIdx.x; i < total; i += (long)gridDim.x * HD_TPB) {
        const long b = i / vol, v = i - b * vol;
        const int pc = hd_argmax(z + i * C, C);
        const int gc = seg_class_rt(y[i], C, has_ignore, ignore);
        for (int k = 0; k < K; ++k) {
            const long e = (b * K + k) * vol + v;
            float dp = fields[(pc == c0 + k ? set : 0L) + e];
            float dg = fields[2 * set + (gc == c0 + k ? set : 0L) + e];
            dp = isinf(dp) ? 0.f : dp;
            dg = isinf(dg) ? 0.f : dg;
            wmap[e] = half == 1.f ? dp + dg : powf(dp, half) + powf(dg, half);
        }
    }
}

bool hd_dims(const int32_t* dims, int& H, int& W, int& D) {
    H = dims[0]; W = dims[1]; D = dims[2];
    return H >= 1 && W >= 1 && D >= 1 && H <= 65535 && W <= 65535 && (long)H * W * D < (1L << 31);
}

// bytes of the four field sets, rounded so that the stack behind them is 256-byte aligned
size_t hd_field_bytes(long B, long K, long vol) { return ((size_t)(4 * B * K * vol) * sizeof(float) + 255) / 256 * 256; }

// ------------------------------------------------------------------------------------------------- the loss term
constexpr int HD_NUM = 0, HD_CNT = 1, HD_K = 2;                 // columns of a partial row: sum (p - g)^2 wmap, valid voxels

struct HdOpt {
    int c0, has_ignore;
    float ignore;
};

// softmax of one voxel, d[c] = p_c - g_c, and whether the voxel is valid
template <int C>
struct HdVoxel {
    float p[C], d[C];
    bool valid;
    MIVP_DEV HdVoxel(const float* zz, float yv, const HdOpt& o) {
        const int cls = seg_class_rt(yv, C, o.has_ignore, o.ignore);
        valid = cls >= 0;
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
            d[c] = c == cls ? -(eo * inv_den) : p[c];              // p_y - 1 as -(1 - p_y), the sum of the others
        }
    }
};

// wm[c]: wmap of the voxel (0 below c0)
template <int C>
MIVP_DEV void hd_voxel_stats(const float* zz, float yv, const float* wm, const HdOpt& o, float* acc) {
    const HdVoxel<C> v(zz, yv, o);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += (v.d[c] * v.d[c]) * wm[c];
    acc[HD_NUM] += v.valid ? s : 0.f;
    acc[HD_CNT] += v.valid ? 1.f : 0.f;
}

template <int C>
MIVP_DEV void hd_voxel_grad(const float* zz, float yv, const float* wm, const HdOpt& o, float coef, float* gz) {
    const HdVoxel<C> v(zz, yv, o);
    float q[C];
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = 2.f * v.d[c] * wm[c];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += v.p[c] * (q[j] - q[c]);
        gz[j] = v.valid ? coef * (v.p[j] * s) : 0.f;
    }
}

// wmap of voxel v of sample b into wm[C]
template <int C>
MIVP_DEV void hd_load_wmap(const float* __restrict__ wmap, long b, long vol, long v, int c0, float* wm) {
#pragma unroll
    for (int c = 0; c < C; ++c) wm[c] = c >= c0 ? wmap[(b * (C - c0) + (c - c0)) * vol + v] : 0.f;
}

// pass 1: per-workgroup partial rows [HD_K], one sample per workgroup row; VEC: four consecutive voxels per thread and
// iteration through 16-byte loads (vol % 4 == 0)
template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_hausdorff_stats(const float* __restrict__ z, const float* __restrict__ y,
                                                         const float* __restrict__ wmap, long vol, HdOpt o, int blocks_per_b,
                                                         float* __restrict__ part) {
    __shared__ float red[4][HD_K];
    const int b = blockIdx.x / blocks_per_b, blk = blockIdx.x % blocks_per_b;
    float acc[HD_K] = {0.f, 0.f};
    if (VEC) {
        const long nq = vol >> 2;
        for (long q = (long)blk * 256 + threadIdx.x; q < nq; q += (long)blocks_per_b * 256) {
            const long v = (long)b * vol + 4 * q;
            float zb[4 * C], wb[4][C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + v * C + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c >= o.c0) f4 = *reinterpret_cast<const float4*>(wmap + ((long)b * (C - o.c0) + (c - o.c0)) * vol + 4 * q);
                wb[0][c] = f4.x; wb[1][c] = f4.y; wb[2][c] = f4.z; wb[3][c] = f4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + v);
            hd_voxel_stats<C>(zb, y4.x, wb[0], o, acc);
            hd_voxel_stats<C>(zb + C, y4.y, wb[1], o, acc);
            hd_voxel_stats<C>(zb + 2 * C, y4.z, wb[2], o, acc);
            hd_voxel_stats<C>(zb + 3 * C, y4.w, wb[3], o, acc);
        }
    } else {
        for (long v = (long)blk * 256 + threadIdx.x; v < vol; v += (long)blocks_per_b * 256) {
            const float* zv = z + ((long)b * vol + v) * C;
            float zz[C], wm[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = zv[c];
            hd_load_wmap<C>(wmap, b, vol, v, o.c0, wm);
            hd_voxel_stats<C>(zz, y[(long)b * vol + v], wm, o, acc);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < HD_K; ++i) {
        float s = acc[i];
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < HD_K) {
        const int i = threadIdx.x;
        part[(long)blockIdx.x * HD_K + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// one workgroup: partials [nrows][HD_K] -> res = {sum, N, 1 / (K max(N, 1))}, then the value: f64, fixed order
__global__ __launch_bounds__(256) void k_hausdorff_finalize(const float* __restrict__ part, int nrows, int K, float lam,
                                                            const float* __restrict__ weight, float* __restrict__ res,
                                                            float* __restrict__ loss) {
    __shared__ double red[256][HD_K];
    double s[HD_K] = {0.0, 0.0};
    for (int r = threadIdx.x; r < nrows; r += 256) {
        s[0] += (double)part[(long)r * HD_K];
        s[1] += (double)part[(long)r * HD_K + 1];
    }
    red[threadIdx.x][0] = s[0]; red[threadIdx.x][1] = s[1];
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) { red[threadIdx.x][0] += red[threadIdx.x + o][0]; red[threadIdx.x][1] += red[threadIdx.x + o][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double num = red[0][0], N = red[0][1];
        const double w = (double)lam * (weight ? (double)weight[0] : 1.0);
        res[HD_NUM] = (float)num;
        res[HD_CNT] = (float)N;
        res[2] = (float)(1.0 / ((double)K * (N > 1.0 ? N : 1.0)));
        if (loss) loss[0] = (float)(w * num / ((double)K * (N > 1.0 ? N : 1.0)));
    }
}

// pass 2: dz (=, or += with ACC) up w / (K max(N, 1)) d sum / dz; every element once.  The product is rounded before the
// add: with accumulate the result is dz + g in the bits, g the value a plain store would have written.
template <int C, bool VEC, bool ACC>
__global__ __launch_bounds__(256) void k_hausdorff_grad(const float* __restrict__ z, const float* __restrict__ y,
                                                        const float* __restrict__ wmap, long vol, int B, HdOpt o, float lam,
                                                        const float* __restrict__ weight, const float* __restrict__ res,
                                                        const float* __restrict__ gscale, float* __restrict__ dz) {
    const long total = (long)B * vol;
    const float up = gscale ? gscale[0] : 1.f;
    const float coef = up * (lam * (weight ? weight[0] : 1.f)) * res[2];
    if (VEC) {
        const long nq = total >> 2;
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
            const long i = 4 * q;
            const long b = i / vol, v = i - b * vol;
            float zb[4 * C], gb[4 * C], wb[4][C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + i * C + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c >= o.c0) f4 = *reinterpret_cast<const float4*>(wmap + (b * (C - o.c0) + (c - o.c0)) * vol + v);
                wb[0][c] = f4.x; wb[1][c] = f4.y; wb[2][c] = f4.z; wb[3][c] = f4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + i);
            hd_voxel_grad<C>(zb, y4.x, wb[0], o, coef, gb);
            hd_voxel_grad<C>(zb + C, y4.y, wb[1], o, coef, gb + C);
            hd_voxel_grad<C>(zb + 2 * C, y4.z, wb[2], o, coef, gb + 2 * C);
            hd_voxel_grad<C>(zb + 3 * C, y4.w, wb[3], o, coef, gb + 3 * C);
#pragma unroll
            for (int j = 0; j < C; ++j) {
                float4* out = reinterpret_cast<float4*>(dz + i * C + 4 * j);
                float4 g4 = make_float4(gb[4 * j], gb[4 * j + 1], gb[4 * j + 2], gb[4 * j + 3]);
                if (ACC) {
                    const float4 d4 = *out;
                    g4 = make_float4(__fadd_rn(d4.x, g4.x), __fadd_rn(d4.y, g4.y), __fadd_rn(d4.z, g4.z), __fadd_rn(d4.w, g4.w));
                }
                *out = g4;
            }
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const long b = i / vol, v = i - b * vol;
            float zz[C], gz[C], wm[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
            hd_load_wmap<C>(wmap, b, vol, v, o.c0, wm);
            hd_voxel_grad<C>(zz, y[i], wm, o, coef, gz);
#pragma unroll
            for (int c = 0; c < C; ++c) dz[i * C + c] = ACC ? __fadd_rn(dz[i * C + c], gz[c]) : gz[c];
        }
    }
}

int hausdorff_run(const float* logits, const float* target, const float* wmap, int32_t B, int64_t vol, int32_t C, const HdOpt& o,
                  float lam, const float* weight, float* workspace, float* loss, const float* gscale, float* dlogits,
                  int accumulate, bool do_loss, mivp_stream_t stream) {
    const long bpb = seg_bpb(vol);
    float* part = workspace;
    float* res = workspace + (long)B * bpb * HD_K;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vol % 4 == 0;                             // 16-byte loads of four voxels
    if (do_loss) {
#define H_STATS1(CC, VV) hipLaunchKernelGGL((k_hausdorff_stats<CC, VV>), dim3((unsigned)(B * bpb)), dim3(256), 0, st, logits, target, \
                                            wmap, (long)vol, o, (int)bpb, part)
#define H_STATS(CC) do { if (vec) H_STATS1(CC, true); else H_STATS1(CC, false); } while (0)
        SEG_C_SWITCH(H_STATS)
#undef H_STATS
#undef H_STATS1
        int rc = mivp_check_launch("hausdorff_stats");
        if (rc) return rc;
        hipLaunchKernelGGL(k_hausdorff_finalize, dim3(1), dim3(256), 0, st, part, (int)(B * bpb), (int)(C - o.c0), lam, weight, res,
                           loss);
        rc = mivp_check_launch("hausdorff_finalize");
        if (rc) return rc;
    }
    if (!dlogits) return MIVP_OK;
    const long total = vec ? (long)B * vol / 4 : (long)B * vol;
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
#define H_GRAD2(CC, VV, AA) hipLaunchKernelGGL((k_hausdorff_grad<CC, VV, AA>), dim3(grid), dim3(256), 0, st, logits, target, wmap, \
                                               (long)vol, (int)B, o, lam, weight, res, gscale, dlogits)
#define H_GRAD1(CC, VV) do { if (accumulate) H_GRAD2(CC, VV, true); else H_GRAD2(CC, VV, false); } while (0)
#define H_GRAD(CC) do { if (vec) H_GRAD1(CC, true); else H_GRAD1(CC, false); } while (0)
    SEG_C_SWITCH(H_GRAD)
#undef H_GRAD
#undef H_GRAD1
#undef H_GRAD2
    return mivp_check_launch("hausdorff_grad");
}
}  // namespace

#define HD_REQUIRE_OPTIONS()                                                                                  \
    MIVP_REQUIRE(B > 0 && vol > 0 && C >= 2 && C <= SEG_MAXC);                                                \
    MIVP_REQUIRE((long)B * seg_bpb(vol) < (1L << 31));                                                        \
    MIVP_REQUIRE(lambda_hausdorff >= 0.f && lambda_hausdorff <= 3.0e38f);                                     \
    const HdOpt o = {include_background ? 0 : 1, has_ignore ? 1 : 0, (float)ignore_index}

extern "C" size_t mivp_hausdorff_maps_ws(int32_t B, int32_t K, const int32_t* dims) {
    int H, W, D;
    if (!dims || B < 1 || K < 1 || K > SEG_MAXC || !hd_dims(dims, H, W, D)) return 0;
    const long vol = (long)H * W * D;
    if (4L * B * K * vol >= (1L << 31)) return 0;
    return hd_field_bytes(B, K, vol) + (size_t)(4L * B * K * vol) * sizeof(int2);
}

extern "C" int mivp_hausdorff_maps(const float* logits, const float* target, int32_t B, int32_t C, int32_t include_background,
                                   int32_t ignore_index, int32_t has_ignore, const int32_t* dims, const float* spacing,
                                   float alpha, float* wmap, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && dims && spacing && wmap && workspace && B >= 1);
    const int c0 = include_background ? 0 : 1;
    const int K = C - c0;
    MIVP_REQUIRE(C >= 2 && C <= SEG_MAXC);
    int H, W, D;
    MIVP_REQUIRE(hd_dims(dims, H, W, D));                       // H, W <= 65535: the 16-bit sites of the envelope's stack
    const long vol = (long)H * W * D;
    MIVP_REQUIRE(4L * B * K * vol < (1L << 31));
    MIVP_REQUIRE(spacing[0] > 0.f && spacing[1] > 0.f && spacing[2] > 0.f);
    MIVP_REQUIRE(isfinite(spacing[0]) && isfinite(spacing[1]) && isfinite(spacing[2]));
    MIVP_REQUIRE(alpha > 0.f && alpha <= 4.f);
    const bool intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    hipStream_t s = (hipStream_t)stream;
    float* fields = (float*)workspace;
    int2* stack = (int2*)((char*)workspace + hd_field_bytes(B, K, vol));
    const float ig = (float)ignore_index;
    const long lines_d = 2L * B * H * W;
    const unsigned grid_d = (unsigned)((lines_d + 3) / 4 > 16384 ? 16384 : (lines_d + 3) / 4);
    hipLaunchKernelGGL(k_hausdorff_d, dim3(grid_d), dim3(HD_TPB), 0, s, logits, target, (int)B, (int)C, c0, has_ignore ? 1 : 0, ig,
                       (long)H * W, D, spacing[2] * spacing[2], (int)intp, fields);
    int rc = mivp_check_launch("hausdorff_d");
    if (rc != MIVP_OK) return rc;
    // W pass: lines (h, d) of a field, elements w at stride D; H pass: lines (w, d), elements h at stride W * D
    const long nf = 4L * B * K;
    const long lpf_w = (long)H * D, lpf_h = (long)W * D;
    const long lines_w = nf * lpf_w, lines_h = nf * lpf_h;
    const float aw = spacing[1] * spacing[1], ah = spacing[0] * spacing[0];
    const unsigned grid_w = (unsigned)((lines_w + HD_TPB - 1) / HD_TPB), grid_h = (unsigned)((lines_h + HD_TPB - 1) / HD_TPB);
    if (intp) {
        hipLaunchKernelGGL(k_hausdorff_line<true>, dim3(grid_w), dim3(HD_TPB), 0, s, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_hausdorff_line<true>, dim3(grid_h), dim3(HD_TPB), 0, s, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    } else {
        hipLaunchKernelGGL(k_hausdorff_line<false>, dim3(grid_w), dim3(HD_TPB), 0, s, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_hausdorff_line<false>, dim3(grid_h), dim3(HD_TPB), 0, s, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    }
    rc = mivp_check_launch("hausdorff_line");
    if (rc != MIVP_OK) return rc;
    const long total = (long)B * vol;
    const unsigned grid_c = (unsigned)((total + HD_TPB - 1) / HD_TPB > 16384 ? 16384 : (total + HD_TPB - 1) / HD_TPB);
    hipLaunchKernelGGL(k_hausdorff_close, dim3(grid_c), dim3(HD_TPB), 0, s, logits, target, fields, (int)B, (int)C, c0,
                       has_ignore ? 1 : 0, ig, vol, 0.5f * alpha, wmap);
    return mivp_check_launch("hausdorff_close");
}

// partial rows [B][bpb][2], then {sum (p - g)^2 wmap, N, 1 / (K max(N, 1)), spare}
extern "C" size_t mivp_hausdorff_loss_ws(int32_t B, int64_t vol) {
    if (B < 1 || vol < 1) return 0;
    return (size_t)B * seg_bpb(vol) * HD_K + 4;
}

extern "C" int mivp_hausdorff_loss(const float* logits, const float* target, const float* wmap, int32_t B, int64_t vol, int32_t C,
                                   int32_t include_background, int32_t ignore_index, int32_t has_ignore, float lambda_hausdorff,
                                   const float* weight, float* workspace, float* loss, float* dlogits, int32_t accumulate,
                                   mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && wmap && workspace && loss);
    HD_REQUIRE_OPTIONS();
    return hausdorff_run(logits, target, wmap, B, vol, C, o, lambda_hausdorff, weight, workspace, loss, nullptr, dlogits,
                         accumulate, true, stream);
}

extern "C" int mivp_hausdorff_loss_grad(const float* logits, const float* target, const float* wmap, int32_t B, int64_t vol,
                                        int32_t C, int32_t include_background, int32_t ignore_index, int32_t has_ignore,
                                        float lambda_hausdorff, const float* weight, const float* workspace, const float* gscale,
                                        float* dlogits, int32_t accumulate, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && wmap && workspace && dlogits);
    HD_REQUIRE_OPTIONS();
    return hausdorff_run(logits, target, wmap, B, vol, C, o, lambda_hausdorff, weight, const_cast<float*>(workspace), nullptr,
                         gscale, dlogits, accumulate, false, stream);
}
