// Boundary (signed-distance) loss term (Kervadec et al., MIDL 2019) with the distance maps built on the device, per step
// (mivp_amd/losses.py signed_distance_maps / boundary_loss / SegLossSpec(lambda_boundary=...)).
//
// 1. mivp_distmap_signed: target f32 [B][H][W][D] class indices -> phi f32 [B][K][H][W][D], K = C - c0 classes c0 .. C - 1.
//    Per (b, c), M = {label == c}; a label that is no class (non-integer, outside [0, C), NaN, the ignore label) is in no M:
//      phi = dist to the nearest voxel of M               outside M   (> 0)
//      phi = -(dist to the nearest voxel outside M - 1)   inside M
//      phi = 0 everywhere in (b, c)                       when M is empty or the whole sample
//    (one_hot2dist of the boundary-loss authors: edt(~M, sampling) ~M - (edt(M, sampling) - 1) M; the space beyond the
//    volume border is neither inside nor outside).  Four launches whatever B and K are:
//      seed / D   one wave per (b, h, w) line, 64 consecutive d per step; the label is classified once per voxel of the sweep
//                 and every class takes its two seed masks (M, not M) from ballots: the scheme of surface.hip's k_edt_d with
//                 the (class, side) state of a line kept one pair per lane.  Writes both squared fields of every class:
//                 field (side, b, k) = f32 [vol] at fields + ((side B + b) K + k) vol, side 0 = distance to M, 1 = to not M.
//      W, H       Meijster's lower envelope (edt_line of csrc/edt_common.hpp), one thread per line, the line index running
//                 across all 2 B K fields: one launch each.
//      closing    per voxel the side it needs, the root, 1 - root inside, 0 for +inf (the side of a degenerate M).
//    No atomics, nothing read back, every launch unconditional.  At unit spacing the squared fields are the exact integers.
//    Limits (those of mivp_edt_sq): H, W <= 65535 and B K vol < 2^31.
//
// 2. mivp_boundary_loss / mivp_boundary_loss_grad: with p = softmax_c(z), V the valid voxels of the batch (the rule of
//    csrc/segloss.hip), N = |V|, w = lambda_boundary weight[0]:
//      loss = w sum_{v in V} sum_{c >= c0} p_c phi_c / (K max(N, 1))
//      dz_j = w p_j sum_c p_c (phit_j - phit_c) / (K max(N, 1)),   phit_c = phi_c for c >= c0, else 0
//    (the difference form of p_j (phit_j - sum_c p_c phit_c): it keeps its digits where p_j -> 1).  A streaming statistics
//    pass (partial rows per workgroup in a fixed order), a one-workgroup f64 finalize, a gradient pass that stores every
//    element of dlogits once or, with accumulate, adds to it.  Launch geometry of csrc/segloss.hip.
#include "edt_common.hpp"
#include "segloss_common.hpp"

namespace {
constexpr int DM_MAXK = 16;
constexpr int DM_TPB = 256;

// seed / D pass.  Lane i < 2 K owns the sweep state of pair i = 2 (c - c0) + side: the last seed before the current step
// and the first seed after some step (stale once passed); a pair's state is read with a uniform-index shuffle.
__global__ __launch_bounds__(DM_TPB) void k_distmap_d(const float* __restrict__ y, int B, int C, int c0, int has_ignore,
                                                      float ignore, long lines_per_b, int D, float a, int intp,
                                                      float* __restrict__ fields) {
    const int lane = threadIdx.x & 63;
    const int nch = (D + 63) >> 6;
    const int K = C - c0;
    const long vol = lines_per_b * D;
    const long nlines = (long)B * lines_per_b;
    for (long line = (long)blockIdx.x * (DM_TPB / 64) + (threadIdx.x >> 6); line < nlines; line += (long)gridDim.x * (DM_TPB / 64)) {
        const int b = (int)(line / lines_per_b);
        const long off = (line - (long)b * lines_per_b) * D;       // of the line inside its sample
        const float* row = y + line * D;
        int prev = -EDT_NO_SEED, next = -1;
        for (int k = 0; k < nch; ++k) {
            const int p = 64 * k + lane;
            const int cls = p < D ? seg_class_rt(row[p], C, has_ignore, ignore) : -2;
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
                        const int cq = q < D ? seg_class_rt(row[q], C, has_ignore, ignore) : -2;
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
                    fields[(((long)side * B + b) * K + (pr >> 1)) * vol + off + p] = edt_d_value(min(p - left, right - p), a, intp);
            }
        }
    }
}

// W / H pass over all fields: line = field * lines_per_field + (outer, inner), inner = d fastest across lanes
template <bool INTP>
__global__ __launch_bounds__(DM_TPB) void k_distmap_line(float* __restrict__ fields, long nlines, long lines_per_field, long vol,
                                                         int inner, long outer_stride, long stride, int n, float a,
                                                         int2* __restrict__ stack) {
    const long line = (long)blockIdx.x * DM_TPB + threadIdx.x;
    if (line >= nlines) return;
    const long field = line / lines_per_field, l = line - field * lines_per_field;
    edt_line<INTP>(fields + field * vol + (l / inner) * outer_stride + (l % inner), stride, n, a, stack, nlines, line);
}

// closing: one thread per element of phi
__global__ __launch_bounds__(DM_TPB) void k_distmap_close(const float* __restrict__ y, const float* __restrict__ fields, int B,
                                                          int C, int c0, int has_ignore, float ignore, long vol,
                                                          float* __restrict__ phi) {
    const int K = C - c0;
    const long total = (long)B * K * vol;
    for (long i = (long)blockIdx.x * DM_TPB + threadIdx.x; i < total; i += (long)gridDim.x * DM_TPB) {
        const long bk = i / vol, v = i - bk * vol;
        const int b = (int)(bk / K), k = (int)(bk - (long)b * K);
        const bool inside = seg_class_rt(y[(long)b * vol + v], C, has_ignore, ignore) == c0 + k;
        const float d2 = fields[(inside ? total : 0L) + i];        // side 1 starts B K vol floats in
        const float r = sqrtf(d2);
        phi[i] = isinf(d2) ? 0.f : (inside ? 1.f - r : r);
    }
}

bool dm_dims(const int32_t* dims, int& H, int& W, int& D) {
    H = dims[0]; W = dims[1]; D = dims[2];
    return H >= 1 && W >= 1 && D >= 1 && H <= 65535 && W <= 65535 && (long)H * W * D < (1L << 31);
}

// bytes of the two field sets, rounded so that the stack behind them is 256-byte aligned
size_t dm_field_bytes(long B, long K, long vol) { return ((size_t)(2 * B * K * vol) * sizeof(float) + 255) / 256 * 256; }

// ------------------------------------------------------------------------------------------------- the loss term
constexpr int BD_NUM = 0, BD_CNT = 1, BD_K = 2;                 // columns of a partial row: sum p phi, valid voxels

struct BdOpt {
    int c0, has_ignore;
    float ignore;
};

// softmax of one voxel and whether it is valid
template <int C>
struct BdVoxel {
    float p[C];
    bool valid;
    MIVP_DEV BdVoxel(const float* zz, float yv, const BdOpt& o) {
        valid = seg_class_rt(yv, C, o.has_ignore, o.ignore) >= 0;
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, zz[c]);
        float den = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { p[c] = __expf(zz[c] - mx); den += p[c]; }
        const float inv_den = __builtin_amdgcn_rcpf(den);
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] *= inv_den;
    }
};

// ph[c]: phit of the voxel (0 below c0)
template <int C>
MIVP_DEV void bd_voxel_stats(const float* zz, float yv, const float* ph, const BdOpt& o, float* acc) {
    const BdVoxel<C> v(zz, yv, o);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += v.p[c] * ph[c];
    acc[BD_NUM] += v.valid ? s : 0.f;
    acc[BD_CNT] += v.valid ? 1.f : 0.f;
}

template <int C>
MIVP_DEV void bd_voxel_grad(const float* zz, float yv, const float* ph, const BdOpt& o, float coef, float* gz) {
    const BdVoxel<C> v(zz, yv, o);
#pragma unroll
    for (int j = 0; j < C; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += v.p[c] * (ph[j] - ph[c]);
        gz[j] = v.valid ? coef * (v.p[j] * s) : 0.f;
    }
}

// phit of voxel v of sample b into ph[C]
template <int C>
MIVP_DEV void bd_load_phi(const float* __restrict__ phi, long b, long vol, long v, int c0, float* ph) {
#pragma unroll
    for (int c = 0; c < C; ++c) ph[c] = c >= c0 ? phi[(b * (C - c0) + (c - c0)) * vol + v] : 0.f;
}

// pass 1: per-workgroup partial rows [BD_K], one sample per workgroup row; VEC: four consecutive voxels per thread and
// iteration through 16-byte loads (vol % 4 == 0)
template <int C, bool VEC>
__global__ __launch_bounds__(256) void k_boundary_stats(const float* __restrict__ z, const float* __restrict__ y,
                                                        const float* __restrict__ phi, long vol, BdOpt o, int blocks_per_b,
                                                        float* __restrict__ part) {
    __shared__ float red[4][BD_K];
    const int b = blockIdx.x / blocks_per_b, blk = blockIdx.x % blocks_per_b;
    float acc[BD_K] = {0.f, 0.f};
    if (VEC) {
        const long nq = vol >> 2;
        for (long q = (long)blk * 256 + threadIdx.x; q < nq; q += (long)blocks_per_b * 256) {
            const long v = (long)b * vol + 4 * q;
            float zb[4 * C], pb[4][C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + v * C + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c >= o.c0) f4 = *reinterpret_cast<const float4*>(phi + ((long)b * (C - o.c0) + (c - o.c0)) * vol + 4 * q);
                pb[0][c] = f4.x; pb[1][c] = f4.y; pb[2][c] = f4.z; pb[3][c] = f4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + v);
            bd_voxel_stats<C>(zb, y4.x, pb[0], o, acc);
            bd_voxel_stats<C>(zb + C, y4.y, pb[1], o, acc);
            bd_voxel_stats<C>(zb + 2 * C, y4.z, pb[2], o, acc);
            bd_voxel_stats<C>(zb + 3 * C, y4.w, pb[3], o, acc);
        }
    } else {
        for (long v = (long)blk * 256 + threadIdx.x; v < vol; v += (long)blocks_per_b * 256) {
            const float* zv = z + ((long)b * vol + v) * C;
            float zz[C], ph[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = zv[c];
            bd_load_phi<C>(phi, b, vol, v, o.c0, ph);
            bd_voxel_stats<C>(zz, y[(long)b * vol + v], ph, o, acc);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < BD_K; ++i) {
        float s = acc[i];
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < BD_K) {
        const int i = threadIdx.x;
        part[(long)blockIdx.x * BD_K + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// one workgroup: partials [nrows][BD_K] -> res = {sum p phi, N}, then the value: f64, fixed order
__global__ __launch_bounds__(256) void k_boundary_finalize(const float* __restrict__ part, int nrows, int K, float lam,
                                                           const float* __restrict__ weight, float* __restrict__ res,
                                                           float* __restrict__ loss) {
    __shared__ double red[256][BD_K];
    double s[BD_K] = {0.0, 0.0};
    for (int r = threadIdx.x; r < nrows; r += 256) {
        s[0] += (double)part[(long)r * BD_K];
        s[1] += (double)part[(long)r * BD_K + 1];
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
        res[BD_NUM] = (float)num;
        res[BD_CNT] = (float)N;
        res[2] = (float)(1.0 / ((double)K * (N > 1.0 ? N : 1.0)));
        if (loss) loss[0] = (float)(w * num / ((double)K * (N > 1.0 ? N : 1.0)));
    }
}

// pass 2: dz (=, or += with ACC) up w / (K max(N, 1)) d sum / dz; every element once.  The product is rounded before the
// add: with accumulate the result is dz + g in the bits, g the value a plain store would have written.
template <int C, bool VEC, bool ACC>
__global__ __launch_bounds__(256) void k_boundary_grad(const float* __restrict__ z, const float* __restrict__ y,
                                                       const float* __restrict__ phi, long vol, int B, BdOpt o, float lam,
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
            float zb[4 * C], gb[4 * C], pb[4][C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float4 t4 = *reinterpret_cast<const float4*>(z + i * C + 4 * j);
                zb[4 * j] = t4.x; zb[4 * j + 1] = t4.y; zb[4 * j + 2] = t4.z; zb[4 * j + 3] = t4.w;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float4 f4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c >= o.c0) f4 = *reinterpret_cast<const float4*>(phi + (b * (C - o.c0) + (c - o.c0)) * vol + v);
                pb[0][c] = f4.x; pb[1][c] = f4.y; pb[2][c] = f4.z; pb[3][c] = f4.w;
            }
            const float4 y4 = *reinterpret_cast<const float4*>(y + i);
            bd_voxel_grad<C>(zb, y4.x, pb[0], o, coef, gb);
            bd_voxel_grad<C>(zb + C, y4.y, pb[1], o, coef, gb + C);
            bd_voxel_grad<C>(zb + 2 * C, y4.z, pb[2], o, coef, gb + 2 * C);
            bd_voxel_grad<C>(zb + 3 * C, y4.w, pb[3], o, coef, gb + 3 * C);
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
            float zz[C], gz[C], ph[C];
#pragma unroll
            for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
            bd_load_phi<C>(phi, b, vol, v, o.c0, ph);
            bd_voxel_grad<C>(zz, y[i], ph, o, coef, gz);
#pragma unroll
            for (int c = 0; c < C; ++c) dz[i * C + c] = ACC ? __fadd_rn(dz[i * C + c], gz[c]) : gz[c];
        }
    }
}

int boundary_run(const float* logits, const float* target, const float* phi, int32_t B, int64_t vol, int32_t C, const BdOpt& o,
                 float lam, const float* weight, float* workspace, float* loss, const float* gscale, float* dlogits,
                 int accumulate, bool do_loss, mivp_stream_t stream) {
    const long bpb = seg_bpb(vol);
    float* part = workspace;
    float* res = workspace + (long)B * bpb * BD_K;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vol % 4 == 0;                             // 16-byte loads of four voxels
    if (do_loss) {
#define B_STATS1(CC, VV) hipLaunchKernelGGL((k_boundary_stats<CC, VV>), dim3((unsigned)(B * bpb)), dim3(256), 0, st, logits, target, \
                                            phi, (long)vol, o, (int)bpb, part)
#define B_STATS(CC) do { if (vec) B_STATS1(CC, true); else B_STATS1(CC, false); } while (0)
        SEG_C_SWITCH(B_STATS)
#undef B_STATS
#undef B_STATS1
        int rc = mivp_check_launch("boundary_stats");
        if (rc) return rc;
        hipLaunchKernelGGL(k_boundary_finalize, dim3(1), dim3(256), 0, st, part, (int)(B * bpb), (int)(C - o.c0), lam, weight, res,
                           loss);
        rc = mivp_check_launch("boundary_finalize");
        if (rc) return rc;
    }
    if (!dlogits) return MIVP_OK;
    const long total = vec ? (long)B * vol / 4 : (long)B * vol;
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
#define B_GRAD2(CC, VV, AA) hipLaunchKernelGGL((k_boundary_grad<CC, VV, AA>), dim3(grid), dim3(256), 0, st, logits, target, phi, \
                                               (long)vol, (int)B, o, lam, weight, res, gscale, dlogits)
#define B_GRAD1(CC, VV) do { if (accumulate) B_GRAD2(CC, VV, true); else B_GRAD2(CC, VV, false); } while (0)
#define B_GRAD(CC) do { if (vec) B_GRAD1(CC, true); else B_GRAD1(CC, false); } while (0)
    SEG_C_SWITCH(B_GRAD)
#undef B_GRAD
#undef B_GRAD1
#undef B_GRAD2
    return mivp_check_launch("boundary_grad");
}
}  // namespace

#define BD_REQUIRE_OPTIONS()                                                                                  \
    MIVP_REQUIRE(B > 0 && vol > 0 && C >= 2 && C <= SEG_MAXC);                                                \
    MIVP_REQUIRE((long)B * seg_bpb(vol) < (1L << 31));                                                        \
    MIVP_REQUIRE(lambda_boundary >= 0.f && lambda_boundary <= 3.0e38f);                                       \
    const BdOpt o = {include_background ? 0 : 1, has_ignore ? 1 : 0, (float)ignore_index}

extern "C" size_t mivp_distmap_ws(int32_t B, int32_t K, const int32_t* dims) {
    int H, W, D;
    if (!dims || B < 1 || K < 1 || K > DM_MAXK || !dm_dims(dims, H, W, D)) return 0;
    const long vol = (long)H * W * D;
    if ((long)B * K * vol >= (1L << 31)) return 0;
    return dm_field_bytes(B, K, vol) + (size_t)(2L * B * K * vol) * sizeof(int2);
}

extern "C" int mivp_distmap_signed(const float* target, int32_t B, int32_t C, int32_t include_background, int32_t ignore_index,
                                   int32_t has_ignore, const int32_t* dims, const float* spacing, float* phi, void* workspace,
                                   mivp_stream_t stream) {
    MIVP_REQUIRE(target && dims && spacing && phi && workspace && B >= 1);
    const int c0 = include_background ? 0 : 1;
    const int K = C - c0;
    MIVP_REQUIRE(C >= 1 && K >= 1 && K <= DM_MAXK);
    int H, W, D;
    MIVP_REQUIRE(dm_dims(dims, H, W, D));                       // H, W <= 65535: the 16-bit sites of the envelope's stack
    const long vol = (long)H * W * D;
    MIVP_REQUIRE((long)B * K * vol < (1L << 31));
    MIVP_REQUIRE(spacing[0] > 0.f && spacing[1] > 0.f && spacing[2] > 0.f);
    MIVP_REQUIRE(isfinite(spacing[0]) && isfinite(spacing[1]) && isfinite(spacing[2]));
    const bool intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    hipStream_t s = (hipStream_t)stream;
    float* fields = (float*)workspace;
    int2* stack = (int2*)((char*)workspace + dm_field_bytes(B, K, vol));
    const float ig = (float)ignore_index;
    const long lines_d = (long)B * H * W;
    const unsigned grid_d = (unsigned)((lines_d + 3) / 4 > 16384 ? 16384 : (lines_d + 3) / 4);
    hipLaunchKernelGGL(k_distmap_d, dim3(grid_d), dim3(DM_TPB), 0, s, target, (int)B, (int)C, c0, has_ignore ? 1 : 0, ig,
                       (long)H * W, D, spacing[2] * spacing[2], (int)intp, fields);
    int rc = mivp_check_launch("distmap_d");
    if (rc != MIVP_OK) return rc;
    // W pass: lines (h, d) of a field, elements w at stride D; H pass: lines (w, d), elements h at stride W * D
    const long nf = 2L * B * K;
    const long lpf_w = (long)H * D, lpf_h = (long)W * D;
    const long lines_w = nf * lpf_w, lines_h = nf * lpf_h;
    const float aw = spacing[1] * spacing[1], ah = spacing[0] * spacing[0];
    const unsigned grid_w = (unsigned)((lines_w + DM_TPB - 1) / DM_TPB), grid_h = (unsigned)((lines_h + DM_TPB - 1) / DM_TPB);
    if (intp) {
        hipLaunchKernelGGL(k_distmap_line<true>, dim3(grid_w), dim3(DM_TPB), 0, s, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_distmap_line<true>, dim3(grid_h), dim3(DM_TPB), 0, s, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    } else {
        hipLaunchKernelGGL(k_distmap_line<false>, dim3(grid_w), dim3(DM_TPB), 0, s, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_distmap_line<false>, dim3(grid_h), dim3(DM_TPB), 0, s, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    }
    rc = mivp_check_launch("distmap_line");
    if (rc != MIVP_OK) return rc;
    const long total = (long)B * K * vol;
    const unsigned grid_c = (unsigned)((total + DM_TPB - 1) / DM_TPB > 16384 ? 16384 : (total + DM_TPB - 1) / DM_TPB);
    hipLaunchKernelGGL(k_distmap_close, dim3(grid_c), dim3(DM_TPB), 0, s, target, fields, (int)B, (int)C, c0, has_ignore ? 1 : 0,
                       ig, vol, phi);
    return mivp_check_launch("distmap_close");
}

// partial rows [B][bpb][2], then {sum p phi, N, 1 / (K max(N, 1)), spare}
extern "C" size_t mivp_boundary_loss_ws(int32_t B, int64_t vol) {
    if (B < 1 || vol < 1) return 0;
    return (size_t)B * seg_bpb(vol) * BD_K + 4;
}

extern "C" int mivp_boundary_loss(const float* logits, const float* target, const float* phi, int32_t B, int64_t vol, int32_t C,
                                  int32_t include_background, int32_t ignore_index, int32_t has_ignore, float lambda_boundary,
                                  const float* weight, float* workspace, float* loss, float* dlogits, int32_t accumulate,
                                  mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && phi && workspace && loss);
    BD_REQUIRE_OPTIONS();
    return boundary_run(logits, target, phi, B, vol, C, o, lambda_boundary, weight, workspace, loss, nullptr, dlogits, accumulate,
                        true, stream);
}

extern "C" int mivp_boundary_loss_grad(const float* logits, const float* target, const float* phi, int32_t B, int64_t vol,
                                       int32_t C, int32_t include_background, int32_t ignore_index, int32_t has_ignore,
                                       float lambda_boundary, const float* weight, const float* workspace, const float* gscale,
                                       float* dlogits, int32_t accumulate, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && phi && workspace && dlogits);
    BD_REQUIRE_OPTIONS();
    return boundary_run(logits, target, phi, B, vol, C, o, lambda_boundary, weight, const_cast<float*>(workspace), nullptr, gscale,
                        dlogits, accumulate, false, stream);
}
