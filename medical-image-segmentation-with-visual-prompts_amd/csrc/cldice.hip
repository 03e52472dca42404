// clDice (soft-skeleton) loss term (Shit et al., CVPR 2021) and the soft skeleton itself
// (mivp_amd/losses.py soft_skeleton / cldice_loss / SegLossSpec(lambda_cldice=...)).
//
// Fields are planar f32 [nf][H][W][D].  For a field x and n >= 1 iterations:
//   erode(x)(v)  = min of x over v and its 6 face neighbours inside the volume
//   dilate(x)(v) = max of x over the 3x3x3 cube around v inside the volume
//   E_0 = x, E_{j+1} = erode(E_j);  O_j = dilate(E_{j+1});  d_j = relu(E_j - O_j)            j = 0 .. n
//   S_0 = d_0, S_j = S_{j-1} + relu(d_j - S_{j-1} d_j)   (every operation rounded on its own);  soft_skeleton = S_n
// relu(x) = x > 0 ? x : +0.  Finite inputs only.
//
// Forward: one launch per j (k_skel_fwd), n + 1 in all whatever the number of fields: field along grid.y, an 8 x 8 x 16
// brick of voxels per workgroup.  The workgroup loads E_j with a two-voxel halo into LDS (+inf beyond the volume), erodes
// it onto the brick with a one-voxel halo (-inf beyond the volume), dilates that onto the brick and steps the recurrence.
// Min and max select copies of input values, so a halo cell recomputed by a neighbouring workgroup has the same bits.
//
// Backward: min and max hand the gradient of a pooled voxel o to the k voxels of its window that hold the selected
// value, g(o) / k each; relu'(0) = 0.  The recurrence is voxel-local: k_skel_point_bwd recomputes S_0 .. S_n of a voxel in
// registers, walks it backwards and writes A_j = [E_j > O_j] d loss / d d_j over O_j (so a workspace serves ONE backward).
// Then, with G_j = d loss / d E_j, from j = n + 1 down to 0 (k_skel_bwd, one launch per j, gather form, fixed order):
//   G_j(u) = A_j(u) + sum_{o in cube(u)} [E_j(u) == O_{j-1}(o)] (-A_{j-1}(o) / kd(o)) + sum_{o in cross(u)} [E_j(u) == E_{j+1}(o)] G_{j+1}(o) / ke(o)
// O_{j-1} = dilate(E_j), E_{j+1} = erode(E_j) and the tie counts kd, ke are recomputed on the LDS tile of E_j.
// No atomics, nothing read back, every launch unconditional.
//
// The term (mivp_cldice_loss): p = softmax_c(z), t = one-hot(label), both 0 at invalid voxels (the rule of
// csrc/segloss.hip), classes c >= 1, K = C - 1, field (b, k) = class k + 1 of sample b, s = smooth:
//   SP = soft_skeleton(p), SL = soft_skeleton(t);  Tprec = (sum SP t + s) / (sum SP + s), Tsens = (sum SL p + s) / (sum SL + s)
//   cl = 1 - 2 Tprec Tsens / (Tprec + Tsens);  loss = lambda weight[0] mean cl   (rows: the samples, or the batch)
// prep (p, t planar) -> n + 1 forward launches (both sides in each) -> statistics (partial rows in a fixed order) -> one
// workgroup f64 finalize (value + the per-(row, class) coefficients of the gradient) | point backward -> n + 2 backward
// launches -> gradient pass through the softmax, stored or added onto dlogits with one rounded add.
#include "segloss_common.hpp"

// the recurrence owes the bits of operations rounded one by one: no contraction anywhere in this file (the pragma is
// lexical: it reaches the operators written here, not the bodies of the __f*_rn helpers of the HIP headers)
#pragma clang fp contract(off)

namespace {
constexpr int CL_MAXN = 16;
constexpr int CL_TPB = 256;
constexpr int CL_BH = 8, CL_BW = 8, CL_BD = 16;                            // the brick
constexpr int CL_T2H = CL_BH + 4, CL_T2W = CL_BW + 4, CL_T2D = CL_BD + 4;  // with a two-voxel halo: 2880 cells
constexpr int CL_T1H = CL_BH + 2, CL_T1W = CL_BW + 2, CL_T1D = CL_BD + 2;  // with a one-voxel halo: 1800 cells
constexpr int CL_N2 = CL_T2H * CL_T2W * CL_T2D, CL_N1 = CL_T1H * CL_T1W * CL_T1D, CL_N0 = CL_BH * CL_BW * CL_BD;
constexpr int CL_STAT = 4;                                                 // sum SP t, sum SP, sum SL p, sum SL
constexpr int CL_COEF = 3;                                                 // dL/dSP = c0 t + c1, dL/dp (direct) = c2 SL

struct ClGeo {
    int H, W, D, nbw, nbd;
    long vol;
};

MIVP_DEV float cl_relu(float x) { return x > 0.f ? x : 0.f; }

// origin of this workgroup's brick
MIVP_DEV void cl_origin(const ClGeo& g, int& h0, int& w0, int& d0) {
    const int bi = blockIdx.x;
    const int bd = bi % g.nbd, bw = (bi / g.nbd) % g.nbw, bh = bi / (g.nbd * g.nbw);
    h0 = bh * CL_BH; w0 = bw * CL_BW; d0 = bd * CL_BD;
}

MIVP_DEV bool cl_inside(const ClGeo& g, int h, int w, int d) {
    return h >= 0 && h < g.H && w >= 0 && w < g.W && d >= 0 && d < g.D;
}

// the field's voxels around the brick with a two-voxel halo -> tile[CL_N2]; `fill` beyond the volume
MIVP_DEV void cl_load_tile2(const float* f, const ClGeo& g, int h0, int w0, int d0, float fill, float* tile) {
    for (int i = threadIdx.x; i < CL_N2; i += CL_TPB) {
        const int dd = i % CL_T2D, ww = (i / CL_T2D) % CL_T2W, hh = i / (CL_T2D * CL_T2W);
        const int h = h0 - 2 + hh, w = w0 - 2 + ww, d = d0 - 2 + dd;
        tile[i] = cl_inside(g, h, w, d) ? f[((long)h * g.W + w) * g.D + d] : fill;
    }
}

// index in the two-halo tile of cell (hh, ww, dd) of the one-halo tile
MIVP_DEV int cl_t2_of_t1(int hh, int ww, int dd) { return ((hh + 1) * CL_T2W + (ww + 1)) * CL_T2D + (dd + 1); }

struct SkelGroup {
    const float* src;      // E_j
    float* dst_e;          // E_{j+1}
    float* dst_o;          // O_j, or NULL
    float* s;              // S_{j-1} in, S_j out (the same voxel by the same thread)
};

// one step j of the forward for the fields of two groups (nfa fields of group a, then those of b)
__global__ __launch_bounds__(CL_TPB) void k_skel_fwd(SkelGroup a, SkelGroup b, int nfa, ClGeo g, int first) {
    __shared__ float t2[CL_N2];
    __shared__ float t1[CL_N1];
    const int fy = blockIdx.y;
    const SkelGroup grp = fy < nfa ? a : b;
    const long off = (long)(fy < nfa ? fy : fy - nfa) * g.vol;
    int h0, w0, d0;
    cl_origin(g, h0, w0, d0);
    cl_load_tile2(grp.src + off, g, h0, w0, d0, INFINITY, t2);
    __syncthreads();
    for (int i = threadIdx.x; i < CL_N1; i += CL_TPB) {
        const int dd = i % CL_T1D, ww = (i / CL_T1D) % CL_T1W, hh = i / (CL_T1D * CL_T1W);
        float m = -INFINITY;                                               // beyond the volume: outside every maximum
        if (cl_inside(g, h0 - 1 + hh, w0 - 1 + ww, d0 - 1 + dd)) {
            const int c = cl_t2_of_t1(hh, ww, dd);
            m = fminf(t2[c], fminf(fminf(t2[c - 1], t2[c + 1]), fminf(fminf(t2[c - CL_T2D], t2[c + CL_T2D]),
                                                                    fminf(t2[c - CL_T2D * CL_T2W], t2[c + CL_T2D * CL_T2W]))));
        }
        t1[i] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CL_N0; i += CL_TPB) {
        const int dd = i % CL_BD, ww = (i / CL_BD) % CL_BW, hh = i / (CL_BD * CL_BW);
        const int h = h0 + hh, w = w0 + ww, d = d0 + dd;
        if (!cl_inside(g, h, w, d)) continue;
        const int c1 = ((hh + 1) * CL_T1W + (ww + 1)) * CL_T1D + (dd + 1);
        float o = -INFINITY;
#pragma unroll
        for (int a3 = -1; a3 <= 1; ++a3)
#pragma unroll
            for (int b3 = -1; b3 <= 1; ++b3)
#pragma unroll
                for (int c3 = -1; c3 <= 1; ++c3) o = fmaxf(o, t1[c1 + (a3 * CL_T1W + b3) * CL_T1D + c3]);
        const long v = off + ((long)h * g.W + w) * g.D + d;
        const float e = t2[cl_t2_of_t1(hh + 1, ww + 1, dd + 1)];
        const float dj = cl_relu(e - o);
        grp.dst_e[v] = t1[c1];
        if (grp.dst_o) grp.dst_o[v] = o;
        if (first) {
            grp.s[v] = dj;
        } else {
            const float sp = grp.s[v];
            grp.s[v] = sp + cl_relu(dj - sp * dj);
        }
    }
}

// the incoming gradient of S_n of the term: c0 t + c1 of the voxel's (row, class), t from the label
struct ClUp {
    const float* coef;     // [rows][K][CL_COEF], or NULL: read gup
    const float* y;        // labels [B][vol]
    int K, C, batch, has_ignore;
    float ignore;
};

MIVP_DEV int cl_class(float yv, int C, int has_ignore, float ignore) {
    const bool ok = yv >= 0.f && yv < (float)C && yv == floorf(yv) && !(has_ignore && yv == ignore);
    return ok ? (int)yv : -1;
}

// voxel-local backward of the recurrence: A_j = [E_j > O_j] d loss / d d_j over O_j.  e0: E_0 [nf][vol]; es: E_1 .. E_{n+1},
// oa: O_0 .. O_n, slabs of F = nf vol floats
__global__ __launch_bounds__(CL_TPB) void k_skel_point_bwd(const float* __restrict__ e0, const float* __restrict__ es,
                                                           float* __restrict__ oa, long F, long vol, int n,
                                                           const float* __restrict__ gup, ClUp up) {
    for (long i = (long)blockIdx.x * CL_TPB + threadIdx.x; i < F; i += (long)gridDim.x * CL_TPB) {
        float dj[CL_MAXN + 1], sj[CL_MAXN + 1];
        bool pos[CL_MAXN + 1];
#pragma unroll
        for (int j = 0; j <= CL_MAXN; ++j) {
            dj[j] = 0.f; sj[j] = 0.f; pos[j] = false;
            if (j <= n) {
                const float e = j == 0 ? e0[i] : es[(long)(j - 1) * F + i];
                const float x = e - oa[(long)j * F + i];
                pos[j] = x > 0.f;
                dj[j] = cl_relu(x);
                sj[j] = j == 0 ? dj[0] : sj[j - 1] + cl_relu(dj[j] - sj[j - 1] * dj[j]);
            }
        }
        float gs;
        if (up.coef) {
            const long f = i / vol, v = i - f * vol;
            const int b = (int)(f / up.K), k = (int)(f - (long)b * up.K);
            const float* cf = up.coef + ((long)(up.batch ? 0 : b) * up.K + k) * CL_COEF;
            const bool hit = cl_class(up.y[(long)b * vol + v], up.C, up.has_ignore, up.ignore) == k + 1;
            gs = hit ? cf[0] + cf[1] : cf[1];
        } else {
            gs = gup[i];
        }
#pragma unroll
        for (int j = CL_MAXN; j >= 1; --j) {
            if (j <= n) {
                const float r = dj[j] - sj[j - 1] * dj[j];
                const float gr = r > 0.f ? gs : 0.f;
                oa[(long)j * F + i] = pos[j] ? gr * (1.f - sj[j - 1]) : 0.f;
                gs = gs - gr * dj[j];
            }
        }
        oa[i] = pos[0] ? gs : 0.f;
    }
}

// one step of the spatial backward: G_j from E_j, A_{j-1} (NULL at j == 0), G_{j+1} (NULL at j == n + 1), A_j (NULL at n + 1)
__global__ __launch_bounds__(CL_TPB) void k_skel_bwd(const float* __restrict__ ej, const float* __restrict__ aprev,
                                                     const float* __restrict__ gnext, const float* __restrict__ acur,
                                                     float* __restrict__ gout, ClGeo g) {
    __shared__ float t2[CL_N2];
    __shared__ float so[CL_N1], sm[CL_N1], hd[CL_N1], he[CL_N1];
    const long off = (long)blockIdx.y * g.vol;
    int h0, w0, d0;
    cl_origin(g, h0, w0, d0);
    cl_load_tile2(ej + off, g, h0, w0, d0, NAN, t2);                      // NaN beyond the volume: equal to nothing
    __syncthreads();
    for (int i = threadIdx.x; i < CL_N1; i += CL_TPB) {
        const int dd = i % CL_T1D, ww = (i / CL_T1D) % CL_T1W, hh = i / (CL_T1D * CL_T1W);
        const int h = h0 - 1 + hh, w = w0 - 1 + ww, d = d0 - 1 + dd;
        float mx = NAN, mn = NAN, vd = 0.f, ve = 0.f;
        if (cl_inside(g, h, w, d)) {
            const int c = cl_t2_of_t1(hh, ww, dd);
            const long v = off + ((long)h * g.W + w) * g.D + d;
            if (aprev) {
                mx = -INFINITY;
#pragma unroll
                for (int a3 = -1; a3 <= 1; ++a3)
#pragma unroll
                    for (int b3 = -1; b3 <= 1; ++b3)
#pragma unroll
                        for (int c3 = -1; c3 <= 1; ++c3) mx = fmaxf(mx, t2[c + (a3 * CL_T2W + b3) * CL_T2D + c3]);
                int kd = 0;
#pragma unroll
                for (int a3 = -1; a3 <= 1; ++a3)
#pragma unroll
                    for (int b3 = -1; b3 <= 1; ++b3)
#pragma unroll
                        for (int c3 = -1; c3 <= 1; ++c3) kd += t2[c + (a3 * CL_T2W + b3) * CL_T2D + c3] == mx ? 1 : 0;
                vd = -aprev[v] / (float)(kd > 0 ? kd : 1);
            }
            if (gnext) {
                const int nb[7] = {0, -1, 1, -CL_T2D, CL_T2D, -CL_T2D * CL_T2W, CL_T2D * CL_T2W};
                mn = INFINITY;
#pragma unroll
                for (int q = 0; q < 7; ++q) mn = fminf(mn, t2[c + nb[q]]);
                int ke = 0;
#pragma unroll
                for (int q = 0; q < 7; ++q) ke += t2[c + nb[q]] == mn ? 1 : 0;
                ve = gnext[v] / (float)(ke > 0 ? ke : 1);
            }
        }
        so[i] = mx; sm[i] = mn; hd[i] = vd; he[i] = ve;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CL_N0; i += CL_TPB) {
        const int dd = i % CL_BD, ww = (i / CL_BD) % CL_BW, hh = i / (CL_BD * CL_BW);
        const int h = h0 + hh, w = w0 + ww, d = d0 + dd;
        if (!cl_inside(g, h, w, d)) continue;
        const int c1 = ((hh + 1) * CL_T1W + (ww + 1)) * CL_T1D + (dd + 1);
        const long v = off + ((long)h * g.W + w) * g.D + d;
        const float e = t2[cl_t2_of_t1(hh + 1, ww + 1, dd + 1)];
        float acc = acur ? acur[v] : 0.f;
#pragma unroll
        for (int a3 = -1; a3 <= 1; ++a3)
#pragma unroll
            for (int b3 = -1; b3 <= 1; ++b3)
#pragma unroll
                for (int c3 = -1; c3 <= 1; ++c3) {
                    const int o = c1 + (a3 * CL_T1W + b3) * CL_T1D + c3;
                    acc += so[o] == e ? hd[o] : 0.f;
                }
        const int nb[7] = {0, -1, 1, -CL_T1D, CL_T1D, -CL_T1D * CL_T1W, CL_T1D * CL_T1W};
#pragma unroll
        for (int q = 0; q < 7; ++q) acc += sm[c1 + nb[q]] == e ? he[c1 + nb[q]] : 0.f;
        gout[v] = acc;
    }
}

bool cl_geo(const int32_t* dims, ClGeo& g, long& nbricks) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    g.H = dims[0]; g.W = dims[1]; g.D = dims[2];
    g.vol = (long)g.H * g.W * g.D;
    if (g.vol >= (1L << 31)) return false;
    g.nbw = (g.W + CL_BW - 1) / CL_BW; g.nbd = (g.D + CL_BD - 1) / CL_BD;
    nbricks = (long)((g.H + CL_BH - 1) / CL_BH) * g.nbw * g.nbd;
    return true;
}

// floats of a skeleton workspace: keep: E_1 .. E_{n+1} | O_0 .. O_n (A_j after a backward) | two gradient fields;
// else the two fields the erosions alternate between
size_t skel_ws_floats(long F, int n, int keep) { return (size_t)F * (keep ? 2 * (n + 1) + 2 : 2); }

// the forward of one or two groups.  Group a: E_0 = xa, kept (es / os slabs of Fa) or alternating between pa0 / pa1;
// group b (nfb may be 0) always alternates between pb0 / pb1, E_0 = xb
int skel_forward(const float* xa, int nfa, float* es, float* os, float* pa0, float* pa1, float* sa, const float* xb, int nfb,
                 float* pb0, float* pb1, float* sb, const ClGeo& g, long nbricks, int n, hipStream_t st) {
    const long Fa = (long)nfa * g.vol;
    for (int j = 0; j <= n; ++j) {
        SkelGroup a, b;
        if (es) {
            a.src = j == 0 ? xa : es + (long)(j - 1) * Fa;
            a.dst_e = es + (long)j * Fa;
            a.dst_o = os + (long)j * Fa;
        } else {
            a.src = j == 0 ? xa : ((j & 1) ? pa0 : pa1);
            a.dst_e = (j & 1) ? pa1 : pa0;
            a.dst_o = nullptr;
        }
        a.s = sa;
        b.src = j == 0 ? xb : ((j & 1) ? pb0 : pb1);
        b.dst_e = (j & 1) ? pb1 : pb0;
        b.dst_o = nullptr;
        b.s = sb;
        hipLaunchKernelGGL(k_skel_fwd, dim3((unsigned)nbricks, (unsigned)(nfa + nfb)), dim3(CL_TPB), 0, st, a, b, nfa, g, j == 0 ? 1 : 0);
        const int rc = mivp_check_launch("cldice_skel_fwd");
        if (rc) return rc;
    }
    return MIVP_OK;
}

// the backward: e0 = E_0, ws = a keep workspace after its forward; G_0 -> dx (may be ws's first gradient field)
int skel_backward(const float* e0, int nf, float* ws, const float* gup, const ClUp& up, float* dx, const ClGeo& g, long nbricks,
                  int n, hipStream_t st) {
    const long F = (long)nf * g.vol;
    float* es = ws;
    float* oa = ws + (long)(n + 1) * F;
    float* gb[2] = {ws + (long)(2 * n + 2) * F, ws + (long)(2 * n + 3) * F};
    const unsigned grid = (unsigned)((F + CL_TPB - 1) / CL_TPB > 16384 ? 16384 : (F + CL_TPB - 1) / CL_TPB);
    hipLaunchKernelGGL(k_skel_point_bwd, dim3(grid), dim3(CL_TPB), 0, st, e0, es, oa, F, g.vol, n, gup, up);
    int rc = mivp_check_launch("cldice_skel_point_bwd");
    if (rc) return rc;
    for (int j = n + 1; j >= 0; --j) {
        const float* ej = j == 0 ? e0 : es + (long)(j - 1) * F;
        const float* aprev = j >= 1 ? oa + (long)(j - 1) * F : nullptr;
        const float* gnext = j <= n ? gb[(j + 1) & 1] : nullptr;
        const float* acur = j <= n ? oa + (long)j * F : nullptr;
        float* out = j == 0 ? dx : gb[j & 1];
        hipLaunchKernelGGL(k_skel_bwd, dim3((unsigned)nbricks, (unsigned)nf), dim3(CL_TPB), 0, st, ej, aprev, gnext, acur, out, g);
        rc = mivp_check_launch("cldice_skel_bwd");
        if (rc) return rc;
    }
    return MIVP_OK;
}

// ------------------------------------------------------------------------------------------------- the term
struct ClOpt {
    int batch, has_ignore;
    float ignore, smooth, lam;
};

// softmax of one voxel and its class (-1: invalid)
template <int C>
struct ClVoxel {
    float p[C];
    int cls;
    MIVP_DEV ClVoxel(const float* zz, float yv, const ClOpt& o) {
        cls = cl_class(yv, C, o.has_ignore, o.ignore);
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

// p_c and t_c of the classes c >= 1 as planar fields [B][K][vol]; zeros at invalid voxels
template <int C>
__global__ __launch_bounds__(CL_TPB) void k_cldice_prep(const float* __restrict__ z, const float* __restrict__ y, long vol, int B,
                                                        ClOpt o, float* __restrict__ pf, float* __restrict__ tf) {
    const long total = (long)B * vol;
    for (long i = (long)blockIdx.x * CL_TPB + threadIdx.x; i < total; i += (long)gridDim.x * CL_TPB) {
        const long b = i / vol, v = i - b * vol;
        float zz[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
        const ClVoxel<C> vx(zz, y[i], o);
#pragma unroll
        for (int c = 1; c < C; ++c) {
            const long at = (b * (C - 1) + (c - 1)) * vol + v;
            pf[at] = vx.cls >= 0 ? vx.p[c] : 0.f;
            tf[at] = vx.cls == c ? 1.f : 0.f;
        }
    }
}

// partial rows [nf][bpb][CL_STAT]: workgroup (blk, f) sums its voxels of field f
__global__ __launch_bounds__(CL_TPB) void k_cldice_stats(const float* __restrict__ pf, const float* __restrict__ sp,
                                                         const float* __restrict__ sl, const float* __restrict__ y, long vol, int K,
                                                         int C, ClOpt o, float* __restrict__ part) {
    __shared__ float red[4][CL_STAT];
    const int f = blockIdx.y, b = f / K, k = f - b * K;
    float acc[CL_STAT] = {0.f, 0.f, 0.f, 0.f};
    for (long v = (long)blockIdx.x * CL_TPB + threadIdx.x; v < vol; v += (long)gridDim.x * CL_TPB) {
        const long at = (long)f * vol + v;
        const bool hit = cl_class(y[(long)b * vol + v], C, o.has_ignore, o.ignore) == k + 1;
        const float a = sp[at], l = sl[at];
        acc[0] += hit ? a : 0.f;
        acc[1] += a;
        acc[2] += l * pf[at];
        acc[3] += l;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CL_STAT; ++i) {
        float s = acc[i];
        for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < CL_STAT) {
        const int i = threadIdx.x;
        part[((long)f * gridDim.x + blockIdx.x) * CL_STAT + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

// one workgroup: partial rows -> sums [nf][CL_STAT] -> the value and the coefficients [rows][K][CL_COEF]: f64, fixed order
__global__ __launch_bounds__(CL_TPB) void k_cldice_finalize(const float* __restrict__ part, int B, int K, int bpb, ClOpt o,
                                                            const float* __restrict__ weight, float* __restrict__ sums,
                                                            float* __restrict__ coef, float* __restrict__ loss) {
    const int nf = B * K;
    for (int i = threadIdx.x; i < nf * CL_STAT; i += CL_TPB) {
        const int f = i / CL_STAT, q = i - f * CL_STAT;
        double s = 0.0;
        for (int j = 0; j < bpb; ++j) s += (double)part[((long)f * bpb + j) * CL_STAT + q];
        sums[i] = (float)s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int rows = o.batch ? 1 : B;
        const double sm = (double)o.smooth, m = 1.0 / ((double)rows * (double)K);
        double total = 0.0;
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < K; ++k) {
                double a[CL_STAT] = {0.0, 0.0, 0.0, 0.0};
                for (int b = (o.batch ? 0 : r); b < (o.batch ? B : r + 1); ++b)
                    for (int q = 0; q < CL_STAT; ++q) a[q] += (double)sums[((long)b * K + k) * CL_STAT + q];
                const double P = (a[0] + sm) / (a[1] + sm), S = (a[2] + sm) / (a[3] + sm);
                total += 1.0 - 2.0 * P * S / (P + S);
                const double dP = -2.0 * S * S / ((P + S) * (P + S)), dS = -2.0 * P * P / ((P + S) * (P + S));
                float* cf = coef + ((long)r * K + k) * CL_COEF;
                cf[0] = (float)(m * dP / (a[1] + sm));
                cf[1] = (float)(-m * dP * (a[0] + sm) / ((a[1] + sm) * (a[1] + sm)));
                cf[2] = (float)(m * dS / (a[3] + sm));
            }
        const double w = (double)o.lam * (weight ? (double)weight[0] : 1.0);
        if (loss) loss[0] = (float)(w * total * m);
    }
}

// dz (=, or += with ACC) up w (G_0 + c2 SL) through the softmax; exact zeros at invalid voxels.  The value is rounded
// before the add: with accumulate the result is dz + g in the bits
template <int C, bool ACC>
__global__ __launch_bounds__(CL_TPB) void k_cldice_grad(const float* __restrict__ z, const float* __restrict__ y,
                                                        const float* __restrict__ g0, const float* __restrict__ sl,
                                                        const float* __restrict__ coef, long vol, int B, ClOpt o,
                                                        const float* __restrict__ weight, const float* __restrict__ gscale,
                                                        float* __restrict__ dz) {
    const long total = (long)B * vol;
    const float scale = (gscale ? gscale[0] : 1.f) * (o.lam * (weight ? weight[0] : 1.f));
    for (long i = (long)blockIdx.x * CL_TPB + threadIdx.x; i < total; i += (long)gridDim.x * CL_TPB) {
        const long b = i / vol, v = i - b * vol;
        float zz[C], gp[C];
#pragma unroll
        for (int c = 0; c < C; ++c) zz[c] = z[i * C + c];
        const ClVoxel<C> vx(zz, y[i], o);
        gp[0] = 0.f;
        float pg = 0.f;
#pragma unroll
        for (int c = 1; c < C; ++c) {
            const long at = (b * (C - 1) + (c - 1)) * vol + v;
            gp[c] = g0[at] + coef[((o.batch ? 0 : b) * (C - 1) + (c - 1)) * CL_COEF + 2] * sl[at];
            pg += vx.p[c] * gp[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float gz = vx.cls >= 0 ? scale * (vx.p[c] * (gp[c] - pg)) : 0.f;
            dz[i * C + c] = ACC ? dz[i * C + c] + gz : gz;
        }
    }
}

// the workspace of the term, in floats from its start; F = B K vol
struct ClLayout {
    long F, p, skel, g0, sp, sl, part, sums, coef, total;
    int bpb;
    ClLayout(int B, int K, long vol, int n) {
        F = (long)B * K * vol;
        bpb = (int)seg_bpb(vol);
        p = 0;                                                  // E_0 of the p side: the planar p
        skel = F;                                               // the keep workspace of the p side
        g0 = skel + (long)(2 * n + 2) * F;                      // its two gradient fields: the t side's erosions, later G_0
        sp = skel + (long)skel_ws_floats(F, n, 1);
        sl = sp + F;
        part = sl + F;
        sums = part + (long)B * K * bpb * CL_STAT;
        coef = sums + (long)B * K * CL_STAT;
        total = coef + (long)B * K * CL_COEF;
    }
};

int cldice_run(const float* z, const float* y, int B, int C, const int32_t* dims, int n, const ClOpt& o, const float* weight,
               float* ws, float* loss, const float* gscale, float* dz, int accumulate, bool do_loss, hipStream_t st) {
    ClGeo g;
    long nbricks;
    if (!cl_geo(dims, g, nbricks)) return MIVP_EINVAL;
    const int K = C - 1;
    const ClLayout lay(B, K, g.vol, n);
    const long total = (long)B * g.vol;
    const unsigned grid = (unsigned)((total + CL_TPB - 1) / CL_TPB > 16384 ? 16384 : (total + CL_TPB - 1) / CL_TPB);
    int rc;
    if (do_loss) {
        float* tf = ws + lay.g0;                                // the planar t: E_0 of the t side
#define CL_PREP(CC) hipLaunchKernelGGL((k_cldice_prep<CC>), dim3(grid), dim3(CL_TPB), 0, st, z, y, g.vol, B, o, ws + lay.p, tf)
        SEG_C_SWITCH(CL_PREP)
#undef CL_PREP
        rc = mivp_check_launch("cldice_prep");
        if (rc) return rc;
        rc = skel_forward(ws + lay.p, B * K, ws + lay.skel, ws + lay.skel + (long)(n + 1) * lay.F, nullptr, nullptr, ws + lay.sp, tf,
                          B * K, ws + lay.g0 + lay.F, tf, ws + lay.sl, g, nbricks, n, st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cldice_stats, dim3((unsigned)lay.bpb, (unsigned)(B * K)), dim3(CL_TPB), 0, st, ws + lay.p, ws + lay.sp,
                           ws + lay.sl, y, g.vol, K, C, o, ws + lay.part);
        rc = mivp_check_launch("cldice_stats");
        if (rc) return rc;
        hipLaunchKernelGGL(k_cldice_finalize, dim3(1), dim3(CL_TPB), 0, st, ws + lay.part, B, K, lay.bpb, o, weight, ws + lay.sums,
                           ws + lay.coef, loss);
        rc = mivp_check_launch("cldice_finalize");
        if (rc) return rc;
    }
    if (!dz) return MIVP_OK;
    const ClUp up = {ws + lay.coef, y, K, C, o.batch, o.has_ignore, o.ignore};
    rc = skel_backward(ws + lay.p, B * K, ws + lay.skel, nullptr, up, ws + lay.g0, g, nbricks, n, st);
    if (rc) return rc;
#define CL_GRAD1(CC, AA) hipLaunchKernelGGL((k_cldice_grad<CC, AA>), dim3(grid), dim3(CL_TPB), 0, st, z, y, ws + lay.g0, ws + lay.sl, \
                                            ws + lay.coef, g.vol, B, o, weight, gscale, dz)
#define CL_GRAD(CC) do { if (accumulate) CL_GRAD1(CC, true); else CL_GRAD1(CC, false); } while (0)
    SEG_C_SWITCH(CL_GRAD)
#undef CL_GRAD
#undef CL_GRAD1
    return mivp_check_launch("cldice_grad");
}

bool cl_fields_ok(long nf, const int32_t* dims, int n, long per_field) {
    ClGeo g;
    long nbricks;
    if (nf < 1 || nf > 32767 || n < 1 || n > CL_MAXN || !cl_geo(dims, g, nbricks)) return false;
    return nbricks < (1L << 31) && nf * g.vol <= ((1L << 40) / per_field);
}
}  // namespace

#define CL_REQUIRE_OPTIONS()                                                                                   \
    MIVP_REQUIRE(B > 0 && C >= 2 && C <= SEG_MAXC && cl_fields_ok((long)B * (C - 1), dims, iterations, 2 * iterations + 8)); \
    MIVP_REQUIRE((long)B * seg_bpb((long)dims[0] * dims[1] * dims[2]) < (1L << 31));                          \
    MIVP_REQUIRE(smooth > 0.f && smooth <= 3.0e38f && lambda_cldice >= 0.f && lambda_cldice <= 3.0e38f);      \
    const ClOpt o = {batch ? 1 : 0, has_ignore ? 1 : 0, (float)ignore_index, smooth, lambda_cldice}

extern "C" size_t mivp_cldice_skeleton_ws(int32_t nf, const int32_t* dims, int32_t iterations, int32_t keep) {
    if (!cl_fields_ok(nf, dims, iterations, 2 * iterations + 4)) return 0;
    return skel_ws_floats((long)nf * dims[0] * dims[1] * dims[2], iterations, keep ? 1 : 0);
}

extern "C" int mivp_cldice_skeleton(const float* x, int32_t nf, const int32_t* dims, int32_t iterations, float* skel,
                                    float* workspace, int32_t keep, mivp_stream_t stream) {
    MIVP_REQUIRE(x && skel && workspace && cl_fields_ok(nf, dims, iterations, 2 * iterations + 4));
    ClGeo g;
    long nbricks;
    cl_geo(dims, g, nbricks);
    const long F = (long)nf * g.vol;
    if (keep)
        return skel_forward(x, nf, workspace, workspace + (long)(iterations + 1) * F, nullptr, nullptr, skel, nullptr, 0, nullptr,
                            nullptr, nullptr, g, nbricks, iterations, (hipStream_t)stream);
    return skel_forward(x, nf, nullptr, nullptr, workspace, workspace + F, skel, nullptr, 0, nullptr, nullptr, nullptr, g, nbricks,
                        iterations, (hipStream_t)stream);
}

extern "C" int mivp_cldice_skeleton_grad(const float* x, const float* gskel, int32_t nf, const int32_t* dims, int32_t iterations,
                                         float* workspace, float* dx, mivp_stream_t stream) {
    MIVP_REQUIRE(x && gskel && workspace && dx && cl_fields_ok(nf, dims, iterations, 2 * iterations + 4));
    ClGeo g;
    long nbricks;
    cl_geo(dims, g, nbricks);
    const ClUp up = {nullptr, nullptr, 1, 2, 0, 0, 0.f};
    return skel_backward(x, nf, workspace, gskel, up, dx, g, nbricks, iterations, (hipStream_t)stream);
}

extern "C" size_t mivp_cldice_ws(int32_t B, int32_t C, const int32_t* dims, int32_t iterations) {
    if (B < 1 || C < 2 || C > SEG_MAXC || !cl_fields_ok((long)B * (C - 1), dims, iterations, 2 * iterations + 8)) return 0;
    return (size_t)ClLayout(B, C - 1, (long)dims[0] * dims[1] * dims[2], iterations).total;
}

extern "C" int mivp_cldice_loss(const float* logits, const float* target, int32_t B, int32_t C, const int32_t* dims,
                                int32_t iterations, float smooth, int32_t batch, int32_t ignore_index, int32_t has_ignore,
                                float lambda_cldice, const float* weight, float* workspace, float* loss, float* dlogits,
                                int32_t accumulate, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && loss);
    CL_REQUIRE_OPTIONS();
    return cldice_run(logits, target, B, C, dims, iterations, o, weight, workspace, loss, nullptr, dlogits, accumulate, true,
                      (hipStream_t)stream);
}

extern "C" int mivp_cldice_loss_grad(const float* logits, const float* target, int32_t B, int32_t C, const int32_t* dims,
                                     int32_t iterations, float smooth, int32_t batch, int32_t ignore_index, int32_t has_ignore,
                                     float lambda_cldice, const float* weight, float* workspace, const float* gscale,
                                     float* dlogits, int32_t accumulate, mivp_stream_t stream) {
    MIVP_REQUIRE(logits && target && workspace && dlogits);
    CL_REQUIRE_OPTIONS();
    return cldice_run(logits, target, B, C, dims, iterations, o, weight, workspace, nullptr, gscale, dlogits, accumulate, false,
                      (hipStream_t)stream);
}
