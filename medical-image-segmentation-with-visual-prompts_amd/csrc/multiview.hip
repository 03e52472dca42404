// Phase-1 multi-view self-supervised step (modules/multi_view.py:115-176, utils.py:267-350,
// losses/contrastive_pair_loss.py): the two (three) views, the reconstruction / mutual MSE terms and the rotation CE +
// NT-Xent heads, with their gradients.  Every reduction is a fixed-order two-stage sum (no float atomics) and every
// per-step input -- rotation codes, keep bits, permutation code, the upstream gradient -- is read from device memory, so a
// recorded graph stays valid when the host refreshes those buffers between replays.
//
// Layouts (all fp32, channels-first, contiguous): x, x_i, x_j, x_k, rec_i, rec_j, rec_k are [B][C][H][W][D].  The model's
// out["reconstruction"] is a channels-first VIEW of channels-last storage; at C = 1 (every configuration of the reference)
// both layouts are the same bytes, otherwise the caller passes a channels-first copy.
// Keep bits: one map per view of n_patches = gh*gw*gd bits (patch (ph, pw, pd) -> bit (ph*gw + pw)*gd + pd of word
// bit >> 5), set = the patch is VISIBLE (the reference's ``~mask``).  Rotation codes int32 [2B]: k_i[0..B) then
// k_j[0..B), the rot90 count in the (H, W) plane.  Permutation code int32 [1]: 0 H<->W, 1 H<->D, 2 W<->D
// (utils.py:295-301).
#include "common.hpp"

namespace {
struct MvGeom {
    int S, D;              // H = W = S (rotation), D innermost
    int mh, mw, md;        // masking patch
    int gw, gd;            // patch grid (gh implied)
};

MIVP_DEV bool keep_bit(const uint32_t* __restrict__ bits, const MvGeom& g, int h, int w, int d) {
    const int p = ((h / g.mh) * g.gw + (w / g.mw)) * g.gd + d / g.md;
    return (bits[p >> 5] >> (p & 31)) & 1u;
}

// output row (h', w') of rot90(x, k, dims=(H, W)) receives input row (h, w) -- torch.rot90 k=1 is flip(W) then transpose
MIVP_DEV void rot_dst(int k, int S, int h, int w, int& ho, int& wo) {
    switch (k & 3) {
        case 0: ho = h; wo = w; break;
        case 1: ho = S - 1 - w; wo = h; break;
        case 2: ho = S - 1 - h; wo = S - 1 - w; break;
        default: ho = w; wo = S - 1 - h; break;
    }
}

// voxel offset inside one [S][S][S] volume of perm(t)[h][w][d]'s source element (each code is its own inverse)
MIVP_DEV long perm_src(int code, int S, int h, int w, int d) {
    const long SS = (long)S * S;
    if (code == 0) return (long)w * SS + (long)h * S + d;
    if (code == 1) return (long)d * SS + (long)w * S + h;
    return (long)h * SS + (long)d * S + w;
}

template <int V>
MIVP_DEV void ld(const float* p, float* v) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int V>
MIVP_DEV void st(float* p, const float* v) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// 1. views: every thread reads V consecutive D voxels of x once and writes them, rotated and masked, into both views
//    (the rotation moves only H and W, so loads and stores are both V*4 bytes per lane along D)
// ---------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_mv_views(const float* __restrict__ x, long n_rows, int C, MvGeom g,
                                                  const int32_t* __restrict__ codes, const uint32_t* __restrict__ keep,
                                                  int nwords, float* __restrict__ xi, float* __restrict__ xj) {
    const int per_row = g.D / V;
    const long items = n_rows * per_row;                     // n_rows = B * C * S * S
    const int B = (int)(n_rows / ((long)C * g.S * g.S));
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
        const long row = it / per_row;
        const int d0 = (int)(it - row * per_row) * V;
        const int w = (int)(row % g.S);
        const int h = (int)((row / g.S) % g.S);
        const long bc = row / ((long)g.S * g.S);
        const int b = (int)(bc / C);
        float v[V], o[V];
        ld<V>(x + row * g.D + d0, v);
#pragma unroll
        for (int view = 0; view < 2; ++view) {
            int ho, wo;
            rot_dst(codes[view * B + b], g.S, h, w, ho, wo);
            const uint32_t* bits = keep + (long)view * nwords;
#pragma unroll
            for (int u = 0; u < V; ++u) o[u] = keep_bit(bits, g, ho, wo, d0 + u) ? v[u] : 0.f;
            st<V>((view ? xj : xi) + ((bc * g.S + ho) * g.S + wo) * g.D + d0, o);
        }
    }
}

// x_k = perm(x_i) on cubes (H = W = D = S).  Code 0 (H<->W) keeps D innermost: a plain V-wide copy of rows.  Codes 1 / 2
// swap an axis with D: 64 x 64 tiles of the (row axis, D) plane go through LDS (row pitch 65: the transposed read walks
// banks).  One grid serves every code (the code is device data): planes x tiles workgroups, code 0 strides over rows.
__global__ __launch_bounds__(256) void k_mv_permute(const float* __restrict__ xi, int BC, int S,
                                                    const int32_t* __restrict__ perm, float* __restrict__ xk) {
    __shared__ float tile[64][65];
    const int code = perm[0];
    const long vol = (long)S * S * S, SS = (long)S * S;
    if (code == 0) {
        const long rows = (long)BC * SS;
        for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
            const long bc = r / SS;
            const int h = (int)((r / S) % S), w = (int)(r % S);
            const float* src = xi + bc * vol + ((long)w * S + h) * S;
            float* dst = xk + r * S;
            for (int d = threadIdx.x & 63; d < S; d += 64) dst[d] = src[d];
        }
        return;
    }
    const int nt = (S + 63) / 64;
    const int t = blockIdx.x % (nt * nt), plane = blockIdx.x / (nt * nt);
    if (plane >= BC * S) return;
    const int ta = t / nt, td = t % nt;
    const long bc = plane / S;
    const int f = plane % S;                                   // the fixed axis: W for code 1, H for code 2
    const long base = bc * vol + (code == 1 ? (long)f * S : (long)f * SS);
    const long rs = code == 1 ? SS : (long)S;                  // stride of the row axis (H for code 1, W for code 2)
    const int c = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < 64; r += 4) {
        const int a = ta * 64 + r, d = td * 64 + c;
        if (a < S && d < S) tile[r][c] = xi[base + a * rs + d];
    }
    __syncthreads();
    for (int r = threadIdx.x >> 6; r < 64; r += 4) {
        const int a = td * 64 + r, d = ta * 64 + c;           // x_k[row a][col d] = x_i[row d][col a]
        if (a < S && d < S) xk[base + a * rs + d] = tile[c][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. reconstruction / mutual MSE.  Per element e of a view batch (N = B*C*H*W*D elements):
//      rec: (rec_v*k_v - x_v*k_v)^2 over both views, mean over 2N, / (1 - ratio)
//      mut: (perm(rec_k)*k_i - rec_i*k_i)^2, mean over N, / (1 - ratio)
//    pass 1 writes per-block partials [nblk][2]; the finalize sums them in a fixed order (double) into vec[0] / vec[3].
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MV_REC_MAX_BLOCKS = 1024;

template <int V>
__global__ __launch_bounds__(256) void k_mv_rec_stats(const float* __restrict__ ri, const float* __restrict__ rj,
                                                      const float* __restrict__ xi, const float* __restrict__ xj,
                                                      const float* __restrict__ rk, long n_rows, int Hh, int Ww, MvGeom g,
                                                      const uint32_t* __restrict__ keep, int nwords,
                                                      const int32_t* __restrict__ perm, int do_rec,
                                                      float* __restrict__ part) {
    __shared__ float red[4][2];
    const int per_row = g.D / V;
    const long items = n_rows * per_row;                     // n_rows = B * C * H * W
    const int code = rk ? perm[0] : 0;
    const long vol = (long)Hh * Ww * g.D;
    float s_rec = 0.f, s_mut = 0.f;
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
        const long row = it / per_row;
        const int d0 = (int)(it - row * per_row) * V;
        const int w = (int)(row % Ww), h = (int)((row / Ww) % Hh);
        const long e = row * g.D + d0;
        float a[V], xa[V], kf_i[V];
#pragma unroll
        for (int u = 0; u < V; ++u) kf_i[u] = keep_bit(keep, g, h, w, d0 + u) ? 1.f : 0.f;
        ld<V>(ri + e, a);
        if (do_rec) {
            float bj[V], xb[V], kf_j[V];
            ld<V>(xi + e, xa);
            ld<V>(rj + e, bj);
            ld<V>(xj + e, xb);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                kf_j[u] = keep_bit(keep + nwords, g, h, w, d0 + u) ? 1.f : 0.f;
                const float di = a[u] * kf_i[u] - xa[u] * kf_i[u], dj = bj[u] * kf_j[u] - xb[u] * kf_j[u];
                s_rec += di * di;
                s_rec += dj * dj;
            }
        }
        if (rk) {
            const long bcv = (row / ((long)Hh * Ww)) * vol;
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float p = rk[bcv + perm_src(code, g.D, h, w, d0 + u)];
                const float dm = p * kf_i[u] - a[u] * kf_i[u];
                s_mut += dm * dm;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) { s_rec += __shfl_xor(s_rec, o); s_mut += __shfl_xor(s_mut, o); }
    if (lane == 0) { red[wave][0] = s_rec; red[wave][1] = s_mut; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int i = threadIdx.x;
        part[(long)blockIdx.x * 2 + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

__global__ void k_mv_rec_finalize(const float* __restrict__ part, int nblk, double n_elem, float inv_keep, int do_rec,
                                  int do_mut, float* __restrict__ vec) {
    // wave 0: the reconstruction sum, wave 1: the mutual sum (lanes stride over the partials, then a butterfly)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double s = 0.0;
    for (int j = lane; j < nblk; j += 64) s += (double)part[2 * j + wv];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        if (wv == 0) vec[0] = do_rec ? (float)(s / (2.0 * n_elem)) / inv_keep : 0.f;
        else vec[3] = do_mut ? (float)(s / n_elem) / inv_keep : 0.f;
    }
}

// gradient pass: d rec_i, d rec_j (element e) and d rec_k (element perm(e): every element of rec_k is written once).
//   grad of rec  w.r.t. rec_v[e] = k_v * 2 (rec_v k_v - x_v k_v) * gr,   gr = g w_rec / (1 - ratio) / (2N)
//   grad of mut  w.r.t. rec_i[e] = k_i * 2 (rec_i k_i - P k_i) * gm,     gm = g / (1 - ratio) / N,   P = perm(rec_k)[e]
//                w.r.t. P[e]     = k_i * 2 (P k_i - rec_i k_i) * gm
template <int V>
__global__ __launch_bounds__(256) void k_mv_rec_grad(const float* __restrict__ ri, const float* __restrict__ rj,
                                                     const float* __restrict__ xi, const float* __restrict__ xj,
                                                     const float* __restrict__ rk, long n_rows, int Hh, int Ww, MvGeom g,
                                                     const uint32_t* __restrict__ keep, int nwords,
                                                     const int32_t* __restrict__ perm, int do_rec,
                                                     const float* __restrict__ gscale, float w_rec, float inv_keep,
                                                     double n_elem, float* __restrict__ dri, float* __restrict__ drj,
                                                     float* __restrict__ drk) {
    const int per_row = g.D / V;
    const long items = n_rows * per_row;
    const int code = rk ? perm[0] : 0;
    const long vol = (long)Hh * Ww * g.D;
    const float up = gscale ? gscale[0] : 1.f;
    const float gr = (float)((double)((up * w_rec) / inv_keep) / (2.0 * n_elem));
    const float gm = (float)((double)(up / inv_keep) / n_elem);
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
        const long row = it / per_row;
        const int d0 = (int)(it - row * per_row) * V;
        const int w = (int)(row % Ww), h = (int)((row / Ww) % Hh);
        const long e = row * g.D + d0;
        float a[V], kf_i[V], gi[V];
#pragma unroll
        for (int u = 0; u < V; ++u) { kf_i[u] = keep_bit(keep, g, h, w, d0 + u) ? 1.f : 0.f; gi[u] = 0.f; }
        ld<V>(ri + e, a);
        if (do_rec) {
            float xa[V], bj[V], xb[V], gj[V];
            ld<V>(xi + e, xa);
            ld<V>(rj + e, bj);
            ld<V>(xj + e, xb);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float kj = keep_bit(keep + nwords, g, h, w, d0 + u) ? 1.f : 0.f;
                gi[u] = kf_i[u] * (2.f * (a[u] * kf_i[u] - xa[u] * kf_i[u]) * gr);
                gj[u] = kj * (2.f * (bj[u] * kj - xb[u] * kj) * gr);
            }
            st<V>(drj + e, gj);
        }
        if (rk) {
            const long bcv = (row / ((long)Hh * Ww)) * vol;
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const long src = bcv + perm_src(code, g.D, h, w, d0 + u);
                const float p = rk[src];
                const float dm = 2.f * (p * kf_i[u] - a[u] * kf_i[u]) * gm;
                gi[u] -= kf_i[u] * dm;
                drk[src] = kf_i[u] * dm;
            }
        }
        st<V>(dri + e, gi);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. heads: rotation CE over the 2B rows and NT-Xent (ContrastivePairLoss) of (z_i, z_j), one workgroup of 1024 threads.
//    u = x / max(|x|, 1e-12) (F.normalize), w = u / max(|u|, 1e-8) (cosine_similarity), s_ab = w_a . w_b;
//    l_a = -log(exp(s_a,pos / T) / sum_{b != a} exp(s_ab / T)), pos(a) = (a + B) mod 2B; con = sum_a l_a / (2B).
//    d con / d s_ab = (p_ab - [b == pos(a)]) / (T 2B), p_ab the softmax of row a over b != a;  d w_a = sum_b H_ab w_b with
//    H = G + G^T;  d x_a = (d w_a - w_a (w_a . d w_a)) / (|u_a| |x_a|)  (the two normalisations compose, u is parallel to w).
//    workspace: w [2B][dim], dw [2B][dim] (global, L2 resident); the 2B x 2B similarity and H live in LDS.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MV_MAX_ROWS = 64;
constexpr int MV_MAX_DIM = 1024;

__global__ __launch_bounds__(1024) void k_mv_heads(const float* __restrict__ zi, const float* __restrict__ zj, int B,
                                                   int dim, float temp, const float* __restrict__ roti,
                                                   const float* __restrict__ rotj, const int32_t* __restrict__ codes,
                                                   float w_rec, float w_rot, float w_con, int has_recmut,
                                                   float* __restrict__ ws, const float* __restrict__ gscale,
                                                   float* __restrict__ dzi, float* __restrict__ dzj,
                                                   float* __restrict__ droti, float* __restrict__ drotj,
                                                   float* __restrict__ vec) {
    __shared__ float sim[MV_MAX_ROWS][MV_MAX_ROWS + 1];
    __shared__ float hm[MV_MAX_ROWS][MV_MAX_ROWS + 1];
    __shared__ float nrm[MV_MAX_ROWS][2];                      // |x_a| clamped, |u_a| clamped
    __shared__ float dots[MV_MAX_ROWS];
    __shared__ float rowv[MV_MAX_ROWS];
    __shared__ float rotv[MV_MAX_ROWS];
    const int n = 2 * B, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nwv = blockDim.x >> 6;
    const bool grad = dzi != nullptr || droti != nullptr;
    const float up = grad ? (gscale ? gscale[0] : 1.f) : 1.f;
    float* wbuf = ws;
    float* dwbuf = ws + (long)n * dim;
    // ---- rotation CE (log_softmax over 4 logits per row)
    if (roti && tid < n) {
        const float* l = tid < B ? roti + 4 * tid : rotj + 4 * (tid - B);
        const int y = codes[tid] & 3;
        const float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
        float e[4], s = 0.f;
        for (int c = 0; c < 4; ++c) { e[c] = expf(l[c] - mx); s += e[c]; }
        const float lse = mx + logf(s);
        rotv[tid] = lse - l[y];
        if (grad && droti) {
            float* dl = tid < B ? droti + 4 * tid : drotj + 4 * (tid - B);
            const float sc = up * w_rot / (float)n;
            for (int c = 0; c < 4; ++c) dl[c] = (e[c] / s - (c == y ? 1.f : 0.f)) * sc;
        }
    }
    if (zi) {
        // ---- the two normalisations, one wave per row
        for (int a = wv; a < n; a += nwv) {
            const float* x = a < B ? zi + (long)a * dim : zj + (long)(a - B) * dim;
            float s = 0.f;
            for (int k = lane; k < dim; k += 64) s += x[k] * x[k];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const float n1 = fmaxf(sqrtf(s), 1e-12f);
            float s2 = 0.f;
            for (int k = lane; k < dim; k += 64) { const float u = x[k] / n1; s2 += u * u; }
            for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
            const float n2 = fmaxf(sqrtf(s2), 1e-8f);
            for (int k = lane; k < dim; k += 64) wbuf[(long)a * dim + k] = (x[k] / n1) / n2;
            if (lane == 0) { nrm[a][0] = n1; nrm[a][1] = n2; }
        }
        __syncthreads();
        // ---- similarity (upper triangle, mirrored: w_a . w_b and w_b . w_a are the same products)
        for (int p = wv; p < n * n; p += nwv) {
            const int a = p / n, b = p % n;
            if (b < a) continue;
            float s = 0.f;
            for (int k = lane; k < dim; k += 64) s += wbuf[(long)a * dim + k] * wbuf[(long)b * dim + k];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) { sim[a][b] = s; sim[b][a] = s; }
        }
        __syncthreads();
        // ---- per-row loss and d con / d s
        if (tid < n) {
            const int a = tid, pos = a < B ? a + B : a - B;
            float den = 0.f;
            for (int b = 0; b < n; ++b)
                if (b != a) den += expf(sim[a][b] / temp);
            const float ep = expf(sim[a][pos] / temp);
            rowv[a] = -logf(ep / den);
            for (int b = 0; b < n; ++b)
                hm[a][b] = b == a ? 0.f : (expf(sim[a][b] / temp) / den - (b == pos ? 1.f : 0.f)) / (temp * (float)n);
        }
        __syncthreads();
        if (grad && dzi) {
            // ---- d w_a = sum_b (G_ab + G_ba) w_b
            const float sc = up * w_con;
            for (long q = tid; q < (long)n * dim; q += blockDim.x) {
                const int a = (int)(q / dim), k = (int)(q % dim);
                float s = 0.f;
                for (int b = 0; b < n; ++b) s += (hm[a][b] + hm[b][a]) * wbuf[(long)b * dim + k];
                dwbuf[q] = s * sc;
            }
            __syncthreads();
            for (int a = wv; a < n; a += nwv) {
                float s = 0.f;
                for (int k = lane; k < dim; k += 64) s += wbuf[(long)a * dim + k] * dwbuf[(long)a * dim + k];
                for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
                if (lane == 0) dots[a] = s;
            }
            __syncthreads();
            for (long q = tid; q < (long)n * dim; q += blockDim.x) {
                const int a = (int)(q / dim), k = (int)(q % dim);
                const float v = (dwbuf[q] - wbuf[q] * dots[a]) / nrm[a][1] / nrm[a][0];
                if (a < B) dzi[(long)a * dim + k] = v;
                else dzj[(long)(a - B) * dim + k] = v;
            }
        }
    }
    __syncthreads();
    if (!grad && tid == 0) {
        float rot = 0.f, con = 0.f;
        if (roti) {
            for (int a = 0; a < n; ++a) rot += rotv[a];
            rot /= (float)n;
        }
        if (zi) {
            for (int a = 0; a < n; ++a) con += rowv[a];
            con /= (float)n;
        }
        const float rec = has_recmut ? vec[0] : 0.f, mut = has_recmut ? vec[3] : 0.f;
        if (!has_recmut) { vec[0] = 0.f; vec[3] = 0.f; }
        vec[1] = rot;
        vec[2] = con;
        vec[4] = w_rec * rec + w_rot * rot + w_con * con + mut;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
static MvGeom mv_geom(const int32_t* dims, const int32_t* mshape) {
    MvGeom g;
    g.S = dims[1];
    g.D = dims[2];
    g.mh = mshape[0]; g.mw = mshape[1]; g.md = mshape[2];
    g.gw = dims[1] / mshape[1];
    g.gd = dims[2] / mshape[2];
    return g;
}

static int mv_shape_ok(const int32_t* dims, const int32_t* mshape) {
    for (int a = 0; a < 3; ++a)
        if (dims[a] <= 0 || mshape[a] <= 0 || dims[a] % mshape[a]) return 0;
    return 1;
}

static int mv_nwords(const int32_t* dims, const int32_t* mshape) {
    const long np = (long)(dims[0] / mshape[0]) * (dims[1] / mshape[1]) * (dims[2] / mshape[2]);
    return (int)((np + 31) / 32);
}

static unsigned mv_grid(long items, long cap) {
    const long g = (items + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" int mivp_mv_views(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* mshape,
                             const int32_t* codes, const void* keep, const int32_t* perm, float* xi, float* xj, float* xk,
                             mivp_stream_t stream) {
    MIVP_REQUIRE(x && dims && mshape && codes && keep && xi && xj);
    MIVP_REQUIRE(B > 0 && C > 0 && dims[0] == dims[1] && mv_shape_ok(dims, mshape));
    MIVP_REQUIRE(!xk || (perm && dims[2] == dims[0]));
    hipStream_t st = (hipStream_t)stream;
    const MvGeom g = mv_geom(dims, mshape);
    const long n_rows = (long)B * C * dims[0] * dims[1];
    const int nw = mv_nwords(dims, mshape);
    const uint32_t* bits = (const uint32_t*)keep;
    if (g.D % 4 == 0)
        hipLaunchKernelGGL(k_mv_views<4>, dim3(mv_grid(n_rows * g.D / 4, 8192)), dim3(256), 0, st, x, n_rows, (int)C, g,
                           codes, bits, nw, xi, xj);
    else
        hipLaunchKernelGGL(k_mv_views<1>, dim3(mv_grid(n_rows * g.D, 8192)), dim3(256), 0, st, x, n_rows, (int)C, g, codes,
                           bits, nw, xi, xj);
    int rc = mivp_check_launch("mv_views");
    if (rc || !xk) return rc;
    const int S = dims[0], nt = (S + 63) / 64;
    hipLaunchKernelGGL(k_mv_permute, dim3((unsigned)((long)B * C * S * nt * nt)), dim3(256), 0, st, xi, (int)(B * C), S,
                       perm, xk);
    return mivp_check_launch("mv_permute");
}

extern "C" size_t mivp_mv_rec_ws(void) { return (size_t)MV_REC_MAX_BLOCKS * 2; }

extern "C" int mivp_mv_rec_loss(const float* ri, const float* rj, const float* xi, const float* xj, const float* rk,
                                int32_t B, int32_t C, const int32_t* dims, const int32_t* mshape, const void* keep,
                                const int32_t* perm, int32_t do_rec, float ratio, float* workspace, float* vec,
                                mivp_stream_t stream) {
    MIVP_REQUIRE(ri && workspace && vec && keep && dims && mshape && mv_shape_ok(dims, mshape));
    MIVP_REQUIRE(!do_rec || (rj && xi && xj));
    MIVP_REQUIRE(!rk || (perm && dims[0] == dims[1] && dims[1] == dims[2]));
    MIVP_REQUIRE(B > 0 && C > 0 && ratio < 1.f);
    hipStream_t st = (hipStream_t)stream;
    MvGeom g = mv_geom(dims, mshape);
    const long n_rows = (long)B * C * dims[0] * dims[1];
    const int nw = mv_nwords(dims, mshape);
    const uint32_t* bits = (const uint32_t*)keep;
    const int V = g.D % 4 == 0 ? 4 : 1;
    const unsigned grid = mv_grid(n_rows * g.D / V, MV_REC_MAX_BLOCKS);
    if (V == 4)
        hipLaunchKernelGGL(k_mv_rec_stats<4>, dim3(grid), dim3(256), 0, st, ri, rj, xi, xj, rk, n_rows, (int)dims[0],
                           (int)dims[1], g, bits, nw, perm, (int)do_rec, workspace);
    else
        hipLaunchKernelGGL(k_mv_rec_stats<1>, dim3(grid), dim3(256), 0, st, ri, rj, xi, xj, rk, n_rows, (int)dims[0],
                           (int)dims[1], g, bits, nw, perm, (int)do_rec, workspace);
    int rc = mivp_check_launch("mv_rec_stats");
    if (rc) return rc;
    hipLaunchKernelGGL(k_mv_rec_finalize, dim3(1), dim3(128), 0, st, workspace, (int)grid, (double)n_rows * g.D,
                       1.f - ratio, (int)do_rec, rk ? 1 : 0, vec);
    return mivp_check_launch("mv_rec_finalize");
}

extern "C" int mivp_mv_rec_grad(const float* ri, const float* rj, const float* xi, const float* xj, const float* rk,
                                int32_t B, int32_t C, const int32_t* dims, const int32_t* mshape, const void* keep,
                                const int32_t* perm, int32_t do_rec, float ratio, float w_rec, const float* gscale,
                                float* dri, float* drj, float* drk, mivp_stream_t stream) {
    MIVP_REQUIRE(ri && dri && keep && dims && mshape && mv_shape_ok(dims, mshape));
    MIVP_REQUIRE(!do_rec || (rj && xi && xj && drj));
    MIVP_REQUIRE(!rk || (perm && drk && dims[0] == dims[1] && dims[1] == dims[2]));
    MIVP_REQUIRE(B > 0 && C > 0 && ratio < 1.f);
    hipStream_t st = (hipStream_t)stream;
    MvGeom g = mv_geom(dims, mshape);
    const long n_rows = (long)B * C * dims[0] * dims[1];
    const int nw = mv_nwords(dims, mshape);
    const uint32_t* bits = (const uint32_t*)keep;
    const double n_elem = (double)n_rows * g.D;
    if (g.D % 4 == 0)
        hipLaunchKernelGGL(k_mv_rec_grad<4>, dim3(mv_grid(n_rows * g.D / 4, 8192)), dim3(256), 0, st, ri, rj, xi, xj, rk,
                           n_rows, (int)dims[0], (int)dims[1], g, bits, nw, perm, (int)do_rec, gscale, w_rec, 1.f - ratio,
                           n_elem, dri, drj, drk);
    else
        hipLaunchKernelGGL(k_mv_rec_grad<1>, dim3(mv_grid(n_rows * g.D, 8192)), dim3(256), 0, st, ri, rj, xi, xj, rk,
                           n_rows, (int)dims[0], (int)dims[1], g, bits, nw, perm, (int)do_rec, gscale, w_rec, 1.f - ratio,
                           n_elem, dri, drj, drk);
    return mivp_check_launch("mv_rec_grad");
}

extern "C" size_t mivp_mv_heads_ws(int32_t B, int32_t dim) { return (size_t)4 * B * (dim > 0 ? dim : 1); }

extern "C" int mivp_mv_heads(const float* zi, const float* zj, int32_t B, int32_t dim, float temp, const float* roti,
                             const float* rotj, const int32_t* codes, float w_rec, float w_rot, float w_con,
                             int32_t has_recmut, float* workspace, const float* gscale, float* dzi, float* dzj,
                             float* droti, float* drotj, float* vec, mivp_stream_t stream) {
    MIVP_REQUIRE(B > 0 && 2 * B <= MV_MAX_ROWS);
    MIVP_REQUIRE(!zi || (zj && workspace && dim > 0 && dim <= MV_MAX_DIM && temp > 0.f));
    MIVP_REQUIRE(!roti || (rotj && codes));
    MIVP_REQUIRE(!dzi || (zi && dzj));
    MIVP_REQUIRE(!droti || (roti && drotj));
    const bool grad = dzi || droti;
    MIVP_REQUIRE(grad || vec);
    hipLaunchKernelGGL(k_mv_heads, dim3(1), dim3(1024), 0, (hipStream_t)stream, zi, zj, (int)B, (int)dim, temp, roti, rotj,
                       codes, w_rec, w_rot, w_con, (int)has_recmut, workspace, gscale, dzi, dzj, droti, drotj, vec);
    return mivp_check_launch("mv_heads");
}
