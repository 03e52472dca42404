// Random intensity augmentation of a resident batch (mivp_amd/augment.py): the reference's ``basic_rand_ts``
// chain -- bias field, std shift, gamma contrast, scale, histogram shift -- on a contiguous fp32 [B][C][H][W][D] batch, each
// step gated per sample by a flag the host drew.  Everything a launch needs beyond the batch is DEVICE memory (the slot:
// one record of REC words per sample, and the partials workspace), so both launches record into a graph and a replay
// picks up whatever the host loaded into the slot since.
//
//   record (int32 / fp32 words): [0] flags  [1] n control points  [2] shift factor  [3] gamma  [4] scale factor
//                                [5..24] bias coefficients c[i][j][k], i + j + k <= 3, i outer, k inner
//                                [25..36] floating control points (n of them, non-decreasing, 0 .. 1)
//
// A sample is walked as ITEMS: item = (row, q), row = (c, h, w), q = a group of four voxels along D (the last one of a row
// holds D % 4 of them and is read voxel by voxel).  G = groups_of(voxels) workgroups share a sample, each a contiguous run of
// items; G depends on the shape alone, so the partials and their merge order never change from run to run.
//
//   k_intensity_stats: per workgroup (min, max, count, mean, M2) of v = x * exp(field) (v = x without the bias flag) -- a
//     mean / M2 pair per item, merged Chan-style into the thread's running pair, then lanes (shuffle tree), then waves.
//   k_intensity_apply: every workgroup merges its sample's G partials in the same fixed order, thread 0 turns them into the
//     scalar plan (below), then the items stream x -> out.  A sample without flags is a plain copy.
//
// The bias field exp(sum c_ijk P_i(h) P_j(w) P_k(d)) is never stored: a row collapses it to A_k = sum_ij c_ijk P_i(h) P_j(w)
// (20 FMAs per item), a voxel costs four FMAs and one expf.  bias_value() is the ONE definition both kernels use, so the
// extremes the statistics see are bitwise the values the apply pass transforms.  The same holds for the rest of the chain:
// the plan pushes the minimum and the maximum through pre_hist() -- the per-voxel function -- which is monotone (a negative
// scale swaps them), so the histogram knots sit exactly on the extremes of what reaches that step.
#include "common.hpp"
#include <math.h>

namespace {
constexpr int TPB = 256;
constexpr int REC = 40;                  // words per sample record
constexpr int MAXG = 256;                // workgroups per sample at most (= TPB: one partial per thread in the merge)
constexpr long GROUP_VOX = 4096;         // voxels per workgroup until MAXG is reached
constexpr int PART = 8;                  // floats per partial: min, max, count, mean, M2, 3 unused
constexpr int MAXCP = 12;
enum { F_BIAS = 1, F_SHIFT = 2, F_CONTRAST = 4, F_SCALE = 8, F_HIST = 16, F_ALL = 31, F_STATS = F_SHIFT | F_CONTRAST | F_HIST };
enum { R_FLAGS = 0, R_NCP = 1, R_SHIFT = 2, R_GAMMA = 3, R_SCALE = 4, R_COEF = 5, R_FLOAT = 25 };

typedef f32x4 f32x4u __attribute__((aligned(4)));      // four voxels of a row: rows start at any multiple of 4 bytes

struct Geo {
    int C, H, W, D, Q;       // Q = items per row
    int G;                   // workgroups per sample
    unsigned rows, items, chunk;
    long nvox;               // voxels per sample
    float sh, sw, sd;        // linspace(-1, 1, dim) steps (0 for an axis of length 1, which sits at -1)
};

struct Stat { float mn, mx, n, mean, m2; };

MIVP_DEV Stat stat_empty() { return Stat{INFINITY, -INFINITY, 0.f, 0.f, 0.f}; }
// a then b (Chan et al.); an empty side has n = 0 and mean = 0, which the formulas pass through exactly
MIVP_DEV Stat stat_merge(const Stat& a, const Stat& b) {
    Stat r;
    r.mn = fminf(a.mn, b.mn);
    r.mx = fmaxf(a.mx, b.mx);
    r.n = a.n + b.n;
    const float inv = 1.f / fmaxf(r.n, 1.f);
    const float d = b.mean - a.mean;
    r.mean = fmaf(d, b.n * inv, a.mean);
    r.m2 = fmaf(d * d, a.n * b.n * inv, a.m2 + b.m2);
    return r;
}
MIVP_DEV Stat stat_shfl_down(const Stat& s, int off) {
    return Stat{__shfl_down(s.mn, off), __shfl_down(s.mx, off), __shfl_down(s.n, off), __shfl_down(s.mean, off),
                __shfl_down(s.m2, off)};
}
// lanes in a fixed tree, then the four waves in order; the result is valid in thread 0
MIVP_DEV Stat stat_block_reduce(Stat s, Stat* lds4) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s = stat_merge(s, stat_shfl_down(s, off));
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = s;
    __syncthreads();
    Stat r = lds4[0];
#pragma unroll
    for (int w = 1; w < TPB / 64; ++w) r = stat_merge(r, lds4[w]);
    return r;
}

MIVP_DEV void legendre(float t, float (&p)[4]) {
    const float t2 = t * t;
    p[0] = 1.f;
    p[1] = t;
    p[2] = fmaf(1.5f, t2, -0.5f);
    p[3] = t * fmaf(2.5f, t2, -1.5f);
}
MIVP_DEV float coord(int i, float step) { return fmaf((float)i, step, -1.f); }
// A_k = sum_ij c_ijk P_i(h) P_j(w)
MIVP_DEV void row_field(const float* cs, float th, float tw, float (&A)[4]) {
    float ph[4], pw[4];
    legendre(th, ph);
    legendre(tw, pw);
    A[0] = A[1] = A[2] = A[3] = 0.f;
    int idx = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4 - i; ++j) {
            const float hw = ph[i] * pw[j];
#pragma unroll
            for (int k = 0; k < 4 - i - j; ++k) A[k] = fmaf(cs[idx++], hw, A[k]);
        }
}
MIVP_DEV float bias_value(float x, const float (&A)[4], float td) {
    float pd[4];
    legendre(td, pd);
    const float f = fmaf(A[3], pd[3], fmaf(A[2], pd[2], fmaf(A[1], pd[1], A[0])));
    return x * expf(f);
}

// the scalar plan of one sample (LDS)
struct Plan {
    int flags;                 // the steps that run (the histogram bit is cleared when min == max at that step)
    int ncp;
    float shift;               // f * std
    float cmin, crange, cden, gamma;
    float scale;               // 1 + f
    float xp[MAXCP], yp[MAXCP], slope[MAXCP];
};

// std shift, contrast and scale of one voxel: every operation monotone in v (for scale < 0: decreasing)
MIVP_DEV float pre_hist(float v, int flags, float shift, float cmin, float crange, float cden, float gamma, float scale) {
    if (flags & F_SHIFT) v = v + shift;
    if (flags & F_CONTRAST) v = fmaf(powf((v - cmin) / cden, gamma), crange, cmin);
    if (flags & F_SCALE) v = v * scale;
    return v;
}
// np.interp: yp[0] at and below xp[0], yp[n-1] at and above xp[n-1], slope_j (v - xp_j) + yp_j on xp_j <= v < xp_j+1
MIVP_DEV float hist_value(float v, const Plan& P) {
    const int n = P.ncp;
    int j = 0;
    for (int k = 1; k < n - 1; ++k) j += v >= P.xp[k] ? 1 : 0;
    float r = fmaf(P.slope[j], v - P.xp[j], P.yp[j]);
    r = v <= P.xp[0] ? P.yp[0] : r;
    return v >= P.xp[n - 1] ? P.yp[n - 1] : r;
}

struct Item { unsigned row; int d0, cnt; long off; };
MIVP_DEV Item item_of(unsigned it, const Geo& g) {
    Item m;
    m.row = it / (unsigned)g.Q;
    m.d0 = 4 * (int)(it - m.row * (unsigned)g.Q);
    m.cnt = min(4, g.D - m.d0);
    m.off = (long)m.row * g.D + m.d0;
    return m;
}
MIVP_DEV void item_coords(const Item& m, const Geo& g, float& th, float& tw) {
    const unsigned hw = m.row % (unsigned)(g.H * g.W);
    const unsigned h = hw / (unsigned)g.W;
    th = coord((int)h, g.sh);
    tw = coord((int)(hw - h * (unsigned)g.W), g.sw);
}
MIVP_DEV void item_load(const float* p, int cnt, float (&v)[4]) {
    if (cnt == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4u*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[j] : 0.f;
    }
}

__global__ __launch_bounds__(TPB) void k_intensity_stats(const float* __restrict__ x, Geo g, const int* __restrict__ slot,
                                                         float* __restrict__ ws) {
    __shared__ float cs[20];
    __shared__ Stat red[TPB / 64];
    const int b = blockIdx.y, wg = blockIdx.x;
    const int* rec = slot + (long)b * REC;
    const int flags = rec[R_FLAGS] & F_ALL;
    if (!(flags & F_STATS)) return;
    const bool bias = flags & F_BIAS;
    if (threadIdx.x < 20) cs[threadIdx.x] = __int_as_float(rec[R_COEF + threadIdx.x]);
    __syncthreads();
    const float* xs = x + (long)b * g.nvox;
    const unsigned i0 = min((unsigned)wg * g.chunk, g.items), i1 = min(i0 + g.chunk, g.items);
    Stat s = stat_empty();
    for (unsigned it = i0 + threadIdx.x; it < i1; it += TPB) {
        const Item m = item_of(it, g);
        float v[4];
        item_load(xs + m.off, m.cnt, v);
        if (bias) {
            float th, tw, A[4];
            item_coords(m, g, th, tw);
            row_field(cs, th, tw, A);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = bias_value(v[j], A, coord(m.d0 + j, g.sd));
        }
        // the item's own (min, max, count, mean, M2), then one merge
        Stat t = stat_empty();
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < m.cnt) { t.mn = fminf(t.mn, v[j]); t.mx = fmaxf(t.mx, v[j]); sum += v[j]; }
        t.n = (float)m.cnt;
        t.mean = sum / t.n;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < m.cnt) { const float d = v[j] - t.mean; t.m2 = fmaf(d, d, t.m2); }
        s = stat_merge(s, t);
    }
    s = stat_block_reduce(s, red);
    if (threadIdx.x == 0) {
        float* p = ws + ((long)b * g.G + wg) * PART;
        p[0] = s.mn; p[1] = s.mx; p[2] = s.n; p[3] = s.mean; p[4] = s.m2;
    }
}

// (x and out may be the same buffer: every voxel is read and written by one thread, read first)
__global__ __launch_bounds__(TPB) void k_intensity_apply(const float* x, Geo g, const int* __restrict__ slot,
                                                         const float* __restrict__ ws, float* out) {
    __shared__ float cs[20];
    __shared__ Stat red[TPB / 64];
    __shared__ Plan P;
    const int b = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x;
    const int* rec = slot + (long)b * REC;
    const int flags = rec[R_FLAGS] & F_ALL;
    const float* xs = x + (long)b * g.nvox;
    float* os = out + (long)b * g.nvox;
    const unsigned i0 = min((unsigned)wg * g.chunk, g.items), i1 = min(i0 + g.chunk, g.items);
    if (flags == 0) {                                             // bit-for-bit copy (nothing to do in place)
        if (xs == os) return;
        for (unsigned it = i0 + tid; it < i1; it += TPB) {
            const Item m = item_of(it, g);
            if (m.cnt == 4) {
                *reinterpret_cast<f32x4u*>(os + m.off) = *reinterpret_cast<const f32x4u*>(xs + m.off);
            } else {
                for (int j = 0; j < m.cnt; ++j) os[m.off + j] = xs[m.off + j];
            }
        }
        return;
    }
    if (tid < 20) cs[tid] = __int_as_float(rec[R_COEF + tid]);
    Stat s = stat_empty();
    if ((flags & F_STATS) && tid < g.G) {
        const float* p = ws + ((long)b * g.G + tid) * PART;
        s = Stat{p[0], p[1], p[2], p[3], p[4]};
    }
    s = stat_block_reduce(s, red);                                // (its barrier also publishes cs)
    if (tid == 0) {
        P.flags = flags;
        P.shift = P.cmin = P.crange = 0.f;
        P.cden = P.gamma = P.scale = 1.f;
        float lo = s.mn, hi = s.mx;
        if (flags & F_SHIFT) {                                    // population std of v
            P.shift = __int_as_float(rec[R_SHIFT]) * (float)sqrt((double)s.m2 / (double)g.nvox);
            lo = lo + P.shift;
            hi = hi + P.shift;
        }
        if (flags & F_CONTRAST) {
            P.cmin = lo;
            P.crange = hi - lo;
            P.cden = P.crange + 1e-7f;
            P.gamma = __int_as_float(rec[R_GAMMA]);
        }
        if (flags & F_SCALE) P.scale = 1.f + __int_as_float(rec[R_SCALE]);
        const int pre = flags & (F_CONTRAST | F_SCALE);           // (the shift is already in lo and hi)
        const float a = pre_hist(lo, pre, 0.f, P.cmin, P.crange, P.cden, P.gamma, P.scale);
        const float c = pre_hist(hi, pre, 0.f, P.cmin, P.crange, P.cden, P.gamma, P.scale);
        lo = fminf(a, c);
        hi = fmaxf(a, c);
        int n = rec[R_NCP];
        n = n < 2 ? 2 : (n > MAXCP ? MAXCP : n);
        P.ncp = n;
        if (flags & F_HIST) {
            if (lo == hi || !(hi - lo < INFINITY)) {
                P.flags &= ~F_HIST;                               // min == max: the values pass through unchanged
            } else {
                const double w = (double)hi - (double)lo;
                for (int k = 0; k < n; ++k) {
                    P.xp[k] = (float)((double)k / (double)(n - 1) * w + (double)lo);
                    P.yp[k] = (float)((double)__int_as_float(rec[R_FLOAT + k]) * w + (double)lo);
                }
                for (int k = 0; k + 1 < n; ++k) {                  // (two knots on one float: that segment is never selected)
                    const double dx = (double)P.xp[k + 1] - (double)P.xp[k];
                    P.slope[k] = dx > 0.0 ? (float)(((double)P.yp[k + 1] - (double)P.yp[k]) / dx) : 0.f;
                }
                P.slope[n - 1] = 0.f;
            }
        }
    }
    __syncthreads();
    const int fl = P.flags;
    const float shift = P.shift, cmin = P.cmin, crange = P.crange, cden = P.cden, gamma = P.gamma, scale = P.scale;
    const bool bias = fl & F_BIAS, hist = fl & F_HIST;
    for (unsigned it = i0 + tid; it < i1; it += TPB) {
        const Item m = item_of(it, g);
        float v[4];
        item_load(xs + m.off, m.cnt, v);
        if (bias) {
            float th, tw, A[4];
            item_coords(m, g, th, tw);
            row_field(cs, th, tw, A);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = bias_value(v[j], A, coord(m.d0 + j, g.sd));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = pre_hist(v[j], fl, shift, cmin, crange, cden, gamma, scale);
            if (hist) v[j] = hist_value(v[j], P);
        }
        if (m.cnt == 4) {
            f32x4 t = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4u*>(os + m.off) = t;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < m.cnt) os[m.off + j] = v[j];
        }
    }
}

int groups_of(long nvox) {
    const long g = (nvox + GROUP_VOX - 1) / GROUP_VOX;
    return (int)(g < 1 ? 1 : (g > MAXG ? MAXG : g));
}

bool fill_geo(Geo& g, int32_t B, int32_t C, const int32_t* dims) {
    if (!dims || B < 1 || B > 65535 || C < 1 || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    const long rows = (long)C * dims[0] * dims[1];
    g.C = C; g.H = dims[0]; g.W = dims[1]; g.D = dims[2];
    g.Q = (g.D + 3) / 4;
    g.nvox = rows * g.D;
    if (g.nvox >= (1L << 31) || rows * g.Q >= (1L << 31)) return false;    // items and rows are 32-bit in the kernels
    g.rows = (unsigned)rows;
    g.items = (unsigned)(rows * g.Q);
    g.G = groups_of(g.nvox);
    g.chunk = (g.items + g.G - 1) / g.G;
    g.sh = g.H > 1 ? 2.f / (float)(g.H - 1) : 0.f;
    g.sw = g.W > 1 ? 2.f / (float)(g.W - 1) : 0.f;
    g.sd = g.D > 1 ? 2.f / (float)(g.D - 1) : 0.f;
    return true;
}
}  // namespace

extern "C" size_t mivp_intensity_ws(int32_t B, int64_t voxels_per_sample) {
    if (B < 1 || voxels_per_sample < 1) return 0;
    return (size_t)B * groups_of((long)voxels_per_sample) * PART * sizeof(float);
}

extern "C" int mivp_intensity_stats(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* slot,
                                    void* workspace, size_t workspace_bytes, mivp_stream_t stream) {
    MIVP_REQUIRE(x && slot && workspace && ((uintptr_t)x & 3) == 0 && ((uintptr_t)workspace & 3) == 0);
    Geo g;
    MIVP_REQUIRE(fill_geo(g, B, C, dims));
    MIVP_REQUIRE(workspace_bytes >= mivp_intensity_ws(B, g.nvox));
    hipLaunchKernelGGL(k_intensity_stats, dim3((unsigned)g.G, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, x, g,
                       (const int*)slot, (float*)workspace);
    return mivp_check_launch("intensity_stats");
}

extern "C" int mivp_intensity_apply(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* slot,
                                    const void* workspace, size_t workspace_bytes, float* out, mivp_stream_t stream) {
    MIVP_REQUIRE(x && out && slot && workspace && ((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0);
    Geo g;
    MIVP_REQUIRE(fill_geo(g, B, C, dims));
    MIVP_REQUIRE(workspace_bytes >= mivp_intensity_ws(B, g.nvox));
    hipLaunchKernelGGL(k_intensity_apply, dim3((unsigned)g.G, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, x, g,
                       (const int*)slot, (const float*)workspace, out);
    return mivp_check_launch("intensity_apply");
}
