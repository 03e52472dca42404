// Neighbourhood augmentation of a resident batch (mivp_amd/augment.py): additive Gaussian noise, separable
// Gaussian blur with zero padding, and low-resolution simulation (nearest down, trilinear up) on a contiguous fp32
// [B][C][H][W][D] batch, each step gated per sample by a flag the host drew.  As in intensity.hip everything a launch needs
// beyond the batch is DEVICE memory (the slot: one record of REC words per sample, and two batch-sized temporaries), so the
// three launches record into a graph and a replay picks up whatever the host loaded into the slot since.
//
//   record (int32 / fp32 words): [0] flags (1 noise, 2 smooth, 4 low-res)  [1] noise key  [2] noise mean  [3] noise std
//                                [4..6] radius of axis H, W, D (0..8, 0 = axis not filtered)  [7..9] low-resolution grid
//                                [10..60] taps [3][17], tap k of axis a at 10 + 17 a + 8 + k  [61..63] unused
//
//   k_filter_dw:     one workgroup = a tile of TW rows x TD voxels of one (c, h) plane.  It stages the tile with a halo of
//                    the sample's OWN radii (the LDS is sized for radius 8), adding the noise while staging, runs the D pass
//                    LDS -> LDS on the tile's rows and their W halo, then the W pass LDS -> global.
//   k_filter_h:      the H pass on the view [C][H][W * D]: a tile of 32 x 64, staged with its H halo.
//   k_filter_lowres: one thread per output voxel blends the eight corners of the low grid, each read straight from the full
//                    grid at its nearest-rule index; the low-resolution volume is never stored.
//
// Arithmetic (fixed, tests/filters_ref.py restates it): every product and every sum is rounded to fp32 on its own -- floating
// point contraction is off in this file -- and a pass accumulates from tap -r upwards into +0.0f.  The halo is zero-filled:
// taps are non-negative and the accumulator can never be -0, so adding tap * 0 leaves its bits alone.
//
// Routing.  A stage that has nothing to do for a sample does not run for it and moves no data: every kernel derives the same
// route from the record (uniform: scalar loads and compares) -- which of the three stages run, and for each its source and
// destination among x, the two temporaries and out.  The last stage that runs writes out.  In place (out == x) a stencil
// or gather stage must not be the only one (it would read what its neighbours overwrite): the route then adds a plain copy
// through a temporary.  A sample without flags, or with a record that fails record_ok(), is copied bit for bit out of place
// and not touched at all in place.
#include "common.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256;
constexpr int REC = MIVP_FILTER_RECORD_WORDS;
constexpr int MAXR = 8;
constexpr int NTAP = 2 * MAXR + 1;
constexpr int TILE = 2048;                              // outputs of a k_filter_dw tile: TW = TILE / TD
constexpr int S_MAX = (TILE / 8 + 2 * MAXR) * (8 + 2 * MAXR);      // staged tile, largest at TD = 8
constexpr int T_MAX = (TILE / 64 + 2 * MAXR) * 64;                 // D-pass result, largest at TD = 64
constexpr int TH = 32, TM = 64;                         // k_filter_h tile
enum { F_NOISE = 1, F_SMOOTH = 2, F_LOWRES = 4, F_ALL = 7 };
enum { R_FLAGS = 0, R_KEY = 1, R_MEAN = 2, R_STD = 3, R_RADIUS = 4, R_LOW = 7, R_TAPS = 10 };
enum { BUF_X = 0, BUF_A = 1, BUF_B = 2, BUF_OUT = 3 };
static_assert(R_TAPS + 3 * NTAP <= REC && REC == 64, "the record layout of mivp.h");
static_assert((TILE / 16 + 2 * MAXR) * (16 + 2 * MAXR) <= S_MAX && (TILE / 32 + 2 * MAXR) * (32 + 2 * MAXR) <= S_MAX &&
              (TILE / 64 + 2 * MAXR) * (64 + 2 * MAXR) <= S_MAX, "staged tile of every TD");
static_assert((TILE / 8 + 2 * MAXR) * 8 <= T_MAX && (TILE / 16 + 2 * MAXR) * 16 <= T_MAX &&
              (TILE / 32 + 2 * MAXR) * 32 <= T_MAX, "D-pass tile of every TD");

struct Geo {
    int C, H, W, D;
    int lg;                  // log2 TD (3..6)
    int tiles_w, tiles_d;    // k_filter_dw tiles per plane
    int tiles_h, tiles_m;    // k_filter_h tiles per channel
    long M;                  // W * D
    long nvox;               // voxels per sample, channels included
};

struct Bufs { const float* x; float* a; float* b; float* out; };

struct Route {
    int flags;
    int r[3];                // radius H, W, D (0 where the smooth flag is off)
    int low[3];
    bool run[3];             // k_filter_dw, k_filter_h, k_filter_lowres
    int src[3], dst[3];
};

// every word an address or a loop bound is formed from (uniform: scalar loads and compares)
MIVP_DEV bool record_ok(const int32_t* __restrict__ rec, const Geo& g) {
    const int dims[3] = {g.H, g.W, g.D};
    if ((unsigned)rec[R_FLAGS] > (unsigned)F_ALL) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if ((unsigned)rec[R_RADIUS + a] > (unsigned)MAXR) return false;
        if (rec[R_LOW + a] < 1 || rec[R_LOW + a] > dims[a]) return false;
    }
    return true;
}

MIVP_DEV Route route_of(const int32_t* __restrict__ rec, const Geo& g, bool inplace) {
    Route t;
    t.flags = record_ok(rec, g) ? rec[R_FLAGS] : 0;
    const int dims[3] = {g.H, g.W, g.D};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t.r[a] = (t.flags & F_SMOOTH) ? rec[R_RADIUS + a] : 0;
        t.low[a] = (t.flags & F_LOWRES) ? rec[R_LOW + a] : dims[a];
    }
    const bool stencil0 = t.r[1] > 0 || t.r[2] > 0;
    t.run[0] = (t.flags & F_NOISE) || stencil0;
    t.run[1] = t.r[0] > 0;
    t.run[2] = (t.flags & F_LOWRES) != 0;
    const int n = (int)t.run[0] + (int)t.run[1] + (int)t.run[2];
    if (n == 0) {
        t.run[0] = !inplace;                             // the plain copy (radii 0, no noise)
    } else if (n == 1 && inplace) {                      // a lone stencil or gather gets a copy through a temporary
        if (t.run[0]) t.run[1] = stencil0;               // (k_filter_h with radius 0 copies)
        else t.run[0] = true;
    }
    // the last stage that runs writes out; the ones before it alternate between the temporaries
    t.src[0] = BUF_X;
    t.dst[0] = (t.run[1] || t.run[2]) ? BUF_A : BUF_OUT;
    t.src[1] = t.run[0] ? BUF_A : BUF_X;
    t.dst[1] = t.run[2] ? (t.run[0] ? BUF_B : BUF_A) : BUF_OUT;
    t.src[2] = t.run[1] ? t.dst[1] : t.src[1];
    t.dst[2] = BUF_OUT;
    return t;
}

MIVP_DEV const float* src_of(const Bufs& p, int id, long off) {
    return (id == BUF_X ? p.x : (id == BUF_A ? p.a : (id == BUF_B ? p.b : p.out))) + off;
}
MIVP_DEV float* dst_of(const Bufs& p, int id, long off) { return (id == BUF_A ? p.a : (id == BUF_B ? p.b : p.out)) + off; }

// n = mean + std * g, g = sqrt(-2 ln u1) cos(2 pi u2) from the two counter hashes of element idx
MIVP_DEV float noise_value(uint32_t idx, uint32_t key, float mean, float std) {
    const uint32_t h1 = drop_hash(2u * idx, key), h2 = drop_hash(2u * idx + 1u, key);
    const float u1 = (float)((h1 >> 8) + 1u) * 0x1p-24f;               // (0, 1]
    const float u2 = (float)(h2 >> 8) * 0x1p-24f;                      // [0, 1)
    const float rad = sqrtf(-2.f * logf(u1));
    const float g = rad * cosf(6.2831855f * u2);
    const float sg = std * g;
    return mean + sg;
}

// sum_{k = -r .. r} tap[k] * p[k * stride], p at the centre; from -r upwards into +0.0f
MIVP_DEV float filter_at(const float* p, int stride, const float* tap, int r) {
    float acc = 0.f;
    for (int k = -r; k <= r; ++k) {
        const float t = tap[MAXR + k] * p[k * stride];
        acc = acc + t;
    }
    return acc;
}

__global__ __launch_bounds__(TPB) void k_filter_dw(Bufs bufs, Geo g, const int32_t* __restrict__ slot, int inplace) {
    __shared__ float S[S_MAX];
    __shared__ float T[T_MAX];
    __shared__ float taps[2][NTAP];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int32_t* rec = slot + (long)b * REC;
    const Route rt = route_of(rec, g, inplace != 0);
    if (!rt.run[0]) return;
    const float* src = src_of(bufs, rt.src[0], (long)b * g.nvox);
    float* dst = dst_of(bufs, rt.dst[0], (long)b * g.nvox);
    const int rw = rt.r[1], rd = rt.r[2];
    if (tid < 2 * NTAP) taps[tid / NTAP][tid % NTAP] = __int_as_float(rec[R_TAPS + NTAP + tid]);
    const bool noise = rt.flags & F_NOISE;
    const uint32_t key = (uint32_t)rec[R_KEY];
    const float mean = __int_as_float(rec[R_MEAN]), std = __int_as_float(rec[R_STD]);

    const int TD = 1 << g.lg, TW = TILE >> g.lg, SS = TD + 2 * MAXR;
    unsigned t = blockIdx.x;
    const int td = (int)(t % (unsigned)g.tiles_d);
    t /= (unsigned)g.tiles_d;
    const int tw = (int)(t % (unsigned)g.tiles_w);
    const long plane = t / (unsigned)g.tiles_w;                          // c * H + h
    const int w0 = tw * TW, d0 = td * TD;
    const int nw = min(TW, g.W - w0), nd = min(TD, g.D - d0);
    const long base = plane * g.M;
    const int rows = nw + 2 * rw, cols = nd + 2 * rd;                    // <= TW + 16, <= TD + 16
    const int ty = tid >> g.lg, tx = tid & (TD - 1), ny = TPB >> g.lg;

    for (int rr = ty; rr < rows; rr += ny)
        for (int cc = tx; cc < cols; cc += TD) {
            const int w = w0 - rw + rr, d = d0 - rd + cc;
            float v = 0.f;
            if (w >= 0 && w < g.W && d >= 0 && d < g.D) {
                const long off = base + (long)w * g.D + d;
                v = src[off];
                if (noise) v = v + noise_value((uint32_t)off, key, mean, std);
            }
            S[rr * SS + cc] = v;
        }
    __syncthreads();
    if (tx < nd)
        for (int rr = ty; rr < rows; rr += ny) {
            const float* p = S + rr * SS + tx + rd;
            T[rr * TD + tx] = rd ? filter_at(p, 1, taps[1], rd) : p[0];
        }
    __syncthreads();
    if (tx < nd)
        for (int wi = ty; wi < nw; wi += ny) {
            const float* p = T + (wi + rw) * TD + tx;
            dst[base + (long)(w0 + wi) * g.D + d0 + tx] = rw ? filter_at(p, TD, taps[0], rw) : p[0];
        }
}

__global__ __launch_bounds__(TPB) void k_filter_h(Bufs bufs, Geo g, const int32_t* __restrict__ slot, int inplace) {
    __shared__ float S[(TH + 2 * MAXR) * TM];
    __shared__ float taps[NTAP];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int32_t* rec = slot + (long)b * REC;
    const Route rt = route_of(rec, g, inplace != 0);
    if (!rt.run[1]) return;
    const float* src = src_of(bufs, rt.src[1], (long)b * g.nvox);
    float* dst = dst_of(bufs, rt.dst[1], (long)b * g.nvox);
    const int rh = rt.r[0];
    if (tid < NTAP) taps[tid] = __int_as_float(rec[R_TAPS + tid]);

    unsigned t = blockIdx.x;
    const long m0 = (long)(t % (unsigned)g.tiles_m) * TM;
    t /= (unsigned)g.tiles_m;
    const int h0 = (int)(t % (unsigned)g.tiles_h) * TH;
    const long base = (long)(t / (unsigned)g.tiles_h) * g.H * g.M + m0;  // channel
    const int nh = min(TH, g.H - h0);
    const int nm = (int)min((long)TM, g.M - m0);
    const int ty = tid >> 6, tx = tid & 63;

    for (int rr = ty; rr < nh + 2 * rh; rr += TPB / 64) {
        const int h = h0 - rh + rr;
        S[rr * TM + tx] = (tx < nm && h >= 0 && h < g.H) ? src[base + (long)h * g.M + tx] : 0.f;
    }
    __syncthreads();
    if (tx < nm)
        for (int hi = ty; hi < nh; hi += TPB / 64) {
            const float* p = S + (hi + rh) * TM + tx;
            dst[base + (long)(h0 + hi) * g.M + tx] = rh ? filter_at(p, TM, taps, rh) : p[0];
        }
}

// torch's rules.  Up-sampling n -> N, linear, align_corners = False: src = max(n / N * (i + 0.5) - 0.5, 0) in fp32,
// lo = floor(src), hi = min(lo + 1, n - 1), weight of hi = src - lo.  Down-sampling N -> n, nearest: low index j reads
// min(floor(j * (N / n)), N - 1), the scale and the product in fp32.  n == N gives lo = i, weight 0, nearest(i) = i.
struct AxisTap { int lo, hi; float w; };           // lo / hi: indices into the FULL grid
MIVP_DEV int nearest_src(int j, int N, int n) {
    const float scale = (float)N / (float)n;
    return min((int)floorf((float)j * scale), N - 1);
}
MIVP_DEV AxisTap axis_tap(int i, int N, int n) {
    const float scale = (float)n / (float)N;
    const float s = fmaxf(scale * ((float)i + 0.5f) - 0.5f, 0.f);
    const int lo = min((int)s, n - 1), hi = min(lo + 1, n - 1);
    return AxisTap{nearest_src(lo, N, n), nearest_src(hi, N, n), s - (float)lo};
}
// a + w (b - a); weight 0 returns a itself, whatever b holds
MIVP_DEV float blend(float a, float b, float w) {
    const float t = w * (b - a);
    return w == 0.f ? a : a + t;
}

__global__ __launch_bounds__(TPB) void k_filter_lowres(Bufs bufs, Geo g, const int32_t* __restrict__ slot, int inplace) {
    const int b = blockIdx.y;
    const Route rt = route_of(slot + (long)b * REC, g, inplace != 0);
    if (!rt.run[2]) return;
    const float* src = src_of(bufs, rt.src[2], (long)b * g.nvox);
    float* dst = dst_of(bufs, rt.dst[2], (long)b * g.nvox);
    const long idx = (long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= g.nvox) return;
    unsigned t = (unsigned)idx;
    const int d = (int)(t % (unsigned)g.D);
    t /= (unsigned)g.D;
    const int w = (int)(t % (unsigned)g.W);
    t /= (unsigned)g.W;
    const int h = (int)(t % (unsigned)g.H);
    const float* sc = src + (long)(t / (unsigned)g.H) * g.H * g.M;       // channel
    const AxisTap th = axis_tap(h, g.H, rt.low[0]), tw = axis_tap(w, g.W, rt.low[1]), tz = axis_tap(d, g.D, rt.low[2]);
    float y[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float xw[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* row = sc + (long)(i ? th.hi : th.lo) * g.M + (long)(j ? tw.hi : tw.lo) * g.D;
            xw[j] = blend(row[tz.lo], row[tz.hi], tz.w);
        }
        y[i] = blend(xw[0], xw[1], tw.w);
    }
    dst[idx] = blend(y[0], y[1], th.w);
}

bool fill_geo(Geo& g, int32_t B, int32_t C, const int32_t* dims) {
    if (!dims || B < 1 || B > 65535 || C < 1 || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    g.C = C; g.H = dims[0]; g.W = dims[1]; g.D = dims[2];
    g.M = (long)g.W * g.D;
    if (g.M >= (1L << 31) || (long)C * g.H >= (1L << 31)) return false;
    g.nvox = (long)C * g.H * g.M;
    if (g.nvox >= (1L << 31)) return false;                              // element indices are 32-bit in the kernels
    g.lg = g.D <= 8 ? 3 : (g.D <= 16 ? 4 : (g.D <= 32 ? 5 : 6));
    const int TD = 1 << g.lg, TW = TILE >> g.lg;
    g.tiles_d = (g.D + TD - 1) / TD;
    g.tiles_w = (g.W + TW - 1) / TW;
    g.tiles_h = (g.H + TH - 1) / TH;
    g.tiles_m = (int)((g.M + TM - 1) / TM);
    return true;
}

size_t temp_floats(const Geo& g, int32_t B) { return ((size_t)B * (size_t)g.nvox + 3) & ~(size_t)3; }
}  // namespace

extern "C" size_t mivp_filter_ws(int32_t B, int32_t C, const int32_t* dims) {
    Geo g;
    if (!fill_geo(g, B, C, dims)) return 0;
    return 2 * temp_floats(g, B) * sizeof(float);
}

extern "C" int mivp_filter_apply(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* slot,
                                 void* workspace, size_t workspace_bytes, float* out, mivp_stream_t stream) {
    MIVP_REQUIRE(x && out && slot && workspace && ((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                 ((uintptr_t)workspace & 3) == 0);
    Geo g;
    MIVP_REQUIRE(fill_geo(g, B, C, dims));
    MIVP_REQUIRE(workspace_bytes >= mivp_filter_ws(B, C, dims));
    const long planes = (long)C * g.H;
    const long grid_dw = planes * g.tiles_w * g.tiles_d, grid_h = (long)C * g.tiles_h * g.tiles_m;
    MIVP_REQUIRE(grid_dw < (1L << 31) && grid_h < (1L << 31));
    Bufs bufs{x, (float*)workspace, (float*)workspace + temp_floats(g, B), out};
    const int inplace = x == out;
    hipLaunchKernelGGL(k_filter_dw, dim3((unsigned)grid_dw, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, bufs, g, slot,
                       inplace);
    hipLaunchKernelGGL(k_filter_h, dim3((unsigned)grid_h, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, bufs, g, slot,
                       inplace);
    hipLaunchKernelGGL(k_filter_lowres, dim3((unsigned)((g.nvox + TPB - 1) / TPB), (unsigned)B), dim3(TPB), 0,
                       (hipStream_t)stream, bufs, g, slot, inplace);
    return mivp_check_launch("filter_apply");
}
