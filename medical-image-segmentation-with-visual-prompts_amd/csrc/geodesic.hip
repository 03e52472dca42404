// Geodesic (image-aware) distance guidance for click and scribble prompts (mivp_amd/geodesic.py): DeepIGeoS,
// MONAI GeodesicDistance / FastGeodis, Criminisi's generalised geodesic transform.
//
// Per sample b and plane r (0 positive, 1 negative), over the 26-neighbour voxel graph of the [H][W][D] volume:
//     g(v) = min over paths seed -> v of the left-to-right float32 sum of w(u, u')
//     w(u, u') = sqrt(l2 + (gamma (I(u) - I(u')))^2),  l2 = (a_h |dh| + a_w |dw|) + a_d |dd|,  a = the float32 squared spacings
// Every operation of w and of the sum is one separately rounded float32 operation: this file is compiled with fp contraction
// off (below) and the build passes no fast-math flag, so the subtraction, the two multiplications, the addition and the sum
// are IEEE operations and sqrtf is the correctly rounded square root.  g = 0 at a seed, +inf in a plane without seeds; an
// edge whose weight is not finite (NaN or inf in the image) is never taken.  Float32 addition is monotone and every w > 0, so
// g(v) = min(seed ? 0 : inf, min_u fl(g(u) + w(u, v))) has one solution reachable from the start state, and any relaxation
// that stops only when nothing changes reaches it, in any order: the converged field is a float32 Dijkstra's, bit for bit.
//
// Workspace (mivp_geodesic_ws): [seed mask u8 B vol][F0 f32 [B][2][vol]][F1 the same][counters i32 [ncnt]], each rounded to
// 256 bytes; ncnt = min(vol, 65535) + 1; then 256 bytes the kernels do not touch (room for the record of mivp_geodesic_end).
//
//   seed    1 or 2 launches: seeds = the two scribble bits of a StrokeSlot mask (or 0), then one thread per click slot entry:
//           count clamped to 0 .. K on the device, a channel other than 0 / 1 or a coordinate outside the volume ignored,
//           the bit set by an integer atomicOr on the containing 32-bit word (as mivp_strokes_draw).
//   begin   F0 = F1 = (bit r of the seed mask ? 0 : +inf); counters[0] = 1 (iteration 1 has no predecessor), the others 0.
//   iter    iteration `it` reads A = F[(it + 1) & 1] and writes B = F[it & 1].  One workgroup of 1024 threads per brick of
//           16 x 16 x 32 voxels and field; it returns at once when counters[it - 1] == 0.  It stages the brick of A and of the
//           image channel with a one-voxel halo in LDS (2 x 18 x 18 x 34 floats = 88,128 bytes: one workgroup = 16 waves per
//           CU of the 160 KB, 4 per SIMD; halo cells outside the volume hold +inf and are never relaxed), relaxes inside LDS
//           until the brick stops changing, and stores the brick's interior to B once.  A round is 8 colour steps with a
//           barrier behind each: step c relaxes the voxels whose coordinate parities are the bits of c, one per thread.  Two
//           voxels of one colour are never neighbours, so a step reads only values no thread writes in that step: the
//           result is a function of A alone, whatever the wave scheduling, converged or not.  The 26 weights are recomputed
//           from the staged image; a neighbour at +inf costs no square root.  The voxels whose stored value is below A's
//           are counted (shuffles, LDS) and added to counters[it] with one integer atomicAdd per workgroup.
//   end     info = (iterations that lowered a voxel, converged) from the counters of iterations 1 .. n.
//   encode  the closing pass of csrc/guidance_common.hpp on F[n & 1]: value = max(box, f(g)), m = g g in float32,
//           f = expf(-m / 2 sigma^2) or m <= radius^2; g = +inf gives +0.
//
// Determinism: an iteration reads only A and the image and writes only B and an integer counter, so B = R(A) for a fixed
// function R.  Parity: after n issued iterations the field is F[n & 1], n the host's count; when an iteration k <= n lowered
// nothing it stored B = A bit for bit and every later launch returned at once, so both buffers hold the converged field and
// the parity of k does not matter.
#include "guidance_common.hpp"
#include <math.h>

#pragma clang fp contract(off)

namespace {
constexpr int GD_TPB = 1024;
constexpr int GD_BH = 16, GD_BW = 16, GD_BD = 32;                   // the brick
constexpr int GD_LH = GD_BH + 2, GD_LW = GD_BW + 2, GD_LD = GD_BD + 2;
constexpr int GD_CELLS = GD_LH * GD_LW * GD_LD;                     // 11,016 staged cells
constexpr int GD_LDS = 2 * GD_CELLS * (int)sizeof(float);           // field + image: 88,128 bytes
constexpr int GD_MAXITER = 65535;
constexpr int GD_MAXK = 64;
constexpr int GD_SMALL_TPB = 256;
static_assert(GD_BH * GD_BW * GD_BD == 8 * GD_TPB, "one 2 x 2 x 2 cell per thread");

struct GdVol {
    int H, W, D, nbw, nbd;
    long vol, nbrick;                                              // bricks per field
};

struct GdMetric { float ah, aw, ad, gamma; };

// the weight of the edge between two voxels of intensities x, y at index offset (dh, dw, dd) in {-1, 0, 1}^3
MIVP_DEV float gd_weight(float x, float y, int dh, int dw, int dd, const GdMetric& m) {
    const float l2 = (m.ah * (float)(dh * dh) + m.aw * (float)(dw * dw)) + m.ad * (float)(dd * dd);
    const float diff = x - y;
    const float t = m.gamma * diff;
    const float q = t * t;
    const float s = l2 + q;
    return sqrtf(s);                                               // correctly rounded: no fast-math flag in the build
}

// ------------------------------------------------------------------------------------------------------------- seeds
__global__ __launch_bounds__(GD_SMALL_TPB) void k_geodesic_seed_mask(const uint8_t* __restrict__ strokes, long n,
                                                                     uint8_t* __restrict__ seeds) {
    for (long i = (long)blockIdx.x * GD_SMALL_TPB + threadIdx.x; i < n; i += (long)gridDim.x * GD_SMALL_TPB)
        seeds[i] = strokes ? (uint8_t)(strokes[i] & 3) : (uint8_t)0;
}

// one thread per (b, k)
__global__ __launch_bounds__(GD_SMALL_TPB) void k_geodesic_seed_clicks(const int32_t* __restrict__ clicks,
                                                                       const int32_t* __restrict__ count, int B, int K, int H,
                                                                       int W, int D, uint8_t* __restrict__ seeds) {
    const int i = blockIdx.x * GD_SMALL_TPB + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K, k = i - b * K;
    if (k >= min(max(count[b], 0), K)) return;
    const int32_t* c = clicks + (long)i * 4;
    const int h = c[0], w = c[1], d = c[2], ch = c[3];
    if ((ch != 0 && ch != 1) || (unsigned)h >= (unsigned)H || (unsigned)w >= (unsigned)W || (unsigned)d >= (unsigned)D) return;
    const long v = (((long)b * H + h) * W + w) * D + d;
    const uintptr_t addr = (uintptr_t)(seeds + v);
    atomicOr(reinterpret_cast<unsigned*>(addr & ~(uintptr_t)3), (unsigned)(1 << ch) << (8 * (addr & 3)));
}

// ------------------------------------------------------------------------------------------------------------- begin
__global__ __launch_bounds__(GD_SMALL_TPB) void k_geodesic_begin(const uint8_t* __restrict__ seeds, long nvox, long vol,
                                                                 float* __restrict__ f0, float* __restrict__ f1, int ncnt,
                                                                 int32_t* __restrict__ counters) {
    const long t0 = (long)blockIdx.x * GD_SMALL_TPB + threadIdx.x, span = (long)gridDim.x * GD_SMALL_TPB;
    for (long i = t0; i < ncnt; i += span) counters[i] = i == 0 ? 1 : 0;
    for (long i = t0; i < nvox; i += span) {
        const long b = i / vol, v = i - b * vol;
        const int m = seeds[i];
        const float p = (m & 1) ? 0.f : INFINITY, q = (m & 2) ? 0.f : INFINITY;
        f0[2 * b * vol + v] = p; f1[2 * b * vol + v] = p;
        f0[(2 * b + 1) * vol + v] = q; f1[(2 * b + 1) * vol + v] = q;
    }
}

// ------------------------------------------------------------------------------------------------------- an iteration
MIVP_DEV int gd_wave_sum(int v) {
    for (int sh = 32; sh > 0; sh >>= 1) v += __shfl_xor(v, sh);
    return v;
}

// grid: 2 B nbrick workgroups; field = blockIdx.x / nbrick.  image: channel `channel` of sample 0; istride floats per sample.
__global__ __launch_bounds__(GD_TPB) void k_geodesic_iter(const float* __restrict__ A, float* __restrict__ Bf,
                                                          const float* __restrict__ image, long istride, GdVol p, GdMetric m,
                                                          const int32_t* __restrict__ prev, int32_t* __restrict__ cur) {
    if (*prev == 0) return;                                        // the predecessor lowered nothing: A is the fixed point
    extern __shared__ __attribute__((aligned(16))) float gd_lds[];
    __shared__ int red[GD_TPB / 64];
    float* F = gd_lds;
    float* I = gd_lds + GD_CELLS;
    const int tid = threadIdx.x;
    const long field = blockIdx.x / p.nbrick, brick = blockIdx.x - field * p.nbrick;
    const int bh = (int)(brick / ((long)p.nbw * p.nbd)), bw = (int)(brick / p.nbd % p.nbw), bd = (int)(brick % p.nbd);
    const int h0 = bh * GD_BH - 1, w0 = bw * GD_BW - 1, d0 = bd * GD_BD - 1;      // volume coordinates of staged cell (0, 0, 0)
    const float* a = A + field * p.vol;
    const float* img = image + (field >> 1) * istride;
    float* dst = Bf + field * p.vol;

    int finite = 0;
    for (int i = tid; i < GD_CELLS; i += GD_TPB) {
        const int lh = i / (GD_LW * GD_LD), lw = i / GD_LD % GD_LW, ld = i % GD_LD;
        const int gh = h0 + lh, gw = w0 + lw, gd = d0 + ld;
        const bool in = (unsigned)gh < (unsigned)p.H && (unsigned)gw < (unsigned)p.W && (unsigned)gd < (unsigned)p.D;
        const long v = ((long)gh * p.W + gw) * p.D + gd;
        const float f = in ? a[v] : INFINITY;                      // outside the volume: +inf, never relaxed
        F[i] = f;
        I[i] = in ? img[v] : 0.f;
        finite |= f < INFINITY;
    }
    if (__syncthreads_or(finite)) {                                // a brick without a finite value cannot change
        const int ch = tid >> 7, cw = (tid >> 4) & 7, cd = tid & 15;
        for (;;) {
            int changed = 0;
            for (int c = 0; c < 8; ++c) {
                const int lh = 2 * ch + (c >> 2) + 1, lw = 2 * cw + ((c >> 1) & 1) + 1, ld = 2 * cd + (c & 1) + 1;
                if (h0 + lh < p.H && w0 + lw < p.W && d0 + ld < p.D) {
                    const int i = (lh * GD_LW + lw) * GD_LD + ld;
                    const float was = F[i], x = I[i];
                    float best = was;
#pragma unroll
                    for (int dh = -1; dh <= 1; ++dh)
#pragma unroll
                        for (int dw = -1; dw <= 1; ++dw)
#pragma unroll
                            for (int dd = -1; dd <= 1; ++dd) {
                                if (dh == 0 && dw == 0 && dd == 0) continue;
                                const int j = i + (dh * GD_LW + dw) * GD_LD + dd;
                                const float g = F[j];
                                if (g < best) {                    // (g + w >= g: a neighbour not below best cannot lower it)
                                    const float w = gd_weight(x, I[j], dh, dw, dd, m);
                                    const float cand = g + w;
                                    if (w < INFINITY && cand < best) best = cand;      // NaN or inf weight: never taken
                                }
                            }
                    if (best < was) { F[i] = best; changed = 1; }
                }
                __syncthreads();
            }
            if (!__syncthreads_or(changed)) break;
        }
    }

    int lowered = 0;
    for (int i = tid; i < GD_BH * GD_BW * GD_BD; i += GD_TPB) {
        const int lh = i / (GD_BW * GD_BD), lw = i / GD_BD % GD_BW, ld = i % GD_BD;
        const int gh = h0 + 1 + lh, gw = w0 + 1 + lw, gd = d0 + 1 + ld;
        if (gh < p.H && gw < p.W && gd < p.D) {
            const long v = ((long)gh * p.W + gw) * p.D + gd;
            const float f = F[((lh + 1) * GD_LW + lw + 1) * GD_LD + ld + 1];
            lowered += f < a[v] ? 1 : 0;
            dst[v] = f;
        }
    }
    lowered = gd_wave_sum(lowered);
    if ((tid & 63) == 0) red[tid >> 6] = lowered;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int k = 0; k < GD_TPB / 64; ++k) sum += red[k];
        if (sum) atomicAdd(cur, sum);
    }
}

// --------------------------------------------------------------------------------------------------------------- end
// one workgroup: info = (the counters of iterations 1 .. n that are not zero, whether iteration n lowered nothing)
__global__ __launch_bounds__(GD_SMALL_TPB) void k_geodesic_end(const int32_t* __restrict__ counters, int n, int32_t* __restrict__ info) {
    __shared__ int ran;
    if (threadIdx.x == 0) ran = 0;
    __syncthreads();
    int mine = 0;
    for (int it = 1 + threadIdx.x; it <= n; it += GD_SMALL_TPB) mine += counters[it] != 0 ? 1 : 0;
    if (mine) atomicAdd(&ran, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        info[0] = ran;
        info[1] = (n >= 1 && counters[n] == 0) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------ encode
struct GdEnc {
    GuideRun run;
    int kind;
    float param;                                               // 2 sigma^2 (gaussian) or radius^2 (disk)
};

MIVP_DEV float gd_value(float g, const GdEnc& e) {
    const float m = g * g;
    return e.kind == 0 ? expf(-m / e.param) : (m <= e.param ? 1.f : 0.f);
}

__global__ __launch_bounds__(GUIDE_TPB) void k_geodesic_encode(const int32_t* __restrict__ boxes, const int32_t* __restrict__ box_count,
                                                               const float* __restrict__ fields, GdEnc e, float* __restrict__ out) {
    __shared__ GuideBox lst[2][GUIDE_MAXKB];
    __shared__ int n[2];
    const int b = blockIdx.y;
    guide_boxes(boxes, box_count, b, e.run.KB, lst, n);
    __syncthreads();
    const long run = 2L * e.run.H * e.run.W * e.run.D;
    guide_close_run(lst, n, fields + (long)b * run, e.run, out, [&](float g) -> float { return gd_value(g, e); });
}

// --------------------------------------------------------------------------------------------------------- host side
bool gd_dims(const int32_t* dims, int32_t B, GdVol& p) {
    if (!dims || B < 1 || B > 65535) return false;
    p.H = dims[0]; p.W = dims[1]; p.D = dims[2];
    if (p.H < 1 || p.W < 1 || p.D < 1 || p.H > 65535 || p.W > 65535 || p.D > 65535) return false;
    p.vol = (long)p.H * p.W * p.D;
    if (p.vol >= (1L << 31) || (long)B * p.vol >= (1L << 31)) return false;
    const long nbh = (p.H + GD_BH - 1) / GD_BH;
    p.nbw = (p.W + GD_BW - 1) / GD_BW;
    p.nbd = (p.D + GD_BD - 1) / GD_BD;
    p.nbrick = nbh * p.nbw * p.nbd;
    return true;
}

bool gd_metric(const float* spacing, float gamma, GdMetric& m) {
    if (!spacing || !isfinite(gamma) || gamma < 0.f) return false;
    for (int a = 0; a < 3; ++a)
        if (!isfinite(spacing[a]) || !(spacing[a] > 0.f)) return false;
    m.ah = spacing[0] * spacing[0]; m.aw = spacing[1] * spacing[1]; m.ad = spacing[2] * spacing[2];
    m.gamma = gamma;
    return isfinite(m.ah) && isfinite(m.aw) && isfinite(m.ad) && m.ah > 0.f && m.aw > 0.f && m.ad > 0.f;
}

size_t gd_round(size_t n) { return (n + 255) / 256 * 256; }

int gd_ncnt(const GdVol& p) { return (int)(p.vol < GD_MAXITER ? p.vol : GD_MAXITER) + 1; }

struct GdWs {
    uint8_t* seeds;
    float* f[2];
    int32_t* counters;
};

GdWs gd_carve(void* workspace, int32_t B, const GdVol& p) {
    GdWs w;
    char* at = (char*)workspace;
    const size_t nf = (size_t)2 * B * p.vol * sizeof(float);
    w.seeds = (uint8_t*)at;      at += gd_round((size_t)B * p.vol);
    w.f[0] = (float*)at;         at += gd_round(nf);
    w.f[1] = (float*)at;         at += gd_round(nf);
    w.counters = (int32_t*)at;
    return w;
}

unsigned gd_grid(long n, long cap) {
    const long want = (n + GD_SMALL_TPB - 1) / GD_SMALL_TPB;
    return (unsigned)(want > cap ? cap : (want < 1 ? 1 : want));
}
}  // namespace

extern "C" size_t mivp_geodesic_ws(int32_t B, const int32_t* dims) {
    GdVol p;
    if (!gd_dims(dims, B, p)) return 0;
    return gd_round((size_t)B * p.vol) + 2 * gd_round((size_t)2 * B * p.vol * sizeof(float)) +
           gd_round((size_t)gd_ncnt(p) * sizeof(int32_t)) + gd_round(2 * sizeof(int32_t));
}

extern "C" int mivp_geodesic_seed(const uint8_t* stroke_mask, const int32_t* clicks, const int32_t* count, int32_t K, int32_t B,
                                  const int32_t* dims, uint8_t* seeds, mivp_stream_t stream) {
    GdVol p;
    MIVP_REQUIRE(gd_dims(dims, B, p));
    MIVP_REQUIRE(seeds && ((uintptr_t)seeds & 3) == 0);
    MIVP_REQUIRE((clicks == nullptr) == (count == nullptr));
    MIVP_REQUIRE(!clicks || (K >= 1 && K <= GD_MAXK && (((uintptr_t)clicks | (uintptr_t)count) & 3) == 0));
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)B * p.vol;                                // (its storage ends on a 32-bit word: the clicks' atomicOr)
    hipLaunchKernelGGL(k_geodesic_seed_mask, dim3(gd_grid(n, 16384)), dim3(GD_SMALL_TPB), 0, st, stroke_mask, n, seeds);
    int rc = mivp_check_launch("geodesic_seed_mask");
    if (rc != MIVP_OK || !clicks) return rc;
    hipLaunchKernelGGL(k_geodesic_seed_clicks, dim3(gd_grid((long)B * K, 1L << 30)), dim3(GD_SMALL_TPB), 0, st, clicks, count, (int)B,
                       (int)K, p.H, p.W, p.D, seeds);
    return mivp_check_launch("geodesic_seed_clicks");
}

extern "C" int mivp_geodesic_begin(const uint8_t* seeds, int32_t B, const int32_t* dims, void* workspace, mivp_stream_t stream) {
    GdVol p;
    MIVP_REQUIRE(gd_dims(dims, B, p));
    MIVP_REQUIRE(seeds && workspace && ((uintptr_t)workspace & 255) == 0);
    const GdWs w = gd_carve(workspace, B, p);
    const int ncnt = gd_ncnt(p);
    const long nvox = (long)B * p.vol;
    hipLaunchKernelGGL(k_geodesic_begin, dim3(gd_grid(nvox, 65536)), dim3(GD_SMALL_TPB), 0, (hipStream_t)stream, seeds, nvox, p.vol, w.f[0], w.f[1], ncnt,
                       w.counters);
    return mivp_check_launch("geodesic_begin");
}

extern "C" int mivp_geodesic_iter(int32_t iteration, const float* image, int32_t C, int32_t channel, int32_t B, const int32_t* dims,
                                  const float* spacing, float gamma, void* workspace, mivp_stream_t stream) {
    GdVol p;
    GdMetric m;
    MIVP_REQUIRE(gd_dims(dims, B, p));
    MIVP_REQUIRE(gd_metric(spacing, gamma, m));
    MIVP_REQUIRE(image && workspace && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)image & 3) == 0);
    MIVP_REQUIRE(C >= 1 && channel >= 0 && channel < C && iteration >= 1 && iteration < gd_ncnt(p));
    const GdWs w = gd_carve(workspace, B, p);
    MIVP_REQUIRE(2L * B * p.nbrick < (1L << 31));
    MIVP_LDS_OPT_IN(k_geodesic_iter, GD_LDS);
    hipLaunchKernelGGL(k_geodesic_iter, dim3((unsigned)(2L * B * p.nbrick)), dim3(GD_TPB), GD_LDS, (hipStream_t)stream,
                       (const float*)w.f[(iteration + 1) & 1], w.f[iteration & 1], image + (size_t)channel * p.vol, (long)C * p.vol, p,
                       m, (const int32_t*)(w.counters + iteration - 1), w.counters + iteration);
    return mivp_check_launch("geodesic_iter");
}

extern "C" int mivp_geodesic_end(int32_t iterations, int32_t B, const int32_t* dims, const void* workspace, int32_t* info,
                                 mivp_stream_t stream) {
    GdVol p;
    MIVP_REQUIRE(gd_dims(dims, B, p));
    MIVP_REQUIRE(workspace && info && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)info & 3) == 0);
    MIVP_REQUIRE(iterations >= 0 && iterations < gd_ncnt(p));
    const GdWs w = gd_carve(const_cast<void*>(workspace), B, p);
    hipLaunchKernelGGL(k_geodesic_end, dim3(1), dim3(GD_SMALL_TPB), 0, (hipStream_t)stream, (const int32_t*)w.counters, (int)iterations,
                       info);
    return mivp_check_launch("geodesic_end");
}

extern "C" int mivp_geodesic_encode(const int32_t* boxes, const int32_t* box_count, int32_t KB, int32_t iterations, int32_t B,
                                    int32_t Ctot, int32_t channel_offset, const int32_t* dims, int32_t frame, int32_t kind,
                                    float param, float* out, const void* workspace, mivp_stream_t stream) {
    GdVol p;
    MIVP_REQUIRE(gd_dims(dims, B, p));
    MIVP_REQUIRE(out && workspace && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)out & 3) == 0);
    MIVP_REQUIRE((boxes == nullptr) == (box_count == nullptr));
    MIVP_REQUIRE(!boxes || (KB >= 1 && KB <= GUIDE_MAXKB && (((uintptr_t)boxes | (uintptr_t)box_count) & 3) == 0));
    MIVP_REQUIRE(Ctot >= 2 && channel_offset >= 0 && channel_offset <= Ctot - 2 && (frame == 0 || frame == 1));
    MIVP_REQUIRE((kind == 0 && param > 0.f && isfinite(param)) || (kind == 1 && param >= 0.f && isfinite(param)));
    MIVP_REQUIRE(iterations >= 0 && iterations < gd_ncnt(p));
    const GdWs w = gd_carve(const_cast<void*>(workspace), B, p);
    GdEnc e;
    e.run.H = p.H; e.run.W = p.W; e.run.D = p.D; e.run.KB = boxes ? KB : 1; e.run.Ctot = Ctot; e.run.off = channel_offset;
    e.run.frame = frame; e.kind = kind; e.param = param;
    hipLaunchKernelGGL(k_geodesic_encode, dim3(guide_grid(p.vol), (unsigned)B), dim3(GUIDE_TPB), 0, (hipStream_t)stream, boxes, box_count,
                       (const float*)w.f[iterations & 1], e, out);
    return mivp_check_launch("geodesic_encode");
}
