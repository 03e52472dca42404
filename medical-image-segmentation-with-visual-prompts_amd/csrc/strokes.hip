// Box and scribble prompts (mivp_amd/strokes.py): boxes and strokes as two guidance channels of the model input,
// and the simulated box and corrective scribble of interactive training (nnInteractive, SAM-Med3D, MONAI Label, DeepEdit).
//
// The device record of a batch (StrokeSlot): boxes i32 [B][KB][7] = (h0, w0, d0, h1, w1, d1, channel; inclusive corners,
// channel 0 positive, 1 negative, anything else an empty row), box_count i32 [B], mask u8 [B][H][W][D] (bit 0 a positive
// scribble voxel, bit 1 a negative one), last i32 [B][8], scratch i32 [B][8] (all zero between calls).  KB <= 16.
//
// 1. mivp_strokes_draw, one launch: a polyline of 1 .. 256 points, one thread per (segment, step).  Step i of a -> b is the
//    voxel a + floor((2 i delta + n) / (2 n)), n = max |delta|, the floor towards minus infinity in 64-bit integers.  Several
//    steps may meet in one byte and four bytes share a word: the bit is set by an integer atomicOr on the containing word.
//
// 2. mivp_strokes_encode, four launches whatever the slot holds:
//      seed / D   one wave per (b, h, w) line, both bit planes: the index distance along D to the nearest scribble voxel of
//                 the plane (ballots; the sweep state of plane r lives in lane r).  fields f32 [B][2][vol].
//      W, H       edt_line of csrc/edt_common.hpp, one thread per line over the 2 B fields.
//      close      the streaming pass over a sample's run of 2 vol floats ([head of 0..3 scalars][16-byte quads][tail], as
//                 k_clicks_encode): value = max(box, stroke), stroke = expf(-m / 2 sigma^2) or m <= radius^2 from the field
//                 (m = +inf without a scribble voxel: +0), box from the sample's rows, compacted per channel in LDS.
//
// 3. mivp_strokes_box, two launches: a reduction of the object's coordinates (wave shuffles, LDS, then one set of six
//    integer atomicMax per workgroup and sample: the low corner is kept as 65536 - lo, so that zero means "no voxel" on
//    all six words), and a one-workgroup finalize that applies margin and jitter, clamps, appends, writes last and puts
//    the scratch words back to zero.
//
// 4. mivp_strokes_scribbles: seed / D (the scheme of 2 on the two error regions, seeds = the voxels outside the region; it
//    also zeroes last), W, H, core (depth^2 = min(field, face) >= min_depth^2 -> a class map 1 / 2 of the batch stacked along
//    H with an even stride and at least one zero slab between samples, so that a voxel keeps the parity of its
//    coordinates), then the thinning entries of csrc/skeleton.hip on the stacked map (begin, max_iter iterations, end), then
//    commit (the skeleton's voxels into the mask's bits; a ballot and a popcount per wave, LDS, one integer atomicAdd per
//    workgroup and counter).  Every launch is unconditional.
#include "edt_common.hpp"
#include "guidance_common.hpp"

namespace {
constexpr int ST_TPB = 256;
constexpr int ST_MAXKB = 16;
static_assert(ST_TPB == GUIDE_TPB && ST_MAXKB == GUIDE_MAXKB, "the closing pass runs the shared walk");
constexpr int ST_MAXPTS = 256;
constexpr int ST_MAXCLS = 32;                                  // labels are classes 0 .. 31; the object is a 32-bit mask

// ------------------------------------------------------------------------------------------------------------- drawing
// grid (blocks over the steps, segments).  points i32 [npts][3]; segment s runs from point s to point min(s + 1, npts - 1)
__global__ __launch_bounds__(ST_TPB) void k_strokes_draw(const int32_t* __restrict__ points, int npts, int H, int W, int D, int bit,
                                                         uint8_t* __restrict__ mask_b) {
    const int s = blockIdx.y, e = min(s + 1, npts - 1);
    const int a0 = points[3 * s], a1 = points[3 * s + 1], a2 = points[3 * s + 2];
    const int b0 = points[3 * e], b1 = points[3 * e + 1], b2 = points[3 * e + 2];
    if ((unsigned)a0 >= (unsigned)H || (unsigned)b0 >= (unsigned)H || (unsigned)a1 >= (unsigned)W || (unsigned)b1 >= (unsigned)W ||
        (unsigned)a2 >= (unsigned)D || (unsigned)b2 >= (unsigned)D)
        return;                                                    // (the host call refuses such points: nothing is stored)
    const long long d0 = b0 - a0, d1 = b1 - a1, d2 = b2 - a2;
    auto mag = [](long long x) -> long long { return x < 0 ? -x : x; };
    const long long n = max(max(mag(d0), mag(d1)), mag(d2));
    const long long i = (long long)blockIdx.x * ST_TPB + threadIdx.x;
    if (i > n) return;
    auto step = [&](long long delta) -> int {
        if (n == 0) return 0;
        const long long num = 2 * i * delta + n, den = 2 * n;
        return (int)(num >= 0 ? num / den : -((-num + den - 1) / den));
    };
    const long v = ((long)(a0 + step(d0)) * W + (a1 + step(d1))) * D + (a2 + step(d2));
    const uintptr_t addr = (uintptr_t)(mask_b + v);
    atomicOr(reinterpret_cast<unsigned*>(addr & ~(uintptr_t)3), (unsigned)bit << (8 * (addr & 3)));
}

// ---------------------------------------------------------------------------------------------------------- the D pass
// One wave, one line of D elements, two planes.  code_at(p): the element's code; is_seed(code, r): whether it is a seed of
// plane r; store(r, p, dd): dd = the index distance of element p to the nearest seed of plane r (>= EDT_NO_SEED / 2 without
// one).  Lane r < 2 owns the sweep state of plane r (k_hausdorff_d, k_clicks_d).
template <class CodeAt, class IsSeed, class Store>
MIVP_DEV void st_d_line(int D, int lane, CodeAt code_at, IsSeed is_seed, Store store) {
    const int nch = (D + 63) >> 6;
    int prev = -EDT_NO_SEED, next = -1;
    for (int k = 0; k < nch; ++k) {
        const int p = 64 * k + lane;
        const int code = p < D ? code_at(p) : 0;
        for (int r = 0; r < 2; ++r) {
            const unsigned long long m = __ballot(p < D && is_seed(code, r));
            const unsigned long long ml = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
            const unsigned long long mr = m & (~0ull << lane);
            const int pv = __shfl(prev, r);
            int nx = __shfl(next, r);
            const int left = ml ? 64 * k + 63 - __builtin_clzll(ml) : pv;
            if (!(m >> 63) && nx <= 64 * k + 63) {                 // wave-uniform: some lanes need the next seed
                nx = EDT_NO_SEED;
                for (int j = k + 1; j < nch; ++j) {
                    const int q = 64 * j + lane;
                    const int cq = q < D ? code_at(q) : 0;
                    const unsigned long long mm = __ballot(q < D && is_seed(cq, r));
                    if (mm) { nx = 64 * j + __builtin_ctzll(mm); break; }
                }
            }
            const int right = mr ? 64 * k + __builtin_ctzll(mr) : nx;
            if (lane == r) {
                next = nx;
                if (m) prev = 64 * k + 63 - __builtin_clzll(m);
            }
            if (p < D) store(r, p, min(p - left, right - p));
        }
    }
}

// seed / D pass of the encoding: line < B H W; field (b, r) at fields + (2 b + r) vol
__global__ __launch_bounds__(ST_TPB) void k_strokes_seed(const uint8_t* __restrict__ mask, long nlines, long lines_per_b, int D,
                                                         float a, int intp, float* __restrict__ fields) {
    const int lane = threadIdx.x & 63;
    const long vol = lines_per_b * D;
    for (long line = (long)blockIdx.x * (ST_TPB / 64) + (threadIdx.x >> 6); line < nlines; line += (long)gridDim.x * (ST_TPB / 64)) {
        const long b = line / lines_per_b, first = (line - b * lines_per_b) * D;
        const uint8_t* src = mask + line * D;
        float* dst = fields + 2 * b * vol + first;
        st_d_line(D, lane, [&](int p) -> int { return src[p]; }, [](int code, int r) -> bool { return (code >> r) & 1; },
                  [&](int r, int p, int dd) { dst[r * vol + p] = edt_d_value(dd, a, intp); });
    }
}

// W / H pass over the 2 B fields: line = field * lines_per_field + (outer, inner), inner = d fastest across lanes
template <bool INTP>
__global__ __launch_bounds__(ST_TPB) void k_strokes_line(float* __restrict__ fields, long nlines, long lines_per_field, long vol,
                                                         int inner, long outer_stride, long stride, int n, float a,
                                                         int2* __restrict__ stack) {
    const long line = (long)blockIdx.x * ST_TPB + threadIdx.x;
    if (line >= nlines) return;
    const long field = line / lines_per_field, l = line - field * lines_per_field;
    edt_line<INTP>(fields + field * vol + (l / inner) * outer_stride + (l % inner), stride, n, a, stack, nlines, line);
}

// ------------------------------------------------------------------------------------------------------------ encoding
// the box rule and the walk over the run: csrc/guidance_common.hpp (shared with csrc/geodesic.hip)
struct StEnc {
    GuideRun run;
    int kind;
    float param;                                               // 2 sigma^2 (gaussian) or radius^2 (disk)
};

MIVP_DEV float st_stroke(float m, const StEnc& e) { return e.kind == 0 ? expf(-m / e.param) : (m <= e.param ? 1.f : 0.f); }

// closing pass: grid (blocks per sample, B).  lst[ch][i] = box i of channel ch, n[ch] of them.
__global__ __launch_bounds__(ST_TPB) void k_strokes_close(const int32_t* __restrict__ boxes, const int32_t* __restrict__ box_count,
                                                          const float* __restrict__ fields, StEnc e, float* __restrict__ out) {
    __shared__ GuideBox lst[2][GUIDE_MAXKB];
    __shared__ int n[2];
    const int b = blockIdx.y;
    guide_boxes(boxes, box_count, b, e.run.KB, lst, n);
    __syncthreads();
    const long run = 2L * e.run.H * e.run.W * e.run.D;             // the two fields of sample b, in the order of the run
    guide_close_run(lst, n, fields + (long)b * run, e.run, out, [&](float m) -> float { return st_stroke(m, e); });
}

// ------------------------------------------------------------------------------------------------------- label reading
struct StSim {
    const void* pred;
    const void* target;
    int pdt, tdt;                                              // dtype codes (0 uint8, 1 int32, 2 int64, 3 float32)
    unsigned mask;                                             // the object's classes
    int has_ignore, ignore;
};

// class 0 .. 31 of element i of a label map, -1 for anything else
MIVP_DEV int st_label(const void* p, int dt, long i) {
    switch (dt) {
        case 0: return class_of<uint8_t>(static_cast<const uint8_t*>(p)[i], ST_MAXCLS);
        case 1: return class_of<int32_t>(static_cast<const int32_t*>(p)[i], ST_MAXCLS);
        case 2: return class_of<long long>(static_cast<const long long*>(p)[i], ST_MAXCLS);
        default: return class_of<float>(static_cast<const float*>(p)[i], ST_MAXCLS);
    }
}

// whether voxel i of the batch is a valid voxel of the object
MIVP_DEV bool st_object(const StSim& s, long i) {
    const int t = st_label(s.target, s.tdt, i);
    return t >= 0 && !(s.has_ignore && t == s.ignore) && ((s.mask >> t) & 1u);
}

// region of voxel i of the batch: 0 none, 1 E_pos (false negative), 2 E_neg (false positive): the rule of simulate_clicks
MIVP_DEV int st_region(const StSim& s, long i) {
    const int t = st_label(s.target, s.tdt, i);
    if (t < 0 || (s.has_ignore && t == s.ignore)) return 0;
    const int p = st_label(s.pred, s.pdt, i);
    const bool tin = (s.mask >> t) & 1u, pin = p >= 0 && ((s.mask >> p) & 1u);
    return tin == pin ? 0 : (tin ? 1 : 2);
}

// ------------------------------------------------------------------------------------------------------ simulated box
MIVP_DEV int st_wave_max(int v) {
    for (int sh = 32; sh > 0; sh >>= 1) v = max(v, __shfl_xor(v, sh));
    return v;
}

// grid (blocks per sample, B).  acc i32 [B][8]: words 0..2 = max of 65536 - coordinate, 3..5 = max of coordinate + 1
__global__ __launch_bounds__(ST_TPB) void k_strokes_box_reduce(StSim s, int H, int W, int D, int32_t* __restrict__ acc) {
    __shared__ int red[ST_TPB / 64][6];
    const int b = blockIdx.y;
    const long vol = (long)H * W * D;
    const int WD = W * D;
    int k[6] = {0, 0, 0, 0, 0, 0};
    for (long lv = (long)blockIdx.x * ST_TPB + threadIdx.x; lv < vol; lv += (long)gridDim.x * ST_TPB) {
        if (!st_object(s, (long)b * vol + lv)) continue;
        const int v = (int)lv;
        const int h = v / WD, w = (v - h * WD) / D, d = v - h * WD - w * D;
        k[0] = max(k[0], 65536 - h); k[1] = max(k[1], 65536 - w); k[2] = max(k[2], 65536 - d);
        k[3] = max(k[3], h + 1); k[4] = max(k[4], w + 1); k[5] = max(k[5], d + 1);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) k[j] = st_wave_max(k[j]);
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < 6; ++j) red[threadIdx.x >> 6][j] = k[j];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int j = threadIdx.x;
        const int m = max(max(red[0][j], red[1][j]), max(red[2][j], red[3][j]));
        if (m) atomicMax(acc + (long)b * 8 + j, m);
    }
}

struct StBoxArgs { int dims[3], margin[3], KB, channel; };

__global__ __launch_bounds__(ST_TPB) void k_strokes_box_finalize(int32_t* __restrict__ acc, const int32_t* __restrict__ jitter, int B,
                                                                 StBoxArgs a, int32_t* __restrict__ boxes,
                                                                 int32_t* __restrict__ box_count, int32_t* __restrict__ last) {
    for (int b = threadIdx.x; b < B; b += ST_TPB) {
        int32_t* k = acc + (long)b * 8;
        int32_t* out = last + (long)b * 8;
        const bool found = k[3] > 0;
        int row[6] = {-1, -1, -1, -1, -1, -1};
        if (found) {
            for (int ax = 0; ax < 3; ++ax) {
                const long long lo = 65536 - k[ax], hi = k[3 + ax] - 1;
                const long long jl = jitter ? jitter[b * 6 + ax] : 0, jh = jitter ? jitter[b * 6 + 3 + ax] : 0;
                row[ax] = (int)min(max(lo - a.margin[ax] + jl, 0LL), hi);
                row[3 + ax] = max((int)min(max(hi + a.margin[ax] + jh, lo), (long long)a.dims[ax] - 1), row[ax]);
            }
        }
        const int cnt = box_count[b];
        const bool place = found && cnt >= 0 && cnt < a.KB;
        if (place) {
            int32_t* dst = boxes + ((long)b * a.KB + cnt) * 7;
            for (int j = 0; j < 6; ++j) dst[j] = row[j];
            dst[6] = a.channel;
            box_count[b] = cnt + 1;
        }
        for (int j = 0; j < 6; ++j) out[j] = row[j];
        out[6] = place ? 1 : 0;
        out[7] = 0;
        for (int j = 0; j < 8; ++j) k[j] = 0;                      // the scratch is all zero between calls
    }
}

// -------------------------------------------------------------------------------------------------- simulated scribble
// seed / D pass of the simulation: the seeds of region r are the voxels outside it.  Also zeroes last[B][8].
__global__ __launch_bounds__(ST_TPB) void k_strokes_region_d(StSim s, int B, long lines_per_b, int D, float a, int intp,
                                                             float* __restrict__ fields, int32_t* __restrict__ last) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 8 * B; i += ST_TPB) last[i] = 0;
    const int lane = threadIdx.x & 63;
    const long vol = lines_per_b * D, nlines = (long)B * lines_per_b;
    for (long line = (long)blockIdx.x * (ST_TPB / 64) + (threadIdx.x >> 6); line < nlines; line += (long)gridDim.x * (ST_TPB / 64)) {
        const long b = line / lines_per_b, first = (line - b * lines_per_b) * D;
        const long src = line * D;
        float* dst = fields + 2 * b * vol + first;
        st_d_line(D, lane, [&](int p) -> int { return st_region(s, src + p); }, [](int code, int r) -> bool { return code != r + 1; },
                  [&](int r, int p, int dd) { dst[r * vol + p] = edt_d_value(dd, a, intp); });
    }
}

// the class map of the cores, stacked: voxel v of [B stride][W][D]; sample b owns the slabs b stride .. b stride + H - 1
__global__ __launch_bounds__(ST_TPB) void k_strokes_core(const float* __restrict__ fields, long nstack, int stride, int H, int W,
                                                         int D, float ah, float aw, float ad, float min_d2,
                                                         uint8_t* __restrict__ core) {
    const long WD = (long)W * D, vol = (long)H * WD;
    for (long v = (long)blockIdx.x * ST_TPB + threadIdx.x; v < nstack; v += (long)gridDim.x * ST_TPB) {
        const long hs = v / WD;
        const int b = (int)(hs / stride), h = (int)(hs - (long)b * stride);
        uint8_t c = 0;
        if (h < H) {
            const int r2 = (int)(v - hs * WD), w = r2 / D, d = r2 - w * D;
            const long r = (long)h * WD + r2;
            const float f0 = fields[2L * b * vol + r], f1 = fields[(2L * b + 1) * vol + r];
            if (f0 > 0.f || f1 > 0.f) {
                const long long eh = min(h + 1, H - h), ew = min(w + 1, W - w), ed = min(d + 1, D - d);
                const float face = fminf(fminf(ah * (float)(eh * eh), aw * (float)(ew * ew)), ad * (float)(ed * ed));
                if (f0 > 0.f) c = fminf(f0, face) >= min_d2 ? 1 : 0;
                else c = fminf(f1, face) >= min_d2 ? 2 : 0;
            }
        }
        core[v] = c;
    }
}

// commit: grid (blocks per sample, B).  state[1] = the thinning's converged flag
__global__ __launch_bounds__(ST_TPB) void k_strokes_commit(const uint8_t* __restrict__ skel, const int32_t* __restrict__ state,
                                                           long vol, long sample_stride, uint8_t* __restrict__ mask,
                                                           int32_t* __restrict__ last) {
    __shared__ int red[ST_TPB / 64][2];
    const int b = blockIdx.y;
    const uint8_t* sk = skel + (long)b * sample_stride;
    uint8_t* mk = mask + (long)b * vol;
    int add0 = 0, add1 = 0;
    const long span = (long)gridDim.x * ST_TPB;
    for (long v0 = (long)blockIdx.x * ST_TPB; v0 < vol; v0 += span) {      // whole waves enter: the ballots are complete
        const long v = v0 + threadIdx.x;
        int fresh = 0;
        if (v < vol) {
            const int c = sk[v];
            const int bit = c == 1 ? 1 : (c == 2 ? 2 : 0);
            if (bit) {
                const int old = mk[v];
                fresh = bit & ~old;
                if (fresh) mk[v] = (uint8_t)(old | bit);
            }
        }
        add0 += __popcll(__ballot(fresh & 1));
        add1 += __popcll(__ballot(fresh & 2));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = add0; red[threadIdx.x >> 6][1] = add1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int j = threadIdx.x;
        const int sum = red[0][j] + red[1][j] + red[2][j] + red[3][j];
        if (sum) atomicAdd(last + (long)b * 8 + j, sum);
    }
    if (blockIdx.x == 0 && threadIdx.x == 2) last[(long)b * 8 + 2] = state[1];
}

// ---------------------------------------------------------------------------------------------------------- host side
bool st_dims(const int32_t* dims, int32_t B, int& H, int& W, int& D) {
    if (!dims || B < 1 || B > 65535) return false;
    H = dims[0]; W = dims[1]; D = dims[2];
    return H >= 1 && W >= 1 && D >= 1 && H <= 65535 && W <= 65535 && D <= 65535 && (long)B * (H + 2) * W * D < (1L << 31);
}

bool st_spacing(const float* sp) {
    return sp[0] > 0.f && sp[1] > 0.f && sp[2] > 0.f && isfinite(sp[0]) && isfinite(sp[1]) && isfinite(sp[2]);
}

size_t st_round(size_t n) { return (n + 255) / 256 * 256; }

int st_stride(int H) { return H + 1 + ((H + 1) & 1); }            // even, and at least one zero slab behind a sample

int st_dtype_size(int dtype) { return dtype == 0 ? 1 : dtype == 2 ? 8 : 4; }

// the line passes shared by the encoding and the simulation
int st_line_passes(float* fields, int2* stack, int B, int H, int W, int D, const float* spacing, hipStream_t st) {
    const long vol = (long)H * W * D, nf = 2L * B;
    const bool intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    const float ah = spacing[0] * spacing[0], aw = spacing[1] * spacing[1];
    // W pass: lines (h, d) of a field, elements w at stride D; H pass: lines (w, d), elements h at stride W * D
    const long lpf_w = (long)H * D, lpf_h = (long)W * D;
    const long lines_w = nf * lpf_w, lines_h = nf * lpf_h;
    const unsigned grid_w = (unsigned)((lines_w + ST_TPB - 1) / ST_TPB), grid_h = (unsigned)((lines_h + ST_TPB - 1) / ST_TPB);
    if (intp) {
        hipLaunchKernelGGL(k_strokes_line<true>, dim3(grid_w), dim3(ST_TPB), 0, st, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_strokes_line<true>, dim3(grid_h), dim3(ST_TPB), 0, st, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    } else {
        hipLaunchKernelGGL(k_strokes_line<false>, dim3(grid_w), dim3(ST_TPB), 0, st, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_strokes_line<false>, dim3(grid_h), dim3(ST_TPB), 0, st, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    }
    return mivp_check_launch("strokes_line");
}

unsigned st_grid_d(long lines) { return (unsigned)((lines + 3) / 4 > 16384 ? 16384 : (lines + 3) / 4); }
}  // namespace

extern "C" int mivp_strokes_draw(const int32_t* points, int32_t npts, int32_t max_steps, int32_t b, int32_t channel, int32_t B,
                                 const int32_t* dims, uint8_t* mask, mivp_stream_t stream) {
    MIVP_REQUIRE(points && mask && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)points & 3) == 0);
    int H, W, D;
    MIVP_REQUIRE(st_dims(dims, B, H, W, D));
    MIVP_REQUIRE(npts >= 1 && npts <= ST_MAXPTS && b >= 0 && b < B && (channel == 0 || channel == 1));
    MIVP_REQUIRE(max_steps >= 0 && max_steps <= 65534);
    const unsigned segs = (unsigned)(npts > 1 ? npts - 1 : 1);
    hipLaunchKernelGGL(k_strokes_draw, dim3((unsigned)(max_steps / ST_TPB + 1), segs), dim3(ST_TPB), 0, (hipStream_t)stream, points,
                       (int)npts, H, W, D, 1 << channel, mask + (size_t)b * H * W * D);
    return mivp_check_launch("strokes_draw");
}

extern "C" size_t mivp_strokes_ws(int32_t B, const int32_t* dims) {
    int H, W, D;
    if (!st_dims(dims, B, H, W, D)) return 0;
    const size_t n = (size_t)2 * B * H * W * D;
    const int32_t sdims[3] = {B * st_stride(H), W, D};
    const size_t nstack = (size_t)sdims[0] * W * D;
    return st_round(n * sizeof(float)) + st_round(n * sizeof(int2)) + 2 * st_round(nstack) + st_round(mivp_skeleton_ws(sdims)) +
           st_round(2 * sizeof(int32_t));
}

extern "C" int mivp_strokes_encode(const int32_t* boxes, const int32_t* box_count, const uint8_t* mask, int32_t B, int32_t KB,
                                   int32_t Ctot, int32_t channel_offset, const int32_t* dims, const float* spacing,
                                   int32_t frame, int32_t kind, float param, float* out, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(boxes && box_count && mask && spacing && out && workspace);
    MIVP_REQUIRE(KB >= 1 && KB <= ST_MAXKB);
    MIVP_REQUIRE(Ctot >= 2 && channel_offset >= 0 && channel_offset <= Ctot - 2);
    int H, W, D;
    MIVP_REQUIRE(st_dims(dims, B, H, W, D));
    MIVP_REQUIRE(st_spacing(spacing) && (frame == 0 || frame == 1));
    MIVP_REQUIRE((kind == 0 && param > 0.f && isfinite(param)) || (kind == 1 && param >= 0.f && isfinite(param)));
    MIVP_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)boxes & 3) == 0 && ((uintptr_t)workspace & 255) == 0);
    const size_t n = (size_t)2 * B * H * W * D;
    float* fields = (float*)workspace;
    int2* stack = (int2*)((char*)workspace + st_round(n * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    const int intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    const long lines_d = (long)B * H * W;
    hipLaunchKernelGGL(k_strokes_seed, dim3(st_grid_d(lines_d)), dim3(ST_TPB), 0, st, mask, lines_d, (long)H * W, D,
                       spacing[2] * spacing[2], intp, fields);
    int rc = mivp_check_launch("strokes_seed");
    if (rc != MIVP_OK) return rc;
    rc = st_line_passes(fields, stack, B, H, W, D, spacing, st);
    if (rc != MIVP_OK) return rc;
    StEnc e;
    e.run.H = H; e.run.W = W; e.run.D = D; e.run.KB = KB; e.run.Ctot = Ctot; e.run.off = channel_offset; e.run.frame = frame;
    e.kind = kind; e.param = param;
    hipLaunchKernelGGL(k_strokes_close, dim3(guide_grid((long)H * W * D), (unsigned)B), dim3(ST_TPB), 0, st, boxes, box_count,
                       (const float*)fields, e, out);
    return mivp_check_launch("strokes_close");
}

extern "C" int mivp_strokes_box(const void* target, int32_t target_dtype, int32_t B, const int32_t* dims, uint32_t object_mask,
                                int32_t ignore_index, int32_t has_ignore, const int32_t* margin, const int32_t* jitter,
                                int32_t channel, int32_t KB, int32_t* boxes, int32_t* box_count, int32_t* last, int32_t* scratch,
                                mivp_stream_t stream) {
    MIVP_REQUIRE(target && margin && boxes && box_count && last && scratch);
    MIVP_REQUIRE(target_dtype >= 0 && target_dtype <= 3 && KB >= 1 && KB <= ST_MAXKB && (channel == 0 || channel == 1));
    int H, W, D;
    MIVP_REQUIRE(st_dims(dims, B, H, W, D));
    MIVP_REQUIRE(margin[0] >= 0 && margin[1] >= 0 && margin[2] >= 0);
    MIVP_REQUIRE(((uintptr_t)target & (uintptr_t)(st_dtype_size(target_dtype) - 1)) == 0);
    MIVP_REQUIRE((((uintptr_t)boxes | (uintptr_t)box_count | (uintptr_t)last | (uintptr_t)scratch | (uintptr_t)jitter) & 3) == 0);
    const StSim s = {nullptr, target, 0, target_dtype, object_mask, has_ignore ? 1 : 0, ignore_index};
    const long vol = (long)H * W * D;
    const unsigned gx = (unsigned)((vol + ST_TPB - 1) / ST_TPB > 1024 ? 1024 : (vol + ST_TPB - 1) / ST_TPB);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_strokes_box_reduce, dim3(gx, (unsigned)B), dim3(ST_TPB), 0, st, s, H, W, D, scratch);
    int rc = mivp_check_launch("strokes_box_reduce");
    if (rc != MIVP_OK) return rc;
    const StBoxArgs a = {{H, W, D}, {margin[0], margin[1], margin[2]}, KB, channel};
    hipLaunchKernelGGL(k_strokes_box_finalize, dim3(1), dim3(ST_TPB), 0, st, scratch, jitter, (int)B, a, boxes, box_count, last);
    return mivp_check_launch("strokes_box_finalize");
}

extern "C" int mivp_strokes_scribbles(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t B,
                                      const int32_t* dims, const float* spacing, uint32_t object_mask, int32_t ignore_index,
                                      int32_t has_ignore, float min_depth_sq, int32_t max_iter, int32_t keep_endpoints,
                                      uint8_t* mask, int32_t* last, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(pred && target && spacing && mask && last && workspace);
    MIVP_REQUIRE(pred_dtype >= 0 && pred_dtype <= 3 && target_dtype >= 0 && target_dtype <= 3);
    MIVP_REQUIRE(min_depth_sq >= 0.f && isfinite(min_depth_sq) && max_iter >= 1 && max_iter <= 4096);
    MIVP_REQUIRE(keep_endpoints == 0 || keep_endpoints == 1);
    int H, W, D;
    MIVP_REQUIRE(st_dims(dims, B, H, W, D));
    MIVP_REQUIRE(st_spacing(spacing));
    MIVP_REQUIRE(((uintptr_t)pred & (uintptr_t)(st_dtype_size(pred_dtype) - 1)) == 0);
    MIVP_REQUIRE(((uintptr_t)target & (uintptr_t)(st_dtype_size(target_dtype) - 1)) == 0);
    MIVP_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)last & 3) == 0);
    const long vol = (long)H * W * D;
    const size_t n = (size_t)2 * B * vol;
    const int stride = st_stride(H);
    const int32_t sdims[3] = {B * stride, W, D};
    const long nstack = (long)sdims[0] * W * D;
    char* at = (char*)workspace;
    float* fields = (float*)at;               at += st_round(n * sizeof(float));
    int2* stack = (int2*)at;                  at += st_round(n * sizeof(int2));
    uint8_t* core = (uint8_t*)at;             at += st_round((size_t)nstack);
    uint8_t* skel = (uint8_t*)at;             at += st_round((size_t)nstack);
    void* skws = at;                          at += st_round(mivp_skeleton_ws(sdims));
    int32_t* state = (int32_t*)at;
    hipStream_t st = (hipStream_t)stream;
    const int intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    const float ah = spacing[0] * spacing[0], aw = spacing[1] * spacing[1], ad = spacing[2] * spacing[2];
    const StSim s = {pred, target, pred_dtype, target_dtype, object_mask, has_ignore ? 1 : 0, ignore_index};
    const long lines_d = (long)B * H * W;
    hipLaunchKernelGGL(k_strokes_region_d, dim3(st_grid_d(lines_d)), dim3(ST_TPB), 0, st, s, (int)B, (long)H * W, D, ad, intp, fields,
                       last);
    int rc = mivp_check_launch("strokes_region_d");
    if (rc != MIVP_OK) return rc;
    rc = st_line_passes(fields, stack, B, H, W, D, spacing, st);
    if (rc != MIVP_OK) return rc;
    const unsigned gc = (unsigned)((nstack + ST_TPB - 1) / ST_TPB > 65536 ? 65536 : (nstack + ST_TPB - 1) / ST_TPB);
    hipLaunchKernelGGL(k_strokes_core, dim3(gc), dim3(ST_TPB), 0, st, (const float*)fields, nstack, stride, H, W, D, ah, aw, ad,
                       min_depth_sq, core);
    rc = mivp_check_launch("strokes_core");
    if (rc != MIVP_OK) return rc;
    rc = mivp_skeleton_begin(core, 0, sdims, 3, 6u, skel, skws, stream);
    for (int it = 1; rc == MIVP_OK && it <= max_iter; ++it) rc = mivp_skeleton_iter(skel, sdims, keep_endpoints, it, skws, stream);
    if (rc == MIVP_OK) rc = mivp_skeleton_end(skws, max_iter, state, state + 1, stream);
    if (rc != MIVP_OK) return rc;
    const unsigned gx = (unsigned)((vol + ST_TPB - 1) / ST_TPB > 1024 ? 1024 : (vol + ST_TPB - 1) / ST_TPB);
    hipLaunchKernelGGL(k_strokes_commit, dim3(gx, (unsigned)B), dim3(ST_TPB), 0, st, (const uint8_t*)skel, (const int32_t*)state, vol,
                       (long)stride * W * D, mask, last);
    return mivp_check_launch("strokes_commit");
}
