// Interactive click prompts (mivp_amd/clicks.py): positive / negative clicks as two guidance channels of the
// model input, and the simulated corrective click of iterative training (RITM, DeepEdit, SAM-Med3D, nnInteractive).
//
// The device record of a batch (ClickSlot): clicks i32 [B][K][4] = (h, w, d, channel; 0 positive, 1 negative, anything else an
// empty entry), count i32 [B], last i32 [B][4] = (bits of the winning depth^2, channel, raster index, placed flag).  K <= 64.
//
// 1. mivp_clicks_encode, one launch: out f32 [B][Ctot][H][W][D], channels off and off + 1 of every sample, each element stored
//    once, nothing else touched.  m = min over the channel's clicks of the squared distance in mm (+inf without a click);
//    gaussian: expf(-m / (2 sigma^2)), disk: m <= radius^2 ? 1 : 0.  The two channels of a sample are one contiguous run of
//    2 vol floats whose start is aligned to 4 bytes only (vol may be odd): a workgroup row walks the run as [head of 0..3
//    scalars][16-byte quads][tail of 0..3 scalars], so every store that can be 16 bytes wide is.  The sample's clicks are
//    compacted per channel into LDS by wave 0 (two ballots), count is read on the device: a recording follows the slot.
//
// 2. mivp_clicks_simulate, five launches whatever B and the data are, each unconditional, nothing read back:
//      seed / D   one wave per (region, b, h, w) line (the scheme of k_hausdorff_d): a voxel's region from the two class maps
//                 (or the argmax of the logits, fused: the lowest index among exact maxima), E_pos = target in the object and
//                 pred not, E_neg = pred in the object and a valid target not.  fields f32 [2][B][vol] = squared distance along
//                 D to the nearest voxel outside the region (0 outside it, +inf on a line that lies inside it).
//      W, H       edt_line of csrc/edt_common.hpp, one thread per line over the 2 B fields.
//      pick       depth^2 = min(field, (distance along an axis to the nearest face)^2): the outside of the volume counts as
//                 outside (the transform of the mask padded by one voxel).  key = bits(depth^2) << 32 | positive << 31 |
//                 (2^31 - 1 - raster index); workgroup maximum, then ONE 64-bit integer atomicMax per workgroup: the largest
//                 depth, ties to the positive region, then to the lowest raster index, whatever the order of arrival.
//      commit     one thread per sample: last[b] always; the click is appended iff a region exists, depth^2 >= min_depth^2
//                 and count[b] < K.
//    At unit spacing every value is the exact integer.  Limits: H, W <= 65535, H W D < 2^31.
#include "edt_common.hpp"

namespace {
constexpr int CK_TPB = 256;
constexpr int CK_MAXK = 64;
constexpr int CK_MAXCLS = 32;                                  // labels are classes 0 .. 31; the object is a 32-bit mask
constexpr int CK_LOGITS = 4;                                   // pred dtype code: f32 logits [B][vol][C], channels last

// ------------------------------------------------------------------------------------------------------------ encoding
struct CkEnc {
    int H, W, D, K, Ctot, off, kind, intp;
    float ah, aw, ad, param;                                   // squared spacings; 2 sigma^2 (gaussian) or radius^2 (disk)
};

MIVP_DEV float ck_value(float m, const CkEnc& e) { return e.kind == 0 ? expf(-m / e.param) : (m <= e.param ? 1.f : 0.f); }

MIVP_DEV float ck_dist(int dh, int dw, int dd, const CkEnc& e) {
    const float fh = (float)dh * (float)dh, fw = (float)dw * (float)dw, fd = (float)dd * (float)dd;   // exact below 4096
    return e.intp ? (fh + fw) + fd : (e.ah * fh + e.aw * fw) + e.ad * fd;
}

// grid (blocks per sample, B).  lst[ch][i] = (h, w, d) of click i of channel ch, n[ch] of them.
__global__ __launch_bounds__(CK_TPB) void k_clicks_encode(const int32_t* __restrict__ clicks, const int32_t* __restrict__ count,
                                                          CkEnc e, float* __restrict__ out) {
    __shared__ int4 lst[2][CK_MAXK];
    __shared__ int n[2];
    const int b = blockIdx.y;
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const int cnt = min(max(count[b], 0), e.K);
        int4 c = make_int4(0, 0, 0, -1);
        if (lane < cnt) c = *reinterpret_cast<const int4*>(clicks + ((long)b * e.K + lane) * 4);
        for (int ch = 0; ch < 2; ++ch) {
            const unsigned long long m = __ballot(c.w == ch);
            if (c.w == ch) lst[ch][__popcll(m & ((1ull << lane) - 1))] = c;
            if (lane == 0) n[ch] = __popcll(m);
        }
    }
    __syncthreads();
    const long vol = (long)e.H * e.W * e.D;
    const long run = 2 * vol;                                      // the two guidance channels of sample b
    float* base = out + ((long)b * e.Ctot + e.off) * vol;
    const long head = min((long)((16 - ((uintptr_t)base & 15)) & 15) >> 2, run);
    const long nq = (run - head) >> 2;
    const long tail0 = head + 4 * nq;                              // first element of the tail
    const int WD = e.W * e.D;
    // value of element el of the run
    auto one = [&](long el) -> float {
        const int ch = el >= vol ? 1 : 0;
        const int r = (int)(el - (ch ? vol : 0L));
        const int h = r / WD, w = (r - h * WD) / e.D, d = r - h * WD - w * e.D;
        float m = INFINITY;
        for (int i = 0; i < n[ch]; ++i) {
            const int4 c = lst[ch][i];
            m = fminf(m, ck_dist(h - c.x, w - c.y, d - c.z, e));
        }
        return ck_value(m, e);
    };
    for (long q = (long)blockIdx.x * CK_TPB + threadIdx.x; q <= nq; q += (long)gridDim.x * CK_TPB) {
        if (q == nq) {                                             // the one item of the unaligned ends
            for (long el = 0; el < head; ++el) base[el] = one(el);
            for (long el = tail0; el < run; ++el) base[el] = one(el);
            continue;
        }
        const long el = head + 4 * q;
        const int ch = el >= vol ? 1 : 0;
        const int r = (int)(el - (ch ? vol : 0L));
        const int h = r / WD, w = (r - h * WD) / e.D, d = r - h * WD - w * e.D;
        float4 v;
        if (d + 3 < e.D) {                                         // four voxels of one line: the (h, w) part once per click
            float m0 = INFINITY, m1 = INFINITY, m2 = INFINITY, m3 = INFINITY;
            for (int i = 0; i < n[ch]; ++i) {
                const int4 c = lst[ch][i];
                const int dh = h - c.x, dw = w - c.y, dd = d - c.z;
                m0 = fminf(m0, ck_dist(dh, dw, dd, e));
                m1 = fminf(m1, ck_dist(dh, dw, dd + 1, e));
                m2 = fminf(m2, ck_dist(dh, dw, dd + 2, e));
                m3 = fminf(m3, ck_dist(dh, dw, dd + 3, e));
            }
            v = make_float4(ck_value(m0, e), ck_value(m1, e), ck_value(m2, e), ck_value(m3, e));
        } else {
            v = make_float4(one(el), one(el + 1), one(el + 2), one(el + 3));
        }
        *reinterpret_cast<float4*>(base + el) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------- simulation
struct CkSim {
    const void* pred;
    const void* target;
    int pdt, tdt, C;                                           // dtype codes (0 uint8, 1 int32, 2 int64, 3 float32, pred 4: logits)
    unsigned mask;                                             // the object's classes
    int has_ignore, ignore;
};

// class 0 .. 31 of element i of a label map, -1 for anything else
MIVP_DEV int ck_label(const void* p, int dt, long i) {
    switch (dt) {
        case 0: return class_of<uint8_t>(static_cast<const uint8_t*>(p)[i], CK_MAXCLS);
        case 1: return class_of<int32_t>(static_cast<const int32_t*>(p)[i], CK_MAXCLS);
        case 2: return class_of<long long>(static_cast<const long long*>(p)[i], CK_MAXCLS);
        default: return class_of<float>(static_cast<const float*>(p)[i], CK_MAXCLS);
    }
}

// region of voxel i of the batch: 0 none, 1 E_pos (false negative), 2 E_neg (false positive)
MIVP_DEV int ck_region(const CkSim& s, long i) {
    const int t = ck_label(s.target, s.tdt, i);
    if (t < 0 || (s.has_ignore && t == s.ignore)) return 0;
    int p;
    if (s.pdt == CK_LOGITS) {                                      // the first maximum of the C logits (hd_argmax)
        const float* zv = static_cast<const float*>(s.pred) + i * s.C;
        p = 0;
        float m = zv[0];
        for (int c = 1; c < s.C; ++c) {
            const float z = zv[c];
            if (z > m) { m = z; p = c; }
        }
    } else {
        p = ck_label(s.pred, s.pdt, i);
    }
    const bool tin = (s.mask >> t) & 1u, pin = p >= 0 && p < CK_MAXCLS && ((s.mask >> p) & 1u);
    return tin == pin ? 0 : (tin ? 1 : 2);
}

// seed / D pass.  Wave line wl < 2 B H W: region = wl / (B H W), then the (b, h, w) line.  Lane r < 2 owns the sweep state
// of region r, as in k_hausdorff_d; the seeds of region r are the voxels outside it.  Also zeroes best[B].
__global__ __launch_bounds__(CK_TPB) void k_clicks_d(CkSim s, int B, long lines_per_b, int D, float a, int intp,
                                                     float* __restrict__ fields, unsigned long long* __restrict__ best) {
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < B; b += CK_TPB) best[b] = 0ull;
    const int lane = threadIdx.x & 63;
    const int nch = (D + 63) >> 6;
    const long nlines = (long)B * lines_per_b;
    for (long line = (long)blockIdx.x * (CK_TPB / 64) + (threadIdx.x >> 6); line < nlines; line += (long)gridDim.x * (CK_TPB / 64)) {
        const long first = line * D;                               // voxel index of the line's start in the batch
        auto reg_at = [&](int p) -> int { return p < D ? ck_region(s, first + p) : -1; };
        int prev = -EDT_NO_SEED, next = -1;
        for (int k = 0; k < nch; ++k) {
            const int p = 64 * k + lane;
            const int rg = reg_at(p);
            for (int r = 0; r < 2; ++r) {
                const unsigned long long m = __ballot(p < D && rg != r + 1);
                const unsigned long long ml = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
                const unsigned long long mr = m & (~0ull << lane);
                const int pv = __shfl(prev, r);
                int nx = __shfl(next, r);
                const int left = ml ? 64 * k + 63 - __builtin_clzll(ml) : pv;
                if (!(m >> 63) && nx <= 64 * k + 63) {             // wave-uniform: some lanes need the next seed
                    nx = EDT_NO_SEED;
                    for (int j = k + 1; j < nch; ++j) {
                        const int q = 64 * j + lane;
                        const int rq = reg_at(q);
                        const unsigned long long mm = __ballot(q < D && rq != r + 1);
                        if (mm) { nx = 64 * j + __builtin_ctzll(mm); break; }
                    }
                }
                const int right = mr ? 64 * k + __builtin_ctzll(mr) : nx;
                if (lane == r) {
                    next = nx;
                    if (m) prev = 64 * k + 63 - __builtin_clzll(m);
                }
                if (p < D) fields[(long)r * nlines * D + first + p] = edt_d_value(min(p - left, right - p), a, intp);
            }
        }
    }
}

// W / H pass over the 2 B fields: line = field * lines_per_field + (outer, inner), inner = d fastest across lanes
template <bool INTP>
__global__ __launch_bounds__(CK_TPB) void k_clicks_line(float* __restrict__ fields, long nlines, long lines_per_field, long vol,
                                                        int inner, long outer_stride, long stride, int n, float a,
                                                        int2* __restrict__ stack) {
    const long line = (long)blockIdx.x * CK_TPB + threadIdx.x;
    if (line >= nlines) return;
    const long field = line / lines_per_field, l = line - field * lines_per_field;
    edt_line<INTP>(fields + field * vol + (l / inner) * outer_stride + (l % inner), stride, n, a, stack, nlines, line);
}

MIVP_DEV unsigned long long ck_shfl_xor(unsigned long long v, int sh) {
    const unsigned lo = __shfl_xor((unsigned)v, sh), hi = __shfl_xor((unsigned)(v >> 32), sh);
    return ((unsigned long long)hi << 32) | lo;
}

// pick: grid (blocks per sample, B)
__global__ __launch_bounds__(CK_TPB) void k_clicks_pick(const float* __restrict__ fields, int B, int H, int W, int D, float ah,
                                                        float aw, float ad, unsigned long long* __restrict__ best) {
    __shared__ unsigned long long red[CK_TPB / 64];
    const int b = blockIdx.y;
    const int vol = H * W * D, WD = W * D;
    unsigned long long key = 0ull;
    for (long lv = (long)blockIdx.x * CK_TPB + threadIdx.x; lv < vol; lv += (long)gridDim.x * CK_TPB) {
        const int v = (int)lv;
        const float f0 = fields[(long)b * vol + v], f1 = fields[((long)B + b) * vol + v];
        if (!(f0 > 0.f) && !(f1 > 0.f)) continue;
        const int h = v / WD, w = (v - h * WD) / D, d = v - h * WD - w * D;
        const long long eh = min(h + 1, H - h), ew = min(w + 1, W - w), ed = min(d + 1, D - d);
        const float face = fminf(fminf(ah * (float)(eh * eh), aw * (float)(ew * ew)), ad * (float)(ed * ed));
        const unsigned inv = 0x7fffffffu - (unsigned)v;
        if (f0 > 0.f) key = max(key, ((unsigned long long)__float_as_uint(fminf(f0, face)) << 32) | 0x80000000u | inv);
        if (f1 > 0.f) key = max(key, ((unsigned long long)__float_as_uint(fminf(f1, face)) << 32) | inv);
    }
    for (int sh = 32; sh > 0; sh >>= 1) key = max(key, ck_shfl_xor(key, sh));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        key = max(max(red[0], red[1]), max(red[2], red[3]));
        if (key) atomicMax(best + b, key);
    }
}

__global__ __launch_bounds__(64) void k_clicks_commit(const unsigned long long* __restrict__ best, int B, int K, int W, int D,
                                                      float min_d2, int32_t* __restrict__ clicks, int32_t* __restrict__ count,
                                                      int32_t* __restrict__ last) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const unsigned long long key = best[b];
    int4 out = make_int4(0, -1, -1, 0);
    if (key) {
        const unsigned bits = (unsigned)(key >> 32);
        const int ch = (key & 0x80000000ull) ? 0 : 1;
        const int v = (int)(0x7fffffffu - ((unsigned)key & 0x7fffffffu));
        const int cnt = count[b];
        const bool place = __uint_as_float(bits) >= min_d2 && cnt >= 0 && cnt < K;
        if (place) {
            const int WD = W * D, h = v / WD, w = (v - h * WD) / D;
            *reinterpret_cast<int4*>(clicks + ((long)b * K + cnt) * 4) = make_int4(h, w, v - h * WD - w * D, ch);
            count[b] = cnt + 1;
        }
        out = make_int4((int)bits, ch, v, place ? 1 : 0);
    }
    *reinterpret_cast<int4*>(last + (long)b * 4) = out;
}

bool ck_dims(const int32_t* dims, int& H, int& W, int& D) {
    H = dims[0]; W = dims[1]; D = dims[2];
    return H >= 1 && W >= 1 && D >= 1 && H <= 65535 && W <= 65535 && (long)H * W * D < (1L << 31);
}

bool ck_spacing(const float* sp) {
    return sp[0] > 0.f && sp[1] > 0.f && sp[2] > 0.f && isfinite(sp[0]) && isfinite(sp[1]) && isfinite(sp[2]);
}

size_t ck_round(size_t n) { return (n + 255) / 256 * 256; }
}  // namespace

extern "C" int mivp_clicks_encode(const int32_t* clicks, const int32_t* count, int32_t B, int32_t K, int32_t Ctot,
                                  int32_t channel_offset, const int32_t* dims, const float* spacing, int32_t kind, float param,
                                  float* out, mivp_stream_t stream) {
    MIVP_REQUIRE(clicks && count && dims && spacing && out);
    MIVP_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && K <= CK_MAXK);
    MIVP_REQUIRE(Ctot >= 2 && channel_offset >= 0 && channel_offset <= Ctot - 2);
    int H, W, D;
    MIVP_REQUIRE(ck_dims(dims, H, W, D) && D <= 65535);            // squared index differences stay below 2^32
    MIVP_REQUIRE(ck_spacing(spacing));
    MIVP_REQUIRE((kind == 0 && param > 0.f && isfinite(param)) || (kind == 1 && param >= 0.f && isfinite(param)));
    MIVP_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)clicks & 15) == 0);
    CkEnc e;
    e.H = H; e.W = W; e.D = D; e.K = K; e.Ctot = Ctot; e.off = channel_offset; e.kind = kind;
    e.intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    e.ah = spacing[0] * spacing[0]; e.aw = spacing[1] * spacing[1]; e.ad = spacing[2] * spacing[2];
    e.param = param;
    const long items = (2L * H * W * D) / 4 + 1;
    const unsigned gx = (unsigned)((items + CK_TPB - 1) / CK_TPB > 8192 ? 8192 : (items + CK_TPB - 1) / CK_TPB);
    hipLaunchKernelGGL(k_clicks_encode, dim3(gx, (unsigned)B), dim3(CK_TPB), 0, (hipStream_t)stream, clicks, count, e, out);
    return mivp_check_launch("clicks_encode");
}

extern "C" size_t mivp_clicks_simulate_ws(int32_t B, const int32_t* dims) {
    int H, W, D;
    if (!dims || B < 1 || B > 65535 || !ck_dims(dims, H, W, D)) return 0;
    const size_t n = (size_t)2 * B * H * W * D;
    return ck_round(n * sizeof(float)) + ck_round(n * sizeof(int2)) + ck_round((size_t)B * sizeof(unsigned long long));
}

extern "C" int mivp_clicks_simulate(const void* pred, int32_t pred_dtype, int32_t C, const void* target, int32_t target_dtype,
                                    int32_t B, const int32_t* dims, const float* spacing, uint32_t object_mask,
                                    int32_t ignore_index, int32_t has_ignore, float min_depth_sq, int32_t K, int32_t* clicks,
                                    int32_t* count, int32_t* last, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(pred && target && dims && spacing && clicks && count && last && workspace);
    MIVP_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && K <= CK_MAXK);
    MIVP_REQUIRE(pred_dtype >= 0 && pred_dtype <= CK_LOGITS && target_dtype >= 0 && target_dtype <= 3);
    MIVP_REQUIRE(pred_dtype != CK_LOGITS || (C >= 1 && C <= CK_MAXCLS));
    MIVP_REQUIRE(min_depth_sq >= 0.f && isfinite(min_depth_sq));
    int H, W, D;
    MIVP_REQUIRE(ck_dims(dims, H, W, D));                          // H, W <= 65535: the 16-bit sites of the envelope's stack
    MIVP_REQUIRE(ck_spacing(spacing));
    MIVP_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)clicks & 15) == 0 && ((uintptr_t)last & 15) == 0);
    const long vol = (long)H * W * D;
    const size_t n = (size_t)2 * B * vol;
    float* fields = (float*)workspace;
    int2* stack = (int2*)((char*)workspace + ck_round(n * sizeof(float)));
    unsigned long long* best = (unsigned long long*)((char*)stack + ck_round(n * sizeof(int2)));
    const bool intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    const float ah = spacing[0] * spacing[0], aw = spacing[1] * spacing[1], ad = spacing[2] * spacing[2];
    hipStream_t st = (hipStream_t)stream;
    const CkSim s = {pred, target, pred_dtype, target_dtype, C, object_mask, has_ignore ? 1 : 0, ignore_index};
    const long lines_d = (long)B * H * W;
    const unsigned grid_d = (unsigned)((lines_d + 3) / 4 > 16384 ? 16384 : (lines_d + 3) / 4);
    hipLaunchKernelGGL(k_clicks_d, dim3(grid_d), dim3(CK_TPB), 0, st, s, (int)B, (long)H * W, D, ad, (int)intp, fields, best);
    int rc = mivp_check_launch("clicks_d");
    if (rc != MIVP_OK) return rc;
    // W pass: lines (h, d) of a field, elements w at stride D; H pass: lines (w, d), elements h at stride W * D
    const long nf = 2L * B;
    const long lpf_w = (long)H * D, lpf_h = (long)W * D;
    const long lines_w = nf * lpf_w, lines_h = nf * lpf_h;
    const unsigned grid_w = (unsigned)((lines_w + CK_TPB - 1) / CK_TPB), grid_h = (unsigned)((lines_h + CK_TPB - 1) / CK_TPB);
    if (intp) {
        hipLaunchKernelGGL(k_clicks_line<true>, dim3(grid_w), dim3(CK_TPB), 0, st, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_clicks_line<true>, dim3(grid_h), dim3(CK_TPB), 0, st, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    } else {
        hipLaunchKernelGGL(k_clicks_line<false>, dim3(grid_w), dim3(CK_TPB), 0, st, fields, lines_w, lpf_w, vol, D, (long)W * D,
                           (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_clicks_line<false>, dim3(grid_h), dim3(CK_TPB), 0, st, fields, lines_h, lpf_h, vol, D, (long)D,
                           (long)W * D, H, ah, stack);
    }
    rc = mivp_check_launch("clicks_line");
    if (rc != MIVP_OK) return rc;
    const unsigned gx = (unsigned)((vol + CK_TPB - 1) / CK_TPB > 1024 ? 1024 : (vol + CK_TPB - 1) / CK_TPB);
    hipLaunchKernelGGL(k_clicks_pick, dim3(gx, (unsigned)B), dim3(CK_TPB), 0, st, fields, (int)B, H, W, D, ah, aw, ad, best);
    rc = mivp_check_launch("clicks_pick");
    if (rc != MIVP_OK) return rc;
    hipLaunchKernelGGL(k_clicks_commit, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, best, (int)B, (int)K, W, D, min_depth_sq,
                       clicks, count, last);
    return mivp_check_launch("clicks_commit");
}
