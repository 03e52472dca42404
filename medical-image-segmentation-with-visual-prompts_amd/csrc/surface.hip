// Surface-distance metrics (ABI 15, mivp_amd/surface.py): surface maps of two label maps, an exact 3-D Euclidean
// distance transform (EDT) to the surface voxels of one class, and the statistics of that transform sampled at the other
// map's surface voxels (maximum, an exact order statistic, the count within a tolerance and the sum of distances).
//
// Volumes are [H][W][D] row-major (D contiguous).  Squared distances are float32, +inf where there is no seed.
//
// EDT = three separable passes over one float buffer:
//   D pass  one wave per (h, w) line, 64 consecutive d per step: the nearest seed on each side comes from the step's
//           ballot plus the last seed of the earlier steps and a look-ahead for the first seed of the later ones.
//   W, H    one thread per line, adjacent lanes on adjacent d, so every step of a wave reads one contiguous 256-byte
//   passes  row.  Meijster's lower envelope of parabolas a (x - i)^2 + f(i); the stack (site | boundary << 16, f(site))
//           lives in a workspace laid out [depth][line], in place over the float buffer.  With unit spacing the
//           envelope's intersections are integer floor divisions, so every squared distance is the exact integer.
//
// Statistics of one (class, direction) without float atomics: one pass over the sampled map builds a 32768-bin LDS
// histogram of the key's high 16 bits (the bits of a non-negative float order like the float), a float64 partial sum
// per workgroup in a slab, an integer max and an integer count within the tolerance.  One workgroup finds the bins of the
// two ranks P_p needs (from the device-resident surface count), and sums the slab in a fixed order.  A second pass
// histograms the low 16 bits inside the lower rank's bin (16-bit LDS counters, two per word) and takes the minimum low
// half inside the upper rank's bin when that is another bin; one workgroup finishes the select.
#include "edt_common.hpp"
#include <limits.h>

namespace {
constexpr int MAXC = 16;
constexpr int TPB = 256;
constexpr int SEL_TPB = 1024;
constexpr int HI_BINS = 32768;      // high 16 bits of a non-negative float key (sign clear)
constexpr int LO_BINS = 65536;
constexpr int SAMPLE_VOX = 32768;   // voxels per sampling workgroup: bounds a 16-bit LDS counter below 65536
constexpr int NO_SEED = EDT_NO_SEED;

// one thread per voxel of both maps: class id on surface voxels (6-neighbourhood, the outside counts as background),
// 255 elsewhere; per-class counts summed in LDS, one integer atomic per (class, map) and workgroup
template <typename T>
__global__ __launch_bounds__(TPB) void k_surface_map(const T* __restrict__ pred, const T* __restrict__ target, int C, int H,
                                                     int W, int D, uint8_t* __restrict__ sp, uint8_t* __restrict__ st,
                                                     unsigned long long* __restrict__ counts) {
    __shared__ unsigned int sm[MAXC * 2];
    for (int i = threadIdx.x; i < MAXC * 2; i += TPB) sm[i] = 0u;
    __syncthreads();
    const long nvox = (long)H * W * D;
    const long sW = D, sH = (long)W * D;
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < nvox; v += (long)gridDim.x * TPB) {
        const int d = (int)(v % D);
        const long r = v / D;
        const int w = (int)(r % W);
        const int h = (int)(r / W);
        for (int m = 0; m < 2; ++m) {
            const T* lab = m == 0 ? pred : target;
            uint8_t* out = m == 0 ? sp : st;
            if (!lab) continue;
            const int c = class_of<T>(lab[v], C);
            bool surf = false;
            if (c >= 0) {
                surf = h == 0 || h == H - 1 || w == 0 || w == W - 1 || d == 0 || d == D - 1;
                if (!surf)
                    surf = class_of<T>(lab[v - sH], C) != c || class_of<T>(lab[v + sH], C) != c ||
                           class_of<T>(lab[v - sW], C) != c || class_of<T>(lab[v + sW], C) != c ||
                           class_of<T>(lab[v - 1], C) != c || class_of<T>(lab[v + 1], C) != c;
            }
            out[v] = surf ? (uint8_t)c : (uint8_t)255;
            if (surf && counts) atomicAdd(&sm[c * 2 + m], 1u);
        }
    }
    if (!counts) return;
    __syncthreads();
    for (int i = threadIdx.x; i < C * 2; i += TPB)
        if (sm[i]) atomicAdd(&counts[i], (unsigned long long)sm[i]);
}

// D pass: one wave per (h, w) line; f = a (d - nearest seed)^2, +inf for a line without a seed
__global__ __launch_bounds__(TPB) void k_edt_d(const uint8_t* __restrict__ smap, int cls, long nlines, int D, float a,
                                               int intp, float* __restrict__ f) {
    const int lane = threadIdx.x & 63;
    const int nch = (D + 63) >> 6;
    for (long line = (long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); line < nlines; line += (long)gridDim.x * (TPB / 64)) {
        const uint8_t* row = smap + line * D;
        float* out = f + line * D;
        int prev = -NO_SEED;                                   // last seed before the current step
        int next = -1;                                         // first seed after some step (stale once passed)
        for (int k = 0; k < nch; ++k) {
            const int p = 64 * k + lane;
            const unsigned long long m = __ballot(p < D && row[p] == cls);
            const unsigned long long ml = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1));
            const unsigned long long mr = m & (~0ull << lane);
            const int left = ml ? 64 * k + 63 - __builtin_clzll(ml) : prev;
            if (!(m >> 63) && next <= 64 * k + 63) {           // wave-uniform: some lanes need the next seed
                next = NO_SEED;
                for (int j = k + 1; j < nch; ++j) {
                    const int q = 64 * j + lane;
                    const unsigned long long mm = __ballot(q < D && row[q] == cls);
                    if (mm) { next = 64 * j + __builtin_ctzll(mm); break; }
                }
            }
            const int right = mr ? 64 * k + __builtin_ctzll(mr) : next;
            if (m) prev = 64 * k + 63 - __builtin_clzll(m);
            if (p >= D) continue;
            out[p] = edt_d_value(min(p - left, right - p), a, intp);
        }
    }
}

// W / H pass: Meijster's lower envelope along one axis of n elements at `stride`, in place over f (edt_line of
// csrc/edt_common.hpp, shared with csrc/distmap.hip).  Lines are (outer, inner) pairs, inner = d fastest across lanes; stack
// entries [depth][line] = (site | boundary << 16, bits of f(site)).
template <bool INTP>
__global__ __launch_bounds__(TPB) void k_edt_line(float* __restrict__ f, long nlines, int inner, long outer_stride,
                                                  long stride, int n, float a, int2* __restrict__ stack) {
    const long line = (long)blockIdx.x * TPB + threadIdx.x;
    if (line >= nlines) return;
    edt_line<INTP>(f + (line / inner) * outer_stride + (line % inner), stride, n, a, stack, nlines, line);
}

// ---------------------------------------------------------------------------------------------------- statistics
struct StatWs {                  // device workspace of one (class, direction), zeroed before each use
    unsigned int hist_hi[HI_BINS];
    unsigned int hist_lo[LO_BINS];
    unsigned long long within;
    unsigned int maxkey;
    unsigned int min_hi;         // smallest low half in the upper rank's bin (when it is another bin)
    int state[4];                // bin_lo, rank of P_lo in it, bin_hi, rank of P_hi in it (-1: nothing to select)
};

MIVP_DEV unsigned int wave_max(unsigned int v) {
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, o));
    return v;
}
MIVP_DEV unsigned int wave_min(unsigned int v) {
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (unsigned int)__shfl_xor((int)v, o));
    return v;
}
MIVP_DEV unsigned long long wave_sum_u64(unsigned long long v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
MIVP_DEV double wave_sum_f64(double v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// pass 1 over the sampled map: high-half histogram, max key, count within tau, float64 partial sum per workgroup
__global__ __launch_bounds__(TPB) void k_stat_hi(const uint8_t* __restrict__ smap, int cls, const float* __restrict__ dist,
                                                 long nvox, double tau, StatWs* __restrict__ ws, double* __restrict__ slab) {
    __shared__ unsigned int hist[HI_BINS];
    __shared__ unsigned int rmax[TPB / 64];
    __shared__ unsigned long long rcnt[TPB / 64];
    __shared__ double rsum[TPB / 64];
    for (int i = threadIdx.x; i < HI_BINS; i += TPB) hist[i] = 0u;
    __syncthreads();
    unsigned int mx = 0u;
    unsigned long long cnt = 0;
    double sum = 0.0;
    const long v0 = (long)blockIdx.x * SAMPLE_VOX;
    const long v1 = min(v0 + SAMPLE_VOX, nvox);
    for (long v = v0 + threadIdx.x; v < v1; v += TPB) {
        if (smap[v] != cls) continue;
        const float d2 = dist[v];
        const unsigned int key = __float_as_uint(d2);
        atomicAdd(&hist[(key >> 16) & (HI_BINS - 1)], 1u);
        mx = max(mx, key);
        const double d = sqrt((double)d2);
        cnt += d <= tau ? 1 : 0;
        sum += d;
    }
    mx = wave_max(mx);
    cnt = wave_sum_u64(cnt);
    sum = wave_sum_f64(sum);
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { rmax[wid] = mx; rcnt[wid] = cnt; rsum[wid] = sum; }
    __syncthreads();
    for (int i = threadIdx.x; i < HI_BINS; i += TPB)
        if (hist[i]) atomicAdd(&ws->hist_hi[i], hist[i]);
    if (threadIdx.x == 0) {
        unsigned int m = rmax[0];
        unsigned long long c = rcnt[0];
        double s = rsum[0];
        for (int i = 1; i < TPB / 64; ++i) { m = max(m, rmax[i]); c += rcnt[i]; s += rsum[i]; }
        if (c) atomicAdd(&ws->within, c);
        atomicMax(&ws->maxkey, m);
        slab[blockIdx.x] = s;
    }
}

// one workgroup: the bin holding rank r in hist[nbins] (nbins / SEL_TPB bins per thread); returns the bin and r's rank in it
template <int NB>
MIVP_DEV void find_rank(const unsigned int* __restrict__ hist, long r0, long r1, unsigned long long* scan, int* out) {
    constexpr int PER = NB / SEL_TPB;
    const int t = threadIdx.x;
    unsigned long long own = 0;
    for (int i = 0; i < PER; ++i) own += hist[t * PER + i];
    scan[t] = own;
    __syncthreads();
    for (int o = 1; o < SEL_TPB; o <<= 1) {                   // inclusive Hillis-Steele scan
        const unsigned long long add = t >= o ? scan[t - o] : 0ull;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const unsigned long long before = scan[t] - own;
    const long rr[2] = {r0, r1};
    for (int q = 0; q < 2; ++q) {
        const unsigned long long r = (unsigned long long)rr[q];
        if (r >= before && r < before + own) {
            unsigned long long c = before;
            for (int i = 0; i < PER; ++i) {
                const unsigned int h = hist[t * PER + i];
                if (r < c + h) { out[2 * q] = t * PER + i; out[2 * q + 1] = (int)(r - c); break; }
                c += h;
            }
        }
    }
    __syncthreads();
}

// one workgroup: ranks from the device count, their high bins, the fixed-order slab sum, the record's first fields
// record int64 [8] = n, max key, count within tau, bits of the sum, key at rank lo, key at rank hi, lo, hi
__global__ __launch_bounds__(SEL_TPB) void k_stat_select_hi(const long long* __restrict__ count, double q,
                                                            StatWs* __restrict__ ws, const double* __restrict__ slab,
                                                            int nslab, long long* __restrict__ rec) {
    __shared__ unsigned long long scan[SEL_TPB];
    __shared__ double red[SEL_TPB];
    __shared__ int found[4];
    const int t = threadIdx.x;
    const long n = (long)count[0];
    if (t == 0) { found[0] = found[1] = found[2] = found[3] = -1; ws->min_hi = 0xffffffffu; }
    double s = 0.0;
    for (int i = t; i < nslab; i += SEL_TPB) s += slab[i];
    red[t] = s;
    __syncthreads();
    for (int o = SEL_TPB / 2; o >= 1; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    long lo = 0, hi = 0;
    if (n > 0) {
        const double vi = (double)(n - 1) * q;                 // numpy.percentile(method="linear")'s virtual index
        if (vi >= (double)(n - 1)) { lo = hi = n - 1; }
        else { lo = (long)floor(vi); hi = lo + 1; }
        find_rank<HI_BINS>(ws->hist_hi, lo, hi, scan, found);
    }
    if (t == 0) {
        for (int i = 0; i < 4; ++i) ws->state[i] = n > 0 ? found[i] : -1;
        rec[0] = n;
        rec[1] = ws->maxkey;
        rec[2] = (long long)ws->within;
        const double sum = red[0];
        rec[3] = *reinterpret_cast<const long long*>(&sum);
        rec[6] = lo;
        rec[7] = hi;
    }
}

// pass 2: low-half histogram inside the lower rank's bin (two 16-bit LDS counters per word), minimum low half inside the
// upper rank's bin when that is another bin
__global__ __launch_bounds__(TPB) void k_stat_lo(const uint8_t* __restrict__ smap, int cls, const float* __restrict__ dist,
                                                 long nvox, StatWs* __restrict__ ws) {
    __shared__ unsigned int hist[LO_BINS / 2];
    __shared__ unsigned int rmin[TPB / 64];
    const int bin_lo = ws->state[0], bin_hi = ws->state[2];
    if (bin_lo < 0) return;                                    // (uniform)
    for (int i = threadIdx.x; i < LO_BINS / 2; i += TPB) hist[i] = 0u;
    __syncthreads();
    unsigned int mn = 0xffffffffu;
    const long v0 = (long)blockIdx.x * SAMPLE_VOX;
    const long v1 = min(v0 + SAMPLE_VOX, nvox);
    for (long v = v0 + threadIdx.x; v < v1; v += TPB) {
        if (smap[v] != cls) continue;
        const unsigned int key = __float_as_uint(dist[v]);
        const int b = (int)(key >> 16);
        const unsigned int low = key & 0xffffu;
        if (b == bin_lo) atomicAdd(&hist[low >> 1], 1u << (16 * (low & 1)));
        else if (b == bin_hi) mn = min(mn, low);
    }
    mn = wave_min(mn);
    if ((threadIdx.x & 63) == 0) rmin[threadIdx.x >> 6] = mn;
    __syncthreads();
    for (int i = threadIdx.x; i < LO_BINS / 2; i += TPB) {
        const unsigned int h = hist[i];
        if (h & 0xffffu) atomicAdd(&ws->hist_lo[2 * i], h & 0xffffu);
        if (h >> 16) atomicAdd(&ws->hist_lo[2 * i + 1], h >> 16);
    }
    if (threadIdx.x == 0) {
        unsigned int m = rmin[0];
        for (int i = 1; i < TPB / 64; ++i) m = min(m, rmin[i]);
        if (m != 0xffffffffu) atomicMin(&ws->min_hi, m);
    }
}

// one workgroup: the keys at ranks lo and hi
__global__ __launch_bounds__(SEL_TPB) void k_stat_select_lo(StatWs* __restrict__ ws, long long* __restrict__ rec) {
    __shared__ unsigned long long scan[SEL_TPB];
    __shared__ int found[4];
    const int bin_lo = ws->state[0], r_lo = ws->state[1], bin_hi = ws->state[2], r_hi = ws->state[3];
    if (bin_lo < 0) return;                                    // (uniform)
    if (threadIdx.x == 0) found[0] = found[1] = found[2] = found[3] = -1;
    __syncthreads();
    find_rank<LO_BINS>(ws->hist_lo, r_lo, bin_hi == bin_lo ? r_hi : r_lo, scan, found);
    if (threadIdx.x == 0) {
        rec[4] = ((long long)bin_lo << 16) | found[0];
        rec[5] = bin_hi == bin_lo ? (((long long)bin_lo << 16) | found[2]) : (((long long)bin_hi << 16) | ws->min_hi);
    }
}

bool fill_dims(const int32_t* dims, int& H, int& W, int& D) {
    H = dims[0]; W = dims[1]; D = dims[2];
    return H >= 1 && W >= 1 && D >= 1 && (long)H * W * D < (1L << 31);
}

long n_sample_groups(long nvox) { return (nvox + SAMPLE_VOX - 1) / SAMPLE_VOX; }
}  // namespace

extern "C" int mivp_surface_map(const void* pred, const void* target, int32_t dtype, int32_t C, const int32_t* dims,
                                uint8_t* surf_pred, uint8_t* surf_target, void* counts, mivp_stream_t stream) {
    MIVP_REQUIRE(pred && surf_pred && dims && C >= 1 && C <= MAXC && dtype >= 0 && dtype <= 3);
    MIVP_REQUIRE((target == nullptr) == (surf_target == nullptr));
    int H, W, D;
    MIVP_REQUIRE(fill_dims(dims, H, W, D));
    const long nvox = (long)H * W * D;
    const unsigned grid = (unsigned)((nvox + TPB - 1) / TPB > 4096 ? 4096 : (nvox + TPB - 1) / TPB);
    auto* cnt = (unsigned long long*)counts;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case 0: hipLaunchKernelGGL(k_surface_map<uint8_t>, dim3(grid), dim3(TPB), 0, s, (const uint8_t*)pred,
                                   (const uint8_t*)target, (int)C, H, W, D, surf_pred, surf_target, cnt); break;
        case 1: hipLaunchKernelGGL(k_surface_map<int32_t>, dim3(grid), dim3(TPB), 0, s, (const int32_t*)pred,
                                   (const int32_t*)target, (int)C, H, W, D, surf_pred, surf_target, cnt); break;
        case 2: hipLaunchKernelGGL(k_surface_map<int64_t>, dim3(grid), dim3(TPB), 0, s, (const int64_t*)pred,
                                   (const int64_t*)target, (int)C, H, W, D, surf_pred, surf_target, cnt); break;
        default: hipLaunchKernelGGL(k_surface_map<float>, dim3(grid), dim3(TPB), 0, s, (const float*)pred,
                                    (const float*)target, (int)C, H, W, D, surf_pred, surf_target, cnt); break;
    }
    return mivp_check_launch("surface_map");
}

extern "C" size_t mivp_edt_ws(const int32_t* dims) {
    int H, W, D;
    if (!dims || !fill_dims(dims, H, W, D)) return 0;
    return (size_t)H * W * D * sizeof(int2);
}

extern "C" int mivp_edt_sq(const uint8_t* seeds, int32_t cls, const int32_t* dims, const float* spacing, float* out,
                           void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(seeds && dims && spacing && out && workspace && cls >= 0 && cls <= 255);
    int H, W, D;
    MIVP_REQUIRE(fill_dims(dims, H, W, D));
    MIVP_REQUIRE(H <= 65535 && W <= 65535);
    MIVP_REQUIRE(spacing[0] > 0.f && spacing[1] > 0.f && spacing[2] > 0.f);
    MIVP_REQUIRE(isfinite(spacing[0]) && isfinite(spacing[1]) && isfinite(spacing[2]));
    const bool intp = spacing[0] == 1.f && spacing[1] == 1.f && spacing[2] == 1.f;
    hipStream_t s = (hipStream_t)stream;
    int2* stack = (int2*)workspace;
    const long lines_d = (long)H * W;
    const unsigned grid_d = (unsigned)((lines_d + 3) / 4 > 8192 ? 8192 : (lines_d + 3) / 4);
    hipLaunchKernelGGL(k_edt_d, dim3(grid_d), dim3(TPB), 0, s, seeds, (int)cls, lines_d, D, spacing[2] * spacing[2],
                       (int)intp, out);
    const int rc = mivp_check_launch("edt_d");
    if (rc != MIVP_OK) return rc;
    // W pass: lines (h, d), elements w at stride D; H pass: lines (w, d), elements h at stride W * D
    const long lines_w = (long)H * D, lines_h = (long)W * D;
    const float aw = spacing[1] * spacing[1], ah = spacing[0] * spacing[0];
    if (intp) {
        hipLaunchKernelGGL(k_edt_line<true>, dim3((unsigned)((lines_w + TPB - 1) / TPB)), dim3(TPB), 0, s, out, lines_w, D,
                           (long)W * D, (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_edt_line<true>, dim3((unsigned)((lines_h + TPB - 1) / TPB)), dim3(TPB), 0, s, out, lines_h, D,
                           (long)D, (long)W * D, H, ah, stack);
    } else {
        hipLaunchKernelGGL(k_edt_line<false>, dim3((unsigned)((lines_w + TPB - 1) / TPB)), dim3(TPB), 0, s, out, lines_w, D,
                           (long)W * D, (long)D, W, aw, stack);
        hipLaunchKernelGGL(k_edt_line<false>, dim3((unsigned)((lines_h + TPB - 1) / TPB)), dim3(TPB), 0, s, out, lines_h, D,
                           (long)D, (long)W * D, H, ah, stack);
    }
    return mivp_check_launch("edt_line");
}

extern "C" size_t mivp_surface_stats_ws(const int32_t* dims) {
    int H, W, D;
    if (!dims || !fill_dims(dims, H, W, D)) return 0;
    const size_t head = (sizeof(StatWs) + 255) / 256 * 256;
    return head + (size_t)n_sample_groups((long)H * W * D) * sizeof(double);
}

extern "C" int mivp_surface_stats(const uint8_t* sampled, int32_t cls, const float* dist_sq, const int32_t* dims,
                                  const int64_t* count, double q, double tau, void* workspace, int64_t* record,
                                  mivp_stream_t stream) {
    MIVP_REQUIRE(sampled && dist_sq && dims && count && workspace && record && cls >= 0 && cls <= 255);
    MIVP_REQUIRE(q >= 0.0 && q <= 1.0 && tau >= 0.0);
    int H, W, D;
    MIVP_REQUIRE(fill_dims(dims, H, W, D));
    const long nvox = (long)H * W * D;
    const long groups = n_sample_groups(nvox);
    StatWs* ws = (StatWs*)workspace;
    double* slab = (double*)((char*)workspace + (sizeof(StatWs) + 255) / 256 * 256);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, sizeof(StatWs), s) != hipSuccess) return mivp_check_launch("surface_stats memset");
    hipLaunchKernelGGL(k_stat_hi, dim3((unsigned)groups), dim3(TPB), 0, s, sampled, (int)cls, dist_sq, nvox, tau, ws, slab);
    hipLaunchKernelGGL(k_stat_select_hi, dim3(1), dim3(SEL_TPB), 0, s, (const long long*)count, q, ws, slab, (int)groups,
                       (long long*)record);
    hipLaunchKernelGGL(k_stat_lo, dim3((unsigned)groups), dim3(TPB), 0, s, sampled, (int)cls, dist_sq, nvox, ws);
    hipLaunchKernelGGL(k_stat_select_lo, dim3(1), dim3(SEL_TPB), 0, s, ws, (long long*)record);
    return mivp_check_launch("surface_stats");
}
