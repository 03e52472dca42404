// Centreline extraction by 3-D thinning, and the centreline counts (joined ABI 18, mivp_amd/skeleton.py).
//
// The state is the uint8 output map itself: a voxel holds its class while it survives and 0 once it is deleted.  The border
// marks live in a byte array of their own (the workspace), so nothing that decides a deletion ever reads a mark of another
// voxel.  One outer iteration is
//   mark      one thread per voxel: flag = the voxel is in an object and one of its six face neighbours is not in that
//             object (outside the volume counts as not).  Taken on the state the iteration starts from.
//   sub-pass  eight launches, subfield s = (h&1)<<2 | (w&1)<<1 | (d&1) in the order 0..7, one thread per voxel of the
//             subfield.  A thread reads its flag first and only a flagged voxel pays for its 26 neighbours.  Two voxels of
//             one subfield differ by an even amount on every axis, so they are never 26-adjacent: no thread reads a byte
//             that another thread of the same launch writes.  The update in place is race-free, independent of the order
//             of the threads, and every single deletion is of a simple point of the state as it is.
// The neighbourhood is a 27-bit word, bit 9 (dh + 1) + 3 (dw + 1) + (dd + 1).  In that layout a step along an axis is a
// shift by 1, 3 or 9 with the wrapped columns masked off, so the two flood fills of the simple-point test need no
// adjacency table: a 26-dilation is the three axis dilations one after the other, a 6-dilation their union.
// Deletions are counted per iteration in one of two int32 words: a ballot and a popcount per wave, one integer atomic per
// wave that deleted something.  Every launch of iteration i > 1 first loads the word of iteration i - 1 (one uniform load)
// and returns when it is zero, so a fixed number of iterations can be issued blind and recorded in a graph.
// No float arithmetic anywhere; integer atomics only: the results are exact and bitwise reproducible.
#include "common.hpp"

namespace {
constexpr int TPB = 256;
constexpr int MAXC = 16;
constexpr size_t HEADER_BYTES = 256;      // the flags start here: 16-byte aligned whatever the header grows to
typedef unsigned long long u64;

struct Header {
    int cnt[2];                           // deletions of the iterations with this parity
    int iters;                            // the last iteration that ran
};

// ---------------------------------------------------------------------------------------------- the 27-bit neighbourhood
constexpr unsigned coord_mask(int axis, int value) {
    unsigned m = 0u;
    for (int i = 0; i < 27; ++i) {
        const int c[3] = {i / 9, (i / 3) % 3, i % 3};
        if (c[axis] == value) m |= 1u << i;
    }
    return m;
}
constexpr unsigned offsets_with(int lo, int hi) {          // the offsets with lo..hi non-zero components
    unsigned m = 0u;
    for (int i = 0; i < 27; ++i) {
        const int nz = (i / 9 != 1) + ((i / 3) % 3 != 1) + (i % 3 != 1);
        if (nz >= lo && nz <= hi) m |= 1u << i;
    }
    return m;
}
constexpr unsigned CENTRE = 1u << 13;
constexpr unsigned A0 = coord_mask(0, 0), A2 = coord_mask(0, 2);
constexpr unsigned B0 = coord_mask(1, 0), B2 = coord_mask(1, 2);
constexpr unsigned C0 = coord_mask(2, 0), C2 = coord_mask(2, 2);
constexpr unsigned N6 = offsets_with(1, 1), N18 = offsets_with(1, 2);
static_assert(A0 == 0x1FFu && C0 == 0x1249249u && B0 == 0x1C0E07u, "neighbourhood layout");
static_assert(N6 == ((1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22)), "face neighbours");

MIVP_DEV unsigned axis_step(unsigned x, int sh, unsigned lo, unsigned hi) { return ((x & ~hi) << sh) | ((x & ~lo) >> sh); }
MIVP_DEV unsigned dilate26(unsigned x) {
    x |= axis_step(x, 1, C0, C2);
    x |= axis_step(x, 3, B0, B2);
    x |= axis_step(x, 9, A0, A2);
    return x;
}
MIVP_DEV unsigned dilate6(unsigned x) { return x | axis_step(x, 1, C0, C2) | axis_step(x, 3, B0, B2) | axis_step(x, 9, A0, A2); }

// (26, 6) simple point: obj = the object neighbours (centre bit clear)
MIVP_DEV bool simple_point(unsigned obj) {
    if (obj == 0u) return false;
    unsigned comp = obj & (0u - obj);
    for (;;) {
        const unsigned n = dilate26(comp) & obj;
        if (n == comp) break;
        comp = n;
    }
    if (comp != obj) return false;
    const unsigned bg = ~obj & N18;                        // N18 has no centre bit
    const unsigned bg6 = bg & N6;
    if (bg6 == 0u) return false;
    comp = bg6 & (0u - bg6);
    for (;;) {
        const unsigned n = dilate6(comp) & bg;
        if (n == comp) break;
        comp = n;
    }
    return (bg6 & ~comp) == 0u;
}

// the neighbours of (h, w, d) that hold c, every read inside the volume
MIVP_DEV unsigned neighbours_of(const uint8_t* __restrict__ skel, int h, int w, int d, int H, int W, int D, unsigned c) {
    unsigned obj = 0u;
#pragma unroll
    for (int dh = -1; dh <= 1; ++dh) {
        const int hh = h + dh;
        if (hh < 0 || hh >= H) continue;
#pragma unroll
        for (int dw = -1; dw <= 1; ++dw) {
            const int ww = w + dw;
            if (ww < 0 || ww >= W) continue;
            const uint8_t* row = skel + ((long)hh * W + ww) * D + d;
            const int base = 9 * (dh + 1) + 3 * (dw + 1);
            if (d > 0 && row[-1] == c) obj |= 1u << base;
            if (row[0] == c) obj |= 1u << (base + 1);
            if (d + 1 < D && row[1] == c) obj |= 1u << (base + 2);
        }
    }
    return obj & ~CENTRE;
}

MIVP_DEV int label_class(const void* x, int dtype, long v, int C) {
    switch (dtype) {
        case 0: return class_of<uint8_t>(((const uint8_t*)x)[v], C);
        case 1: return class_of<int32_t>(((const int32_t*)x)[v], C);
        case 2: return class_of<int64_t>(((const int64_t*)x)[v], C);
        default: return class_of<float>(((const float*)x)[v], C);
    }
}

// ---------------------------------------------------------------------------------------------- thinning
__global__ __launch_bounds__(TPB) void k_skel_begin(const void* __restrict__ x, int dtype, unsigned V, int C, unsigned mask,
                                                    uint8_t* __restrict__ skel, Header* hdr) {
    const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (hdr && v == 0u) { hdr->cnt[0] = 0; hdr->cnt[1] = 0; hdr->iters = 0; }
    if (v >= V) return;
    const int c = label_class(x, dtype, (long)v, C);
    skel[v] = (c > 0 && ((mask >> c) & 1u)) ? (uint8_t)c : (uint8_t)0;
}

__global__ __launch_bounds__(TPB) void k_skel_mark(const uint8_t* __restrict__ skel, uint8_t* __restrict__ flags, int H, int W,
                                                   int D, unsigned V, Header* hdr, int iteration) {
    const int slot = iteration & 1;
    const bool skip = iteration > 1 && hdr->cnt[slot ^ 1] == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {             // the sub-passes of this iteration add to a clean word
        hdr->cnt[slot] = 0;
        if (!skip) hdr->iters = iteration;
    }
    if (skip) return;
    const unsigned v = blockIdx.x * (unsigned)TPB + threadIdx.x;
    if (v >= V) return;
    const uint8_t c = skel[v];
    uint8_t f = 0;
    if (c) {
        const unsigned row = v / (unsigned)D;
        const int d = (int)(v - row * (unsigned)D);
        const int h = (int)(row / (unsigned)W);
        const int w = (int)(row - (unsigned)h * (unsigned)W);
        const long sw = D, sh = (long)W * D;
        const uint8_t* p = skel + v;
        const bool inside = d > 0 && p[-1] == c && d + 1 < D && p[1] == c && w > 0 && p[-sw] == c && w + 1 < W &&
                            p[sw] == c && h > 0 && p[-sh] == c && h + 1 < H && p[sh] == c;
        f = inside ? 0 : 1;
    }
    flags[v] = f;
}

__global__ __launch_bounds__(TPB) void k_skel_subpass(uint8_t* __restrict__ skel, const uint8_t* __restrict__ flags, int H, int W,
                                                      int D, int ph, int pw, int pd, int nw, int nd, int n, int keep_endpoints,
                                                      Header* hdr, int iteration) {
    const int slot = iteration & 1;
    if (iteration > 1 && hdr->cnt[slot ^ 1] == 0) return;  // uniform: the iteration before deleted nothing
    const int t = (int)(blockIdx.x * (unsigned)TPB + threadIdx.x);
    bool del = false;
    if (t < n) {
        const int r = t / nd;
        const int d = 2 * (t - r * nd) + pd;
        const int kh = r / nw;
        const int w = 2 * (r - kh * nw) + pw;
        const int h = 2 * kh + ph;
        const long v = ((long)h * W + w) * D + d;
        if (flags[v]) {
            const unsigned c = skel[v];
            if (c) {
                const unsigned obj = neighbours_of(skel, h, w, d, H, W, D, c);
                del = simple_point(obj) && !(keep_endpoints && __popc(obj) <= 1);
                if (del) skel[v] = 0;
            }
        }
    }
    const u64 b = __ballot(del);
    if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&hdr->cnt[slot], __popcll(b));
}

__global__ void k_skel_end(const Header* hdr, int iteration, int* iterations, int* converged) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        iterations[0] = hdr->iters;
        converged[0] = hdr->cnt[iteration & 1] == 0 ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------- counts
constexpr int CL_WORDS = 4;               // |S_P|, |S_P and V_L|, |S_L|, |S_L and V_P|
constexpr int ST_WORDS = 18;              // voxels, degree 0, 1, 2, >= 3, then the 13 forward edge counts
constexpr unsigned GRID_CAP = 2048;

MIVP_DEV void cl_add(unsigned* tab, unsigned a, unsigned b, const void* pred, int dtp, const void* tgt, int dtt, long v, int C) {
    if (a && a < (unsigned)C) {
        atomicAdd(&tab[a * CL_WORDS + 0], 1u);
        if (label_class(tgt, dtt, v, C) == (int)a) atomicAdd(&tab[a * CL_WORDS + 1], 1u);
    }
    if (b && b < (unsigned)C) {
        atomicAdd(&tab[b * CL_WORDS + 2], 1u);
        if (label_class(pred, dtp, v, C) == (int)b) atomicAdd(&tab[b * CL_WORDS + 3], 1u);
    }
}

// items of four voxels: the two skeletons are mostly zero, so a dword of each decides whether the label maps are read
__global__ __launch_bounds__(TPB) void k_centerline_counts(const void* __restrict__ pred, int dtp, const void* __restrict__ tgt,
                                                           int dtt, const uint8_t* __restrict__ sp, const uint8_t* __restrict__ sl,
                                                           long V, int C, int vec, u64* __restrict__ counts) {
    __shared__ unsigned tab[MAXC * CL_WORDS];
    const int tid = (int)threadIdx.x;
    if (tid < MAXC * CL_WORDS) tab[tid] = 0u;
    __syncthreads();
    const long items = (V + 3) / 4;
    for (long i = (long)blockIdx.x * TPB + tid; i < items; i += (long)gridDim.x * TPB) {
        const long v0 = i * 4;
        if (vec) {
            const unsigned a = *reinterpret_cast<const unsigned*>(sp + v0);
            const unsigned b = *reinterpret_cast<const unsigned*>(sl + v0);
            if ((a | b) == 0u) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) cl_add(tab, (a >> (8 * j)) & 255u, (b >> (8 * j)) & 255u, pred, dtp, tgt, dtt, v0 + j, C);
        } else {
            const int nv = (int)min(4L, V - v0);
            for (int j = 0; j < nv; ++j) cl_add(tab, sp[v0 + j], sl[v0 + j], pred, dtp, tgt, dtt, v0 + j, C);
        }
    }
    __syncthreads();
    if (tid < C * CL_WORDS && tab[tid]) atomicAdd(counts + tid, (u64)tab[tid]);
}

__global__ __launch_bounds__(TPB) void k_skeleton_stats(const uint8_t* __restrict__ skel, int H, int W, int D, unsigned V, int C,
                                                        unsigned mask, u64* __restrict__ counts) {
    __shared__ unsigned tab[MAXC * ST_WORDS];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < MAXC * ST_WORDS; i += TPB) tab[i] = 0u;
    __syncthreads();
    for (unsigned v = blockIdx.x * (unsigned)TPB + tid; v < V; v += gridDim.x * (unsigned)TPB) {
        const unsigned c = skel[v];
        if (c == 0u || c >= (unsigned)C || !((mask >> c) & 1u)) continue;
        const unsigned row = v / (unsigned)D;
        const int d = (int)(v - row * (unsigned)D);
        const int h = (int)(row / (unsigned)W);
        const int w = (int)(row - (unsigned)h * (unsigned)W);
        const unsigned obj = neighbours_of(skel, h, w, d, H, W, D, c);
        unsigned* t = tab + c * ST_WORDS;
        atomicAdd(&t[0], 1u);
        atomicAdd(&t[1 + min((int)__popc(obj), 3)], 1u);
        unsigned fwd = obj >> 14;                          // bits above the centre: the 13 forward offsets in order
        while (fwd) {
            const int k = __ffs((int)fwd) - 1;
            atomicAdd(&t[5 + k], 1u);
            fwd &= fwd - 1u;
        }
    }
    __syncthreads();
    for (int i = tid; i < C * ST_WORDS; i += TPB)
        if (tab[i]) atomicAdd(counts + i, (u64)tab[i]);
}

bool dims_ok(const int32_t* dims) {
    return dims && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long)dims[0] * dims[1] * dims[2] < (1L << 31);
}
int dtype_size(int dtype) { return dtype == 0 ? 1 : dtype == 2 ? 8 : 4; }
unsigned blocks_for(long n) { return (unsigned)((n + TPB - 1) / TPB); }
}  // namespace

extern "C" size_t mivp_skeleton_ws(const int32_t* dims) {
    if (!dims_ok(dims)) return 0;
    return HEADER_BYTES + (size_t)dims[0] * dims[1] * dims[2];
}

extern "C" int mivp_skeleton_begin(const void* labels, int32_t dtype, const int32_t* dims, int32_t C, uint32_t class_mask,
                                   uint8_t* skeleton, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(labels && skeleton && dims_ok(dims) && dtype >= 0 && dtype <= 3);
    MIVP_REQUIRE(C >= 1 && C <= MAXC && class_mask != 0u && (class_mask & 1u) == 0u && (class_mask >> C) == 0u);
    MIVP_REQUIRE(((uintptr_t)labels & (uintptr_t)(dtype_size(dtype) - 1)) == 0 && ((uintptr_t)workspace & 3u) == 0);
    const long V = (long)dims[0] * dims[1] * dims[2];
    hipLaunchKernelGGL(k_skel_begin, dim3(blocks_for(V)), dim3(TPB), 0, (hipStream_t)stream, labels, (int)dtype, (unsigned)V,
                       (int)C, (unsigned)class_mask, skeleton, (Header*)workspace);
    return mivp_check_launch("skeleton_begin");
}

extern "C" int mivp_skeleton_iter(uint8_t* skeleton, const int32_t* dims, int32_t keep_endpoints, int32_t iteration,
                                  void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(skeleton && workspace && dims_ok(dims) && iteration >= 1 && (keep_endpoints == 0 || keep_endpoints == 1));
    MIVP_REQUIRE(((uintptr_t)workspace & 3u) == 0);
    const int H = dims[0], W = dims[1], D = dims[2];
    const long V = (long)H * W * D;
    Header* hdr = (Header*)workspace;
    uint8_t* flags = (uint8_t*)workspace + HEADER_BYTES;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_skel_mark, dim3(blocks_for(V)), dim3(TPB), 0, st, (const uint8_t*)skeleton, flags, H, W, D,
                       (unsigned)V, hdr, (int)iteration);
    for (int s = 0; s < 8; ++s) {
        const int ph = (s >> 2) & 1, pw = (s >> 1) & 1, pd = s & 1;
        const int nh = (H - ph + 1) / 2, nw = (W - pw + 1) / 2, nd = (D - pd + 1) / 2;
        const long n = (long)nh * nw * nd;
        if (n == 0) continue;                              // an axis of extent 1 has no odd plane
        hipLaunchKernelGGL(k_skel_subpass, dim3(blocks_for(n)), dim3(TPB), 0, st, skeleton, (const uint8_t*)flags, H, W, D, ph,
                           pw, pd, nw, nd, (int)n, (int)keep_endpoints, hdr, (int)iteration);
    }
    return mivp_check_launch("skeleton_iter");
}

extern "C" int mivp_skeleton_end(const void* workspace, int32_t iteration, int32_t* iterations, int32_t* converged,
                                 mivp_stream_t stream) {
    MIVP_REQUIRE(workspace && iterations && converged && iteration >= 1 && ((uintptr_t)workspace & 3u) == 0);
    hipLaunchKernelGGL(k_skel_end, dim3(1), dim3(64), 0, (hipStream_t)stream, (const Header*)workspace, (int)iteration,
                       (int*)iterations, (int*)converged);
    return mivp_check_launch("skeleton_end");
}

extern "C" int mivp_centerline_counts(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype,
                                      const uint8_t* skeleton_pred, const uint8_t* skeleton_target, const int32_t* dims,
                                      int32_t C, int64_t* counts, mivp_stream_t stream) {
    MIVP_REQUIRE(pred && target && skeleton_pred && skeleton_target && counts && dims_ok(dims));
    MIVP_REQUIRE(pred_dtype >= 0 && pred_dtype <= 3 && target_dtype >= 0 && target_dtype <= 3 && C >= 1 && C <= MAXC);
    MIVP_REQUIRE(((uintptr_t)pred & (uintptr_t)(dtype_size(pred_dtype) - 1)) == 0);
    MIVP_REQUIRE(((uintptr_t)target & (uintptr_t)(dtype_size(target_dtype) - 1)) == 0 && ((uintptr_t)counts & 7u) == 0);
    const long V = (long)dims[0] * dims[1] * dims[2];
    const int vec = (V % 4 == 0 && (((uintptr_t)skeleton_pred | (uintptr_t)skeleton_target) & 3u) == 0) ? 1 : 0;
    const unsigned want = blocks_for((V + 3) / 4);
    hipLaunchKernelGGL(k_centerline_counts, dim3(want > GRID_CAP ? GRID_CAP : want), dim3(TPB), 0, (hipStream_t)stream, pred,
                       (int)pred_dtype, target, (int)target_dtype, skeleton_pred, skeleton_target, V, (int)C, vec, (u64*)counts);
    return mivp_check_launch("centerline_counts");
}

extern "C" int mivp_skeleton_stats(const uint8_t* skeleton, const int32_t* dims, int32_t C, uint32_t class_mask,
                                   int64_t* counts, mivp_stream_t stream) {
    MIVP_REQUIRE(skeleton && counts && dims_ok(dims) && C >= 1 && C <= MAXC && ((uintptr_t)counts & 7u) == 0);
    MIVP_REQUIRE(class_mask != 0u && (class_mask & 1u) == 0u && (class_mask >> C) == 0u);
    const long V = (long)dims[0] * dims[1] * dims[2];
    const unsigned want = blocks_for(V);
    hipLaunchKernelGGL(k_skeleton_stats, dim3(want > GRID_CAP ? GRID_CAP : want), dim3(TPB), 0, (hipStream_t)stream, skeleton,
                       (int)dims[0], (int)dims[1], (int)dims[2], (unsigned)V, (int)C, (unsigned)class_mask, (u64*)counts);
    return mivp_check_launch("skeleton_stats");
}
