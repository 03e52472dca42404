// Connected-component labelling and label-map post-processing (ABI 16, mivp_amd/components.py).
//
// Volumes are [H][W][D] row-major (D contiguous), fewer than 2^31 voxels.  Two adjacent voxels (6-, 18- or
// 26-neighbourhood) are joined when both take part and hold the same value.  In labelling mode every nonzero voxel takes
// part; in post-processing mode the voxels whose class (class_of) is in a class mask.
//
// Union-find over int32 parent[N] with global linear indices.  Every link points to a smaller index (parent[v] <= v) and
// links only decrease, so a root is always the minimum index of its set, whatever the scheduling order:
//   local     one workgroup per 8x8x16 tile: values into LDS, the in-tile backward neighbours united with LDS atomicMin
//             links, parent[v] = global index of the tile-local root (tile-local order is monotone in global order).
//   boundary  one workgroup per tile: each voxel on a tile face unites with its backward neighbours in other tiles by
//             lock-free atomicMin on parent (the Playne-Hawick union).  Finds read words other workgroups write in the
//             same launch with relaxed agent-scope atomic loads; a stale word is an earlier link of the same set, so a
//             find still ends at a member of the set and the atomicMin's returned old value repairs a stale root.
//   compress  after the kernel boundary, parent[v] = root(v): the component's minimum index.
// Labelling: per 4096-voxel chunk count the roots, one workgroup scans the chunk counts, each root's label is
// 1 + its rank among the roots (the order of first voxels, scipy's numbering), then every voxel takes its root's label.
// The output buffer is the parent array itself.
// Post-processing: component sizes by integer atomics at the root, aggregated per lane run, per wave (one add per
// distinct root in a wave) and per workgroup (LDS slots); per class the best root by a 64-bit atomicMax of
// (size << 32 | ~root), reduced per wave and per workgroup first; one filter pass writes the output (optionally the per-class Dice / IoU counts against a target).
#include "common.hpp"
#include <limits.h>

namespace {
constexpr int MAXC = 16;
constexpr int TPB = 256;
constexpr int TH = 8, TW = 8, TD = 16, TILE = TH * TW * TD;   // tile of the local and boundary passes
constexpr int PER_TILE = TILE / TPB;
constexpr int CHUNK = 4096;                                     // voxels per workgroup of the size / numbering passes
constexpr int PER_CHUNK = CHUNK / TPB;
constexpr int SCAN_TPB = 1024;
constexpr unsigned GRID_CAP = 4096;

// backward neighbours in raster order (dh, dw, dd): the first 3 are the 6-neighbourhood, the first 9 the 18-, all 13
// the 26-neighbourhood
__constant__ int8_t OFF[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1},  {-1, -1, 0}, {-1, 1, 0},
                                  {-1, 0, -1}, {-1, 0, 1},  {0, -1, -1}, {0, -1, 1},  {-1, -1, -1},
                                  {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

struct Geo {
    int H, W, D;       // volume
    int nW, nD;        // tiles along W and D
};

// mask == 0: labelling (every nonzero voxel); otherwise the voxels whose class is a set bit of mask (bit 0 never set)
struct Sel {
    int C;
    unsigned mask;
};

template <typename T> MIVP_DEV bool takes_part(T v, Sel s) {
    if (s.mask == 0u) return v != (T)0;
    const int c = class_of<T>(v, s.C);
    return c > 0 && ((s.mask >> c) & 1u);
}

template <int SCOPE> MIVP_DEV int ld_link(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// root of x, splitting the path on the way (every visited node is linked to its grandparent by atomicMin: the
// grandparent is in the same set and smaller, and a root is never touched, so no union is lost)
template <int SCOPE> MIVP_DEV int find_root(int* p, int x) {
    int px = ld_link<SCOPE>(p + x);
    while (px != x) {
        const int ppx = ld_link<SCOPE>(p + px);
        if (ppx != px) atomicMin(p + x, ppx);
        x = px;
        px = ppx;
    }
    return x;
}

// lock-free union: link the larger root below the smaller one; when the atomicMin finds that the word is no longer a
// root (another union got there first, or the find read a stale word), go on with the value it returned.  a + b
// strictly decreases on every retry, so the loop ends.
template <int SCOPE> MIVP_DEV void unite(int* p, int a, int b) {
    for (;;) {
        a = find_root<SCOPE>(p, a);
        b = find_root<SCOPE>(p, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(p + b, a);
        if (old == b) return;
        b = old;
    }
}

MIVP_DEV void tile_origin(const Geo& g, int& h0, int& w0, int& d0) {
    const int t = (int)blockIdx.x;
    d0 = (t % g.nD) * TD;
    w0 = ((t / g.nD) % g.nW) * TW;
    h0 = (t / (g.nD * g.nW)) * TH;
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_cc_local(const T* __restrict__ x, Geo g, Sel s, int nk, int* __restrict__ parent) {
    __shared__ T sv[TILE];
    __shared__ int lp[TILE];
    int h0, w0, d0;
    tile_origin(g, h0, w0, d0);
    bool part[PER_TILE];
#pragma unroll
    for (int j = 0; j < PER_TILE; ++j) {
        const int i = threadIdx.x + j * TPB;
        const int h = h0 + i / (TW * TD), w = w0 + (i / TD) % TW, d = d0 + i % TD;
        const bool in = h < g.H && w < g.W && d < g.D;
        const T v = in ? x[((long)h * g.W + w) * g.D + d] : (T)0;
        part[j] = in && takes_part<T>(v, s);
        sv[i] = v;
        lp[i] = part[j] ? i : -1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER_TILE; ++j) {
        if (!part[j]) continue;
        const int i = threadIdx.x + j * TPB;
        const int lh = i / (TW * TD), lw = (i / TD) % TW, ld = i % TD;
        for (int k = 0; k < nk; ++k) {
            const int nh = lh + OFF[k][0], nw = lw + OFF[k][1], nd = ld + OFF[k][2];
            if (nh < 0 || nw < 0 || nw >= TW || nd < 0 || nd >= TD) continue;
            const int n = (nh * TW + nw) * TD + nd;
            // same value => the neighbour takes part too (participation depends on the value only; outside the volume
            // the LDS holds 0, which never takes part)
            if (sv[n] == sv[i]) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, i, n);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER_TILE; ++j) {
        const int i = threadIdx.x + j * TPB;
        const int h = h0 + i / (TW * TD), w = w0 + (i / TD) % TW, d = d0 + i % TD;
        if (h >= g.H || w >= g.W || d >= g.D) continue;
        int root = -1;
        if (part[j]) {
            const int r = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, i);
            root = (int)(((long)(h0 + r / (TW * TD)) * g.W + (w0 + (r / TD) % TW)) * g.D + (d0 + r % TD));
        }
        parent[((long)h * g.W + w) * g.D + d] = root;
    }
}

template <typename T>
__global__ __launch_bounds__(TPB) void k_cc_boundary(const T* __restrict__ x, Geo g, Sel s, int nk, int* parent) {
    int h0, w0, d0;
    tile_origin(g, h0, w0, d0);
    for (int i = threadIdx.x; i < TILE; i += TPB) {
        const int lh = i / (TW * TD), lw = (i / TD) % TW, ld = i % TD;
        // a backward neighbour in another tile needs lh == 0, lw at either face (dw = +1 occurs with dh = -1) or ld at
        // either face
        if (!(lh == 0 || lw == 0 || lw == TW - 1 || ld == 0 || ld == TD - 1)) continue;
        const int h = h0 + lh, w = w0 + lw, d = d0 + ld;
        if (h >= g.H || w >= g.W || d >= g.D) continue;
        const long v = ((long)h * g.W + w) * g.D + d;
        const T a = x[v];
        if (!takes_part<T>(a, s)) continue;
        for (int k = 0; k < nk; ++k) {
            const int nlh = lh + OFF[k][0], nlw = lw + OFF[k][1], nld = ld + OFF[k][2];
            if (nlh >= 0 && nlw >= 0 && nlw < TW && nld >= 0 && nld < TD) continue;      // same tile: done by k_cc_local
            const int nh = h + OFF[k][0], nw = w + OFF[k][1], nd = d + OFF[k][2];
            if (nh < 0 || nw < 0 || nw >= g.W || nd < 0 || nd >= g.D) continue;
            const long n = ((long)nh * g.W + nw) * g.D + nd;
            if (x[n] == a) unite<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)v, (int)n);
        }
    }
}

// after the boundary launch the forest is final: every voxel links straight to its root.  Concurrent stores only
// replace a link by the root of the same set, so a read of either value leads to the root.  Zeroes size[] and best[]
// for the post-processing passes on the way.
__global__ __launch_bounds__(TPB) void k_cc_compress(int* parent, long n, int* __restrict__ size,
                                                     unsigned long long* __restrict__ best) {
    if (best && blockIdx.x == 0 && threadIdx.x < MAXC) best[threadIdx.x] = 0ull;
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < n; v += (long)gridDim.x * TPB) {
        const int p = parent[v];
        if (p >= 0 && p != (int)v) {
            int r = p, q;
            while ((q = ld_link<__HIP_MEMORY_SCOPE_WORKGROUP>(parent + r)) != r) r = q;
            if (r != p) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (size) size[v] = 0;
    }
}

MIVP_DEV int lane_id() { return (int)__lane_id(); }

constexpr int SLOTS = 8;   // per-workgroup LDS counters of the first distinct roots the size pass meets

// one add of s to size[r]: into the workgroup's LDS slot of r (claimed on first use) while a slot is free, else global
MIVP_DEV void add_size(int r, int s, int* size, int* skey, int* scnt) {
    for (int k = 0; k < SLOTS; ++k) {
        int key = __hip_atomic_load(skey + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (key == -1) {
            const int old = atomicCAS(skey + k, -1, r);
            key = old == -1 ? r : old;
        }
        if (key == r) { atomicAdd(scnt + k, s); return; }
    }
    atomicAdd(size + r, s);
}

// wave-uniform call: every pending lane adds cnt to root's size, one add per distinct root among the pending lanes
MIVP_DEV void wave_add(bool pending, int root, int cnt, int* size, int* skey, int* scnt) {
    unsigned long long m = __ballot(pending);
    while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int r0 = __shfl(root, leader);
        const bool match = pending && root == r0;
        int sum = match ? cnt : 0;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane_id() == leader) add_size(r0, sum, size, skey, scnt);
        pending = pending && !match;
        m &= ~__ballot(match);
    }
}

// component sizes: each lane walks 16 voxels of a 4096-voxel chunk (coalesced across lanes) and keeps a run (root,
// count) across background voxels that it flushes when another root comes; a flush adds once per distinct root of the
// wave, into LDS slots for the workgroup's first SLOTS roots (one global atomic per slot at the end).  A component
// spanning the volume thus gets about one global add per workgroup, not one per wave and run.
__global__ __launch_bounds__(TPB) void k_cc_size(const int* __restrict__ parent, long n, int* size) {
    __shared__ int skey[SLOTS], scnt[SLOTS];
    if (threadIdx.x < SLOTS) { skey[threadIdx.x] = -1; scnt[threadIdx.x] = 0; }
    __syncthreads();
    const long base = (long)blockIdx.x * CHUNK + threadIdx.x;
    int cur = -1, cnt = 0;
    for (int it = 0; it < PER_CHUNK; ++it) {
        const long v = base + (long)it * TPB;
        const int r = v < n ? parent[v] : -1;
        wave_add(r >= 0 && cur >= 0 && r != cur, cur, cnt, size, skey, scnt);
        if (r >= 0) {
            if (r != cur) { cur = r; cnt = 0; }
            ++cnt;
        }
    }
    wave_add(cur >= 0, cur, cnt, size, skey, scnt);
    __syncthreads();
    if (threadIdx.x < SLOTS && skey[threadIdx.x] >= 0) atomicAdd(size + skey[threadIdx.x], scnt[threadIdx.x]);
}

MIVP_DEV unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
MIVP_DEV unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}

// per class the best component: the maximum of (size << 32 | 0xFFFFFFFF - root) over the roots of the class, i.e. the
// largest component, ties to the smallest root (the first in raster order).  Wave max per class, then an LDS max per
// workgroup, then one global atomicMax per class and workgroup.
template <typename T>
__global__ __launch_bounds__(TPB) void k_cc_best(const T* __restrict__ x, const int* __restrict__ parent,
                                                 const int* __restrict__ size, long n, int C,
                                                 unsigned long long* __restrict__ best) {
    __shared__ unsigned long long sb[MAXC];
    if (threadIdx.x < MAXC) sb[threadIdx.x] = 0ull;
    __syncthreads();
    const long stride = (long)gridDim.x * TPB;
    const long iters = (n + stride - 1) / stride;       // uniform trip count: the wave reduction needs every lane
    for (long it = 0; it < iters; ++it) {
        const long v = it * stride + (long)blockIdx.x * TPB + threadIdx.x;
        bool pending = v < n && parent[v] == (int)v;
        const int c = pending ? class_of<T>(x[v], C) : -1;
        const unsigned long long key =
            pending ? ((unsigned long long)(unsigned)size[v] << 32) | (0xFFFFFFFFu - (unsigned)v) : 0ull;
        unsigned long long m = __ballot(pending);
        while (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            const int c0 = __shfl(c, leader);
            const bool match = pending && c == c0;
            unsigned long long k = match ? key : 0ull;
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long t = shfl_xor_u64(k, o);
                k = t > k ? t : k;
            }
            if (lane_id() == leader) atomicMax(&sb[c0], k);
            pending = pending && !match;
            m &= ~__ballot(match);
        }
    }
    __syncthreads();
    if (threadIdx.x < C && sb[threadIdx.x]) atomicMax(&best[threadIdx.x], sb[threadIdx.x]);
}

// out = x with the removed components zeroed; with a target, counts [C][3] += (inter, pred, target) per class as
// mivp_stitch_finalize does (LDS, then one integer atomic per class and workgroup)
template <typename T>
__global__ __launch_bounds__(TPB) void k_cc_filter(const T* x, const int* __restrict__ parent, const int* __restrict__ size,
                                                   const unsigned long long* __restrict__ best, long n, int C,
                                                   long long min_size, int largest, T* out,
                                                   const float* __restrict__ target,
                                                   unsigned long long* __restrict__ counts) {
    __shared__ unsigned int sm[MAXC * 3];
    for (int i = threadIdx.x; i < MAXC * 3; i += TPB) sm[i] = 0u;
    __syncthreads();
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < n; v += (long)gridDim.x * TPB) {
        const T a = x[v];
        const int p = parent[v];
        bool keep = true;
        if (p >= 0) {
            keep = (long long)size[p] >= min_size;
            if (keep && largest)
                keep = (unsigned)(best[class_of<T>(a, C)] & 0xFFFFFFFFull) == 0xFFFFFFFFu - (unsigned)p;
        }
        const T o = keep ? a : (T)0;
        out[v] = o;
        if (target) {
            const int pc = class_of<T>(o, C);
            const float tv = target[v];
            if (pc >= 0) atomicAdd(&sm[pc * 3 + 1], 1u);
            for (int c = 0; c < C; ++c)
                if (tv == (float)c) { atomicAdd(&sm[c * 3 + 2], 1u); if (pc == c) atomicAdd(&sm[c * 3 + 0], 1u); }
        }
    }
    if (!target) return;                                       // (uniform: the whole grid returns together)
    __syncthreads();
    for (int i = threadIdx.x; i < C * 3; i += TPB)
        if (sm[i]) atomicAdd(&counts[i], (unsigned long long)sm[i]);
}

// ---- numbering (labelling mode): lab is the compressed parent array, rewritten in place into labels
__global__ __launch_bounds__(TPB) void k_cc_count(const int* __restrict__ lab, long n, int* __restrict__ cnt) {
    __shared__ int ws[TPB / 64];
    const long base = (long)blockIdx.x * CHUNK + threadIdx.x;
    int c = 0;
    for (int it = 0; it < PER_CHUNK; ++it) {
        const long v = base + (long)it * TPB;
        c += (v < n && lab[v] == (int)v) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane_id() == 0) ws[threadIdx.x / 64] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < TPB / 64; ++w) t += ws[w];
        cnt[blockIdx.x] = t;
    }
}

// one workgroup: exclusive scan of the chunk counts in place, total into *n_out
__global__ __launch_bounds__(SCAN_TPB) void k_cc_scan(int* cnt, int nb, int* __restrict__ n_out) {
    __shared__ int part[SCAN_TPB];
    const int per = (nb + SCAN_TPB - 1) / SCAN_TPB;
    const int beg = min(nb, (int)threadIdx.x * per), end = min(nb, beg + per);
    int s = 0;
    for (int i = beg; i < end; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_TPB; o <<= 1) {               // inclusive Hillis-Steele scan of the per-thread sums
        const int t = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = beg; i < end; ++i) {
        const int c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    if (threadIdx.x == SCAN_TPB - 1) *n_out = part[SCAN_TPB - 1];
}

// roots get -(1 + rank) (rank among all roots in raster order), background INT_MIN; links stay (>= 0)
__global__ __launch_bounds__(TPB) void k_cc_rank(int* lab, long n, const int* __restrict__ off) {
    __shared__ int ws[TPB / 64];
    const int wave = threadIdx.x / 64, lane = lane_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    const long base = (long)blockIdx.x * CHUNK + threadIdx.x;
    int run = off[blockIdx.x];
    for (int it = 0; it < PER_CHUNK; ++it) {
        const long v = base + (long)it * TPB;
        const int p = v < n ? lab[v] : 0;
        const bool root = v < n && p == (int)v;
        const unsigned long long b = __ballot(root);
        if (lane == 0) ws[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < TPB / 64; ++w) {
            before += w < wave ? ws[w] : 0;
            total += ws[w];
        }
        if (root) lab[v] = -(1 + run + before + __popcll(b & below));
        else if (v < n && p < 0) lab[v] = INT_MIN;
        run += total;
        __syncthreads();
    }
}

// every voxel takes its root's label; a root may be flipped to positive by its own thread meanwhile, hence abs
__global__ __launch_bounds__(TPB) void k_cc_gather(int* lab, long n) {
    for (long v = (long)blockIdx.x * TPB + threadIdx.x; v < n; v += (long)gridDim.x * TPB) {
        const int a = lab[v];
        if (a == INT_MIN) lab[v] = 0;
        else if (a < 0) lab[v] = -a;
        else lab[v] = abs(ld_link<__HIP_MEMORY_SCOPE_WORKGROUP>(lab + a));
    }
}

bool fill_geo(const int32_t* dims, Geo& g) {
    g.H = dims[0]; g.W = dims[1]; g.D = dims[2];
    if (g.H < 1 || g.W < 1 || g.D < 1 || (long)g.H * g.W * g.D >= (1L << 31)) return false;
    g.nW = (g.W + TW - 1) / TW;
    g.nD = (g.D + TD - 1) / TD;
    return true;
}

long n_tiles(const Geo& g) { return (long)((g.H + TH - 1) / TH) * g.nW * g.nD; }
long n_chunks(long nvox) { return (nvox + CHUNK - 1) / CHUNK; }
unsigned stride_grid(long nvox) { return (unsigned)((nvox + TPB - 1) / TPB > GRID_CAP ? GRID_CAP : (nvox + TPB - 1) / TPB); }
int n_neighbours(int connectivity) { return connectivity == 6 ? 3 : connectivity == 18 ? 9 : connectivity == 26 ? 13 : 0; }

// local + boundary + compress: parent[v] = the minimum index of v's component, -1 where v takes no part
template <typename T>
void forest(const void* x, const Geo& g, Sel s, int nk, int* parent, int* size, unsigned long long* best, hipStream_t st) {
    const long nvox = (long)g.H * g.W * g.D;
    const unsigned tiles = (unsigned)n_tiles(g);
    hipLaunchKernelGGL(k_cc_local<T>, dim3(tiles), dim3(TPB), 0, st, (const T*)x, g, s, nk, parent);
    hipLaunchKernelGGL(k_cc_boundary<T>, dim3(tiles), dim3(TPB), 0, st, (const T*)x, g, s, nk, parent);
    hipLaunchKernelGGL(k_cc_compress, dim3(stride_grid(nvox)), dim3(TPB), 0, st, parent, nvox, size, best);
}

template <typename T>
void postprocess(const void* x, const Geo& g, Sel s, int nk, long long min_size, int largest, void* out,
                 const float* target, unsigned long long* counts, unsigned long long* best, int* parent, int* size,
                 hipStream_t st) {
    const long nvox = (long)g.H * g.W * g.D;
    forest<T>(x, g, s, nk, parent, size, best, st);
    hipLaunchKernelGGL(k_cc_size, dim3((unsigned)n_chunks(nvox)), dim3(TPB), 0, st, (const int*)parent, nvox, size);
    if (largest)
        hipLaunchKernelGGL(k_cc_best<T>, dim3(stride_grid(nvox)), dim3(TPB), 0, st, (const T*)x, (const int*)parent,
                           (const int*)size, nvox, s.C, best);
    hipLaunchKernelGGL(k_cc_filter<T>, dim3(stride_grid(nvox)), dim3(TPB), 0, st, (const T*)x, (const int*)parent,
                       (const int*)size, (const unsigned long long*)best, nvox, s.C, min_size, largest, (T*)out, target,
                       counts);
}

constexpr size_t WS_HEAD = 256;                 // best[MAXC] (uint64), padded
}  // namespace

extern "C" size_t mivp_label_ws(const int32_t* dims) {
    Geo g;
    if (!dims || !fill_geo(dims, g)) return 0;
    return (size_t)n_chunks((long)g.H * g.W * g.D) * sizeof(int);
}

extern "C" int mivp_label_components(const void* x, int32_t dtype, const int32_t* dims, int32_t connectivity,
                                     int32_t* labels, int32_t* n_out, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(x && dims && labels && n_out && workspace && dtype >= 0 && dtype <= 3);
    const int nk = n_neighbours(connectivity);
    MIVP_REQUIRE(nk > 0);
    Geo g;
    MIVP_REQUIRE(fill_geo(dims, g));
    const long nvox = (long)g.H * g.W * g.D;
    const Sel s{0, 0u};
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case 0: forest<uint8_t>(x, g, s, nk, labels, nullptr, nullptr, st); break;
        case 1: forest<int32_t>(x, g, s, nk, labels, nullptr, nullptr, st); break;
        case 2: forest<int64_t>(x, g, s, nk, labels, nullptr, nullptr, st); break;
        default: forest<float>(x, g, s, nk, labels, nullptr, nullptr, st); break;
    }
    const int nb = (int)n_chunks(nvox);
    int* cnt = (int*)workspace;
    hipLaunchKernelGGL(k_cc_count, dim3(nb), dim3(TPB), 0, st, (const int*)labels, nvox, cnt);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(SCAN_TPB), 0, st, cnt, nb, n_out);
    hipLaunchKernelGGL(k_cc_rank, dim3(nb), dim3(TPB), 0, st, labels, nvox, (const int*)cnt);
    hipLaunchKernelGGL(k_cc_gather, dim3(stride_grid(nvox)), dim3(TPB), 0, st, labels, nvox);
    return mivp_check_launch("label_components");
}

extern "C" size_t mivp_postprocess_ws(const int32_t* dims) {
    Geo g;
    if (!dims || !fill_geo(dims, g)) return 0;
    return WS_HEAD + (size_t)g.H * g.W * g.D * 2 * sizeof(int);
}

extern "C" int mivp_postprocess_labels(const void* x, int32_t dtype, const int32_t* dims, int32_t C, uint32_t class_mask,
                                       int64_t min_size, int32_t largest, int32_t connectivity, void* out,
                                       const float* target, void* counts, void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(x && dims && out && workspace && dtype >= 0 && dtype <= 3 && C >= 1 && C <= MAXC);
    MIVP_REQUIRE((target == nullptr) == (counts == nullptr));
    MIVP_REQUIRE(class_mask != 0u && (class_mask & 1u) == 0u && (class_mask >> C) == 0u);
    MIVP_REQUIRE(min_size >= 0 && (largest == 0 || largest == 1) && (largest || min_size > 0));
    const int nk = n_neighbours(connectivity);
    MIVP_REQUIRE(nk > 0);
    Geo g;
    MIVP_REQUIRE(fill_geo(dims, g));
    const long nvox = (long)g.H * g.W * g.D;
    auto* best = (unsigned long long*)workspace;
    int* parent = (int*)((char*)workspace + WS_HEAD);
    int* size = parent + nvox;
    const Sel s{(int)C, (unsigned)class_mask};
    auto* cnt = (unsigned long long*)counts;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case 0: postprocess<uint8_t>(x, g, s, nk, min_size, largest, out, target, cnt, best, parent, size, st); break;
        case 1: postprocess<int32_t>(x, g, s, nk, min_size, largest, out, target, cnt, best, parent, size, st); break;
        case 2: postprocess<int64_t>(x, g, s, nk, min_size, largest, out, target, cnt, best, parent, size, st); break;
        default: postprocess<float>(x, g, s, nk, min_size, largest, out, target, cnt, best, parent, size, st); break;
    }
    return mivp_check_launch("postprocess_labels");
}
