// Per-lesion region statistics and lesion-wise detection metrics (joined ABI 18, mivp_amd/regions.py).
//
// Volumes are [H][W][D] row-major (D contiguous), fewer than 2^31 voxels.
//   select    the class map -> uint8 class per voxel, 0 where the class is not a set bit of the class mask; the existing
//             labelling entry (mivp_label_components) numbers the components of that map 1..n as scipy does and leaves n
//             on the device.
//   reduce    one pass over the dense labels: every lane walks 16 consecutive voxels along D and keeps one run (label,
//             size, first voxel, bounding box, coordinate sums, image min / max / sum / sum of squares) across
//             background voxels; a run ends when another label comes and is then added to the workgroup's LDS table
//             (REG_SLOTS regions, a slot is claimed by an LDS atomicCAS on first use; a workgroup that meets more regions
//             adds the surplus runs to global memory directly).  At the end one lane per used slot flushes it: one set of
//             global atomics per (workgroup, region).  Integer add / min / max everywhere; float images add their sums
//             as float64 with the hardware global_atomic_add_f64, the one part that depends on arrival order.
//             Minima and maxima of image values travel as order-preserving uint32 keys and are decoded by `finish`.
//   overlap   one pass over two dense label maps with the same run and LDS pre-aggregation, keyed by (p << 32) | t, into
//             an open-addressing hash table in global memory (atomicCAS on the key, int64 atomic add on the count).  The
//             probe sequence is bounded by the table size and every insert first reads the overflow flag, so a full table
//             sets the flag and ends; it never spins.
//   match     one thread per hash slot: per reference lesion overlap, touching and a packed 64-bit atomicMax
//             (n_pt << 32 | ~p) for best_pred (ties to the smaller label whatever the arrival order), detection flags by
//             one float64 division per pair; then one thread per region: the per-class counts.  Integer atomics only.
//   score      one more pass over the hash slots with the same pair rules (pair_counts / pair_matches): per
//             reference lesion the largest vmax of its matching predictions, an atomicMax on order-preserving keys.
// Labels above a table's capacity are skipped everywhere (the table's overflow flag says so).
#include "common.hpp"
#include <limits.h>

namespace {
constexpr int MAXC = 16;
constexpr int TPB = 256;
constexpr int PER = 16;                  // consecutive voxels per lane
constexpr int CHUNK = TPB * PER;         // voxels per workgroup
constexpr int REG_SLOTS = 32;            // regions (pairs) a workgroup aggregates in LDS
constexpr unsigned GRID_CAP = 4096;
typedef unsigned long long u64;

struct Dims { int H, W, D; };

bool fill_dims(const int32_t* dims, Dims& g) {
    g.H = dims[0]; g.W = dims[1]; g.D = dims[2];
    return g.H >= 1 && g.W >= 1 && g.D >= 1 && (long)g.H * g.W * g.D < (1L << 31);
}
unsigned stride_grid(long n) { const long b = (n + TPB - 1) / TPB; return (unsigned)(b > GRID_CAP ? GRID_CAP : (b < 1 ? 1 : b)); }
unsigned chunk_grid(long n) { return (unsigned)((n + CHUNK - 1) / CHUNK); }

// ---------------------------------------------------------------------------------------------------- select
template <typename T> MIVP_DEV uint8_t listed_class(T v, int C, unsigned mask) {
    const int c = class_of<T>(v, C);
    return (c > 0 && ((mask >> c) & 1u)) ? (uint8_t)c : (uint8_t)0;
}

// 16 consecutive voxels per lane: vector loads of x (the host checked its 16-byte alignment, else ALIGNED = false and
// the loads stay scalar), one 16-byte store of the classes
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(TPB) void k_rg_select(const T* __restrict__ x, long n, int C, unsigned mask,
                                                   uint8_t* __restrict__ sel) {
    for (long v0 = ((long)blockIdx.x * TPB + threadIdx.x) * PER; v0 < n; v0 += (long)gridDim.x * TPB * PER) {
        if (ALIGNED && v0 + PER <= n) {
            const T* px = (const T*)__builtin_assume_aligned(x + v0, 16);
            union { uint8_t b[PER]; uint4 q; } o;
#pragma unroll
            for (int j = 0; j < PER; ++j) o.b[j] = listed_class<T>(px[j], C, mask);
            *reinterpret_cast<uint4*>(sel + v0) = o.q;
        } else {
            for (int j = 0; j < PER && v0 + j < n; ++j) sel[v0 + j] = listed_class<T>(x[v0 + j], C, mask);
        }
    }
}

template <typename T>
void select(const void* x, long n, int C, unsigned mask, uint8_t* sel, hipStream_t st) {
    const unsigned grid = stride_grid((n + PER - 1) / PER);
    if ((((uintptr_t)x | (uintptr_t)sel) & 15u) == 0)
        hipLaunchKernelGGL((k_rg_select<T, true>), dim3(grid), dim3(TPB), 0, st, (const T*)x, n, C, mask, sel);
    else
        hipLaunchKernelGGL((k_rg_select<T, false>), dim3(grid), dim3(TPB), 0, st, (const T*)x, n, C, mask, sel);
}

// ---------------------------------------------------------------------------------------------------- image values
// order-preserving uint32 key of a 32-bit value (min / max by unsigned atomics), and back
MIVP_DEV unsigned okey(int v) { return (unsigned)v ^ 0x80000000u; }
MIVP_DEV unsigned okey(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MIVP_DEV unsigned okey_decode_int(unsigned k) { return k ^ 0x80000000u; }
MIVP_DEV unsigned okey_decode_float(unsigned k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

struct NoImage {};
template <typename IT> struct ImgTraits {                       // integer images: int64 sums, exact modulo 2^64
    typedef long long Sum;
    typedef int Val;
    static MIVP_DEV Val load(const IT* p, long v) { return (int)p[v]; }
    static MIVP_DEV void add_lds(Sum* p, Sum s) { atomicAdd((u64*)p, (u64)s); }
    static MIVP_DEV void add_global(void* p, Sum s) { atomicAdd((u64*)p, (u64)s); }
};
template <> struct ImgTraits<float> {                           // float images: float64 sums, hardware atomics
    typedef double Sum;
    typedef float Val;
    static MIVP_DEV Val load(const float* p, long v) { return p[v]; }
    static MIVP_DEV void add_lds(Sum* p, Sum s) { atomicAdd(p, s); }
    static MIVP_DEV void add_global(void* p, Sum s) { unsafeAtomicAdd((double*)p, s); }
};
template <> struct ImgTraits<NoImage> {
    typedef long long Sum;
    typedef int Val;
    static MIVP_DEV Val load(const NoImage*, long) { return 0; }
    static MIVP_DEV void add_lds(Sum*, Sum) {}
    static MIVP_DEV void add_global(void*, Sum) {}
};

// device view of an MivpRegionTable
struct Tab {
    int cap;
    int* n; int* overflow; int* cls;
    long long* size; long long* first; int* bbox; long long* csum;
    unsigned* vmin; unsigned* vmax; void* vsum; void* vsq;
};
Tab view(const MivpRegionTable* t) {
    return Tab{t->capacity, t->n, t->overflow, t->cls, (long long*)t->size, (long long*)t->first, t->bbox,
               (long long*)t->coord_sum, (unsigned*)t->vmin, (unsigned*)t->vmax, t->vsum, t->vsqsum};
}
bool tab_ok(const MivpRegionTable* t) {
    return t && t->capacity >= 1 && t->n && t->overflow && t->cls && t->size && t->first && t->bbox && t->coord_sum;
}

template <typename IT> struct Run {
    typedef typename ImgTraits<IT>::Sum Sum;
    int lab, size, first;
    int mn[3], mx[3];
    long long cs[3];
    unsigned vmin, vmax;
    Sum vsum, vsq;
};

template <typename IT> struct SlotTable {
    typedef typename ImgTraits<IT>::Sum Sum;
    int key[REG_SLOTS];
    unsigned size[REG_SLOTS], first[REG_SLOTS];
    int mn[REG_SLOTS][3], mx[REG_SLOTS][3];
    u64 cs[REG_SLOTS][3];
    unsigned vmin[REG_SLOTS], vmax[REG_SLOTS];
    Sum vsum[REG_SLOTS], vsq[REG_SLOTS];
};

constexpr bool has_image(NoImage*) { return false; }
template <typename IT> constexpr bool has_image(IT*) { return true; }

// one run into global memory (label r + 1)
template <typename IT, typename R>
MIVP_DEV void run_to_global(const Tab& t, int r, unsigned size, unsigned first, const int* mn, const int* mx, const R* cs,
                            unsigned vmin, unsigned vmax, typename ImgTraits<IT>::Sum vsum,
                            typename ImgTraits<IT>::Sum vsq) {
    atomicAdd((u64*)t.size + r, (u64)size);
    atomicMin((u64*)t.first + r, (u64)first);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(t.bbox + r * 6 + a, mn[a]);
        atomicMax(t.bbox + r * 6 + 3 + a, mx[a]);
        atomicAdd((u64*)t.csum + r * 3 + a, (u64)cs[a]);
    }
    if (has_image((IT*)nullptr)) {
        atomicMin(t.vmin + r, vmin);
        atomicMax(t.vmax + r, vmax);
        ImgTraits<IT>::add_global((char*)t.vsum + 8 * (long)r, vsum);
        ImgTraits<IT>::add_global((char*)t.vsq + 8 * (long)r, vsq);
    }
}

// slot of `key` in the workgroup's table (claimed on first use), -1 when the table holds REG_SLOTS other keys
template <typename K> MIVP_DEV int claim_slot(K* keys, K key, K empty, unsigned start) {
    for (int i = 0; i < REG_SLOTS; ++i) {
        const int s = (int)((start + (unsigned)i) & (REG_SLOTS - 1));
        K k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == empty) {
            const K old = atomicCAS(keys + s, empty, key);
            k = old == empty ? key : old;
        }
        if (k == key) return s;
    }
    return -1;
}

template <typename IT> MIVP_DEV void flush_run(const Run<IT>& r, SlotTable<IT>& st, const Tab& t) {
    const int s = claim_slot<int>(st.key, r.lab, 0, (unsigned)r.lab);
    if (s < 0) {
        run_to_global<IT>(t, r.lab - 1, (unsigned)r.size, (unsigned)r.first, r.mn, r.mx, r.cs, r.vmin, r.vmax, r.vsum, r.vsq);
        return;
    }
    atomicAdd(&st.size[s], (unsigned)r.size);
    atomicMin(&st.first[s], (unsigned)r.first);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(&st.mn[s][a], r.mn[a]);
        atomicMax(&st.mx[s][a], r.mx[a]);
        atomicAdd(&st.cs[s][a], (u64)r.cs[a]);
    }
    if (has_image((IT*)nullptr)) {
        atomicMin(&st.vmin[s], r.vmin);
        atomicMax(&st.vmax[s], r.vmax);
        ImgTraits<IT>::add_lds(&st.vsum[s], r.vsum);
        ImgTraits<IT>::add_lds(&st.vsq[s], r.vsq);
    }
}

// ---------------------------------------------------------------------------------------------------- reduce
__global__ __launch_bounds__(TPB) void k_rg_init(Tab t, int image) {
    for (int r = blockIdx.x * TPB + threadIdx.x; r < t.cap; r += gridDim.x * TPB) {
        t.size[r] = 0;
        t.first[r] = LLONG_MAX;
        for (int a = 0; a < 3; ++a) { t.bbox[r * 6 + a] = INT_MAX; t.bbox[r * 6 + 3 + a] = INT_MIN; t.csum[r * 3 + a] = 0; }
        if (image) { t.vmin[r] = 0xFFFFFFFFu; t.vmax[r] = 0u; ((u64*)t.vsum)[r] = 0ull; ((u64*)t.vsq)[r] = 0ull; }
    }
}

template <typename IT>
__global__ __launch_bounds__(TPB) void k_rg_reduce(const int* __restrict__ lab, const IT* __restrict__ img, Dims g, long n,
                                                   Tab t) {
    typedef typename ImgTraits<IT>::Sum Sum;
    __shared__ SlotTable<IT> st;
    if (threadIdx.x < REG_SLOTS) {
        const int s = threadIdx.x;
        st.key[s] = 0; st.size[s] = 0u; st.first[s] = 0xFFFFFFFFu;
        for (int a = 0; a < 3; ++a) { st.mn[s][a] = INT_MAX; st.mx[s][a] = INT_MIN; st.cs[s][a] = 0ull; }
        st.vmin[s] = 0xFFFFFFFFu; st.vmax[s] = 0u; st.vsum[s] = (Sum)0; st.vsq[s] = (Sum)0;
    }
    __syncthreads();
    const long v0 = (long)blockIdx.x * CHUNK + (long)threadIdx.x * PER;
    if (v0 < n) {
        int l[PER];
        if (v0 + PER <= n) {
#pragma unroll
            for (int j = 0; j < PER; j += 4) {
                const int4 q = *reinterpret_cast<const int4*>(lab + v0 + j);
                l[j] = q.x; l[j + 1] = q.y; l[j + 2] = q.z; l[j + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PER; ++j) l[j] = v0 + j < n ? lab[v0 + j] : 0;
        }
        int d = (int)(v0 % g.D);
        const long hw = v0 / g.D;
        int w = (int)(hw % g.W), h = (int)(hw / g.W);
        Run<IT> r;
        r.lab = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int a = l[j];
            if (a > 0 && a <= t.cap) {
                if (a != r.lab) {
                    if (r.lab) flush_run<IT>(r, st, t);
                    r.lab = a; r.size = 0; r.first = (int)(v0 + j);
                    r.mn[0] = h; r.mn[1] = w; r.mn[2] = d; r.mx[0] = h; r.mx[1] = w; r.mx[2] = d;
                    r.cs[0] = r.cs[1] = r.cs[2] = 0;
                    r.vmin = 0xFFFFFFFFu; r.vmax = 0u; r.vsum = (Sum)0; r.vsq = (Sum)0;
                }
                ++r.size;
                r.cs[0] += h; r.cs[1] += w; r.cs[2] += d;
                r.mn[0] = min(r.mn[0], h); r.mn[1] = min(r.mn[1], w); r.mn[2] = min(r.mn[2], d);
                r.mx[0] = max(r.mx[0], h); r.mx[1] = max(r.mx[1], w); r.mx[2] = max(r.mx[2], d);
                if (has_image((IT*)nullptr)) {
                    const typename ImgTraits<IT>::Val x = ImgTraits<IT>::load(img, v0 + j);
                    const unsigned k = okey(x);
                    r.vmin = min(r.vmin, k); r.vmax = max(r.vmax, k);
                    const Sum xs = (Sum)x;
                    r.vsum += xs; r.vsq += xs * xs;
                }
            }
            if (++d == g.D) { d = 0; if (++w == g.W) { w = 0; ++h; } }
        }
        if (r.lab) flush_run<IT>(r, st, t);
    }
    __syncthreads();
    if (threadIdx.x < REG_SLOTS && st.key[threadIdx.x] != 0) {
        const int s = threadIdx.x;
        run_to_global<IT>(t, st.key[s] - 1, st.size[s], st.first[s], st.mn[s], st.mx[s], st.cs[s], st.vmin[s], st.vmax[s],
                          st.vsum[s], st.vsq[s]);
    }
}

// entries below min(n, capacity): the class from the first voxel, image minima / maxima decoded; the rest zeroed
__global__ __launch_bounds__(TPB) void k_rg_finish(Tab t, const uint8_t* __restrict__ sel, int image) {
    const int n = t.n[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) t.overflow[0] = n > t.cap ? 1 : 0;
    for (int r = blockIdx.x * TPB + threadIdx.x; r < t.cap; r += gridDim.x * TPB) {
        if (r < n) {
            t.cls[r] = (int)sel[t.first[r]];
            if (image == 1) { t.vmin[r] = okey_decode_int(t.vmin[r]); t.vmax[r] = okey_decode_int(t.vmax[r]); }
            if (image == 2) { t.vmin[r] = okey_decode_float(t.vmin[r]); t.vmax[r] = okey_decode_float(t.vmax[r]); }
        } else {
            t.cls[r] = 0; t.size[r] = 0; t.first[r] = 0;
            for (int a = 0; a < 6; ++a) t.bbox[r * 6 + a] = 0;
            for (int a = 0; a < 3; ++a) t.csum[r * 3 + a] = 0;
            if (image) { t.vmin[r] = 0u; t.vmax[r] = 0u; ((u64*)t.vsum)[r] = 0ull; ((u64*)t.vsq)[r] = 0ull; }
        }
    }
}

template <typename IT>
void reduce(const int* lab, const void* img, const Dims& g, const Tab& t, hipStream_t st) {
    const long n = (long)g.H * g.W * g.D;
    hipLaunchKernelGGL(k_rg_reduce<IT>, dim3(chunk_grid(n)), dim3(TPB), 0, st, lab, (const IT*)img, g, n, t);
}

// ---------------------------------------------------------------------------------------------------- overlap
// pair workspace: int64 words; [0] number of distinct pairs, [1] overflow flag, then keys[slots], then counts[slots]
constexpr int PAIR_HEAD = 2;
long pair_slots(long max_pairs) {
    long s = 64;
    while (s < 2 * max_pairs) s <<= 1;
    return s;
}
struct Pairs { long long* head; u64* keys; long long* counts; long slots; long max_pairs; };
Pairs pairs_view(void* ws, long max_pairs) {
    Pairs p;
    p.head = (long long*)ws;
    p.slots = pair_slots(max_pairs);
    p.keys = (u64*)ws + PAIR_HEAD;
    p.counts = (long long*)ws + PAIR_HEAD + p.slots;
    p.max_pairs = max_pairs;
    return p;
}

__global__ __launch_bounds__(TPB) void k_ov_init(Pairs p) {
    const long words = PAIR_HEAD + 2 * p.slots;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < words; i += (long)gridDim.x * TPB) p.head[i] = 0;
}

MIVP_DEV unsigned hash_pair(u64 k) {
    k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33;
    return (unsigned)k;
}

// count += cnt for key; the probe sequence visits every slot at most once, and nothing is tried once the table overflowed
MIVP_DEV void pair_insert(const Pairs& p, u64 key, long long cnt) {
    if (__hip_atomic_load(p.head + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const u64 m = (u64)p.slots - 1;
    u64 h = hash_pair(key) & m;
    for (long i = 0; i < p.slots; ++i) {
        u64 k = __hip_atomic_load(p.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0ull) {
            const u64 old = atomicCAS(p.keys + h, 0ull, key);
            if (old == 0ull) {
                k = key;
                const u64 before = atomicAdd((u64*)p.head, 1ull);
                if ((long long)before >= p.max_pairs) atomicMax((u64*)p.head + 1, 1ull);
            } else {
                k = old;
            }
        }
        if (k == key) { atomicAdd((u64*)p.counts + h, (u64)cnt); return; }
        h = (h + 1) & m;
    }
    atomicMax((u64*)p.head + 1, 1ull);
}

struct PairSlots { u64 key[REG_SLOTS]; unsigned cnt[REG_SLOTS]; };

MIVP_DEV void flush_pair(u64 key, int cnt, PairSlots& st, const Pairs& p, const int* __restrict__ cls_p,
                         const int* __restrict__ cls_t) {
    if (cls_p[(int)(key >> 32) - 1] != cls_t[(int)(unsigned)key - 1]) return;      // pairs of one class only
    const int s = claim_slot<u64>(st.key, key, 0ull, hash_pair(key));
    if (s < 0) pair_insert(p, key, cnt);
    else atomicAdd(&st.cnt[s], (unsigned)cnt);
}

__global__ __launch_bounds__(TPB) void k_ov_count(const int* __restrict__ lp, const int* __restrict__ lt, long n, int cap_p,
                                                  int cap_t, const int* __restrict__ cls_p, const int* __restrict__ cls_t,
                                                  Pairs p) {
    __shared__ PairSlots st;
    if (threadIdx.x < REG_SLOTS) { st.key[threadIdx.x] = 0ull; st.cnt[threadIdx.x] = 0u; }
    __syncthreads();
    const long v0 = (long)blockIdx.x * CHUNK + (long)threadIdx.x * PER;
    if (v0 < n) {
        int a[PER], b[PER];
        if (v0 + PER <= n) {
#pragma unroll
            for (int j = 0; j < PER; j += 4) {
                const int4 q = *reinterpret_cast<const int4*>(lp + v0 + j);
                const int4 s = *reinterpret_cast<const int4*>(lt + v0 + j);
                a[j] = q.x; a[j + 1] = q.y; a[j + 2] = q.z; a[j + 3] = q.w;
                b[j] = s.x; b[j + 1] = s.y; b[j + 2] = s.z; b[j + 3] = s.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PER; ++j) { a[j] = v0 + j < n ? lp[v0 + j] : 0; b[j] = v0 + j < n ? lt[v0 + j] : 0; }
        }
        u64 cur = 0ull;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (a[j] > 0 && a[j] <= cap_p && b[j] > 0 && b[j] <= cap_t) {
                const u64 key = ((u64)(unsigned)a[j] << 32) | (u64)(unsigned)b[j];
                if (key != cur) {
                    if (cur) flush_pair(cur, cnt, st, p, cls_p, cls_t);
                    cur = key; cnt = 0;
                }
                ++cnt;
            }
        }
        if (cur) flush_pair(cur, cnt, st, p, cls_p, cls_t);
    }
    __syncthreads();
    if (threadIdx.x < REG_SLOTS && st.key[threadIdx.x] != 0ull) pair_insert(p, st.key[threadIdx.x], (long long)st.cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------- match
struct Match {
    long long* counts;      // [C][4]
    long long* overlap; long long* touching; long long* best;   // per reference lesion; best: packed key, then n_pt
    int* best_pred; int* detected; int* matched;                // detected per reference lesion, matched per prediction
};

__global__ __launch_bounds__(TPB) void k_mt_init(Match m, int cap_p, int cap_t, int C) {
    const int i0 = blockIdx.x * TPB + threadIdx.x;
    if (i0 < C * 4) m.counts[i0] = 0;
    for (int i = i0; i < cap_t; i += gridDim.x * TPB) {
        m.overlap[i] = 0; m.touching[i] = 0; m.best[i] = 0; m.best_pred[i] = 0; m.detected[i] = 0;
    }
    for (int i = i0; i < cap_p; i += gridDim.x * TPB) m.matched[i] = 0;
}

// The pair rules of DESIGN 4.20, shared by k_mt_pairs and k_bs_pairs.  A pair counts when it overlaps and neither region is
// below min_size; it is a match when its IoU (one float64 division) meets the threshold.
MIVP_DEV bool pair_counts(long long n, long long sp, long long st, long long min_size) {
    return n > 0 && sp >= min_size && st >= min_size;
}
MIVP_DEV bool pair_matches(long long n, long long sp, long long st, double thr) {
    const double iou = (double)n / (double)(sp + st - n);
    return thr == 0.0 ? iou > 0.0 : iou >= thr;
}

__global__ __launch_bounds__(TPB) void k_mt_pairs(Pairs p, const long long* __restrict__ size_p,
                                                  const long long* __restrict__ size_t_, long long min_size, double thr,
                                                  Match m) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < p.slots; i += (long)gridDim.x * TPB) {
        const u64 key = p.keys[i];
        if (key == 0ull) continue;
        const int pp = (int)(key >> 32), tt = (int)(unsigned)key;
        const long long n = p.counts[i], sp = size_p[pp - 1], st = size_t_[tt - 1];
        if (!pair_counts(n, sp, st, min_size)) continue;
        atomicAdd((u64*)m.overlap + (tt - 1), (u64)n);
        atomicAdd((u64*)m.touching + (tt - 1), (u64)sp);
        atomicMax((u64*)m.best + (tt - 1), ((u64)n << 32) | (u64)(0xFFFFFFFFu - (unsigned)pp));
        if (pair_matches(n, sp, st, thr)) {
            atomicMax(m.detected + (tt - 1), 1);
            atomicMax(m.matched + (pp - 1), 1);
        }
    }
}

// best_score: per reference lesion the largest vmax over its matching predictions, as order-preserving keys until
// k_bs_finish decodes them (-inf where there is no match); score: a copy of the predictions' vmax
__global__ __launch_bounds__(TPB) void k_bs_init(unsigned* __restrict__ best, float* __restrict__ score,
                                                 const float* __restrict__ vmax_p, int cap_p, int cap_t) {
    const int i0 = blockIdx.x * TPB + threadIdx.x;
    for (int i = i0; i < cap_t; i += gridDim.x * TPB) best[i] = okey(-INFINITY);
    for (int i = i0; i < cap_p; i += gridDim.x * TPB) score[i] = vmax_p[i];
}

__global__ __launch_bounds__(TPB) void k_bs_pairs(Pairs p, const long long* __restrict__ size_p,
                                                  const long long* __restrict__ size_t_, const float* __restrict__ vmax_p,
                                                  long long min_size, double thr, unsigned* __restrict__ best) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < p.slots; i += (long)gridDim.x * TPB) {
        const u64 key = p.keys[i];
        if (key == 0ull) continue;
        const int pp = (int)(key >> 32), tt = (int)(unsigned)key;
        const long long n = p.counts[i], sp = size_p[pp - 1], st = size_t_[tt - 1];
        if (pair_counts(n, sp, st, min_size) && pair_matches(n, sp, st, thr)) atomicMax(best + (tt - 1), okey(vmax_p[pp - 1]));
    }
}

__global__ __launch_bounds__(TPB) void k_bs_finish(unsigned* __restrict__ best, int cap_t) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < cap_t; i += gridDim.x * TPB) best[i] = okey_decode_float(best[i]);
}

__global__ __launch_bounds__(TPB) void k_mt_finish(Tab tp, Tab tt, long long min_size, int C, Match m) {
    __shared__ unsigned sm[MAXC * 4];
    if (threadIdx.x < MAXC * 4) sm[threadIdx.x] = 0u;
    __syncthreads();
    const int np = min(tp.n[0], tp.cap), nt = min(tt.n[0], tt.cap);
    for (int i = blockIdx.x * TPB + threadIdx.x; i < max(np, nt); i += gridDim.x * TPB) {
        if (i < nt) {
            const u64 b = (u64)m.best[i];
            m.best_pred[i] = b ? (int)(0xFFFFFFFFu - (unsigned)b) : 0;
            m.best[i] = (long long)(b >> 32);
            const int c = tt.cls[i];
            if (tt.size[i] >= min_size && c > 0 && c < C) {
                atomicAdd(&sm[c * 4 + 0], 1u);
                if (m.detected[i]) atomicAdd(&sm[c * 4 + 2], 1u);
            }
        }
        if (i < np) {
            const int c = tp.cls[i];
            if (tp.size[i] >= min_size && c > 0 && c < C) {
                atomicAdd(&sm[c * 4 + 1], 1u);
                if (m.matched[i]) atomicAdd(&sm[c * 4 + 3], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < C * 4 && sm[threadIdx.x]) atomicAdd((u64*)m.counts + threadIdx.x, (u64)sm[threadIdx.x]);
}

size_t align256(size_t b) { return (b + 255) / 256 * 256; }
}  // namespace

extern "C" size_t mivp_region_stats_ws(const int32_t* dims) {
    Dims g;
    if (!dims || !fill_dims(dims, g)) return 0;
    return align256((size_t)g.H * g.W * g.D) + mivp_label_ws(dims);
}

extern "C" int mivp_region_stats(const void* x, int32_t dtype, const int32_t* dims, int32_t C, uint32_t class_mask,
                                 int32_t connectivity, const void* image, int32_t* labels, const MivpRegionTable* table,
                                 void* workspace, mivp_stream_t stream) {
    MIVP_REQUIRE(x && dims && labels && workspace && dtype >= 0 && dtype <= 3 && C >= 1 && C <= MAXC);
    MIVP_REQUIRE(class_mask != 0u && (class_mask & 1u) == 0u && (class_mask >> C) == 0u);
    MIVP_REQUIRE(tab_ok(table));
    MIVP_REQUIRE(((uintptr_t)labels & 15u) == 0);
    const int idt = table->image_dtype;
    MIVP_REQUIRE(idt == -1 || idt == 0 || idt == 1 || idt == 3 || idt == 4);
    MIVP_REQUIRE((image == nullptr) == (idt == -1));
    MIVP_REQUIRE(idt == -1 || (table->vmin && table->vmax && table->vsum && table->vsqsum));
    Dims g;
    MIVP_REQUIRE(fill_dims(dims, g));
    const long nvox = (long)g.H * g.W * g.D;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* sel = (uint8_t*)workspace;
    void* label_ws = (char*)workspace + align256((size_t)nvox);
    switch (dtype) {
        case 0: select<uint8_t>(x, nvox, (int)C, class_mask, sel, st); break;
        case 1: select<int32_t>(x, nvox, (int)C, class_mask, sel, st); break;
        case 2: select<int64_t>(x, nvox, (int)C, class_mask, sel, st); break;
        default: select<float>(x, nvox, (int)C, class_mask, sel, st); break;
    }
    const int rc = mivp_label_components(sel, 0, dims, connectivity, labels, table->n, label_ws, stream);
    if (rc != MIVP_OK) return rc;
    const Tab t = view(table);
    const int image_kind = idt == -1 ? 0 : idt == 3 ? 2 : 1;
    hipLaunchKernelGGL(k_rg_init, dim3(stride_grid(t.cap)), dim3(TPB), 0, st, t, image_kind);
    switch (idt) {
        case -1: reduce<NoImage>(labels, nullptr, g, t, st); break;
        case 0: reduce<uint8_t>(labels, image, g, t, st); break;
        case 1: reduce<int32_t>(labels, image, g, t, st); break;
        case 3: reduce<float>(labels, image, g, t, st); break;
        default: reduce<int16_t>(labels, image, g, t, st); break;
    }
    hipLaunchKernelGGL(k_rg_finish, dim3(stride_grid(t.cap)), dim3(TPB), 0, st, t, (const uint8_t*)sel, image_kind);
    return mivp_check_launch("region_stats");
}

extern "C" size_t mivp_region_overlap_ws(int64_t max_pairs) {
    if (max_pairs < 1 || max_pairs > (1LL << 28)) return 0;
    return (size_t)(PAIR_HEAD + 2 * pair_slots((long)max_pairs)) * 8;
}

extern "C" int mivp_region_overlap(const int32_t* labels_pred, const int32_t* labels_target, const int32_t* dims,
                                   const MivpRegionTable* pred, const MivpRegionTable* target, int64_t max_pairs,
                                   void* pairs, mivp_stream_t stream) {
    MIVP_REQUIRE(labels_pred && labels_target && dims && pairs && tab_ok(pred) && tab_ok(target));
    MIVP_REQUIRE(max_pairs >= 1 && max_pairs <= (1LL << 28));
    MIVP_REQUIRE((((uintptr_t)labels_pred | (uintptr_t)labels_target) & 15u) == 0 && ((uintptr_t)pairs & 7u) == 0);
    Dims g;
    MIVP_REQUIRE(fill_dims(dims, g));
    const long nvox = (long)g.H * g.W * g.D;
    hipStream_t st = (hipStream_t)stream;
    const Pairs p = pairs_view(pairs, (long)max_pairs);
    hipLaunchKernelGGL(k_ov_init, dim3(stride_grid(PAIR_HEAD + 2 * p.slots)), dim3(TPB), 0, st, p);
    hipLaunchKernelGGL(k_ov_count, dim3(chunk_grid(nvox)), dim3(TPB), 0, st, (const int*)labels_pred,
                       (const int*)labels_target, nvox, (int)pred->capacity, (int)target->capacity,
                       (const int*)pred->cls, (const int*)target->cls, p);
    return mivp_check_launch("region_overlap");
}

extern "C" int mivp_lesion_match(const MivpRegionTable* pred, const MivpRegionTable* target, const void* pairs,
                                 int64_t max_pairs, int32_t C, int64_t min_size, double iou_threshold, int64_t* counts,
                                 int64_t* overlap, int64_t* touching, int64_t* best_overlap, int32_t* best_pred,
                                 int32_t* detected, int32_t* matched, mivp_stream_t stream) {
    MIVP_REQUIRE(tab_ok(pred) && tab_ok(target) && pairs && counts && overlap && touching && best_overlap && best_pred &&
                 detected && matched);
    MIVP_REQUIRE(max_pairs >= 1 && max_pairs <= (1LL << 28) && C >= 1 && C <= MAXC && min_size >= 0);
    MIVP_REQUIRE(iou_threshold >= 0.0 && iou_threshold <= 1.0);
    hipStream_t st = (hipStream_t)stream;
    const Pairs p = pairs_view(const_cast<void*>(pairs), (long)max_pairs);
    const Tab tp = view(pred), tt = view(target);
    const Match m{(long long*)counts, (long long*)overlap, (long long*)touching, (long long*)best_overlap, best_pred,
                  detected, matched};
    const int cap = tp.cap > tt.cap ? tp.cap : tt.cap;
    hipLaunchKernelGGL(k_mt_init, dim3(stride_grid(cap > 64 ? cap : 64)), dim3(TPB), 0, st, m, tp.cap, tt.cap, (int)C);
    hipLaunchKernelGGL(k_mt_pairs, dim3(stride_grid(p.slots)), dim3(TPB), 0, st, p, (const long long*)tp.size,
                       (const long long*)tt.size, (long long)min_size, iou_threshold, m);
    hipLaunchKernelGGL(k_mt_finish, dim3(stride_grid(cap)), dim3(TPB), 0, st, tp, tt, (long long)min_size, (int)C, m);
    return mivp_check_launch("lesion_match");
}

extern "C" int mivp_lesion_best_score(const MivpRegionTable* pred, const MivpRegionTable* target, const void* pairs,
                                      int64_t max_pairs, int64_t min_size, double iou_threshold, float* best_score,
                                      float* score, mivp_stream_t stream) {
    MIVP_REQUIRE(tab_ok(pred) && tab_ok(target) && pairs && best_score && score);
    MIVP_REQUIRE(pred->image_dtype == 3 && pred->vmax);
    MIVP_REQUIRE(max_pairs >= 1 && max_pairs <= (1LL << 28) && min_size >= 0);
    MIVP_REQUIRE(iou_threshold >= 0.0 && iou_threshold <= 1.0);
    hipStream_t st = (hipStream_t)stream;
    const Pairs p = pairs_view(const_cast<void*>(pairs), (long)max_pairs);
    const Tab tp = view(pred), tt = view(target);
    const int cap = tp.cap > tt.cap ? tp.cap : tt.cap;
    hipLaunchKernelGGL(k_bs_init, dim3(stride_grid(cap)), dim3(TPB), 0, st, (unsigned*)best_score, score,
                       (const float*)tp.vmax, tp.cap, tt.cap);
    hipLaunchKernelGGL(k_bs_pairs, dim3(stride_grid(p.slots)), dim3(TPB), 0, st, p, (const long long*)tp.size,
                       (const long long*)tt.size, (const float*)tp.vmax, (long long)min_size, iou_threshold,
                       (unsigned*)best_score);
    hipLaunchKernelGGL(k_bs_finish, dim3(stride_grid(tt.cap)), dim3(TPB), 0, st, (unsigned*)best_score, tt.cap);
    return mivp_check_launch("lesion_best_score");
}
