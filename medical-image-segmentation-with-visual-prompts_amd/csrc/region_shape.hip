// Per-lesion shape descriptors over the dense label map of mivp_region_stats (joined ABI 18, mivp_amd/regions.py
// region_shape).
//
// Volumes are [H][W][D] row-major (D contiguous), fewer than 2^31 voxels, no dimension above 65535.
//   shape     one pass over the labels.  A workgroup owns a brick of BH x BW x BD voxels and stages its labels with a
//             one-voxel halo in LDS (0 outside the volume).  Wave s of the workgroup owns the D segment [16 s, 16 s + 16) of
//             every (h, w) row of the brick, lane = row, so a lane walks 16 consecutive voxels along D with a sliding window
//             over the four earlier neighbour columns.  Per voxel of region r, all from LDS:
//               moment2  h*h, w*w, d*d, h*w, h*d, w*d on voxel indices (each below 2^32; fewer than 2^31 voxels: no sum
//                        reaches 2^63);
//               faces    per axis the faces whose voxel across does not carry r (or lies outside): 0..2 each;
//               cells    the vertices (of 8) and edges (of 12) of the closed unit cube that no EARLIER voxel of r shares:
//                        a vertex has 8 incident voxels, an edge 4, and the first incident voxel of r in raster order counts
//                        it.  The 13 raster-earlier voxels of the 3x3x3 neighbourhood give a 13-bit "same label" mask; a
//                        vertex (edge) is counted when the mask misses the constant set of its earlier incident voxels.
//             A lane keeps one run (label, count, sum d, sum d*d, 5 counts) across background voxels, like the reduce pass of
//             regions.hip; h and w are the lane's, so the six moments are formed when the run ends.  A run
//             that ends is added to the workgroup's LDS slot table (SHP_SLOTS regions, claimed by an LDS atomicCAS on first
//             use; surplus regions go to global memory directly), and one lane per used slot flushes it: one set of global
//             atomics per (workgroup, region).  Integer atomics only: bitwise reproducible.
//   axes      one thread per region, float64: the covariance numerator n M_ab - S_a S_b exactly in 128-bit integers, one
//             correctly rounded conversion, one division by n * n (exact below 2^26 voxels), scaled by the spacings; then a
//             cyclic Jacobi iteration with a fixed sweep order and JACOBI_SWEEPS sweeps at most.
// Labels above the capacity are skipped (the region table's overflow flag says so); they still differ from every listed
// label, so they expose the faces of their neighbours like background does.
#include "common.hpp"

namespace {
constexpr int TPB = 256;
constexpr int BH = 8, BW = 8, BD = 64;            // brick
constexpr int PER = 16;                           // consecutive voxels per lane along D: BD = 4 waves x PER
constexpr int LW = BW + 2;                        // halo'd rows per h
constexpr int LD = BD + 3;                        // halo'd row length, padded to an odd number of dwords (banks)
constexpr int TILE = (BH + 2) * LW * LD;
constexpr int SHP_SLOTS = 32;                     // regions a workgroup aggregates in LDS
constexpr int JACOBI_SWEEPS = 16;
typedef unsigned long long u64;
static_assert(BH * BW == 64 && BD == (TPB / 64) * PER, "wave s owns D segment s of the 64 rows");

struct Dims { int H, W, D; };

bool fill_dims(const int32_t* dims, Dims& g) {
    g.H = dims[0]; g.W = dims[1]; g.D = dims[2];
    return g.H >= 1 && g.W >= 1 && g.D >= 1 && g.H <= 65535 && g.W <= 65535 && g.D <= 65535 &&
           (long)g.H * g.W * g.D < (1L << 31);
}

// ---------------------------------------------------------------------------------------------------- the cell masks
// bit of the raster-earlier neighbour at offset (dh, dw, dd), -1 for the voxel itself and the later ones
constexpr int earlier_bit(int dh, int dw, int dd) {
    return dh < 0 ? (dw + 1) * 3 + (dd + 1) : dh > 0 ? -1 : dw < 0 ? 9 + (dd + 1) : dw > 0 ? -1 : dd < 0 ? 12 : -1;
}
// the earlier voxels incident to the vertex at corner (a, b, c) of the unit cube, a, b, c in {0, 1}
constexpr unsigned vertex_mask(int a, int b, int c) {
    unsigned m = 0;
    for (int i = a - 1; i <= a; ++i)
        for (int j = b - 1; j <= b; ++j)
            for (int k = c - 1; k <= c; ++k)
                if (earlier_bit(i, j, k) >= 0) m |= 1u << earlier_bit(i, j, k);
    return m;
}
// the earlier voxels incident to the edge along `axis` at corner (p, q) of the two other axes (in h, w, d order)
constexpr unsigned edge_mask(int axis, int p, int q) {
    unsigned m = 0;
    for (int i = p - 1; i <= p; ++i)
        for (int j = q - 1; j <= q; ++j) {
            const int b = axis == 0 ? earlier_bit(0, i, j) : axis == 1 ? earlier_bit(i, 0, j) : earlier_bit(i, j, 0);
            if (b >= 0) m |= 1u << b;
        }
    return m;
}
static_assert(vertex_mask(1, 1, 1) == 0u && edge_mask(2, 1, 1) == 0u && edge_mask(2, 0, 0) == ((1u << 1) | (1u << 4) | (1u << 10)) &&
              vertex_mask(0, 0, 0) == ((1u << 0) | (1u << 1) | (1u << 3) | (1u << 4) | (1u << 9) | (1u << 10) | (1u << 12)),
              "the last corner has no earlier owner; the first d-edge has three, the first corner seven");

MIVP_DEV void count_cells(unsigned m, unsigned& v, unsigned& e) {
    v = 0u; e = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) v += (m & vertex_mask(c >> 2, (c >> 1) & 1, c & 1)) == 0u ? 1u : 0u;
#pragma unroll
    for (int x = 0; x < 12; ++x) e += (m & edge_mask(x >> 2, (x >> 1) & 1, x & 1)) == 0u ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------------- shape
struct ShapeOut { u64* moment2; u64* faces; u64* cells; int cap; };

__global__ __launch_bounds__(TPB) void k_rs_zero(ShapeOut o) {
    const long n = (long)o.cap;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < 6 * n; i += (long)gridDim.x * TPB) {
        o.moment2[i] = 0ull;
        if (i < 3 * n) o.faces[i] = 0ull;
        if (i < 2 * n) o.cells[i] = 0ull;
    }
}

// a lane's run: h and w are the lane's, so the six moments follow from the count, sum d and sum d*d when the run ends
struct Run { int lab; unsigned cnt, sd; u64 sdd; unsigned f[3], c[2]; };
struct SlotTable { int key[SHP_SLOTS]; u64 m[SHP_SLOTS][6]; unsigned f[SHP_SLOTS][3], c[SHP_SLOTS][2]; };

template <typename F> MIVP_DEV void sums_to_global(const ShapeOut& o, int r, const u64* m, const F* f, const F* c) {
#pragma unroll
    for (int a = 0; a < 6; ++a) atomicAdd(o.moment2 + (long)r * 6 + a, m[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(o.faces + (long)r * 3 + a, (u64)f[a]);
#pragma unroll
    for (int a = 0; a < 2; ++a) atomicAdd(o.cells + (long)r * 2 + a, (u64)c[a]);
}

// slot of `key` in the workgroup's table (claimed on first use), -1 when the table holds SHP_SLOTS other keys (the private
// copy of the sibling pass's helper)
MIVP_DEV int claim_slot(int* keys, int key) {
    for (int i = 0; i < SHP_SLOTS; ++i) {
        const int s = (key + i) & (SHP_SLOTS - 1);
        int k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0) {
            const int old = atomicCAS(keys + s, 0, key);
            k = old == 0 ? key : old;
        }
        if (k == key) return s;
    }
    return -1;
}

MIVP_DEV void flush_run(const Run& r, u64 h, u64 w, SlotTable& st, const ShapeOut& o) {
    const u64 m[6] = {r.cnt * h * h, r.cnt * w * w, r.sdd, r.cnt * h * w, h * r.sd, w * r.sd};
    const int s = claim_slot(st.key, r.lab);
    if (s < 0) { sums_to_global<unsigned>(o, r.lab - 1, m, r.f, r.c); return; }
#pragma unroll
    for (int a = 0; a < 6; ++a) atomicAdd(&st.m[s][a], m[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) atomicAdd(&st.f[s][a], r.f[a]);
#pragma unroll
    for (int a = 0; a < 2; ++a) atomicAdd(&st.c[s][a], r.c[a]);
}

__global__ __launch_bounds__(TPB) void k_rs_shape(const int* __restrict__ lab, Dims g, int nbw, int nbd, ShapeOut o) {
    __shared__ int tile[TILE];
    __shared__ SlotTable st;
    const int tid = threadIdx.x;
    if (tid < SHP_SLOTS) {
        st.key[tid] = 0;
        for (int a = 0; a < 6; ++a) st.m[tid][a] = 0ull;
        for (int a = 0; a < 3; ++a) st.f[tid][a] = 0u;
        for (int a = 0; a < 2; ++a) st.c[tid][a] = 0u;
    }
    const int bd = (int)(blockIdx.x % (unsigned)nbd);
    const int bhw = (int)(blockIdx.x / (unsigned)nbd);
    const int h0 = (bhw / nbw) * BH, w0 = (bhw % nbw) * BW, d0 = bd * BD;
    // the brick with its halo: consecutive lanes read consecutive d of one (h, w) row; 0 outside the volume
    // (a wave takes every fourth halo'd row: the row's place is wave-uniform, lane l reads d0 - 1 + l, lanes 0 and 1 also the
    // last two)
    const int lane = tid & 63;
#pragma unroll 5
    for (int row = tid >> 6; row < (BH + 2) * LW; row += TPB / 64) {
        const int hh = row / LW, ww = row - hh * LW;
        const int h = h0 + hh - 1, w = w0 + ww - 1;
        const bool in = h >= 0 && h < g.H && w >= 0 && w < g.W;
        const int* src = lab + ((long)(in ? h : 0) * g.W + (in ? w : 0)) * g.D;
        const int d = d0 - 1 + lane, dt = d0 + BD - 1 + lane;
        int v = 0, vt = 0;
        if (in && d >= 0 && d < g.D) v = src[d];
        if (in && lane < 2 && dt < g.D) vt = src[dt];
        tile[row * LD + lane] = v;
        if (lane < 2) tile[row * LD + BD + lane] = vt;
    }
    __syncthreads();
    const int seg = tid >> 6, lh = (tid & 63) >> 3, lw = tid & 7;
    const int h = h0 + lh, w = w0 + lw, dbase = d0 + seg * PER;
    if (h < g.H && w < g.W && dbase < g.D) {
        // tile rows of this lane's neighbour columns (dh, dw), at the lane's first voxel minus one along d
        const int* S = tile + ((lh + 1) * LW + (lw + 1)) * LD + seg * PER;
        int s[PER + 2];
        int any = 0;
#pragma unroll
        for (int j = 0; j < PER + 2; ++j) s[j] = S[j];
#pragma unroll
        for (int j = 1; j <= PER; ++j) any |= s[j];
        if (any != 0) {
            const int* A = S - LW * LD - LD;          // (-1, -1)
            const int* B = S - LW * LD;               // (-1,  0)
            const int* C = S - LW * LD + LD;          // (-1, +1)
            const int* E = S - LD;                    // ( 0, -1)
            int a0 = A[0], a1 = A[1], b0 = B[0], b1 = B[1], c0 = C[0], c1 = C[1], e0 = E[0], e1 = E[1];
            const u64 uh = (u64)h, uw = (u64)w;
            Run r;
            r.lab = 0;
#pragma unroll
            for (int j = 1; j <= PER; ++j) {
                const int a2 = A[j + 1], b2 = B[j + 1], c2 = C[j + 1], e2 = E[j + 1];
                const int x = s[j];
                if (x > 0 && x <= o.cap) {                     // (voxels beyond D were staged as 0)
                    if (x != r.lab) {
                        if (r.lab) flush_run(r, uh, uw, st, o);
                        r.lab = x; r.cnt = 0u; r.sd = 0u; r.sdd = 0ull;
                        r.f[0] = r.f[1] = r.f[2] = 0u; r.c[0] = r.c[1] = 0u;
                    }
                    const unsigned m = (unsigned)(a0 == x) | (unsigned)(a1 == x) << 1 | (unsigned)(a2 == x) << 2 |
                                       (unsigned)(b0 == x) << 3 | (unsigned)(b1 == x) << 4 | (unsigned)(b2 == x) << 5 |
                                       (unsigned)(c0 == x) << 6 | (unsigned)(c1 == x) << 7 | (unsigned)(c2 == x) << 8 |
                                       (unsigned)(e0 == x) << 9 | (unsigned)(e1 == x) << 10 | (unsigned)(e2 == x) << 11 |
                                       (unsigned)(s[j - 1] == x) << 12;
                    unsigned nv, ne;
                    count_cells(m, nv, ne);
                    r.c[0] += nv; r.c[1] += ne;
                    r.f[0] += (unsigned)(b1 != x) + (unsigned)(S[LW * LD + j] != x);
                    r.f[1] += (unsigned)(e1 != x) + (unsigned)(S[LD + j] != x);
                    r.f[2] += (unsigned)(s[j - 1] != x) + (unsigned)(s[j + 1] != x);
                    const unsigned ud = (unsigned)(dbase + j - 1);
                    ++r.cnt; r.sd += ud; r.sdd += (u64)(ud * ud);              // d <= 65534: d * d fits 32 bits
                }
                a0 = a1; a1 = a2; b0 = b1; b1 = b2; c0 = c1; c1 = c2; e0 = e1; e1 = e2;
            }
            if (r.lab) flush_run(r, uh, uw, st, o);
        }
    }
    __syncthreads();
    if (tid < SHP_SLOTS && st.key[tid] != 0) sums_to_global<unsigned>(o, st.key[tid] - 1, st.m[tid], st.f[tid], st.c[tid]);
}

// ---------------------------------------------------------------------------------------------------- axes
// |v| < 2^127 as a correctly rounded float64: the top 64 bits with the rest folded into the lowest one (far below the
// rounding position of a 53-bit significand), one hardware conversion, one exact scaling
MIVP_DEV double i128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    const u64 hi = (u64)(u >> 64), lo = (u64)u;
    double d;
    if (hi == 0ull) {
        d = (double)lo;
    } else {
        const int k = __clzll((long long)hi);                  // 0..63
        u64 top = k ? (hi << k) | (lo >> (64 - k)) : hi;
        if ((k ? (lo << k) : lo) != 0ull) top |= 1ull;
        d = ldexp((double)top, 64 - k);
    }
    return neg ? -d : d;
}

// rotation that zeroes a[p][q] of the symmetric 3x3 matrix (r is the third index); v accumulates the eigenvectors as columns
MIVP_DEV void jacobi_rotate(double (&a)[3][3], double (&v)[3][3], int p, int q, int r) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[p][p] -= t * apq;
    a[q][q] += t * apq;
    a[p][q] = a[q][p] = 0.0;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = c * arp - s * arq;
    a[r][q] = a[q][r] = s * arp + c * arq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vip = v[i][p], viq = v[i][q];
        v[i][p] = c * vip - s * viq;
        v[i][q] = s * vip + c * viq;
    }
}

__global__ __launch_bounds__(TPB) void k_rs_axes(const long long* __restrict__ size, const long long* __restrict__ csum,
                                                 const long long* __restrict__ mom, int cap, double sh, double sw, double sd,
                                                 double* __restrict__ cov, double* __restrict__ eig, double* __restrict__ axes) {
    const int r = blockIdx.x * TPB + threadIdx.x;
    if (r >= cap) return;
    const long long n = size[r];
    double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double lam[3] = {0.0, 0.0, 0.0};
    if (n <= 0) {
        for (int i = 0; i < 9; ++i) { cov[(long)r * 9 + i] = 0.0; axes[(long)r * 9 + i] = 0.0; }
        for (int i = 0; i < 3; ++i) eig[(long)r * 3 + i] = 0.0;
        return;
    }
    const double sp[3] = {sh, sw, sd};
    const double nn = (double)n * (double)n;
    const int ia[6] = {0, 1, 2, 0, 0, 1}, ib[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const __int128 num = (__int128)n * (__int128)mom[(long)r * 6 + k] -
                             (__int128)csum[(long)r * 3 + ia[k]] * (__int128)csum[(long)r * 3 + ib[k]];
        const double c = i128_to_double(num) / nn * (sp[ia[k]] * sp[ib[k]]);
        a[ia[k]][ib[k]] = c;
        a[ib[k]][ia[k]] = c;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) cov[(long)r * 9 + i * 3 + j] = a[i][j];
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
        jacobi_rotate(a, v, 0, 1, 2);
        jacobi_rotate(a, v, 0, 2, 1);
        jacobi_rotate(a, v, 1, 2, 0);
    }
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i) lam[i] = a[i][i] > 0.0 ? a[i][i] : 0.0;
    // descending, by a fixed network; equal values keep their axis order
#define MIVP_RS_SWAP(x, y) if (lam[ord[x]] < lam[ord[y]]) { const int t_ = ord[x]; ord[x] = ord[y]; ord[y] = t_; }
    MIVP_RS_SWAP(0, 1) MIVP_RS_SWAP(1, 2) MIVP_RS_SWAP(0, 1)
#undef MIVP_RS_SWAP
    for (int i = 0; i < 3; ++i) {
        const int col = ord[i];
        double e[3] = {v[0][col], v[1][col], v[2][col]};
        int big = 0;
        if (fabs(e[1]) > fabs(e[big])) big = 1;
        if (fabs(e[2]) > fabs(e[big])) big = 2;
        const double sg = e[big] < 0.0 ? -1.0 : 1.0;
        eig[(long)r * 3 + i] = lam[col];
        for (int j = 0; j < 3; ++j) axes[(long)r * 9 + i * 3 + j] = sg * e[j] + 0.0;       // (+ 0.0: no negative zeros)
    }
}
}  // namespace

extern "C" int mivp_region_shape(const int32_t* labels, const int32_t* dims, int32_t capacity, int64_t* moment2,
                                 int64_t* faces, int64_t* cells, mivp_stream_t stream) {
    MIVP_REQUIRE(labels && dims && moment2 && faces && cells && capacity >= 1);
    Dims g;
    MIVP_REQUIRE(fill_dims(dims, g));
    hipStream_t st = (hipStream_t)stream;
    const ShapeOut o{(u64*)moment2, (u64*)faces, (u64*)cells, (int)capacity};
    const long zb = ((long)capacity * 6 + TPB - 1) / TPB;
    hipLaunchKernelGGL(k_rs_zero, dim3((unsigned)(zb > 1024 ? 1024 : zb)), dim3(TPB), 0, st, o);
    const long nbh = (g.H + BH - 1) / BH, nbw = (g.W + BW - 1) / BW, nbd = (g.D + BD - 1) / BD;
    const long bricks = nbh * nbw * nbd;                       // at most 2^31 / 64 + the ragged ones: far below 2^31
    MIVP_REQUIRE(bricks < (1L << 31));
    hipLaunchKernelGGL(k_rs_shape, dim3((unsigned)bricks), dim3(TPB), 0, st, (const int*)labels, g, (int)nbw, (int)nbd, o);
    return mivp_check_launch("region_shape");
}

extern "C" int mivp_region_axes(const int64_t* size, const int64_t* coord_sum, const int64_t* moment2, int32_t capacity,
                                double sh, double sw, double sd, void* covariance, void* eigenvalues, void* axes,
                                mivp_stream_t stream) {
    MIVP_REQUIRE(size && coord_sum && moment2 && covariance && eigenvalues && axes && capacity >= 1);
    MIVP_REQUIRE(sh > 0.0 && sw > 0.0 && sd > 0.0 && sh < 1e30 && sw < 1e30 && sd < 1e30);
    MIVP_REQUIRE((((uintptr_t)covariance | (uintptr_t)eigenvalues | (uintptr_t)axes) & 7u) == 0);
    hipLaunchKernelGGL(k_rs_axes, dim3((unsigned)((capacity + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream,
                       (const long long*)size, (const long long*)coord_sum, (const long long*)moment2, (int)capacity, sh, sw,
                       sd, (double*)covariance, (double*)eigenvalues, (double*)axes);
    return mivp_check_launch("region_axes");
}
