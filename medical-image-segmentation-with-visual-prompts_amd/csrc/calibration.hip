// Calibration and threshold-sweep tables of a probability volume (joined ABI 18, mivp_amd/calibration.py).
//
// probs is fp32 [C][V] (V = H * W * D voxels, one plane per class), target a class map of V values.  Nothing here depends
// on a voxel's coordinates, so the volume is walked flat: an item is four consecutive voxels, one lane takes one item per
// trip and every workgroup makes the same number of trips (the cross-lane steps below need whole waves).
//   load      C 16-byte loads, a plane stride apart, and one vector load of the four reference values, when V is a
//             multiple of 4 and both pointers are 16-byte aligned; else the planes start unaligned and every value is its
//             own load.  The volume is read once.
//   classify  a voxel is valid when each of its C probabilities is in [0, 1] (a NaN is not) and its reference value is a
//             class; q = rint(p * 2^20) (the product is exact, v_rndne rounds half to even), bin = min(B - 1, q * B >> 20).
//   count     C + 1 rows (one-vs-rest, then top-label) of B cells (count | pos << 32, qsum) live in the workgroup's LDS as
//             64-bit words; a workgroup counts fewer than 2^31 voxels, so neither half of the packed word can carry.  A lane
//             whose four voxels share a bin adds once, and then every lane adds for itself: measured faster than COMBINE
//             on a spread and on a saturated field alike, so that is the default.  COMBINE (flags bit 0): the
//             lanes of a wave that hit the cell of the first active lane are summed with six shuffle steps and that lane
//             adds for all of them, twice over, and only when at least COMBINE_MIN lanes agree; what is left adds for
//             itself.
//   totals    n_pos and the two halves of the squared error are 32-bit lane registers, summed over the wave and added to
//             LDS every FLUSH_TRIPS trips (1024 voxels of at most 2^20 each stay below 2^32).
//   merge     one 64-bit global atomic add per (workgroup, non-empty cell and table): integers, so the order of arrival
//             does not matter and the tables are bitwise reproducible.
// Above LDS_CELLS cells ((C + 1) * B > 3072: 48 KiB of LDS) the cells are added in global memory directly, with the same
// combining.  No float atomics anywhere.
#include "common.hpp"

namespace {
constexpr int MAXC = 16;
constexpr int MAXB = 1024;
constexpr int TPB = 256;
constexpr int VPL = 4;                    // voxels per lane and trip
constexpr int QBITS = 20;
constexpr int Q = 1 << QBITS;
constexpr int LDS_CELLS = 3072;           // cells a workgroup keeps in LDS (16 bytes each)
constexpr int COMBINE_MIN = 8;            // lanes that must share a cell before a wave sums them
constexpr int FLUSH_TRIPS = 256;
constexpr unsigned GRID_CAP = 1024;
typedef unsigned long long u64;

// row totals in LDS: [row][n_pos, sq_hi, sq_lo], then n, n_ignored, n_invalid
constexpr int TOT_ROW = 3;
constexpr int TOT_WORDS = (MAXC + 1) * TOT_ROW + 3;

struct Tables {                           // views into the caller's int64 block (mivp_calibration_ws)
    u64* count; u64* pos; u64* qsum;      // [R][B]
    u64* n; u64* n_pos; u64* sq_hi; u64* sq_lo;   // [R]
    u64* misc;                            // n_ignored, n_invalid
};
size_t table_words(int C, int B) { return (size_t)3 * (C + 1) * B + (size_t)4 * (C + 1) + 2; }
Tables view(int64_t* t, int C, int B) {
    const long R = C + 1, RB = R * B;
    u64* p = (u64*)t;
    return Tables{p, p + RB, p + 2 * RB, p + 3 * RB, p + 3 * RB + R, p + 3 * RB + 2 * R, p + 3 * RB + 3 * R,
                  p + 3 * RB + 4 * R};
}

struct Cells {
    u64* cp; u64* qs;                     // LDS (nullptr: the global tables take every add)
    Tables g;
};

MIVP_DEV unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}
MIVP_DEV u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (u64)__shfl_xor((long long)v, o);
    return v;
}

MIVP_DEV void add(const Cells& cx, int cell, unsigned cnt, unsigned ps, unsigned qs) {
    if (cx.cp) {
        atomicAdd(cx.cp + cell, (u64)cnt | ((u64)ps << 32));
        if (qs) atomicAdd(cx.qs + cell, (u64)qs);
    } else {
        atomicAdd(cx.g.count + cell, (u64)cnt);
        if (ps) atomicAdd(cx.g.pos + cell, (u64)ps);
        if (qs) atomicAdd(cx.g.qsum + cell, (u64)qs);
    }
}

// every lane of the wave calls this; `active` lanes add (cnt voxels, ps of them positive, qs their summed q) to `cell`
template <bool COMBINE>
MIVP_DEV void add_cell(const Cells& cx, bool active, int cell, unsigned cnt, unsigned ps, unsigned qs) {
    if (COMBINE) {
        const int lane = (int)(threadIdx.x & 63u);
        u64 todo = __ballot(active);
#pragma unroll
        for (int round = 0; round < 2; ++round) {
            if (todo == 0ull) break;
            const int leader = __ffsll((long long)todo) - 1;
            const int kl = __shfl(cell, leader);
            const bool mine = active && cell == kl;
            const u64 same = __ballot(mine);
            if (__popcll(same) < COMBINE_MIN) break;
            const unsigned w = wave_sum(mine ? (cnt | (ps << 16)) : 0u);      // at most 64 * 4 of each: 16 bits hold them
            const unsigned s = wave_sum(mine ? qs : 0u);                      // at most 2^28
            if (lane == leader) add(cx, kl, w & 0xFFFFu, w >> 16, s);
            todo &= ~same;
            active = active && !mine;
        }
    }
    if (active) add(cx, cell, cnt, ps, qs);
}

struct RowAcc { unsigned n_pos, sq_hi, sq_lo; };

// one row of one item: q, y of the four voxels (bit j of ok: voxel j counts)
template <bool COMBINE>
MIVP_DEV void row_add(const Cells& cx, int rowbase, int B, const int (&q)[VPL], unsigned ymask, unsigned ok, RowAcc& acc) {
    int b[VPL];
    int bf = -1;
    bool uni = true;
    unsigned cnt = 0u, ps = 0u, qs = 0u;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        b[j] = min(B - 1, (q[j] * B) >> QBITS);
        if ((ok >> j) & 1u) {
            const unsigned y = (ymask >> j) & 1u;
            const unsigned e = y ? (unsigned)(Q - q[j]) : (unsigned)q[j];
            const u64 e2 = (u64)e * e;
            acc.sq_hi += (unsigned)(e2 >> QBITS);
            acc.sq_lo += (unsigned)e2 & (unsigned)(Q - 1);
            acc.n_pos += y;
            if (bf < 0) bf = b[j];
            uni = uni && b[j] == bf;
            ++cnt; ps += y; qs += (unsigned)q[j];
        }
    }
    if (__all(uni)) {
        add_cell<COMBINE>(cx, ok != 0u, rowbase + max(bf, 0), cnt, ps, qs);
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            add_cell<COMBINE>(cx, ((ok >> j) & 1u) != 0u, rowbase + b[j], 1u, (ymask >> j) & 1u, (unsigned)q[j]);
    }
}

MIVP_DEV int target_class(const void* t, int dtype, long v, int C) {
    switch (dtype) {
        case 0: return class_of<uint8_t>(((const uint8_t*)t)[v], C);
        case 1: return class_of<int32_t>(((const int32_t*)t)[v], C);
        case 2: return class_of<int64_t>(((const int64_t*)t)[v], C);
        default: return class_of<float>(((const float*)t)[v], C);
    }
}

// the four reference classes of an aligned item
MIVP_DEV void target_class4(const void* t, int dtype, long v0, int C, int (&cls)[VPL]) {
    switch (dtype) {
        case 0: {
            const uchar4 a = *reinterpret_cast<const uchar4*>((const uint8_t*)t + v0);
            cls[0] = class_of<uint8_t>(a.x, C); cls[1] = class_of<uint8_t>(a.y, C);
            cls[2] = class_of<uint8_t>(a.z, C); cls[3] = class_of<uint8_t>(a.w, C);
            break;
        }
        case 1: {
            const int4 a = *reinterpret_cast<const int4*>((const int32_t*)t + v0);
            cls[0] = class_of<int32_t>(a.x, C); cls[1] = class_of<int32_t>(a.y, C);
            cls[2] = class_of<int32_t>(a.z, C); cls[3] = class_of<int32_t>(a.w, C);
            break;
        }
        case 2: {
            const longlong2 a = *reinterpret_cast<const longlong2*>((const int64_t*)t + v0);
            const longlong2 c = *reinterpret_cast<const longlong2*>((const int64_t*)t + v0 + 2);
            cls[0] = class_of<int64_t>(a.x, C); cls[1] = class_of<int64_t>(a.y, C);
            cls[2] = class_of<int64_t>(c.x, C); cls[3] = class_of<int64_t>(c.y, C);
            break;
        }
        default: {
            const float4 a = *reinterpret_cast<const float4*>((const float*)t + v0);
            cls[0] = class_of<float>(a.x, C); cls[1] = class_of<float>(a.y, C);
            cls[2] = class_of<float>(a.z, C); cls[3] = class_of<float>(a.w, C);
            break;
        }
    }
}

// CT: the number of class planes held in registers (C <= CT); vec: 16-byte loads (V % 4 == 0, aligned pointers)
template <int CT, bool COMBINE>
__global__ __launch_bounds__(TPB) void k_cal_hist(const float* __restrict__ probs, const void* __restrict__ target,
                                                  int dtype, long V, int C, int B, int vec, int lds_cells, Tables g) {
    extern __shared__ u64 cells[];                 // cp [lds_cells], qs [lds_cells]
    __shared__ u64 tot[TOT_WORDS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int ncell = (C + 1) * B;
    for (int i = tid; i < 2 * lds_cells; i += TPB) cells[i] = 0ull;
    if (tid < TOT_WORDS) tot[tid] = 0ull;
    __syncthreads();
    Cells cx;
    cx.cp = lds_cells ? cells : nullptr;
    cx.qs = cells + lds_cells;
    cx.g = g;

    RowAcc acc[CT], top;
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = RowAcc{0u, 0u, 0u};
    top = RowAcc{0u, 0u, 0u};
    unsigned nvalid = 0u, nign = 0u, ninv = 0u;
    int trips = 0;

    auto flush_totals = [&]() {                   // whole waves: called at trip counts every lane of the workgroup shares
#pragma unroll
        for (int c = 0; c <= CT; ++c) {
            if (c < CT && c >= C) continue;
            RowAcc& a = c < CT ? acc[c < CT ? c : 0] : top;
            const int r = c < CT ? c : C;
            const u64 np = wave_sum((u64)a.n_pos), hi = wave_sum((u64)a.sq_hi), lo = wave_sum((u64)a.sq_lo);
            if (lane == 0) {
                if (np) atomicAdd(&tot[r * TOT_ROW + 0], np);
                if (hi) atomicAdd(&tot[r * TOT_ROW + 1], hi);
                if (lo) atomicAdd(&tot[r * TOT_ROW + 2], lo);
            }
            a = RowAcc{0u, 0u, 0u};
        }
        const u64 nv = wave_sum((u64)nvalid), ni = wave_sum((u64)nign), nb = wave_sum((u64)ninv);
        if (lane == 0) {
            if (nv) atomicAdd(&tot[(MAXC + 1) * TOT_ROW + 0], nv);
            if (ni) atomicAdd(&tot[(MAXC + 1) * TOT_ROW + 1], ni);
            if (nb) atomicAdd(&tot[(MAXC + 1) * TOT_ROW + 2], nb);
        }
        nvalid = nign = ninv = 0u;
    };

    const long items = (V + VPL - 1) / VPL;
    for (long i0 = (long)blockIdx.x * TPB; i0 < items; i0 += (long)gridDim.x * TPB) {
        const long item = i0 + tid;
        const long v0 = item * VPL;
        const int nv = item < items ? (int)min((long)VPL, V - v0) : 0;
        float p[CT][VPL];
        int cls[VPL];
        if (vec && nv == VPL) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c < C) {
                    const float4 a = *reinterpret_cast<const float4*>(probs + (long)c * V + v0);
                    p[c][0] = a.x; p[c][1] = a.y; p[c][2] = a.z; p[c][3] = a.w;
                } else {
                    p[c][0] = p[c][1] = p[c][2] = p[c][3] = 0.f;
                }
            }
            target_class4(target, dtype, v0, C, cls);
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
#pragma unroll
                for (int c = 0; c < CT; ++c) p[c][j] = (c < C && j < nv) ? probs[(long)c * V + v0 + j] : 0.f;
                cls[j] = j < nv ? target_class(target, dtype, v0 + j, C) : -1;
            }
        }
        // validity, arg-max (the lowest index among equals) and the quantised values
        unsigned ok = 0u, ytop = 0u;
        int qtop[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            bool good = true;
            float best = p[0][j];
            int arg = 0;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                if (c < C) {
                    good = good && (p[c][j] >= 0.f && p[c][j] <= 1.f);
                    if (c > 0 && p[c][j] > best) { best = p[c][j]; arg = c; }
                }
            }
            const bool in = j < nv;
            const bool valid = in && good && cls[j] >= 0;
            ninv += (in && !good) ? 1u : 0u;
            nign += (in && good && cls[j] < 0) ? 1u : 0u;
            nvalid += valid ? 1u : 0u;
            ok |= (valid ? 1u : 0u) << j;
            ytop |= ((valid && arg == cls[j]) ? 1u : 0u) << j;
            qtop[j] = valid ? (int)rintf(best * (float)Q) : 0;
            if (!valid) cls[j] = -1;
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (c < C) {                                   // uniform
                int q[VPL];
                unsigned ymask = 0u;
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    q[j] = ((ok >> j) & 1u) ? (int)rintf(p[c][j] * (float)Q) : 0;
                    ymask |= (cls[j] == c ? 1u : 0u) << j;
                }
                row_add<COMBINE>(cx, c * B, B, q, ymask, ok, acc[c]);
            }
        }
        row_add<COMBINE>(cx, C * B, B, qtop, ytop, ok, top);
        if (++trips == FLUSH_TRIPS) { flush_totals(); trips = 0; }
    }
    flush_totals();
    __syncthreads();
    // merge: one set of global atomics per non-empty cell of this workgroup
    for (int i = tid; i < (lds_cells ? ncell : 0); i += TPB) {
        const u64 cp = cx.cp[i], qs = cx.qs[i];
        if (cp) {
            atomicAdd(g.count + i, cp & 0xFFFFFFFFull);
            if (cp >> 32) atomicAdd(g.pos + i, cp >> 32);
            if (qs) atomicAdd(g.qsum + i, qs);
        }
    }
    const u64 nvt = tot[(MAXC + 1) * TOT_ROW + 0];
    if (tid <= C) {
        if (nvt) atomicAdd(g.n + tid, nvt);
        if (tot[tid * TOT_ROW + 0]) atomicAdd(g.n_pos + tid, tot[tid * TOT_ROW + 0]);
        if (tot[tid * TOT_ROW + 1]) atomicAdd(g.sq_hi + tid, tot[tid * TOT_ROW + 1]);
        if (tot[tid * TOT_ROW + 2]) atomicAdd(g.sq_lo + tid, tot[tid * TOT_ROW + 2]);
    }
    if (tid == 64) {
        if (tot[(MAXC + 1) * TOT_ROW + 1]) atomicAdd(g.misc + 0, tot[(MAXC + 1) * TOT_ROW + 1]);
        if (tot[(MAXC + 1) * TOT_ROW + 2]) atomicAdd(g.misc + 1, tot[(MAXC + 1) * TOT_ROW + 2]);
    }
}

template <int CT>
void launch(bool combine, unsigned grid, size_t lds, hipStream_t st, const float* probs, const void* target, int dtype,
            long V, int C, int B, int vec, int lds_cells, const Tables& g) {
    if (combine)
        hipLaunchKernelGGL((k_cal_hist<CT, true>), dim3(grid), dim3(TPB), lds, st, probs, target, dtype, V, C, B, vec,
                           lds_cells, g);
    else
        hipLaunchKernelGGL((k_cal_hist<CT, false>), dim3(grid), dim3(TPB), lds, st, probs, target, dtype, V, C, B, vec,
                           lds_cells, g);
}
}  // namespace

extern "C" size_t mivp_calibration_ws(int32_t C, int32_t n_bins) {
    if (C < 1 || C > MAXC || n_bins < 1 || n_bins > MAXB) return 0;
    return table_words((int)C, (int)n_bins) * 8;
}

extern "C" int mivp_calibration_hist(const float* probs, const void* target, int32_t target_dtype, const int32_t* dims,
                                     int32_t C, int32_t n_bins, int32_t flags, int64_t* tables, mivp_stream_t stream) {
    MIVP_REQUIRE(probs && target && dims && tables && target_dtype >= 0 && target_dtype <= 3);
    MIVP_REQUIRE(C >= 1 && C <= MAXC && n_bins >= 1 && n_bins <= MAXB && (flags & ~1) == 0);
    MIVP_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long)dims[0] * dims[1] * dims[2] < (1L << 31));
    MIVP_REQUIRE(((uintptr_t)probs & 3u) == 0 && ((uintptr_t)tables & 7u) == 0);
    const int tsize = target_dtype == 0 ? 1 : target_dtype == 2 ? 8 : 4;
    MIVP_REQUIRE(((uintptr_t)target & (uintptr_t)(tsize - 1)) == 0);
    const long V = (long)dims[0] * dims[1] * dims[2];
    const int vec = (V % VPL == 0 && (((uintptr_t)probs | (uintptr_t)target) & 15u) == 0) ? 1 : 0;
    const int ncell = ((int)C + 1) * (int)n_bins;
    const int lds_cells = ncell <= LDS_CELLS ? ncell : 0;
    const long items = (V + VPL - 1) / VPL;
    const long want = (items + TPB - 1) / TPB;
    const unsigned grid = (unsigned)(want > GRID_CAP ? GRID_CAP : want);
    const size_t lds = (size_t)2 * lds_cells * sizeof(u64);
    const Tables g = view(tables, (int)C, (int)n_bins);
    const bool combine = (flags & 1) != 0;
    hipStream_t st = (hipStream_t)stream;
    if (C <= 2) launch<2>(combine, grid, lds, st, probs, target, (int)target_dtype, V, (int)C, (int)n_bins, vec, lds_cells, g);
    else if (C <= 4) launch<4>(combine, grid, lds, st, probs, target, (int)target_dtype, V, (int)C, (int)n_bins, vec, lds_cells, g);
    else if (C <= 8) launch<8>(combine, grid, lds, st, probs, target, (int)target_dtype, V, (int)C, (int)n_bins, vec, lds_cells, g);
    else launch<16>(combine, grid, lds, st, probs, target, (int)target_dtype, V, (int)C, (int)n_bins, vec, lds_cells, g);
    return mivp_check_launch("calibration_hist");
}
