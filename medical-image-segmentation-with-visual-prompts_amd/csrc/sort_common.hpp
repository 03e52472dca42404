// Device-wide exact sort of 32-bit keys by segments: a keys-only LSD radix sort, four passes of 8 bits.  Used by
// csrc/lovasz.hip, which also exports it as mivp_sort_u32.
//
// keys u32 [S][n]: S segments of one length, each sorted ascending on its own.  A pass has three launches whatever S, n and the
// data are, the segment being grid dimension y:
//   histogram   one workgroup per tile of SORT_TILE keys: the count of each digit in the tile (LDS integer atomics: a count
//               does not depend on their order) -> hist [S][nblk][256]
//   scan        one workgroup per segment, thread d owns digit d: the exclusive running count of d over the tiles in tile
//               order (in place), then the exclusive scan of the digit totals -> base [S][256]
//   scatter     one workgroup per tile.  A tile is read in rounds of 256 keys (round r, thread t: key r 256 + t of the tile), so
//               a key's place in its tile is (round, wave, lane).  Per round every lane finds the lanes of its wave that hold
//               its digit (8 ballots), its rank among them, and the wave's count of the digit; the counts of the earlier
//               waves and rounds come from LDS.  A key lands at base[d] + hist[tile][d] + its rank among the tile's keys of
//               digit d: keys of one digit keep their order inside a tile and across tiles, which the later passes rely on.
// No float arithmetic, no global atomics: equal input gives equal output.  The passes alternate between keys and alt and end
// in keys.  Limits: S <= 65535, S n < 2^31.
#pragma once
#include "common.hpp"

namespace {
constexpr int SORT_TPB = 256, SORT_IPT = 16, SORT_TILE = SORT_TPB * SORT_IPT, SORT_RADIX = 256;

inline long sort_nblk(int64_t n) { return (n + SORT_TILE - 1) / SORT_TILE; }
inline size_t sort_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

__global__ __launch_bounds__(SORT_TPB) void k_sort_hist(const uint32_t* __restrict__ keys, long n, int shift, int nblk,
                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[SORT_RADIX];
    const int seg = blockIdx.y, blk = blockIdx.x;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t* k = keys + (long)seg * n;
    const long first = (long)blk * SORT_TILE;
#pragma unroll
    for (int r = 0; r < SORT_IPT; ++r) {
        const long i = first + r * SORT_TPB + threadIdx.x;
        if (i < n) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[((long)seg * nblk + blk) * SORT_RADIX + threadIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(SORT_TPB) void k_sort_scan(uint32_t* __restrict__ hist, int nblk, uint32_t* __restrict__ base) {
    __shared__ uint32_t tot[SORT_RADIX];
    const int seg = blockIdx.x, d = threadIdx.x;
    uint32_t* col = hist + (long)seg * nblk * SORT_RADIX + d;
    uint32_t run = 0u;
    int blk = 0;
    for (; blk + 8 <= nblk; blk += 8) {                       // eight loads in flight, then their running counts
        uint32_t t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = col[(long)(blk + u) * SORT_RADIX];
#pragma unroll
        for (int u = 0; u < 8; ++u) { col[(long)(blk + u) * SORT_RADIX] = run; run += t[u]; }
    }
    for (; blk < nblk; ++blk) {
        const uint32_t t = col[(long)blk * SORT_RADIX];
        col[(long)blk * SORT_RADIX] = run;
        run += t;
    }
    tot[d] = run;
    __syncthreads();
    for (int o = 1; o < SORT_RADIX; o <<= 1) {                // inclusive scan of the digit totals
        const uint32_t add = d >= o ? tot[d - o] : 0u;
        __syncthreads();
        tot[d] += add;
        __syncthreads();
    }
    base[seg * SORT_RADIX + d] = tot[d] - run;
}

__global__ __launch_bounds__(SORT_TPB) void k_sort_scatter(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, long n,
                                                           int shift, int nblk, const uint32_t* __restrict__ hist,
                                                           const uint32_t* __restrict__ base) {
    __shared__ uint32_t run[SORT_RADIX];                      // where the next key of digit d of this tile goes
    __shared__ uint32_t wc[SORT_TPB / 64][SORT_RADIX];        // this round's count of digit d in wave w
    const int seg = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* k = in + (long)seg * n;
    uint32_t* o = out + (long)seg * n;
    const long first = (long)blk * SORT_TILE;
    run[tid] = base[seg * SORT_RADIX + tid] + hist[((long)seg * nblk + blk) * SORT_RADIX + tid];
    for (int r = 0; r < SORT_IPT; ++r) {
#pragma unroll
        for (int w = 0; w < SORT_TPB / 64; ++w) wc[w][tid] = 0u;
        __syncthreads();
        const long i = first + r * SORT_TPB + tid;
        const bool live = i < n;
        const uint32_t key = live ? k[i] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        unsigned long long peers = __ballot(live);            // the live lanes of this wave that hold digit d
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const unsigned long long below = peers & ((1ull << lane) - 1ull);
        if (live && below == 0ull) wc[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (live) {
            uint32_t at = run[d] + (uint32_t)__popcll(below);
            for (int w = 0; w < wave; ++w) at += wc[w][d];
            if (at < (uint64_t)n) o[at] = key;                // always true: hist counted these very keys
        }
        __syncthreads();
        run[tid] += (wc[0][tid] + wc[1][tid]) + (wc[2][tid] + wc[3][tid]);
    }
}

// bytes behind the keys: alt [S n] | hist [S][nblk][256] | base [S][256], each part 256-byte aligned
struct SortWs {
    size_t alt, hist, base, total;
    SortWs(long S, int64_t n) {
        alt = 0;
        hist = alt + sort_align((size_t)S * n * sizeof(uint32_t));
        base = hist + sort_align((size_t)S * sort_nblk(n) * SORT_RADIX * sizeof(uint32_t));
        total = base + sort_align((size_t)S * SORT_RADIX * sizeof(uint32_t));
    }
};

inline bool sort_fits(long S, int64_t n) { return S >= 1 && S <= 65535 && n >= 1 && n < (1L << 31) && S * n < (1L << 31); }

// twelve launches; the sorted keys end in `keys`
inline int sort_u32_run(uint32_t* keys, int S, int64_t n, char* ws, hipStream_t st) {
    const SortWs w(S, n);
    uint32_t* alt = (uint32_t*)(ws + w.alt);
    uint32_t* hist = (uint32_t*)(ws + w.hist);
    uint32_t* base = (uint32_t*)(ws + w.base);
    const int nblk = (int)sort_nblk(n);
    const dim3 grid((unsigned)nblk, (unsigned)S);
    for (int pass = 0; pass < 4; ++pass) {
        const uint32_t* src = pass & 1 ? alt : keys;
        uint32_t* dst = pass & 1 ? keys : alt;
        hipLaunchKernelGGL(k_sort_hist, grid, dim3(SORT_TPB), 0, st, src, (long)n, 8 * pass, nblk, hist);
        hipLaunchKernelGGL(k_sort_scan, dim3((unsigned)S), dim3(SORT_TPB), 0, st, hist, nblk, base);
        hipLaunchKernelGGL(k_sort_scatter, grid, dim3(SORT_TPB), 0, st, src, dst, (long)n, 8 * pass, nblk, hist, base);
        const int rc = mivp_check_launch("sort_u32");
        if (rc != MIVP_OK) return rc;
    }
    return MIVP_OK;
}
}  // namespace
