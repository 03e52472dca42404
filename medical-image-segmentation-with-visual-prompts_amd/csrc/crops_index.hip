// Class-balanced crop centres for the batch filler (mivp_amd/batches.py): the centre of a crop is the rank-th
// voxel, in C order of the stored [H][W][D] label map, of a chosen class of a chosen volume -- MONAI's
// RandCropByPosNegLabeld / RandCropByLabelClassesd -- resolved on the device from a small per-volume index, so that the
// step reads nothing back and records into a graph.
//
//   class of a voxel:  c = lut[lab]; the voxel belongs to class c if c < num_classes, otherwise to no class
//   index of a volume: int32 [num_classes][nchunks + 1], the exclusive prefix sums of the per-chunk class counts (a chunk
//                      is 1024 consecutive voxels); the last column is the class total
//   pick of a sample:  (cls, rank) -> the chunk j with prefix[cls][j] <= rank < prefix[cls][j + 1] by binary search, then
//                      the (rank - prefix[cls][j])-th match inside that chunk
//
// Lane-to-voxel map, common to the count and the pick: lane t of the 256 holds voxels 1024 j + 4 t .. + 3, one aligned
// dword of four labels; a lane whose four voxels are not all inside the volume (the tail of the last chunk) and a label map
// that is not dword-aligned go byte by byte.  Integers only: counts are wave ballots and popcounts, added in a fixed order.
// The pick writes the crop origin -- correct_crop_centers: clamp(r - roi / 2, 0, max(n_rot - roi, 0)) -- into words 2..4 of
// the sample's slot record with a plain store from the one lane that holds the voxel; k_crop (crops.hip) reads it from
// there.  Anything invalid in the record or the pick makes the workgroup return without writing.  k_crop_pick keeps its own
// decode and turn (see there); the small definitions and the host checks are crops_common.hpp's.
#include "crops_common.hpp"

namespace {
constexpr int CHUNK = 1024;              // = 4 * TPB (batches.ClassIndex.CHUNK)
constexpr int MAXCLS = 16;
constexpr uint32_t NONE4 = 0xFFFFFFFFu;  // four voxels of no class

// the classes of lane `tid`'s four voxels of the chunk that starts at q0 - 4 tid, one byte each, 0xFF = no class / outside
MIVP_DEV uint32_t lane_classes(const uint8_t* __restrict__ lab, uint32_t n, uint32_t q0, bool aligned,
                               const uint8_t* s_lut, int nc) {
    if (q0 >= n) return NONE4;
    const uint32_t nv = min(4u, n - q0);
    uint32_t raw = 0;
    if (aligned && nv == 4) {
        raw = *reinterpret_cast<const uint32_t*>(lab + q0);
    } else {
        for (uint32_t k = 0; k < nv; ++k) raw |= (uint32_t)lab[q0 + k] << (8 * k);
    }
    uint32_t out = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t c = s_lut[(raw >> (8 * k)) & 255u];
        out |= ((k < nv && c < (uint32_t)nc) ? c : 255u) << (8 * k);
    }
    return out;
}

// how many of the four bytes of `cls4` equal c, as a 4-bit mask of the matching voxels
MIVP_DEV uint32_t match_mask(uint32_t cls4, uint32_t c) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) m |= (uint32_t)(((cls4 >> (8 * k)) & 255u) == c) << k;
    return m;
}

// ---------------------------------------------------------------------------------------------------------------------
// count: workgroup j writes the class counts of chunk j into column j of the index (raw counts; k_label_scan turns the
// rows into prefix sums in place)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_label_count(const uint8_t* __restrict__ lab, uint32_t n,
                                                     const uint8_t* __restrict__ lut, int nc, int32_t* __restrict__ index,
                                                     int nch) {
    __shared__ uint8_t s_lut[256];
    __shared__ int s_w[TPB / 64][MAXCLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    load_lut(s_lut, lut);
    const uint32_t j = blockIdx.x;
    const uint32_t cls4 = lane_classes(lab, n, j * (uint32_t)CHUNK + 4u * tid, ((uintptr_t)lab & 3) == 0, s_lut, nc);
    for (int c = 0; c < nc; ++c) {
        int cnt = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) cnt += __popcll(__ballot(((cls4 >> (8 * k)) & 255u) == (uint32_t)c));
        if (lane == 0) s_w[wave][c] = cnt;
    }
    __syncthreads();
    if (tid < nc) index[(long)tid * (nch + 1) + j] = s_w[0][tid] + s_w[1][tid] + s_w[2][tid] + s_w[3][tid];
}

// scan: workgroup c turns row c -- nch counts, then one unused word -- into nch + 1 exclusive prefix sums, in place, tile by
// tile of 256 in ascending order (a thread reads its element before any thread of the tile writes)
__global__ __launch_bounds__(TPB) void k_label_scan(int32_t* __restrict__ index, int nch) {
    __shared__ int s_w[TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t* row = index + (long)blockIdx.x * (nch + 1);
    int carry = 0;
    for (int base = 0; base <= nch; base += TPB) {
        const int i = base + tid;
        const int v = i < nch ? row[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TPB / 64; ++w) {
            before += w < wave ? s_w[w] : 0;
            total += s_w[w];
        }
        if (i <= nch) row[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// pick: one workgroup per sample
// ---------------------------------------------------------------------------------------------------------------------
struct PickArgs {
    const int64_t* table;    // the bank's source table [n_volumes][5]
    const int64_t* itable;   // the index table [n_volumes][2] = (prefix pointer or 0, nchunks)
    int n_volumes, nc, B;
    const uint8_t* lut;
    int32_t* slot;
    int slot_stride;
    const int32_t* pick;     // [B][2] = (cls, rank)
    int h, w, d;             // roi
};

MIVP_DEV int crop_origin(int r, int roi, int m) { return min(max(r - (roi >> 1), 0), max(m - roi, 0)); }

__global__ __launch_bounds__(TPB) void k_crop_pick(PickArgs a) {
    __shared__ uint8_t s_lut[256];
    __shared__ int s_w[TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    int32_t* rec = a.slot + (long)b * a.slot_stride;
    const int vol = rec[0], code = rec[1];
    const int cls = a.pick[2 * b], rank = a.pick[2 * b + 1];
    if ((unsigned)vol >= (unsigned)a.n_volumes || (unsigned)code > 3u || (unsigned)cls >= (unsigned)a.nc) return;
    const int64_t* irow = a.itable + (long)vol * 2;
    const int32_t* prefix = reinterpret_cast<const int32_t*>(irow[0]);
    const int nch = (int)irow[1];
    if (!prefix) return;                                                 // a volume that is not indexed (yet)
    const int64_t* row = a.table + (long)vol * 5;
    const uint8_t* lab = reinterpret_cast<const uint8_t*>(row[1]);
    const int n0 = (int)row[2], n1 = (int)row[3], n2 = (int)row[4];
    if (!lab || n0 < 1 || n1 < 1 || n2 < 1) return;
    const uint32_t n = (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2;       // below 2^31 (the bank refuses more)
    if (nch < 1 || (uint32_t)nch != (n + CHUNK - 1) / CHUNK) return;     // an index of another volume: never follow it
    const int32_t* pre = prefix + (long)cls * (nch + 1);
    if ((unsigned)rank >= (unsigned)pre[nch]) return;
    // the chunk: the largest j in [0, nch) with pre[j] <= rank (pre[0] = 0 <= rank < pre[nch]); uniform, about log2(nch) loads
    int lo = 0, hi = nch;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] <= rank) lo = mid; else hi = mid;
    }
    const int target = rank - pre[lo];                                   // the target-th match of chunk lo

    load_lut(s_lut, a.lut);
    const uint32_t q0 = (uint32_t)lo * (uint32_t)CHUNK + 4u * tid;
    const uint32_t m = match_mask(lane_classes(lab, n, q0, ((uintptr_t)lab & 3) == 0, s_lut, a.nc), (uint32_t)cls);
    const int cnt = __popc(m);                                           // 0..4: three bits
    // matches in the lanes below this one: a ballot per bit of the count
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long b0 = __ballot(cnt & 1), b1 = __ballot(cnt & 2), b2 = __ballot(cnt & 4);
    int before = __popcll(b0 & below) + 2 * __popcll(b1 & below) + 4 * __popcll(b2 & below);
    if (lane == 0) s_w[wave] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TPB / 64; ++w) before += w < wave ? s_w[w] : 0;
    int t = target - before;
    if (t < 0 || t >= cnt) return;                                       // one lane at most holds the target
    uint32_t k = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if ((m >> i) & 1u) {
            if (t == 0) k = i;
            --t;
        }
    }
    const uint32_t q = q0 + k, plane = (uint32_t)n1 * (uint32_t)n2;
    const int p0 = (int)(q / plane);
    const uint32_t rem = q - (uint32_t)p0 * plane;
    const int p1 = (int)(rem / (uint32_t)n2), p2 = (int)(rem - (uint32_t)p1 * (uint32_t)n2);
    // p (stored frame) -> r (rotated frame) with the rotated extents, in one switch: to_rotated and rotate_extents of
    // crops_common.hpp written out, like the decode above with its own read order (the index row first) -- through the
    // shared functions this kernel's assembly changes (profiles/README.md)
    int r0 = p0, r1 = p1, r2 = p2, m0 = n0, m1 = n1, m2 = n2;
    switch (code) {
        case 1: r0 = n1 - 1 - p1; r1 = p0; m0 = n1; m1 = n0; break;
        case 2: r0 = n2 - 1 - p2; r2 = p0; m0 = n2; m2 = n0; break;
        case 3: r1 = n2 - 1 - p2; r2 = p1; m1 = n2; m2 = n1; break;
        default: break;
    }
    rec[2] = crop_origin(r0, a.h, m0);
    rec[3] = crop_origin(r1, a.w, m1);
    rec[4] = crop_origin(r2, a.d, m2);
}
}  // namespace

extern "C" int mivp_label_index_build(const uint8_t* labels, int64_t numel, const uint8_t* lut, int32_t num_classes,
                                      int32_t* index, int32_t nchunks, mivp_stream_t stream) {
    MIVP_REQUIRE(labels && lut && index && ((uintptr_t)index & 3) == 0);
    MIVP_REQUIRE(numel >= 1 && numel < (1L << 31) && num_classes >= 1 && num_classes <= MAXCLS);
    MIVP_REQUIRE(nchunks >= 1 && (int64_t)nchunks == (numel + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(k_label_count, dim3((unsigned)nchunks), dim3(TPB), 0, (hipStream_t)stream, labels, (uint32_t)numel,
                       lut, num_classes, index, nchunks);
    const int rc = mivp_check_launch("label_index_build (count)");
    if (rc) return rc;
    hipLaunchKernelGGL(k_label_scan, dim3((unsigned)num_classes), dim3(TPB), 0, (hipStream_t)stream, index, nchunks);
    return mivp_check_launch("label_index_build (scan)");
}

extern "C" int mivp_crop_pick(const int64_t* table, const int64_t* index_table, int32_t n_volumes, const uint8_t* lut,
                              int32_t num_classes, int32_t* slot, int32_t slot_stride, const int32_t* pick, int32_t B,
                              const int32_t* roi, mivp_stream_t stream) {
    const int rc = check_bank_args(table, n_volumes, slot, slot_stride, B, roi);
    if (rc) return rc;
    MIVP_REQUIRE(index_table && lut && pick && ((uintptr_t)index_table & 7) == 0 && ((uintptr_t)pick & 3) == 0);
    MIVP_REQUIRE(num_classes >= 1 && num_classes <= MAXCLS);
    PickArgs a{};
    a.table = table; a.itable = index_table; a.n_volumes = n_volumes; a.nc = num_classes; a.B = B;
    a.lut = lut; a.slot = slot; a.slot_stride = slot_stride; a.pick = pick;
    a.h = roi[0]; a.w = roi[1]; a.d = roi[2];
    hipLaunchKernelGGL(k_crop_pick, dim3((unsigned)B), dim3(TPB), 0, (hipStream_t)stream, a);
    return mivp_check_launch("crop_pick");
}
