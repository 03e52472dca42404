// What the batch filler's sources crops.hip, crops_index.hip, crops_affine.hip and crops_corrupt.hip (which takes the block
// size, the row vector type and the extent checks) share, written once:
// how a workgroup decodes its sample's slot record and table row, the quarter turn between the rotated and the stored
// frame in both directions, the symmetric pad, the label table's way into LDS, and the host checks of the arguments the
// bank-mode entries have in common (the rule itself is written out in mivp.h).  Device helpers are inlined into the
// kernels that call them; no kernel and no entry point lives here.
#pragma once
#include "common.hpp"

namespace {
constexpr int TPB = 256;
constexpr int MAXC = 16;
typedef f32x4 f32x4u __attribute__((aligned(4)));      // four voxels of a row: crops start at any multiple of 4 bytes

MIVP_DEV int pad_before(int roi, int m) { return (roi - min(roi, m)) >> 1; }   // SpatialPad's symmetric rule
MIVP_DEV bool inside(int r, int m) { return (unsigned)r < (unsigned)m; }

// A bank volume as a workgroup sees it: uniform values, scalar registers.  k_crop_pick (crops_index.hip) keeps its own decode
// and its own stored-to-rotated switch: through the functions below its assembly changes (profiles/README.md).
struct BankVol {
    const float* img;
    const uint8_t* lab;
    int n0, n1, n2;          // stored extents H, W, D
    int m0, m1, m2;          // rotated extents (rotate_extents)
    int code;                // 0 none, 1 / 2 / 3 = rot90(k = 1) over the spatial axes (0,1) / (0,2) / (1,2)
};
// The volume of slot record rec = (volume id, code, ..): img, lab, n and code from the bank's table [n_volumes][5] = (image
// pointer, label pointer or 0, H, W, D).  False -- the workgroup returns without writing -- for a volume id or a code out of
// range (never follow a wild row) and for an empty row of a fixed-capacity table (no image pointer).
MIVP_DEV bool bank_volume(BankVol& v, const int64_t* table, int n_volumes, const int32_t* rec) {
    const int vol = rec[0];
    v.code = rec[1];
    if ((unsigned)vol >= (unsigned)n_volumes || (unsigned)v.code > 3u) return false;
    const int64_t* row = table + (long)vol * 5;
    v.img = reinterpret_cast<const float*>(row[0]);
    if (!v.img) return false;
    v.lab = reinterpret_cast<const uint8_t*>(row[1]);
    v.n0 = (int)row[2]; v.n1 = (int)row[3]; v.n2 = (int)row[4];
    return true;
}
// m from n and the code; apart from bank_volume because the tensor mode of k_crop, which builds its own volume, needs it too
MIVP_DEV void rotate_extents(BankVol& v) {
    const int code = v.code, n0 = v.n0, n1 = v.n1, n2 = v.n2;            // (values: a choice between two fields would be one
    v.m0 = code == 2 ? n2 : (code == 1 ? n1 : n0);                       //  between two addresses, and pin the struct in memory)
    v.m1 = code == 3 ? n2 : (code == 1 ? n0 : n1);
    v.m2 = code == 2 ? n0 : (code == 3 ? n1 : n2);
}

// The quarter turn, torch.rot90(x, 1, (a, b)): out[i_a, i_b] = in[i_b, n_b - 1 - i_a].
// r (rotated frame) -> p (stored frame): p_a = r_b, p_b = (n_b - 1) - r_a; integer voxels and continuous positions alike
template <typename T> struct Vox { T p0, p1, p2; };
template <typename T>
MIVP_DEV Vox<T> to_stored(const BankVol& v, T r0, T r1, T r2) {
    T p0, p1, p2;
    switch (v.code) {
        case 1: p0 = r1; p1 = (T)(v.n1 - 1) - r0; p2 = r2; break;
        case 2: p0 = r2; p1 = r1; p2 = (T)(v.n2 - 1) - r0; break;
        case 3: p0 = r0; p1 = r2; p2 = (T)(v.n2 - 1) - r1; break;
        default: p0 = r0; p1 = r1; p2 = r2; break;
    }
    return {p0, p1, p2};
}
// p (stored frame) -> r (rotated frame), the inverse: r_b = p_a, r_a = n_b - 1 - p_b
MIVP_DEV void to_rotated(const BankVol& v, int p0, int p1, int p2, int& r0, int& r1, int& r2) {
    r0 = p0; r1 = p1; r2 = p2;
    switch (v.code) {
        case 1: r0 = v.n1 - 1 - p1; r1 = p0; break;
        case 2: r0 = v.n2 - 1 - p2; r2 = p0; break;
        case 3: r1 = v.n2 - 1 - p2; r2 = p1; break;
        default: break;
    }
}
// r (rotated frame, in range) -> the offset of p in the stored volume
MIVP_DEV long stored_offset(const BankVol& v, int r0, int r1, int r2) {
    const Vox<int> p = to_stored(v, r0, r1, r2);
    return ((long)p.p0 * v.n1 + p.p1) * v.n2 + p.p2;
}

// the 256-byte label table into LDS, one byte per thread of the TPB
MIVP_DEV void load_lut(uint8_t* s_lut, const uint8_t* __restrict__ lut) {
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
}

// host ----------------------------------------------------------------------------------------------------------------
inline bool extents_ok(const int32_t* e) {
    return e && e[0] >= 1 && e[0] <= 65535 && e[1] >= 1 && e[1] <= 65535 && e[2] >= 1 && e[2] <= 65535;
}
// extents of a tensor of fewer than 2^31 voxels
inline bool roi_ok(const int32_t* roi) { return extents_ok(roi) && (long)roi[0] * roi[1] * roi[2] < (1L << 31); }

// what every bank-mode entry takes: the source table, the slot, the batch and the roi
inline int check_bank_args(const int64_t* table, int32_t n_volumes, const int32_t* slot, int32_t slot_stride, int32_t B,
                           const int32_t* roi) {
    MIVP_REQUIRE(table && slot && ((uintptr_t)table & 7) == 0 && ((uintptr_t)slot & 3) == 0);
    MIVP_REQUIRE(n_volumes >= 1 && B >= 1 && B <= 65535 && slot_stride >= 5 && extents_ok(roi));
    return MIVP_OK;
}
// and what the two teacher fills add: the channel count and the outputs
inline int check_fill_args(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot, int32_t slot_stride,
                           int32_t B, const int32_t* roi, const uint8_t* lut, const float* image, const float* mask,
                           const float* coord) {
    const int rc = check_bank_args(table, n_volumes, slot, slot_stride, B, roi);
    if (rc) return rc;
    MIVP_REQUIRE(image && ((uintptr_t)image & 3) == 0 && ((uintptr_t)mask & 3) == 0 && ((uintptr_t)coord & 3) == 0);
    MIVP_REQUIRE(C >= 1 && C <= MAXC && (long)roi[0] * roi[1] * roi[2] * (C > 3 ? C : 3) < (1L << 31));
    MIVP_REQUIRE(!mask || lut);
    return MIVP_OK;
}
}  // namespace
