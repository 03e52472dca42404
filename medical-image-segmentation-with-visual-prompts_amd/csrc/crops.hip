// Training-batch sampling from a bank of resident scans (mivp_amd/batches.py): the reference's Rotate90d (a
// OneOf over three axis pairs), RandSpatialCropSamplesd, SpatialPadd, LoadCoordGridd and map_label_indices
// (datasets/transforms.py:84-98,186-212,323-344, modules/utils.py:372-388) as ONE gather, and the students' RandSpatialCropd
// + SpatialPadd (transforms.py:299-313) as the same gather from the teacher batch.  Pure data movement: every output voxel
// is written exactly once, nothing is accumulated, and what selects the crops is DEVICE memory (the slot), so a launch
// records into a graph and a replay follows whatever the host loaded since.
//
//   output voxel u of sample b:  r = origin + u - pad_before               (position in the ROTATED volume)
//                                pad_before = (roi - min(roi, n_rot)) / 2  (SpatialPad's symmetric rule)
//   r outside the rotated volume -> 0 everywhere; else p = r mapped back through the rotation and
//                                image = vol[:, p]   mask = lut[lab[p]]   coord[k] = p[k] - (n[k] - 1) / 2
//
// A workgroup decodes its sample's slot record and table row once (uniform values: scalar registers) and then takes one of
// two paths; the grid is the larger of the two decompositions, surplus workgroups return at once:
//   rows  (codes 0, 1 and the tensor mode: D stays the contiguous axis): unit = (u_h, a chunk of 256 / LX rows along w),
//         LX lanes along d, four voxels per lane and step -- one 16-byte load and store per tensor (4-byte aligned: a crop
//         starts anywhere) where the four voxels lie inside the volume, voxel by voxel at the edges and in the d % 4 tail.
//   tiles (codes 2, 3: D is exchanged with H or W): unit = (fixed axis, 64 x 64 tile over the exchanged output axis and d).
//         The tile is read along the source's D (which runs backwards along the exchanged output axis), crosses LDS
//         ([64][65]: the transposed read is conflict-free) and is written along the output's d, as k_mv_permute does.  The
//         coordinates are arithmetic and skip the LDS.
// No division in the voxel loops; the per-workgroup ones are 32-bit and uniform.  No out-of-range address can be formed from
// the slot: the volume id and the code are checked per workgroup, r per voxel.  The record and row decode, the quarter turn
// and the pad rule are crops_common.hpp's, shared with crops_index.hip and crops_affine.hip.
#include "crops_common.hpp"

namespace {
constexpr int TILE = 64;

struct CropArgs {
    const int64_t* table;    // bank mode: [n_volumes][5]; NULL in tensor mode
    const float* src;        // tensor mode: [B][C][sdims]
    int n_volumes, C, B;
    int sd[3];               // tensor mode: the source extents
    const int32_t* slot;
    int slot_stride;
    int h, w, d;             // roi
    int lxs;                 // rows path: log2 of the lanes along d
    int nwc;                 // rows path: chunks of (TPB >> lxs) rows along w
    const uint8_t* lut;
    float* image;
    float* mask;
    float* coord;
};

// what a workgroup knows about its sample
struct Sample : BankVol {
    int s0, s1, s2;          // origin - pad_before: r = s + u
};

// ---------------------------------------------------------------------------------------------------------------------
// rows: D in place.  Thread = (row u_w of the chunk, lane along d).
// ---------------------------------------------------------------------------------------------------------------------
MIVP_DEV void crop_rows(const CropArgs& a, const Sample& s, int b, const uint8_t* s_lut) {
    const int unit = blockIdx.x;
    if (unit >= a.h * a.nwc) return;
    const int uh = unit / a.nwc, wc = unit - uh * a.nwc;
    const int lx = 1 << a.lxs;
    const int uw = wc * (TPB >> a.lxs) + ((int)threadIdx.x >> a.lxs);
    if (uw >= a.w) return;
    const int r0 = s.s0 + uh, r1 = s.s1 + uw;
    const bool row_ok = inside(r0, s.m0) & inside(r1, s.m1);
    int p0 = 0, p1 = 0;
    if (row_ok) { const Vox<int> p = to_stored(s, r0, r1, 0); p0 = p.p0; p1 = p.p1; }
    const long cs = (long)s.n0 * s.n1 * s.n2;                            // source channel stride
    const long srow = ((long)p0 * s.n1 + p1) * s.n2;
    const long ovol = (long)a.h * a.w * a.d;
    const long orow = ((long)uh * a.w + uw) * a.d;
    const float* src = s.img + srow;
    const uint8_t* lab = s.lab ? s.lab + srow : nullptr;
    float* oi = a.image + (long)b * a.C * ovol + orow;
    float* om = a.mask ? a.mask + (long)b * ovol + orow : nullptr;
    float* oc = a.coord ? a.coord + (long)b * 3 * ovol + orow : nullptr;
    const float c0 = (float)p0 - 0.5f * (float)(s.n0 - 1), c1 = (float)p1 - 0.5f * (float)(s.n1 - 1);
    const float h2 = 0.5f * (float)(s.n2 - 1);
    const int Q = (a.d + 3) >> 2;
    for (int q = (int)threadIdx.x & (lx - 1); q < Q; q += lx) {
        const int ud = 4 * q, r2 = s.s2 + ud;
        const int nv = min(4, a.d - ud);
        if (row_ok && nv == 4 && s.n2 >= 4 && (unsigned)r2 <= (unsigned)(s.n2 - 4)) {     // (no r2 + 4: it could wrap)
            for (int c = 0; c < a.C; ++c)
                *reinterpret_cast<f32x4u*>(oi + c * ovol + ud) = *reinterpret_cast<const f32x4u*>(src + c * cs + r2);
            if (om) {
                f32x4 m = fzero4();
                if (lab) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) m[j] = (float)s_lut[lab[r2 + j]];
                }
                *reinterpret_cast<f32x4u*>(om + ud) = m;
            }
            if (oc) {
                const f32x4 k0 = {c0, c0, c0, c0}, k1 = {c1, c1, c1, c1};
                f32x4 k2;
#pragma unroll
                for (int j = 0; j < 4; ++j) k2[j] = (float)(r2 + j) - h2;
                *reinterpret_cast<f32x4u*>(oc + ud) = k0;
                *reinterpret_cast<f32x4u*>(oc + ovol + ud) = k1;
                *reinterpret_cast<f32x4u*>(oc + 2 * ovol + ud) = k2;
            }
        } else {
            for (int j = 0; j < nv; ++j) {
                const int rj = r2 + j;
                const bool ok = row_ok && inside(rj, s.n2);
                for (int c = 0; c < a.C; ++c) oi[c * ovol + ud + j] = ok ? src[c * cs + rj] : 0.f;
                if (om) om[ud + j] = (ok && lab) ? (float)s_lut[lab[rj]] : 0.f;
                if (oc) {
                    oc[ud + j] = ok ? c0 : 0.f;
                    oc[ovol + ud + j] = ok ? c1 : 0.f;
                    oc[2 * ovol + ud + j] = ok ? (float)rj - h2 : 0.f;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// tiles: codes 2 and 3.  The exchanged output axis e is h (code 2) or w (code 3), the fixed one f is the other; in both the
// source's D index is n2 - 1 - r_e and the source's H (code 2) or W (code 3) index is r_2.
// ---------------------------------------------------------------------------------------------------------------------
MIVP_DEV void crop_tiles(const CropArgs& a, const Sample& s, int b, const uint8_t* s_lut, float (*tile)[TILE + 1]) {
    const bool c2 = s.code == 2;
    const int ne = c2 ? a.h : a.w, nf = c2 ? a.w : a.h;                  // output extents of the exchanged / fixed axis
    const int te = (ne + TILE - 1) / TILE, td = (a.d + TILE - 1) / TILE;
    int unit = blockIdx.x;
    if (unit >= nf * te * td) return;
    const int uf = unit / (te * td);
    unit -= uf * (te * td);
    const int e0 = (unit / td) * TILE, d0 = (unit % td) * TILE;
    const int se = c2 ? s.s0 : s.s1, sf = c2 ? s.s1 : s.s0;              // r = s + u on those axes
    const int me = c2 ? s.m0 : s.m1, mf = c2 ? s.m1 : s.m0;
    const int rf = sf + uf;
    const bool f_ok = inside(rf, mf);
    const long cs = (long)s.n0 * s.n1 * s.n2;
    // source offset of (r_e, r_2) = fbase + r_2 * xs + (n2 - 1 - r_e)
    const long xs = c2 ? (long)s.n1 * s.n2 : (long)s.n2;
    const long fbase = c2 ? (long)rf * s.n2 : (long)rf * s.n1 * s.n2;
    const long ovol = (long)a.h * a.w * a.d;
    const long es = c2 ? (long)a.w * a.d : (long)a.d;                    // output stride of the exchanged axis
    const long obase = (c2 ? (long)uf * a.d : (long)uf * a.w * a.d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int planes = a.C + (a.mask ? 1 : 0);
    for (int pl = 0; pl < planes; ++pl) {
        const bool is_mask = pl == a.C;
        if (pl) __syncthreads();                                         // the tile's readers of the last plane are done
        // read: lane along the exchanged output axis (the source's D, backwards), rows along the output's d
        for (int rr = wave; rr < TILE; rr += TPB / 64) {
            const int re = se + e0 + lane, r2 = s.s2 + d0 + rr;
            const bool ok = f_ok && e0 + lane < ne && d0 + rr < a.d && inside(re, me) && inside(r2, s.m2);
            float v = 0.f;
            if (ok) {
                const long off = fbase + (long)r2 * xs + (s.n2 - 1 - re);
                if (!is_mask) v = s.img[pl * cs + off];
                else if (s.lab) v = (float)s_lut[s.lab[off]];
            }
            tile[rr][lane] = v;
        }
        __syncthreads();
        // write: lane along the output's d
        float* out = is_mask ? a.mask + (long)b * ovol : a.image + ((long)b * a.C + pl) * ovol;
        for (int rr = wave; rr < TILE; rr += TPB / 64) {
            const int ue = e0 + rr, ud = d0 + lane;
            if (ue < ne && ud < a.d) out[obase + ue * es + ud] = tile[lane][rr];
        }
    }
    if (a.coord) {
        float* oc = a.coord + (long)b * 3 * ovol;
        for (int rr = wave; rr < TILE; rr += TPB / 64) {
            const int ue = e0 + rr, ud = d0 + lane;
            if (ue >= ne || ud >= a.d) continue;
            const int re = se + ue, r2 = s.s2 + ud;
            const bool ok = f_ok && inside(re, me) && inside(r2, s.m2);
            float k0 = 0.f, k1 = 0.f, k2 = 0.f;
            if (ok) {
                const Vox<int> p = to_stored(s, c2 ? re : rf, c2 ? rf : re, r2);
                const int p0 = p.p0, p1 = p.p1, p2 = p.p2;
                k0 = (float)p0 - 0.5f * (float)(s.n0 - 1);
                k1 = (float)p1 - 0.5f * (float)(s.n1 - 1);
                k2 = (float)p2 - 0.5f * (float)(s.n2 - 1);
            }
            const long o = obase + ue * es + ud;
            oc[o] = k0;
            oc[ovol + o] = k1;
            oc[2 * ovol + o] = k2;
        }
    }
}

__global__ __launch_bounds__(TPB) void k_crop(CropArgs a) {
    __shared__ float tile[TILE][TILE + 1];
    __shared__ uint8_t s_lut[256];
    const int b = blockIdx.y;
    if (a.lut) load_lut(s_lut, a.lut);
    const int32_t* rec = a.slot + (long)b * a.slot_stride;
    Sample s;
    if (a.table) {
        if (!bank_volume(s, a.table, a.n_volumes, rec)) return;
        rec += 2;
    } else {
        s.code = 0;
        s.n0 = a.sd[0]; s.n1 = a.sd[1]; s.n2 = a.sd[2];
        s.img = a.src + (long)b * a.C * s.n0 * s.n1 * s.n2;
        s.lab = nullptr;
    }
    rotate_extents(s);
    s.s0 = rec[0] - pad_before(a.h, s.m0);
    s.s1 = rec[1] - pad_before(a.w, s.m1);
    s.s2 = rec[2] - pad_before(a.d, s.m2);
    if (s.code >= 2) crop_tiles(a, s, b, s_lut, tile);
    else crop_rows(a, s, b, s_lut);
}

int launch(CropArgs& a, bool tiles, mivp_stream_t stream, const char* what) {
    // lanes along d: the smallest power of two that covers the 16-byte groups of a row, 64 at most
    const int Q = (a.d + 3) / 4;
    a.lxs = 0;
    while ((1 << a.lxs) < Q && a.lxs < 6) ++a.lxs;
    const int rpb = TPB >> a.lxs;
    a.nwc = (a.w + rpb - 1) / rpb;
    long units = (long)a.h * a.nwc;
    if (tiles) {
        const long td = (a.d + TILE - 1) / TILE;
        const long u2 = (long)a.w * ((a.h + TILE - 1) / TILE) * td, u3 = (long)a.h * ((a.w + TILE - 1) / TILE) * td;
        units = units > u2 ? units : u2;
        units = units > u3 ? units : u3;
    }
    if (units >= (1L << 31)) { mivp_set_error("crop: too many work units"); return MIVP_EINVAL; }
    hipLaunchKernelGGL(k_crop, dim3((unsigned)units, (unsigned)a.B), dim3(TPB), 0, (hipStream_t)stream, a);
    return mivp_check_launch(what);
}
}  // namespace

extern "C" int mivp_crop_fill(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot, int32_t slot_stride,
                              int32_t B, const int32_t* roi, const uint8_t* lut, float* image, float* mask, float* coord,
                              mivp_stream_t stream) {
    const int rc = check_fill_args(table, n_volumes, C, slot, slot_stride, B, roi, lut, image, mask, coord);
    if (rc) return rc;
    CropArgs a{};
    a.table = table; a.n_volumes = n_volumes; a.C = C; a.B = B;
    a.slot = slot; a.slot_stride = slot_stride;
    a.h = roi[0]; a.w = roi[1]; a.d = roi[2];
    a.lut = mask ? lut : nullptr;
    a.image = image; a.mask = mask; a.coord = coord;
    return launch(a, true, stream, "crop_fill");
}

extern "C" int mivp_crop_tensor(const float* src, int32_t Cs, const int32_t* sdims, const int32_t* slot,
                                int32_t slot_stride, int32_t B, const int32_t* roi, float* out, mivp_stream_t stream) {
    MIVP_REQUIRE(src && slot && out && src != out && ((uintptr_t)src & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
                 ((uintptr_t)slot & 3) == 0);
    MIVP_REQUIRE(Cs >= 1 && Cs <= MAXC && B >= 1 && B <= 65535 && slot_stride >= 3);
    MIVP_REQUIRE(roi_ok(roi) && roi_ok(sdims));
    MIVP_REQUIRE((long)roi[0] * roi[1] * roi[2] * Cs < (1L << 31) && (long)sdims[0] * sdims[1] * sdims[2] * Cs < (1L << 31));
    CropArgs a{};
    a.src = src; a.C = Cs; a.B = B;
    a.sd[0] = sdims[0]; a.sd[1] = sdims[1]; a.sd[2] = sdims[2];
    a.slot = slot; a.slot_stride = slot_stride;
    a.h = roi[0]; a.w = roi[1]; a.d = roi[2];
    a.image = out;
    return launch(a, false, stream, "crop_tensor");
}
