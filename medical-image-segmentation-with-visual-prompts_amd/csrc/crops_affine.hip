// Random flip, rotation and zoom for the batch filler (mivp_amd/batches.py): the teacher launch of crops.hip
// with an affine map per sample and interpolation -- MONAI's RandFlipd / RandAffined (rotate, scale) as ONE gather.  The
// rule (mivp.h) for output voxel u, all fp32:
//
//   q = u - (roi - 1) / 2        r_k = fma(A_k2, q_2, fma(A_k1, q_1, A_k0 * q_0)) + t_k
//   t_k = (roi_k - 1) / 2 + (origin_k - pad_before_k) + s_k                         (position in the ROTATED volume)
//   image: trilinear over the eight corners floor(r) + e (zero outside the rotated volume), D, then W, then H
//   mask : lut[lab] at floor(r + 0.5), coord: r mapped back through the quarter turn, both 0 outside the volume
//
// One workgroup owns an 8 x 8 x 16 output brick of one sample; thread = (u_h, u_w, a group of four voxels along d), so a
// lane stores 16 bytes per tensor.  Every workgroup bounds its brick's source positions by an integer box -- the eight brick
// corners through the map, one voxel of slack for the rounding of r inside the brick, clipped to the volume plus a
// one-voxel rim that holds zeros -- and then takes one of two paths of the same template.  MEASURED: on
// typical draws the staged path took 2.0-2.2x the time of the direct one, so mivp_crop_fill_affine sends every workgroup down
// the direct path; the staged one is kept behind mivp_crop_fill_affine_debug(stage = 1), where the tests prove it equal.
//   staged   (stage = 1 only) the box fits BOXV cells: it is read once per channel by rows along the STORED D axis (32 lanes per row,
//            coalesced; under codes 2 and 3 that is another axis of the box, the LDS write is the strided side) and the
//            eight corners of every voxel come from LDS.  The rim makes the zero rule free: no per-corner range test.  The
//            label map is staged through the lut as bytes in the same pass.  Rows have an odd pitch.
//   direct   the corners are read from global memory, each range-checked and mapped through the quarter turn (strong
//            minification, a non-finite map, a brick wholly outside the volume -- which then loads nothing; with
//            stage = 0, every workgroup).
// No atomics, no per-lane arrays in scratch (everything below is unrolled over constant indices), no host synchronisation.
// No out-of-range address can be formed from device memory: the volume id and the code are checked per workgroup, r per
// voxel with float comparisons BEFORE it becomes an integer, and every LDS index is clamped into the box.  The record and row
// decode, the quarter turn and the pad rule are crops_common.hpp's; `stage` writes out its box permutation (a box, not a point).
//
// Elastic deformation (mivp_crop_fill_elastic): a second kernel of the same template, r = A (q + d(u)) + t
// with d the cubic B-spline of a per-sample control lattice P[3][n0][n1][n2] (4..8 nodes per axis, output-voxel units;
// the rule is in mivp.h).  A sample's workgroups read its int32 flag first: 0 takes fill_brick<false, false>, the affine
// launch's direct path and its bits, and never touches the lattice; otherwise the lattice (at most 6 KiB) is staged in
// LDS and fill_brick<false, true> adds d to q in front of the unchanged fma chain -- d = +0 gives the affine r bit for
// bit.  The basis is separable and a lane's four voxels share (u_h, u_w): the 16 taps over axes 0 and 1 are summed once
// per lattice d-column (`lat_column`), four columns are live, and a voxel that steps into the next knot interval shifts
// them by one and sums one new column.  Only the direct path: the staged box is bounded through an affine map, and that
// bound does not hold under a deformation.  Every LDS index is clamped (an idle lane's too); a non-finite or huge d makes
// r fail make_tap's and make_near's float comparisons, which give zeros.
#include "crops_common.hpp"

namespace {
constexpr int BH = 8, BW = 8, BD = 16;     // the output brick; BD / 4 lanes along d
constexpr int BOXV = 12288;                // cells of the staged box: 48 KiB of image + 12 KiB of labels

struct AffArgs {
    const int64_t* table;
    int n_volumes, C, B;
    const int32_t* slot;
    int slot_stride;
    const float* affine;
    int h, w, d;
    int nbw, nbd;            // bricks along w and d
    const uint8_t* lut;
    float* image;
    float* mask;
    float* coord;
    int stage;               // 0: every workgroup reads global memory; 1: a workgroup stages its box where it fits
    int32_t* paths;
};

struct Src : BankVol {
    float A[9];
    float t[3];              // (roi - 1) / 2 + (origin - pad_before) + s
    float c[3];              // (roi - 1) / 2
};

struct Box {
    int lo0, lo1, lo2;       // first cell, rotated frame (-1: the rim)
    int e0, e1, e2;          // extents
    int pitch;               // e2 | 1
};

MIVP_DEV int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

MIVP_DEV float src_pos(const Src& s, int k, float q0, float q1, float q2) {
    return __builtin_fmaf(s.A[3 * k + 2], q2, __builtin_fmaf(s.A[3 * k + 1], q1, s.A[3 * k] * q0)) + s.t[k];
}

// the trilinear taps of one voxel: false (and harmless integers) where every corner is outside, NaN included
struct Tap {
    int i0, i1, i2;
    float w0, w1, w2;
    bool ok;
};
MIVP_DEV Tap make_tap(const Src& s, float r0, float r1, float r2) {
    Tap t;
    t.ok = r0 >= -1.f && r0 < (float)s.m0 && r1 >= -1.f && r1 < (float)s.m1 && r2 >= -1.f && r2 < (float)s.m2;
    const float a0 = t.ok ? r0 : 0.f, a1 = t.ok ? r1 : 0.f, a2 = t.ok ? r2 : 0.f;
    const float f0 = floorf(a0), f1 = floorf(a1), f2 = floorf(a2);
    t.i0 = (int)f0; t.i1 = (int)f1; t.i2 = (int)f2;
    t.w0 = a0 - f0; t.w1 = a1 - f1; t.w2 = a2 - f2;
    return t;
}

// the nearest voxel: false where it is outside
struct Near {
    int j0, j1, j2;
    bool ok;
};
MIVP_DEV Near make_near(const Src& s, float r0, float r1, float r2) {
    const float h0 = r0 + 0.5f, h1 = r1 + 0.5f, h2 = r2 + 0.5f;
    Near n;
    n.ok = h0 >= 0.f && h0 < (float)s.m0 && h1 >= 0.f && h1 < (float)s.m1 && h2 >= 0.f && h2 < (float)s.m2;
    n.j0 = n.ok ? (int)floorf(h0) : 0;
    n.j1 = n.ok ? (int)floorf(h1) : 0;
    n.j2 = n.ok ? (int)floorf(h2) : 0;
    return n;
}

// v[4 e0 + 2 e1 + e2]: along D, then W, then H
MIVP_DEV float lerp3(const float (&v)[8], const Tap& t) {
    const float c00 = v[0] + t.w2 * (v[1] - v[0]), c01 = v[2] + t.w2 * (v[3] - v[2]);
    const float c10 = v[4] + t.w2 * (v[5] - v[4]), c11 = v[6] + t.w2 * (v[7] - v[6]);
    const float c0 = c00 + t.w1 * (c01 - c00), c1 = c10 + t.w1 * (c11 - c10);
    return c0 + t.w0 * (c1 - c0);
}

// A sample's control lattice as its workgroups see it: uniform values, the nodes in LDS.
struct Lat {
    const float* P;          // LDS [3][n0][n1][n2], output-voxel units
    int n0, n1, n2;          // 4..8 (checked on the host)
    float sc0, sc1, sc2;     // (n_k - 3) / roi_k
};
// The knot interval and the four cubic B-spline weights of output index u on one axis: x = (u + 0.5) * sc,
// i = min(floor(x), n - 4), f = x - i.  An idle lane's u lies past the roi: its i is clamped like any other.
struct Knot {
    int i;
    float b[4];
};
MIVP_DEV Knot make_knot(int u, float sc, int n) {
    const float x = ((float)u + 0.5f) * sc;
    Knot k;
    k.i = clampi((int)floorf(x), 0, n - 4);
    const float f = x - (float)k.i, g = 1.f - f, f2 = f * f, sixth = 1.f / 6.f;
    k.b[0] = g * g * g * sixth;
    k.b[1] = __builtin_fmaf(f2, __builtin_fmaf(3.f, f, -6.f), 4.f) * sixth;
    k.b[2] = __builtin_fmaf(f, __builtin_fmaf(f, __builtin_fmaf(-3.f, f, 3.f), 3.f), 1.f) * sixth;
    k.b[3] = f2 * f * sixth;
    return k;
}
// One lattice d-column: the 16 taps over axes 0 and 1, w[4 a + b] = B_a(f_0) B_b(f_1), summed in the order a, then b, for
// the three components.  p -> P[0][i_0][i_1][column].
MIVP_DEV void lat_column(const Lat& lt, const float* p, const float (&w)[16], float& c0, float& c1, float& c2) {
    const int s1 = lt.n2, s0 = lt.n1 * lt.n2, cs = lt.n0 * s0;
    c0 = w[0] * p[0]; c1 = w[0] * p[cs]; c2 = w[0] * p[2 * cs];
#pragma unroll
    for (int t = 1; t < 16; ++t) {
        const float* n = p + (t >> 2) * s0 + (t & 3) * s1;
        c0 = __builtin_fmaf(w[t], n[0], c0);
        c1 = __builtin_fmaf(w[t], n[cs], c1);
        c2 = __builtin_fmaf(w[t], n[2 * cs], c2);
    }
}

template <bool STAGED>
MIVP_DEV float sample_image(const Src& s, const Box& bx, const float* box, const float* img, const Tap& t) {
    float v[8];
    if (STAGED) {
        const int b0 = clampi(t.i0 - bx.lo0, 0, bx.e0 - 2), b1 = clampi(t.i1 - bx.lo1, 0, bx.e1 - 2);
        const int b2 = clampi(t.i2 - bx.lo2, 0, bx.e2 - 2);
        const int s1 = bx.pitch, s0 = bx.e1 * bx.pitch;
        const float* p = box + b0 * s0 + b1 * s1 + b2;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p[(e >> 2) * s0 + ((e >> 1) & 1) * s1 + (e & 1)];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c0 = t.i0 + (e >> 2), c1 = t.i1 + ((e >> 1) & 1), c2 = t.i2 + (e & 1);
            const bool ok = t.ok && inside(c0, s.m0) && inside(c1, s.m1) && inside(c2, s.m2);
            v[e] = ok ? img[stored_offset(s, c0, c1, c2)] : 0.f;
        }
    }
    const float out = lerp3(v, t);
    return t.ok ? out : 0.f;
}

template <bool STAGED>
MIVP_DEV float sample_mask(const Src& s, const Box& bx, const uint8_t* lbox, const uint8_t* s_lut, const Near& n) {
    if (!s.lab) return 0.f;
    if (STAGED) {
        const int b0 = clampi(n.j0 - bx.lo0, 0, bx.e0 - 1), b1 = clampi(n.j1 - bx.lo1, 0, bx.e1 - 1);
        const int b2 = clampi(n.j2 - bx.lo2, 0, bx.e2 - 1);
        const float v = (float)lbox[(b0 * bx.e1 + b1) * bx.pitch + b2];
        return n.ok ? v : 0.f;
    }
    return n.ok ? (float)s_lut[s.lab[stored_offset(s, n.j0, n.j1, n.j2)]] : 0.f;
}

// One channel of the box (and, with `labels`, the label map through the lut): rows along the stored D axis.
MIVP_DEV void stage(const Src& s, const Box& bx, const float* img, float* box, bool labels, uint8_t* lbox,
                    const uint8_t* s_lut) {
    const int hi0 = bx.lo0 + bx.e0 - 1, hi1 = bx.lo1 + bx.e1 - 1;
    int plo0 = bx.lo0, plo1 = bx.lo1, plo2 = bx.lo2, E0 = bx.e0, E1 = bx.e1, E2 = bx.e2;       // the box in the stored frame
    switch (s.code) {
        case 1: plo0 = bx.lo1; E0 = bx.e1; plo1 = s.n1 - 1 - hi0; E1 = bx.e0; break;
        case 2: plo0 = bx.lo2; E0 = bx.e2; plo2 = s.n2 - 1 - hi0; E2 = bx.e0; break;
        case 3: plo1 = bx.lo2; E1 = bx.e2; plo2 = s.n2 - 1 - hi1; E2 = bx.e1; break;
        default: break;
    }
    const int nrows = E0 * E1;
    for (int row = (int)threadIdx.x >> 5; row < nrows; row += TPB >> 5) {
        const int ra = row / E1;
        const int p0 = plo0 + ra, p1 = plo1 + (row - ra * E1);
        const bool row_ok = inside(p0, s.n0) && inside(p1, s.n1);
        const long base = ((long)p0 * s.n1 + p1) * s.n2;
        for (int x = (int)threadIdx.x & 31; x < E2; x += 32) {
            const int p2 = plo2 + x;
            const bool ok = row_ok && inside(p2, s.n2);
            int r0, r1, r2;
            to_rotated(s, p0, p1, p2, r0, r1, r2);
            const int cell = ((r0 - bx.lo0) * bx.e1 + (r1 - bx.lo1)) * bx.pitch + (r2 - bx.lo2);
            box[cell] = ok ? img[base + p2] : 0.f;
            if (labels) lbox[cell] = ok ? s_lut[s.lab[base + p2]] : (uint8_t)0;
        }
    }
}

template <bool STAGED, bool ELASTIC>
MIVP_DEV void fill_brick(const AffArgs& a, const Src& s, const Box& bx, int b, int u0h, int u0w, int u0d, float* box,
                         uint8_t* lbox, const uint8_t* s_lut, const Lat& lt) {
    const int tid = threadIdx.x;
    const int uh = u0h + (tid >> 5), uw = u0w + ((tid >> 2) & 7), ud = u0d + 4 * (tid & 3);
    const bool active = uh < a.h && uw < a.w && ud < a.d;        // (an idle lane still stages and meets the barriers)
    const int nv = active ? min(4, a.d - ud) : 0;
    const long ovol = (long)a.h * a.w * a.d;
    const long orow = ((long)uh * a.w + uw) * a.d + ud;
    const float q0 = (float)uh - s.c[0], q1 = (float)uw - s.c[1];
    float r0[4], r1[4], r2[4];
    if (ELASTIC) {
        const Knot k0 = make_knot(uh, lt.sc0, lt.n0), k1 = make_knot(uw, lt.sc1, lt.n1);
        float w[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) w[t] = k0.b[t >> 2] * k1.b[t & 3];
        const float* row = lt.P + (k0.i * lt.n1 + k1.i) * lt.n2;
        float S0[4], S1[4], S2[4];                               // columns cb .. cb + 3 of the three components
        int cb = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Knot k2 = make_knot(ud + j, lt.sc2, lt.n2);
            if (k2.i != cb) {
                if (j && k2.i == cb + 1) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) { S0[e] = S0[e + 1]; S1[e] = S1[e + 1]; S2[e] = S2[e + 1]; }
                    lat_column(lt, row + k2.i + 3, w, S0[3], S1[3], S2[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) lat_column(lt, row + k2.i + e, w, S0[e], S1[e], S2[e]);
                }
                cb = k2.i;
            }
            float d0 = k2.b[0] * S0[0], d1 = k2.b[0] * S1[0], d2 = k2.b[0] * S2[0];
#pragma unroll
            for (int e = 1; e < 4; ++e) {
                d0 = __builtin_fmaf(k2.b[e], S0[e], d0);
                d1 = __builtin_fmaf(k2.b[e], S1[e], d1);
                d2 = __builtin_fmaf(k2.b[e], S2[e], d2);
            }
            const float p0 = q0 + d0, p1 = q1 + d1, p2 = ((float)(ud + j) - s.c[2]) + d2;     // q + d first: d = 0 keeps r
            r0[j] = src_pos(s, 0, p0, p1, p2);
            r1[j] = src_pos(s, 1, p0, p1, p2);
            r2[j] = src_pos(s, 2, p0, p1, p2);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float q2 = (float)(ud + j) - s.c[2];
            r0[j] = src_pos(s, 0, q0, q1, q2);
            r1[j] = src_pos(s, 1, q0, q1, q2);
            r2[j] = src_pos(s, 2, q0, q1, q2);
        }
    }
    if (a.coord && active) {
        const float h0 = 0.5f * (float)(s.n0 - 1), h1 = 0.5f * (float)(s.n1 - 1), h2 = 0.5f * (float)(s.n2 - 1);
        f32x4 k0, k1, k2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Near n = make_near(s, r0[j], r1[j], r2[j]);
            const Vox<float> p = to_stored(s, r0[j], r1[j], r2[j]);
            const float p0 = p.p0, p1 = p.p1, p2 = p.p2;
            k0[j] = n.ok ? p0 - h0 : 0.f;
            k1[j] = n.ok ? p1 - h1 : 0.f;
            k2[j] = n.ok ? p2 - h2 : 0.f;
        }
        float* oc = a.coord + (long)b * 3 * ovol + orow;
        if (nv == 4) {
            *reinterpret_cast<f32x4u*>(oc) = k0;
            *reinterpret_cast<f32x4u*>(oc + ovol) = k1;
            *reinterpret_cast<f32x4u*>(oc + 2 * ovol) = k2;
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < nv) { oc[j] = k0[j]; oc[ovol + j] = k1[j]; oc[2 * ovol + j] = k2[j]; }
        }
    }
    const long cs = (long)s.n0 * s.n1 * s.n2;
    for (int c = 0; c < a.C; ++c) {
        const bool labels = c == 0 && a.mask && s.lab;
        if (STAGED) {
            if (c) __syncthreads();                              // the box's readers of the last channel are done
            stage(s, bx, s.img + c * cs, box, labels, lbox, s_lut);
            __syncthreads();
        }
        if (!active) continue;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sample_image<STAGED>(s, bx, box, s.img + c * cs, make_tap(s, r0[j], r1[j], r2[j]));
        float* oi = a.image + ((long)b * a.C + c) * ovol + orow;
        if (nv == 4) *reinterpret_cast<f32x4u*>(oi) = v;
        else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < nv) oi[j] = v[j];
        }
        if (c == 0 && a.mask) {
            f32x4 m;
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = sample_mask<STAGED>(s, bx, lbox, s_lut, make_near(s, r0[j], r1[j], r2[j]));
            float* om = a.mask + (long)b * ovol + orow;
            if (nv == 4) *reinterpret_cast<f32x4u*>(om) = m;
            else {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < nv) om[j] = m[j];
            }
        }
    }
}

struct ElArgs {
    const int32_t* flags;    // DEVICE int32 [B]
    const float* lattice;    // DEVICE fp32 [B][3][n0][n1][n2]
    int n0, n1, n2;
};
constexpr int MAXN = 8;      // nodes per axis: 4 .. MAXN

// The body of both kernels: k_crop_affine is crop_body<false>; k_crop_elastic, crop_body<true>, never stages a box and
// branches per sample on its flag.  box: BOXV floats, then BOXV label bytes -- or nothing (stage == 0, ELASTIC); s_lat: room
// for one sample's lattice (ELASTIC).
template <bool ELASTIC>
MIVP_DEV void crop_body(const AffArgs& a, const ElArgs& el, float* box, float* s_lat) {
    uint8_t* lbox = reinterpret_cast<uint8_t*>(box + BOXV);
    __shared__ uint8_t s_lut[256];
    const int b = blockIdx.y;
    if (a.lut) load_lut(s_lut, a.lut);
    const int32_t* rec = a.slot + (long)b * a.slot_stride;
    Src s;
    if (!bank_volume(s, a.table, a.n_volumes, rec)) return;
    s.m0 = s.code == 2 ? s.n2 : (s.code == 1 ? s.n1 : s.n0);      // rotate_extents, written out: through the shared function
    s.m1 = s.code == 3 ? s.n2 : (s.code == 1 ? s.n0 : s.n1);      // this kernel's registers are numbered differently
    s.m2 = s.code == 2 ? s.n0 : (s.code == 3 ? s.n1 : s.n2);      // (profiles/README.md)
    const float* aff = a.affine + (long)b * 12;
#pragma unroll
    for (int i = 0; i < 9; ++i) s.A[i] = aff[i];
    const int roi[3] = {a.h, a.w, a.d};
    const int m[3] = {s.m0, s.m1, s.m2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.c[k] = 0.5f * (float)(roi[k] - 1);
        s.t[k] = (s.c[k] + (float)(rec[2 + k] - pad_before(roi[k], m[k]))) + aff[9 + k];
    }
    // the brick and the box of its source positions
    int unit = blockIdx.x;
    const int bh = unit / (a.nbw * a.nbd);
    unit -= bh * (a.nbw * a.nbd);
    const int bw = unit / a.nbd, bd = unit - bw * a.nbd;
    const int u0h = bh * BH, u0w = bw * BW, u0d = bd * BD;
    const int u1h = min(u0h + BH, a.h) - 1, u1w = min(u0w + BW, a.w) - 1, u1d = min(u0d + BD, a.d) - 1;
    float mn[3], mx[3];
    bool finite = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float q0 = (float)((e & 4) ? u1h : u0h) - s.c[0], q1 = (float)((e & 2) ? u1w : u0w) - s.c[1];
        const float q2 = (float)((e & 1) ? u1d : u0d) - s.c[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float r = src_pos(s, k, q0, q1, q2);
            finite = finite && fabsf(r) < 1e9f;                  // false for NaN and infinity
            mn[k] = e ? fminf(mn[k], r) : r;
            mx[k] = e ? fmaxf(mx[k], r) : r;
        }
    }
    Box bx = {};
    bool staged = !ELASTIC && finite && a.stage;
    if (staged) {
        // r is affine in u up to its rounding (far below one voxel): the brick's floor(r) lie in [floor(mn) - 1,
        // floor(mx) + 1] and their upper corners one above; clipped to the volume and its rim of zeros at -1 and m
        const int lo0 = max((int)floorf(mn[0]) - 1, -1), hi0 = min((int)floorf(mx[0]) + 2, s.m0);
        const int lo1 = max((int)floorf(mn[1]) - 1, -1), hi1 = min((int)floorf(mx[1]) + 2, s.m1);
        const int lo2 = max((int)floorf(mn[2]) - 1, -1), hi2 = min((int)floorf(mx[2]) + 2, s.m2);
        bx.lo0 = lo0; bx.lo1 = lo1; bx.lo2 = lo2;
        bx.e0 = hi0 - lo0 + 1; bx.e1 = hi1 - lo1 + 1; bx.e2 = hi2 - lo2 + 1;
        bx.pitch = bx.e2 | 1;
        staged = bx.e0 >= 2 && bx.e1 >= 2 && bx.e2 >= 2 && (long)bx.e0 * bx.e1 * bx.pitch <= (long)BOXV;
    }
    if (a.paths && threadIdx.x == 0) a.paths[(long)b * gridDim.x + blockIdx.x] = staged ? 1 : 0;
    Lat lt = {};
    if (ELASTIC && el.flags[b] != 0) {                           // workgroup-uniform; flag 0 never reads the lattice
        const int words = 3 * el.n0 * el.n1 * el.n2;
        const float* P = el.lattice + (long)b * words;
        for (int i = threadIdx.x; i < words; i += TPB) s_lat[i] = P[i];
        __syncthreads();
        lt.P = s_lat; lt.n0 = el.n0; lt.n1 = el.n1; lt.n2 = el.n2;
        lt.sc0 = (float)(el.n0 - 3) / (float)a.h; lt.sc1 = (float)(el.n1 - 3) / (float)a.w;
        lt.sc2 = (float)(el.n2 - 3) / (float)a.d;
        fill_brick<false, true>(a, s, bx, b, u0h, u0w, u0d, box, lbox, s_lut, lt);
    } else if (staged) fill_brick<true, false>(a, s, bx, b, u0h, u0w, u0d, box, lbox, s_lut, lt);
    else fill_brick<false, false>(a, s, bx, b, u0h, u0w, u0d, box, lbox, s_lut, lt);
}

__global__ __launch_bounds__(TPB) void k_crop_affine(AffArgs a) {
    extern __shared__ float box[];
    crop_body<false>(a, ElArgs{}, box, nullptr);
}

__global__ __launch_bounds__(TPB) void k_crop_elastic(AffArgs a, ElArgs el) {      // a.stage = 0: the direct path only
    __shared__ float s_lat[3 * MAXN * MAXN * MAXN];
    crop_body<true>(a, el, nullptr, s_lat);
}

// the checks and the kernel arguments both launches share; `units`: the bricks of one sample
int make_args(AffArgs& a, long& units, const char* who, const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot,
              int32_t slot_stride, const float* affine, int32_t B, const int32_t* roi, const uint8_t* lut, float* image,
              float* mask, float* coord) {
    const int rc = check_fill_args(table, n_volumes, C, slot, slot_stride, B, roi, lut, image, mask, coord);
    if (rc) return rc;
    MIVP_REQUIRE(affine && ((uintptr_t)affine & 3) == 0);
    a.table = table; a.n_volumes = n_volumes; a.C = C; a.B = B;
    a.slot = slot; a.slot_stride = slot_stride; a.affine = affine;
    a.h = roi[0]; a.w = roi[1]; a.d = roi[2];
    a.nbw = (a.w + BW - 1) / BW; a.nbd = (a.d + BD - 1) / BD;
    a.lut = mask ? lut : nullptr;
    a.image = image; a.mask = mask; a.coord = coord;
    units = (long)((a.h + BH - 1) / BH) * a.nbw * a.nbd;
    if (units >= (1L << 31)) { mivp_set_error(who); return MIVP_EINVAL; }
    return MIVP_OK;
}

int launch(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot, int32_t slot_stride, const float* affine,
           int32_t B, const int32_t* roi, const uint8_t* lut, float* image, float* mask, float* coord, int stage,
           int32_t* paths, mivp_stream_t stream) {
    AffArgs a{};
    long units;
    const int rc = make_args(a, units, "crop_fill_affine: too many work units", table, n_volumes, C, slot, slot_stride, affine,
                             B, roi, lut, image, mask, coord);
    if (rc) return rc;
    MIVP_REQUIRE(((uintptr_t)paths & 3) == 0);
    a.stage = stage; a.paths = paths;
    // the box is dynamic LDS: a launch that stages nothing asks for none, and its occupancy is the registers'
    const size_t lds = stage ? (size_t)BOXV * (sizeof(float) + 1) : 0;
    hipLaunchKernelGGL(k_crop_affine, dim3((unsigned)units, (unsigned)B), dim3(TPB), lds, (hipStream_t)stream, a);
    return mivp_check_launch("crop_fill_affine");
}
}  // namespace

extern "C" int mivp_crop_fill_affine(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot,
                                     int32_t slot_stride, const float* affine, int32_t B, const int32_t* roi,
                                     const uint8_t* lut, float* image, float* mask, float* coord, mivp_stream_t stream) {
    return launch(table, n_volumes, C, slot, slot_stride, affine, B, roi, lut, image, mask, coord, 0, nullptr, stream);
}

extern "C" int mivp_crop_fill_affine_debug(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot,
                                           int32_t slot_stride, const float* affine, int32_t B, const int32_t* roi,
                                           const uint8_t* lut, float* image, float* mask, float* coord,
                                           int32_t stage, int32_t* paths, mivp_stream_t stream) {
    return launch(table, n_volumes, C, slot, slot_stride, affine, B, roi, lut, image, mask, coord, stage != 0, paths, stream);
}

extern "C" int mivp_crop_fill_elastic(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot,
                                      int32_t slot_stride, const float* affine, int32_t B, const int32_t* roi,
                                      const uint8_t* lut, float* image, float* mask, float* coord, const int32_t* flags,
                                      const float* lattice, const int32_t* nodes, mivp_stream_t stream) {
    AffArgs a{};
    long units;
    const int rc = make_args(a, units, "crop_fill_elastic: too many work units", table, n_volumes, C, slot, slot_stride, affine,
                             B, roi, lut, image, mask, coord);
    if (rc) return rc;
    MIVP_REQUIRE(flags && lattice && nodes && ((uintptr_t)flags & 3) == 0 && ((uintptr_t)lattice & 3) == 0);
    MIVP_REQUIRE(nodes[0] >= 4 && nodes[0] <= MAXN && nodes[1] >= 4 && nodes[1] <= MAXN && nodes[2] >= 4 && nodes[2] <= MAXN);
    ElArgs el{flags, lattice, nodes[0], nodes[1], nodes[2]};
    hipLaunchKernelGGL(k_crop_elastic, dim3((unsigned)units, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, a, el);
    return mivp_check_launch("crop_fill_elastic");
}
