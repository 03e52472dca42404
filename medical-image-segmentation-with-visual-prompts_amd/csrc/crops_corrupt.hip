// The students' own corruption for the batch filler (mivp_amd/batches.py): the reference's students_rand_ts
// (datasets/transforms.py:244-297) -- a OneOf over nothing, RandCoarseDropoutd with dropout_holes True / False and
// RandCoarseShuffled -- applied in place to a student's image tensor AFTER the student crop.  The rule is written out in
// mivp.h; what selects it is DEVICE memory (one record per sample), so both launches record into a graph and a replay
// follows whatever the host loaded since.  Two kernels per student:
//   k_corrupt_range: per sample in mode 1 or 2, NPART workgroups stream the sample (16-byte loads, 4-byte aligned) and each
//         leaves its (min, max) in range[b][part]: no atomics and nothing to zero between calls.  Minimum and maximum do
//         not depend on the order, so the partials may be cut anywhere.
//   k_corrupt_apply: a workgroup decodes and CHECKS its sample's record (uniform values) and then
//         mode 0: returns -- the sample is never written;
//         modes 1, 2: rows, as k_crop's rows path: unit = (channel, u_h, a chunk of 256 / LX rows along w), LX lanes along
//                  d, four voxels per lane and step.  A replaced value depends on the range and the voxel's index alone, so
//                  the path only STORES: 16 bytes where all four voxels are replaced, voxel by voxel elsewhere and in the
//                  d % 4 tail; a row no hole touches is skipped in mode 1;
//         mode 3: workgroup c < C takes channel c: hole after hole, in list order, the hole is staged in LDS (at most 4096
//                  voxels: 16 KB) and written back through the keyed permutation.  One workgroup owns a (sample, channel),
//                  so overlapping holes compose in order with workgroup barriers alone.
// A record that fails the check (mode, hole count, a hole outside the tensor, a shuffle hole above 4096 voxels) leaves its
// sample unwritten: no address is ever formed from an unchecked word.
#include "crops_common.hpp"

namespace {
constexpr int MAXH = MIVP_CORRUPT_MAX_HOLES;
constexpr int HOLE_WORDS = 7;                          // origin[3], size[3], key
constexpr int REC_WORDS = MIVP_CORRUPT_RECORD_WORDS;   // mode, hole count, noise key, then MAXH holes
constexpr int NPART = MIVP_CORRUPT_PARTIALS;
constexpr int MAXSHUF = MIVP_CORRUPT_SHUFFLE_VOXELS;
static_assert(REC_WORDS == 3 + MAXH * HOLE_WORDS && NPART == 64 && MAXSHUF == 4096, "mivp.h");

struct CorruptArgs {
    float* x;                // [B][C][h][w][d], corrupted in place
    const int32_t* rec;      // [B][REC_WORDS]
    const float* range;      // [B][NPART][2]
    int C, h, w, d;
    int lxs, nwc;            // rows path: log2 of the lanes along d, chunks of (TPB >> lxs) rows along w
};

MIVP_DEV bool span_ok(int o, int s, int ext) { return s >= 1 && s <= ext && o >= 0 && o <= ext - s; }

// every word an address or a loop bound is formed from (uniform: scalar loads and compares)
MIVP_DEV bool record_ok(const int32_t* __restrict__ rec, int h, int w, int d) {
    const int mode = rec[0], n = rec[1];
    if ((unsigned)mode > 3u || (unsigned)n > (unsigned)MAXH) return false;
    for (int k = 0; k < n; ++k) {
        const int32_t* q = rec + 3 + k * HOLE_WORDS;
        if (!(span_ok(q[0], q[3], h) && span_ok(q[1], q[4], w) && span_ok(q[2], q[5], d))) return false;
        if (mode == 3 && (long)q[3] * q[4] * q[5] > MAXSHUF) return false;       // (each size <= 65535: no overflow)
    }
    return true;
}

// lo + (hi - lo) * u, u = the top 24 bits of the hash times 2^-24: the product and the sum are rounded separately
MIVP_DEV float noise_value(float lo, float span, uint32_t key, uint32_t idx) {
#pragma clang fp contract(off)
    const float u = (float)(drop_hash(idx, key) >> 8) * 0x1p-24f;
    const float t = span * u;
    return lo + t;
}

// The keyed bijection of {0 .. n-1}: a balanced Feistel network of four rounds over the 2^bits values of the next even
// bit count (at least 2), walked until the value falls below n.  A permutation of the 2^bits values returns into [0, n)
// from any start below n, after fewer than 2^bits steps.
MIVP_DEV int hole_perm(int j, int n, uint32_t key) {
    int bits = n > 1 ? 32 - __clz(n - 1) : 0;
    bits = max(2, (bits + 1) & ~1);
    const int half = bits >> 1;
    const uint32_t mask = (1u << half) - 1u;
    uint32_t v = (uint32_t)j;
    for (int it = 0; it < (1 << bits); ++it) {
        uint32_t l = v >> half, r = v & mask;
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            const uint32_t t = l ^ ((drop_hash(r + 64u * round, key) >> 16) & mask);     // (r < 64: the counters differ)
            l = r;
            r = t;
        }
        v = (l << half) | r;
        if (v < (uint32_t)n) break;
    }
    return (int)v;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_corrupt_range(const float* __restrict__ x, const int32_t* __restrict__ rec,
                                                       int per_sample, float* __restrict__ range) {
    __shared__ float s_lo[TPB / 64], s_hi[TPB / 64];
    const int b = blockIdx.y;
    const int mode = rec[(long)b * REC_WORDS];
    if (mode != 1 && mode != 2) return;                                  // the others never read the range
    const float* p = x + (long)b * per_sample;
    float lo = INFINITY, hi = -INFINITY;
    const int n4 = per_sample >> 2;
    for (int q = blockIdx.x * TPB + threadIdx.x; q < n4; q += NPART * TPB) {
        const f32x4 v = *reinterpret_cast<const f32x4u*>(p + 4 * (long)q);
        lo = fminf(fminf(lo, v[0]), fminf(v[1], fminf(v[2], v[3])));
        hi = fmaxf(fmaxf(hi, v[0]), fmaxf(v[1], fmaxf(v[2], v[3])));
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < per_sample - 4 * n4) {     // the % 4 tail
        const float v = p[4 * (long)n4 + threadIdx.x];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    for (int off = 32; off; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < TPB / 64; ++i) { lo = fminf(lo, s_lo[i]); hi = fmaxf(hi, s_hi[i]); }
        float* out = range + ((long)b * NPART + blockIdx.x) * 2;
        out[0] = lo;
        out[1] = hi;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// modes 1 and 2.  Thread = (row u_w of the chunk, lane along d).
MIVP_DEV void noise_rows(const CorruptArgs& a, const int32_t* __restrict__ rec, float* xs, float lo, float hi) {
    const int per_c = a.h * a.nwc;
    const int unit = blockIdx.x;
    if (unit >= a.C * per_c) return;
    const int c = unit / per_c, rem = unit - c * per_c;
    const int uh = rem / a.nwc, wc = rem - uh * a.nwc;
    const int lx = 1 << a.lxs;
    const int uw = wc * (TPB >> a.lxs) + ((int)threadIdx.x >> a.lxs);
    if (uw >= a.w) return;
    const int n = rec[1];
    const bool keep = rec[0] == 2;
    // the holes that cross this row, as spans along d (length 0: not this row)
    int z0[MAXH], zn[MAXH];
    bool any = false;
#pragma unroll
    for (int k = 0; k < MAXH; ++k) {
        const int32_t* q = rec + 3 + k * HOLE_WORDS;                     // (inside the record for every k)
        const bool on = k < n && (unsigned)(uh - q[0]) < (unsigned)q[3] && (unsigned)(uw - q[1]) < (unsigned)q[4];
        z0[k] = q[2];
        zn[k] = on ? q[5] : 0;
        any |= on;
    }
    if (!keep && !any) return;
    const uint32_t key = (uint32_t)rec[2];
    const float span = hi - lo;
    const uint32_t ridx = (uint32_t)(((c * a.h + uh) * a.w + uw) * a.d);      // the row's index within the sample (< 2^31)
    float* row = xs + ridx;
    const int Q = (a.d + 3) >> 2;
    for (int q = (int)threadIdx.x & (lx - 1); q < Q; q += lx) {
        const int ud = 4 * q;
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool in = false;
#pragma unroll
            for (int k = 0; k < MAXH; ++k) in |= (unsigned)(ud + j - z0[k]) < (unsigned)zn[k];
            m |= (unsigned)((in != keep) && ud + j < a.d) << j;
        }
        if (!m) continue;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = noise_value(lo, span, key, ridx + (uint32_t)(ud + j));
        if (m == 0xFu) {
            *reinterpret_cast<f32x4u*>(row + ud) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((m >> j) & 1u) row[ud + j] = v[j];
        }
    }
}

// mode 3, one channel: the holes in list order.  Voxel j of a hole counts in C order of the hole's own extents.
MIVP_DEV void shuffle_channel(const CorruptArgs& a, const int32_t* __restrict__ rec, float* xc, float* s_hole) {
    const int n_holes = rec[1];
    for (int k = 0; k < n_holes; ++k) {
        const int32_t* q = rec + 3 + k * HOLE_WORDS;
        const int o0 = q[0], o1 = q[1], o2 = q[2], e1 = q[4], e2 = q[5];
        const int n = q[3] * e1 * e2;                                    // <= MAXSHUF (record_ok)
        const uint32_t key = (uint32_t)q[6];
        auto offset = [&](int j) {
            const int t = j / e2, u2 = j - t * e2;
            const int u0 = t / e1, u1 = t - u0 * e1;
            return ((o0 + u0) * a.w + (o1 + u1)) * a.d + (o2 + u2);
        };
        for (int j = threadIdx.x; j < n; j += TPB) s_hole[j] = xc[offset(j)];
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += TPB) xc[offset(j)] = s_hole[hole_perm(j, n, key)];
        __syncthreads();                                                 // the next hole reads what this one wrote
    }
}

__global__ __launch_bounds__(TPB) void k_corrupt_apply(CorruptArgs a) {
    __shared__ float s_hole[MAXSHUF];
    __shared__ float s_range[2];
    const int b = blockIdx.y;
    const int32_t* rec = a.rec + (long)b * REC_WORDS;
    const int mode = rec[0];
    if (mode == 0 || !record_ok(rec, a.h, a.w, a.d)) return;
    const int vox = a.h * a.w * a.d;
    float* xs = a.x + (long)b * a.C * vox;
    if (mode == 3) {
        if ((int)blockIdx.x < a.C) shuffle_channel(a, rec, xs + (long)blockIdx.x * vox, s_hole);
        return;
    }
    if (threadIdx.x < 64) {                                              // NPART == the wave
        const float* part = a.range + ((long)b * NPART + threadIdx.x) * 2;
        float lo = part[0], hi = part[1];
        for (int off = 32; off; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        if (threadIdx.x == 0) { s_range[0] = lo + 0.f; s_range[1] = hi + 0.f; }      // (-0 -> +0: the sign of a zero
    }                                                                                //  extreme depends on the order)
    __syncthreads();
    noise_rows(a, rec, xs, s_range[0], s_range[1]);
}

int check_args(const float* x, int32_t C, const int32_t* dims, const int32_t* rec, int32_t B, const float* range) {
    MIVP_REQUIRE(x && rec && range && ((uintptr_t)x & 3) == 0 && ((uintptr_t)rec & 3) == 0 && ((uintptr_t)range & 3) == 0);
    MIVP_REQUIRE(C >= 1 && C <= MAXC && B >= 1 && B <= 65535 && roi_ok(dims));
    MIVP_REQUIRE((long)dims[0] * dims[1] * dims[2] * C < (1L << 31));
    return MIVP_OK;
}
}  // namespace

extern "C" int mivp_crop_corrupt_range(const float* x, int32_t C, const int32_t* dims, const int32_t* records, int32_t B,
                                       float* range, mivp_stream_t stream) {
    const int rc = check_args(x, C, dims, records, B, range);
    if (rc) return rc;
    hipLaunchKernelGGL(k_corrupt_range, dim3(NPART, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, x, records,
                       C * dims[0] * dims[1] * dims[2], range);
    return mivp_check_launch("crop_corrupt_range");
}

extern "C" int mivp_crop_corrupt(float* x, int32_t C, const int32_t* dims, const int32_t* records, int32_t B,
                                 const float* range, mivp_stream_t stream) {
    const int rc = check_args(x, C, dims, records, B, range);
    if (rc) return rc;
    CorruptArgs a{};
    a.x = x; a.rec = records; a.range = range;
    a.C = C; a.h = dims[0]; a.w = dims[1]; a.d = dims[2];
    // lanes along d: the smallest power of two that covers the 16-byte groups of a row, 64 at most (as crops.hip)
    const int Q = (a.d + 3) / 4;
    while ((1 << a.lxs) < Q && a.lxs < 6) ++a.lxs;
    const int rpb = TPB >> a.lxs;
    a.nwc = (a.w + rpb - 1) / rpb;
    const long units = (long)a.C * a.h * a.nwc;                          // >= C: the shuffle's workgroups are among them
    if (units >= (1L << 31)) { mivp_set_error("crop_corrupt: too many work units"); return MIVP_EINVAL; }
    hipLaunchKernelGGL(k_corrupt_apply, dim3((unsigned)units, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, a);
    return mivp_check_launch("crop_corrupt");
}
