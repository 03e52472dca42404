// Device code shared by the two exact Euclidean distance transforms: csrc/surface.hip (one volume, one class: mivp_edt_sq,
// DESIGN 4.16) and csrc/distmap.hip (all samples, classes and both sides in one launch per pass: mivp_distmap_signed,
// DESIGN 4.35).  Both run the same per-element and per-line arithmetic, so a field of the batched transform has the bits
// of the single one on the same seeds.
//   edt_d_value  the D pass's value from the index distance to the nearest seed of the line
//   edt_line     Meijster's lower envelope of parabolas a (x - i)^2 + f(i) along one line of n elements at `stride`, in
//                place; the stack (site | boundary << 16, bits of f(site)) lives at stack[depth * nlines + line].  With unit
//                spacing (INTP) the envelope's intersections are integer floor divisions and every squared distance is the
//                exact integer.  n <= 65535 (16-bit site and boundary).
#pragma once
#include "common.hpp"
#include <math.h>

namespace {
constexpr int EDT_NO_SEED = 1 << 29;
constexpr int EDT_UNROLL = 8;

// dd: index distance to the nearest seed of the line (>= EDT_NO_SEED / 2: the line has none)
MIVP_DEV float edt_d_value(int dd, float a, int intp) {
    if (dd >= EDT_NO_SEED / 2) return INFINITY;
    return intp ? (float)((long long)dd * dd) : a * (float)((long long)dd * dd);
}

template <bool INTP>
MIVP_DEV void edt_line(float* __restrict__ base, long stride, int n, float a, int2* __restrict__ stack, long nlines, long line) {
    // F(x, i) = a (x - i)^2 + f(i); integers at unit spacing
    using val_t = typename std::conditional<INTP, long long, float>::type;
    auto F = [&](int x, int i, float fi) -> val_t {
        const long long dx = x - i;
        if (INTP) return (val_t)(dx * dx + (long long)fi);
        return (val_t)(a * (float)(dx * dx) + fi);
    };
    // first x where u's parabola is below i's (i < u): 1 + floor((a (u^2 - i^2) + f(u) - f(i)) / (2 a (u - i)))
    auto start = [&](int i, float fi, int u, float fu) -> int {
        long long sep;
        if (INTP) {
            const long long num = (long long)u * u - (long long)i * i + (long long)fu - (long long)fi;
            const long long den = 2LL * (u - i);
            sep = num >= 0 ? num / den : -((-num + den - 1) / den);
        } else {
            const float q = (fu - fi + a * (float)((long long)u * u - (long long)i * i)) / (2.f * a * (float)(u - i));
            sep = (long long)floorf(fminf(fmaxf(q, -2.f), (float)n + 1.f));
        }
        return (int)min(max(sep + 1, 0LL), (long long)n + 1);
    };
    int k = -1;
    int ts = 0, tt = 0;                                        // top of the stack: site, boundary, f(site)
    float tf = 0.f;
    for (int u0 = 0; u0 < n; u0 += EDT_UNROLL) {
        float fv[EDT_UNROLL];
#pragma unroll
        for (int e = 0; e < EDT_UNROLL; ++e) fv[e] = u0 + e < n ? base[(long)(u0 + e) * stride] : INFINITY;
#pragma unroll
        for (int e = 0; e < EDT_UNROLL; ++e) {
            const int u = u0 + e;
            const float fu = fv[e];
            if (isinf(fu)) continue;
            while (k >= 0 && F(tt, ts, tf) > F(tt, u, fu)) {
                --k;
                if (k >= 0) {
                    const int2 s = stack[(long)k * nlines + line];
                    ts = s.x & 0xffff; tt = (unsigned)s.x >> 16; tf = __int_as_float(s.y);
                }
            }
            int w = 0;
            if (k >= 0) {
                w = start(ts, tf, u, fu);
                if (w >= n) continue;
            }
            ++k;
            ts = u; tt = w; tf = fu;
            stack[(long)k * nlines + line] = make_int2(u | (w << 16), __float_as_int(fu));
        }
    }
    if (k < 0) {
        for (int u = 0; u < n; ++u) base[(long)u * stride] = INFINITY;
        return;
    }
    for (int u = n - 1; u >= 0; --u) {
        while (k > 0 && tt > u) {
            --k;
            const int2 s = stack[(long)k * nlines + line];
            ts = s.x & 0xffff; tt = (unsigned)s.x >> 16; tf = __int_as_float(s.y);
        }
        base[(long)u * stride] = (float)F(u, ts, tf);
    }
}
}  // namespace
