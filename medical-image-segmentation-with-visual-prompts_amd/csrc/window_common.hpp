// What the whole-volume prediction sources stitch.hip, window_skip.hip and window_fit.hip share,
// written once: the window geometry with its argument check, and the plain accumulation of one blend contribution.
// Device helpers are inlined into the kernels that call them; no kernel and no entry point lives here.
#pragma once
#include "common.hpp"
#include <limits.h>

namespace {
constexpr int MAXC = 16;
constexpr int TPB = 256;

struct Geo {
    int n[3];      // image size
    int pad[3];    // zeros in front of the image (padded volume coordinates = image coordinates + pad)
    int p[3];      // padded size, max(n, roi)
    int r[3];      // roi
};

bool fill_geo(Geo& g, const int32_t* dims, const int32_t* pad, const int32_t* pdims, const int32_t* roi) {
    for (int a = 0; a < 3; ++a) {
        g.n[a] = dims[a]; g.pad[a] = pad[a]; g.p[a] = pdims[a]; g.r[a] = roi[a];
        if (g.n[a] < 1 || g.r[a] < 1 || g.pad[a] < 0 || g.pad[a] + g.n[a] > g.p[a] || g.r[a] > g.p[a]) return false;
    }
    return (long)g.p[0] * g.p[1] * g.p[2] < (1L << 31) / MAXC;
}

// the plain accumulation of one contribution: k_window_blend, and k_window_blend_tta without COMP
MIVP_DEV void add_weighted(float (&a)[MAXC], int C, float wt, const float* src, long cs) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) a[c] += wt * src[c * cs];
}
}  // namespace
