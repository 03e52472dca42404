// The closing pass of the prompt encodings that evaluate boxes (csrc/strokes.hip; csrc/geodesic.hip):
// the box rule and the walk over a sample's run of two guidance channels, one definition for both.
//
// A sample's two channels are one run of 2 vol floats whose start is aligned to 4 bytes only (vol may be odd).  A workgroup
// row walks it as [head of 0..3 scalars][16-byte quads][tail], as k_clicks_encode does; every element is stored once.
// value = max(box, prompt(field element)): box = 1 inside a box of the channel (frame == 0) or on a box's surface (frame != 0:
// inside, with a coordinate equal to the box's lo or hi), else 0; prompt is the caller's function of the field.
#pragma once
#include "common.hpp"

constexpr int GUIDE_TPB = 256;
constexpr int GUIDE_MAXKB = 16;

struct GuideBox { int l0, l1, l2, h0, h1, h2; };

struct GuideRun {
    int H, W, D, KB, Ctot, off, frame;
};

// whether (h, w) is inside box c, and on its surface already
MIVP_DEV bool guide_hw_in(const GuideBox& c, int h, int w, bool& edge) {
    edge = h == c.l0 || h == c.h0 || w == c.l1 || w == c.h1;
    return h >= c.l0 && h <= c.h0 && w >= c.l1 && w <= c.h1;
}

MIVP_DEV bool guide_d_in(const GuideBox& c, int d, bool edge, int frame) {
    return d >= c.l2 && d <= c.h2 && (!frame || edge || d == c.l2 || d == c.h2);
}

// Wave 0 compacts the boxes of sample b per channel: lst[ch][i] = box i of channel ch, n[ch] of them.  boxes == nullptr: none.
// The caller puts a __syncthreads() behind it.
MIVP_DEV void guide_boxes(const int32_t* __restrict__ boxes, const int32_t* __restrict__ box_count, int b, int KB,
                          GuideBox (*lst)[GUIDE_MAXKB], int* n) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const int cnt = boxes ? min(max(box_count[b], 0), KB) : 0;
    GuideBox c = {0, 0, 0, -1, -1, -1};
    int chn = -1;
    if (lane < cnt) {
        const int32_t* row = boxes + ((long)b * KB + lane) * 7;
        c.l0 = row[0]; c.l1 = row[1]; c.l2 = row[2]; c.h0 = row[3]; c.h1 = row[4]; c.h2 = row[5];
        chn = row[6];
    }
    for (int ch = 0; ch < 2; ++ch) {
        const unsigned long long m = __ballot(chn == ch);
        if (chn == ch) lst[ch][__popcll(m & ((1ull << lane) - 1))] = c;
        if (lane == 0) n[ch] = __popcll(m);
    }
}

// The walk: grid (blocks per sample, B), GUIDE_TPB threads.  fb: the two fields of sample b, in the order of the run.
template <class Prompt>
MIVP_DEV void guide_close_run(const GuideBox (*lst)[GUIDE_MAXKB], const int* n, const float* __restrict__ fb, const GuideRun& e,
                              float* __restrict__ out, Prompt prompt) {
    const int b = blockIdx.y;
    const long vol = (long)e.H * e.W * e.D;
    const long run = 2 * vol;                                      // the two guidance channels of sample b
    float* base = out + ((long)b * e.Ctot + e.off) * vol;
    const long head = min((long)((16 - ((uintptr_t)base & 15)) & 15) >> 2, run);
    const long nq = (run - head) >> 2;
    const long tail0 = head + 4 * nq;                              // first element of the tail
    const int WD = e.W * e.D;
    // value of element el of the run
    auto one = [&](long el) -> float {
        const int ch = el >= vol ? 1 : 0;
        const int r = (int)(el - (ch ? vol : 0L));
        const int h = r / WD, w = (r - h * WD) / e.D, d = r - h * WD - w * e.D;
        bool hit = false;
        for (int i = 0; i < n[ch]; ++i) {
            const GuideBox c = lst[ch][i];
            bool edge;
            hit |= guide_hw_in(c, h, w, edge) && guide_d_in(c, d, edge, e.frame);
        }
        return fmaxf(hit ? 1.f : 0.f, prompt(fb[el]));
    };
    for (long q = (long)blockIdx.x * GUIDE_TPB + threadIdx.x; q <= nq; q += (long)gridDim.x * GUIDE_TPB) {
        if (q == nq) {                                             // the one item of the unaligned ends
            for (long el = 0; el < head; ++el) base[el] = one(el);
            for (long el = tail0; el < run; ++el) base[el] = one(el);
            continue;
        }
        const long el = head + 4 * q;
        const int ch = el >= vol ? 1 : 0;
        const int r = (int)(el - (ch ? vol : 0L));
        const int h = r / WD, w = (r - h * WD) / e.D, d = r - h * WD - w * e.D;
        float4 v;
        if (d + 3 < e.D) {                                         // four voxels of one line: the (h, w) part once per box
            bool h0 = false, h1 = false, h2 = false, h3 = false;
            for (int i = 0; i < n[ch]; ++i) {
                const GuideBox c = lst[ch][i];
                bool edge;
                if (!guide_hw_in(c, h, w, edge)) continue;
                h0 |= guide_d_in(c, d, edge, e.frame); h1 |= guide_d_in(c, d + 1, edge, e.frame);
                h2 |= guide_d_in(c, d + 2, edge, e.frame); h3 |= guide_d_in(c, d + 3, edge, e.frame);
            }
            const float m0 = fb[el], m1 = fb[el + 1], m2 = fb[el + 2], m3 = fb[el + 3];
            v = make_float4(fmaxf(h0 ? 1.f : 0.f, prompt(m0)), fmaxf(h1 ? 1.f : 0.f, prompt(m1)),
                            fmaxf(h2 ? 1.f : 0.f, prompt(m2)), fmaxf(h3 ? 1.f : 0.f, prompt(m3)));
        } else {
            v = make_float4(one(el), one(el + 1), one(el + 2), one(el + 3));
        }
        *reinterpret_cast<float4*>(base + el) = v;
    }
}

// blocks per sample of the walk
inline unsigned guide_grid(long vol) {
    const long items = (2L * vol) / 4 + 1;
    return (unsigned)((items + GUIDE_TPB - 1) / GUIDE_TPB > 8192 ? 8192 : (items + GUIDE_TPB - 1) / GUIDE_TPB);
}
