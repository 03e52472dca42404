// Pixel-space visual prompt: x' = x + scale * T(P), P a coarse f32 lattice [Cin][gh][gw][gd], T its trilinear interpolation
// to the roi [H][W][D] under torch's align_corners=True rule (nodes on the corners; an axis with one node is constant).
//
// Coordinates are exact rationals.  Along an axis with n voxels and g nodes, voxel o sits at o * num / den lattice units,
// num = g - 1, den = n - 1 (num = 0 when g == 1 or n == 1, den = 1 when n == 1):
//     i0 = floor(o num / den),  lambda = ((o num) mod den) / den  (one correctly rounded division),  i1 = min(i0 + 1, g - 1)
// With g == n every lambda is exactly 0: the full-resolution prompt through the same kernels, x' = x + scale * P in the bits.
//
// Forward: one launch, streams x -> x'.  The three per-axis (i0, lambda) tables are built in LDS by every workgroup
// (H + W + D integer divisions), the lattice is staged in LDS when it is at most 32 KiB and read from global memory
// otherwise; seven lerps a + lambda (b - a) along d, w, h.  No roi-sized prompt volume exists anywhere.
//
// Backward: dP[ci][node] = scale * sum_b sum_{voxels of the node's support} weight * dy -- a GATHER per node.  The support
// of node k along an axis is the open interval of voxels with |o num - k den| < den; the weight is 1 - lambda where
// i0 == k and lambda where i0 == k - 1, the product of the three axes taken as (wh * ww) * wd.  Order of the sum:
//   * node kernel (largest support times B at most 64, the full-resolution case): one thread per node, b outermost,
//     then h, w, d ascending, one fp32 accumulator starting at 0;
//   * workgroup kernels (NT = 64 or 256 threads per node): element e = ((b sh + ih) sw + iw) sd + id of the node's support
//     box goes to thread e mod NT, a thread adds its elements in ascending e, the 64 lanes of a wave are combined by the
//     xor butterfly 32, 16, .., 1 and the waves as (w0 + w1) + (w2 + w3).
// No float atomics, nothing zero-filled, nothing read back: equal calls give equal bits.
#include "common.hpp"

namespace {

__host__ __device__ inline void axis_ratio(int n, int g, int& num, int& den) {
    num = (n > 1 && g > 1) ? g - 1 : 0;
    den = n > 1 ? n - 1 : 1;
}

// voxels o of an axis that node k reaches with a non-zero weight: lo .. hi (empty when hi < lo)
__host__ __device__ inline void node_range(int k, int n, int num, int den, int& lo, int& hi) {
    if (num == 0) { lo = 0; hi = k == 0 ? n - 1 : -1; return; }
    lo = k == 0 ? 0 : ((k - 1) * den) / num + 1;
    hi = ((k + 1) * den + num - 1) / num - 1;
    if (hi > n - 1) hi = n - 1;
}

MIVP_DEV float node_weight(int o, int k, int num, int den) {
    const int t = o * num - k * den;
    const float lam = (float)(t >= 0 ? t : t + den) / (float)den;
    return t >= 0 ? 1.f - lam : lam;
}

MIVP_DEV float lerp(float a, float b, float l) { return a + l * (b - a); }

constexpr int LATTICE_LDS_BYTES = 32 * 1024;
constexpr int MAX_AXES_SUM = 4096;                // H + W + D: the tables are 8 bytes per voxel of an axis

template <int V, bool LDSP>
__global__ __launch_bounds__(256) void k_input_prompt_fwd(const float* __restrict__ x, const float* __restrict__ p,
                                                          const float* __restrict__ scale, int B, int Cin, int H, int W, int D,
                                                          int gh, int gw, int gd, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* ti = reinterpret_cast<int*>(smem);                    // [H + W + D] i0
    float* tl = reinterpret_cast<float*>(smem) + (H + W + D);  // [H + W + D] lambda
    const float* lat = p;
    const int tid = threadIdx.x;
    for (int i = tid; i < H + W + D; i += 256) {
        const int a = i < H ? 0 : (i < H + W ? 1 : 2);
        const int o = a == 0 ? i : (a == 1 ? i - H : i - H - W);
        int num, den;
        axis_ratio(a == 0 ? H : (a == 1 ? W : D), a == 0 ? gh : (a == 1 ? gw : gd), num, den);
        const int t = o * num, i0 = t / den;
        ti[i] = i0;
        tl[i] = (float)(t - i0 * den) / (float)den;
    }
    const int nodes = gh * gw * gd;
    if (LDSP) {
        float* ll = reinterpret_cast<float*>(smem) + 2 * (H + W + D);
        for (int i = tid; i < Cin * nodes; i += 256) ll[i] = p[i];
        lat = ll;
    }
    __syncthreads();
    const float s = scale[0];
    const int DV = D / V;
    const long items = (long)B * Cin * H * W * DV;             // host checks B Cin H W D < 2^31: 32-bit decode
    for (long it = (long)blockIdx.x * 256 + tid; it < items; it += (long)gridDim.x * 256) {
        unsigned r = (unsigned)it;
        const int dv = (int)(r % (unsigned)DV); r /= (unsigned)DV;
        const int w = (int)(r % (unsigned)W); r /= (unsigned)W;
        const int h = (int)(r % (unsigned)H); r /= (unsigned)H;
        const int ci = (int)(r % (unsigned)Cin);
        const int h0 = ti[h], w0 = ti[H + w];
        const int h1 = min(h0 + 1, gh - 1), w1 = min(w0 + 1, gw - 1);
        const float lh = tl[h], lw = tl[H + w];
        const float* pl = lat + (long)ci * nodes;
        const float* r00 = pl + ((long)h0 * gw + w0) * gd;
        const float* r01 = pl + ((long)h0 * gw + w1) * gd;
        const float* r10 = pl + ((long)h1 * gw + w0) * gd;
        const float* r11 = pl + ((long)h1 * gw + w1) * gd;
        float xin[V], out[V];
        if constexpr (V == 4) {
            const float4 v = *reinterpret_cast<const float4*>(x + it * 4);
            xin[0] = v.x; xin[1] = v.y; xin[2] = v.z; xin[3] = v.w;
        } else if constexpr (V == 2) {
            const float2 v = *reinterpret_cast<const float2*>(x + it * 2);
            xin[0] = v.x; xin[1] = v.y;
        } else {
            xin[0] = x[it];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int dd = dv * V + v;
            const int d0 = ti[H + W + dd], d1 = min(d0 + 1, gd - 1);
            const float ld = tl[H + W + dd];
            const float c0 = lerp(lerp(r00[d0], r00[d1], ld), lerp(r01[d0], r01[d1], ld), lw);
            const float c1 = lerp(lerp(r10[d0], r10[d1], ld), lerp(r11[d0], r11[d1], ld), lw);
            out[v] = xin[v] + s * lerp(c0, c1, lh);
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(y + it * 4) = make_float4(out[0], out[1], out[2], out[3]);
        else if constexpr (V == 2) *reinterpret_cast<float2*>(y + it * 2) = make_float2(out[0], out[1]);
        else y[it] = out[0];
    }
}

// one thread per node: small supports (the full-resolution prompt: one voxel per sample)
__global__ __launch_bounds__(256) void k_input_prompt_bwd_node(const float* __restrict__ dy, const float* __restrict__ scale,
                                                               int B, int Cin, int H, int W, int D, int gh, int gw, int gd,
                                                               float* __restrict__ dp) {
    const long total = (long)Cin * gh * gw * gd;
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    unsigned r = (unsigned)n;
    const int kd = (int)(r % (unsigned)gd); r /= (unsigned)gd;
    const int kw = (int)(r % (unsigned)gw); r /= (unsigned)gw;
    const int kh = (int)(r % (unsigned)gh);
    const int ci = (int)(r / (unsigned)gh);
    int nh, dh, nw, dw, nd, dd, hlo, hhi, wlo, whi, dlo, dhi;
    axis_ratio(H, gh, nh, dh); axis_ratio(W, gw, nw, dw); axis_ratio(D, gd, nd, dd);
    node_range(kh, H, nh, dh, hlo, hhi); node_range(kw, W, nw, dw, wlo, whi); node_range(kd, D, nd, dd, dlo, dhi);
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* g = dy + ((long)b * Cin + ci) * H * W * D;
        for (int h = hlo; h <= hhi; ++h) {
            const float wh = node_weight(h, kh, nh, dh);
            for (int w = wlo; w <= whi; ++w) {
                const float whw = wh * node_weight(w, kw, nw, dw);
                for (int d = dlo; d <= dhi; ++d)
                    acc += (whw * node_weight(d, kd, nd, dd)) * g[((long)h * W + w) * D + d];
            }
        }
    }
    dp[n] = scale[0] * acc;
}

// one workgroup of NT threads per node
template <int NT>
__global__ __launch_bounds__(NT) void k_input_prompt_bwd_group(const float* __restrict__ dy, const float* __restrict__ scale,
                                                               int B, int Cin, int H, int W, int D, int gh, int gw, int gd,
                                                               float* __restrict__ dp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* wt = reinterpret_cast<float*>(smem);                // [sh + sw + sd] axis weights of this node
    __shared__ float wsum[4];
    const int tid = threadIdx.x;
    unsigned r = blockIdx.x;
    const int kd = (int)(r % (unsigned)gd); r /= (unsigned)gd;
    const int kw = (int)(r % (unsigned)gw); r /= (unsigned)gw;
    const int kh = (int)(r % (unsigned)gh);
    const int ci = (int)(r / (unsigned)gh);
    int nh, dh, nw, dw, nd, dd, hlo, hhi, wlo, whi, dlo, dhi;
    axis_ratio(H, gh, nh, dh); axis_ratio(W, gw, nw, dw); axis_ratio(D, gd, nd, dd);
    node_range(kh, H, nh, dh, hlo, hhi); node_range(kw, W, nw, dw, wlo, whi); node_range(kd, D, nd, dd, dlo, dhi);
    const int sh = max(hhi - hlo + 1, 0), sw = max(whi - wlo + 1, 0), sd = max(dhi - dlo + 1, 0);
    for (int i = tid; i < sh + sw + sd; i += NT)
        wt[i] = i < sh ? node_weight(hlo + i, kh, nh, dh)
                       : (i < sh + sw ? node_weight(wlo + i - sh, kw, nw, dw) : node_weight(dlo + i - sh - sw, kd, nd, dd));
    __syncthreads();
    const unsigned total = (unsigned)B * sh * sw * sd;         // <= B H W D < 2^31
    const long ivol = (long)H * W * D;
    float acc = 0.f;
    for (unsigned e = tid; e < total; e += NT) {
        unsigned q = e;
        const int id = (int)(q % (unsigned)sd); q /= (unsigned)sd;
        const int iw = (int)(q % (unsigned)sw); q /= (unsigned)sw;
        const int ih = (int)(q % (unsigned)sh);
        const int b = (int)(q / (unsigned)sh);
        const float g = dy[((long)b * Cin + ci) * ivol + ((long)(hlo + ih) * W + (wlo + iw)) * D + (dlo + id)];
        acc += ((wt[ih] * wt[sh + iw]) * wt[sh + sw + id]) * g;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (NT > 64) {
        if ((tid & 63) == 0) wsum[tid >> 6] = acc;
        __syncthreads();
        acc = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
    if (tid == 0) dp[blockIdx.x] = scale[0] * acc;
}

bool shape_ok(int B, int Cin, int H, int W, int D, int gh, int gw, int gd) {
    if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || D <= 0 || gh <= 0 || gw <= 0 || gd <= 0) return false;
    if (gh > H || gw > W || gd > D) return false;
    if (H + W + D > MAX_AXES_SUM) return false;
    return (long)B * Cin * H * W * D < (1L << 31);
}

int max_support(int n, int g) {
    int num, den, best = 0;
    axis_ratio(n, g, num, den);
    for (int k = 0; k < g; ++k) {
        int lo, hi;
        node_range(k, n, num, den, lo, hi);
        if (hi - lo + 1 > best) best = hi - lo + 1;
    }
    return best;
}

}  // namespace

extern "C" int mivp_input_prompt_fwd(const float* x, const float* p, const float* scale, int32_t B, int32_t Cin, int32_t H,
                                     int32_t W, int32_t D, int32_t gh, int32_t gw, int32_t gd, float* y, mivp_stream_t stream) {
    MIVP_REQUIRE(x && p && scale && y);
    MIVP_REQUIRE(shape_ok(B, Cin, H, W, D, gh, gw, gd));
    const long elems = (long)B * Cin * H * W * D;
    const bool a16 = ((uintptr_t)x | (uintptr_t)y) % 16 == 0, a8 = ((uintptr_t)x | (uintptr_t)y) % 8 == 0;
    const int V = (D % 4 == 0 && a16) ? 4 : ((D % 2 == 0 && a8) ? 2 : 1);
    const size_t lat_bytes = (size_t)Cin * gh * gw * gd * sizeof(float);
    const bool in_lds = lat_bytes <= (size_t)LATTICE_LDS_BYTES;
    const size_t lds = (size_t)(H + W + D) * 8 + (in_lds ? lat_bytes : 0);
    const long want = (elems / V + 255) / 256;
    const unsigned grid = (unsigned)(want > 4096 ? 4096 : want);
#define IP_LAUNCH(VV, LL) hipLaunchKernelGGL((k_input_prompt_fwd<VV, LL>), dim3(grid), dim3(256), lds, (hipStream_t)stream, x, p, \
                                             scale, (int)B, (int)Cin, (int)H, (int)W, (int)D, (int)gh, (int)gw, (int)gd, y)
    if (V == 4) { if (in_lds) IP_LAUNCH(4, true); else IP_LAUNCH(4, false); }
    else if (V == 2) { if (in_lds) IP_LAUNCH(2, true); else IP_LAUNCH(2, false); }
    else { if (in_lds) IP_LAUNCH(1, true); else IP_LAUNCH(1, false); }
#undef IP_LAUNCH
    return mivp_check_launch("input_prompt_fwd");
}

extern "C" int mivp_input_prompt_bwd(const float* dy, const float* scale, int32_t B, int32_t Cin, int32_t H, int32_t W,
                                     int32_t D, int32_t gh, int32_t gw, int32_t gd, float* dp, mivp_stream_t stream) {
    MIVP_REQUIRE(dy && scale && dp);
    MIVP_REQUIRE(shape_ok(B, Cin, H, W, D, gh, gw, gd));
    const long nodes = (long)Cin * gh * gw * gd;
    const int sh = max_support(H, gh), sw = max_support(W, gw), sd = max_support(D, gd);
    const long support = (long)B * sh * sw * sd;
#define IP_ARGS dy, scale, (int)B, (int)Cin, (int)H, (int)W, (int)D, (int)gh, (int)gw, (int)gd, dp
    if (support <= 64) {
        hipLaunchKernelGGL(k_input_prompt_bwd_node, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, IP_ARGS);
    } else {
        const size_t lds = (size_t)(sh + sw + sd) * sizeof(float);
        if (support < 4096)
            hipLaunchKernelGGL((k_input_prompt_bwd_group<64>), dim3((unsigned)nodes), dim3(64), lds, (hipStream_t)stream, IP_ARGS);
        else
            hipLaunchKernelGGL((k_input_prompt_bwd_group<256>), dim3((unsigned)nodes), dim3(256), lds, (hipStream_t)stream, IP_ARGS);
    }
#undef IP_ARGS
    return mivp_check_launch("input_prompt_bwd");
}
