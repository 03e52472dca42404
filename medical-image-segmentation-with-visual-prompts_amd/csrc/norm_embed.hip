// Patch embedding (Conv3d k=s=2) and training-mode BatchNorm3d pieces on channels-last bf16.
// Reference: swin_unetr/swin_unetr.py:148-158 (input_layer), :229-237 (head BatchNorm),
// swin_unetr/unet_blocks.py:41-45,74 (norm_concat).  All of these are HBM-bound: 16-byte
// accesses, per-thread fp32 partials, LDS atomics per workgroup, deterministic final reduction.
#include "common.hpp"

// ---------------------------------------------------------------------------------------------
// patch embedding: y[b,h,w,d,co] = bias[co] + sum_{ci,a,b,c} x[b,ci,2h+a,2w+b,2d+c] * w[co,ci,a,b,c]
//   work item = (output voxel, group of 8 output channels); total threads is a multiple of C/8 so a
//   thread keeps one channel group for its whole grid-stride walk.
//   mode 0: per-channel sum / sum of squares -> part[block][2C]     mode 1: affine + bf16 store
// ---------------------------------------------------------------------------------------------
template <int mode, bool CIN1>
__global__ __launch_bounds__(256, CIN1 ? 8 : 4) void k_patch_embed(MivpEmbedDesc d, const float* __restrict__ x,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     float* __restrict__ part, bf16_t* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = d.C, Cin = CIN1 ? 1 : d.Cin, G = C / 8;     // CIN1: the CT configurations, offsets fold into immediates
    // weights in LDS as [channel group][8 channels][Cin*8 taps], group stride padded by 4 floats: the (at most G) distinct
    // groups of a wave read different banks, all lanes of one group broadcast.  Keeping them out of registers leaves
    // the kernel at 8 waves/SIMD, which is what hides the latency of the strided x loads.
    const int gstride = 64 * Cin + 4;
    float* wl = reinterpret_cast<float*>(smem);               // [G][gstride]
    float* lsum = wl + G * gstride;                            // [256 * 16] reduction scratch
    const int tid = threadIdx.x;
    for (int i = tid; i < C * Cin * 8; i += 256) {
        const int g = i / (64 * Cin);
        wl[g * gstride + (i - g * 64 * Cin)] = w[i];
    }
    __syncthreads();
    const int H = d.dims[0], W = d.dims[1], D = d.dims[2];
    const int oh = H / 2, ow = W / 2, od = D / 2;
    const long ovol = (long)oh * ow * od, ivol = (long)H * W * D;
    const long items = (long)d.B * ovol * G;
    const long gtid = (long)blockIdx.x * 256 + tid;
    const long stride = (long)gridDim.x * 256;
    const int cg = (int)(gtid % G);
    const float* wg = wl + cg * gstride;
    float s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
    const unsigned uovol = (unsigned)ovol, uwd = (unsigned)(ow * od);      // host checks items < 2^31: 32-bit decode
    for (long it = gtid; it < items; it += stride) {
        const unsigned vox = (unsigned)it / (unsigned)G;
        const unsigned b = vox / uovol;
        unsigned rem = vox - b * uovol;
        const int h = (int)(rem / uwd);
        rem -= (unsigned)h * uwd;
        const int ww = (int)(rem / (unsigned)od);
        const int z = (int)(rem - (unsigned)ww * (unsigned)od);
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = bias[cg * 8 + i];
        asm volatile("" ::: "memory");                            // keep the weight reads in the loop (LICM would pin 64 VGPRs)
        for (int ci = 0; ci < Cin; ++ci) {
            const float* xb = x + ((long)b * Cin + ci) * ivol + ((long)(2 * h) * W + 2 * ww) * D + 2 * z;
            const float2 x00 = *reinterpret_cast<const float2*>(xb);
            const float2 x01 = *reinterpret_cast<const float2*>(xb + D);
            const float2 x10 = *reinterpret_cast<const float2*>(xb + (long)W * D);
            const float2 x11 = *reinterpret_cast<const float2*>(xb + (long)W * D + D);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 wa = *reinterpret_cast<const float4*>(wg + (i * Cin + ci) * 8);
                const float4 wb = *reinterpret_cast<const float4*>(wg + (i * Cin + ci) * 8 + 4);
                acc[i] += x00.x * wa.x + x00.y * wa.y + x01.x * wa.z + x01.y * wa.w +
                          x10.x * wb.x + x10.y * wb.y + x11.x * wb.z + x11.y * wb.w;
                if (i & 1) __builtin_amdgcn_sched_barrier(0);    // at most two channels' weights in flight
            }
        }
        if (mode == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { s1[i] += acc[i]; s2[i] += acc[i] * acc[i]; }
        } else {
            bf16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (bf16_t)(acc[i] * scale[cg * 8 + i] + shift[cg * 8 + i]);
            st8(y + (long)vox * C + cg * 8, o);
        }
    }
    if (mode == 0) block_reduce_groups(lsum, s1, s2, G, C, (long)blockIdx.x * 256, part + (long)blockIdx.x * 2 * C);
}

extern "C" int mivp_patch_embed(const MivpEmbedDesc* d, int mode, const float* x, const float* w, const float* bias,
                                const float* scale, const float* shift, float* part, void* y, mivp_stream_t stream) {
    MIVP_REQUIRE(d && x && w && bias);
    MIVP_REQUIRE(d->C % 8 == 0 && d->Cin > 0 && d->nblk > 0);
    MIVP_REQUIRE(d->dims[0] % 2 == 0 && d->dims[1] % 2 == 0 && d->dims[2] % 2 == 0);
    MIVP_REQUIRE((d->nblk * 256) % (d->C / 8) == 0);
    MIVP_REQUIRE(mode == 0 ? part != nullptr : (y && scale && shift));
    MIVP_REQUIRE((long)d->B * (d->dims[0] / 2) * (d->dims[1] / 2) * (d->dims[2] / 2) * (d->C / 8) < (1L << 31));   // 32-bit decode
    const size_t lds = ((size_t)(d->C / 8) * (64 * d->Cin + 4) + 256 * 16) * sizeof(float);
#define PE_LAUNCH(M, S) hipLaunchKernelGGL((k_patch_embed<M, S>), dim3(d->nblk), dim3(256), lds, (hipStream_t)stream, *d, x, w, \
                                           bias, scale, shift, part, (bf16_t*)y)
    if (mode == 0) { if (d->Cin == 1) PE_LAUNCH(0, true); else PE_LAUNCH(0, false); }
    else           { if (d->Cin == 1) PE_LAUNCH(1, true); else PE_LAUNCH(1, false); }
#undef PE_LAUNCH
    return mivp_check_launch("patch_embed");
}

// im2col of the k=s=2 patches (they tile the input exactly): p[tok][ci*8 + a*4 + b*2 + c] = x[b,ci,2h+a,2w+b,2d+c]
// in bf16 -- the B operand of mivp_gemm_tn for the patch-embedding weight gradient (columns in nn.Conv3d order).
__global__ __launch_bounds__(256) void k_patch_im2col(MivpEmbedDesc d, const float* __restrict__ x, bf16_t* __restrict__ p) {
    const int Cin = d.Cin, H = d.dims[0], W = d.dims[1], D = d.dims[2];
    const int oh = H / 2, ow = W / 2, od = D / 2;
    const long ovol = (long)oh * ow * od, ivol = (long)H * W * D;
    const long items = (long)d.B * ovol * Cin * 4;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const int ab = (int)(it & 3);
        const unsigned r = (unsigned)(it >> 2);                    // host checks items < 2^31
        const unsigned vox = r / (unsigned)Cin;
        const int ci = (int)(r - vox * (unsigned)Cin);
        const unsigned b = vox / (unsigned)ovol;
        unsigned rem = vox - b * (unsigned)ovol;
        const int h = (int)(rem / (unsigned)(ow * od));
        rem -= (unsigned)h * (unsigned)(ow * od);
        const int ww = (int)(rem / (unsigned)od);
        const int z = (int)(rem - (unsigned)ww * (unsigned)od);
        const float2 xv = *reinterpret_cast<const float2*>(x + ((long)b * Cin + ci) * ivol + ((long)(2 * h + (ab >> 1)) * W + (2 * ww + (ab & 1))) * D + 2 * z);
        bf16_t* o = p + (long)vox * (Cin * 8) + ci * 8 + ab * 2;
        o[0] = (bf16_t)xv.x;
        o[1] = (bf16_t)xv.y;
    }
}

extern "C" int mivp_patch_im2col(const MivpEmbedDesc* d, const float* x, void* p, mivp_stream_t stream) {
    MIVP_REQUIRE(d && x && p && d->Cin > 0);
    MIVP_REQUIRE(d->dims[0] % 2 == 0 && d->dims[1] % 2 == 0 && d->dims[2] % 2 == 0);
    const long items = (long)d->B * (d->dims[0] / 2) * (d->dims[1] / 2) * (d->dims[2] / 2) * d->Cin * 4;
    MIVP_REQUIRE(items < (1L << 31));                            // 32-bit decode
    const unsigned grid = (unsigned)((items + 255) / 256 > 8192 ? 8192 : (items + 255) / 256);
    hipLaunchKernelGGL(k_patch_im2col, dim3(grid), dim3(256), 0, (hipStream_t)stream, *d, x, (bf16_t*)p);
    return mivp_check_launch("patch_im2col");
}

// ---------------------------------------------------------------------------------------------
// patch embedding, data gradient: dx[b,ci,2h+a,2w+b,2d+c] = sum_co w[co,ci,a,b,c] * dz[b,h,w,d,co]
//   kernel == stride: the 2x2x2 patches tile the input, so one thread owns one output voxel of dz and writes its eight
//   input voxels per input channel -- every dx element exactly once, no atomics, no zero fill, one summation order
//   (co ascending, fp32).  A lane reads its voxel's C bf16 as 16-byte pieces; the weights are the same for every lane,
//   so they sit in LDS as [ci][co][8 taps] and every ds_read_b128 is one address for the whole wave (a broadcast, no
//   bank conflict, no padding).  In registers they would be 8 C values per thread; in LDS the kernel stays at 8 waves
//   per SIMD, which is what hides the latency of the 96-byte-strided dz loads.  Stores are float2 along D, four rows
//   per (voxel, ci); lanes are consecutive along d, so a wave writes contiguous runs.
//   Cin > 1 walks the channels inside the item and re-reads the voxel's dz from L1 (CIN1: read once).
// ---------------------------------------------------------------------------------------------
template <bool CIN1>
__global__ __launch_bounds__(256) void k_patch_embed_dgrad(MivpEmbedDesc d, const bf16_t* __restrict__ dz,
                                                           const float* __restrict__ w, float* __restrict__ dx) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = d.C, Cin = CIN1 ? 1 : d.Cin, G = C / 8;
    float* wl = reinterpret_cast<float*>(smem);               // [Cin][C][8]
    const int tid = threadIdx.x;
    for (int i = tid; i < C * Cin * 8; i += 256) {
        const int r = i >> 3, co = r / Cin, ci = r - co * Cin;
        wl[(ci * C + co) * 8 + (i & 7)] = w[i];
    }
    __syncthreads();
    const int H = d.dims[0], W = d.dims[1], D = d.dims[2];
    const int oh = H / 2, ow = W / 2, od = D / 2;
    const long ovol = (long)oh * ow * od, ivol = (long)H * W * D;
    const long items = (long)d.B * ovol;
    const long stride = (long)gridDim.x * 256;
    const unsigned uovol = (unsigned)ovol, uwd = (unsigned)(ow * od);      // host checks items < 2^31: 32-bit decode
    for (long it = (long)blockIdx.x * 256 + tid; it < items; it += stride) {
        const unsigned vox = (unsigned)it;
        const unsigned b = vox / uovol;
        unsigned rem = vox - b * uovol;
        const int h = (int)(rem / uwd);
        rem -= (unsigned)h * uwd;
        const int ww = (int)(rem / (unsigned)od);
        const int z = (int)(rem - (unsigned)ww * (unsigned)od);
        const bf16_t* zp = dz + (long)vox * C;
        float* xb = dx + (long)b * Cin * ivol + ((long)(2 * h) * W + 2 * ww) * D + 2 * z;
        for (int ci = 0; ci < Cin; ++ci) {
            const float* wc = wl + ci * C * 8;
            float acc[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) acc[t] = 0.f;
            for (int g = 0; g < G; ++g) {
                const bf16x8 v = ld8(zp + g * 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float f = (float)v[i];
                    const float4 wa = *reinterpret_cast<const float4*>(wc + (g * 8 + i) * 8);
                    const float4 wb = *reinterpret_cast<const float4*>(wc + (g * 8 + i) * 8 + 4);
                    acc[0] += f * wa.x; acc[1] += f * wa.y; acc[2] += f * wa.z; acc[3] += f * wa.w;
                    acc[4] += f * wb.x; acc[5] += f * wb.y; acc[6] += f * wb.z; acc[7] += f * wb.w;
                }
            }
            float* xc = xb + (long)ci * ivol;
            *reinterpret_cast<float2*>(xc) = make_float2(acc[0], acc[1]);
            *reinterpret_cast<float2*>(xc + D) = make_float2(acc[2], acc[3]);
            *reinterpret_cast<float2*>(xc + (long)W * D) = make_float2(acc[4], acc[5]);
            *reinterpret_cast<float2*>(xc + (long)W * D + D) = make_float2(acc[6], acc[7]);
        }
    }
}

extern "C" int mivp_patch_embed_dgrad(const MivpEmbedDesc* d, const void* dz, const float* w, float* dx, mivp_stream_t stream) {
    MIVP_REQUIRE(d && dz && w && dx);
    MIVP_REQUIRE(d->C > 0 && d->C % 8 == 0 && d->Cin > 0 && d->B > 0 && d->nblk > 0);
    MIVP_REQUIRE(d->dims[0] > 0 && d->dims[1] > 0 && d->dims[2] > 0);
    MIVP_REQUIRE(d->dims[0] % 2 == 0 && d->dims[1] % 2 == 0 && d->dims[2] % 2 == 0);
    MIVP_REQUIRE((long)d->B * (d->dims[0] / 2) * (d->dims[1] / 2) * (d->dims[2] / 2) * (d->C / 8) < (1L << 31));   // 32-bit decode
    const size_t lds = (size_t)d->C * d->Cin * 8 * sizeof(float);
    MIVP_REQUIRE(lds <= 64 * 1024);
    const long items = (long)d->B * (d->dims[0] / 2) * (d->dims[1] / 2) * (d->dims[2] / 2);
    const long want = (items + 255) / 256;
    const unsigned grid = (unsigned)(want < d->nblk ? want : d->nblk);   // nblk caps the grid; the walk strides beyond it
    if (d->Cin == 1)
        hipLaunchKernelGGL((k_patch_embed_dgrad<true>), dim3(grid), dim3(256), lds, (hipStream_t)stream, *d, (const bf16_t*)dz, w, dx);
    else
        hipLaunchKernelGGL((k_patch_embed_dgrad<false>), dim3(grid), dim3(256), lds, (hipStream_t)stream, *d, (const bf16_t*)dz, w, dx);
    return mivp_check_launch("patch_embed_dgrad");
}

// ---------------------------------------------------------------------------------------------
// BatchNorm statistics of a bf16 [n_vox][C] tensor
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_stats(const bf16_t* __restrict__ x, long n_vox, int C,
                                                  float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lsum = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, G = C / 8;
    const long items = n_vox * G;
    const long gtid = (long)blockIdx.x * 256 + tid;
    const long stride = (long)gridDim.x * 256;
    float s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
    for (long it = gtid; it < items; it += stride) {
        const bf16x8 v = ld8(x + it * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float f = (float)v[i]; s1[i] += f; s2[i] += f * f; }
    }
    block_reduce_groups(lsum, s1, s2, G, C, (long)blockIdx.x * 256, part + (long)blockIdx.x * 2 * C);
}

extern "C" int mivp_bn_stats(const void* x, int64_t n_vox, int32_t C, int32_t nblk, float* part, mivp_stream_t stream) {
    MIVP_REQUIRE(x && part && n_vox > 0 && C % 8 == 0 && nblk > 0);
    MIVP_REQUIRE((nblk * 256) % (C / 8) == 0);
    hipLaunchKernelGGL(k_bn_stats, dim3(nblk), dim3(256), 256 * 16 * sizeof(float), (hipStream_t)stream, (const bf16_t*)x,
                       (long)n_vox, (int)C, part);
    return mivp_check_launch("bn_stats");
}

// part [nblk][2C] -> batch mean / biased var -> scale, shift ; running stats (unbiased var) ; mean_rstd
// one 256-thread workgroup per channel: threads stride over the partial blocks in double precision (with 1024 partial rows
// every load of a thread is in flight at once: one memory round trip instead of two to four for a single wave), a butterfly
// per wave, then the four wave sums in wave order (fixed order: bit-reproducible)
__global__ __launch_bounds__(256) void k_bn_finalize(const float* __restrict__ part, int nblk, int C, double count,
                                                     const float* __restrict__ w, const float* __restrict__ b, float eps,
                                                     float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                     float* __restrict__ scale, float* __restrict__ shift,
                                                     float* __restrict__ mean_rstd) {
    __shared__ double wsum[4][2];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double s1 = 0.0, s2 = 0.0;
    int i = tid;
    for (; i + 256 * 3 < nblk; i += 256 * 4) {                   // 8 independent loads per round trip, same summation order
        float v1[4], v2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { v1[u] = part[(long)(i + 256 * u) * 2 * C + c]; v2[u] = part[(long)(i + 256 * u) * 2 * C + C + c]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s1 += (double)v1[u]; s2 += (double)v2[u]; }
    }
    for (; i < nblk; i += 256) { s1 += (double)part[(long)i * 2 * C + c]; s2 += (double)part[(long)i * 2 * C + C + c]; }
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if (lane == 0) { wsum[wv][0] = s1; wsum[wv][1] = s2; }
    __syncthreads();
    if (tid != 0) return;
    s1 = (wsum[0][0] + wsum[1][0]) + (wsum[2][0] + wsum[3][0]);
    s2 = (wsum[0][1] + wsum[1][1]) + (wsum[2][1] + wsum[3][1]);
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = (w ? w[c] : 1.f) * rstd;
    scale[c] = sc;
    shift[c] = (b ? b[c] : 0.f) - (float)mean * sc;
    if (mean_rstd) { mean_rstd[c] = (float)mean; mean_rstd[C + c] = rstd; }
    if (rmean && rvar) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mean;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
    }
}

extern "C" int mivp_bn_finalize(const float* part, int32_t nblk, int32_t C, double count, const float* w, const float* b,
                                float eps, float momentum, float* running_mean, float* running_var, float* scale,
                                float* shift, float* mean_rstd, mivp_stream_t stream) {
    MIVP_REQUIRE(part && scale && shift && nblk > 0 && C > 0 && count > 0);
    hipLaunchKernelGGL(k_bn_finalize, dim3(C), dim3(256), 0, (hipStream_t)stream, part, (int)nblk, (int)C, count,
                       w, b, eps, momentum, running_mean, running_var, scale, shift, mean_rstd);
    return mivp_check_launch("bn_finalize");
}

__global__ __launch_bounds__(256) void k_affine_act(const bf16_t* __restrict__ x, long n_vox, int C,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    int lrelu, bf16_t* __restrict__ y) {
    // the launch guarantees (gridDim.x * 256) % (C/8) == 0: a thread keeps one channel group, constants in registers
    const int G = C / 8;
    const long items = n_vox * G;
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    const int cg = (int)(gtid % G);
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { sc[i] = scale[cg * 8 + i]; sh[i] = shift[cg * 8 + i]; }
    for (long it = gtid; it < items; it += stride) {
        const bf16x8 v = ld8(x + it * 8);
        bf16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float f = (float)v[i] * sc[i] + sh[i];
            if (lrelu) f = f > 0.f ? f : 0.01f * f;
            o[i] = (bf16_t)f;
        }
        st8(y + it * 8, o);
    }
}

extern "C" int mivp_affine_act(const void* x, int64_t n_vox, int32_t C, const float* scale, const float* shift,
                               int32_t lrelu, void* y, mivp_stream_t stream) {
    MIVP_REQUIRE(x && y && scale && shift && n_vox > 0 && C % 8 == 0);
    const unsigned grid = fixed_group_grid(n_vox * (C / 8), C / 8, 4096);
    hipLaunchKernelGGL(k_affine_act, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (long)n_vox, (int)C,
                       scale, shift, (int)lrelu, (bf16_t*)y);
    return mivp_check_launch("affine_act");
}

// ---------------------------------------------------------------------------------------------
// BatchNorm backward (training mode): z = x*scale + shift, y = act(z)
//   dz = dy * act'(z) ; sums: S1 = sum dz, S2 = sum dz * xhat ; xhat = (x - mean) * rstd
//   dx = scale * (dz - S1/n - xhat * S2/n)        (scale = gamma * rstd)
//   dgamma = S2, dbeta = S1
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bn_bwd_stats(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                      long n_vox, int C, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, const float* __restrict__ mean_rstd,
                                                      int lrelu, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lsum = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, G = C / 8;
    const long items = n_vox * G;
    const long gtid = (long)blockIdx.x * 256 + tid;
    const long stride = (long)gridDim.x * 256;
    const int cg = (int)(gtid % G);
    float s1[8], s2[8], sc[8], sh[8], mu[8], rs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s1[i] = 0.f; s2[i] = 0.f;
        sc[i] = scale[cg * 8 + i]; sh[i] = shift[cg * 8 + i];
        mu[i] = mean_rstd[cg * 8 + i]; rs[i] = mean_rstd[C + cg * 8 + i];
    }
    for (long it = gtid; it < items; it += stride) {
        const bf16x8 xv = ld8(x + it * 8), gv = ld8(dy + it * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float xf = (float)xv[i];
            float gz = (float)gv[i];
            if (lrelu && xf * sc[i] + sh[i] <= 0.f) gz *= 0.01f;
            s1[i] += gz;
            s2[i] += gz * (xf - mu[i]) * rs[i];
        }
    }
    block_reduce_groups(lsum, s1, s2, G, C, (long)blockIdx.x * 256, part + (long)blockIdx.x * 2 * C);
}

extern "C" int mivp_bn_bwd_stats(const void* x, const void* dy, int64_t n_vox, int32_t C, const float* scale,
                                 const float* shift, const float* mean_rstd, int32_t lrelu, int32_t nblk, float* part,
                                 mivp_stream_t stream) {
    MIVP_REQUIRE(x && dy && scale && shift && mean_rstd && part && n_vox > 0 && C % 8 == 0 && nblk > 0);
    MIVP_REQUIRE((nblk * 256) % (C / 8) == 0);
    hipLaunchKernelGGL(k_bn_bwd_stats, dim3(nblk), dim3(256), 256 * 16 * sizeof(float), (hipStream_t)stream,
                       (const bf16_t*)x, (const bf16_t*)dy, (long)n_vox, (int)C, scale, shift, mean_rstd, (int)lrelu, part);
    return mivp_check_launch("bn_bwd_stats");
}

__global__ __launch_bounds__(256) void k_bn_bwd_apply(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                      long n_vox, int C, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, const float* __restrict__ mean_rstd,
                                                      const float* __restrict__ sums, int lrelu, bf16_t* __restrict__ dx) {
    // fixed channel group per thread (see k_affine_act): dx = a*gz + b*x + c with per-channel a, b, c
    const int G = C / 8;
    const long items = n_vox * G;
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)gridDim.x * 256;
    const int cg = (int)(gtid % G);
    const float inv_n = 1.0f / (float)n_vox;
    float sc[8], sh[8], ca[8], cb[8], cc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = cg * 8 + i;
        sc[i] = scale[c]; sh[i] = shift[c];
        const float mu = mean_rstd[c], rs = mean_rstd[C + c];
        const float k2 = sums[C + c] * inv_n * rs;          // xhat * S2/n = (x - mu) * k2
        ca[i] = sc[i];
        cb[i] = -sc[i] * k2;
        cc[i] = sc[i] * (mu * k2 - sums[c] * inv_n);
    }
    for (long it = gtid; it < items; it += stride) {
        const bf16x8 xv = ld8(x + it * 8), gv = ld8(dy + it * 8);
        bf16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float xf = (float)xv[i];
            float gz = (float)gv[i];
            if (lrelu && xf * sc[i] + sh[i] <= 0.f) gz *= 0.01f;
            o[i] = (bf16_t)(ca[i] * gz + cb[i] * xf + cc[i]);
        }
        st8(dx + it * 8, o);
    }
}

extern "C" int mivp_bn_bwd_apply(const void* x, const void* dy, int64_t n_vox, int32_t C, const float* scale,
                                 const float* shift, const float* mean_rstd, const float* sums, int32_t lrelu, void* dx,
                                 mivp_stream_t stream) {
    MIVP_REQUIRE(x && dy && scale && shift && mean_rstd && sums && dx && n_vox > 0 && C % 8 == 0);
    const unsigned grid = fixed_group_grid(n_vox * (C / 8), C / 8, 4096);
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy,
                       (long)n_vox, (int)C, scale, shift, mean_rstd, sums, (int)lrelu, (bf16_t*)dx);
    return mivp_check_launch("bn_bwd_apply");
}
