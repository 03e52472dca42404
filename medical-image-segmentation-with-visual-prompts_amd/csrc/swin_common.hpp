// What the Swin sources swin_fwd.hip, swin_bwd.hip, swin_bwd_fused.hip, swin_tok_wide.hip and swin_fwd_fp8.hip share
// (DESIGN 4), written once: the prototypes of the functions they call across files, the device helpers more than one of
// them uses, and the host dispatch on a channel-tile count (the transposing LDS read tr_read, which the
// convolution sources use too, is in common.hpp).  Device helpers are inlined into the kernels that call them;
// no kernel and no entry point lives here.
#pragma once
#include "common.hpp"

// swin_fwd.hip: which (NT, DKS = DVT) attention instantiation covers this shape (forward and backward dispatch)
int mivp_attn_tile_config(const MivpSwinDesc* d, int* dks, int* nt);
// swin_tok_wide.hip: the row-image token kernels of C = 48 / 96 / 192 / 384, called by the C entries of swin_fwd.hip and
// swin_bwd.hip when mivp_tok_wide_supported() (the QKV pair) / mivp_tok_rows_supported() (the proj + MLP pair)
int mivp_tok_wide_supported(const MivpSwinDesc* d);
int mivp_tok_rows_supported(const MivpSwinDesc* d);
long mivp_tok_natural_offset(int C);
int mivp_tok_wide_qkv_fwd(const MivpSwinDesc* d, const void* x, const int32_t* tok_src, const float* ln_w, const float* ln_b,
                          const void* wqkv, void* q, void* k, void* v, hipStream_t st);
int mivp_tok_wide_proj_mlp_fwd(const MivpSwinDesc* d, const void* o, const void* x, const int32_t* tok_src, const int32_t* tok_dst,
                               const void* wproj, const float* bproj, const float* ln_w, const float* ln_b, const void* wmlp,
                               const float* bmlp, void* t1_out, void* y, hipStream_t st);
int mivp_tok_wide_proj_mlp_bwd(const MivpSwinDesc* d, const void* dy, const int32_t* tok_dst, const void* t1, const float* ln_w,
                               const void* wmlp_t, const void* wproj_t, void* d_o, void* d_t1, hipStream_t st);
int mivp_tok_wide_qkv_bwd(const MivpSwinDesc* d, const void* dq, const void* dk, const void* dv, const void* x, const int32_t* tok_src,
                          const float* ln_w, const void* wqkv_t, const void* d_t1, void* dx, void* dn_out, hipStream_t st);

namespace {

// Token t of the [B][P][Nqp] window order: batch b, window pw, slot; bp = b * P + pw.  T = B * P * Nqp fits 32 bits (checked
// on the host), so the divisions are 32-bit ones; a dead token (t >= T) decodes as token 0: its addresses are valid.
struct TokInfo { long tt, bp, b; int slot, pw; bool live; };
MIVP_DEV TokInfo token_info(const MivpSwinDesc& d, long t) {
    TokInfo ti;
    const long T = (long)d.B * d.P * d.Nqp;
    ti.live = t < T;
    const unsigned tu = ti.live ? (unsigned)t : 0u;
    const unsigned bpu = tu / (unsigned)d.Nqp;
    ti.tt = tu;
    ti.bp = bpu;
    ti.slot = (int)(tu - bpu * (unsigned)d.Nqp);
    ti.pw = (int)(bpu % (unsigned)d.P);
    ti.b = bpu / (unsigned)d.P;
    return ti;
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
MIVP_DEV f32x4 mfma16k16(bf16x4 a, bf16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}

// LDS-DMA staging: one 4-byte global -> LDS transfer per lane (LDS address = wave-uniform base + 4 * lane)
MIVP_DEV void glds4(const void* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}
// LDS image of 32-byte rows, the two 16-byte halves swapped in rows 8..15 of every 16 (conflict-free 8-byte reads)
MIVP_DEV int row32_off(int row, int byte) { return row * 32 + (byte ^ (((row >> 3) & 1) << 4)); }

// Host dispatch on a channel-tile count (or a channel count): calls f(std::integral_constant<int, V>) for the V of the list
// equal to `value`; false when the list holds no such V (the caller reports its own unsupported-shape message)
template <int... Vs, class F>
bool for_tile_count(int value, F&& f) {
    return ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// the 16-token kernels of swin_fwd.hip / swin_bwd.hip: CT = ceil(C / 16)
template <class F>
bool for_tok16_ct(int ct, F&& f) { return for_tile_count<1, 2, 3, 4, 6, 8, 12>(ct, f); }

}  // namespace
