/*
 * mivp.h -- C ABI of the MI355X-native (gfx950) Swin-UNETR hot path.
 *
 * Drop-in boundary: the reference has no FFI of its own -- its
 * hot path is eager PyTorch inside `SwinUnetR.forward` -- so these entry points
 * are what a binding from the reference's Python would call (ctypes stub in
 * INTEGRATION.md).  Each entry cites the reference lines it replaces (paths
 * relative to /root/reference/src/modules).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless it is a descriptor struct;
 *  - activations are bf16, channels-last `[B, H, W, D, C]` ("NDHWC");
 *  - parameters arrive as bf16 (GEMM weights, `[out][in]` row-major like
 *    nn.Linear.weight) or fp32 (norm scale/shift, biases);
 *  - no allocation, no host sync, no global state inside any call: the caller
 *    owns every buffer (torch allocations in the Python host) and passes the
 *    HIP stream to launch on; calls are thread-compatible;
 *  - return 0 on success, negative MIVP_E* on error; nothing throws.
 *
 * Window index tables (`tok_src`, `tok_dst`, `tok_rid`) are immutable per
 * (dims, window, shift) and are built by the host exactly as SURVEY Appendix
 * A.1 states (swin_transformer/swin_block.py:145-178,247-253,292-364):
 *    tok_src[P*Nqp]  voxel offset (h*W+w)*D+d inside one volume of x that feeds
 *                    token (window, slot); -1 = zero-pad token; -2 = slot >= Nq
 *    tok_dst[P*Nqp]  voxel offset in the block OUTPUT that the token writes; -1 = cropped
 *    tok_rid[P*Nqp]  int32 region id of the token for the shift mask
 * with Nqp = Nq rounded up to 16.
 */
#ifndef MIVP_H
#define MIVP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mivp_stream_t;     /* hipStream_t */

#define MIVP_OK            0
#define MIVP_EINVAL       -1     /* bad argument / shape contract violated          */
#define MIVP_EUNSUPPORTED -2     /* shape outside the instantiated kernel set       */
#define MIVP_ELAUNCH      -3     /* hipLaunch reported an error                     */

/* library identity: returns the ABI version (bumped on any signature change) */
int mivp_abi_version(void);
/* last HIP error string for MIVP_ELAUNCH (static storage, never NULL) */
const char* mivp_last_error(void);

/* ------------------------------------------------------------------------ */
/* Swin block (swin_block.py:145-255, window_attention.py:35-61)             */
/* ------------------------------------------------------------------------ */
typedef struct MivpSwinDesc {
    int32_t B;          /* batch                                              */
    int32_t C;          /* channels, multiple of 8                            */
    int32_t heads;      /* C % heads == 0, (C/heads) % 4 == 0                  */
    int32_t vol_in;     /* H*W*D of the block input  (voxels per volume)       */
    int32_t vol_out;    /* H*W*D of the block output (== vol_in)               */
    int32_t P;          /* windows per volume                                  */
    int32_t Nq;         /* tokens per window                                   */
    int32_t Nqp;        /* Nq rounded up to 16                                 */
    int32_t Np;         /* prompt tokens (0 = none)                            */
    int32_t Npp;        /* rows of the prompt K/V buffers (>= Np, multiple of 16) */
    int32_t Nkp;        /* key rows the attention kernel sees: multiple of 32, >= Nqp+Npp */
    int32_t aug;        /* bias augmentation dims  w0 + w1 + (w2-1)            */
    int32_t augp;       /* aug rounded up to 4                                 */
    int32_t has_mask;   /* 1 for a shifted block                               */
    int32_t win[3];     /* window size per axis                                */
    float   q_scale;    /* head_dim ** -0.5                                    */
    float   ln_eps;     /* 1e-6                                                */
    /* dropout of the training forward (window_attention.py:30,33,57,60): an element is dropped when the   */
    /* 16-bit counter hash of its index under `seed` is below `thr` (= round(p * 65536), 0 = no dropout);   */
    /* kept elements are scaled by `scale` = 65536 / (65536 - thr).  Backward re-derives the same mask.     */
    uint32_t attn_drop_thr;   float attn_drop_scale;   uint32_t attn_seed;
    uint32_t proj_drop_thr;   float proj_drop_scale;   uint32_t proj_seed;
    /* ABI 12: optional DEVICE pointer to one 32-bit epoch word (NULL = none).  Every dropout kernel uses the seeds      */
    /* seed + epoch[0] * 0x9E3779B1: a recorded HIP graph freezes this descriptor (a kernel argument), so a replay draws */
    /* a fresh mask by incrementing the word in device memory at the start of the graph; forward and backward kernels of */
    /* one step read the same value.                                                                                     */
    const uint32_t* seed_epoch;
} MivpSwinDesc;

/* Weight fragment images (ABI 9).  The four token kernels below read their GEMM weights as MFMA-fragment-major images:
 *   [ceil(rows / 16) row tiles][k_steps][64 lanes][8] bf16, zero padded; lane 16 g + r of (row tile nt, k-step s) holds
 *   W[16 nt + r][32 s + 8 g .. + 8]  ("natural"), or W[..][32 s + 4 g .. + 4] | W[..][32 s + 16 + 4 g .. + 4] ("paired": the k
 *   order of a GEMM whose B operand is the previous GEMM's accumulator tile pair).  A wave's A fragment is then one
 *   contiguous 1 KB load.  k_steps = ceil(cols / 32), except wqkv_t: ceil(3 * 16 * ceil(C / 16) / 32).
 *   mivp_pack_weight_frags builds one image from a row-major [rows][cols] bf16 matrix (out: ceil(rows/16) * k_steps * 512
 *   elements).  Images per entry:
 *     mivp_swin_qkv_fwd       wqkv    = natural image of [3C][C]
 *     mivp_swin_proj_mlp_fwd  wproj   = natural image of [C][C];  wmlp = paired image of [C][C], and for C in {48, 96, 192,
 *                                       384} the natural image directly behind it (the row-image kernels of those widths
 *                                       feed the second GEMM from LDS in natural k order; dropout calls use the paired one)
 *     mivp_swin_proj_mlp_bwd  wmlp_t  = natural image of Wmlp^T;  wproj_t = paired (+ natural, as above) image of Wproj^T
 *     mivp_swin_qkv_bwd       wqkv_t  = natural image of Wqkv^T [C][3C]
 *   (mivp_prompt_kv_fwd / _bwd keep the row-major wqkv.)                                                                  */
int mivp_pack_weight_frags(const void* w, int32_t rows, int32_t cols, int32_t k_steps, int32_t paired, void* out,
                           mivp_stream_t stream);
/* Every image of one Swin block in one launch, from the f32 [C][C] masters of to_q, to_k, to_v, proj and mlp
 * (swin_block.py:60-80).  Outputs bf16, any may be NULL: wqkv_rm [3C][C] row-major (for mivp_prompt_kv_fwd / _bwd),
 * wqkv_f, wproj_f, wmlp_f, wqkv_t, wmlp_t, wproj_t exactly as the table above; with_natural != 0 appends the natural images
 * behind the paired ones of wmlp_f / wproj_t (element offset ceil(C/16) * ceil(C/32) * 512).                            */
int mivp_pack_block_weights(int32_t C, const float* wq, const float* wk, const float* wv, const float* wproj,
                            const float* wmlp, int32_t with_natural, void* wqkv_rm, void* wqkv_f, void* wproj_f,
                            void* wmlp_f, void* wqkv_t, void* wmlp_t, void* wproj_t, mivp_stream_t stream);

/* gather + LayerNorm + q/k/v projections  (swin_block.py:205-214, window_attention.py:42-47)
 *   x [B, vol_in, C] bf16;  ln_w, ln_b [C] f32;  wqkv = fragment image of [3C][C] (to_q, to_k, to_v stacked), see above
 *   q, k, v [B*P][heads][Nqp][hd] bf16 ; q is pre-multiplied by q_scale ; slots >= Nq are zero.
 *   k is stored multiplied by log2(e): the attention kernels keep logits in log2 units so that S = K'Q'^T feeds
 *   v_exp_f32 directly (the gradient entries below still take / return dk w.r.t. the un-scaled k).           */
int mivp_swin_qkv_fwd(const MivpSwinDesc* d, const void* x, const int32_t* tok_src,
                      const float* ln_w, const float* ln_b, const void* wqkv,
                      void* q, void* k, void* v, mivp_stream_t stream);

/* prompt tokens -> LayerNorm -> to_k / to_v, once per block
 *   prompt [Np][C] f32 (the nn.Parameter) -> kp, vp [heads][Npp][hd] bf16 (rows >= Np zero; kp x log2(e) like k)
 *   yln [Np][C] f32: the normalised prompt, saved for backward                            */
int mivp_prompt_kv_fwd(const MivpSwinDesc* d, const float* prompt, const float* ln_w, const float* ln_b,
                       const void* wqkv, void* kp, void* vp, float* yln, mivp_stream_t stream);

/* prompt-token bias scores and their gradients (relative_positional_encoding.py:128-135):
 *   ts[h][t] = scale * sum_k W[h][k] * E[t][k]   (W = weights_token [heads][e], E = enc_token rows [Np][e], all f32)
 *   dW[h][k] = scale * sum_t dts[h][t] E[t][k],  dE[t][k] = scale * sum_h dts[h][t] W[h][k]                       */
int mivp_token_scores_fwd(const float* W, const float* E, int32_t heads, int32_t np, int32_t e, float scale, float* ts,
                          mivp_stream_t stream);
int mivp_token_scores_bwd(const float* dts, const float* W, const float* E, int32_t heads, int32_t np, int32_t e, float scale,
                          float* dW, float* dE, mivp_stream_t stream);
/* Batched forms for prompt tuning (n <= 16 blocks per call, arrays of n host-side entries): every one of these kernels lasts
 * 5-10 us whatever it computes, and a step runs one per prompted block.  mivp_prompt_kv_fwd_multi also writes the token bias
 * ts into the prompt rows of each block's K'-augmentation image ka[i] (an image mivp_relbias_aug produced with ts = 0: with
 * frozen content tables the rest of it is constant), so mivp_relbias_aug leaves the per-step path of those blocks. */
int mivp_token_scores_fwd_multi(int32_t n, const float* const* W, const float* const* E, const int32_t* heads, const int32_t* np,
                                int32_t e, const float* scale, float* const* ts, mivp_stream_t stream);
int mivp_token_scores_bwd_multi(int32_t n, const float* const* dts /* entries may be NULL */, const float* const* W,
                                const float* const* E, const int32_t* heads, const int32_t* np, int32_t e, const float* scale,
                                float* const* dW, float* const* dE, mivp_stream_t stream);
int mivp_prompt_kv_fwd_multi(int32_t n, const MivpSwinDesc* d, const float* const* prompt, const float* const* ln_w,
                             const float* const* ln_b, const void* const* wqkv, const float* const* ts, void* const* kp,
                             void* const* vp, void* const* ka, mivp_stream_t stream);

/* relative-position bias as MFMA augmentation dims (relative_positional_encoding.py:99-142)
 *   t_h [heads][2*w0-1], t_w, t_d: per-axis relative tables  T_a[h][j-i+w_a-1] = s/3 * W_a[h] . E_a[...]
 *   (scale embed_dim**-0.5 and the /3 already applied by the host), ts [heads][Np] f32 prompt-token
 *   scores (scaled), or NULL when Np == 0.
 *   Because the bias is a sum of three terms that each depend on ONE slot coordinate of the query, it
 *   equals <onehot(query coords), table values at the key coords>: the kernel emits that as extra K
 *   columns of the QK^T MFMA:   qa [Nqp][augp] bf16 (query one-hots),  ka [heads][Nkp][augp] bf16 (x log2(e)).
 *   Padding key rows (Nq..Nqp-1 and the unused prompt rows) carry -30000 in the w0 query-h columns: every valid query
 *   sees that logit there, P underflows to exactly 0 and the attention kernels never test for padding keys.      */
int mivp_relbias_aug(const MivpSwinDesc* d, const float* t_h, const float* t_w, const float* t_d,
                     const float* ts, void* qa, void* ka, mivp_stream_t stream);

/* softmax((q k^T + bias) * mask) v per (window, head)  (window_attention.py:49-59)
 *   o [B*P][Nqp][C] bf16 (heads merged, channel = head*hd + j) ; lse [B*P][heads][Nqp] f32 (natural log; may be NULL
 *   when no backward pass will follow -- ABI 11)
 *   tok_rid [P][Nqp] int32: shift-mask region id of every window slot, 0 <= id < 254 (27 regions in 3D)
 *   mask_words / cut_flags (ABI 12, shifted blocks only; both may be NULL: the kernel then compares tok_rid classes per
 *   logit): the shift mask of swin_block.py:187-200,312-364 precomputed per window geometry as lane masks.
 *   mask_words [P][Nqp/16 query tiles][Nqp/16 key tiles][4] uint64: bit 16 g + r of word j of (window pw, query tile qt, key
 *   tile kt) is set when the logit of query slot 16 qt + r and key slot 16 kt + 4 g + j SURVIVES the multiplicative mask
 *   (same region id; key rows >= Nq always survive -- they are excluded by their bias); query rows >= Nq carry class 0.
 *   cut_flags [P] uint8: 1 when the window's content slots hold more than one region id (the others skip the mask).
 *   The kernels load the words with scalar loads and apply each as ONE v_cndmask per logit.                         */
int mivp_win_attn_fwd(const MivpSwinDesc* d, const void* q, const void* k, const void* v,
                      const void* kp, const void* vp, const void* qa, const void* ka,
                      const int32_t* tok_rid, void* o, float* lse, const uint64_t* mask_words,
                      const uint8_t* cut_flags, mivp_stream_t stream);

/* proj + residual, drop prompts, LayerNorm + Linear + residual, scatter + crop
 * (window_attention.py:60, swin_block.py:221-253)
 *   t1 [B*P][Nqp][C] bf16 (saved for backward, may be NULL) ; y [B, vol_out, C] bf16
 *   wproj, wmlp: weight fragment images (see "Weight fragment images" above) */
int mivp_swin_proj_mlp_fwd(const MivpSwinDesc* d, const void* o, const void* x,
                           const int32_t* tok_src, const int32_t* tok_dst,
                           const void* wproj, const float* bproj, const float* ln_w, const float* ln_b,
                           const void* wmlp, const float* bmlp, void* t1, void* y, mivp_stream_t stream);

/* ---- backward of the block: data gradients + prompt / token-bias gradients ---- */
/* dy [B, vol_out, C] bf16 -> dO [B*P][Nqp][C] bf16 and dt1 [B*P][Nqp][C] bf16
 *   wmlp_t, wproj_t = fragment images of mlp.weight^T, proj.weight^T  ([in][out] -> rows are input channels)
 *   weight-gradient mode (both or neither, else NULL): dn_out [B*P][Nqp][C] bf16 = gradient w.r.t. the
 *   mlp_norm output, dyw [B*P][Nqp][C] bf16 = dy in window order (zero rows where the token was cropped) */
int mivp_swin_proj_mlp_bwd(const MivpSwinDesc* d, const void* dy, const int32_t* tok_dst, const void* t1,
                           const float* ln_w, const float* ln_b, const void* wmlp_t, const void* wproj_t,
                           void* d_o, void* d_t1, void* dn_out, void* dyw, void* d_pj, mivp_stream_t stream);
/*   d_pj (NULL unless proj dropout is on in weight-gradient mode): dt1 with the proj-dropout mask applied,
 *   i.e. the gradient w.r.t. the proj output (A operand of the proj weight gradient) */

/* delta[bp][head][n] = sum_j dO * O  (flash-attention backward row term) */
int mivp_win_attn_delta(const MivpSwinDesc* d, const void* o, const void* d_o, float* delta,
                        mivp_stream_t stream);

/* EXPERIMENTAL E4M3 variant of mivp_win_attn_fwd for head_dim < 16 without dropout (BASELINE.json configs[4]): same
 * operands and outputs; Q', K', V and P are converted to fp8 inside the kernel (csrc/swin_fwd_fp8.hip).  Measured against the
 * bf16 kernel in profiles/r02_fp8_attention.json; not used by the model unless mivp_amd.swin_ops.USE_FP8_ATTN_FWD is set. */
int mivp_win_attn_fwd_fp8(const MivpSwinDesc* d, const void* q, const void* k, const void* v,
                          const void* kp, const void* vp, const void* qa, const void* ka,
                          const int32_t* tok_rid, void* o, float* lse, mivp_stream_t stream);

/* query-owner pass: dq [B*P][heads][Nqp][hd] bf16 (w.r.t. the stored, pre-scaled q).
 * Also WRITES delta [B*P][heads][Nqp] (= mivp_win_attn_delta) for the key-owner pass that follows. */
int mivp_win_attn_bwd_dq(const MivpSwinDesc* d, const void* q, const void* k, const void* v,
                         const void* kp, const void* vp, const void* qa, const void* ka,
                         const int32_t* tok_rid, const void* o, const void* d_o, const float* lse, float* delta,
                         void* dq, mivp_stream_t stream);

/* ONE-PASS attention backward for head_dim <= 16 (every encoder stage, the last decoder stage): dq, dk, dv and the prompt
 * partials of the two passes above from a single launch that forms S, dP and the exponentials once per (query, key) pair
 * (csrc/swin_bwd_fused.hip; autograd of window_attention.py:49-61 with the prompt keys of swin_block.py:187-225).
 * Same operand layouts as mivp_win_attn_bwd_dq / _dkv; delta is computed internally.  mivp_win_attn_bwd_fused_supported
 * returns 1 when the shape is covered (otherwise use the two-pass entries). */
int mivp_win_attn_bwd_fused_supported(const MivpSwinDesc* d);
int mivp_win_attn_bwd_fused(const MivpSwinDesc* d, const void* q, const void* k, const void* v,
                            const void* kp, const void* vp, const void* qa, const void* ka,
                            const int32_t* tok_rid, const void* o, const void* d_o, const float* lse,
                            void* dq, void* dk, void* dv, float* dkp_part, float* dvp_part, float* dtok_part,
                            mivp_stream_t stream);

/* Prompt-only attention backward for the first prompted block behind a frozen stem (no data gradient there): the prompt
 * keys' per-window partials dkp_part / dvp_part / dtok_part exactly as mivp_win_attn_bwd_dkv writes them, from one launch
 * that also forms delta (head_dim <= 16, Npp / 16 in {1, 2, 4, 8}; mivp_win_attn_bwd_prompt_supported tells). */
int mivp_win_attn_bwd_prompt_supported(const MivpSwinDesc* d);
int mivp_win_attn_bwd_prompt(const MivpSwinDesc* d, const void* q, const void* kp, const void* vp, const void* qa,
                             const void* ka, const void* o, const void* d_o, const float* lse, float* dkp_part,
                             float* dvp_part, float* dtok_part, mivp_stream_t stream);

/* key-owner pass: dk, dv [B*P][heads][Nqp][hd] bf16 for window keys;
 *   dkp_part, dvp_part [B*P][heads][Npp][hd] f32 and dtok_part [B*P][heads][Npp] f32:
 *   per-window partial sums for the prompt keys (reduced by mivp_reduce_rows)            */
int mivp_win_attn_bwd_dkv(const MivpSwinDesc* d, const void* q, const void* k, const void* v,
                          const void* kp, const void* vp, const void* qa, const void* ka,
                          const int32_t* tok_rid, const void* d_o, const float* lse, const float* delta,
                          void* dk, void* dv, float* dkp_part, float* dvp_part, float* dtok_part,
                          float* dka_part, mivp_stream_t stream);
/*   dka_part (NULL or f32 [B*P][heads][Nkp][32]): per-window gradient of the key-side bias augmentation
 *   columns (mivp_relbias_aug's ka); summed over windows and folded by mivp_relbias_grad into the
 *   gradients of the three relative-position tables (relative_positional_encoding.py:99-142)       */
int mivp_relbias_grad(const MivpSwinDesc* d, const float* dka /* [heads][Nkp][32] */, float* d_th, float* d_tw,
                      float* d_td, mivp_stream_t stream);

/* dq,dk,dv -> (x W^T backward) -> LayerNorm backward -> + dt1 -> scatter to dx [B, vol_in, C] bf16
 *   wqkv_t = fragment image of the stacked weight transposed [C][3C]; q part is multiplied by q_scale inside
 *   dn_out (NULL or [B*P][Nqp][C] bf16): gradient w.r.t. the attn_norm output (weight-gradient mode) */
int mivp_swin_qkv_bwd(const MivpSwinDesc* d, const void* dq, const void* dk, const void* dv,
                      const void* x, const int32_t* tok_src, const float* ln_w, const float* ln_b,
                      const void* wqkv_t, const void* d_t1, void* dx, void* dn_out, mivp_stream_t stream);

/* prompt K/V gradients -> through to_k/to_v and LayerNorm -> dprompt [Np][C] f32
 *   dkp, dvp [heads][Npp][hd] f32 (already reduced over windows) ; wqkv [3C][C] bf16
 *   weight-gradient mode (all three or NULL): wg_a [2][Np][C] bf16 = dK rows then dV rows (head-merged),
 *   wg_n [Np][C] bf16 = attn_norm(prompt), wg_ln [2][Np][C] f32 = per-row dbeta terms then dgamma terms */
int mivp_prompt_kv_bwd(const MivpSwinDesc* d, const float* dkp, const float* dvp, const float* prompt,
                       const float* ln_w, const float* ln_b, const void* wqkv, float* dprompt,
                       void* wg_a, void* wg_n, float* wg_ln, mivp_stream_t stream);

/* test hook: the keep masks the kernels derive from the descriptor's dropout fields, 1 = kept.
 *   attn_keep u8 [B*P*heads][Nqp][Nkp] (NULL to skip), proj_keep u8 [B*P*Nqp][C] (NULL to skip) */
int mivp_dropout_masks(const MivpSwinDesc* d, uint8_t* attn_keep, uint8_t* proj_keep, mivp_stream_t stream);

/* out[r] = sum_i in[i][r]  for i < n, r < rows  (deterministic two-level tree) */
int mivp_reduce_rows(const float* in, int64_t n, int64_t rows, float* out, mivp_stream_t stream);
/* the same for up to four arrays that share n (the prompt-gradient partials of one block), one launch:
 * out[i][r] = sum_k in[i][k*rows[i] + r];  in / rows / out are HOST arrays of nseg entries */
int mivp_reduce_rows_multi(int32_t nseg, const float* const* in, const int64_t* rows, float* const* out, int64_t n,
                           mivp_stream_t stream);


/* ------------------------------------------------------------------------ */
/* Patch merging (swin_transformer/down.py:21-53)                           */
/* ------------------------------------------------------------------------ */
typedef struct MivpMergeDesc {
    int32_t B, C;               /* input channels (multiple of 8)                      */
    int32_t dims[3];            /* input H, W, D                                       */
    int32_t odims[3];           /* output dims                                         */
    int32_t merge_last;         /* 1: 2x2x2 -> 8C ; 0: 2x2x1 -> 4C                     */
    int32_t Cout;               /* output channels                                     */
    float   ln_eps;
} MivpMergeDesc;
/* x [B,H,W,D,C] bf16 -> y [B,oh,ow,od,Cout] bf16 ; w [Cout][kC] bf16 ; ln over kC */
int mivp_patch_merge_fwd(const MivpMergeDesc* d, const void* x, const float* ln_w, const float* ln_b,
                         const void* w, void* y, mivp_stream_t stream);
/* dy -> dx ; w_t [kC][Cout] bf16; yfwd = the forward output [T][Cout] bf16; wgam[n] = sum_c W[n][c]*gamma[c] and
 * wbet[n] = sum_c W[n][c]*beta[c] (f32 [Cout], W = the bf16 weight): the LayerNorm-backward row sums follow from
 * dy, yfwd and these two vectors without a second GEMM.
 *   weight-gradient mode (both or NULL): wg_dn, wg_x [T][kC] bf16 = gradient w.r.t. the LayerNorm output and the
 *   gathered LayerNorm input rows */
int mivp_patch_merge_bwd(const MivpMergeDesc* d, const void* dy, const void* x, const void* yfwd, const float* ln_w,
                         const float* ln_b, const float* wgam, const float* wbet, const void* w_t, void* dx,
                         void* wg_dn, void* wg_x, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* 3x3x3 stride-1 pad-1 convolution as implicit GEMM                         */
/* (swin_unetr.py:87,229-237,260-266; unet_blocks.py:46-56,74)              */
/* ------------------------------------------------------------------------ */
typedef struct MivpConvDesc {
    int32_t B;
    int32_t dims[3];            /* H, W, D (same for input and output)                 */
    int32_t Cin;                /* multiple of 8                                       */
    int32_t Cout;               /* real output channels                                */
    int32_t Kp;                 /* 27*Cin rounded up to 32 = row length of w           */
    int32_t pro_affine;         /* 1: x' = x*scale[ci] + shift[ci] on in-bounds voxels */
    int32_t pro_lrelu;          /* 1: then LeakyReLU(0.01)                             */
    int32_t add_residual;       /* 1: y += residual (bf16, same shape as y)            */
    int32_t out_f32;            /* 1: y is fp32 [B,vol,Cout], else bf16                */
} MivpConvDesc;
/* x [B,H,W,D,Cin] bf16 ; w [Cout_p][Kp] bf16 with k = tap*Cin + ci, tap = (kh*3+kw)*3+kd,
 * rows >= Cout and columns >= 27*Cin zero (Cout_p = Cout rounded up to 16) ; bias [Cout] f32 or NULL */
int mivp_conv3d_fwd(const MivpConvDesc* d, const void* x, const void* w, const float* bias,
                    const float* scale, const float* shift, const void* residual, void* y,
                    void* workspace, size_t ws_bytes, mivp_stream_t stream);
/* bytes of f32 split-K workspace the call above wants for this shape (0 = none).  Few voxels with a very
 * long K (bottleneck, first decoder stages) cannot fill 256 CUs by voxel tiles alone: K is cut into slices
 * that write f32 partials, summed in a fixed order by an epilogue kernel.  Passing NULL runs unsplit. */
size_t mivp_conv3d_fwd_ws(const MivpConvDesc* d);

/* The same convolution for LARGE volumes with few output channels (conv_concat of the last decoder stage,
 * unet_blocks.py:46-56,74): a workgroup stages the 6x10x18 (6x6x18) input halo of a 4x8x16 (4x4x16) output brick once per
 * 16-channel chunk in LDS instead of fetching every voxel once per tap.
 *   supported: bf16 output, Cin % 16 == 0, Cout % 4 == 0, Cout <= 48 or a multiple of 48
 *   wh: bf16 [groups][Cin/16][14][BN][32]: groups of 48 output channels (BN = 48, or Cout rounded to 16 when there is
 *       one group), k-step j = taps (2j, 2j+1) x 16 channels of the chunk, tap 27 = zeros */
int mivp_conv3d_halo_supported(const MivpConvDesc* d);
int mivp_conv3d_halo_fwd(const MivpConvDesc* d, const void* x, const void* wh, const float* bias,
                         const float* scale, const float* shift /* prologue, NULL unless d->pro_affine */,
                         const void* residual /* NULL unless d->add_residual */, void* y, int32_t brick_w /* 8: 4x8x16 bricks, 8 waves; 4: 4x4x16 bricks, 4 waves; 6: 6x6x16 bricks, 12 waves; 66: 6x6x8 and 36: 3x6x8 bricks of 2x8-voxel tiles (6 / 3 waves) */, mivp_stream_t stream);
/* Segmentation-head forward (swin_unetr.py:229-237): y = conv3x3x3(x * scale + shift) + bias for 27*Cout <= 64
 * (Cout <= 2), Cin + 1 <= 64.  x [B,H,W,D,Cin] bf16 (pre-BatchNorm), w f32 [Cout][Cin][3][3][3] (the nn.Conv3d
 * weight as stored), scale/shift f32 [Cin] (BatchNorm as an affine), y f32 [B,H,W,D,Cout].
 * Per-voxel GEMM to the 27*Cout tap outputs on MFMA + 27-point gather through LDS (csrc/head.hip). */
size_t mivp_head_conv_ws(void);            /* bytes of workspace (the folded bf16 weight tile) */
int mivp_head_conv_fwd(const MivpConvDesc* d, const void* x, const float* w, const float* bias,
                       const float* scale, const float* shift, void* workspace, float* y, mivp_stream_t stream);

/* weight + bias gradient for small Cout (segmentation heads, Cout <= 8):
 *   dwdb [Cout*27*Cin + Cout] f32 : dw[co][tap][ci] = sum_v dy[v][co] * x'[v+tap][ci] followed by db[co]
 *   (x' = the operand the forward conv saw, i.e. after the fused scale/shift/activation);
 *   dy [B,vol,dy_stride] bf16 with dy_stride >= Cout channels per voxel ; per-workgroup partial sums
 *   land in part[] (mivp_conv3d_wgrad_small_ws(d) floats) and are reduced deterministically.        */
size_t mivp_conv3d_wgrad_small_ws(const MivpConvDesc* d);
int mivp_conv3d_wgrad_small(const MivpConvDesc* d, const void* x, const float* scale, const float* shift,
                            const void* dy, int32_t dy_stride, float* part, float* dwdb,
                            mivp_stream_t stream);

/* MFMA form of the same gradient (what the product uses): gs [3][80][64] f32 with, for the tap
 * (sh, sw, sd) in {-1,0,1}^3, nb = (sh+1)*3 + (sw+1):
 *   gs[sd+1][nb*8 + co][c]   = sum_u dy[u - tap][co] * x[u][c]          (raw x, no affine)   for c < Cin
 *   gs[sd+1][nb*8 + co][Cin] = sum_{u in bounds} dy[u - tap][co]
 * dy carries 8 channels (dy_stride == 8, zero padded), Cout <= 8, Cin % 8 == 0, Cin < 64.  The conv weight
 * gradient, its bias gradient and the gradients of a BatchNorm fused in front of the conv are linear
 * functions of gs.  `_ws` = number of f32 partial values the call needs in `part`. */
size_t mivp_conv3d_wgrad_rows_ws(const MivpConvDesc* d);
int mivp_conv3d_wgrad_rows(const MivpConvDesc* d, const void* x, const void* dy, int32_t dy_stride,
                           float* part, float* gs, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Patch embedding + BatchNorm statistics (swin_unetr.py:148-158)            */
/* ------------------------------------------------------------------------ */
typedef struct MivpEmbedDesc {
    int32_t B, Cin;
    int32_t dims[3];            /* input H, W, D (fp32, channels-first [B,Cin,H,W,D])  */
    int32_t C;                  /* output channels, multiple of 8                      */
    int32_t nblk;               /* stats blocks: rows of `part`                        */
} MivpEmbedDesc;
/* mode 0: accumulate per-channel sum / sum-of-squares of conv(x)+bias into part [nblk][2C] f32
 * mode 1: y = (conv(x)+bias) * scale + shift -> bf16 [B,h,w,d,C]                        */
int mivp_patch_embed(const MivpEmbedDesc* d, int mode, const float* x, const float* w, const float* bias,
                     const float* scale, const float* shift, float* part, void* y, mivp_stream_t stream);
/* bf16 im2col of the 2x2x2 patches, p [B*(H/2)*(W/2)*(D/2)][Cin*8] with columns in nn.Conv3d.weight order:
 * the input-side operand of mivp_gemm_tn for the patch-embedding weight gradient */
int mivp_patch_im2col(const MivpEmbedDesc* d, const float* x, void* p, mivp_stream_t stream);
/* data gradient of the k = s = 2 convolution: dx[b,ci,2h+a,2w+b,2d+c] = sum_co w[co,ci,a,b,c] * dz[b,h,w,d,co]
 *   dz bf16 [B,H/2,W/2,D/2,C] (the BatchNorm backward's output for the recomputed conv output), w f32 nn.Conv3d weight,
 *   dx f32 [B,Cin,H,W,D]: every element written exactly once (no atomics, no zero fill), co ascending in fp32.
 *   Even dims, C % 8 == 0, C*Cin*32 bytes of LDS <= 64 KiB; nblk caps the grid (no channel-group rule here) */
int mivp_patch_embed_dgrad(const MivpEmbedDesc* d, const void* dz, const float* w, float* dx, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* BatchNorm3d, training mode (batch statistics), channels-last bf16         */
/* ------------------------------------------------------------------------ */
/* per-channel partial sums of a bf16 [n_vox][C] tensor -> part [nblk][2C] f32 */
int mivp_bn_stats(const void* x, int64_t n_vox, int32_t C, int32_t nblk, float* part, mivp_stream_t stream);
/* part -> mean/rstd -> scale = w*rstd, shift = b - mean*scale ; running stats updated in place
 * (momentum, unbiased variance) ; mean_rstd [2C] f32 saved for backward                 */
int mivp_bn_finalize(const float* part, int32_t nblk, int32_t C, double count, const float* w, const float* b,
                     float eps, float momentum, float* running_mean, float* running_var,
                     float* scale, float* shift, float* mean_rstd, mivp_stream_t stream);
/* y = act(x*scale + shift), bf16 -> bf16 (used where the consumer cannot fuse the affine) */
int mivp_affine_act(const void* x, int64_t n_vox, int32_t C, const float* scale, const float* shift,
                    int32_t lrelu, void* y, mivp_stream_t stream);
/* backward reductions: part [nblk][2C] : sum(dy), sum(dy * xhat) over voxels, where
 * dy is taken AFTER the activation derivative when lrelu=1 (z = x*scale+shift, dy *= z>0 ? 1 : 0.01) */
int mivp_bn_bwd_stats(const void* x, const void* dy, int64_t n_vox, int32_t C, const float* scale,
                      const float* shift, const float* mean_rstd, int32_t lrelu, int32_t nblk, float* part,
                      mivp_stream_t stream);
/* dx = scale * (dyz - sum_dy/n - xhat * sum_dy_xhat/n) ; sums [2C] f32 (already reduced) */
int mivp_bn_bwd_apply(const void* x, const void* dy, int64_t n_vox, int32_t C, const float* scale,
                      const float* shift, const float* mean_rstd, const float* sums, int32_t lrelu,
                      void* dx, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Trilinear upsample (align_corners=False) + crop + concat                  */
/* (unet_blocks.py:31-35,72-73; swin_unetr.py:351-355)                       */
/* ------------------------------------------------------------------------ */
typedef struct MivpUpcatDesc {
    int32_t B;
    int32_t idims[3];           /* low-res input dims                                  */
    int32_t odims[3];           /* output dims (= skip dims; <= scale*idims)            */
    int32_t scale[3];           /* 1 or 2 per axis                                     */
    int32_t Cx;                 /* channels of the low-res tensor                      */
    int32_t Cs;                 /* channels of the skip tensor (0 = no concat)         */
    int32_t align_corners;      /* 0: half-pixel centres (output_layer, SwinUpBlock); 1: align_corners=True  */
                                /*    (the reconstruction head's nn.Upsample, swin_unetr.py:199-201)          */
} MivpUpcatDesc;
/* x [B,ih,iw,id,Cx] bf16, skip [B,oh,ow,od,Cs] bf16 -> y [B,oh,ow,od,Cx+Cs] bf16 */
int mivp_upcat_fwd(const MivpUpcatDesc* d, const void* x, const void* skip, void* y, mivp_stream_t stream);
/* ABI 11: the concat tensor of SwinUpBlock (unet_blocks.py:72-75: up -> cat -> norm_concat -> act -> conv_concat) is
 * never stored un-normalised when nothing upstream needs a gradient:
 *   mivp_upcat_stats       per-channel sum / sum of squares of the bf16-rounded upsample + concat values ->
 *                          part [nblk][2*(Cx+Cs)] f32 in mivp_bn_stats' layout (mivp_bn_finalize reduces the nblk rows);
 *                          nblk = nx*B*oh with 1 <= nx <= ow (nx workgroups walk one (b, oh) line of output rows), Cx/8 <= 192 (256 without skip), Cs/8 <= 64, id*Cx/8 <= 2048
 *   mivp_upcat_affine_fwd  y = act(scale[c] * v + shift[c]) of the bf16-rounded concat value v (lrelu: slope 0.01),
 *                          bit-identical to mivp_upcat_fwd followed by mivp_affine_act                                  */
int mivp_upcat_stats(const MivpUpcatDesc* d, const void* x, const void* skip, int32_t nblk, float* part,
                     mivp_stream_t stream);
int mivp_upcat_affine_fwd(const MivpUpcatDesc* d, const void* x, const void* skip, const float* scale,
                          const float* shift, int32_t lrelu, void* y, mivp_stream_t stream);
/* dy [B,oh,ow,od,Cx+Cs] bf16 -> dx [B,ih,iw,id,Cx] bf16 (transposed stencil), dskip (slice copy; may be NULL) */
int mivp_upcat_bwd(const MivpUpcatDesc* d, const void* dy, void* dx, void* dskip, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Dice + focal loss of the downstream step (modules/segmentation.py:44-50)  */
/* ------------------------------------------------------------------------ */
/* logits f32 [B, vol, C] channels-last (C <= 8), target f32 [B, vol] class indices.
 * loss[0] = mean_bc dice_bc + mean focal (MONAI DiceFocalLoss(include_background, to_onehot_y, softmax,
 * gamma) as documented; class 0 dropped when include_background == 0); dlogits f32 [B, vol, C] = d loss / d logits.
 * workspace: mivp_dice_focal_ws(B, vol) floats.
 * dlogits may be NULL (ABI 10): the value pass alone; the gradient pass then runs when autograd asks for it,
 * mivp_dice_focal_grad on the SAME workspace (it holds the per-sample Dice sums), scaled by gscale[0] (device pointer to
 * the incoming d total / d loss, NULL = 1) inside the pass instead of a second sweep over the 28 MB gradient.
 * gamma < 0 (ABI 12): the Dice term ALONE -- MONAI DiceLoss(include_background, to_onehot_y, softmax) of the students /
 * teacher trainer's supervised modes (modules/students_teacher.py:96-100,190-197): loss[0] = mean_bc dice_bc, no sigmoid /
 * focal work in either pass.                                                                                          */
size_t mivp_dice_focal_ws(int32_t B, int64_t vol);
int mivp_dice_focal(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                    int32_t include_background, float gamma, float* workspace, float* loss, float* dlogits,
                    mivp_stream_t stream);
int mivp_dice_focal_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                         int32_t include_background, float gamma, float* workspace, const float* gscale, float* dlogits,
                         mivp_stream_t stream);

/* Tversky region term + weighted (focal) softmax cross-entropy with an ignore label (csrc/segloss.hip; mivp_amd/losses.py
 * SegLossSpec / seg_loss / SegLoss).  These entry points joined ABI 18 without a bump: they are additive and
 * no earlier signature changed.  Operands as for mivp_dice_focal: logits f32 [B, vol, C] channels-last (2 <= C <= 8),
 * target f32 [B, vol] class indices.  A voxel is VALID when its label is an integer in [0, C) and, with has_ignore != 0,
 * differs from ignore_index (compared as a float: exact for |ignore_index| < 2^24; has_ignore == 0: ignore_index is not
 * read).  An invalid voxel (ignored, non-integer, out of range, NaN) adds to no sum, gets an exactly zero gradient and
 * never selects a class weight.  With p = softmax_c(z), t = one-hot(label), sums over the valid voxels of a sample (of the
 * whole batch when batch != 0) and s = 1e-5:
 *   TI_c   = (2 I_c + s) / (2 I_c + 2 alpha (P_c - I_c) + 2 beta (T_c - I_c) + s),  I = sum p t, P = sum p, T = sum t
 *   region = mean over (b, c >= c0) [over c >= c0 when batch] of (1 - TI_c),        c0 = include_background ? 0 : 1
 *   voxel  = - sum_v w[y_v] (1 - p_y)^focal_gamma log p_y / sum_v w[y_v]   over the valid voxels of the whole batch, exactly 0
 *            (and a zero gradient) when sum_v w[y_v] == 0
 *   loss[0] = lambda_region region + lambda_voxel voxel
 * alpha, beta >= 0; focal_gamma == 0 or >= 1; lambda_region, lambda_voxel >= 0, not both 0; class_weights: DEVICE pointer
 * to C floats >= 0, NULL = all ones (the values are not read back to be checked).
 * workspace: mivp_seg_loss_ws(B, vol) floats = partial rows [B][bpb][26], the samples' rows [B][26], the batch-wide row [26]
 * (row: (I, P, T) x 8 classes, voxel numerator, voxel weight sum).  dlogits may be NULL: the value pass alone;
 * mivp_seg_loss_grad then runs the gradient pass on the SAME workspace with the SAME options, scaled by gscale[0] (device
 * pointer, NULL = 1); it writes every element of dlogits once.  No atomics: equal calls give equal bits. */
size_t mivp_seg_loss_ws(int32_t B, int64_t vol);
int mivp_seg_loss(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                  int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                  const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                  float lambda_voxel, float* workspace, float* loss, float* dlogits, mivp_stream_t stream);
int mivp_seg_loss_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                       int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                       const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                       float lambda_voxel, float* workspace, const float* gscale, float* dlogits,
                       mivp_stream_t stream);

/* The same region term + TOP-K (hard-voxel) cross-entropy (csrc/segtopk.hip; SegLossSpec(top_k=...)).  These
 * entry points joined ABI 18 without a bump: they are additive and no earlier signature changed.  Arguments, validity rule
 * and region term as for mivp_seg_loss, plus top_k in (0, 1] (lambda_voxel > 0 is required).  Over the valid voxels of the
 * whole batch:
 *   u_v   = w[y_v] (1 - p_y)^focal_gamma (-log p_y) >= 0,  N = their number,  k = max(1, floor(top_k N)) (in double)
 *   tau   = the k-th largest u_v as the statistics pass computed it in f32, n_gt = #{u > tau}, n_eq = #{u == tau}
 *   voxel = (sum_{u > tau} u + (k - n_gt) tau) / k                  (the mean of the k largest; 0 when N == 0)
 *   d voxel = (1 / k) sum_v s_v d u_v,  s_v = 1 where u_v > tau, rho = (k - n_gt) / n_eq where u_v == tau, 0 elsewhere:
 *   tied voxels share the remaining weight equally, whatever their place in memory.
 * The select is an exact three-level radix select (11 + 10 + 10 bits) over one 32-bit key per voxel: the bit pattern of
 * u_v clamped to >= +0 (monotone as an unsigned integer), 0xFFFFFFFF at an invalid voxel.  The statistics pass stores the
 * keys; every later pass, the gradient pass included, reads them back.  Only integer atomics; float sums in a fixed order:
 * equal calls give equal bits.  No host read, every launch unconditional (k and tau are device data), the call zeroes its
 * own histograms: recordable, and a recording holds for any later content.
 * workspace: mivp_seg_topk_ws(B, vol) 4-byte words, 16-byte aligned.  With R = mivp_seg_loss_ws(B, vol) rounded up to a
 * multiple of 4:
 *   [0, mivp_seg_loss_ws)                 the rows of mivp_seg_loss (the two voxel columns stay 0)
 *   [R, R + MIVP_SEG_TOPK_RECORD_WORDS)   the record: [0] N, [1] k, [2] tau (the key: f32 bits), [3] n_gt, [4] n_eq (uint32),
 *                                         [5] rho, [6] voxel (f32 bits); the other words are internal
 *   then the three histograms (2048, 1024, 1024 uint32) and 1024 f32 partial sums
 *   [R + MIVP_SEG_TOPK_KEYS_OFFSET, + B vol)   the keys (uint32), voxel order of the target
 * B vol < 2^31.  dlogits may be NULL; mivp_seg_topk_grad then runs the gradient pass on the SAME workspace with the SAME
 * options, scaled by gscale[0] (device pointer, NULL = 1), and writes every element of dlogits once. */
#define MIVP_SEG_TOPK_RECORD_WORDS 16
#define MIVP_SEG_TOPK_KEYS_OFFSET 5136
size_t mivp_seg_topk_ws(int32_t B, int64_t vol);
int mivp_seg_topk(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                  int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                  const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                  float lambda_voxel, double top_k, float* workspace, float* loss, float* dlogits, mivp_stream_t stream);
int mivp_seg_topk_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                       int32_t include_background, int32_t batch, float alpha, float beta, float focal_gamma,
                       const float* class_weights, int32_t ignore_index, int32_t has_ignore, float lambda_region,
                       float lambda_voxel, double top_k, float* workspace, const float* gscale, float* dlogits,
                       mivp_stream_t stream);

/* Boundary (signed-distance) loss term with batched on-device distance maps (csrc/distmap.hip; mivp_amd/losses.py
 * signed_distance_maps / boundary_loss / SegLossSpec(lambda_boundary=...)).  These entry points joined ABI 18
 * without a bump: they are additive and no earlier signature changed.
 *
 * mivp_distmap_signed: target f32 [B][H][W][D] class indices (dims = {H, W, D}, host) -> phi f32 [B][K][H][W][D], K = C - c0
 * classes c0 .. C - 1, c0 = include_background ? 0 : 1, 1 <= K <= 16.  Per (b, c), M = {label == c}; a label that is no class
 * (non-integer, outside [0, C), NaN, or, with has_ignore != 0, equal to ignore_index) belongs to no M.  With distances
 * sqrt(sum_a (spacing[a] delta_a)^2) (spacing: host f32 {s0, s1, s2}, finite and > 0) and the space beyond the volume border
 * neither inside nor outside:
 *   phi = distance to the nearest voxel of M                 at voxels outside M   (> 0)
 *   phi = -(distance to the nearest voxel outside M - 1)     at voxels inside M    (<= 0 at unit spacing)
 *   phi = +0 everywhere in (b, c)                            when M is empty or the whole sample
 * Four launches whatever B and K are (seed / D pass, W pass, H pass, closing), no atomics, nothing read back, every launch
 * unconditional: equal calls give equal bits, and a recording holds for any later content.  At unit spacing the squared
 * distances under the root are the exact integers (those of mivp_edt_sq).  Limits: H, W <= 65535 and B K H W D < 2^31.
 * workspace: mivp_distmap_ws(B, K, dims) bytes (0 for arguments the call would refuse), 256-byte aligned:
 *   [0, 8 B K vol)                 the squared fields f32 [2][B][K][vol]: side 0 = distance to M, side 1 = to its complement
 *   [that rounded up to 256, + 16 B K vol)   the lower envelope's stack, int32 pairs [depth][line]
 * reused by every call in stream order.
 *
 * mivp_boundary_loss: logits f32 [B, vol, C] channels-last (2 <= C <= 8), target f32 [B, vol], phi f32 [B][K][vol] (any
 * values; a constant of the step).  Validity rule of mivp_seg_loss.  With p = softmax_c(z), V the valid voxels of the batch,
 * N = |V|, w = lambda_boundary weight[0] (weight: DEVICE pointer to one float, NULL = 1; lambda_boundary >= 0):
 *   loss[0]   = w sum_{v in V} sum_{c >= c0} p_c phi_c / (K max(N, 1))
 *   dlogits_j = w p_j (phit_j - sum_c p_c phit_c) / (K max(N, 1)),   phit_c = phi_c for c >= c0, else 0;  exactly 0 at an
 *               invalid voxel
 * dlogits may be NULL: the value pass alone.  accumulate == 0: every element of dlogits is stored once; accumulate != 0: the
 * value is added to what dlogits holds (one rounded add per element: the bits of dlogits + g).  mivp_boundary_loss_grad runs
 * the gradient pass on the SAME workspace with the SAME options, scaled by gscale[0] (device pointer, NULL = 1).
 * workspace: mivp_boundary_loss_ws(B, vol) floats = partial rows [B][bpb][2] (sum p phi, valid voxels), then
 * {sum p phi, N, 1 / (K max(N, 1)), spare}.  No atomics: equal calls give equal bits. */
size_t mivp_distmap_ws(int32_t B, int32_t K, const int32_t* dims);
int mivp_distmap_signed(const float* target, int32_t B, int32_t C, int32_t include_background, int32_t ignore_index,
                        int32_t has_ignore, const int32_t* dims, const float* spacing, float* phi, void* workspace,
                        mivp_stream_t stream);
size_t mivp_boundary_loss_ws(int32_t B, int64_t vol);
int mivp_boundary_loss(const float* logits, const float* target, const float* phi, int32_t B, int64_t vol, int32_t C,
                       int32_t include_background, int32_t ignore_index, int32_t has_ignore, float lambda_boundary,
                       const float* weight, float* workspace, float* loss, float* dlogits, int32_t accumulate,
                       mivp_stream_t stream);
int mivp_boundary_loss_grad(const float* logits, const float* target, const float* phi, int32_t B, int64_t vol, int32_t C,
                            int32_t include_background, int32_t ignore_index, int32_t has_ignore, float lambda_boundary,
                            const float* weight, const float* workspace, const float* gscale, float* dlogits,
                            int32_t accumulate, mivp_stream_t stream);

/* Hausdorff distance-transform loss term (Karimi & Salcudean, IEEE TMI 2019, "HD_DT") with on-device distance fields of the
 * hard prediction and of the labels (csrc/hausdorff.hip; mivp_amd/losses.py hausdorff_weight_maps / hausdorff_dt_loss /
 * HausdorffDTLoss).  These entry points joined ABI 18 without a bump: they are additive and no earlier signature
 * changed.
 *
 * mivp_hausdorff_maps: logits f32 [B][vol][C] channels-last (2 <= C <= 8, vol = H W D), target f32 [B][H][W][D] class indices
 * (dims = {H, W, D}, host) -> wmap f32 [B][K][H][W][D], K = C - c0 classes c0 .. C - 1, c0 = include_background ? 0 : 1.  Per
 * (b, c) two masks:
 *   P = {argmax_j z_j == c}   the hard prediction: comparisons on the logits alone, the LOWEST index among exact maxima, at
 *                             every voxel, valid or not (NaN logits are out of contract)
 *   G = {label == c}          the rule of mivp_distmap_signed: a label that is no class (non-integer, outside [0, C), NaN, or,
 *                             with has_ignore != 0, equal to ignore_index) belongs to no G
 * field(M)(v) = the distance sqrt(sum_a (spacing[a] delta_a)^2) from v to the nearest voxel on the other side of M (to the
 * complement of M inside M, to M outside; the space beyond the volume border is neither side), +0 everywhere in (b, c) when M
 * is empty or the whole sample.
 *   wmap = field(P)^alpha + field(G)^alpha,   0 < alpha <= 4
 * alpha == 2: the sum of the two squared fields, no root and no pow taken (exact integers at unit spacing); any other alpha:
 * powf(squared field, alpha / 2) of each.  Four launches whatever B and K are (seed / D pass over both sources with the
 * argmax fused in, W pass, H pass, closing), no atomics, nothing read back, every launch unconditional: equal calls give equal
 * bits, and a recording holds for any later content.  Limits: H, W <= 65535 and 4 B K H W D < 2^31.
 * workspace: mivp_hausdorff_maps_ws(B, K, dims) bytes (0 for arguments the call would refuse), 256-byte aligned:
 *   [0, 16 B K vol)                the squared fields f32 [2][2][B][K][vol]: source (0 = P, 1 = G), then side (0 = distance to
 *                                  M, 1 = to its complement; +inf where that side has no voxel), those of mivp_edt_sq
 *   [that rounded up to 256, + 32 B K vol)   the lower envelope's stack, int32 pairs [depth][line]
 * reused by every call in stream order.
 *
 * mivp_hausdorff_loss: logits f32 [B, vol, C] channels-last (2 <= C <= 8), target f32 [B, vol], wmap f32 [B][K][vol] (any
 * values; a constant of the step: no gradient flows through it).  Validity rule of mivp_seg_loss.  With p = softmax_c(z),
 * g_c = [y == c], V the valid voxels of the batch, N = |V|, w = lambda_hausdorff weight[0] (weight: DEVICE pointer to one
 * float, NULL = 1; lambda_hausdorff >= 0):
 *   loss[0]   = w sum_{v in V} sum_{c >= c0} (p_c - g_c)^2 wmap_c / (K max(N, 1))
 *   dlogits_j = w p_j sum_c p_c (q_j - q_c) / (K max(N, 1)),   q_c = 2 (p_c - g_c) wmap_c for c >= c0, else 0;  exactly +0 at
 *               an invalid voxel
 * dlogits may be NULL: the value pass alone.  accumulate == 0: every element of dlogits is stored once; accumulate != 0: the
 * value is added to what dlogits holds (one rounded add per element: the bits of dlogits + g).  mivp_hausdorff_loss_grad runs
 * the gradient pass on the SAME workspace with the SAME options, scaled by gscale[0] (device pointer, NULL = 1).
 * workspace: mivp_hausdorff_loss_ws(B, vol) floats = partial rows [B][bpb][2] (the sum, valid voxels), then
 * {the sum, N, 1 / (K max(N, 1)), spare}.  No atomics: equal calls give equal bits. */
size_t mivp_hausdorff_maps_ws(int32_t B, int32_t K, const int32_t* dims);
int mivp_hausdorff_maps(const float* logits, const float* target, int32_t B, int32_t C, int32_t include_background,
                        int32_t ignore_index, int32_t has_ignore, const int32_t* dims, const float* spacing, float alpha,
                        float* wmap, void* workspace, mivp_stream_t stream);
size_t mivp_hausdorff_loss_ws(int32_t B, int64_t vol);
int mivp_hausdorff_loss(const float* logits, const float* target, const float* wmap, int32_t B, int64_t vol, int32_t C,
                        int32_t include_background, int32_t ignore_index, int32_t has_ignore, float lambda_hausdorff,
                        const float* weight, float* workspace, float* loss, float* dlogits, int32_t accumulate,
                        mivp_stream_t stream);
int mivp_hausdorff_loss_grad(const float* logits, const float* target, const float* wmap, int32_t B, int64_t vol, int32_t C,
                             int32_t include_background, int32_t ignore_index, int32_t has_ignore, float lambda_hausdorff,
                             const float* weight, const float* workspace, const float* gscale, float* dlogits,
                             int32_t accumulate, mivp_stream_t stream);

/* Lovasz-Softmax loss term (Berman, Triki & Blaschko, CVPR 2018) on an exact device-wide key sort (csrc/lovasz.hip,
 * csrc/sort_common.hpp; mivp_amd/losses.py lovasz_softmax_loss / LovaszSoftmaxLoss).  These entry points joined
 * ABI 18 without a bump: they are additive and no earlier signature changed.
 *
 * mivp_sort_u32: keys u32 [segments][n] (device) -> every segment sorted ascending in place, the bits of a stable sort (keys
 * only, so of any exact sort).  LSD radix sort, four passes of 8 bits, three launches each (tile histograms, scan, stable
 * scatter; the segment is a grid dimension): twelve launches whatever segments, n and the data are; no float arithmetic, no
 * global atomics.  mivp_sort_tile(): the keys one workgroup handles.  Limits: segments <= 65535, segments n < 2^31.
 * workspace: mivp_sort_u32_ws(segments, n) bytes (0 for arguments the call would refuse): the second key buffer, the tile
 * histograms [segments][tiles][256] and the digit bases [segments][256].
 *
 * mivp_lovasz_loss: logits f32 [B, vol, C] channels-last (2 <= C <= 8), target f32 [B, vol].  Validity rule of mivp_seg_loss.
 * A segment is class c >= c0 (c0 = include_background ? 0 : 1) of sample b (per_image != 0) or of the batch; S segments of N
 * voxels.  Per segment over its valid voxels, with p = softmax_c(z), g = [y == c], e = g ? 1 - p_c : p_c, G = sum g,
 * J(F, K) = 1 - (G - F) / (G + K) and J(0, 0) = 0:
 *   loss_seg  = sum_j e_(j) (J_j - J_(j-1))            the errors in descending order, F_j / K_j the foreground / background
 *                                                      voxels among the first j
 *   d loss_seg / d e_i, tie rule: inside a group of equal e the foreground voxels come first and get 1 / (G + K) each, K the
 *               background voxels with a larger error; the b tied background voxels share J(F, K + b) - J(F, K) equally, F the
 *               foreground voxels with an error >= theirs.  Independent of memory order, and a subgradient.
 * A group (a sample with per_image, else the batch) averages its segments with G > 0 (classes_all != 0: all of them; no
 * segment: 0); loss[0] = w x the mean of the groups, w = lambda_lovasz weight[0] (weight: DEVICE pointer to one float, NULL =
 * 1; lambda_lovasz >= 0).  dlogits_k = w sum_c factor_c s_c sgn_c p_c (delta_ck - p_k), exactly +0 at an invalid voxel.
 * dlogits may be NULL; accumulate and mivp_lovasz_loss_grad (gscale) as for mivp_hausdorff_loss.  Every launch is
 * unconditional and their number (20 with the gradient) depends on nothing; integer atomics only for the two counts per
 * segment: equal calls give equal bits, nothing is read back, a recording holds for any later content.
 * Limits: B <= 65535, S N < 2^31.  workspace: mivp_lovasz_ws(B, C, include_background, per_image, vol) bytes (0 for arguments
 * the call would refuse): sorted keys [S][N], the sort's workspace, prefix u32 [S][N] (foreground keys up to a position), tile
 * counts, counts u32 [S][2] = (G, valid voxels), partial sums f32 [S][tiles], factors f32 [S].
 *
 * mivp_lovasz_keys: the key pass alone.  keys u32 [S][N] in memory order: 0x7F000001 - ((bits(e) << 1) | g) at a valid voxel
 * (ascending keys = descending errors, foreground first), 0xFFFFFFFF at an invalid one; counts u32 [S][2]. */
int mivp_sort_tile(void);
size_t mivp_sort_u32_ws(int32_t segments, int64_t n);
int mivp_sort_u32(uint32_t* keys, int32_t segments, int64_t n, void* workspace, mivp_stream_t stream);
size_t mivp_lovasz_ws(int32_t B, int32_t C, int32_t include_background, int32_t per_image, int64_t vol);
int mivp_lovasz_keys(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, int32_t include_background,
                     int32_t ignore_index, int32_t has_ignore, int32_t per_image, uint32_t* keys, uint32_t* counts,
                     mivp_stream_t stream);
int mivp_lovasz_loss(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C, int32_t include_background,
                     int32_t ignore_index, int32_t has_ignore, int32_t per_image, int32_t classes_all, float lambda_lovasz,
                     const float* weight, void* workspace, float* loss, float* dlogits, int32_t accumulate,
                     mivp_stream_t stream);
int mivp_lovasz_loss_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t C,
                          int32_t include_background, int32_t ignore_index, int32_t has_ignore, int32_t per_image,
                          int32_t classes_all, float lambda_lovasz, const float* weight, const void* workspace,
                          const float* gscale, float* dlogits, int32_t accumulate, mivp_stream_t stream);

/* clDice (soft-skeleton) loss term (Shit et al., CVPR 2021) and the soft skeleton itself (csrc/cldice.hip; mivp_amd/losses.py
 * soft_skeleton / cldice_loss / SegLossSpec(lambda_cldice=...)).  These entry points joined ABI 18 without a
 * bump: they are additive and no earlier signature changed.
 *
 * Fields are planar f32 [nf][H][W][D] (dims = {H, W, D}, host), finite values.  For a field x and n = iterations in 1 .. 16:
 *   erode(x)(v)  = min of x over v and its 6 face neighbours inside the volume
 *   dilate(x)(v) = max of x over the 3x3x3 cube around v inside the volume
 *   E_0 = x, E_{j+1} = erode(E_j);  O_j = dilate(E_{j+1});  d_j = relu(E_j - O_j)                j = 0 .. n
 *   S_0 = d_0, S_j = S_{j-1} + relu(d_j - S_{j-1} d_j)                                           j = 1 .. n
 * every operation rounded on its own (no fused multiply-add), relu(x) = x > 0 ? x : +0: the bits of the clDice authors'
 * soft_skel.  mivp_cldice_skeleton writes skel = S_n in n + 1 launches whatever nf is.  keep != 0 stores what the backward
 * needs; workspace = mivp_cldice_skeleton_ws(nf, dims, iterations, keep) FLOATS (0 for arguments the call would refuse), with
 * F = nf H W D:  keep: E_1 .. E_{n+1} [n + 1][F] | O_0 .. O_n [n + 1][F] | two gradient fields [2][F];  else [2][F].
 * mivp_cldice_skeleton_grad: dx = d loss / d x from gskel = d loss / d S_n, on the keep workspace of the forward of the same
 * x.  Min and max hand the gradient of a pooled voxel to the k voxels of its window that hold the selected value, 1 / k each
 * (the result does not depend on memory order); relu'(0) = 0.  It overwrites the O fields: ONE backward per forward.
 * Gather form, no atomics, n + 3 launches.  Limits: nf <= 32767, H W D < 2^31, nf H W D (2 n + 8) <= 2^40.
 *
 * mivp_cldice_loss: logits f32 [B, vol, C] channels-last (2 <= C <= 8), target f32 [B, vol]; validity rule of mivp_seg_loss.
 * p = softmax_c(z) and t = one-hot(label), both taken as 0 at invalid voxels; classes c >= 1 always, K = C - 1; s = smooth > 0;
 * sums over the voxels of a sample (of the batch with batch != 0):
 *   SP_c = S_n(p_c), SL_c = S_n(t_c);  Tprec = (sum SP_c t_c + s) / (sum SP_c + s),  Tsens = (sum SL_c p_c + s) / (sum SL_c + s)
 *   cl_c = 1 - 2 Tprec Tsens / (Tprec + Tsens);  loss[0] = lambda_cldice weight[0] mean over (row, c >= 1) of cl_c
 * (weight: DEVICE pointer to one float, NULL = 1).  dlogits may be NULL: the value alone.  Otherwise d loss / d logits
 * (through SP, through Tsens' p, then the softmax; exactly 0 at an invalid voxel) is stored once per element, or with
 * accumulate != 0 added to what dlogits holds with one rounded add (the bits of dlogits + g).  mivp_cldice_loss_grad runs
 * the gradient on the SAME workspace with the SAME options, scaled by gscale[0] (device pointer, NULL = 1): once per value call.
 * workspace: mivp_cldice_ws(B, C, dims, iterations) floats; with F = B K vol, fields [B][K][vol]:
 *   [0, F)                       the planar p (p_c of class c = k + 1; 0 at invalid voxels)
 *   [F, (2 n + 5) F)             the keep workspace of the p side (above); its two gradient fields also serve the
 *                                erosions of the t side and end holding d loss / d p through SP
 *   [(2 n + 5) F, (2 n + 7) F)   SP, SL
 *   then partial rows [B K][bpb][4], sums [B K][4], gradient coefficients [B K][3]
 * 2 n + 7 fields in all.  No atomics, nothing read back, every launch unconditional: equal calls give equal bits. */
size_t mivp_cldice_skeleton_ws(int32_t nf, const int32_t* dims, int32_t iterations, int32_t keep);
int mivp_cldice_skeleton(const float* x, int32_t nf, const int32_t* dims, int32_t iterations, float* skel, float* workspace,
                         int32_t keep, mivp_stream_t stream);
int mivp_cldice_skeleton_grad(const float* x, const float* gskel, int32_t nf, const int32_t* dims, int32_t iterations,
                              float* workspace, float* dx, mivp_stream_t stream);
size_t mivp_cldice_ws(int32_t B, int32_t C, const int32_t* dims, int32_t iterations);
int mivp_cldice_loss(const float* logits, const float* target, int32_t B, int32_t C, const int32_t* dims, int32_t iterations,
                     float smooth, int32_t batch, int32_t ignore_index, int32_t has_ignore, float lambda_cldice,
                     const float* weight, float* workspace, float* loss, float* dlogits, int32_t accumulate,
                     mivp_stream_t stream);
int mivp_cldice_loss_grad(const float* logits, const float* target, int32_t B, int32_t C, const int32_t* dims,
                          int32_t iterations, float smooth, int32_t batch, int32_t ignore_index, int32_t has_ignore,
                          float lambda_cldice, const float* weight, float* workspace, const float* gscale, float* dlogits,
                          int32_t accumulate, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* downstream head on the LOW-resolution decoder output                      */
/* (swin_unetr.py:351-355 nn.Upsample x2 trilinear, then :229-237 BatchNorm3d */
/*  -> Conv3d 3^3): upsample, statistics, conv and the head's parameter       */
/*  gradients are all linear in x [B,h,w,d,C] bf16, so the C-channel          */
/*  full-resolution tensor is never formed.  C % 8 == 0, C < 64, Cout <= 4.   */
/* ------------------------------------------------------------------------ */
/* BatchNorm statistics of upsample(x): part [mivp_uphead_nblk(...)][2C] f32 partial (sum | sum of squares),   */
/* reduce with mivp_bn_finalize exactly like mivp_bn_stats' output (count = 8*B*h*w*d)                         */
int mivp_uphead_nblk(int32_t B, int32_t h, int32_t w, int32_t d, int32_t C);
/* gx (may be NULL): f32 [B*h*w*d][C] = U^T U x, the 27-point Gram stencil of the upsample applied to x -- the   */
/* per-cell term mivp_uphead_dx needs for the BatchNorm backward; keeping it saves that kernel a 27-point gather  */
int mivp_uphead_stats(const void* x, int32_t B, int32_t h, int32_t w, int32_t d, int32_t C, float* part, float* gx,
                      mivp_stream_t stream);
/* y [B,2h,2w,2d,Cout] f32 = bias + conv3x3x3(affine(upsample(x))).  wf: bf16 [16*ceil(27*Cout/16)][64], row
 * tap*Cout + co = (weight[co][:, tap] * scale | sum_c weight[co][c, tap] * shift[c] | 0...): the BatchNorm affine
 * folded into the weights, column C multiplying a constant-one channel.  workspace: mivp_uphead_fwd_ws bytes. */
size_t mivp_uphead_fwd_ws(int32_t B, int32_t h, int32_t w, int32_t d, int32_t Cout);
int mivp_uphead_fwd(const void* x, const void* wf, const float* bias, int32_t B, int32_t h, int32_t w, int32_t d,
                    int32_t C, int32_t Cout, void* workspace, float* y, mivp_stream_t stream);
/* D [B*h*w*d][ldD] bf16, column tap*Cout + co: the adjoint of the gather applied to dy [B,2h,2w,2d,dy_stride] f32.
 * mivp_gemm_tn(D, x) then gives G[tap*Cout + co][c] = sum_u dy[u - tap][co] * upsample(x)[u][c] and the column
 * sums of D give S = sum_{u in bounds} dy[u - tap][co]: the (G, S) of mivp_conv3d_wgrad_rows. */
int mivp_uphead_adjoint(const float* dy, int32_t dy_stride, int32_t B, int32_t h, int32_t w, int32_t d, int32_t Cout,
                        void* D, int32_t ldD, mivp_stream_t stream);
/* BatchNorm affine folded into the head conv (swin_unetr.py:229-237): wf bf16 [2][16*ceil(27*Cout/16)][64], row tap*Cout + co
 * = ( conv_w[co][c][tap] * scale[c]  for c < Cin | sum_c conv_w[co][c][tap] * shift[c] | 0 ... );  Cin < 64.  Plane 0 holds
 * the bf16 rounding of each value, plane 1 the bf16 rounding of the remainder (hi + lo pair, both fed to the MFMA). */
int mivp_uphead_fold(const float* conv_w, const float* scale, const float* shift, int32_t Cout, int32_t Cin, void* wf,
                     mivp_stream_t stream);

/* the four parameter gradients of the (BatchNorm -> conv 3^3) head from the (G, S) sums of mivp_uphead_adjoint +
 * mivp_gemm_tn (or mivp_conv3d_wgrad_rows): element (co, tap, ci) of G at G[co*gs_co + tap*gs_tap + ci], (co, tap) of S
 * at S[co*ss_co + tap*ss_tap];  dW [Cout][Cin][27], db [Cout], dgamma / dbeta [Cin] (autograd of swin_unetr.py:229-237) */
int mivp_head_grads(const float* G, int64_t gs_co, int64_t gs_tap, const float* S, int64_t ss_co, int64_t ss_tap,
                    const float* conv_w, const float* scale, const float* shift, const float* mean_rstd, int32_t Cout,
                    int32_t Cin, float* dW, float* db, float* dgamma, float* dbeta, mivp_stream_t stream);

/* the two small operands of mivp_uphead_dx from the head's parameters and batch statistics (layouts: see mivp_uphead_dx);
 * n_hr = number of high-resolution voxels 8*B*h*w*d; dgamma / dbeta may be NULL when training == 0 */
int mivp_uphead_dx_prep(const float* conv_w, const float* scale, const float* mean_rstd, const float* dgamma,
                        const float* dbeta, double n_hr, int32_t training, int32_t Cout, int32_t Cin, void* wc, float* coef,
                        mivp_stream_t stream);

/* gradient w.r.t. x [B,h,w,d,C] (bf16) through upsample -> BatchNorm -> conv, all at low resolution:
 *   D with ldD == 64; wc bf16 [16*ceil(C/16)][64] = conv weight as [c][tap*Cout + co] (zero padded);
 *   coef f32 [4][C] = (BN scale | sum(dz)/N | rstd*sum(dz*xhat)/N | batch mean), rows 1-2 zero for eval-mode BN;
 *   gx: mivp_uphead_stats' optional output for the same x, or NULL (the kernel then gathers the stencil itself) */
int mivp_uphead_dx(const void* D, const void* wc, const void* x, const float* coef, const float* gx, int32_t B, int32_t h,
                   int32_t w, int32_t d, int32_t C, void* dx, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* weight gradients: out[M][N] (+)= alpha * sum_t A[t][m] * B[t][n]          */
/* (the dW of every nn.Linear / nn.Conv3d on the path when autograd reaches */
/*  it: `loss.backward()` in segmentation.py:104, students_teacher.py:176)   */
/* ------------------------------------------------------------------------ */
typedef struct MivpOperandDesc {   /* where element (t, c) of a bf16 token-major operand lives */
    int32_t mode;       /* 0: t*ld + c                                                          */
                        /* 1: head-split [T/rows][C/hd][rows][hd] (attention q/k/v gradients)   */
                        /* 2: conv tap: column c = tap*cin + ci reads voxel t displaced by the  */
                        /*    tap (kh-1, kw-1, kd-1), zero outside the volume                   */
    int32_t ld;         /* mode 0/2: elements per row, multiple of 4                             */
    int32_t rows, hd;   /* mode 1 (hd multiple of 4)                                            */
    int32_t dims[3];    /* mode 2: H, W, D; t = ((b*H + h)*W + w)*D + d                          */
    int32_t cin;        /* mode 2: channels per tap, multiple of 4                               */
} MivpOperandDesc;

typedef struct MivpGemmTnDesc {
    int64_t T;          /* tokens / voxels summed over                                          */
    int32_t M, N;       /* out is fp32 [M][N] row-major                                          */
    MivpOperandDesc a;  /* supplies the M index (gradient w.r.t. the layer output)              */
    MivpOperandDesc b;  /* supplies the N index (the layer input)                               */
    float   alpha;
    int32_t accumulate; /* 1: out += result                                                      */
    int32_t perm_cin;   /* > 0 (== b.cin, mode 2): store column tap*cin + ci at ci*27 + tap,     */
                        /* i.e. out is nn.Conv3d.weight's [Cout][Cin][3][3][3]                   */
} MivpGemmTnDesc;

/* LayerNorm parameter gradients and the normalised rows the Linear weight gradients multiply with
 * (nn.LayerNorm of swin_block.py:117-118, down.py:16): rows x[t] are read directly (tok_src NULL) or
 * gathered through the block's tok_src table; dn = gradient w.r.t. the LayerNorm output.
 *   stats  [T][2] f32 scratch;  n_out [T][C] bf16 = LN(x) (zero rows on padding slots);
 *   part   [nblk][2C] f32: per-block (dbeta | dgamma) partials, reduce with mivp_reduce_rows;
 *   (nblk*256) % (C/8) == 0 */
int mivp_ln_wgrad(const void* x, const int32_t* tok_src, const void* dn, int64_t T, int32_t C, int32_t Nqp,
                  int32_t P, int64_t vol, float eps, const float* gamma, const float* beta, float* stats,
                  void* n_out, int32_t nblk, float* part, mivp_stream_t stream);

size_t mivp_gemm_tn_ws(const MivpGemmTnDesc* d);   /* fp32 split partials */
int mivp_gemm_tn(const MivpGemmTnDesc* d, const void* a, const void* b, void* workspace, size_t ws_bytes,
                 float* out, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* 1x1x1 convolution with <= 4 output channels (last layer of the            */
/* reconstruction head, swin_unetr.py:204-209)                               */
/* ------------------------------------------------------------------------ */
/* y [n_vox][Cout] f32 = bias + x [n_vox][C] bf16 . w [Cout][C] f32 */
int mivp_pointwise_fwd(const void* x, const float* w, const float* bias, int64_t n_vox, int32_t C, int32_t Cout,
                       float* y, mivp_stream_t stream);
/* dx [n_vox][C] bf16 = dy [n_vox][Cout] f32 . w;  dyb (optional) [n_vox][4] bf16 = dy zero-padded: the A operand of
 * mivp_gemm_tn for the weight gradient */
int mivp_pointwise_bwd(const float* dy, const float* w, int64_t n_vox, int32_t C, int32_t Cout, void* dx, void* dyb,
                       mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* small utilities                                                          */
/* ------------------------------------------------------------------------ */
/* fp32 -> bf16 cast of n elements (weight staging) */
int mivp_cast_f32_bf16(const float* in, int64_t n, void* out, mivp_stream_t stream);
/* y = a + b (bf16, n elements) : gradient accumulation at skip joins */
int mivp_add_bf16(const void* a, const void* b, int64_t n, void* y, mivp_stream_t stream);
/* MFMA lane-map self test: c[16][16] f32 = a[16][32] * b[16][32]^T via one 16x16x32 MFMA */
int mivp_selftest_mfma(const void* a, const void* b, float* c, mivp_stream_t stream);

/* ---- students/teacher objective and optimizer side ---------------------------------------------------
 * Point sampling of clustered_prototype_loss.py:162-204 (identity affine_grid + bilinear grid_sample, align_corners = False,
 * on an optional jitter crop): out f32 [B][o0*o1*o2][C] from vol [B][H][W][D][C] (channels_last) or [B][C][H][W][D], bf16 or
 * f32.  lo / hi / w: per axis, per output index: absolute voxel coordinates of the two taps and the weight of the upper one
 * (arrays of three device pointers).  The backward is a gather over voxels: per axis and voxel coordinate up to two
 * (output index, weight) pairs (index -1 = none); gvol bf16 [B][H][W][D][C], C % 8 == 0. */
int mivp_sample_points_fwd(const void* vol, int32_t is_bf16, int32_t channels_last, int32_t B, int32_t H, int32_t W, int32_t D,
                           int32_t C, const int32_t* out_dims, const int32_t* const* lo, const int32_t* const* hi,
                           const float* const* w, float* out, mivp_stream_t stream);
int mivp_sample_points_bwd(const float* gout, int32_t B, int32_t H, int32_t W, int32_t D, int32_t C, const int32_t* out_dims,
                           const int32_t* const* i1, const int32_t* const* i2, const float* const* w1, const float* const* w2,
                           void* gvol, mivp_stream_t stream);
/* torch.optim.AdamW over many tensors in one launch (students_teacher.py:27-68, segmentation.py:25-39).
 * tensors: device array of {float* p, float* exp_avg, float* exp_avg_sq, int64 n, int32 group, int32 pad} (40 bytes), static
 * across steps; grads: HOST array of n_tensors device pointers (they change every backward and travel as kernel arguments,
 * 384 per launch); chunk_begin: HOST int32 [n_tensors + 1], first chunk of each tensor; groups: HOST [n_groups][8] f32 =
 * {lr, beta1, beta2, eps, weight_decay, 1 - beta1^step, sqrt(1 - beta2^step), 0}; chunks: device int32 [.][2] = (tensor
 * index, 1024-element chunk), tensor-major. */
int mivp_adamw_multi(const void* tensors, const void* const* grads, int32_t n_tensors, const int32_t* chunk_begin,
                     const float* groups, int32_t n_groups, const void* chunks, mivp_stream_t stream);
/* The same step with the per-group hyper-parameters read from DEVICE memory (groups_dev: [8][8] f32, rows as above): the
 * form a HIP graph records, so that every replay uses the learning rate (WarmupCosineSchedule, modules/utils.py:67-89) and
 * bias corrections of its own step.  Bit-equal to mivp_adamw_multi for equal values. */
int mivp_adamw_multi_dev(const void* tensors, const void* const* grads, int32_t n_tensors, const int32_t* chunk_begin,
                         const float* groups_dev, int32_t n_groups, const void* chunks, mivp_stream_t stream);
/* Global gradient-norm clipping and non-finite step skipping for the AdamW step (mivp_amd/optim.py FusedAdamW(max_grad_norm,
 * skip_nonfinite)): three launches, nothing read back.  These entry points joined ABI 18 without a bump: they
 * are additive and no earlier signature changed.
 * 1. Sum of squares: tensors, grads, n_tensors, chunk_begin and chunks as for mivp_adamw_multi (only n of a tensor record is
 *    read); partials: device f32 [chunk_begin[n_tensors]], partials[c] = sum of g*g over chunk c in a fixed order (at most 12
 *    f32 additions on any path), every slot written once per call by a plain store; elements at or beyond n are not read. */
int mivp_grad_sumsq_multi(const void* tensors, const void* const* grads, int32_t n_tensors, const int32_t* chunk_begin,
                          const void* chunks, float* partials, mivp_stream_t stream);
/* 2. The plan, one workgroup: sumsq = the partials added in index order in f64, norm = sqrt(sumsq), coef = min(1, max_norm /
 *    (norm + 1e-6)) in f64 (torch.nn.utils.clip_grad_norm_; a NaN norm gives a NaN coef), exactly 1 for max_norm = +infinity
 *    (no clipping); max_norm > 0.  record: device, mivp_sizeof_opt(3) = 56 bytes, zeroed once by the caller:
 *    {f64 sumsq, f32 norm, f32 coef, u32 nonfinite = !isfinite(sumsq), u32 apply = !(skip_nonfinite && nonfinite),
 *     i64 steps, i64 clipped (apply && coef < 1), i64 skipped (!apply), f32 max_norm_seen (finite norms only), f32 pad};
 *    the last four run on from call to call.  One lane writes the record. */
int mivp_grad_clip_plan(const float* partials, int32_t n_partials, double max_norm, int32_t skip_nonfinite, void* record,
                        mivp_stream_t stream);
/* 3. mivp_adamw_multi / mivp_adamw_multi_dev under the record: nothing is touched when apply is 0; otherwise the gradient
 *    used is g * coef rounded to f32 once, so the step is bit-equal to the plain entry on gradients multiplied by coef
 *    beforehand (and to the plain entry itself for coef == 1). */
int mivp_adamw_multi_clip(const void* tensors, const void* const* grads, int32_t n_tensors, const int32_t* chunk_begin,
                          const float* groups, int32_t n_groups, const void* chunks, const void* record, mivp_stream_t stream);
int mivp_adamw_multi_clip_dev(const void* tensors, const void* const* grads, int32_t n_tensors, const int32_t* chunk_begin,
                              const float* groups_dev, int32_t n_groups, const void* chunks, const void* record,
                              mivp_stream_t stream);
/* n <= 64 floats from a HOST array into device memory as the arguments of a one-wave kernel (stream-ordered; refreshes the
 * scalars a recorded graph reads: the optimizer's groups_dev) */
int mivp_store_floats(float* dst, const float* host_values, int32_t n, mivp_stream_t stream);
/* EMA teacher update (momentum_model.py:27-36): tensors = device array of {float* teacher, const float* student, int64 n} */
int mivp_ema_multi(const void* tensors, const void* chunks, int32_t n_chunks, float tau, mivp_stream_t stream);
int mivp_sizeof_opt(int which);   /* 0: AdamW tensor record, 1: group record, 2: EMA record, 3: gradient-norm record */
/* sizeof of the descriptor structs as the LIBRARY was compiled (bindings compare them with their own layout):
 * 0 MivpSwinDesc, 1 MivpMergeDesc, 2 MivpConvDesc, 3 MivpEmbedDesc, 4 MivpUpcatDesc, 5 MivpOperandDesc, 6 MivpGemmTnDesc */
int mivp_sizeof_desc(int which);

/* Per-class counts of arg-max(logits) against a label volume (modules/utils.py:14-64 MeanIoU / DiceCoefficient without
 * host round trips): counts int64 [C][3] += (|pred = c and target = c|, |pred = c|, |target = c|); logits f32 [B][vol][C]
 * (channels_last) or [B][C][vol], target f32 [B][vol] class indices, nvox = B * vol, C <= 16. */
int mivp_seg_counts(const float* logits, const float* target, int64_t nvox, int32_t C, int32_t channels_last, int64_t vol,
                    void* counts, mivp_stream_t stream);

/* Transposed convolution with kernel == stride in {1, 2} per axis, no bias (the up-sampling step of MONAI's UnetrUpBlock,
 * swin_unetr.py:338-348,372-380): x bf16 [B][h][w][d][Cin] -> y bf16 [B][h*s0][w*s1][d*s2][Cout].
 * w1 bf16 [taps*Cout][Cin] (row (tap, co), tap = (a*s1 + b)*s2 + c of the nn.ConvTranspose3d weight [Cin][Cout][a][b][c]);
 * the data gradient takes w2 bf16 [Cin][taps*Cout].  Cin % 8 == 0, Cout % 8 == 0.  (Weight gradient: mivp_gemm_tn.) */
int mivp_convt_fwd(int32_t B, const int32_t* dims, const int32_t* stride, int32_t Cin, int32_t Cout, const void* x, const void* w1,
                   void* y, mivp_stream_t stream);
int mivp_convt_dgrad(int32_t B, const int32_t* dims, const int32_t* stride, int32_t Cin, int32_t Cout, const void* dy,
                     const void* w2, void* dx, mivp_stream_t stream);

/* Phase-1 multi-view self-supervised step (ABI 13; modules/multi_view.py:115-176, utils.py:267-350,
 * losses/contrastive_pair_loss.py).  Volumes are fp32 CHANNELS-FIRST [B][C][H][W][D] contiguous (out["reconstruction"] of
 * the model is channels-last storage: the same bytes at C = 1, a channels-first copy otherwise).  dims = {H, W, D},
 * mshape = masking patch {mh, mw, md} (host arrays); the patch grid is dims / mshape.
 *   codes int32 [2B]: rotation counts k_i[0..B) then k_j[0..B) (rot90 in the (H, W) plane, H == W)
 *   keep  uint32 [2][ceil(n_patches / 32)]: one bit per masking patch and view, patch (ph, pw, pd) -> bit
 *         (ph*gw + pw)*gd + pd; SET = visible (the reference's ``~mask``), shared by every sample and channel
 *   perm  int32 [1]: x_k = perm(x_i), 0 H<->W, 1 H<->D, 2 W<->D (cubes only)
 *   vec   float [5]: reconstruction, rotation, contrastive, mutual, weighted total
 * All of codes / keep / perm / gscale are DEVICE data: a recorded graph is refreshed by rewriting their content.
 *
 * mivp_mv_views: x_i / x_j = mask(rot90(x)), and x_k = perm(x_i) when xk != NULL (a second launch; 64 x 64 LDS tile
 *   transpose for the swaps that move D).
 * mivp_mv_rec_loss: value pass of rec = MSE over both views of (rec_v*k_v, x_v*k_v) / (1 - ratio) (when do_rec) and of
 *   mut = MSE(perm(rec_k)*k_i, rec_i*k_i) / (1 - ratio) (when rk != NULL) -> vec[0], vec[3];
 *   workspace: mivp_mv_rec_ws() floats.
 * mivp_mv_rec_grad: d rec_i, d rec_j, d rec_k of w_rec*rec + mut, times gscale[0] (device, NULL = 1).
 * mivp_mv_heads: one workgroup; rotation CE over cat(rot_i, rot_j) [2B][4] with targets codes, and NT-Xent
 *   (ContrastivePairLoss, temperature temp) of z_i, z_j [B][dim]; 2B <= 64, dim <= 1024; roti / zi may be NULL (term off).
 *   Value mode (dzi == droti == NULL): vec[1], vec[2] and vec[4] = w_rec*vec[0] + w_rot*vec[1] + w_con*vec[2] + vec[3]
 *   (vec[0] / vec[3] read when has_recmut, else written 0).  Gradient mode: dzi / dzj scaled by gscale[0]*w_con and
 *   droti / drotj by gscale[0]*w_rot; vec untouched.  workspace: mivp_mv_heads_ws(B, dim) floats.                       */
int mivp_mv_views(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* mshape, const int32_t* codes,
                  const void* keep, const int32_t* perm, float* xi, float* xj, float* xk, mivp_stream_t stream);
size_t mivp_mv_rec_ws(void);
int mivp_mv_rec_loss(const float* ri, const float* rj, const float* xi, const float* xj, const float* rk, int32_t B,
                     int32_t C, const int32_t* dims, const int32_t* mshape, const void* keep, const int32_t* perm,
                     int32_t do_rec, float ratio, float* workspace, float* vec, mivp_stream_t stream);
int mivp_mv_rec_grad(const float* ri, const float* rj, const float* xi, const float* xj, const float* rk, int32_t B,
                     int32_t C, const int32_t* dims, const int32_t* mshape, const void* keep, const int32_t* perm,
                     int32_t do_rec, float ratio, float w_rec, const float* gscale, float* dri, float* drj, float* drk,
                     mivp_stream_t stream);
size_t mivp_mv_heads_ws(int32_t B, int32_t dim);
int mivp_mv_heads(const float* zi, const float* zj, int32_t B, int32_t dim, float temp, const float* roti, const float* rotj,
                  const int32_t* codes, float w_rec, float w_rot, float w_con, int32_t has_recmut, float* workspace,
                  const float* gscale, float* dzi, float* dzj, float* droti, float* drotj, float* vec,
                  mivp_stream_t stream);

/* Whole-volume sliding-window prediction (ABI 14, csrc/stitch.hip; mivp_amd/inference.py SlidingWindowPredictor).
 * dims = image {H, W, D}, pad = zeros in front per axis, pdims = padded size max(dims, roi), roi = window size (host arrays).
 * table int32 [n_entries][4] = (o0, o1, o2, valid), origins in padded coordinates, n_entries a multiple of B; entry w is slot
 * w % B of sub-batch w / B.  sub_idx: DEVICE int32 [1], the current sub-batch, read by gather and blend and bumped by
 * mivp_window_advance (a recorded graph of gather -> model -> blend -> advance replays the next sub-batch each time).
 *   mivp_window_gather: vol f32 [1][Cin][H][W][D] (Cin <= 4) -> out f32 [B][Cin][roi] contiguous; zero outside the image and
 *     for invalid entries; 16-byte row accesses where aligned.
 *   mivp_window_blend: acc f32 [pdims][C] += w * logits, wsum f32 [pdims] += w, w(i, j, k) = max(w0[i] * w1[j] * w2[k],
 *     w_floor) (device tables), for every valid window of the sub-batch; logits f32 [B][roi][C] (channels_last) or [B][C][roi].
 *     No float atomics: each voxel adds its covering windows in increasing window index (bitwise independent of B).
 *     ubox = host {U0, U1, U2}: the largest union box of a sub-batch's windows (sizes the grid).  C <= 16.
 *   mivp_stitch_finalize: per image voxel acc / wsum -> labels uint8 [H][W][D] (first arg-max), logits f32 [C][H][W][D] when
 *     non-NULL, and when target f32 [H][W][D] is non-NULL counts int64 [C][3] += as mivp_seg_counts.
 *   mivp_window_advance: sub_idx[0] += 1 (one thread). */
int mivp_window_gather(const float* vol, int32_t Cin, const int32_t* dims, const int32_t* pad, const int32_t* pdims,
                       const int32_t* roi, const int32_t* table, int32_t n_entries, const int32_t* sub_idx, int32_t B,
                       float* out, mivp_stream_t stream);
int mivp_window_blend(const float* logits, int32_t channels_last, int32_t C, const int32_t* pdims, const int32_t* roi,
                      const int32_t* table, int32_t n_entries, const int32_t* sub_idx, int32_t B, const int32_t* ubox,
                      const float* w0, const float* w1, const float* w2, float w_floor, float* acc, float* wsum,
                      mivp_stream_t stream);
int mivp_stitch_finalize(const float* acc, const float* wsum, int32_t C, const int32_t* dims, const int32_t* pad,
                         const int32_t* pdims, uint8_t* labels, float* logits, const float* target, void* counts,
                         mivp_stream_t stream);
int mivp_window_advance(int32_t* sub_idx, mivp_stream_t stream);

/* Mirror test-time augmentation and probability maps (ABI 18, csrc/stitch.hip; SlidingWindowPredictor(mirror_axes=...)).
 * The _tta entries take the arguments of mivp_window_gather / mivp_window_blend; word 3 of a table entry is
 * valid | code << 1, bit a of the 3-bit code flipping roi axis a (0 = H, 1 = W, 2 = D).  The table lists every window under
 * every code, window-major (entry w * F + j = window w under the j-th code), and must be 16-byte aligned.  s_a(i) = r_a - 1 - i
 * where bit a is set, else i:
 *   mivp_window_gather_tta: out[b][c][i0][i1][i2] = padded volume[c][o + s(i)] (zero outside the image and for invalid
 *     entries); a D flip loads the mirrored 16-byte quad and reverses it in registers where rows are aligned.
 *   mivp_window_blend_tta: voxel o + p of the padded volume receives w(p) * logits[slot][c][s(p)] and w(p), w as in
 *     mivp_window_blend, indexed by the UNFLIPPED position p; contributions add in increasing entry index (bitwise
 *     independent of B).  comp: NULL, or f32 [pdims][C + 1] zeroed with acc / wsum: the sums are then compensated (Kahan),
 *     comp carrying each accumulator word's and the weight sum's running rounding error between launches, so F times as many
 *     contributions round like a few; acc / wsum remain the values to finalize.  With comp NULL and code 0 everywhere the
 *     result is bitwise that of mivp_window_blend.  The sub-batch's entries and union box are staged in LDS once per
 *     workgroup.  ubox: the largest union box over the sub-batches of THIS table.
 *   mivp_stitch_finalize_probs: mivp_stitch_finalize (the same labels, logits and counts, bit for bit) plus, each when
 *     non-NULL: probs f32 [C][H][W][D] = softmax over classes of acc / wsum (max-subtracted), confidence f32 [H][W][D] = the
 *     maximum probability, entropy f32 [H][W][D] = -sum p ln p / ln C in [0, 1] (0 when C == 1).  C <= 16. */
int mivp_window_gather_tta(const float* vol, int32_t Cin, const int32_t* dims, const int32_t* pad, const int32_t* pdims,
                           const int32_t* roi, const int32_t* table, int32_t n_entries, const int32_t* sub_idx, int32_t B,
                           float* out, mivp_stream_t stream);
int mivp_window_blend_tta(const float* logits, int32_t channels_last, int32_t C, const int32_t* pdims, const int32_t* roi,
                          const int32_t* table, int32_t n_entries, const int32_t* sub_idx, int32_t B, const int32_t* ubox,
                          const float* w0, const float* w1, const float* w2, float w_floor, float* acc, float* wsum,
                          float* comp, mivp_stream_t stream);
int mivp_stitch_finalize_probs(const float* acc, const float* wsum, int32_t C, const int32_t* dims, const int32_t* pad,
                               const int32_t* pdims, uint8_t* labels, float* logits, float* probs, float* confidence,
                               float* entropy, const float* target, void* counts, mivp_stream_t stream);

/* Surface-distance metrics (ABI 15, csrc/surface.hip; mivp_amd/surface.py).  dims = {H, W, D} (host), volumes
 * [H][W][D] row-major, fewer than 2^31 voxels.
 *   mivp_surface_map: pred / target class maps (dtype 0 uint8, 1 int32, 2 int64, 3 float32; values outside [0, C) and
 *     non-integer floats belong to no class) -> surf uint8 [H][W][D]: the class on surface voxels (in the class, with a
 *     6-neighbour outside it or outside the volume), 255 elsewhere.  target / surf_target may both be NULL.  counts int64
 *     [C][2] (pred, target) += surface voxels per class when non-NULL.  C <= 16.
 *   mivp_edt_sq: out f32 [H][W][D] = squared Euclidean distance (spacing: host f32 {s0, s1, s2} mm per voxel, > 0) to the
 *     nearest voxel with seeds == cls, +inf when there is none.  Exact integers when spacing == (1, 1, 1).  H, W <= 65535.
 *     workspace: mivp_edt_ws(dims) bytes, reused by every call in stream order.
 *   mivp_surface_stats: statistics of dist_sq sampled at {sampled == cls}, whose size *count (DEVICE int64) is:
 *     record int64 [8] = n, max key, #{sqrt(d2) <= tau}, bits of the float64 sum of sqrt(d2), key at rank lo, key at
 *     rank hi, lo, hi; keys are the bits of the float32 d2, lo / hi the ranks numpy.percentile(method="linear") reads
 *     for the quantile q in [0, 1] (virtual index (n - 1) q).  Fields 4-5 are untouched when n == 0.  No float atomics:
 *     bitwise reproducible.  workspace: mivp_surface_stats_ws(dims) bytes (zeroed by the call). */
int mivp_surface_map(const void* pred, const void* target, int32_t dtype, int32_t C, const int32_t* dims, uint8_t* surf_pred,
                     uint8_t* surf_target, void* counts, mivp_stream_t stream);
size_t mivp_edt_ws(const int32_t* dims);
int mivp_edt_sq(const uint8_t* seeds, int32_t cls, const int32_t* dims, const float* spacing, float* out, void* workspace,
                mivp_stream_t stream);
size_t mivp_surface_stats_ws(const int32_t* dims);
int mivp_surface_stats(const uint8_t* sampled, int32_t cls, const float* dist_sq, const int32_t* dims, const int64_t* count,
                       double q, double tau, void* workspace, int64_t* record, mivp_stream_t stream);

/* Connected components (ABI 16, csrc/components.hip; mivp_amd/components.py).  dims = {H, W, D} (host), volumes
 * [H][W][D] row-major, fewer than 2^31 voxels; x dtype as mivp_surface_map (0 uint8, 1 int32, 2 int64, 3 float32).
 * connectivity 6, 18 or 26: scipy.ndimage.generate_binary_structure(3, 1 / 2 / 3).  Adjacent voxels are joined when
 * both take part and hold the same value.  Exact integer arithmetic, bitwise reproducible, no host synchronisation.
 *   mivp_label_components: every nonzero voxel takes part.  labels int32 [H][W][D] = 0 on background, else 1 + the rank
 *     of the component's first voxel (raster order) among all components' first voxels (scipy.ndimage.label's
 *     numbering); *n_out (DEVICE int32) = the number of components.  workspace: mivp_label_ws(dims) bytes.
 *   mivp_postprocess_labels: the voxels whose class (value in [0, C), integer for floats) is a set bit of class_mask
 *     (bits 1..C-1 only, not empty) take part.  A component is kept iff its size >= min_size and, when largest, it is the
 *     largest of its class (ties: the one whose first voxel comes first in raster order); out (same dtype as x, may be x)
 *     = x with the voxels of removed components set to 0, every other voxel unchanged.  largest = 0 needs min_size > 0.
 *     When target f32 [H][W][D] is non-NULL, counts int64 [C][3] += (inter, pred, target) of out against it, as
 *     mivp_stitch_finalize.  C <= 16.  workspace: mivp_postprocess_ws(dims) bytes (8 per voxel + 256), reused by every
 *     call in stream order. */
size_t mivp_label_ws(const int32_t* dims);
int mivp_label_components(const void* x, int32_t dtype, const int32_t* dims, int32_t connectivity, int32_t* labels,
                          int32_t* n_out, void* workspace, mivp_stream_t stream);
size_t mivp_postprocess_ws(const int32_t* dims);
int mivp_postprocess_labels(const void* x, int32_t dtype, const int32_t* dims, int32_t C, uint32_t class_mask,
                            int64_t min_size, int32_t largest, int32_t connectivity, void* out, const float* target,
                            void* counts, void* workspace, mivp_stream_t stream);

/* Scan preparation and native-grid restore (ABI 17, csrc/scan.hip; mivp_amd/scan.py).  Every entry is one launch of a
 * resample-gather from a source grid src_dims = {m0, m1, m2} to an output grid out_dims = {k0, k1, k2} (host arrays, both
 * row-major, fewer than 2^31 voxels each): output axis a walks source axis axes[a] (host array, a permutation of 0..2).
 * tables: DEVICE int32 [3][K], K = k0 + k1 + k2, output axis a at offset k0 + .. + k(a-1) of each section; section 0 = the
 * lower source index per output index, section 1 = the upper one, section 2 = the bits of the fp32 weight of the upper one
 * (flips and the resize are folded into them; indices are clamped to the source axis).  A pure gather (interp = 0, and the
 * label entries always) reads section 0 only, and tables may then be int32 [K].  dtype: 0 uint8, 1 int32, 3 float32 (as
 * mivp_label_components), 4 int16.  When output axis 2 does not walk source axis 2, mivp_scan_prepare stages tiles through
 * LDS and the other three read directly (what measured faster); flags bit 0 forces direct reads, bit 1 staging (same bits
 * either way).  No workspace, no host synchronisation.
 *   mivp_scan_prepare: raw [C][m0][m1][m2] (C <= 4) -> out f32 [C][k0][k1][k2].  Per SOURCE voxel
 *     v = fma(x, map[0], map[1]), clamped to [map[2], map[3]] when clip (map: host f32 [4]); then with interp the blend
 *     fma(w, hi - lo, lo) along output axis 2, then 1, then 0 (torch trilinear, align_corners = False, when the tables say
 *     so); without interp out = v at the section-0 tap, exactly.
 *   mivp_scan_prepare_labels: seg [m0][m1][m2] -> out uint8 [k0][k1][k2], nearest.  A value outside 0..255 or a
 *     non-integer float writes 0 and sets bad[0] = 1 (DEVICE int32, zeroed by the caller).
 *   mivp_scan_restore_labels: the same gather for uint8 labels (no range to check).
 *   mivp_scan_restore_argmax: logits f32 [C][m0][m1][m2] (C <= 16) -> out uint8 [k0][k1][k2] = the first arg-max over the
 *     classes of the blended logits (as mivp_stitch_finalize breaks ties); the output-size logits are never stored. */
int mivp_scan_prepare(const void* raw, int32_t dtype, int32_t C, const int32_t* src_dims, const int32_t* out_dims,
                      const int32_t* axes, const int32_t* tables, int32_t interp, const float* map, int32_t clip,
                      int32_t flags, float* out, mivp_stream_t stream);
int mivp_scan_prepare_labels(const void* seg, int32_t dtype, const int32_t* src_dims, const int32_t* out_dims,
                             const int32_t* axes, const int32_t* tables, int32_t flags, uint8_t* out, int32_t* bad,
                             mivp_stream_t stream);
int mivp_scan_restore_labels(const uint8_t* labels, const int32_t* src_dims, const int32_t* out_dims, const int32_t* axes,
                             const int32_t* tables, int32_t flags, uint8_t* out, mivp_stream_t stream);
int mivp_scan_restore_argmax(const float* logits, int32_t C, const int32_t* src_dims, const int32_t* out_dims,
                             const int32_t* axes, const int32_t* tables, int32_t interp, int32_t flags, uint8_t* out,
                             mivp_stream_t stream);

/* Scan statistics and data-driven intensity windows (csrc/scanstats.hip, csrc/scan.hip; mivp_amd/scanstats.py, DESIGN
 * 4.23).  These entry points joined ABI 18 without a bump: they are additive and no earlier signature changed.
 *   mivp_scan_hist: raw [C][H][W][D] (C <= 4) of dtype 0 uint8 or 4 int16, dims = {H, W, D} (host), fewer than 2^31 voxels
 *     per channel.  hist: DEVICE int64 [C][65536], 8-byte aligned; the bin of value v is v + 32768 for both dtypes.  The
 *     launch ADDS to hist: zero it first, or pool scans in it.  A voxel counts when mask (DEVICE uint8 [H][W][D] shared by
 *     the channels, or NULL) is non-zero there and, with use_above, v > above.  base: the lowest value of the 16384
 *     consecutive values a workgroup counts in LDS; a value outside them adds to hist directly, so any base gives the same
 *     table and a base near the scan's minimum gives it fastest.  flags: bit 0 adds every value on its own, 0 (the
 *     default) merges the equal consecutive values of a lane's 16-byte load first (tools/bench_scanstats.py times both).
 *     Integer atomics only: exact, bitwise reproducible, independent of the launch shape.
 *   mivp_scan_window_plan: hist [C][65536] -> slot: DEVICE f32 [C][8], one workgroup per channel.  With N the count,
 *     a_lo / a_hi the k-th smallest counted values for k = max(1, ceil(q * (double)N)), q = q_lo / q_hi (0 <= q_lo <= q_hi
 *     <= 1; nearest rank, not an interpolating percentile), mean = S1 / N and std = sqrt(max(0, S2 / N - mean^2)) in
 *     float64 from the int64 sums S1 = sum v n_v, S2 = sum v^2 n_v (exact while S2 < 2^63: always for N < 2^33):
 *       slot[c] = {s, t, lo, hi, a_lo, a_hi, mean, std}, every word rounded from float64 to float32 once.
 *       mode 0 (percentile): s = (b_max - b_min) / (a_hi - a_lo), t = b_min - a_lo * s, lo = b_min, hi = b_max: the map of
 *         a_min = a_lo, a_max = a_hi, bit for bit; a_hi == a_lo (a constant scan, N == 0): s = 0, t = b_min.  clip unused.
 *       mode 1 (z-score): s = 1 / std, t = -mean / std (std == 0 or N == 0: s = 1, t = -mean; N == 0: mean = 0, a_lo =
 *         a_hi = 0); with clip lo = fmaf(a_lo, s, t), hi = fmaf(a_hi, s, t) in float32 from the rounded s and t, else
 *         -FLT_MAX and FLT_MAX.  b_min / b_max unused.
 *   mivp_scan_prepare_dev: mivp_scan_prepare with the map in DEVICE memory and per channel: channel c applies words 0..3
 *     of slot[c] (f32 [C][8], what mivp_scan_window_plan wrote).  The same kernels, staging choices and flag bits.
 * No workspace, no host synchronisation: histogram -> plan -> prepare record into a graph as a linear chain. */
int mivp_scan_hist(const void* raw, int32_t dtype, int32_t C, const int32_t* dims, const uint8_t* mask, int32_t use_above,
                   int32_t above, int32_t base, int32_t flags, int64_t* hist, mivp_stream_t stream);
int mivp_scan_window_plan(const int64_t* hist, int32_t C, int32_t mode, double q_lo, double q_hi, double b_min, double b_max,
                          int32_t clip, float* slot, mivp_stream_t stream);
int mivp_scan_prepare_dev(const void* raw, int32_t dtype, int32_t C, const int32_t* src_dims, const int32_t* out_dims,
                          const int32_t* axes, const int32_t* tables, int32_t interp, const float* slot, int32_t clip,
                          int32_t flags, float* out, mivp_stream_t stream);

/* Anti-aliased scan preparation (csrc/scan_aa.hip; mivp_amd/scan.py prepare_scan(antialias=True)).  These
 * entry points joined ABI 18 without a bump: they are additive and no earlier signature changed.  raw, dtype, C, src_dims,
 * out_dims, axes, map / slot, clip and out as mivp_scan_prepare / mivp_scan_prepare_dev.  Oriented axis a has n_in =
 * src_dims[axes[a]] inputs and n_out = out_dims[a] outputs and runs backwards through the source where flips[a] (host
 * int32 [3]) is set.  An axis with n_out < n_in is filtered with the normalised triangle filter of support n_in / n_out
 * (the separable filter of torch's bilinear antialias = True), an axis with n_out > n_in keeps the two-tap form
 * fma(w, hi - lo, lo), an axis with n_out == n_in is copied.  The map is applied per SOURCE voxel before any filtering.
 *   tables: DEVICE int32, the axes one after another in ORIENTED source coordinates (no flip folded in):
 *     n_out <  n_in: first[n_out], count[n_out], then the fp32 bits of w[n_out][tmax[a]], zero padded (tmax: host int32 [3],
 *                    1 <= tmax[a] <= 32, read for filtered axes only); out = sum_j w[k][j] * v[first[k] + j], j ascending,
 *                    one fmaf per tap
 *     n_out >  n_in: lo[n_out], hi[n_out], then the fp32 bits of the weight of hi
 *     n_out == n_in: nothing
 *   One launch per filtered axis, ordered by ascending n_out / n_in (compared as integers n_out[a] n_in[b] < n_out[b]
 *   n_in[a]; equal ratios: the higher axis first); the two-tap axes are folded into the last launch, blended along axis 2,
 *   then 1, then 0 inside every tap of its filter.  All launches but the last write fp32 intermediates [C][..] in oriented
 *   order into workspace (mivp_scan_prepare_aa_ws bytes, DEVICE, 256-byte aligned).  No atomics, every output written once:
 *   equal calls give equal bits.  No host synchronisation; the launches record into a graph as a linear chain.
 *   MIVP_EINVAL when no axis is filtered (mivp_scan_prepare serves that case) and for the refusals of mivp_scan_prepare;
 *   MIVP_EUNSUPPORTED, before any launch, when a filtered axis has tmax[a] > 32. */
size_t mivp_scan_prepare_aa_ws(int32_t C, const int32_t* src_dims, const int32_t* out_dims, const int32_t* axes);
int mivp_scan_prepare_aa(const void* raw, int32_t dtype, int32_t C, const int32_t* src_dims, const int32_t* out_dims,
                         const int32_t* axes, const int32_t* flips, const int32_t* tmax, const int32_t* tables,
                         const float* map, int32_t clip, float* out, void* workspace, mivp_stream_t stream);
int mivp_scan_prepare_aa_dev(const void* raw, int32_t dtype, int32_t C, const int32_t* src_dims, const int32_t* out_dims,
                             const int32_t* axes, const int32_t* flips, const int32_t* tmax, const int32_t* tables,
                             const float* slot, int32_t clip, float* out, void* workspace, mivp_stream_t stream);

/* Otsu foreground thresholds from the device histogram (csrc/scanstats.hip; mivp_amd/otsu.py otsu_slot / foreground_mask /
 * window_slot_above, mivp_amd/scanstats.py IntensityWindow(foreground="otsu")).  These entry points joined
 * ABI 18 without a bump: they are additive and no earlier signature changed.  No workspace, no host synchronisation.
 *   mivp_scan_otsu_plan: hist [C][65536] (what mivp_scan_hist wrote) -> otsu: DEVICE int64 [C][4], 8-byte aligned, one
 *     workgroup per channel.  With N = sum n_v and S = sum v n_v, a candidate t is a counted value that is not the largest
 *     counted value; n0 = sum_{v<=t} n_v, A = sum_{v<=t} v n_v, P = A N - S n0, q = n0 (N - n0).  The threshold is the
 *     candidate with the largest P^2 / q (Otsu's between-class variance is P^2 / (N^2 q)): two candidates compare by the
 *     integers P_a^2 q_b and P_b^2 q_a in 256 bits, equal values pick the lower t.  No floating-point arithmetic: bitwise
 *     reproducible.  otsu[c] = {t, n_le, n_gt, valid}: the counts at or below t and above it.  Fewer than two distinct
 *     counted values, N == 0 or N >= 2^33: valid = 0, t = the largest counted value (0 if none), n_le = N, n_gt = 0.
 *   mivp_scan_window_plan_above: mivp_scan_window_plan with the bins at or below otsu[c][0] read as zero (for N, S1, S2
 *     and both ranks) where otsu[c][3] is set: the plan of mivp_scan_hist with above = t added.  valid = 0: the
 *     unrestricted plan.  otsu must not be NULL.
 *   mivp_scan_threshold_mask: out uint8 [H][W][D] = (raw[channel] > otsu[channel][0]), all ones where otsu[channel][3] is
 *     0.  raw, dtype, C, dims as mivp_scan_hist; 0 <= channel < C; out needs no alignment.  One streaming launch. */
int mivp_scan_otsu_plan(const int64_t* hist, int32_t C, int64_t* otsu, mivp_stream_t stream);
int mivp_scan_window_plan_above(const int64_t* hist, int32_t C, int32_t mode, double q_lo, double q_hi, double b_min,
                                double b_max, int32_t clip, const int64_t* otsu, float* slot, mivp_stream_t stream);
int mivp_scan_threshold_mask(const void* raw, int32_t dtype, int32_t C, const int32_t* dims, int32_t channel,
                             const int64_t* otsu, uint8_t* out, mivp_stream_t stream);

/* Intensity transfer tables: equalisation, matching and Nyul-Udupa landmark standardisation (csrc/scan_transfer.hip;
 * mivp_amd/transfer.py).  These entry points joined ABI 18 without a bump: they are additive and no earlier
 * signature changed.  No workspace, no host synchronisation, no atomics: equal calls give equal bits, and the launches record
 * into a graph as a linear chain.  hist: DEVICE int64 [C][65536] as mivp_scan_hist wrote it, n_v the count of value v,
 * C(v) = sum_{w <= v} n_w, N = C(32767).  otsu: DEVICE int64 [C][4] of mivp_scan_otsu_plan or NULL; where otsu[c][3] is set
 * the bins at or below otsu[c][0] read as zero everywhere below, as in mivp_scan_window_plan_above.  table: DEVICE f32
 * [C][65536], table[c][v + 32768] the model-input intensity of raw value v, written for every v.  meta: DEVICE int32 [C][4] =
 * {lowest counted value, highest counted value, valid, 0}, both values 0 when nothing is counted.  One workgroup per
 * channel; every float64 operation below rounds on its own and the result rounds to float32 once.
 *   mivp_scan_transfer_equalize: v0 the lowest counted value, c0 = n_v0, d = N - c0; r = (double)max(C(v) - c0, 0) / (double)d
 *     (0 when d == 0); table = r * (b_max - b_min) + b_min, multiply then add.  b_min <= b_max, finite.  valid = N > 0.
 *   mivp_scan_transfer_match: u(v) = the smallest value u with C_ref(u) * N_src >= max(C_src(v), 1) * N_ref in 128-bit
 *     integers (ref_hist: the reference histogram, DEVICE int64 [C][65536]; otsu restricts hist, not ref_hist); N_src == 0
 *     or N_ref == 0: u(v) = v; a histogram with N >= 2^33: u(v) = v and valid = 0.  table = fmaf((float)u, s, t), clamped
 *     to [lo, hi] when clip, with {s, t, lo, hi} = words 0..3 of ref_slot[c] (DEVICE f32 [C][8], what mivp_scan_window_plan
 *     wrote for ref_hist): the map mivp_scan_prepare_dev applies, so matching a scan to its own histogram reproduces it.
 *   mivp_scan_landmarks: landmarks: DEVICE int64 [C][17] = {valid, m_0 .. m_{n-1}, 0 ..}, m_i the k-th smallest counted
 *     value for k = max(1, ceil(quantiles[i] * (double)N)) (nearest rank, as mivp_scan_window_plan; all 0 when N == 0);
 *     valid = N > 0 and m_{n-1} > m_0.  quantiles: HOST float64 [n] (void*: the header's pointer vocabulary has no
 *     pointer to double), 2 <= n <= 16, strictly increasing in [0, 1].
 *   mivp_scan_landmark_bank_add: bank: DEVICE float64 [C][17] (void*) = {count, sum_0 .. sum_{n-1}, 0 ..}, zeroed by the caller.  A
 *     valid record adds 1 to count and s_lo + (double)(m_i - m_0) / (double)(m_{n-1} - m_0) * (s_hi - s_lo) to sum_i (divide,
 *     multiply, add s_lo); an invalid one adds nothing.  s_lo <= s_hi, finite.  One tiny launch.
 *   mivp_scan_transfer_landmarks: S_i = sum_i / count; the knots M_j are the distinct m_i in increasing order and T_j the
 *     mean of the S_i that share M_j (summed in index order, divided by their number), j < K.  Segment j serves
 *     M_j <= v < M_{j+1}, segment 0 every v below M_0, segment K - 2 every v from M_{K-1} on:
 *     table = T_j + (double)(v - M_j) / (double)(M_{j+1} - M_j) * (T_{j+1} - T_j) (divide, multiply, add), with clip clamped
 *     to [T_0, T_{K-1}].  K < 2: T_0 everywhere, 0 when N == 0.  count == 0: 0 everywhere.  valid = count > 0, N > 0 and
 *     K >= 2.  hist (and otsu) are those the record was taken from: they give N and the two values of meta.
 *   mivp_scan_transfer_apply: out f32 [C][H][W][D] = table[c][raw[c] + 32768] on the native grid, one streaming launch.
 *     raw, dtype, C, dims as mivp_scan_hist; out needs 4-byte alignment only (16-byte stores are used where out is aligned
 *     like raw).  By default a workgroup first copies the table entries of the values meta[c][0] .. meta[c][1], 16384 at
 *     most (all 256 for uint8), into LDS and gathers from there, a value outside them from the table itself; flags bit 0
 *     gathers every value from the table in global memory.  The same bits either way (tools/bench_transfer.py times both).
 * MIVP_EINVAL before any launch for a NULL (other than otsu) or misaligned pointer, C outside 1..4, n outside 2..16,
 * quantiles not strictly increasing in [0, 1], and an unknown dtype or flag bit. */
int mivp_scan_transfer_equalize(const int64_t* hist, int32_t C, double b_min, double b_max, const int64_t* otsu,
                                float* table, int32_t* meta, mivp_stream_t stream);
int mivp_scan_transfer_match(const int64_t* hist, const int64_t* ref_hist, const float* ref_slot, int32_t C, int32_t clip,
                             const int64_t* otsu, float* table, int32_t* meta, mivp_stream_t stream);
int mivp_scan_landmarks(const int64_t* hist, int32_t C, const void* quantiles, int32_t n, const int64_t* otsu,
                        int64_t* landmarks, mivp_stream_t stream);
int mivp_scan_landmark_bank_add(const int64_t* landmarks, int32_t C, int32_t n, double s_lo, double s_hi, void* bank,
                                mivp_stream_t stream);
int mivp_scan_transfer_landmarks(const int64_t* hist, const int64_t* landmarks, const void* bank, int32_t C, int32_t n,
                                 int32_t clip, const int64_t* otsu, float* table, int32_t* meta, mivp_stream_t stream);
int mivp_scan_transfer_apply(const void* raw, int32_t dtype, int32_t C, const int32_t* dims, const float* table,
                             const int32_t* meta, int32_t flags, float* out, mivp_stream_t stream);

/* Per-lesion region statistics and lesion-wise detection metrics (csrc/regions.hip; mivp_amd/regions.py).
 * These entry points joined ABI 18 without a bump: they are additive and no earlier signature changed.  dims = {H, W, D}
 * (host), volumes [H][W][D] row-major, fewer than 2^31 voxels; connectivity as mivp_label_components.  No host
 * synchronisation: every count stays on the device.  Integer results are exact and bitwise reproducible.
 *   MivpRegionTable: DEVICE arrays of `capacity` entries, entry r describes the component labelled r + 1.  n[0] = the number
 *     of components (it may exceed capacity; entries at and above min(n, capacity) are zero), overflow[0] = (n > capacity).
 *     cls = the class, size = voxels, first = linear index of the first voxel in raster order, bbox [6] = minimum h, w, d
 *     and maximum h, w, d (inclusive), coord_sum [3] = sums of h, w, d.  image_dtype: -1 no image (vmin, vmax, vsum, vsqsum
 *     may be NULL), else the dtype of mivp_scan_prepare (0 uint8, 1 int32, 3 float32, 4 int16): vmin / vmax are int32
 *     (float32 for a float image), vsum / vsqsum int64 and exact while they fit (int64 arithmetic wraps modulo 2^64, which
 *     only the sum of squares of an int32 image with values beyond about 2^31 / sqrt(voxels) can reach) (float64 for a float image: added with hardware float64
 *     atomics, so these two alone depend on the order of arrival in their last bits).
 *   mivp_region_stats: x (dtype 0 uint8, 1 int32, 2 int64, 3 float32) is a class map; the voxels whose class (value in
 *     [0, C), integer for floats) is a set bit of class_mask (bits 1..C-1 only, not empty) are labelled as
 *     mivp_label_components labels them: labels int32 [H][W][D], 16-byte aligned, numbered 1..n in the raster order of first
 *     voxels.  One pass over labels (and image, of table->image_dtype, same shape) fills the table: runs along D per lane,
 *     one LDS table per workgroup, one set of global atomics per (workgroup, region).  C <= 16.  workspace:
 *     mivp_region_stats_ws(dims) bytes.
 *   mivp_region_overlap: the sparse table of n_pt = |p and t| over the pairs (p of labels_pred, t of labels_target) of one
 *     class with p <= pred->capacity and t <= target->capacity: an open-addressing hash table in `pairs`
 *     (mivp_region_overlap_ws(max_pairs) bytes, 8-byte aligned) of int64 words: [0] the number of distinct pairs, [1] the
 *     overflow flag (more than max_pairs distinct pairs; the table is then incomplete), then keys [S] = (p << 32) | t,
 *     0 = empty, then counts [S], S = the smallest power of two >= max(64, 2 * max_pairs).  Probing is bounded: a full table
 *     sets the flag and the launch ends.
 *   mivp_lesion_match: components smaller than min_size are ignored on both sides.  Per reference lesion t (arrays of
 *     target->capacity entries): overlap = sum_p n_pt, touching = sum of |p| over the p with n_pt > 0, best_pred = the p
 *     with the largest n_pt (ties: the smaller label; 0 when none), best_overlap = its n_pt, detected = 1 iff some pair
 *     (p, t) matches: IoU = (double)n_pt / (double)(|p| + |t| - n_pt) > 0 when iou_threshold == 0, else >= iou_threshold.
 *     matched [pred->capacity] = 1 iff p has a match.  counts int64 [C][4] = (reference lesions, predicted lesions,
 *     detected reference lesions, matched predictions) per class. */
typedef struct {
    int32_t capacity;
    int32_t image_dtype;
    int32_t* n;
    int32_t* overflow;
    int32_t* cls;
    int64_t* size;
    int64_t* first;
    int32_t* bbox;
    int64_t* coord_sum;
    void* vmin;
    void* vmax;
    void* vsum;
    void* vsqsum;
} MivpRegionTable;
size_t mivp_region_stats_ws(const int32_t* dims);
int mivp_region_stats(const void* x, int32_t dtype, const int32_t* dims, int32_t C, uint32_t class_mask,
                      int32_t connectivity, const void* image, int32_t* labels, const MivpRegionTable* table,
                      void* workspace, mivp_stream_t stream);
size_t mivp_region_overlap_ws(int64_t max_pairs);
int mivp_region_overlap(const int32_t* labels_pred, const int32_t* labels_target, const int32_t* dims,
                        const MivpRegionTable* pred, const MivpRegionTable* target, int64_t max_pairs, void* pairs,
                        mivp_stream_t stream);
int mivp_lesion_match(const MivpRegionTable* pred, const MivpRegionTable* target, const void* pairs, int64_t max_pairs,
                      int32_t C, int64_t min_size, double iou_threshold, int64_t* counts, int64_t* overlap,
                      int64_t* touching, int64_t* best_overlap, int32_t* best_pred, int32_t* detected, int32_t* matched,
                      mivp_stream_t stream);
/* Lesion scores for FROC (additive, ABI 18).  pred must carry a float32 image (image_dtype 3).  One pass over
 * the pair table with the pair rules of mivp_lesion_match (one device function serves both): best_score [target->capacity]
 * = the largest pred->vmax over the predictions that match the reference lesion, -inf where none does; score
 * [pred->capacity] = a copy of pred->vmax.  vmax is exact, so both are bitwise reproducible. */
int mivp_lesion_best_score(const MivpRegionTable* pred, const MivpRegionTable* target, const void* pairs,
                           int64_t max_pairs, int64_t min_size, double iou_threshold, float* best_score, float* score,
                           mivp_stream_t stream);
/* Per-lesion shape descriptors (csrc/region_shape.hip; mivp_amd/regions.py region_shape).  These entry points
 * joined ABI 18 without a bump: they are additive and no earlier signature changed.  Two launches after mivp_region_stats,
 * nothing read back; every output is a DEVICE array of `capacity` entries, entry r describes the component labelled r + 1,
 * every entry is written by every call and an absent region's entry is zero.
 *   mivp_region_shape: one pass over labels, the dense int32 [H][W][D] map that mivp_region_stats wrote (values 0..n; labels
 *     above capacity are skipped).  dims = {H, W, D} (host), fewer than 2^31 voxels and NO DIMENSION ABOVE 65535: a
 *     coordinate product is then below 2^32 and, with fewer than 2^31 voxels, no sum can reach 2^63.  The outputs are zeroed
 *     inside the call, on the stream.  Integer atomics only: exact and bitwise reproducible.
 *       moment2 int64 [capacity][6]: the sums over the region's voxels of h*h, w*w, d*d, h*w, h*d, w*d on voxel indices.
 *       faces   int64 [capacity][3]: the exposed voxel faces normal to h, w and d.  A face of a voxel of region r is exposed
 *               when the voxel across it does not carry label r or lies outside the volume; both sides of the region
 *               count, so an isolated voxel gives (2, 2, 2).
 *       cells   int64 [capacity][2]: the distinct vertices and the distinct edges of the region's closed cubical complex
 *               (the union of its closed unit cubes).  A vertex is shared by up to 8 voxels and an edge by up to 4; the first
 *               incident voxel of the region in raster order counts it.  The distinct faces follow from
 *               F = (6 * size + faces[0] + faces[1] + faces[2]) / 2, and the Euler number is V - E + F - size.
 *   mivp_region_axes: one thread per region, float64.  size, coord_sum: the arrays of the MivpRegionTable; moment2 as above;
 *     sh, sw, sd: the voxel spacing in mm (> 0).  covariance, eigenvalues and axes are float64 arrays, 8-byte aligned.
 *       covariance  [capacity][3][3]: (n * M_ab - S_a * S_b), formed exactly in 128-bit integers, converted to float64 once
 *                   (correctly rounded), divided by (double)n * (double)n (exact below 2^26 voxels) and multiplied by
 *                   spacing_a * spacing_b: the covariance of the voxel centres in mm^2, without a 1/12 voxel-extent term.
 *                   A one-voxel region and a region flat along an axis have exact zeros in that row and column.
 *       eigenvalues [capacity][3]: of that matrix, descending, by a cyclic Jacobi iteration with the fixed sweep order
 *                   (h,w), (h,d), (w,d) and at most 16 sweeps (it ends early only when all off-diagonals are exactly 0);
 *                   values that round below zero are clamped to 0.
 *       axes        [capacity][3][3]: row i is the unit eigenvector of eigenvalue i in (h, w, d) order, its sign chosen so
 *                   that its largest-magnitude component is positive (ties: the first such component).
 *     Entries with size == 0 are all zero. */
int mivp_region_shape(const int32_t* labels, const int32_t* dims, int32_t capacity, int64_t* moment2, int64_t* faces,
                      int64_t* cells, mivp_stream_t stream);
int mivp_region_axes(const int64_t* size, const int64_t* coord_sum, const int64_t* moment2, int32_t capacity, double sh,
                     double sw, double sd, void* covariance, void* eigenvalues, void* axes, mivp_stream_t stream);

/* Centreline extraction by 3-D thinning and the centreline counts (csrc/skeleton.hip; mivp_amd/skeleton.py).
 * These entry points joined ABI 18 without a bump: they are additive and no earlier signature changed.  dims = {H, W, D}
 * (host), volumes [H][W][D] row-major, fewer than 2^31 voxels; label dtypes as mivp_label_components (0 uint8, 1 int32,
 * 2 int64, 3 float32); class_mask: bits 1..C-1 only, not empty; C <= 16.  No host synchronisation, integer arithmetic and
 * integer atomics only: every result is exact and bitwise reproducible.
 *   The object of a voxel is the set of voxels that hold its (selected) class; everything else, the outside of the volume
 *   included, is background.  With obj the object voxels among the 26 neighbours, a voxel is SIMPLE iff obj is not empty and
 *   is one component under 26-adjacency within the neighbourhood, and the background voxels among the 18-neighbours contain a
 *   6-neighbour and all background 6-neighbours lie in one component of them under 6-adjacency; an END POINT has at most one
 *   object neighbour.  One iteration marks the object voxels with a face neighbour outside their object, on the state it
 *   starts from, then runs eight sub-passes, subfield s = (h&1)<<2 | (w&1)<<1 | (d&1) for s = 0..7: a sub-pass deletes every
 *   marked voxel of its subfield that is simple on the current state and, with keep_endpoints, is no end point on it.
 *   mivp_skeleton_begin: skeleton (uint8 [H][W][D]) = the class of labels where it is a set bit of class_mask, else 0.  With
 *     workspace (mivp_skeleton_ws(dims) bytes, 4-byte aligned; may be NULL when only the selection is wanted) it also resets
 *     the iteration state kept there.
 *   mivp_skeleton_iter: iteration number `iteration` (1, 2, 3, .. in this order after mivp_skeleton_begin) on skeleton, in
 *     place: one mark launch and up to eight sub-pass launches (a subfield without voxels has none).  The deletions of an
 *     iteration are counted in the int32 word iteration & 1 at the start of the workspace (the mark launch zeroes it); every
 *     launch of an iteration > 1 returns at once when the word of the iteration before is zero, so any number of iterations
 *     may be issued without reading anything back.
 *   mivp_skeleton_end: after `iteration` iterations were issued, iterations[0] (DEVICE int32) = the number that ran, the one
 *     that deleted nothing included, and converged[0] = 1 when the last one issued deleted nothing (or did not run).
 *   mivp_centerline_counts: one pass over the two label maps and their two skeletons.  counts: DEVICE int64 [C][4], per class
 *     c: the voxels with skeleton_pred == c, those of them where target is c, the voxels with skeleton_target == c, those of
 *     them where pred is c.  The launch ADDS to counts: zero it first, or pool scans in it.
 *   mivp_skeleton_stats: one pass over one skeleton.  counts: DEVICE int64 [C][18], per class c of class_mask: the voxels that
 *     hold c; those with 0, 1, 2 and >= 3 26-neighbours that hold c; then, for the 13 offsets (dh, dw, dd) whose first
 *     non-zero component is positive, in lexicographic order, the voxel pairs that far apart that both hold c.  ADDS. */
size_t mivp_skeleton_ws(const int32_t* dims);
int mivp_skeleton_begin(const void* labels, int32_t dtype, const int32_t* dims, int32_t C, uint32_t class_mask,
                        uint8_t* skeleton, void* workspace, mivp_stream_t stream);
int mivp_skeleton_iter(uint8_t* skeleton, const int32_t* dims, int32_t keep_endpoints, int32_t iteration, void* workspace,
                       mivp_stream_t stream);
int mivp_skeleton_end(const void* workspace, int32_t iteration, int32_t* iterations, int32_t* converged,
                      mivp_stream_t stream);
int mivp_centerline_counts(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype,
                           const uint8_t* skeleton_pred, const uint8_t* skeleton_target, const int32_t* dims, int32_t C,
                           int64_t* counts, mivp_stream_t stream);
int mivp_skeleton_stats(const uint8_t* skeleton, const int32_t* dims, int32_t C, uint32_t class_mask, int64_t* counts,
                        mivp_stream_t stream);

/* Calibration and threshold-sweep tables (csrc/calibration.hip; mivp_amd/calibration.py).  These entry points
 * joined ABI 18 without a bump: they are additive and no earlier signature changed.  probs: contiguous fp32 [C][H][W][D],
 * target: a class map [H][W][D] of target_dtype (0 uint8, 1 int32, 2 int64, 3 float32), dims = {H, W, D} (host), fewer
 * than 2^31 voxels, 1 <= C <= 16, 1 <= n_bins <= 1024.  With Q = 2^20, q = rint(p * Q) and bin = min(n_bins - 1,
 * q * n_bins >> 20), a voxel whose C probabilities are all in [0, 1] and whose reference value is a class adds to C + 1
 * rows: rows 0..C-1 one-vs-rest (p = p_c, y = [target == c]), row C top-label (p = max p_c, y = [argmax == target], the
 * lowest index among equals).  A voxel with a probability outside [0, 1] (or NaN) only adds 1 to n_invalid; otherwise one
 * whose reference value is no class only adds 1 to n_ignored.
 *   tables: DEVICE int64 block of mivp_calibration_ws(C, n_bins) bytes, with R = C + 1: count [R][n_bins], pos [R][n_bins]
 *     (sum of y), qsum [R][n_bins] (sum of q), n [R], n_pos [R], sq_hi [R], sq_lo [R] (sums of e^2 >> 20 and e^2 & (Q - 1)
 *     for e = |q - y Q|), n_ignored, n_invalid.  The launch ADDS to the block: zero it first, or pool volumes in it.
 *   flags: bit 0 sums the lanes of a wave that hit the same cell before the atomic (measured slower than plain adds,
 *     DESIGN 4.22; tools/bench_calibration.py times both).  0 is the default path.
 * One launch, no host synchronisation, integer atomics only: the result is exact and bitwise reproducible. */
size_t mivp_calibration_ws(int32_t C, int32_t n_bins);
int mivp_calibration_hist(const float* probs, const void* target, int32_t target_dtype, const int32_t* dims, int32_t C,
                          int32_t n_bins, int32_t flags, int64_t* tables, mivp_stream_t stream);

/* Random intensity augmentation of a resident batch (csrc/intensity.hip; mivp_amd/augment.py).  These entry
 * points joined ABI 18 without a bump: they are additive and no earlier signature changed.  x: contiguous fp32
 * [B][C][H][W][D], dims = {H, W, D} (host), fewer than 2^31 voxels per sample, B <= 65535.  slot: DEVICE int32 [B][40], one
 * record per sample (fp32 values as their bits): [0] flags (bit 0 bias field, 1 std shift, 2 gamma contrast, 3 scale,
 * 4 histogram shift), [1] n control points (2..12), [2] shift factor, [3] gamma, [4] scale factor, [5..24] the bias
 * coefficients c[i][j][k] of the Legendre degree-3 field (i + j + k <= 3; i outer, k inner), [25..36] the floating control
 * points, [37..39] unused.  The steps run in bit order; a sample's statistics run over all of its channels.
 *   mivp_intensity_ws(B, voxels_per_sample): bytes of the partials workspace (never more than B * 256 * 32).
 *   mivp_intensity_stats: per-workgroup (min, max, count, mean, M2) partials of v = x * exp(field) (v = x without the bias
 *     flag) of every sample whose flags need statistics (shift, contrast, histogram); the others are not read.
 *   mivp_intensity_apply: merges a sample's partials in a fixed order, derives the scalar plan (std, contrast min / range,
 *     the histogram knots on the tracked extremes) and streams x to out.  out may be x.  A sample without flags is copied
 *     bit for bit.  Results are bitwise reproducible.
 * No host synchronisation and no host-side parameter other than the shape: both launches record into a graph and a replay
 * uses whatever the slot holds then. */
size_t mivp_intensity_ws(int32_t B, int64_t voxels_per_sample);
int mivp_intensity_stats(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* slot, void* workspace,
                         size_t workspace_bytes, mivp_stream_t stream);
int mivp_intensity_apply(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* slot,
                         const void* workspace, size_t workspace_bytes, float* out, mivp_stream_t stream);

/* Neighbourhood augmentation of a resident batch: Gaussian noise, Gaussian blur, low-resolution simulation
 * (csrc/filters.hip; mivp_amd/augment.py).  These entry points joined ABI 18 without a bump: they are additive
 * and no earlier signature changed.  x, dims, B as for mivp_intensity_apply.  slot: DEVICE int32
 * [B][MIVP_FILTER_RECORD_WORDS], one record per sample (fp32 values as their bits): [0] flags (bit 0 noise, 1 smooth,
 * 2 low-res), [1] noise key, [2] noise mean, [3] noise std, [4..6] radius of axis H, W, D (0..8; 0: the axis is not
 * filtered), [7..9] the low-resolution grid (1..dims per axis), [10..60] taps [3][17], tap k = -r..r of axis a at
 * 10 + 17 a + 8 + k (non-negative), [61..63] unused.  Per sample, in this order:
 *   noise:   v = x + (mean + std * g), g = sqrt(-2 ln u1) cos(2 pi u2), u1 = ((h1 >> 8) + 1) 2^-24, u2 = (h2 >> 8) 2^-24,
 *            h1 / h2 the counter hashes of 2 idx / 2 idx + 1 under the key, idx the element's index inside the sample.
 *   smooth:  separable, D then W then H, out[i] = sum_k tap[k] in[i + k] with zeros outside the volume, summed from -r
 *            upwards, every product and sum rounded to fp32 on its own.
 *   low-res: torch's nearest down-sampling to the low grid and trilinear (align_corners = False) up-sampling back, per
 *            output voxel from the eight corners; the low-resolution volume is never stored.
 *   mivp_filter_ws(B, C, dims): bytes of the workspace (two batch-sized temporaries); 0 for a shape outside the contract.
 *   mivp_filter_apply: three launches (D and W pass with the noise, H pass, low-res), always, whatever the records hold.  out
 *     may be x.  A sample without flags -- or with a flag word, radius or low grid outside the ranges above -- is copied bit
 *     for bit (in place: not written).  Results are bitwise reproducible.
 * No host synchronisation and no host-side parameter other than the shape: the launches record into a graph and a replay
 * uses whatever the slot holds then. */
#define MIVP_FILTER_RECORD_WORDS 64
size_t mivp_filter_ws(int32_t B, int32_t C, const int32_t* dims);
int mivp_filter_apply(const float* x, int32_t B, int32_t C, const int32_t* dims, const int32_t* slot, void* workspace,
                      size_t workspace_bytes, float* out, mivp_stream_t stream);

/* Skipping all-background windows in whole-volume prediction (csrc/window_skip.hip; SlidingWindowPredictor(skip=...),
 * DESIGN 4.24).  These entry points joined the current ABI without a bump: they are additive and no earlier signature
 * changed.  dims / pad / pdims / roi as for mivp_window_gather (host int32 [3]).
 *   mivp_window_occupancy: counts int32 [n_windows] = foreground voxels of each window; the call zeroes counts itself.
 *     Exactly one source: vol f32 [Cin][H][W][D] with channel and threshold (foreground: vol[channel] > threshold, strict
 *     fp32, so NaN is not foreground), or mask uint8 [H][W][D] (foreground: mask != 0; vol NULL, Cin / channel / threshold
 *     ignored).  Voxels of the zero padding are never foreground.  origins: DEVICE int32 [n_windows][origin_stride],
 *     origin_stride 3 or 4, padded-volume coordinates; a window that does not lie in the padded volume counts 0.  The grid
 *     is (window, slab of rows), four D voxels per load where D % 4 == 0 and the base is aligned, one integer atomic per
 *     workgroup: exact and bitwise reproducible.
 *   mivp_window_compact: full_table int32 [n_entries][4] (the immutable work list, entry e = window e / n_flips, never
 *     written) -> table int32 [n_entries][4]: the valid entries of the windows with counts[w] >= min_voxels first, in their
 *     original order and with word 3 unchanged, every later row zero (invalid); meta int32 [2] = (kept windows, kept
 *     entries).  One workgroup, an ordered block prefix scan: deterministic.  table != full_table, both 16-byte aligned.
 *   mivp_window_blend_any: the arguments and the per-voxel arithmetic of mivp_window_blend_tta (comp NULL: that of
 *     mivp_window_blend; bitwise the same sums for the same entries), for a table whose sub-batches can have ANY union box
 *     inside the padded volume: ubox only sizes the launch grid (the recorded graph's is fixed), a larger box is walked
 *     with a grid stride and never dropped.
 *   mivp_stitch_fill: every voxel of the padded volume with wsum == 0 gets acc[v][c] = +fill_logit at fill_class and
 *     -fill_logit elsewhere and wsum = 1, so that mivp_stitch_finalize(_probs) returns exactly those logits there. */
int mivp_window_occupancy(const float* vol, int32_t Cin, int32_t channel, float threshold, const uint8_t* mask,
                          const int32_t* dims, const int32_t* pad, const int32_t* pdims, const int32_t* roi,
                          const int32_t* origins, int32_t origin_stride, int32_t n_windows, int32_t* counts,
                          mivp_stream_t stream);
int mivp_window_compact(const int32_t* full_table, int32_t n_entries, int32_t n_windows, int32_t n_flips,
                        const int32_t* counts, int32_t min_voxels, int32_t* table, int32_t* meta, mivp_stream_t stream);
int mivp_window_blend_any(const float* logits, int32_t channels_last, int32_t C, const int32_t* pdims, const int32_t* roi,
                          const int32_t* table, int32_t n_entries, const int32_t* sub_idx, int32_t B, const int32_t* ubox,
                          const float* w0, const float* w1, const float* w2, float w_floor, float* acc, float* wsum,
                          float* comp, mivp_stream_t stream);
int mivp_stitch_fill(float* acc, float* wsum, int32_t C, const int32_t* pdims, int32_t fill_class, float fill_logit,
                     mivp_stream_t stream);

/* Fitting the prediction windows to the foreground bounding box (csrc/window_fit.hip; SlidingWindowPredictor(fit=...),
 * DESIGN 4.25).  These entry points joined the current ABI without a bump: they are additive and no earlier signature
 * changed.
 *   mivp_foreground_box: box DEVICE int32 [6] = (lo0, lo1, lo2, hi0, hi1, hi2), the inclusive bounding box of the
 *     foreground in image coordinates; no foreground gives lo = dims and hi = -1.  Exactly one source, as for
 *     mivp_window_occupancy: vol f32 [Cin][H][W][D] with channel and threshold (vol[channel] > threshold, strict fp32, so
 *     NaN is not foreground), or mask uint8 [H][W][D] (mask != 0; vol NULL, Cin / channel / threshold ignored).  dims =
 *     {H, W, D} (host), fewer than 2^31 voxels.  Two launches on the stream: one initialises the six words, one reads the
 *     channel (or the mask) once, four D voxels per load where D % 4 == 0 and the base is aligned, and issues six integer
 *     atomicMin / atomicMax per workgroup that saw foreground.  No host synchronisation; exact and bitwise reproducible.
 *   mivp_window_fit_plan: the work list of the windows that tile the box.  Per axis, with p = pdims, r = roi, m = margin,
 *     the box [lo, hi]: b0 = max(lo + pad - m, 0), b1 = min(hi + pad + m + 1, p), n = b1 - b0; if n < r then
 *     b0 = clamp(b0 - (r - n) / 2, 0, p - r) and n = r; count = ceil((n - r) / interval) + 1 and window i starts at
 *     b0 + min(i * interval, n - r).  interval: host int32 [3], max(int(r * (1 - overlap)), 1), in 1..r.  margin: host
 *     int32 [3], 0..2^30.  codes: host int32 [n_flips], the 3-bit flip codes (n_flips in 1..8).  table: DEVICE int32
 *     [n_entries][4], 16-byte aligned: entry w * n_flips + j = window w (row-major over the three counts) under codes[j],
 *     word 3 = 1 | code << 1; every remaining row is zero.  origins: DEVICE int32 [n_origins][3], the origins of the
 *     windows, zero behind them.  meta: DEVICE int32 [2] = (windows, entries).  An empty box (hi < lo on an axis, or a box
 *     outside the image) plans zero windows.  A plan of more than n_entries entries or n_origins windows writes an
 *     all-zero table and meta = (-1, -1); with the capacities of the full tiling it cannot happen (n <= p per axis).  One
 *     workgroup, no host synchronisation, nothing is written outside the capacities given. */
int mivp_foreground_box(const float* vol, int32_t Cin, int32_t channel, float threshold, const uint8_t* mask,
                        const int32_t* dims, int32_t* box, mivp_stream_t stream);
int mivp_window_fit_plan(const int32_t* box, const int32_t* dims, const int32_t* pad, const int32_t* pdims,
                         const int32_t* roi, const int32_t* interval, const int32_t* margin, const int32_t* codes,
                         int32_t n_flips, int32_t* table, int32_t n_entries, int32_t* origins, int32_t n_origins,
                         int32_t* meta, mivp_stream_t stream);

/* The four sources of the batch filler named below (csrc/crops.hip, crops_index.hip, crops_affine.hip, crops_corrupt.hip)
 * share csrc/crops_common.hpp: the slot record and table row decode, the quarter turn, the pad rule and the host checks. */
/* Training-batch sampling from a bank of resident scans (csrc/crops.hip; mivp_amd/batches.py).  These entry
 * points joined the current ABI without a bump: they are additive and no earlier signature changed.  One gather kernel
 * family (k_crop): every output voxel is written exactly once, no atomics, bitwise reproducible, no host synchronisation.
 * Whatever selects the crops is DEVICE memory (the slot), so a launch records into a graph and a replay follows whatever
 * the slot holds then.
 *   slot: DEVICE int32 [B][slot_stride], one record per sample: [0] volume id, [1] rotation code -- 0 none, 1 / 2 / 3 =
 *     rot90(k = 1) over the spatial axes (0,1) / (0,2) / (1,2) --, [2..4] the crop origin in the ROTATED frame; words 5..
 *     are the caller's (batches.py keeps the students' origins there).  slot_stride >= 5.
 *   roi: host int32 [3] = {h, w, d}, the output extents (each 1..65535; fewer than 2^31 voxels per output tensor).
 *   Rule for output voxel u of sample b, with n the stored extents and n_rot the rotated ones: r = origin + u - pad_before,
 *     pad_before = (roi - min(roi, n_rot)) / 2 per axis (the symmetric pad: the larger half comes after the crop).  r
 *     outside the rotated volume on any axis: every output is 0.  Otherwise p = r mapped back through the rotation (for
 *     axes (a, b): p_a = r_b, p_b = n_b - 1 - r_a) and image = vol[:, p], mask = lut[lab[p]], coord[k] = p[k] - (n[k] - 1) / 2.
 *   mivp_crop_fill: table DEVICE int64 [n_volumes][5] = (image pointer, label pointer or 0, H, W, D); images fp32
 *     [C][H][W][D] (C in 1..16, common to the bank), labels uint8 [H][W][D].  image fp32 [B][C][h][w][d]; mask fp32
 *     [B][1][h][w][d] or NULL (lut: DEVICE uint8 [256], required with mask; a volume without labels gives 0); coord fp32
 *     [B][3][h][w][d] or NULL.  A sample whose volume id is outside [0, n_volumes), whose table row is empty (image pointer
 *     0: the table may be a fixed-capacity one that the host fills in place, so that a recorded launch sees volumes added
 *     later) or whose code is outside 0..3 is left unwritten; any origin is safe (r is range-checked per voxel).  The host validates the draws before it uploads them.
 *   mivp_crop_tensor: the same kernel with sample b's source being row b of src fp32 [B][Cs][sdims] (Cs in 1..16): no
 *     rotation, no table, out fp32 [B][Cs][h][w][d]; the origin is read at slot[b * slot_stride + 0..2] (pass the slot
 *     pointer advanced to the origin words).  The student views are this call on the teacher's image, coord and mask.
 * Codes 0 and 1 keep D in place: rows move in 16-byte pieces (4-byte aligned) with a scalar path at the edges; codes 2
 * and 3 exchange D with H or W and move 64 x 64 tiles through LDS so that loads and stores both run along D. */
int mivp_crop_fill(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot, int32_t slot_stride, int32_t B,
                   const int32_t* roi, const uint8_t* lut, float* image, float* mask, float* coord, mivp_stream_t stream);
int mivp_crop_tensor(const float* src, int32_t Cs, const int32_t* sdims, const int32_t* slot, int32_t slot_stride,
                     int32_t B, const int32_t* roi, float* out, mivp_stream_t stream);

/* Class-balanced crop centres for the batch filler (csrc/crops_index.hip; mivp_amd/batches.py).  Additive
 * again: the ABI stays 18.  The centre of a crop is the rank-th voxel, in C order of the stored [H][W][D] label map, of
 * class cls of the sample's volume (RandCropByPosNegLabeld / RandCropByLabelClassesd); the device resolves it from a
 * per-volume index and writes the crop origin into the slot record that mivp_crop_fill reads.  Integers only, no atomics,
 * bitwise reproducible, no host synchronisation; the pick records into a graph.
 *   class of a voxel: c = lut[lab] (lut: DEVICE uint8 [256]); the voxel belongs to class c if c < num_classes (1..16),
 *     otherwise to no class.  A chunk is 1024 consecutive voxels; nchunks = ceil(numel / 1024).
 *   mivp_label_index_build: labels DEVICE uint8 [numel] (1 <= numel < 2^31; any alignment, dword loads where it is
 *     4-byte aligned) -> index DEVICE int32 [num_classes][nchunks + 1]: row c holds the exclusive prefix sums of the
 *     per-chunk counts of class c, the last column is the class total.  Two launches: a count (one 256-thread workgroup
 *     per chunk, lane t reads voxels 4 t .. 4 t + 3 of the chunk, wave ballots and popcounts) and a scan (one workgroup per
 *     class, in place, ascending).  MIVP_EINVAL for null pointers, non-positive sizes, num_classes outside 1..16 and an
 *     nchunks other than ceil(numel / 1024).
 *   mivp_crop_pick: table = the bank's source table of mivp_crop_fill; index_table DEVICE int64 [n_volumes][2] = (pointer
 *     to the volume's index or 0, its nchunks); slot as for mivp_crop_fill (this call WRITES words 2..4 of a record);
 *     pick DEVICE int32 [B][2] = (cls, rank); roi host int32 [3].  One 256-thread workgroup per sample: a binary search
 *     of the class's prefix row for the chunk j with prefix[j] <= rank < prefix[j + 1], the chunk's labels with the
 *     count's lane-to-voxel map, the (rank - prefix[j])-th match q by popcounts and ballots, q -> p = (q / (W D),
 *     (q / D) % W, q % D), p -> r through the rotation (for axes (a, b): r_b = p_a, r_a = n_b - 1 - p_b, the inverse of the
 *     rule above), and origin[k] = clamp(r[k] - roi[k] / 2, 0, max(n_rot[k] - roi[k], 0)) (MONAI's correct_crop_centers),
 *     stored by the one lane that holds the voxel.  A sample whose volume id is outside [0, n_volumes), whose index row or
 *     label pointer is 0, whose nchunks does not fit the volume, whose class is outside [0, num_classes), whose rank is
 *     outside [0, total) or whose code is outside 0..3 is left unwritten.  The host validates the draws before it
 *     uploads them. */
int mivp_label_index_build(const uint8_t* labels, int64_t numel, const uint8_t* lut, int32_t num_classes, int32_t* index,
                           int32_t nchunks, mivp_stream_t stream);
int mivp_crop_pick(const int64_t* table, const int64_t* index_table, int32_t n_volumes, const uint8_t* lut,
                   int32_t num_classes, int32_t* slot, int32_t slot_stride, const int32_t* pick, int32_t B,
                   const int32_t* roi, mivp_stream_t stream);

/* Random flip, rotation and zoom for the batch filler (csrc/crops_affine.hip; mivp_amd/batches.py).  Additive
 * again: the ABI stays 18.  The teacher launch of mivp_crop_fill with an affine map per sample and interpolation: every
 * output voxel is written exactly once, no atomics, bitwise reproducible, no host synchronisation; the map is DEVICE
 * memory like the slot, so the launch records into a graph and a replay follows what both hold then.
 *   affine: DEVICE fp32 [B][12]: A row-major (9 words: output offset -> source offset), then the sub-voxel shift s (3).
 *   Rule for output voxel u of sample b; origin, rot, n, n_rot and pad_before exactly as for mivp_crop_fill above; all
 *   arithmetic is fp32, per axis k:
 *       q = u - (roi - 1) / 2
 *       r_k = fma(A_k2, q_2, fma(A_k1, q_1, A_k0 * q_0)) + ((roi_k - 1) / 2 + (origin_k - pad_before_k) + s_k)
 *     image: trilinear.  i = floor(r), w = r - i; of the eight corners i + e, one outside [0, n_rot) on any axis reads 0,
 *       the others read vol[:, p(corner)] with p the corner mapped back through the quarter turn as above; interpolated
 *       along D first, then W, then H, each step a + w * (b - a).
 *     mask: j = floor(r + 0.5); lut[lab[p(j)]] if j is inside [0, n_rot) on every axis, else 0 (0 without a label map).
 *     coord: under the mask's inside test the continuous r mapped back through the quarter turn (for axes (a, b):
 *       p_a = r_b, p_b = (n_b - 1) - r_a), coord[k] = p[k] - (n[k] - 1) / 2; otherwise 0.
 *     a non-finite r_k gives 0 in every output (float comparisons before any conversion to an integer).
 *   With A = diag(+-1) and s = 0 every r is an exact integer and every w is 0: the outputs equal mivp_crop_fill's (at the
 *   mirrored voxel) bit for bit.  With dyadic A and s and small integer voxel values every step is exact in fp32.
 *   mivp_crop_fill_affine: every other argument and every refusal as for mivp_crop_fill (an empty table row, a volume id
 *     outside [0, n_volumes) or a code outside 0..3 leaves the sample unwritten; MIVP_EINVAL for null required pointers
 *     and bad sizes).  One 256-thread workgroup per 8 x 8 x 16 output brick of one sample, each lane four voxels along d
 *     (16-byte stores), the eight corners of every voxel read from global memory, each range-checked (the direct path).
 *   mivp_crop_fill_affine_debug: the same launch with the staged path switched on by stage != 0.  A workgroup then bounds
 *     the source positions of its brick by a box (the eight brick corners through the map, one voxel of slack, clipped to
 *     the volume plus a one-voxel rim of zeros); if the box has at least two planes on every axis and e0 * e1 * (e2 | 1)
 *     <= 12288 cells it is staged into LDS once per channel, by rows along the stored D axis, and the corners come from
 *     LDS; otherwise (strong minification, a non-finite map) the workgroup takes the direct path.  Both paths give the
 *     same bits.  The staged path measured slower on typical draws, which is why the product entry does not
 *     take it.  paths (DEVICE int32 [B][bricks], bricks = ceil(h / 8) * ceil(w / 8) * ceil(d / 16), brick index
 *     ((bh * nbw) + bw) * nbd + bd; may be NULL) receives 1 where a workgroup took the staged path and 0 where the direct
 *     one.  For the tests and tools/bench_batches.py. */
int mivp_crop_fill_affine(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot, int32_t slot_stride,
                          const float* affine, int32_t B, const int32_t* roi, const uint8_t* lut, float* image, float* mask,
                          float* coord, mivp_stream_t stream);
int mivp_crop_fill_affine_debug(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot,
                                int32_t slot_stride, const float* affine, int32_t B, const int32_t* roi, const uint8_t* lut,
                                float* image, float* mask, float* coord, int32_t stage, int32_t* paths,
                                mivp_stream_t stream);

/* Elastic (non-rigid) deformation for the batch filler (csrc/crops_affine.hip; mivp_amd/batches.py).
 * Additive again: the ABI stays 18.  The affine teacher launch with one more term in the source position: a smooth
 * displacement evaluated on the fly from a small control lattice per sample.  No displacement volume is stored; every
 * output voxel is written exactly once, no atomics, bitwise reproducible, no host synchronisation; flags and lattice
 * are DEVICE memory like the slot and the map, so the launch records into a graph and a replay follows all of them.
 *   nodes: HOST int32 [3] = (n0, n1, n2), 4 <= n_k <= 8, the same for the whole batch.
 *   lattice: DEVICE fp32 [B][3][n0][n1][n2]: P[c][j0][j1][j2], component c of the displacement of node j, in output voxels.
 *   flags: DEVICE int32 [B]: 0 = the sample is not deformed, anything else = it is.
 *   Rule for output voxel u of a sample whose flag is not 0, all arithmetic fp32, per axis k:
 *       x_k = (u_k + 0.5) * ((n_k - 3) / roi_k)               (in (0, n_k - 3))
 *       i_k = min(floor(x_k), n_k - 4),  f_k = x_k - i_k
 *       the uniform cubic B-spline basis  B0 = (1 - f)^3 / 6,        B1 = (3 f^3 - 6 f^2 + 4) / 6,
 *                                         B2 = (-3 f^3 + 3 f^2 + 3 f + 1) / 6,  B3 = f^3 / 6
 *       d_c(u) = sum over a, b, e in 0..3 of B_a(f_0) B_b(f_1) B_e(f_2) * P[c][i_0 + a][i_1 + b][i_2 + e]
 *       r = A (q + d(u)) + t
 *     with q, A and t exactly as for mivp_crop_fill_affine: the offset first, then the affine map (MONAI's order).  The sum
 *     q_k + d_k is formed first and goes through the same fma chain, so a displacement of exactly 0.0f gives that launch's
 *     r bit for bit.  The order of the sum: w_ab = B_a(f_0) * B_b(f_1); per lattice column i_2 + e the 16 taps accumulate
 *     by fma over a, then b, from w_00 * P; then d_c = fma over e = 1..3 onto B_0(f_2) * column 0.
 *     Everything after r is mivp_crop_fill_affine's: the trilinear image with zeros outside, the mask through the lut at
 *     floor(r + 0.5), coord = r mapped back through the quarter turn.  A non-finite or huge displacement gives a
 *     non-finite or far r, which fails the float comparisons in front of every conversion to an integer: zeros.
 *   A sample whose flag is 0 never reads the lattice (which may then hold anything): its workgroups run the arithmetic of
 *     mivp_crop_fill_affine and give its bits.  The branch is uniform per workgroup.
 *   mivp_crop_fill_elastic: every other argument and every refusal as for mivp_crop_fill_affine; MIVP_EINVAL also for a
 *     null flags, lattice or nodes and for a node count outside 4..8.  The same bricks and lanes; a deformed sample's
 *     workgroups stage its lattice (at most 6 KiB) in LDS and read every corner from global memory (the direct path: the
 *     staged path's box is bounded through an affine map, which does not hold under a deformation).  A lane's four voxels
 *     share (u_0, u_1), so the 16-tap sums are formed once per lattice column its voxels touch. */
int mivp_crop_fill_elastic(const int64_t* table, int32_t n_volumes, int32_t C, const int32_t* slot, int32_t slot_stride,
                           const float* affine, int32_t B, const int32_t* roi, const uint8_t* lut, float* image, float* mask,
                           float* coord, const int32_t* flags, const float* lattice, const int32_t* nodes,
                           mivp_stream_t stream);

/* The students' own corruption for the batch filler (csrc/crops_corrupt.hip; mivp_amd/batches.py): the
 * reference's students_rand_ts (datasets/transforms.py:244-297) -- nothing, RandCoarseDropoutd with dropout_holes True or
 * False, RandCoarseShuffled -- in place on a student's image tensor, after the student crop.  Additive again: the ABI stays
 * 18.  No atomics, no host synchronisation, bitwise reproducible; the records are DEVICE memory like the slot, so both
 * launches record into a graph and a replay follows what the records hold then.  MONAI's own streams are not reproduced.
 *   x: DEVICE fp32 [B][C][dims] (C in 1..16; dims host int32 [3], each 1..65535, C * voxels < 2^31), corrupted IN PLACE.
 *   records: DEVICE int32 [B][MIVP_CORRUPT_RECORD_WORDS], one per sample: [0] mode, [1] the number of holes n (0..8),
 *     [2] the noise key (32 bits), then 8 holes of 7 words: origin[3], size[3], the hole's shuffle key (32 bits).  Holes
 *     n.. are not read.  A hole is the box origin <= u < origin + size, size >= 1, inside dims on every axis.
 *   Rule for sample b by its mode:
 *     0: the sample is not written at all (its workgroups return).
 *     1 (dropout): every voxel inside the union of the holes, in every channel, is replaced by noise.
 *     2 (keep): every voxel OUTSIDE the union of the holes, in every channel, is replaced by noise.
 *       noise at element i = ((c * h + u0) * w + u1) * d + u2 of the sample (its linear index over [C][dims]):
 *         lo, hi = the minimum and maximum of the sample over all channels BEFORE the corruption (fminf / fmaxf: values are
 *           expected finite), each with +0.0f added so that a zero extreme is +0 whatever the order of the reduction;
 *         t = i + key; t ^= t >> 16; t = (t & 0xFFFFFF) * 0xB5AD4F; t ^= t >> 13;
 *         hash = (t & 0xFFFFFF) * 0x6C62B9 + (t >> 8) + rotl(key, 13)      (all mod 2^32: the dropout hash of common.hpp,
 *           full-rate 24-bit multiplies only);
 *         u = (hash >> 8) * 2^-24 in [0, 1);  value = lo + (hi - lo) * u, fp32, the difference, the product and the sum
 *           each rounded to nearest, never contracted.  lo == hi gives exactly lo.  (The value lies in [lo, hi) before
 *           the last rounding, which can reach hi when u is within a few ulp of 1.)
 *     3 (shuffle): for each hole in list order, and for each channel alone: with n = the hole's voxel count (<= 4096),
 *       voxel j = (u0 * size1 + u1) * size2 + u2 of the hole (C order of its own extents) receives the value voxel P(j)
 *       held before this hole was applied; later holes see what earlier ones wrote.  Every channel uses the same P
 *       (MONAI permutes across channels; at one channel the two coincide).
 *       P: bits = max(2, the next even number >= ceil(log2 n)), half = bits / 2, mask = 2^half - 1; v = j; repeat
 *         { l = v >> half, r = v & mask; four rounds r' = l ^ ((hash(r + 64 * round, key) >> 16) & mask), l' = r, with the
 *         hash above and key = the hole's; v = (l << half) | r } until v < n; P(j) = v.  A Feistel network is a bijection
 *         of the 2^bits values, and walking it until it returns below n makes P a bijection of {0 .. n-1}.
 *   mivp_crop_corrupt_range: range DEVICE fp32 [B][MIVP_CORRUPT_PARTIALS][2], scratch: workgroup p of a sample in mode 1
 *     or 2 writes the (min, max) of its share of the sample; other samples' rows are left alone.  16-byte loads at 4-byte
 *     alignment with a scalar tail for a voxel count that is no multiple of 4.
 *   mivp_crop_corrupt: reads range (written by the call above on the same stream) and the records and applies the rule.
 *     Modes 1 and 2 only store: 16 bytes where four voxels along d are all replaced, single voxels elsewhere and in the
 *     d % 4 tail.  Mode 3 stages each hole in LDS (16 KB at the bound) in one workgroup per (sample, channel).
 *   Both: MIVP_EINVAL, before any launch, for a null or misaligned pointer and for sizes outside the ranges above.  The
 *     records are device memory the host entry cannot see: a sample whose mode is above 3, whose hole count is above 8,
 *     one of whose holes is empty or reaches outside dims, or (mode 3) holds more than 4096 voxels, is left unwritten by
 *     the kernel.  The host validates the draws before it uploads them (batches.CorruptionDraws.check). */
#define MIVP_CORRUPT_MAX_HOLES 8
#define MIVP_CORRUPT_RECORD_WORDS 59
#define MIVP_CORRUPT_SHUFFLE_VOXELS 4096
#define MIVP_CORRUPT_PARTIALS 64
int mivp_crop_corrupt_range(const float* x, int32_t C, const int32_t* dims, const int32_t* records, int32_t B,
                            float* range, mivp_stream_t stream);
int mivp_crop_corrupt(float* x, int32_t C, const int32_t* dims, const int32_t* records, int32_t B, const float* range,
                      mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Pixel-space visual prompt (csrc/input_prompt.hip)                        */
/* ------------------------------------------------------------------------ */
/* y = x + scale[0] * T(p): x, y f32 [B,Cin,H,W,D]; p f32 [Cin,gh,gw,gd]; scale a DEVICE float; T = trilinear
 * interpolation of the lattice to the roi under torch's align_corners=True rule, evaluated on the fly (no roi-sized
 * prompt volume).  Voxel o of an axis sits at o (g-1) / (n-1) as an exact rational (0 when g == 1 or n == 1):
 * i0 = floor, lambda = remainder / (n-1), i1 = min(i0+1, g-1); g == n gives lambda == 0 everywhere (y = x + scale p).
 * The lattice is staged in LDS up to 32 KiB, read from global memory above.  1 <= g <= n per axis, H+W+D <= 4096,
 * B Cin H W D < 2^31.
 * mivp_input_prompt_bwd: dp[ci][node] = scale[0] * sum_b sum_voxels weight * dy, a gather per node over its support
 * in a fixed order (stated in the source file): no atomics, nothing zero-filled, equal calls give equal bits. */
int mivp_input_prompt_fwd(const float* x, const float* p, const float* scale, int32_t B, int32_t Cin, int32_t H, int32_t W,
                          int32_t D, int32_t gh, int32_t gw, int32_t gd, float* y, mivp_stream_t stream);
int mivp_input_prompt_bwd(const float* dy, const float* scale, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t D,
                          int32_t gh, int32_t gw, int32_t gd, float* dp, mivp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Multi-label targets: overlapping label groups (csrc/multilabel.hip)      */
/* ------------------------------------------------------------------------ */
/* Loss, decode and counts for R overlapping label GROUPS with one sigmoid channel each (mivp_amd/multilabel.py LabelGroups /
 * MultiLabelSpec / multilabel_loss / decode_groups / group_counts).  These entry points joined ABI 18 without a
 * bump: they are additive and no earlier signature changed.
 *
 * member: DEVICE int32 [256]; bits 0..R-1 of entry l = the groups that contain label l, bit 8 = l is a known label.
 * lut:    DEVICE uint8 [2^R]; the label of each pattern of predicted groups.
 *
 * Loss.  logits f32 [B, vol, R] channels-last (1 <= R <= 8), target f32 [B, vol] labels.  A voxel is VALID when its label is
 * an integer in 0..255, known (member bit 8) and, with has_ignore != 0, differs from ignore_index (compared as a float);
 * V = the valid voxels, N = |V| over the whole batch.  With t_r = [label in group r], p_r = sigmoid(z_r), s = 1e-5 and sums
 * over V of a sample (of the whole batch when batch != 0):
 *   I_r = sum p_r t_r,  P_r = sum p_r,  T_r = sum t_r
 *   TI_r   = (2 I + s) / (2 I + 2 alpha (P - I) + 2 beta (T - I) + s)
 *   region = mean over (b, r) [over r when batch] of 1 - TI_r
 *   f_r    = w_r [ t_r pi_r (1 - p_r)^gamma (-log p_r) + (1 - t_r) p_r^gamma (-log(1 - p_r)) ]
 *   voxel  = sum_{v in V} sum_r f_r / (R max(N, 1))
 *   loss[0] = lambda_region region + lambda_voxel voxel
 * An invalid voxel adds to no sum and gets an exactly zero gradient in all R channels.  log p and log(1 - p) come from
 * e = exp(-|z|), log1p(e) and one reciprocal: finite, and with their digits, at |z| = 30.  alpha, beta >= 0; gamma =
 * focal_gamma == 0 or >= 1; lambda_region, lambda_voxel >= 0, not both 0; group_weights (w) and pos_weight (pi): DEVICE
 * pointers to R floats >= 0, NULL = all ones (the values are not read back to be checked).
 * workspace: mivp_multilabel_loss_ws(B, vol) floats, the layout of mivp_seg_loss_ws (row: (I, P, T) x 8 groups, voxel
 * numerator, N).  Three launches: a statistics pass with one partial row per workgroup, a one-workgroup f64 finalize in a
 * fixed order, and the gradient pass.  dlogits may be NULL: the value alone; mivp_multilabel_loss_grad then runs the gradient
 * pass on the SAME workspace with the SAME options, scaled by gscale[0] (device pointer, NULL = 1); it writes every element
 * of dlogits once.  No atomics, no host read, every launch unconditional: equal calls give equal bits. */
size_t mivp_multilabel_loss_ws(int32_t B, int64_t vol);
int mivp_multilabel_loss(const float* logits, const float* target, int32_t B, int64_t vol, int32_t R,
                         const int32_t* member, int32_t batch, float alpha, float beta, float focal_gamma,
                         const float* group_weights, const float* pos_weight, int32_t ignore_index, int32_t has_ignore,
                         float lambda_region, float lambda_voxel, float* workspace, float* loss, float* dlogits,
                         mivp_stream_t stream);
int mivp_multilabel_loss_grad(const float* logits, const float* target, int32_t B, int64_t vol, int32_t R,
                              const int32_t* member, int32_t batch, float alpha, float beta, float focal_gamma,
                              const float* group_weights, const float* pos_weight, int32_t ignore_index,
                              int32_t has_ignore, float lambda_region, float lambda_voxel, float* workspace,
                              const float* gscale, float* dlogits, mivp_stream_t stream);

/* Decode, one streaming launch.  logits f32 [B][R][vol] (channels_last == 0) or [B][vol][R]; thresholds: DEVICE f32 [R] in
 * logit space (the host turns a probability q into log(q / (1 - q)); q = 0.5 is exactly 0).  bits = sum_r [z_r > tau_r] << r
 * (a logit equal to its threshold gives bit 0).  Each output is written when its pointer is non-NULL (at least one is):
 * labels uint8 [B][vol] = lut[bits], bits uint8 [B][vol], probs f32 [B][R][vol] = sigmoid(z).  With vol % 4 == 0 and aligned
 * pointers a thread owns four voxels: 16-byte loads, one 32-bit store per byte map, 16-byte stores of the probabilities. */
int mivp_multilabel_decode(const float* logits, int32_t B, int64_t vol, int32_t R, int32_t channels_last,
                           const float* thresholds, const uint8_t* lut, uint8_t* labels, uint8_t* bits, float* probs,
                           mivp_stream_t stream);

/* Group counts, one launch: counts int64 [R][3] += (|pred_r & t_r|, |pred_r|, |t_r|) over the valid voxels of target (the
 * validity rule of the loss; nvox < 2^31).  dtype codes: 0 = uint8, 3 = float32.  pred is a bits map (pred_is_labels == 0;
 * uint8) or a label map mapped through member (pred_is_labels != 0; a predicted value that is no label in 0..255 is in no
 * group).  Per-wave ballots and popcounts, an LDS table, one set of 64-bit integer atomics per workgroup: the result does
 * not depend on the order.  counts accumulates across calls, like mivp_seg_counts. */
int mivp_group_counts(const void* pred, int32_t pred_dtype, int32_t pred_is_labels, const void* target,
                      int32_t target_dtype, int64_t nvox, int32_t R, const int32_t* member, int32_t ignore_index,
                      int32_t has_ignore, int64_t* counts, mivp_stream_t stream);

/* Interactive click prompts (csrc/clicks.hip; mivp_amd/clicks.py).  These entry points joined ABI 18 without a
 * bump: they are additive and no earlier signature changed.
 *
 * The record of a batch, all DEVICE memory: clicks i32 [B][K][4] = (h, w, d, channel), 16-byte aligned, channel 0 = positive,
 * 1 = negative, any other value = an empty entry; count i32 [B], the first count[b] entries of sample b are read (clamped to
 * 0 .. K); last i32 [B][4], 16-byte aligned, written by the simulation.  1 <= K <= 64, 1 <= B <= 65535.
 *
 * mivp_clicks_encode, one launch: out f32 [B][Ctot][H][W][D] (dims = {H, W, D}, host; H, W, D <= 65535, H W D < 2^31).  Writes
 * channels channel_offset and channel_offset + 1 (0 <= channel_offset <= Ctot - 2) of every sample, every element of them stored
 * exactly once, and no other byte.  Per voxel v and channel c, over the valid clicks p of sample b with that channel:
 *   m = min_p sum_a (spacing[a] (v_a - p_a))^2        +inf without a click; the exact integer at spacing {1, 1, 1}
 *   kind 0 (gaussian): expf(-m / param), param = 2 sigma^2 > 0      kind 1 (disk): m <= param ? 1 : 0, param = radius^2 >= 0
 * A channel without a click is +0 everywhere.  spacing: host f32 {s0, s1, s2} mm, > 0.  count is read on the device and the
 * launch is unconditional: a recording follows later slot contents.  out needs 4-byte alignment only; stores are 16 bytes
 * wide wherever the two channels' run allows (unaligned head and tail of at most 3 floats each per sample).
 *
 * mivp_clicks_simulate: the next corrective click per sample.  pred / target: class maps [B][H][W][D] of dtype 0 uint8,
 * 1 int32, 2 int64, 3 float32; a value that is no integer in 0 .. 31 is no class.  pred_dtype 4: pred is f32 logits
 * [B][vol][C] channels-last (1 <= C <= 32) and the class is the LOWEST index among the exact maxima (C is ignored otherwise).
 * The object = the classes whose bit is set in object_mask.
 *   E_pos = {target in the object, pred not}  -> a positive click (channel 0)
 *   E_neg = {pred in the object, target a class outside it}  -> a negative click (channel 1)
 * A voxel whose target is no class, or equals ignore_index with has_ignore != 0, is in neither.
 *   depth^2(v), v in a region = the squared distance sqrt(sum_a (spacing[a] delta_a)^2)^2 to the nearest voxel of the sample
 *   outside that region, the space beyond the volume counting as outside (the transform of the mask padded by one voxel):
 *   min(the exact transform inside the volume, min_a (spacing[a] (distance to the nearest face along a, >= 1))^2).
 * The click is the voxel with the largest depth^2 over both regions, ties to E_pos, then to the lowest raster index
 * (h W + w) D + d.  last[b] = {bits of depth^2, channel, raster index, placed} or {0, -1, -1, 0} when both regions are empty.
 * The click is appended at clicks[b][count[b]] and count[b] incremented iff a region exists, depth^2 >= min_depth_sq and
 * 0 <= count[b] < K (placed = 1); otherwise clicks and count are untouched.  Five launches whatever B and the data are (seed
 * / D pass, W pass, H pass, pick, commit), each unconditional, nothing read back, no float atomics: one 64-bit integer
 * atomicMax per workgroup on a packed key, so equal calls give equal bits.  Exact integers at unit spacing.
 * Limits: H, W <= 65535, H W D < 2^31.  workspace: mivp_clicks_simulate_ws(B, dims) bytes (0 for arguments the call would
 * refuse), 256-byte aligned: the squared fields f32 [2][B][vol], the lower envelope's stack (int32 pairs), the keys u64 [B]. */
int mivp_clicks_encode(const int32_t* clicks, const int32_t* count, int32_t B, int32_t K, int32_t Ctot,
                       int32_t channel_offset, const int32_t* dims, const float* spacing, int32_t kind, float param,
                       float* out, mivp_stream_t stream);
size_t mivp_clicks_simulate_ws(int32_t B, const int32_t* dims);
int mivp_clicks_simulate(const void* pred, int32_t pred_dtype, int32_t C, const void* target, int32_t target_dtype,
                         int32_t B, const int32_t* dims, const float* spacing, uint32_t object_mask,
                         int32_t ignore_index, int32_t has_ignore, float min_depth_sq, int32_t K, int32_t* clicks,
                         int32_t* count, int32_t* last, void* workspace, mivp_stream_t stream);

/* Box and scribble prompts (csrc/strokes.hip; mivp_amd/strokes.py).  These entry points joined ABI 18 without a
 * bump: they are additive and no earlier signature changed.
 *
 * The record of a batch, all DEVICE memory, 4-byte aligned: boxes i32 [B][KB][7] = (h0, w0, d0, h1, w1, d1, channel), corners
 * inclusive with lo <= hi, channel 0 = positive, 1 = negative, any other value = an empty row; box_count i32 [B], the first
 * box_count[b] rows of sample b are read (clamped to 0 .. KB); mask u8 [B][H][W][D], bit 0 = a positive scribble voxel, bit 1 =
 * a negative one, its storage a multiple of 4 bytes long; last i32 [B][8], written by the simulations; scratch i32 [B][8], all
 * zero between calls.  1 <= KB <= 16, 1 <= B <= 65535, dims = {H, W, D} (host), 1 <= H, W, D <= 65535, B (H + 2) W D < 2^31.
 * spacing: host f32 {s0, s1, s2} mm, > 0.  Label maps [B][H][W][D] of dtype 0 uint8, 1 int32, 2 int64, 3 float32; a value that
 * is no integer in 0 .. 31 is no class; the object = the classes whose bit is set in object_mask; a voxel whose target is no
 * class, or equals ignore_index with has_ignore != 0, is not valid.  Nothing is read back and no float atomic is used: equal
 * calls give equal bits.
 *
 * mivp_strokes_draw, one launch: points DEVICE i32 [npts][3], 1 <= npts <= 256, every point inside the volume.  Each pair
 * a -> b of consecutive points sets bit `channel` of the voxels a + floor((2 i delta + n) / (2 n)), i = 0 .. n, delta = b - a,
 * n = max |delta_a| (floor towards minus infinity, per axis; n = 0 or a single point: that voxel) of sample b.  max_steps >= the
 * largest n of the polyline.  One thread per (segment, step), an integer atomicOr on the containing 32-bit word.
 *
 * mivp_strokes_encode, four launches whatever the record holds (seed / D pass, W pass, H pass, closing pass): out f32
 * [B][Ctot][H][W][D]; channels channel_offset and channel_offset + 1 of every sample are written, every element of them exactly
 * once, and no other byte.  Per voxel v and channel c the value is max(box, stroke):
 *   box     1 where v is inside a box of the channel (frame == 0), or inside one with a coordinate equal to that box's lo or
 *           hi (frame != 0: the surface), else 0
 *   stroke  m = min over the scribble voxels p of the channel of sum_a (spacing[a] (v_a - p_a))^2, the exact transform (the
 *           exact integer at spacing {1, 1, 1}); kind 0 (gaussian): expf(-m / param), param = 2 sigma^2 > 0; kind 1 (disk):
 *           m <= param ? 1 : 0, param = radius^2 >= 0; +0 without a scribble voxel
 * out needs 4-byte alignment only; stores are 16 bytes wide wherever the two channels' run allows.
 *
 * mivp_strokes_box, two launches (reduction, finalize): (lo, hi) = the tight bounding box of the valid object voxels of the
 * target per sample; lo' = clamp(lo - margin + jitter[b][0..2], 0, hi), hi' = clamp(hi + margin + jitter[b][3..5], lo,
 * dim - 1) per axis (margin: host i32 {3} >= 0; jitter: DEVICE i32 [B][6] or NULL).  The row (lo', hi', channel) is appended at
 * boxes[b][box_count[b]] and box_count[b] incremented iff the object is not empty and 0 <= box_count[b] < KB.  last[b] =
 * {lo', hi', placed, 0}, or {-1 x 6, 0, 0} for an empty object.  One set of integer atomicMax per workgroup and sample.
 *
 * mivp_strokes_scribbles: E_pos / E_neg and depth^2 as in mivp_clicks_simulate; the core of a region = {depth^2 >=
 * min_depth_sq}; the scribble = the curve skeleton of each core by the thinning of mivp_skeleton_iter (classes 1 = E_pos,
 * 2 = E_neg, each thinned on its own, max_iter iterations issued, 1 <= max_iter <= 4096), per sample what that thinning gives
 * on the sample's own [H][W][D] core map.  Positive skeleton voxels set bit 0 of mask, negative ones bit 1; bits already there
 * stay.  last[b] = {voxels that gained bit 0, voxels that gained bit 1, converged, 0, 0, 0, 0, 0}; converged = 1 when the
 * thinning of the batch stopped by itself within max_iter.  6 + 9 max_iter launches at most (fewer where an axis has extent
 * 1), the count a function of dims and max_iter alone, each unconditional.
 *
 * workspace: mivp_strokes_ws(B, dims) bytes (0 for arguments the calls would refuse), 256-byte aligned, serves both
 * mivp_strokes_encode and mivp_strokes_scribbles: the squared fields f32 [B][2][vol], the lower envelope's stack (int32
 * pairs), two class maps of the batch stacked along H, the thinning's workspace and two state words. */
int mivp_strokes_draw(const int32_t* points, int32_t npts, int32_t max_steps, int32_t b, int32_t channel, int32_t B,
                      const int32_t* dims, uint8_t* mask, mivp_stream_t stream);
size_t mivp_strokes_ws(int32_t B, const int32_t* dims);
int mivp_strokes_encode(const int32_t* boxes, const int32_t* box_count, const uint8_t* mask, int32_t B, int32_t KB,
                        int32_t Ctot, int32_t channel_offset, const int32_t* dims, const float* spacing, int32_t frame,
                        int32_t kind, float param, float* out, void* workspace, mivp_stream_t stream);
int mivp_strokes_box(const void* target, int32_t target_dtype, int32_t B, const int32_t* dims, uint32_t object_mask,
                     int32_t ignore_index, int32_t has_ignore, const int32_t* margin, const int32_t* jitter, int32_t channel,
                     int32_t KB, int32_t* boxes, int32_t* box_count, int32_t* last, int32_t* scratch, mivp_stream_t stream);
int mivp_strokes_scribbles(const void* pred, int32_t pred_dtype, const void* target, int32_t target_dtype, int32_t B,
                           const int32_t* dims, const float* spacing, uint32_t object_mask, int32_t ignore_index,
                           int32_t has_ignore, float min_depth_sq, int32_t max_iter, int32_t keep_endpoints, uint8_t* mask,
                           int32_t* last, void* workspace, mivp_stream_t stream);

/* Geodesic (image-aware) distance guidance for click and scribble prompts (csrc/geodesic.hip; mivp_amd/geodesic.py, DESIGN
 * 4.48).  These entry points joined ABI 18 without a bump: they are additive and no earlier signature changed.
 *
 * Per sample b and plane r (0 positive, 1 negative), over the 26-neighbour voxel graph of the [H][W][D] volume:
 *   g(v) = min over paths seed -> v of the left-to-right float32 sum of w(u, u')
 *   w(u, u') = sqrt(l2 + (gamma (I(u) - I(u')))^2), l2 = (a_h |dh| + a_w |dw|) + a_d |dd|, a = the f32 squares of spacing
 * every operation a separately rounded float32 one, the square root correctly rounded.  g = 0 at a seed, +inf in a plane without
 * seeds; an edge whose weight is not finite is never taken.  The converged field equals a float32 Dijkstra's in every bit.
 * I = channel `channel` of image f32 [B][C][H][W][D].  dims = {H, W, D} (host), 1 <= H, W, D <= 65535, B H W D < 2^31,
 * 1 <= B <= 65535; spacing: host f32 {s0, s1, s2} mm, finite and > 0 (their squares too); gamma finite and >= 0.  Every entry
 * refuses other arguments before it touches a pointer.  No float atomics; equal calls give equal bits, converged or not.
 *
 * workspace: mivp_geodesic_ws bytes (0 for arguments the calls would refuse), 256-byte aligned: [room for the seed mask, B H W
 * D bytes][F0 f32 [B][2][vol]][F1, the same][counters i32 [min(vol, 65535) + 1]][room for info, 8 bytes], each part rounded
 * up to 256 bytes; the first and the last part are the caller's, no entry reads or writes them through `workspace`.
 *
 * mivp_geodesic_seed, one launch, two with clicks: seeds u8 [B][H][W][D] (4-byte aligned, its storage a multiple of 4 bytes
 * long; the front of the workspace serves) = bits 0 and 1 of stroke_mask (the mask of a stroke record; NULL: none) | bit
 * `channel` at every click of the first count[b] (clamped to 0 .. K) entries of clicks i32 [B][K][4] (the click record, 1 <= K
 * <= 64; NULL with count NULL: none); an entry whose channel is neither 0 nor 1, or that lies outside the volume, is skipped.
 * One integer atomicOr per click on the containing 32-bit word.
 * mivp_geodesic_begin: F0 = F1 = (bit r of seeds ? 0 : +inf) and the counters.
 * mivp_geodesic_iter: iteration number `iteration` (1, 2, 3, .. in this order after mivp_geodesic_begin, at most min(vol,
 * 65535)): reads F[(iteration + 1) & 1], writes F[iteration & 1] = that field relaxed inside every 16 x 16 x 32 brick (with the
 * brick's one-voxel halo held fixed) until the brick stops changing, and adds the number of voxels it lowered to its counter.
 * It returns at once when the previous iteration lowered nothing.  One launch, unconditional on the host.
 * mivp_geodesic_end: after `iterations` iterations were issued, info[0] (DEVICE i32 [2]) = the number of them that lowered a
 * voxel, info[1] = 1 when the last one lowered nothing (the field is the fixed point), else 0.  The field is F[iterations & 1];
 * once converged, both buffers hold it.
 * mivp_geodesic_encode, one launch: out f32 [B][Ctot][H][W][D]; channels channel_offset and channel_offset + 1 of every sample
 * are written, every element of them exactly once, and no other byte (the walk of mivp_strokes_encode).  Per voxel and channel
 * the value is max(box, f(g)), g from F[iterations & 1], m = g g in float32; kind 0 (gaussian): f = expf(-m / param), param = 2
 * sigma^2 > 0; kind 1 (disk): f = m <= param ? 1 : 0, param = radius^2 >= 0; g = +inf gives +0.  box: the rule of
 * mivp_strokes_encode on boxes / box_count (1 <= KB <= 16), or none with both NULL. */
size_t mivp_geodesic_ws(int32_t B, const int32_t* dims);
int mivp_geodesic_seed(const uint8_t* stroke_mask, const int32_t* clicks, const int32_t* count, int32_t K, int32_t B,
                       const int32_t* dims, uint8_t* seeds, mivp_stream_t stream);
int mivp_geodesic_begin(const uint8_t* seeds, int32_t B, const int32_t* dims, void* workspace, mivp_stream_t stream);
int mivp_geodesic_iter(int32_t iteration, const float* image, int32_t C, int32_t channel, int32_t B, const int32_t* dims,
                       const float* spacing, float gamma, void* workspace, mivp_stream_t stream);
int mivp_geodesic_end(int32_t iterations, int32_t B, const int32_t* dims, const void* workspace, int32_t* info,
                      mivp_stream_t stream);
int mivp_geodesic_encode(const int32_t* boxes, const int32_t* box_count, int32_t KB, int32_t iterations, int32_t B,
                         int32_t Ctot, int32_t channel_offset, const int32_t* dims, int32_t frame, int32_t kind, float param,
                         float* out, const void* workspace, mivp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIVP_H */
