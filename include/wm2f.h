/*
 * wm2f.h -- C ABI of libwm2f.so: hand-written HIP (gfx950 / MI355X) kernels for the
 * Mask2Former hot path of marco-conciatori-public/weed_instance_segmentation.
 *
 * The reference has no FFI for this path: it calls the Python package `transformers`
 * (train.py:196, metrics.py:56, inference.py:27).  Each entry point below therefore
 * cites the Python function of that dependency whose arithmetic it replaces
 * ("HF:n" = transformers/models/mask2former/modeling_mask2former.py line n,
 *  "TORCHF:n" = torch/nn/functional.py line n, transformers 5.15.0 / torch 2.10).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory unless marked "host";
 *     tensors are contiguous, row-major, in the shape written next to them;
 *   - nothing is allocated, freed or retained; there is no global mutable state (host or device) and no
 *     environment variable is read: behaviour is a function of the arguments alone;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), no hidden syncs;
 *   - return 0 on success, a negative WM2F_E* code otherwise; wm2f_last_error() gives the
 *     thread-local message of the last failing call on this thread;
 *   - dtype: WM2F_F32 = 0 (fp32 storage + fp32 arithmetic); WM2F_BF16 = 1 where an entry point says so (bf16 storage of the
 *     named tensors, fp32 arithmetic).
 */
#ifndef WM2F_H
#define WM2F_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WM2F_VERSION 100 /* 0.1.0 */

#define WM2F_F32 0
#define WM2F_BF16 1
#define WM2F_I32 2 /* integer maps of the mAP entry points */
#define WM2F_U8 3
#define WM2F_U16 4 /* semantic maps of the CCL entry points */
#define WM2F_I64 5 /* class maps of wm2f_semantic_confusion */

#define WM2F_OK 0
#define WM2F_EINVAL (-1)      /* bad argument / unsupported shape */
#define WM2F_EUNSUPPORTED (-2) /* dtype or configuration not built */
#define WM2F_ELAUNCH (-3)     /* hipLaunch / runtime error */

#define WM2F_MAX_LEVELS 8

int wm2f_version(void);
const char* wm2f_last_error(void);

/* ---- K1: multi-scale deformable attention core ------------------------------------------
 * Replaces multi_scale_deformable_attention(), HF:798-837.
 *   value   (B, S, heads, D)        S = sum_l H_l*W_l, levels stored back to back
 *   loc     (B, Q, heads, L, P, 2)  normalised (x, y); pixel = loc * (W_l, H_l) - 0.5
 *   attn_w  (B, Q, heads, L, P)
 *   out     (B, Q, heads*D)
 *   level_hw  host int32 [L][2] = (H_l, W_l)
 * Bilinear, zero padding, align_corners = False.  D in {8, 16, 32, 64}.
 */
int wm2f_msdeform_fwd(const void* value, const void* loc, const void* attn_w, void* out,
                      const int32_t* level_hw, int B, int S, int Q, int heads, int D, int L, int P,
                      int dtype, void* stream);

/* Backward of the above.  grad_value (B,S,heads,D) must be ZEROED by the caller (it is
 * accumulated with float atomics); grad_loc, grad_attn_w are overwritten. */
int wm2f_msdeform_bwd(const void* value, const void* loc, const void* attn_w, const void* grad_out,
                      void* grad_value, void* grad_loc, void* grad_attn_w,
                      const int32_t* level_hw, int B, int S, int Q, int heads, int D, int L, int P,
                      int dtype, void* stream);

/* K1 backward with run-to-run identical results (same arguments and outputs as wm2f_msdeform_bwd plus a workspace of
 * wm2f_msdeform_bwd_det_workspace(level_hw, B, S, heads, D, L) bytes; 0 = not built for these levels).  No float atomics:
 * every tile stores its LDS window into its own slab of the workspace and a second kernel sums, per grad_value element,
 * the windows covering it in a fixed tile order; the rare points outside a window are added as integers into an int64
 * fixed-point image (unit 2^-44 of the largest |grad_out| of the image and head; overflow-free for S < 2^17).
 * grad_loc / grad_attn_w never had a scatter.  `grad_value` need not be cleared by the caller.
 * Built for the LDS-window backward only (head_dim 32, 4 points, Q == S, levels that fit its windows); otherwise
 * WM2F_EUNSUPPORTED. */
int64_t wm2f_msdeform_bwd_det_workspace(const int32_t* level_hw, int B, int S, int heads, int D, int L);
int wm2f_msdeform_bwd_det(const void* value, const void* loc, const void* attn_w, const void* grad_out,
                          void* grad_value, void* grad_loc, void* grad_attn_w, void* workspace,
                          const int32_t* level_hw, int B, int S, int Q, int heads, int D, int L, int P, int dtype,
                          void* stream);

/* K1 for TRAINING on the merged projection's rows (replaces, as one differentiable op of (value, rows), the prologue of
 * transformers modeling_mask2former.py:983-1002 -- offsets / (W, H) + reference points, softmax over the L * P logits -- the
 * core :798-837 and the autograd of both):
 *   value      (B, S, heads, 32)       fp32 (the arithmetic is fp32, as the dependency's grid_sample is under autocast)
 *   rows       (B, Q, heads * L*P*3)   [offsets (heads, L, P, 2) in pixels | logits (heads, L*P)] per token, as
 *                                      cat(sampling_offsets, attention_weights) writes them
 *   out        (B, Q, heads * 32)
 *   grad_out   as out;  grad_rows as rows (every element written);  grad_value as value (need not be cleared)
 * dtype = WM2F_F32: rows, out, grad_out, grad_rows are fp32; WM2F_BF16: all four are bf16 (what a bf16-autocast Linear writes
 * and reads; bf16 -> fp32 is exact, the outputs are rounded to nearest even once).  Reference points are the tokens' pixel
 * centres (:1127-1156 with valid ratios of 1).  Forward: the streaming kernel (3 levels 1 : 2 : 4 coarse first or a pyramid
 * it takes, P = 4, Q == S); backward: the LDS-window kernels; heads even.  Otherwise WM2F_EUNSUPPORTED (compose the op from
 * wm2f_msdeform_fwd / _bwd). */
int wm2f_msdeform_rows_fwd(const void* value, const void* rows, void* out, const int32_t* level_hw, int B, int S, int Q,
                           int heads, int D, int L, int P, int dtype, void* stream);
int wm2f_msdeform_rows_bwd(const void* value, const void* rows, const void* grad_out, void* grad_value, void* grad_rows,
                           const int32_t* level_hw, int B, int S, int Q, int heads, int D, int L, int P, int dtype,
                           void* stream);

/* K1 with the module prologue fused (HF:983-1002): softmax over the L*P logits and
 * loc = ref + offset / (W_l, H_l) are computed in-kernel.
 *   offsets (B, Q, heads, L, P, 2)  raw sampling_offsets output
 *   logits  (B, Q, heads, L*P)      raw attention_weights output (pre-softmax)
 *   ref     (Q, L, 2)               reference points, shared by the batch (valid ratios are 1)
 */
int wm2f_msdeform_fused_fwd(const void* value, const void* offsets, const void* logits, const void* ref,
                            void* out, const int32_t* level_hw, int B, int S, int Q, int heads, int D,
                            int L, int P, int dtype, void* stream);

/* Fused variant reading the two projections from ONE packed row per token, as a single merged
 * Linear writes them:  packed (B, Q, heads*L*P*3) = [offsets (heads,L,P,2) | logits (heads,L*P)].
 * LDS-window kernel only (D = 32, P = 4, Q == S, L <= 4); returns WM2F_EUNSUPPORTED otherwise. */
int wm2f_msdeform_fused_packed_fwd(const void* value, const void* packed, void* out,
                                   const int32_t* level_hw, int B, int S, int Q, int heads, int D, int L,
                                   int P, int dtype, int margin, void* stream);

/* The same for rows in the kernel's RECORD order -- a free choice of the row order of the merged Linear that writes them
 * (ops.k1_lane_order), made for the kernel's loads.  Per token and head 36 floats = 144 bytes, in 16-byte pieces; lane j of
 * a query's quad owns sampling-point slot j of every level:
 *   rec[ 4 j + {0,1,2,3}]      = offsets[.., h, level 0, j, {x,y}], offsets[.., h, level 1, j, {x,y}]
 *   rec[16 + 4 j + {0,1,2,3}]  = offsets[.., h, level 2, j, {x,y}], logits[.., h, 0*4 + j], logits[.., h, 1*4 + j]
 *   rec[32 + j]                = logits[.., h, 2*4 + j]
 * A lane fetches two aligned 16-byte pieces and one dword per query (3 loads inside one 144-byte record) instead of 6 loads
 * scattered over the token's 1152-byte row.  Streaming kernel only (D = 32, P = 4, L = 3, Q == S, levels coarse first with
 * sides 1:2:4); any other shape returns WM2F_EUNSUPPORTED (use the [offsets | logits] form).  `head_major` is a bit set:
 *   bit 0  lanes is (heads, B, Q, 36) instead of (B, Q, heads, 36): a head's records of consecutive tokens are contiguous
 *          (what wm2f_token_linear_fwd with out_group = 36 writes);
 *   bit 1  `value` is stored (heads, B, S, 32) instead of (B, S, heads, 32) (out_group = 32);
 *   bit 2  SLAB order: the tiles are walked heads-outermost, so that the workgroups of an XCD share ONE (image, head) slab
 *          of `value` (2.75 MB at config 2) in its 4 MiB L2 and the window halos (3.6 x the slab at L2 level) come from HBM
 *          once.  Meant for bit 0 = 1 (with token-major records every 1152-byte row would be fetched once per head).
 *          Measured in the model: HBM traffic 1.29 x -> 1.005 x the algorithmic bytes, 156 -> 136 us.
 * The result does not depend on any of the bits (tests: bit-identical). */
int wm2f_msdeform_fused_lanes_fwd(const void* value, const void* lanes, void* out, const int32_t* level_hw, int B, int S,
                                  int Q, int heads, int D, int L, int P, int dtype, int head_major, void* stream);

/* Same two operations with the kernel choice exposed, so that the two fall-back kernels can be held to the golden vectors
 * on shapes `auto` gives to the first:
 *   fused   0: a = loc, b = attn_w, ref unused      1: a = offsets, b = logits, ref as above
 *   variant 0: auto (tries 4, 2, 1 in that order)
 *           1: direct gather (any D)
 *           2: LDS-window kernel (D = 32, P = 4, Q == S, L <= 4)
 *           4: streaming quad kernel (3 levels coarse first whose sides about double, P = 4, D = 32, Q == S; persistent
 *              workgroups + loader waves), one workgroup per CU
 *   margin  window margin in pixels for the LDS-window kernel; sampling points farther than that
 *           from their reference point take a slow path (results never depend on it).
 * Any other variant returns WM2F_EUNSUPPORTED: timing ablations and stamped builds of these kernels live in the separate
 * profiling library (include/wm2f_prof.h), never in libwm2f.so; the superseded kernels and measured negatives that other
 * numbers once selected were removed and are recorded in DESIGN.md.  wm2f_msdeform_fwd / _fused_fwd are variant 0, margin 4. */
int wm2f_msdeform_fwd_v(const void* value, const void* a, const void* b, const void* ref, void* out,
                        const int32_t* level_hw, int B, int S, int Q, int heads, int D, int L, int P,
                        int dtype, int fused, int variant, int margin, void* stream);

/* ---- K3 in bf16 (BASELINE configs 3-5: bf16 autocast) ---------------------------------------------
 * Same line as wm2f_mask_einsum_fwd (HF:2046) with bf16 operands, fp32 accumulation on the bf16 matrix cores and
 * fp32 output; HBM-bound (478 MB per call at config 2).
 *   emb (B, Q, C) bf16, Q <= 112 per call;  pix_pixel_major (B, HW, C) bf16 -- the pixel features PIXEL-MAJOR (the
 *   MFMA operands want the contraction index contiguous), made once per forward by wm2f_nchw_to_pixel_major_bf16
 *   from the (B, C, HW) map;  out (B, Q, HW) fp32;  C % 32 == 0, C <= 512. */
int wm2f_mask_einsum_bf16_fwd(const void* emb, const void* pix_pixel_major, void* out, int B, int Q, int C,
                              int HW, void* stream);

/* K3 backward under bf16 autocast (replaces grad.to(bfloat16) + two batched library GEMMs): grad_out is fp32 (the
 * logits are), emb / pix and both gradients bf16 (round-to-nearest-even), accumulation fp32; g_emb summed in a fixed
 * order.  Either output may be NULL.  `pix` is the NCHW tensor (B, C, HW), not the pixel-major copy.
 * `workspace`: wm2f_mask_einsum_bf16_bwd_workspace(B, Q, C, HW) bytes.
 *   C % 64 == 0, Q % 4 == 0, Q <= 112, HW % 8 == 0; other shapes: WM2F_EUNSUPPORTED */
int64_t wm2f_mask_einsum_bf16_bwd_workspace(int B, int Q, int C, int HW);
int wm2f_mask_einsum_bf16_bwd(const void* emb, const void* pix, const void* grad_out, void* g_emb, void* g_pix,
                              void* workspace, int B, int Q, int C, int HW, void* stream);
int wm2f_nchw_to_pixel_major_bf16(const void* src, void* dst, int B, int C, int HW, void* stream);

/* ---- K3: mask einsum --------------------------------------------------------------------
 * Replaces torch.einsum("bqc,bchw->bqhw"), HF:2046.
 *   emb (B, Q, C)   pix (B, C, HW)   out (B, Q, HW)      C % 16 == 0
 */
int wm2f_mask_einsum_fwd(const void* emb, const void* pix, void* out, int B, int Q, int C, int HW,
                         int dtype, void* stream);

/* K3 with the attention-mask epilogue fused (the `out_attn_mask` of SURVEY section 8b): HF:2046 followed by
 * HF:2051-2053 (sigmoid, `< 0.5`) and the row flag of HF:1912-1914, for predictions that only feed the next layer's
 * mask -- the logits are never written.  There is no resize in it: `pix` is the mask-feature map ALREADY resized to
 * the level's resolution (wm2f_resize_bilinear once per forward; resize and einsum commute), so HW = Hn * Wn.
 *   emb (B, Q, C)   pix (B, C, HW)   mask (B, Q, HW) uint8, 1 = blocked   row_open (B, Q) int32 (cleared by the call)
 *   C % 16 == 0, HW % 4 == 0 */
int wm2f_mask_einsum_attn_mask_fwd(const void* emb, const void* pix, void* mask, void* row_open, int B, int Q, int C,
                                   int HW, int dtype, void* stream);

/* K3 backward (HF:2046 under autograd; replaces the two batched library GEMMs autograd derives from the einsum):
 *   g_pix[b][c][p] = sum_q emb[b][q][c] * grad_out[b][q][p]      g_emb[b][q][c] = sum_p grad_out[b][q][p] * pix[b][c][p]
 * Either output may be NULL (not wanted).  g_emb is summed in a fixed order (pixel ranges to a workspace, then in range
 * order): no atomics, run-to-run identical.  `workspace`: wm2f_mask_einsum_bwd_workspace(B, Q, C, HW) bytes.
 *   emb (B, Q, C)   pix (B, C, HW)   grad_out (B, Q, HW)   g_emb (B, Q, C)   g_pix (B, C, HW)   all fp32
 *   C % 64 == 0, Q % 4 == 0, HW % 4 == 0; other shapes: WM2F_EUNSUPPORTED */
int64_t wm2f_mask_einsum_bwd_workspace(int B, int Q, int C, int HW);
int wm2f_mask_einsum_bwd(const void* emb, const void* pix, const void* grad_out, void* g_emb, void* g_pix,
                         void* workspace, int B, int Q, int C, int HW, int dtype, void* stream);

/* ---- attention-mask build ----------------------------------------------------------------
 * Replaces HF:2048-2054 (bilinear resize, sigmoid, < 0.5) WITHOUT the x num_heads replication,
 * and the row fix-up of HF:1912-1914.
 *   logits   (B, Q, H, W) fp32
 *   mask     (B, Q, Hn*Wn) uint8, 1 = blocked
 *   row_open (B, Q) int32, 1 if at least one key of the row is open (0 => attend everywhere)
 */
int wm2f_attn_mask_build(const void* logits, void* mask, void* row_open, int B, int Q, int H, int W,
                         int Hn, int Wn, void* stream);

/* ---- K2: masked cross-attention ------------------------------------------------------------
 * Replaces the attention arithmetic of nn.MultiheadAttention as called at HF:1644-1650
 * (TORCHF:6578-6600): softmax(bias + (q/sqrt(D)) k^T) v, bias = -inf where mask == 1; rows with
 * row_open == 0 ignore the mask (HF:1912-1914).  Projections stay outside.
 *   q (B, Q, heads*D) ALREADY scaled by 1/sqrt(D);  k, v (B, N, heads*D)
 *   mask (B, Q, N) uint8 shared by all heads, or NULL;  row_open (B, Q) int32 or NULL
 *   out (B, Q, heads*D);  lse (B, heads, Q) fp32 log-sum-exp per row (for backward) or NULL
 *   workspace: device scratch of at least wm2f_masked_xattn_workspace(...) bytes
 * D in {16, 32, 64}.
 */
int64_t wm2f_masked_xattn_workspace(int B, int heads, int Q, int N, int D);
int wm2f_masked_xattn_fwd(const void* q, const void* k, const void* v, const void* mask,
                          const void* row_open, void* out, void* lse, void* workspace,
                          int B, int heads, int Q, int N, int D, int dtype, void* stream);

/* The same with bf16 operands, for the bf16-autocast configurations (BASELINE configs 2-4), where the dependency's two
 * attention products are bf16 matrix products around an fp32 softmax (TORCHF:6578-6600 under autocast): q, k, v bf16 as the
 * in_proj Linears emit them (no cast pass, half the K / V bytes), both products on the bf16 matrix cores with fp32
 * accumulation, softmax / (m, l) / O in fp32, P rounded to bf16 for the second product; out (B, Q, heads*D) and lse fp32.
 * Same mask / row_open / workspace (wm2f_masked_xattn_workspace) as the fp32 form.  Full-tile form only: D = 32,
 * N % 16 == 0, 16-byte aligned operands -- anything else returns WM2F_EUNSUPPORTED (cast to fp32, call the form above). */
int wm2f_masked_xattn_bf16_fwd(const void* q, const void* k, const void* v, const void* mask, const void* row_open,
                               void* out, void* lse, void* workspace, int B, int heads, int Q, int N, int D, void* stream);

/* Backward of the above (P is recomputed from q, k and lse).  grad_q is the gradient w.r.t. the
 * PRE-SCALED q; grad_q / grad_k / grad_v are overwritten.
 *   out, lse: the forward's results; grad_out (B, Q, heads*D)
 *   workspace: at least wm2f_masked_xattn_bwd_workspace(...) bytes */
int64_t wm2f_masked_xattn_bwd_workspace(int B, int heads, int Q, int N, int D);
int wm2f_masked_xattn_bwd(const void* q, const void* k, const void* v, const void* mask,
                          const void* row_open, const void* out, const void* lse, const void* grad_out,
                          void* grad_q, void* grad_k, void* grad_v, void* workspace,
                          int B, int heads, int Q, int N, int D, int dtype, void* stream);

/* Backward of wm2f_masked_xattn_bf16_fwd: q, k, v bf16 as saved by the forward, out / lse / grad_out fp32; grad_q fp32,
 * grad_k / grad_v bf16 (the operands' dtype).  The five products per (key tile, query tile) on the bf16 matrix cores, p and dS
 * in fp32 from fp32 accumulators.  Workspace: wm2f_masked_xattn_bwd_workspace.  D = 32, N % 16 == 0, Q <= 112 (one query
 * chunk), 16-byte aligned operands; anything else returns WM2F_EUNSUPPORTED (cast to fp32, wm2f_masked_xattn_bwd). */
int wm2f_masked_xattn_bf16_bwd(const void* q, const void* k, const void* v, const void* mask, const void* row_open,
                               const void* out, const void* lse, const void* grad_out, void* grad_q, void* grad_k,
                               void* grad_v, void* workspace, int B, int heads, int Q, int N, int D, void* stream);

/* The kernel a K2 call runs (host arithmetic only, no GPU needed): the four entry points above decide with this function, so
 * what it reports is what they launch.  dtype WM2F_F32 / WM2F_BF16 selects the fp32 or the bf16 entry points, backward != 0
 * the backward.  mask_aligned != 0: the pointer conditions of the call hold -- fp32 forward: the mask's address is a
 * multiple of 4 (or it is NULL); bf16: also 16-byte aligned operands; the fp32 backward ignores it.  Fills
 *   route[0] kernel (WM2F_K2_*)            route[1] NQT, the kernel's template query tiles per workgroup
 *   route[2] q_chunks                      route[3] n_splits (key splits)
 *   route[4] tiles_per_split (16-key tiles; the last splits may own fewer, or none)
 *   route[5] accumulate (1: the query chunks add grad_k / grad_v atomically)
 * and returns WM2F_OK; a shape, head size or dtype no kernel is built for gives route[0] = WM2F_K2_UNSUPPORTED and zeros.
 * The entry points' own argument checks (null pointers, heads or B above the grid limit of 65535) are not part of the
 * route: a call they refuse never gets here.  NULL route: WM2F_EINVAL. */
#define WM2F_K2_UNSUPPORTED 0
#define WM2F_K2_FWD_GENERAL 1
#define WM2F_K2_FWD_FULL 2
#define WM2F_K2_BF16_FWD 3
#define WM2F_K2_BWD_GENERAL 4
#define WM2F_K2_BWD_FULL 5
#define WM2F_K2_BF16_BWD 6
int wm2f_masked_xattn_route(int B, int heads, int Q, int N, int D, int dtype, int backward, int mask_aligned, int* route);

/* ---- Swin backbone: shifted-window attention, inference forward ---------------------------------
 * One launch per Swin layer for pad + roll + window partition + q k^T * D^-1/2 + relative-position bias + shift mask +
 * softmax + p v + window reverse + roll back + crop (transformers modeling_swin.py:401-468, :486-505, :553-626).
 *   q, k, v    (B, H*W, heads*D) in IMAGE order, as the three Linears write them
 *   k_pad, v_pad (heads*D): key / value row of a padding token (a zero row through the Linear = its bias); NULL = zeros
 *   bias_table ((2 ws - 1)^2, heads) fp32: the relative-position-bias PARAMETER itself, indexed in the kernel
 *   out        (B, H*W, heads*D) in image order, dtype of q
 * Contract: Hp = ceil(H / ws) ws, Wp likewise; padding tokens sit at the bottom / right of the (Hp, Wp) frame, are NOT masked
 * (they are keys of every real query of their window) and get no output.  Window (wy, wx), slot (i, j) holds the token at
 * padded-frame position ((wy ws + i + shift) mod Hp, (wx ws + j + shift) mod Wp).  With shift > 0 a slot's region id is
 * 3 ((r >= Hp - ws) + (r >= Hp - shift)) + ((c >= Wp - ws) + (c >= Wp - shift)) of its rolled-frame coordinates
 * r = wy ws + i, c = wx ws + j, and a score gets -100 (finite) where query and key ids differ.  Softmax in fp32 over the ws^2
 * keys of the window.  0 <= shift < ws; the window is never reduced for small maps.
 * dtype WM2F_F32: fp32 operands, exact-fp32 products.  WM2F_BF16: bf16 operands as a bf16-autocast Linear writes them, bf16
 * matrix cores with fp32 accumulation, scores and softmax in fp32, P rounded to bf16 once, bf16 out.
 * ws in {4, 7, 12}, D in {16, 32}, 16-byte aligned operands; anything else returns WM2F_EUNSUPPORTED. */
int wm2f_swin_window_attn_fwd(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad,
                              const void* bias_table, void* out, int B, int H, int W, int heads, int D, int ws, int shift,
                              int dtype, void* stream);

/* ---- Swin backbone: shifted-window attention, training forward and backward -----------------------
 * wm2f_swin_window_attn_train_fwd is wm2f_swin_window_attn_fwd (same kernel template, same contract and numbers) that also
 * writes lse (B, heads, H*W) fp32: the log-sum-exp of every real query's score row, which the backward needs.
 *
 * wm2f_swin_window_attn_bwd: the gradients of that forward under the contract paragraph above.
 *   q, k, v, k_pad, v_pad, bias_table: the forward's inputs;  lse: the training forward's;  grad_out (B, H*W, heads*D) in
 *   image order, dtype of q
 *   grad_q, grad_k, grad_v (B, H*W, heads*D), image order, dtype of q: overwritten, every row (each real token is a query and a
 *     key of exactly one window, so the three are complete inside one workgroup: plain vector stores)
 *   grad_k_pad, grad_v_pad (heads*D) fp32 or NULL: dK / dV summed over every padding slot of every window and image -- the
 *     share of the k / v Linear's bias gradient that comes from padding rows
 *   grad_bias_table ((2 ws - 1)^2, heads) fp32 or NULL: per head and relative offset, dS summed over every (query, key) pair of
 *     that offset, window and image; masked pairs and padding keys included, padding queries contribute nothing
 * S is recomputed as the forward computes it, P = exp(S - lse), dP = dO V^T, delta = rowsum(P dP), dS = P (dP - delta),
 * dV = P^T dO, dK = dS^T Q D^-1/2, dQ = dS K D^-1/2.  WM2F_F32: exact-fp32 products.  WM2F_BF16: bf16 matrix cores, fp32
 * S / P / dS / accumulation, P and dS rounded to bf16 once as MFMA operands, bf16 grad_q / k / v.
 * The two cross-workgroup sums (table, padding rows) go through `workspace` -- one partial per (image, window, head) written by
 * its workgroup, added in a fixed order by a second kernel: no float atomics to global memory, bit-identical run to run.
 * workspace: wm2f_swin_window_attn_bwd_workspace(...) bytes = 4 B nW heads ((2 ws - 1)^2 + 2 D), 16-byte aligned; the largest
 * case, Swin-L stage 1 at 1024 x 1024 with B = 8 (484 windows, 6 heads, ws 12): 55.1 MB.  May be NULL when all three optional
 * outputs are NULL.  ws in {4, 7, 12}, D in {16, 32}, 16-byte aligned operands; anything else returns WM2F_EUNSUPPORTED (the
 * workspace query returns 0). */
int wm2f_swin_window_attn_train_fwd(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad,
                                    const void* bias_table, void* out, void* lse, int B, int H, int W, int heads, int D, int ws,
                                    int shift, int dtype, void* stream);
int64_t wm2f_swin_window_attn_bwd_workspace(int B, int H, int W, int heads, int D, int ws);
int wm2f_swin_window_attn_bwd(const void* q, const void* k, const void* v, const void* k_pad, const void* v_pad,
                              const void* bias_table, const void* lse, const void* grad_out, void* grad_q, void* grad_k,
                              void* grad_v, void* grad_k_pad, void* grad_v_pad, void* grad_bias_table, void* workspace, int B,
                              int H, int W, int heads, int D, int ws, int shift, int dtype, void* stream);

/* ---- K4: Hungarian-matcher cost matrices ------------------------------------------------------
 * Replaces Mask2FormerHungarianMatcher.forward up to (not including) the scipy solver,
 * HF:444-472 with sample_point HF:245-274 and the pair-wise losses HF:328-374, batched over
 * NL prediction levels and B images so that ONE device->host copy feeds every solver call.
 *   mask_logits  (NL, B, Q, h, w) fp32, NL <= 16   class_logits (NL, B, Q, C1) fp32
 *   tgt_masks    concatenation over images of (T_i, Ht, Wt); tgt_dtype 0 = fp32, 1 = uint8
 *   tgt_offset   host int32 [B+1]: image i owns targets [tgt_offset[i], tgt_offset[i+1])
 *   tgt_classes  int64 [sum T_i]
 *   points       (NL, B, P, 2) fp32 in [0,1] as (x, y)
 *   cost         (NL, B, Q, Tmax) fp32; columns >= T_i are left untouched
 *   workspace    scratch, at least wm2f_matcher_workspace(...) bytes (sampled targets, the grouped points, band offsets)
 * cost = w_mask*BCE_pair + w_class*(-softmax(class)[:, tgt]) + w_dice*dice_pair, clamped to
 * +-1e10 with NaN -> 0.
 * The points may come in any order (the cost is a sum over them): with P >= 1024 and maps up to ~2000 wide the call groups
 * each (level, image)'s points by band of map rows (stable, so results are reproducible) and samples the predictions from LDS
 * bands instead of gathering from memory.
 */
int64_t wm2f_matcher_workspace(int NL, int B, int Q, int P, int Tsum);
int wm2f_matcher_cost(const void* mask_logits, const void* class_logits, const void* tgt_masks,
                      int tgt_dtype, const int32_t* tgt_offset, const void* tgt_classes,
                      const void* points, void* cost, void* workspace, int NL, int B, int Q, int C1,
                      int h, int w, int Ht, int Wt, int P, int Tmax, float w_class, float w_mask,
                      float w_dice, void* stream);
/* The same with the levels NOT stacked: mask_levels = HOST array of NL (<= 16) DEVICE pointers, each (B, Q, h, w) fp32
 * (the mask predictor's outputs where they are; a stacked copy is 10 x 210 MB at config 2). */
int wm2f_matcher_cost_levels(const void* const* mask_levels, const void* class_logits, const void* tgt_masks,
                             int tgt_dtype, const int32_t* tgt_offset, const void* tgt_classes,
                             const void* points, void* cost, void* workspace, int NL, int B, int Q, int C1, int h,
                             int w, int Ht, int Wt, int P, int Tmax, float w_class, float w_mask, float w_dice,
                             void* stream);

/* ---- linear sum assignment on the device (HF:474: scipy.optimize.linear_sum_assignment on a host copy of each cost matrix) ----
 *   cost    (problems, Q, Tmax) fp32 -- wm2f_matcher_cost's output, problems = levels x B, image = problem % B
 *   counts  (B) int32, DEVICE: targets of each image (its valid columns)
 *   rows / cols (problems, Tcap) int32: the min(Q, T) matched (query, target) pairs of each problem, sorted by query -- exactly
 *           what scipy returns for cost[:, :T] (entries beyond min(Q, T) are not written; Tcap >= max over images of min(Q, T_b)).
 * scipy's own shortest-augmenting-path algorithm with its arithmetic (float64), scan order, tie rule and output order, one wave
 * per problem: bit-identical indices, ties included (tests).  Sides up to 1024; larger returns WM2F_EUNSUPPORTED. */
int wm2f_lsa_batched(const void* cost, const void* counts, void* rows, void* cols, int problems, int B, int Q, int Tmax, int Tcap,
                     void* stream);

/* ---- point sampling (shared by the loss, HF:245-274) ----------------------------------------
 *   feat (N, H, W) fp32 or uint8 (feat_dtype 0 / 1); pts (M, P, 2); out (M, P) fp32.
 *   map_index: int32 [M] -- row m samples feat[map_index[m]] (matched prediction / target maps are
 *   sampled in place instead of being gathered into a copy); NULL means M == N, identity.
 * Backward (fp32 feat only): grad_feat (N,H,W) must be zeroed by the caller (float atomics). */
int wm2f_point_sample_fwd(const void* feat, int feat_dtype, const void* pts, const void* map_index,
                          void* out, int M, int H, int W, int P, void* stream);
int wm2f_point_sample_bwd(const void* grad_out, const void* pts, const void* map_index, void* grad_feat,
                          int M, int H, int W, int P, void* stream);

/* ---- fused HBM-bound passes around the stock GEMMs / convolutions (inference) -------------------
 * wm2f_bias_act:      y = act(x + bias[c] (+ residual)), x / y / residual (N, C, H*W) fp32, H*W % 4 == 0;
 *                     y may alias x.  relu = 1 applies max(., 0).
 * wm2f_add_layernorm: out = LayerNorm(x + residual) * gamma + beta over rows of C = 256 (HF:1076-1078,
 *                     :1086-1088); residual may be NULL; if out_plus_pos != NULL it receives
 *                     out + pos[row % pos_rows] (the next layer's `hidden + pos`, HF:972). */
/* out[b][i] = a[b][i] + p[i], b < B, i < n (fp32, n % 4 == 0, 16-byte aligned): a level's positional embedding added to its tokens
 * for every image of the batch -- the keys of the masked cross-attention, `with_pos_embed` at HF:1644-1650 (inference). */
int wm2f_add_broadcast(const void* a, const void* p, void* out, int B, int64_t n, void* stream);
int wm2f_bias_act(const void* x, const void* bias, const void* residual, void* y, int N, int C, int HW,
                  int relu, void* stream);
int wm2f_add_layernorm(const void* x, const void* residual, const void* gamma, const void* beta,
                       const void* pos, void* out, void* out_plus_pos, int64_t rows, int C,
                       int64_t pos_rows, float eps, void* stream);
/* wm2f_add_layernorm_train_fwd / _bwd: the same residual add + LayerNorm for the TRAIN step (HF:1076-1078, :1086-1088, and the
 *                     next layer's `hidden + pos`, HF:972), C = 256, with the tensors its consumers read written in the same pass:
 *                       y (rows, 256) fp32 = LayerNorm(x + residual) * gamma + beta;   x fp32 or bf16 (x_dtype), residual fp32 or NULL
 *                       y_bf16      NULL, or y rounded to bf16 (the next Linear's operand under bf16 autocast)
 *                       y_plus_pos  NULL, or y + pos[row % pos_rows] in yp_dtype (fp32 / bf16)
 *                       stats (rows, 2) fp32 = (mean, rstd) for the backward;
 *                       clamp > 0: y is limited to [-clamp, clamp], NaN left as it is -- the overflow guard of HF:1090-1093
 *                       (clamp to finfo.max - 1000 when a value is not finite) without the host synchronisation its `if` costs:
 *                       on finite values the clamp is the identity, so applying it always is the same function.
 *                     Backward: the gradients of the three outputs (any of them NULL) are summed in registers;
 *                       grad_sum (rows, 256) fp32 = d loss / d (x + residual) (NULL: not written), grad_x the same in x's dtype
 *                       (NULL: not written), grad_gamma / grad_beta (256) fp32 -- per-workgroup partial sums over fixed row
 *                       ranges in `workspace` (wm2f_add_layernorm_train_workspace(rows) bytes), added in workgroup order:
 *                       deterministic.  Replaces torch's two LayerNorm-backward kernels, the gradient-accumulation adds and the
 *                       casts around them; every operand byte moves once (HBM-bound). */
int64_t wm2f_add_layernorm_train_workspace(int64_t rows);
int wm2f_add_layernorm_train_fwd(const void* x, int x_dtype, const void* residual, const void* gamma, const void* beta,
                                 const void* pos, void* y, void* y_bf16, void* y_plus_pos, int yp_dtype, void* stats,
                                 int64_t rows, int C, int64_t pos_rows, float eps, float clamp, void* stream);
int wm2f_add_layernorm_train_bwd(const void* x, int x_dtype, const void* residual, const void* gamma, const void* stats,
                                 const void* grad_y, const void* grad_y_bf16, const void* grad_y_plus_pos, int gyp_dtype,
                                 void* grad_sum, void* grad_x, void* grad_gamma, void* grad_beta, void* workspace,
                                 int64_t rows, int C, void* stream);
/* wm2f_token_linear_fwd: out (M, N) = epilogue(x (M, K) . W (N, K)^T + bias[N]) on the fp32 matrix cores, for the narrow Linears
 *                        of the pixel decoder's encoder layers (HF:978 value_proj, :983-991 sampling_offsets | attention_weights
 *                        merged, :1012 output_proj, :1086 fc2).  N = 256 or 288, K % 64 == 0, all fp32 row-major (W as
 *                        nn.Linear stores it).  Epilogue, in this order:  relu != 0: max(., 0);  ln_gamma / ln_beta != NULL:
 *                        LayerNorm over the N features of (value + residual[M, N]) (residual may be NULL) -- HF:1076-1078,
 *                        :1086-1088;  out_plus_pos != NULL: additionally out + pos[row % pos_rows] (the next layer's
 *                        `hidden + pos`, HF:972).  x / out below 2 GiB each.
 *                        out_group = G > 0 (G % 4 == 0, N % G == 0, no LayerNorm): out is written (N / G, M, G), feature-group
 *                        major, instead of (M, N): with G = 36 the merged projection writes K1's operand rows head-major
 *                        (wm2f_msdeform_fused_lanes_fwd, head_major = 1). */
int wm2f_token_linear_fwd(const void* x, const void* w, const void* bias, const void* residual, const void* ln_gamma,
                          const void* ln_beta, const void* pos, void* out, void* out_plus_pos, int64_t M, int K, int N, int relu,
                          int64_t pos_rows, float eps, int out_group, void* stream);

/* wm2f_token_linear_split_weight: W (N, K) fp32 row-major -> w_split, N * K * 6 bytes: the three bf16 pieces of every weight
 *                        (w = h + m + l, each piece the RNE bf16 of what the previous ones leave) in the fragment order
 *                        wm2f_token_linear_split_fwd reads.  N % 16 == 0, K % 32 == 0.  Run once per weight version.
 * wm2f_token_linear_split_fwd: what wm2f_token_linear_fwd computes, with the same epilogues and arguments, at fp32 accuracy on
 *                        the bf16 matrix cores: x split into three bf16 pieces in registers, six of the nine piece products
 *                        accumulated in fp32.  N = 256, 288, 512, 768 or 1024 (the LayerNorm epilogue: N <= 288),
 *                        K % 32 == 0.  Deterministic; a token's output does not depend on M or on the other tokens.
 *                        Non-finite inputs give non-finite outputs in the same positions (NaN where fp32 may give inf). */
int wm2f_token_linear_split_weight(const void* w, void* w_split, int N, int K, void* stream);
int wm2f_token_linear_split_fwd(const void* x, const void* w_split, const void* bias, const void* residual, const void* ln_gamma,
                                const void* ln_beta, const void* pos, void* out, void* out_plus_pos, int64_t M, int K, int N,
                                int relu, int64_t pos_rows, float eps, int out_group, void* stream);

/* wm2f_token_ffn_split_fwd: the feed-forward pair of a pixel-decoder encoder layer (HF:1080-1088) in one kernel, at the
 *                        accuracy and with the arithmetic of wm2f_token_linear_split_fwd:
 *                        out (M, N) = LayerNorm(relu(x (M, K) . W1 (F, K)^T + b1[F]) . W2 (N, F)^T + b2[N] + residual (M, N))
 *                        with ln_gamma / ln_beta / eps, and, with pos (pos_rows, N) and out_plus_pos, also
 *                        out_plus_pos = out + pos[row % pos_rows] as one fp32 add.  The (M, F) intermediate is never written.
 *                        out and out_plus_pos are, bit for bit, what wm2f_token_linear_split_fwd (relu = 1) followed by
 *                        wm2f_token_linear_split_fwd (residual, LayerNorm, pos) store.
 *                        w1_split = wm2f_token_linear_split_weight_rows(W1, F, K, WM2F_ROWS_FFN);
 *                        w2_split = wm2f_token_linear_split_weight(W2, N, F), the plain split.
 *                        K = N = 256; F = 256, 512, 768 or 1024; residual, ln_gamma and ln_beta are required; pos and
 *                        out_plus_pos are optional and come together, with any pos_rows >= 1; M * 256 * 4 < 2 GiB.  Anything
 *                        else returns WM2F_EINVAL with nothing launched and the outputs untouched.  Deterministic, no atomics;
 *                        a token's output does not depend on M, on the other tokens or on how rows are cut into calls.
 *                        Non-finite inputs: a token of x that holds an inf or a NaN makes that token's rows of both outputs
 *                        non-finite and touches no other token.  (Here the two launches differ: their ReLU is a
 *                        v_max_f32, which answers 0 for a NaN; this kernel puts the NaN back behind the max.)
 * wm2f_token_linear_split_weight_rows: wm2f_token_linear_split_weight with the rows of W (N, K) in another order.  row_order =
 *                        WM2F_ROWS_NATURAL: the same bytes.  WM2F_ROWS_FFN (N % 32 == 0): row position n of the split holds row
 *                        wm2f_token_ffn_row(n) of W -- inside every block of 32 rows, position 16 h + 4 g + e (h < 2, g < 4,
 *                        e < 4) holds row 8 g + 4 h + e, so that the fp32 C tiles of two neighbouring row tiles are, register
 *                        for register, the B fragment of the next product's 32-deep k-step in natural k order.
 * wm2f_token_ffn_row:    that map on the host (-1 for n < 0). */
#define WM2F_ROWS_NATURAL 0
#define WM2F_ROWS_FFN 1
int wm2f_token_linear_split_weight_rows(const void* w, void* w_split, int N, int K, int row_order, void* stream);
int wm2f_token_ffn_row(int n);
int wm2f_token_ffn_split_fwd(const void* x, const void* w1_split, const void* b1, const void* w2_split, const void* b2,
                             const void* residual, const void* ln_gamma, const void* ln_beta, const void* pos, void* out,
                             void* out_plus_pos, int64_t M, int K, int F, int N, int64_t pos_rows, float eps, void* stream);
/* (wm2f_token_ffn_split_fwd_p, with a trailing `pieces`, is declared with the other *_p entry points below: at every
 * level it gives the bits of the two wm2f_token_linear_split_fwd_p launches at that level.) */

/* wm2f_conv1x1_split_fwd: 1x1 convolution without padding, NCHW fp32, at fp32 accuracy on the bf16 matrix cores (the split
 *                        arithmetic of wm2f_token_linear_split_fwd):  out (B, N, Ho, Wo) = epilogue(W (N, K) .
 *                        x (B, K, Hi, Wi) sampled at (stride ho, stride wo)), Ho = (Hi - 1) / stride + 1, likewise Wo.  w_split =
 *                        wm2f_token_linear_split_weight of W (N, K).  Epilogue, fixed by the arguments: bias == NULL: none;
 *                        + bias[N]; relu != 0: max(., 0) after it; residual (B, N, Ho, Wo) != NULL: + residual before the ReLU
 *                        (needs bias and relu).  K % 32 == 0, N % 64 == 0, stride 1 or 2, one image of x / out below 2 GiB.
 *                        Deterministic; an image's output does not depend on B or on the other images.  config = -1: the
 *                        kernel's choice of tile configuration; >= 0: that entry of its table (the same bits, another speed).
 * wm2f_conv1x1_split_config: the tile configuration wm2f_conv1x1_split_fwd picks for (N, P = Ho * Wo, B) on n_cu CUs: an index
 *                        into the kernel's table, -1 if none fits (for tests and profiles). */
int wm2f_conv1x1_split_fwd(const void* x, const void* w_split, const void* bias, const void* residual, void* out, int B, int K,
                           int N, int Hi, int Wi, int stride, int relu, int config, void* stream);
int wm2f_conv1x1_split_config(int N, int P, int B, int n_cu);

/* wm2f_conv3x3_split_fwd: 3x3 convolution with padding 1, NCHW fp32, at fp32 accuracy on the bf16 matrix cores (the split
 *                        arithmetic of wm2f_conv1x1_split_fwd):  out (B, N, Ho, Wo) = epilogue(conv3x3(x (B, Cin,
 *                        Hi, Wi), W (N, Cin, 3, 3)), stride 1 or 2), Ho = (Hi - 1) / stride + 1, likewise Wo.  w_split =
 *                        wm2f_token_linear_split_weight of the tap-major weight W.permute(0, 2, 3, 1) seen as (N, 9 Cin).
 *                        Epilogue: bias == NULL: none; + bias[N]; relu != 0: max(., 0) after it (needs bias).  Cin % 32 == 0,
 *                        N % 64 == 0, one image of x / out below 2 GiB.  Deterministic, no split-K: an image's output does not
 *                        depend on B, on the other images or on config.  config = -1: the kernel's choice of tile
 *                        configuration; >= 0: that entry of its table (the same bits, another speed).
 * wm2f_conv3x3_split_config: the tile configuration wm2f_conv3x3_split_fwd picks for (N, P = Ho * Wo, B) on n_cu CUs: an index
 *                        into the kernel's table, -1 if none fits (for tests and profiles). */
int wm2f_conv3x3_split_fwd(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N, int Hi,
                           int Wi, int stride, int relu, int config, void* stream);
int wm2f_conv3x3_split_config(int N, int P, int B, int n_cu);

/* GroupNorm folded into the convolutions around it (inference).  `out` of each is bit for bit what the entry
 * point above stores, under every config; only the statistics carry the ordering freedom of their fp64 atomics.
 * wm2f_conv1x1_split_gn_fwd: wm2f_conv1x1_split_fwd (epilogue none or + bias) with one of
 *     stats_out != NULL: stats_out[(b * G_out + g) * 2 + {0, 1}] = (sum, sum of squares) of out over group g of image b --
 *                        the workspace of wm2f_group_norm_act / wm2f_group_norm_tokens, zeroed here on the stream and
 *                        filled from the epilogue.  N / G_out in {4, 8, 16}; any other group size is refused before
 *                        anything is launched (the caller keeps the separate statistics pass).
 *     norm_stats != NULL: x is read as act(GroupNorm_{norm_G}(x) * norm_gamma + norm_beta) from the FILLED workspace
 *                        norm_stats of x, act = max(., 0) if norm_relu -- the bits wm2f_group_norm_act_apply would have
 *                        written.  Needs bias, stride 1, K <= 2048.  The two together are not built.
 * wm2f_conv3x3_split_stats_fwd: wm2f_conv3x3_split_fwd without bias, plus stats_out as above.
 * wm2f_group_norm_act_apply, wm2f_group_norm_tokens_apply: wm2f_group_norm_act / wm2f_group_norm_tokens from a filled
 *                        workspace `stats` (of x, resp. of x + bias): no statistics pass.  wm2f_group_norm_act_apply
 *                        without `up` takes any W (W % 4 != 0: one element per thread, the same bits per element). */
int wm2f_conv1x1_split_gn_fwd(const void* x, const void* w_split, const void* bias, void* out, void* stats_out, int G_out,
                              const void* norm_stats, const void* norm_gamma, const void* norm_beta, int norm_G, float norm_eps,
                              int norm_relu, int B, int K, int N, int Hi, int Wi, int stride, int config, void* stream);
int wm2f_conv3x3_split_stats_fwd(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B, int Cin,
                                 int N, int Hi, int Wi, int stride, int config, void* stream);
int wm2f_group_norm_act_apply(const void* x, const void* gamma, const void* beta, const void* up, void* y, const void* stats,
                              int B, int C, int G, int H, int W, int Hs, int Ws, float eps, int relu, void* stream);
int wm2f_group_norm_tokens_apply(const void* x, const void* bias, const void* gamma, const void* beta, void* tokens,
                                 const void* stats, int B, int C, int G, int HW, int S, int start, float eps, void* stream);

/* wm2f_stem7x7_pool_fwd: the ResNet stem in one kernel, NCHW fp32, at fp32 accuracy on the bf16 matrix cores (the split
 *                        arithmetic of wm2f_conv1x1_split_fwd):  out (B, N, Hp, Wp) = MaxPool2d(3, stride 2,
 *                        pad 1)(ReLU(conv7x7(x (B, Cin, Hi, Wi), W (N, Cin, 7, 7), stride 2, pad 3) + bias[N])),
 *                        Hc = (Hi - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1, likewise W -- transformers' ResNetEmbeddings with
 *                        BatchNorm folded into W and bias by the caller.  The raw convolution never reaches memory.
 *                        w_split = wm2f_token_linear_split_weight of the (N, 160) matrix whose column 8 G + i, i < 7, is tap
 *                        (c, ky, kx) = (G / 7, G % 7, i) for G < min(7 Cin, 20), whose column 8 G + 7, G < 7, is tap
 *                        (2, 6, G) when Cin = 3, and which is zero elsewhere (ops.stem_weight_matrix).  Any Hi, Wi >= 1;
 *                        Cin in {1, 2, 3} (49 Cin <= 160), N = 64, one image of x / out below 2 GiB; anything else is
 *                        refused before any launch.  Conv pixels outside the conv map take no part in a pool window,
 *                        input pixels outside the image are zero.  An output is non-finite exactly where its pool o conv
 *                        receptive field holds a non-finite input.  Deterministic, no split-K, no atomics: an output does
 *                        not depend on B, on the other images or on grid.  grid <= 0: one workgroup per CU, capped by the
 *                        work; > 0: that many workgroups (the same bits, another speed). */
int wm2f_stem7x7_pool_fwd(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N, int Hi,
                          int Wi, int grid, void* stream);

/* Selectable precision of the split-bf16 GEMMs and convolutions (inference).  Every forward entry point above
 * has a variant that takes a trailing `int pieces` before `stream`; the entry point without it means pieces = 3.  With the
 * operands written as three bf16 pieces a = h + m + l (h = bf16 of a clamped to the largest finite bf16, m = bf16(a - h),
 * l = bf16(a - h - m)), W pieces first, a 32-deep k-step sums
 *     pieces = 3  "highest"  all six products  m.m, l.h, h.l, m.h, h.m, h.h          e <= 2 e32 + 2^-23   (§13)
 *     pieces = 2  "high"     three products    m.h, h.m, h.h  (in this order, the one they have in the six-product chain)
 *                                                                                  e <= 2 e32 + 2^-14
 *     pieces = 1  "medium"   one product       h.h                                  e <= 2 e32 + 2^-6
 * where e = max |out - ref64| / (sum_k |x_k w_k| + |bias| + |residual|) and e32 is the same measure of an fp32 computation.
 * The floors: at two pieces the dropped h.l, l.h and m.m are each at most 2^-16 (1 + 2^-7) sum |x_k w_k| (|m| <= 2^-8 |a|,
 * |a - h - m| <= 2^-16 |a|), three of them stay below 2^-14; at one piece |a - h| <= 2^-8 |a| (with the clamp) on both
 * operands gives 2^-7 + 2^-16 < 2^-6.  Operands that are exact in bf16 (small integers, bf16 data) give the same bits at
 * every level.  pieces = 1 computes, bit for bit, what pieces = 3 computes on the operands rounded to their h piece.
 * Everything else is per level what it is at pieces = 3: the accumulation structure of each kernel (the convolutions and the
 * stem sum a k-step from zero and add it to the accumulator once, the token kernel chains into the accumulator), the
 * epilogues, the tile tables and the host's choice among them, the refusals, the determinism (no split-K, no output atomics:
 * one MFMA sequence per output under every tile configuration, batch and sub-batch) and the non-finite rule: an inf or a NaN
 * in x makes every output it touches non-finite (at pieces = 1, where no residual piece carries it on, the h piece itself is
 * made NaN for a non-finite x; finite values as large as FLT_MAX stay finite, clamped).
 * w_split is ALWAYS the three-piece split of wm2f_token_linear_split_weight, N * K * 6 bytes: its first `pieces` pieces per
 * row tile are the `pieces`-piece split, and a kernel loads and stages only those (x is split into `pieces` pieces only).
 * A `pieces` value outside {1, 2, 3} returns WM2F_EINVAL with nothing launched and the outputs untouched. */
int wm2f_token_linear_split_fwd_p(const void* x, const void* w_split, const void* bias, const void* residual,
                                  const void* ln_gamma, const void* ln_beta, const void* pos, void* out, void* out_plus_pos,
                                  int64_t M, int K, int N, int relu, int64_t pos_rows, float eps, int out_group, int pieces,
                                  void* stream);
int wm2f_token_ffn_split_fwd_p(const void* x, const void* w1_split, const void* b1, const void* w2_split, const void* b2,
                               const void* residual, const void* ln_gamma, const void* ln_beta, const void* pos, void* out,
                               void* out_plus_pos, int64_t M, int K, int F, int N, int64_t pos_rows, float eps, int pieces,
                               void* stream);
int wm2f_conv1x1_split_fwd_p(const void* x, const void* w_split, const void* bias, const void* residual, void* out, int B, int K,
                             int N, int Hi, int Wi, int stride, int relu, int config, int pieces, void* stream);
int wm2f_conv1x1_split_gn_fwd_p(const void* x, const void* w_split, const void* bias, void* out, void* stats_out, int G_out,
                                const void* norm_stats, const void* norm_gamma, const void* norm_beta, int norm_G, float norm_eps,
                                int norm_relu, int B, int K, int N, int Hi, int Wi, int stride, int config, int pieces,
                                void* stream);
/* wm2f_conv1x1_split_dual_fwd_p: two 1x1 convolutions onto one output map as ONE GEMM over the concatenated K (a ResNet
 *                        bottleneck's conv3 plus its projection shortcut), NCHW fp32, the split arithmetic of
 *                        wm2f_conv1x1_split_fwd_p at `pieces`:
 *                            out (B, N, Ho, Wo) = max(W1 (N, K1) . x1 (B, K1, Ho, Wo)
 *                                                     + W2 (N, K2) . x2 (B, K2, H2, W2) sampled at (stride2 ho, stride2 wo)
 *                                                     + bias[N], 0).
 *                        ws1, ws2 = wm2f_token_linear_split_weight of W1 and of W2, two separate buffers: that split is
 *                        k-step major, so ws1 followed by ws2 is byte for byte the split of [W1 | W2], and the kernel reads
 *                        the two through two pointers.  The k-steps of source 1 come first, in order, then those of source 2;
 *                        each k-step is summed from zero and added to the accumulator with one fp32 add.  An output therefore
 *                        sees one MFMA sequence under every config, B and sub-batch (deterministic, no split-K, no atomics),
 *                        and a source whose weight is all zero adds nothing: the result is then bit for bit
 *                        wm2f_conv1x1_split_fwd_p of the other source with bias and ReLU.  Pixels of x2 that stride2 skips are
 *                        never read.  An inf or a NaN in a sampled pixel of either source makes that pixel's N outputs
 *                        non-finite and no other.
 *                        Refused with WM2F_EINVAL before any launch, out untouched: a null pointer (bias included);
 *                        K1 % 32, K2 % 32 or N % 64 non-zero; stride2 outside {1, 2}; (H2 - 1) / stride2 + 1 != Ho or the same
 *                        for W; one image of x1, x2 or out, or either split, at or above 2 GiB; a config >= 0 whose tile does
 *                        not divide N (or outside the table); pieces outside {1, 2, 3}.  config = -1: the tile pick of
 *                        wm2f_conv1x1_split_config(N, Ho * Wo, B, CUs), which does not depend on K. */
int wm2f_conv1x1_split_dual_fwd_p(const void* x1, const void* ws1, const void* x2, const void* ws2, const void* bias, void* out,
                                  int B, int K1, int K2, int N, int Ho, int Wo, int H2, int W2, int stride2, int config,
                                  int pieces, void* stream);
int wm2f_conv3x3_split_fwd_p(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N, int Hi,
                             int Wi, int stride, int relu, int config, int pieces, void* stream);
int wm2f_conv3x3_split_stats_fwd_p(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B, int Cin,
                                   int N, int Hi, int Wi, int stride, int config, int pieces, void* stream);
int wm2f_stem7x7_pool_fwd_p(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N, int Hi,
                            int Wi, int grid, int pieces, void* stream);

/* The 3x3 entry points with the route of the launch: 0 the direct kernel, which loads and splits x once per tap;
 * 1 the staged kernel, which splits an 8 x 32 pixel tile plus its halo once per channel block into LDS and reads the nine
 * taps from there -- the same MFMAs in the same order, so the same bits in `out`; -1 the host's rule, which is what every
 * entry point above means.  The staged kernel is built for stride 1 and the WN = 1 entries of the tile table, within the
 * device's LDS per workgroup; route = 1 anywhere else returns WM2F_EINVAL, launches nothing and leaves out and stats_out
 * untouched.  config keeps meaning the tile-table entry.
 * wm2f_conv3x3_split_route: pure host function, the route (0 / 1) and in *entry the tile-table entry the rule takes on a
 *                        device of n_cu CUs with 160 KiB of LDS per workgroup; -1 for arguments no launch accepts. */
int wm2f_conv3x3_split_fwd_r(const void* x, const void* w_split, const void* bias, void* out, int B, int Cin, int N, int Hi,
                             int Wi, int stride, int relu, int config, int pieces, int route, void* stream);
int wm2f_conv3x3_split_stats_fwd_r(const void* x, const void* w_split, void* out, void* stats_out, int G_out, int B, int Cin,
                                   int N, int Hi, int Wi, int stride, int config, int pieces, int route, void* stream);
int wm2f_conv3x3_split_route(int N, int Hi, int Wi, int stride, int B, int n_cu, int pieces, int* entry);

/* wm2f_swin_linear_split_fwd_p: the Linears of a Swin block and of patch merging (inference), all fp32, row-major
 *                        and token-major, W as nn.Linear stores it, at `pieces` of the split arithmetic above:
 *                            out (M, N) = epilogue(x (M, K) . W (N, K)^T + bias[N]).
 *                        Weights: w_split is exactly what wm2f_token_linear_split_weight(W, N, K) writes, the three-piece
 *                        split in fragment order [k-step][row tile][piece][lane][8 bf16], N * K * 6 bytes; there is no
 *                        second format.  A (feature tile, k-step) panel of any tile width that is a multiple of 16 is
 *                        contiguous in that order.  pieces in {1, 2, 3} reads the first `pieces` pieces of each row tile and
 *                        splits x into `pieces` pieces.
 *                        Shapes: K % 32 == 0, N % 16 == 0, M >= 1; x, every out and residual below 2 GiB each (32-bit
 *                        buffer offsets), N * K * 6 < 2 GiB.  M needs no alignment: the last token tile is partial, its
 *                        loads and stores are bounded.  N need not be a multiple of the workgroup's feature-tile width:
 *                        the last feature tile is partial in whole 16-row tiles.  Every pointer is 16-byte aligned.
 *                        epilogue = 0: + bias (bias may be NULL: patch merging's reduction has none);
 *                                   1: + bias, then exact GELU 0.5 v (1 + erf(v / sqrt 2)) on the fp32 value (F.gelu's default);
 *                                   2: + bias, then + residual[M, N]; residual is required (and NULL otherwise), and out0 may
 *                                      not alias it.
 *                        n_out = 1: out0 is (M, N), out1 and out2 are not looked at.
 *                                3: feature n goes to out{n / (N / 3)} at column n % (N / 3), each buffer (M, N / 3) and
 *                                   contiguous -- the merged q | k | v projection written as the three image-order tensors
 *                                   wm2f_swin_window_attn_fwd reads.  Needs (N / 3) % 16 == 0 and epilogue == 0.
 *                        config = -1: the host's choice from (M, N, pieces, CUs), wm2f_swin_linear_split_config;
 *                                 0 .. wm2f_swin_linear_split_configs() - 1: that entry of the tile table (tests, tuning).
 *                        Accumulation: as the token kernel, the products are chained into the accumulator -- every MFMA of
 *                        every k-step takes the running sum as its C operand, from +0 at k = 0 -- and the bias is added to
 *                        the finished sum, then the GELU or the residual.
 *                        Determinism: no split-K, no atomics.  Every output has one MFMA sequence, the same under every
 *                        config, every M, every position of the token in M and every way of cutting rows into calls: the
 *                        outputs are bit-identical across configs and across runs.
 *                        Non-finite: an inf or a NaN in x makes every output of its token non-finite and touches no other
 *                        token; finite values up to FLT_MAX stay finite where the result is representable.
 *                        Refusals: anything outside the above returns WM2F_EINVAL with nothing launched and the outputs
 *                        untouched; sizes (pieces, M, K, N, epilogue, n_out, config, the 2 GiB limits, a residual that does
 *                        not match the epilogue) are checked before a pointer is looked at.
 * wm2f_swin_linear_split_config: the host's choice for (M, N, pieces) on n_cu CUs, an index into the tile table; -1 for
 *                        sizes the kernel refuses.  wm2f_swin_linear_split_configs: how many entries the table has. */
int wm2f_swin_linear_split_fwd_p(const void* x, const void* w_split, const void* bias, const void* residual, void* out0,
                                 void* out1, void* out2, int64_t M, int K, int N, int epilogue, int n_out, int config,
                                 int pieces, void* stream);
int wm2f_swin_linear_split_config(int64_t M, int N, int pieces, int n_cu);
int wm2f_swin_linear_split_configs(void);

/* wm2f_token_wgrad_bf16: the weight / bias gradient of such a Linear (the backward autograd derives for nn.Linear; train
 *                        step of HF:1036-1103 under bf16 autocast):  dw (N, K) fp32 = dy (M, N)^T . x (M, K),
 *                        db (N) fp32 = column sums of dy (NULL: skipped); dy, x bf16 row-major, fp32 accumulation on the bf16
 *                        matrix cores.  Split over the M = batch x tokens contraction with one fp32 partial tile per
 *                        workgroup in `workspace` (wm2f_token_wgrad_workspace(M, N, K) bytes), added in split order by a
 *                        second kernel: deterministic, no atomics.  HBM-bound (each operand read once).  N % 8 == 0,
 *                        K % 8 == 0, operands below 2 GiB, pointers 16-byte aligned. */
int64_t wm2f_token_wgrad_workspace(int64_t M, int N, int K);
int wm2f_token_wgrad_bf16(const void* dy, const void* x, void* dw, void* db, void* workspace, int64_t M, int N, int K,
                          void* stream);
/* The same with fp32 operands (the fp32 train step) on the fp32 matrix cores: exact fp32 products, MFMA-bound
 * (2 M N K flop at 157 TFLOP/s).  N % 4 == 0, K % 4 == 0; same workspace function. */
int wm2f_token_wgrad_f32(const void* dy, const void* x, void* dw, void* db, void* workspace, int64_t M, int N, int K,
                         void* stream);
/* wm2f_tokens_to_nchw: out (B, C, HW) = tokens (B, S, C) rows [start, start + HW) transposed per image -- the
 *                      `hidden[:, start:start+hw].transpose(1, 2).reshape(B, C, h, w)` of HF:1384-1391. */
int wm2f_tokens_to_nchw(const void* tokens, void* out, int B, int S, int C, int start, int HW, void* stream);
/* wm2f_group_norm_tokens: tokens[b][start + p][c] = GroupNorm_G(x + bias)[b][c][p] * gamma + beta for x (B, C, HW) fp32,
 *                         bias (C) or NULL, tokens (B, S, C) -- one level's input projection of the pixel decoder
 *                         (HF:1341-1357: Conv2d 1x1 [+ bias] + GroupNorm, flatten(2).transpose(1, 2), cat over levels)
 *                         written into its rows of the token buffer.  stats_ws: 2 * B * G doubles of scratch. */
int wm2f_group_norm_tokens(const void* x, const void* bias, const void* gamma, const void* beta, void* tokens,
                           void* stats_ws, int B, int C, int G, int HW, int S, int start, float eps, void* stream);
/* wm2f_resize_bilinear: y (NC, Ho, Wo) = torch.nn.functional.interpolate(x (NC, H, W), size=(Ho, Wo), mode="bilinear",
 *                       align_corners=False) in fp32, Wo % 4 == 0 -- the resize of HF:2048-2050, applied to the mask
 *                       FEATURES once per level instead of to every layer's logits (resize and einsum commute). */
int wm2f_resize_bilinear(const void* x, void* y, int NC, int H, int W, int Ho, int Wo, void* stream);
/* wm2f_resize_pyramid: the same resize to (H/2, W/2), (H/4, W/4) and (H/8, W/8) in one pass over x (NC, H, W), H and W
 *                      divisible by 8: y2 (NC, H/2, W/2), y4 (NC, H/4, W/4), y8 (NC, H/8, W/8), each bit for bit what
 *                      wm2f_resize_bilinear gives for that size (at these ratios every output is the mean of a 2 x 2 block). */
int wm2f_resize_pyramid(const void* x, void* y2, void* y4, void* y8, int NC, int H, int W, void* stream);
/* wm2f_bias_relu_maxpool: y (N, C, H/2, W/2) = MaxPool2d(kernel 3, stride 2, padding 1)(ReLU(x + bias[c])), x (N, C, H, W)
 *                         fp32, H even, W % 8 == 0 -- the stem of transformers' ResNet embeddings
 *                         (modeling_resnet.py ResNetEmbeddings: convolution, normalization folded, ReLU, pooler). */
int wm2f_bias_relu_maxpool(const void* x, const void* bias, void* y, int N, int C, int H, int W, void* stream);
/* wm2f_group_norm_act: y = act(GroupNorm_G(x) * gamma + beta (+ bilinear_upsample(up -> H x W))) on (B, C, H, W) fp32,
 *                      W % 4 == 0 -- the GroupNorm tails of the FPN step, HF:1395-1405 (adapter: with `up` =
 *                      the coarser map (B, C, Hs, Ws), align_corners = False, no ReLU; output layer: up = NULL,
 *                      relu = 1).  stats_ws: 2 * B * G doubles of scratch.  y may alias x. */
int wm2f_group_norm_act(const void* x, const void* gamma, const void* beta, const void* up, void* y, void* stats_ws,
                        int B, int C, int G, int H, int W, int Hs, int Ws, float eps, int relu, void* stream);

/* Importance sampling of the mask losses, HF:688-704 (sample_points_using_uncertainty): the points of the k largest scores of
 * each row -- gather(coords, topk(uncertainty, k)[1]) -- by radix selection in LDS instead of the sort a stock top-k of
 * thousands is.
 *   score (rows, n) fp32; pts (rows, n, 2) fp32; out (rows, out_row_points, 2) fp32: entries [0, k) of each row are written,
 *   in INDEX order (the losses sum over points, so only the set matters); equal scores at the threshold: lowest indices first;
 *   NaN ranks highest (as torch.topk).  n <= 38400 (the row's keys live in LDS), else WM2F_EUNSUPPORTED. */
int wm2f_select_top_points(const void* score, const void* pts, void* out, int rows, int n, int k, int out_row_points,
                           void* stream);

/* ---- point-sampled mask loss, batched over the prediction levels --------
 * Replaces, for all levels of a step in one launch each, the per-level tensor work of Mask2FormerLoss.loss_masks
 * (HF:580-640) with sample_points_using_uncertainty (HF:671-724), sample_point (HF:245-274),
 * sigmoid_cross_entropy_loss (HF:308-324) and dice_loss (HF:278-305).
 *   level_maps / level_grads: HOST array of n_levels (<= 16) DEVICE pointers, each (N, H, W) fp32 -- the level
 *   tensors are used where they are, not stacked.   pts (n_levels, M, P, 2) in [0,1] (x, y); index (n_levels, M)
 *   int32 DEVICE: which map of its level row m samples.
 * wm2f_point_sample_levels_fwd: out (n_levels, M, P); neg_abs != 0 stores -|value| (the uncertainty, HF:688-690).
 * wm2f_point_sample_levels_bwd: atomically adds grad_out * bilinear weights into the (zero-initialised) level_grads.
 * wm2f_point_sample_levels_bwd_unique: the same when every (level, index) pair is distinct (the matched rows of a
 *                               one-to-one assignment): each indexed map is accumulated band by band in LDS and
 *                               OVERWRITTEN with plain stores (no global atomics; maps that no row indexes are not
 *                               touched -- clear those).  W <= 16384.
 * wm2f_mask_loss_rows_fwd:      logits, labels (R, P) -> bce_mean (R), dice (R), sums (R, 4) kept for the backward.
 * wm2f_mask_loss_rows_bwd:      grad (R, P) = g_bce[r] * d bce_mean[r] + g_dice[r] * d dice[r]. */
int wm2f_point_sample_levels_fwd(const void* const* level_maps, int n_levels, const void* pts, const int32_t* index,
                                 void* out, int M, int H, int W, int P, int neg_abs, void* stream);
int wm2f_point_sample_levels_bwd(const void* grad_out, const void* pts, const int32_t* index,
                                 void* const* level_grads, int n_levels, int M, int H, int W, int P, void* stream);
int wm2f_point_sample_levels_bwd_unique(const void* grad_out, const void* pts, const int32_t* index,
                                        void* const* level_grads, int n_levels, int M, int H, int W, int P, void* stream);
int wm2f_mask_loss_rows_fwd(const void* logits, const void* labels, void* sums, void* bce_mean, void* dice,
                            int R, int P, void* stream);
int wm2f_mask_loss_rows_bwd(const void* logits, const void* labels, const void* sums, const void* g_bce,
                            const void* g_dice, void* grad, int R, int P, void* stream);

/* ---- instance post-processing on device ----------------------------------
 * Replaces the tensor work of Mask2FormerImageProcessor.post_process_instance_segmentation,
 * transformers 5.15.0 models/mask2former/image_processing_mask2former.py:627-746 (callers: reference
 * models/metrics.py:58-63, models/mask2former/inference.py:30).  The dependency resizes the logits to a fixed
 * gh x gw = 384 x 384 grid (bilinear, :680-682); these kernels evaluate that resize on the fly.
 *   mask_logits (B, Q, h, w) fp32; qidx (B, K) int32 DEVICE: the source query of each selected (query, class)
 *   pair (:698-702).
 * wm2f_instance_scores:        sum_sig[b,k] = sum sigmoid(l) over grid pixels with l > 0, cnt[b,k] = their number
 *                              (:703-708: mask score = sum_sig / (cnt + 1e-6)).
 * wm2f_instance_any:           any_out[b,k] = does the `nearest`-resized (Ho x Wo) mask have a set pixel (:715-717,
 *                              :724); evaluated only where cand[b,k] != 0.
 * wm2f_instance_segmentation:  segmentation (B, Ho, Wo) fp32: id r of the LAST kept instance covering the pixel,
 *                              -1 elsewhere (:712-735).  kept_q (B, K) int32: source query of kept instance r,
 *                              n_kept (B) int32, both DEVICE.
 * wm2f_instance_maps:          the kept binary masks of ONE image, (n, Ho, Wo) fp32 0/1 (return_binary_maps, :741-743);
 *                              image_logits = that image's (Q, h, w) slab. */
int wm2f_instance_scores(const void* mask_logits, const int32_t* qidx, void* sum_sig, void* cnt, int B, int Q,
                         int K, int h, int w, int gh, int gw, void* stream);
int wm2f_instance_any(const void* mask_logits, const int32_t* qidx, const uint8_t* cand, int32_t* any_out, int B,
                      int Q, int K, int h, int w, int gh, int gw, int Ho, int Wo, void* stream);
int wm2f_instance_segmentation(const void* mask_logits, const int32_t* kept_q, const int32_t* n_kept,
                               void* segmentation, int B, int Q, int K, int h, int w, int gh, int gw, int Ho,
                               int Wo, void* stream);
int wm2f_instance_maps(const void* image_logits, const int32_t* kept_q, int n, void* maps, int h, int w, int gh,
                       int gw, int Ho, int Wo, void* stream);

/* ---- semantic and panoptic post-processing on device ------------------------------------
 * The pixel work of Mask2FormerImageProcessor.post_process_semantic_segmentation and
 * post_process_panoptic_segmentation, transformers 5.15.0 image_processing_mask2former.py:550-625 and :748-841
 * (compute_segments :167-224).  mask_logits (B, Q, h, w) fp32 DEVICE; gh x gw = the dependency's 384 x 384 grid;
 * Ho x Wo = one target size (one call per distinct size); rows (nrows) int32 DEVICE: the image of each output slot.
 * wm2f_semantic_scores:        scores (B, C, gh, gw) fp32 = sum over q, ascending, of class_probs[b,q,c] *
 *                              sigmoid(bilinear(logits[b,q])); class_probs (B, Q, C) fp32 DEVICE (softmax without the
 *                              null class).
 * wm2f_semantic_resize_argmax: segmentation (nrows, Ho, Wo) int64 = first-max argmax over c of the bilinear resize of
 *                              scores[rows[j]] to Ho x Wo; out_scores (nrows, C, Ho, Wo) fp32 = that resize, or NULL.
 * wm2f_panoptic_probs:         probs (B, K, gh, gw) fp32 = sigmoid(bilinear(logits[b, kept_q[b,k]])) for
 *                              k < n_kept[b]; kept_q (B, K), n_kept (B) int32 DEVICE.
 * wm2f_panoptic_segments:      segmentation (nrows, Ho, Wo) int32 = first-max argmax over k < n_kept of
 *                              bilinear(probs[b,k]) * scores[b,k] (b = rows[j]); counts (B, K, 2) int32, zeroed by the
 *                              caller, accumulates [0] = #pixels with that product >= mask_threshold, [1] = #pixels
 *                              whose argmax is k.  scores (B, K) fp32 DEVICE.  n_kept[rows[j]] > 0 is required.
 * wm2f_panoptic_relabel:       segmentation[j][p] = table[rows[j] * K + segmentation[j][p]] in place; table (B, K)
 *                              int32 DEVICE (segment id of each kept query, 0 = rejected). */
int wm2f_semantic_scores(const void* mask_logits, const void* class_probs, void* scores, int B, int Q, int C, int h,
                         int w, int gh, int gw, void* stream);
int wm2f_semantic_resize_argmax(const void* scores, const int32_t* rows, int nrows, void* segmentation,
                                void* out_scores, int C, int gh, int gw, int Ho, int Wo, void* stream);
int wm2f_panoptic_probs(const void* mask_logits, const int32_t* kept_q, const int32_t* n_kept, void* probs, int B,
                        int Q, int K, int h, int w, int gh, int gw, void* stream);
int wm2f_panoptic_segments(const void* probs, const int32_t* rows, const int32_t* n_kept, const void* scores,
                           int32_t* segmentation, int32_t* counts, int nrows, int K, int gh, int gw, int Ho, int Wo,
                           float mask_threshold, void* stream);
int wm2f_panoptic_relabel(int32_t* segmentation, const int32_t* rows, const int32_t* table, int nrows, int K,
                          int64_t n_pixels, void* stream);

/* ---- label expansion on device ------------------------------------------
 * The tensor work of convert_segmentation_map_to_binary_masks (image_processing_mask2former.py:227-259,
 * image_processing_pil_mask2former.py:81-114), so that a sample can travel as its (H, W) instance-id map instead of
 * the float (T, H, W) mask stack the reference stores (datasets/dataset_utils.py:56-70).
 *   label_map (n_pixels) int32 DEVICE, n_pixels % 4 == 0; ids (T) int32 DEVICE (ascending unique ids, ignore
 *   index removed); masks (T, n_pixels) uint8: masks[t][i] = (label_map[i] == ids[t]). */
int wm2f_labelmap_to_masks(const int32_t* label_map, const int32_t* ids, uint8_t* masks, int64_t n_pixels, int T,
                           void* stream);

/* ---- segmentation mAP on device ----------------------------------------------------
 * The hot part of torchmetrics MeanAveragePrecision(iou_type="segm") -- pycocotools COCOeval.evaluate on binary
 * masks -- as the reference's models/metrics.py::test_with_metrics and show_worst_predictions.py use it.  The host
 * keeps COCOeval.accumulate / summarize (weed_instance_segmentation_amd/metrics.py).
 * wm2f_labelmap_pair_counts: hist (B, P+1, G+1) int32 = joint histogram of, per image, the prediction id map
 *                         pred_map (B, n_pixels) -- WM2F_F32 (ids as floats, -1 background: the post-processor's output)
 *                         or WM2F_I32 -- and the GT raw-id map gt_map (B, n_pixels), WM2F_U8 or WM2F_I32.  Row r > 0 is
 *                         prediction id r-1 (ids outside [0, P) count as row 0); column c > 0 is the GT raw id
 *                         gt_ids[b][c-1] -- gt_ids (B, G) int32, ascending, n_ids (B) int32 of them valid per image --
 *                         any other raw id is column 0.  Inner bins are intersections, row / column sums are areas.
 *                         The histogram is overwritten (cleared on the stream first).  G <= 4096, else WM2F_EUNSUPPORTED.
 *                         An LDS histogram per block while (P+1)(G+1) <= 12288, global atomics above.
 * wm2f_mask_pair_counts:   det_masks (D, n_pixels), gt_masks (G, n_pixels) uint8 (any nonzero byte is set, masks may
 *                         overlap) -> inter (D, G), det_area (D), gt_area (G) int32, all overwritten.  workspace of
 *                         wm2f_mask_pair_counts_workspace(D, G, n_pixels) bytes (the bit-packed stacks).  n_pixels < 2^31.
 * wm2f_coco_match:         greedy COCO matching (COCOeval.evaluateImg) of B images at once, one 64-lane workgroup per
 *                         image, one lane per (area range, IoU threshold), IoU = inter / union in fp64.
 *                         inter (B, D, G), det_area / det_label / det_order (B, D), gt_area / gt_label (B, G),
 *                         n_det / n_gt (B) int32.  det_order: the image's detection indices by descending score, stable
 *                         (padding after the n_det real ones).  A GT labelled INT32_MIN does not exist.
 *                         iou_thresholds (T) and area_ranges (A, 2) fp64 (inclusive [lo, hi]), A * T <= 64.
 *                         Out: det_rank (B, D) = rank of the detection among its image's detections of its category in
 *                         score order (-1 for padding); det_matched / det_ignored (B, A, T, D) uint8 (0 for ranks >=
 *                         max_det); gt_ignored (B, A, G) uint8.  Only the first max_det detections per (image, category)
 *                         are matched.  LDS holds the image's detections (16 B each), its GT (20 B each), and a flag
 *                         per (lane, GT): D <= 1024 and G <= 512 per image (46 KiB at both bounds and A * T = 40), else
 *                         WM2F_EUNSUPPORTED.
 * wm2f_coco_match_min:     wm2f_coco_match with a second triple inter2 (B, D, G), det_area2 (B, D), gt_area2 (B, G) int32:
 *                         the IoU of a pair is min(inter / union, inter2 / union2), each quotient in fp64 and 0 where its
 *                         intersection is 0 (Boundary AP, DESIGN section 25: the first triple counts mask pixels, the
 *                         second the pixels of the boundary bands).  Area ranges, labels, order, ranks and every output are
 *                         as in wm2f_coco_match, taken from the first triple; with a second triple equal to the first the
 *                         outputs are those of wm2f_coco_match bit for bit.  The same kernel body (a template flag): the
 *                         second intersection row sits in registers next to the first, the second areas add 4 B per
 *                         detection and per GT to LDS -- 52 KiB at D = 1024, G = 512, A * T = 40.  Same bounds. */
int wm2f_labelmap_pair_counts(const void* pred_map, int pred_dtype, const void* gt_map, int gt_dtype,
                              const int32_t* gt_ids, const int32_t* n_ids, int32_t* hist, int B, int64_t n_pixels, int P,
                              int G, void* stream);
int64_t wm2f_mask_pair_counts_workspace(int D, int G, int64_t n_pixels);
int wm2f_mask_pair_counts(const uint8_t* det_masks, const uint8_t* gt_masks, int32_t* inter, int32_t* det_area,
                          int32_t* gt_area, void* workspace, int D, int G, int64_t n_pixels, void* stream);
int wm2f_coco_match(const int32_t* inter, const int32_t* det_area, const int32_t* gt_area, const int32_t* det_label,
                    const int32_t* gt_label, const int32_t* det_order, const int32_t* n_det, const int32_t* n_gt,
                    const double* iou_thresholds, const double* area_ranges, int32_t* det_rank, uint8_t* det_matched,
                    uint8_t* det_ignored, uint8_t* gt_ignored, int B, int D, int G, int T, int A, int max_det,
                    void* stream);
int wm2f_coco_match_min(const int32_t* inter, const int32_t* det_area, const int32_t* gt_area, const int32_t* inter2,
                        const int32_t* det_area2, const int32_t* gt_area2, const int32_t* det_label,
                        const int32_t* gt_label, const int32_t* det_order, const int32_t* n_det, const int32_t* n_gt,
                        const double* iou_thresholds, const double* area_ranges, int32_t* det_rank,
                        uint8_t* det_matched, uint8_t* det_ignored, uint8_t* gt_ignored, int B, int D, int G, int T,
                        int A, int max_det, void* stream);

/* ---- per-instance statistics of id maps on device ---------------------------------------
 * Area, bounding box and coordinate sums of every instance of B id maps, in one read of the maps: what a consumer of
 * post_process_instance_segmentation's map (counts, targets, box mAP) otherwise takes with one `map == id` pass per
 * instance.
 * wm2f_labelmap_instance_stats: map (B, H, W) is WM2F_F32 (ids as floats, -1 background: the post-processor's output;
 *                         a value counts as the integer it equals, +-0 as 0, and a value that is negative, fractional,
 *                         not finite or >= 2^24 as no id), WM2F_I32 or WM2F_U8.
 *                         ids == NULL (then n_ids == NULL): row r of the result is id r, r in [0, N); every other
 *                         value is ignored.  Otherwise ids (B, N) int32 DEVICE, ascending, n_ids (B) int32 DEVICE of
 *                         them valid per image (the GT form of wm2f_labelmap_pair_counts): row r is the raw id
 *                         ids[b][r]; rows at or beyond n_ids[b] are empty, raw ids not listed are ignored.
 *                         stats (B, N, 8) int64, overwritten: [area, xmin, ymin, xmax, ymax, sum_x, sum_y, 0] with
 *                         xmax / ymax inclusive pixel indices; an id without a pixel gets [0, W, H, -1, -1, 0, 0, 0].
 *                         All integer: the result does not depend on the order of accumulation and is bit-identical
 *                         from run to run.  H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED.
 *                         A workgroup owns a strip of whole rows and keeps its accumulators in LDS while N <= 1024
 *                         (32 B per id, and 4 B per listed id: 36 KiB at the cap, four workgroups per CU), flushing the
 *                         ids it saw with 64-bit integer atomics; above that it accumulates into stats directly.  Rows
 *                         are read four pixels per lane when W % 4 == 0 and the map is 16-byte (uint8: 4-byte) aligned,
 *                         pixel by pixel otherwise, with the same results. */
int wm2f_labelmap_instance_stats(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids, int64_t* stats,
                                 int B, int H, int W, int N, void* stream);

/* ---- boundary bands of id maps on device ------------------------------------------------
 * The pixel work of Boundary IoU (Cheng et al., CVPR 2021) for every instance of B id maps at once.  For a mask M the
 * band is M minus its erosion by a (2d+1) x (2d+1) square, pixels beyond the image counting as outside M; on an id map
 * a pixel with id k is INTERIOR iff that square around it lies inside the image and every pixel of it has id k, and is
 * in the band of k otherwise.
 * wm2f_labelmap_boundary:  map (B, H, W) is WM2F_F32, WM2F_I32 or WM2F_U8.  Which float is which id follows
 *                         wm2f_labelmap_instance_stats (negative, fractional, not finite or >= 2^24: no id); a negative
 *                         int32 is no id either.  A pixel without an id equals no id, so it ends every run it touches.
 *                         out (B, H, W) int32, overwritten: the pixel's id where the pixel is in its instance's band,
 *                         -1 where it is interior or has no id -- again an id map with -1 background.
 *                         workspace: wm2f_labelmap_boundary_workspace(B, H, W) bytes = B * H * W, one byte per pixel,
 *                         4-byte aligned for the four-pixel path; it needs no clearing and holds nothing afterwards.
 *                         1 <= d <= 16384 (a d larger than both sides leaves no interior), H, W <= 16384, B <= 32, else
 *                         WM2F_EUNSUPPORTED; sizes or d below 1 are WM2F_EINVAL.
 *                         Two launches, each reading the map once, whatever d and the number of instances:
 *                         rows -- a wave per row; the run of equal ids ending at x has length x - lastchange(x) + 1 and
 *                         lastchange is a max-scan (in the lane, across the wave by shuffles, across 64- or 256-pixel
 *                         steps by a carry); plane[y][x] = 1 iff that run has at least 2d+1 pixels, so the row segment
 *                         centred at x passes iff x + d < W and plane[y][x + d].  Four pixels per lane when W % 4 == 0
 *                         and map and workspace are aligned (16 B, uint8: 4 B), one otherwise, with the same results.
 *                         columns -- a lane per column marching down a chunk of rows (at least 64 and 2d of them) with
 *                         the count of consecutive rows that pass and carry one id in a register; at 2d+1 the pixel d
 *                         rows up is interior.  A chunk walks d rows beyond each end of the rows it owns.
 *                         All integer, bit-identical from run to run. */
int64_t wm2f_labelmap_boundary_workspace(int B, int H, int W);
int wm2f_labelmap_boundary(const void* map, int dtype, int32_t* out, void* workspace, int B, int H, int W, int d,
                           void* stream);

/* ---- interior distance maps and aim points of id maps on device ---------------------------
 * Where inside an instance to aim: the pixel farthest from everything that is not the instance, i.e. the maximum of the
 * instance's interior Euclidean distance transform, and that maximum (the clearance) as its size measure.
 * wm2f_labelmap_distance:  map (B, H, W) is WM2F_F32, WM2F_I32 or WM2F_U8.  Which value is which id follows
 *                         wm2f_labelmap_instance_stats (a float that is negative, fractional, not finite or >= 2^24 is
 *                         no id; +-0 is id 0); a negative int32 is no id either.
 *                         d2 (B, H, W) int32, overwritten, every element: for a pixel with id k the squared Euclidean
 *                         distance between pixel centres to the nearest position that does not carry id k; 0 for a
 *                         pixel without an id.  border_outside != 0: the positions just beyond the image (x = -1, x = W,
 *                         y = -1, y = H) count as not carrying k, the convention of the boundary bands.
 *                         border_outside == 0: only real pixels count, and a pixel whose id fills its whole image gets
 *                         INT32_MAX.  d2 <= 2 * 16384^2 fits int32.
 *                         workspace: wm2f_labelmap_distance_workspace(B, H, W) bytes, 16-byte aligned: two bytes per
 *                         pixel (g, below) rounded up to 16, then 16 bytes per column and chunk of rows.  It needs no
 *                         clearing and holds nothing afterwards.
 *                         H, W <= 16384, B <= 32, else WM2F_EUNSUPPORTED; sizes below 1 are WM2F_EINVAL (both are
 *                         decided before a pointer is looked at).
 *                         Three launches whatever B and the number of instances; the map is read four times in all.
 *                         summary -- a lane per column marching down a chunk of rows (at least 32 of them): the id
 *                         and length of the run of equal ids at the chunk's top and bottom.
 *                         columns -- the same grid; a lane takes the run that ends just above its chunk from the
 *                         summaries, marches down, takes the run below and marches back up:
 *                         g(x, y) = vertical distance to the nearest position of column x that does not carry the
 *                         pixel's id, uint16, 0 without an id, 0xffff where there is none (border-inside mode only).
 *                         rows -- a workgroup stages whole rows in LDS (ids, g and h: 8 bytes per pixel, 128 KiB for
 *                         a row of 16384; rows shorter than 1024 share a workgroup).  A wave per row finds every
 *                         pixel's run of equal ids (ballot and bit scan with a carry) and from it h, the horizontal
 *                         distance to the nearest position off the pixel's id.  A pixel starts from min(g, h)^2 and
 *                         walks outwards while step^2 is below its best, offering step^2 + min(g(x - step),
 *                         g(x + step))^2.  Exact: beyond a pixel of another id nothing is nearer than that pixel, and
 *                         the walk ends before it leaves the run.  Rows are staged four pixels per lane when
 *                         W % 4 == 0 and the map is 16-byte (uint8: 4-byte) aligned, pixel by pixel otherwise, with the
 *                         same results.  All integer, bit-identical from run to run.
 * wm2f_labelmap_aim_points: map and d2 as above (d2 is that kernel's output for this map), ids / n_ids as in
 *                         wm2f_labelmap_instance_stats (NULL: row r is id r of [0, N); else (B, N) ascending raw ids,
 *                         n_ids (B) of them valid), stats that kernel's (B, N, 8) int64 output for the same map and
 *                         rows, or NULL.
 *                         points (B, N, 4) int32, 16-byte aligned, overwritten: [x, y, d2max, 0] for an instance with
 *                         pixels, [-1, -1, 0, 0] for an id without one.  (x, y) is a pixel of the instance with the
 *                         largest d2; among equals the one nearest the rounded centroid cx = (2 sum_x + area) /
 *                         (2 area), cy likewise (int64 division), by (x - cx)^2 + (y - cy)^2 as integers; among those
 *                         the smallest y * W + x.  stats == NULL: the centroid term is 0 and the raster rule decides.
 *                         workspace: wm2f_labelmap_aim_points_workspace(B, N) = 20 * B * N bytes, 8-byte aligned.
 *                         H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED; sizes below 1 are WM2F_EINVAL.
 *                         Four launches, nothing read back: init, an atomicMax of d2 per instance, an unsigned 64-bit
 *                         atomicMin of (centroid distance^2 << 32 | y * W + x) over the pixels that attain it (<= 2^29
 *                         and < 2^28), and the rows.  Accumulators live in LDS while N <= 1024.  Integer atomics only:
 *                         the result does not depend on their order. */
int64_t wm2f_labelmap_distance_workspace(int B, int H, int W);
int wm2f_labelmap_distance(const void* map, int dtype, int32_t* d2, void* workspace, int B, int H, int W,
                           int border_outside, void* stream);
int64_t wm2f_labelmap_aim_points_workspace(int B, int N);
int wm2f_labelmap_aim_points(const void* map, int dtype, const int32_t* d2, const int32_t* ids, const int32_t* n_ids,
                             const int64_t* stats, int32_t* points, void* workspace, int B, int H, int W, int N,
                             void* stream);

/* ---- nearest-instance maps and per-cell pixel counts of id maps on device ------------------
 * The exterior counterpart of wm2f_labelmap_distance: for every pixel the nearest instance and how far away it is, up
 * to a cap -- growing ids by a margin (skimage's expand_labels), a protection distance round crop plants, bare pixels
 * assigned to the plant that owns them -- and the pixel counts of the cells of a sprayer's grid.
 * wm2f_labelmap_nearest:   map (B, H, W) is WM2F_F32, WM2F_I32 or WM2F_U8.  The instances are the ids 0 .. N-1, by the
 *                         rule of wm2f_labelmap_instance_stats for floats; every other value is free (the convention
 *                         of wm2f_labelmap_clean).  source (B, N) uint8 or NULL: instance id of image b is a source when
 *                         source is NULL or source[b, id] != 0.
 *                         nearest, d2 (B, H, W) int32, overwritten, every element.  For a pixel p take the source
 *                         pixels q with |p - q|^2 <= max_d2, distances between pixel centres; the image border is not
 *                         a source.  None: nearest = -1, d2 = INT32_MAX.  Otherwise d2 is the smallest such distance
 *                         and nearest the smallest id among the sources that attain it; a source pixel so gets its
 *                         own id and d2 = 0.
 *                         flags: WM2F_NEAREST_BLOCKED -- a pixel of an instance that is not a source is written as
 *                         its own id with d2 = 0 (growth: other plants keep their pixels); without it such a pixel is
 *                         a query like a free pixel (protection: a weed pixel's distance to the crop).  Growth is
 *                         Euclidean, as in skimage: it may jump across a blocking plant; geodesic growth is out of
 *                         scope.  WM2F_NEAREST_WALK_ALL -- every pixel walks its row even where the prefix count
 *                         (below) says nothing is in range; same results, for measuring what the count saves.
 *                         0 <= max_d2 <= 1024^2 (the margin r = floor(sqrt(max_d2)) <= 1024), H, W <= 16384, B <= 32,
 *                         N <= 4096, else WM2F_EUNSUPPORTED; sizes below 1, a negative max_d2 and unknown flags are
 *                         WM2F_EINVAL (both are decided before a pointer is looked at).  The uncapped (Voronoi) map is
 *                         out of scope: its walk has no bound.
 *                         workspace: wm2f_labelmap_nearest_workspace(B, H, W) bytes, 16-byte aligned: six bytes per
 *                         pixel (g uint16 rounded up to 16 bytes, then the column's id int32).  It needs no clearing.
 *                         Two launches whatever B and N.  Exact in integers and separable: with g(x', y) the vertical
 *                         distance to the nearest source pixel of column x', the answer is the minimum over x' of
 *                         ((x - x')^2 + g(x', y)^2, id).
 *                         columns -- a lane per column over chunks of at least 32 rows; a chunk starts its march r
 *                         rows above itself and its march back r rows below, so it needs no summary of other chunks.
 *                         It writes g (r + 1: none within r) and the id of that source pixel, the smaller id where
 *                         the one above and the one below are equally far (within a column the smaller |dy| wins and
 *                         an equal |dy| occurs at most twice).
 *                         rows -- a workgroup stages whole rows of g and id in LDS (rows shorter than 1024 share
 *                         one; a row longer than 4096 gets 1024 threads), builds per row the prefix count of pixels
 *                         with g <= r, and a pixel whose window [x - r, x + r] counts none writes "none" after one
 *                         subtraction.  Every other pixel walks s = 0, 1, ... <= r while s^2 <= its best (not <: a
 *                         candidate at equal distance with a smaller id still has to be seen), four steps' reads in
 *                         flight.  All integer, bit-identical from run to run.
 * wm2f_labelmap_cell_counts: map as above.  Pixel (x, y) lies in cell ((y + off_y) / cell_h, (x + off_x) / cell_w),
 *                         0 <= off < cell; GH = ceil((H + off_y) / cell_h), GW = ceil((W + off_x) / cell_w).
 *                         group (B, N) uint8: group[b, id] in 0 .. G-1 names the column an instance's pixels are
 *                         counted in; 255 (any value >= G): not counted.  Free pixels are not counted.
 *                         veto_d2 (B, H, W) int32 or NULL (wm2f_labelmap_nearest's d2 towards the protected
 *                         instances): counts[b, cy, cx, g] gets the pixel when veto_d2 is NULL or veto_d2[p] > veto_max,
 *                         counts[b, cy, cx, G + g] otherwise -- what the protection zone took away.
 *                         counts (B, GH, GW, 2G) int32, written in full by the call (no memset contract).  1 <= G <= 8.
 *                         H, W, cell_h, cell_w <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED; sizes below 1, an
 *                         offset outside [0, cell), G outside [1, 8] and a negative veto_max are WM2F_EINVAL (decided
 *                         before a pointer is looked at).
 *                         One launch, one read of the map: a workgroup owns a tile of cells, counts its pixels into
 *                         integer LDS accumulators and stores the tile.  Bit-identical from run to run. */
#define WM2F_NEAREST_BLOCKED 1
#define WM2F_NEAREST_WALK_ALL 2
#define WM2F_NEAREST_MAX_D2 (1024 * 1024)
#define WM2F_CELL_MAX_GROUPS 8
int64_t wm2f_labelmap_nearest_workspace(int B, int H, int W);
int wm2f_labelmap_nearest(const void* map, int dtype, const uint8_t* source, int32_t* nearest, int32_t* d2,
                          void* workspace, int B, int H, int W, int N, int max_d2, int flags, void* stream);
int wm2f_labelmap_cell_counts(const void* map, int dtype, const uint8_t* group, const int32_t* veto_d2, int veto_max,
                              int32_t* counts, int B, int H, int W, int N, int G, int cell_h, int cell_w, int off_y,
                              int off_x, void* stream);

/* ---- panoptic quality and semantic mIoU on device ---------------------------------------
 * What scores the maps of post_process_panoptic_segmentation and post_process_semantic_segmentation: the segment
 * matching of panopticapi's pq_compute (which torchmetrics' PanopticQuality follows) and the confusion matrix mIoU is
 * made of.  The host keeps the per-class sums (weed_instance_segmentation_amd/panoptic_metrics.py).
 * wm2f_panoptic_match:     segment matching of B images in one launch, one 256-thread workgroup per image.
 *                         hist (B, P+1, G+1) int32 in the layout of wm2f_labelmap_pair_counts: row r > 0 is prediction
 *                         segment r-1, row 0 no prediction; column c > 0 is GT segment c-1, column 0 no listed GT (void).
 *                         Rows or columns that form one segment (a stuff class, a fused id) are added up by the caller
 *                         first, in integers.  An image's bins sum to its pixel count, < 2^31.
 *                         pred_label (B, P), gt_label (B, G), n_pred / n_gt (B) int32.  A row at or beyond n_pred[b], or
 *                         labelled INT32_MIN, or without a pixel, does not exist; the same for columns.
 *                         Areas are row and column sums over the whole histogram, taken inside the kernel.
 *                         pred_void = hist[p][0], or 0 when void_as_background != 0.  For an existing pair of equal
 *                         label with inter > 0: union = pred_area - pred_void + gt_area - inter, and the pair matches
 *                         iff 2 * inter > union, decided in int64 (an IoU of exactly 1/2 does not match; no rounding
 *                         takes part).  Segments being disjoint, a row and a column match at most once.
 *                         Out, all overwritten: gt_match (B, G) int32 = the matched prediction row, -1 for an existing
 *                         GT segment without a match (a false negative), -2 for a column that does not exist;
 *                         gt_iou (B, G) fp64 = (double)inter / (double)union of the match, one division, else 0;
 *                         pred_state (B, P) uint8 = 0 matched, 1 false positive, 2 dropped because mostly void
 *                         (unmatched and 2 * pred_void > pred_area; exactly half in void is a false positive),
 *                         3 does not exist.
 *                         Rows are walked in the outer loop with the lanes across the GT columns.  LDS: 16 B per row,
 *                         8 B per column.  P <= 1024 and G <= 4096 (48 KiB), else WM2F_EUNSUPPORTED.
 * wm2f_semantic_confusion: conf (C, C) int64 += the confusion matrix of B class maps, rows = GT, columns = prediction.
 *                         pred (B, n_pixels) is WM2F_I64 (post_process_semantic_segmentation's output), WM2F_I32 or
 *                         WM2F_U8.  gt (B, n_pixels) is WM2F_U8 or WM2F_I32 and holds
 *                           - classes when gt_ids == NULL (then gt_cls == n_ids == NULL and G == 0), or
 *                           - raw ids otherwise: gt_ids (B, G) int32 ascending, gt_cls (B, G) int32 their classes,
 *                             n_ids (B) int32 of them valid per image (the GT form of wm2f_labelmap_pair_counts); a raw
 *                             id that is not listed has class background_label (pass a negative one to ignore it).
 *                         A pixel whose GT class equals ignore_index or lies outside [0, C) is ignored (pass INT32_MIN
 *                         for no ignore_index).  A pixel that is not ignored and whose prediction lies outside [0, C)
 *                         is counted in n_out_of_range[0] (int64) and in no bin.
 *                         conf and n_out_of_range are ACCUMULATED INTO, never cleared: a metric keeps its state on the
 *                         device across calls.  All integer: bit-identical from run to run, and two calls equal one
 *                         call on the concatenation.  n_pixels < 2^31.  C <= 1024 and G <= 4096, else
 *                         WM2F_EUNSUPPORTED.  Bins live in LDS per workgroup (int32, 16 KiB at the bound: eight
 *                         workgroups per CU) while C <= 64, non-zero ones flushed with 64-bit adds; above that every
 *                         add goes to conf directly.  Four pixels per lane and load when n_pixels % 4 == 0 and both
 *                         maps are aligned to four elements (16 bytes for int64), pixel by pixel otherwise, with the
 *                         same results. */
int wm2f_panoptic_match(const int32_t* hist, const int32_t* pred_label, const int32_t* gt_label, const int32_t* n_pred,
                        const int32_t* n_gt, int32_t* gt_match, double* gt_iou, uint8_t* pred_state, int B, int P, int G,
                        int void_as_background, void* stream);
int wm2f_semantic_confusion(const void* pred, int pred_dtype, const void* gt, int gt_dtype, const int32_t* gt_ids,
                            const int32_t* gt_cls, const int32_t* n_ids, int64_t* conf, int64_t* n_out_of_range, int B,
                            int64_t n_pixels, int G, int C, int ignore_index, int background_label, void* stream);

/* ---- segmentation overlays and contours on device ----------------------------------------
 * What models/model_utils.py::plot_segmentation and the dataset visualisers draw with one `segmentation == id` pass
 * per segment on the host: every listed segment filled at its alpha and outlined at full colour, in one read of the
 * picture and the map whatever the number of segments.
 * wm2f_labelmap_overlay:   image and out (B, H, W, 3) uint8; out is overwritten and must not overlap image (neighbours
 *                         are read), else WM2F_EINVAL.  map (B, H, W) is WM2F_F32, WM2F_I32 or WM2F_U8; a float value
 *                         is an id by the rule of wm2f_labelmap_instance_stats (negative, fractional, not finite or
 *                         >= 2^24: no id).  ids (B, N) int32, ascending, n_ids (B) int32 of them valid per image;
 *                         rgba (B, N, 4) uint8 (4-byte aligned) and order (B, N) int32 belong to the listed entry.
 *                         N == 0 is legal (the four pointers may then be NULL): every pixel takes the default.
 *                         default_rgba = r | g << 8 | b << 16 | a << 24, for every pixel whose value is not listed.
 *                         0 <= inner, outer <= 4, else WM2F_EINVAL.
 *                         Write e(p) for the listed entry of pixel p's value, or none.  Distances are |dx| + |dy|;
 *                         pixels outside the picture are no neighbours.
 *                         Fill: (r, g, b, a) = rgba[e(p)], or the default when e(p) is none;
 *                           out_c = (image_c * (255 - a) + col_c * a + 127) / 255 in integers
 *                         (a == 0 copies the picture's byte, a == 255 gives the colour).
 *                         Contour, opaque, over the fill: the candidates of p are
 *                           - e(p), if some q within `inner` has e(q) != e(p),
 *                           - e(q) for every q within `outer` with e(q) != e(p),
 *                         none and entries of negative order left out; p takes the rgb of the candidate of greatest
 *                         order (painter's order; of equal orders the later entry wins), and its fill when there is no
 *                         candidate.  So entry s outlines itself `inner` pixels inwards and `outer` pixels outwards,
 *                         never along the picture's border, and inner == outer == 0 draws no contour.
 *                         All integer and nothing accumulated: bit-identical from run to run.
 *                         H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED.
 *                         A workgroup owns a tile of 32 x 128 pixels; the entries of the tile and its halo live in LDS
 *                         as int16 (11 KiB).  e(p) is a binary search of the image's id list, which with order and
 *                         rgba lives in LDS while N <= 1024 (12 B per entry) and is read from global memory above
 *                         that.  Four pixels per lane and load when W % 4 == 0 and image, out (4-byte) and map
 *                         (16-byte, uint8: 4-byte) are aligned, pixel by pixel otherwise, with the same results. */
int wm2f_labelmap_overlay(const uint8_t* image, const void* map, int dtype, const int32_t* ids, const int32_t* n_ids,
                          const uint8_t* rgba, const int32_t* order, uint32_t default_rgba, int inner, int outer,
                          uint8_t* out, int B, int H, int W, int N, void* stream);

/* ---- image preprocessing on device ---------------------------------------------------
 * The tensor work of Mask2FormerImageProcessorPil._preprocess (image_processing_pil_mask2former.py:485-585), bit-exact.
 * wm2f_resize_normalize_u8: B packed uint8 HWC RGB images of different sizes -> pixel_values (B, 3, Hp, Wp) float32 and
 *     pixel_mask (B, Hp, Wp) int64.  Per image, Pillow's 8-bit bilinear resample: a horizontal pass into the uint8 (H, w, 3)
 *     intermediate in `workspace`, then a vertical pass; each output = clip8((2^21 + sum coef * u8) >> 22).  Then
 *     lut (3, 256) float32 maps (channel, byte) to the rescaled, normalised value.  Outside the (h, w) image:
 *     pixel_values 0, pixel_mask 0; inside: pixel_mask 1.
 *       desc   HOST int64 (B, WM2F_PRE_DESC_LEN): in_off (bytes into images), ws_off (bytes into workspace), H, W, h, w,
 *              tx, cx, kx, ty, cy, ky.
 *       tables (n_table) int32: at tx, w pairs (xmin, count) of the columns; at cx, w * kx fixed-point coefficients (22
 *              fraction bits); ty / cy / ky the same for the h rows.  An unchanged side takes an identity table
 *              (xmin = i, count 1, coefficient 2^22).
 *     The horizontal pass reads every input row.  B <= WM2F_PRE_MAX_IMAGES and every side <= WM2F_PRE_MAX_SIDE, else
 *     WM2F_EUNSUPPORTED.
 * wm2f_resize_nearest_labels: B packed id maps (WM2F_U8 or WM2F_I32, n_map_elems elements) -> out (B, Hp, Wp) int32,
 *     out[y][x] = map[yi[y]][xi[x]] inside the (h, w) image, ignore_index outside; present (B, 256) uint8 is cleared on
 *     the stream and then flags every id value 0..255 that occurs inside the image.
 *       desc   HOST int64 (B, WM2F_LAB_DESC_LEN): in_off (elements), H, W, h, w, xi, yi (offsets of the w column and h
 *              row source indices in tables). */
#define WM2F_PRE_MAX_IMAGES 32
#define WM2F_PRE_MAX_SIDE 16384
#define WM2F_PRE_DESC_LEN 12
#define WM2F_LAB_DESC_LEN 7
int wm2f_resize_normalize_u8(const uint8_t* images, int64_t images_bytes, const int64_t* desc, const int32_t* tables,
                             int64_t n_table, const float* lut, uint8_t* workspace, int64_t workspace_bytes,
                             float* pixel_values, int64_t* pixel_mask, int B, int Hp, int Wp, void* stream);
int wm2f_resize_nearest_labels(const void* maps, int dtype, int64_t n_map_elems, const int64_t* desc,
                               const int32_t* tables, int64_t n_table, int32_t* out, uint8_t* present, int B, int Hp,
                               int Wp, int ignore_index, void* stream);

/* ---- training augmentation on device: flip, resize, crop --------------------------------
 * Per image, explicit parameters flip in {0, 1}, the resized size (h, w), the window origin (y0, x0) and the window size
 * (ch, cw) with y0 + ch <= h, x0 + cw <= w and (ch, cw) <= (Hp, Wp).  The result is, bit for bit, what Pillow makes of
 * image.transpose(FLIP_LEFT_RIGHT).resize((w, h)).crop((x0, y0, x0 + cw, y0 + ch)), then the processor's lookup / padding:
 *   1. the flip is applied to the SOURCE, before the resize: column c of the flipped image is column W - 1 - c of the
 *      stored one, and the tap tables are those of (W -> w) applied to the mirrored image.  The output is never mirrored
 *      instead (Pillow's nearest index table is not mirror-symmetric);
 *   2. the resize is the one of wm2f_resize_normalize_u8 / wm2f_resize_nearest_labels, of the whole flipped frame;
 *   3. the window's pixels are exactly that frame's pixels at rows y0 .. y0 + ch - 1, columns x0 .. x0 + cw - 1.  The
 *      (h, w) frame is virtual: only the window is computed, and nothing of size h or w is stored;
 *   4. lut (3, 256) maps (channel, byte) to the rescaled, normalised value;
 *   5. below and right of the window up to (Hp, Wp): pixel_values 0, pixel_mask 0, maps ignore_index;
 *   6. present flags the id values inside the window only.
 * With flip 0, origin (0, 0) and window (h, w) the outputs equal those of the two calls above.
 * The tap and index tables are handed over WHOLE, built for the full (H -> h), (W -> w) resize exactly as for the calls
 * above; the kernels index them at y0 + y and x0 + x.
 * wm2f_augment_resize_normalize_u8: one launch and no workspace.  A workgroup owns a 16 x 128 output tile, runs the
 *     horizontal pass for the tile's columns over the source rows its vertical taps reach (64 rows at a time, uint8 in
 *     LDS, clipped as the workspace bytes of wm2f_resize_normalize_u8 are) and sums the vertical taps in registers; a
 *     downscale of any ratio takes more 64-row rounds, never a second launch.
 *       desc   HOST int64 (B, WM2F_AUG_PRE_DESC_LEN): in_off (bytes into images), H, W, h, w, tx, cx, kx, ty, cy, ky,
 *              flip, y0, x0, ch, cw.
 * wm2f_augment_nearest_labels: out (B, Hp, Wp) int32, out[y][x] = map[yi[y0 + y]][mirror(xi[x0 + x])] inside the window.
 *       desc   HOST int64 (B, WM2F_AUG_LAB_DESC_LEN): in_off (elements), H, W, h, w, xi, yi, flip, y0, x0, ch, cw.
 * Bounds: B <= WM2F_PRE_MAX_IMAGES; H, W, Hp, Wp <= WM2F_PRE_MAX_SIDE; the virtual h, w <= WM2F_AUG_MAX_VIRTUAL; else
 * WM2F_EUNSUPPORTED.  A window outside its frame or larger than (Hp, Wp) is WM2F_EINVAL. */
#define WM2F_AUG_MAX_VIRTUAL 65536
#define WM2F_AUG_PRE_DESC_LEN 16
#define WM2F_AUG_LAB_DESC_LEN 12
int wm2f_augment_resize_normalize_u8(const uint8_t* images, int64_t images_bytes, const int64_t* desc,
                                     const int32_t* tables, int64_t n_table, const float* lut, float* pixel_values,
                                     int64_t* pixel_mask, int B, int Hp, int Wp, void* stream);
int wm2f_augment_nearest_labels(const void* maps, int dtype, int64_t n_map_elems, const int64_t* desc,
                                const int32_t* tables, int64_t n_table, int32_t* out, uint8_t* present, int B, int Hp,
                                int Wp, int ignore_index, void* stream);

/* ---- colour jitter on device: brightness, contrast, saturation, hue ----------------------
 * Four operations on uint8 RGB images, each defined by a Pillow 12.2 expression and reproduced byte for byte:
 *   WM2F_PHOTO_BRIGHTNESS  factor f >= 0   ImageEnhance.Brightness(im).enhance(f)
 *   WM2F_PHOTO_CONTRAST    factor f >= 0   ImageEnhance.Contrast(im).enhance(f)
 *   WM2F_PHOTO_SATURATION  factor f >= 0   ImageEnhance.Color(im).enhance(f)
 *   WM2F_PHOTO_HUE         dh in 0 .. 255  h, s, v = im.convert("HSV").split(); h = (h + dh) mod 256;
 *                                          Image.merge("HSV", (h, s, v)).convert("RGB")
 * A chain is an ordered list of at most four operations, each kind at most once, applied left to right; each operation
 * produces a uint8 image that the next one reads.
 * Blend.  The three enhancers are Image.blend(degenerate, image, f).  Per byte, with d the degenerate byte, v the image
 *   byte and a = float32(f): t = fl32(fl32(d) + fl32(a * fl32(v - d))) -- the product is rounded to float32, then the
 *   sum; NOT a fused multiply-add -- and the result is 0 if t <= 0, 255 if t >= 255, else trunc(t).  (Pillow skips the
 *   clip for 0 <= f <= 1, where t lies in range already.)
 * Degenerates.  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of a pixel.
 *   brightness: d = 0.  saturation: d = L of the same pixel.
 *   contrast: d = m for every byte of the image, m = int(S / (H W) + 0.5) with S the integer sum of L over the image AS IT
 *   STANDS WHEN THE CONTRAST STEP IS REACHED (after the steps in front of it), the division and the sum in float64.
 * RGB -> HSV.  mx, mn the largest and smallest of the three bytes; V = mx.  mx == mn: H = S = 0.  Otherwise, in float32
 *   unless said: cr = mx - mn; s = cr / mx; rc = (mx - r) / cr, gc, bc alike; h = bc - gc if r == mx, else
 *   2.0 + rc - bc if g == mx, else 4.0 + gc - rc, the two forms with a constant evaluated left to right in float64 and
 *   then stored to float32; h = float32(fmod(float64(h) / 6.0 + 1.0, 1.0)) (the operand lies in [5/6, 11/6), so
 *   x >= 1 ? x - 1 : x is exact); H = clip8(int(float64(h) * 255.0)), S = clip8(int(float64(s) * 255.0)).
 * HSV -> RGB.  S == 0: all three bytes are V.  Otherwise hf = float64(float32(H)) * 6.0 / 255.0; i = floor(hf);
 *   f = float32(hf - i); fs = float32(float64(S) / 255.0); p = round(V (1 - fs)), q = round(V (1 - fs f)),
 *   t = round(V (1 - fs (1 - f))) in float64 -- except the product fs f, which is a float32 product -- with C round (half
 *   away from zero), clipped to a byte; (R, G, B) by i mod 6 = (V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V),
 *   (V, p, q).  A hue step with dh = 0 still goes through both conversions and changes pixels, as Pillow does.
 * wm2f_photometric_u8 works IN PLACE on B packed HWC uint8 images.
 *       desc       HOST int64 (B, WM2F_PHOTO_DESC_LEN): in_off (bytes into images), H, W, n_ops, then four (kind,
 *                  parameter) pairs; the parameter is the bit pattern of the float32 factor (0 .. 2^32 - 1), or dh for
 *                  WM2F_PHOTO_HUE.  Pairs from n_ops on are ignored.  An image with n_ops = 0 is left untouched.
 *       workspace  wm2f_photometric_workspace(B) bytes (-1 for a bad B), 8-byte aligned: B int64 sums of L, cleared on
 *                  the stream inside the call.
 *   Two launches at most and no host synchronisation.  The sum launch runs only when some chain holds a contrast step and
 *   its grid covers only those images: it applies the steps in front of the contrast step per pixel in registers and adds
 *   L up as integers (wave reduction, one 64-bit atomic add per workgroup), so S does not depend on the schedule.  The
 *   apply launch covers the images with n_ops > 0, runs the whole chain per pixel in registers, forms m in float64 and
 *   writes the bytes back.  Images start at any byte: the pixels in front of the first 4-byte boundary that is also a
 *   pixel boundary, and those behind the last whole group of four, go byte by byte; the body goes 12 bytes per thread.
 * Bounds: B <= WM2F_PRE_MAX_IMAGES and sides <= WM2F_PRE_MAX_SIDE, else WM2F_EUNSUPPORTED.  WM2F_EINVAL: a repeated or
 * unknown kind, n_ops outside 0 .. 4, a negative or non-finite factor, dh outside 0 .. 255, an image that leaves
 * images_bytes. */
#define WM2F_PHOTO_BRIGHTNESS 0
#define WM2F_PHOTO_CONTRAST 1
#define WM2F_PHOTO_SATURATION 2
#define WM2F_PHOTO_HUE 3
#define WM2F_PHOTO_DESC_LEN 12
int64_t wm2f_photometric_workspace(int B);
int wm2f_photometric_u8(uint8_t* images, int64_t images_bytes, const int64_t* desc, void* workspace, int B, void* stream);

/* ---- orientation on device: vertical flip, quarter turns, rotation ------------------------
 * Per image, with im the stored RGB image (or id map) of size (H, W), the output is byte for byte what Pillow 12.2 makes
 * of these steps, each taken only when enabled, in this order:
 *   1. vflip = 1:      im.transpose(FLIP_TOP_BOTTOM): row y is stored row H - 1 - y.
 *   2. turns = 1, 2, 3: im.transpose(ROTATE_90 / ROTATE_180 / ROTATE_270), counter-clockwise.  With (H, W) the size in
 *      front of the turn: 1: out[y][x] = in[x][W - 1 - y]; 2: out[y][x] = in[H - 1 - y][W - 1 - x];
 *      3: out[y][x] = in[H - 1 - x][y].  Turns 1 and 3 make the frame (W, H).
 *   3. affine = 1:     image  im.rotate(angle, resample=BILINEAR, expand=False, fillcolor=fill),
 *                      map    im.rotate(angle, resample=NEAREST, expand=False, fillcolor=fill).
 *      The frame keeps its size.  Below, (H, W) is the size of the turned frame the rotation reads.
 * Matrix.  Computed on the host in Python floats exactly as Image.rotate does: a = -radians(angle % 360.0);
 *   m = [round(cos a, 15), round(sin a, 15), 0, round(-sin a, 15), round(cos a, 15), 0]; with cx = W / 2.0, cy = H / 2.0:
 *   m2 = m0 (-cx) + m1 (-cy), m5 = m3 (-cx) + m4 (-cy), then m2 += cx, m5 += cy.  The six float64 values travel as bit
 *   patterns.  Pillow routes angle % 360 of 0 and 180, and of 90 and 270 on a square image, to transpose: the host folds
 *   those into `turns` and leaves affine = 0.
 * Image, bilinear.  All arithmetic is float64, every product rounded before its sum (nothing fused).  For output pixel
 *   (x, y): xi = x + 0.5, yi = y + 0.5; xin = m0 xi + m1 yi + m2, yin = m3 xi + m4 yi + m5 (left to right).  The pixel is
 *   `fill` when xin < 0, xin >= W, yin < 0 or yin >= H.  Otherwise xin -= 0.5, yin -= 0.5; X = floor(xin), Y = floor(yin);
 *   dx = xin - X, dy = yin - Y.  Columns X and X + 1 are clamped to [0, W - 1], row Y to [0, H - 1].  Per channel, with a, b
 *   the bytes at the two columns: v1 = a + (b - a) dx on row Y; v2 the same on row Y + 1 when 0 <= Y + 1 < H, else
 *   v2 = v1; v = v1 + (v2 - v1) dy; the byte is v truncated.
 * Map, nearest.  Pillow's 16.16 fixed point, FIX(v) = floor(v 65536.0 + 0.5) as host integers: a0, a1, a3, a4 = FIX(m0),
 *   FIX(m1), FIX(m3), FIX(m4); a2 = FIX(m2 + m0 0.5 + m1 0.5), a5 = FIX(m5 + m3 0.5 + m4 0.5).  Source column
 *   (a2 + a1 y + a0 x) >> 16 and row (a5 + a4 y + a3 x) >> 16 (arithmetic shift, 64-bit in the kernel; with sides
 *   <= 16384 the values stay inside int32, so Pillow's 32-bit accumulators never wrap); `fill` when either index is
 *   outside the frame.
 * wm2f_orient_u8: packed HWC uint8 images, out of place; offsets and buffer sizes in bytes.
 * wm2f_orient_labels_u8 / _i32: id maps, one templated kernel; offsets and buffer sizes in elements.
 *       desc   HOST int64 (B, WM2F_ORIENT_DESC_LEN): in_off, H, W (the stored size), out_off, vflip, turns, affine, the six
 *              float64 bit patterns m0 .. m5, the six fixed-point integers a0 .. a5, then the fill: three bytes r, g, b
 *              (images) or the id and two ignored entries (maps).  The output of an image holds H W pixels, as a
 *              (W, H) frame when turns is odd.  An image with nothing enabled is copied.
 *   One launch for the whole batch, no workspace and no host synchronisation.  A workgroup owns a 64 x 64 output tile and
 *   builds it in LDS: flips and turns read the tile's footprint in contiguous runs and transpose it in LDS; the rotation
 *   computes the coordinates once per pixel and takes the three channels from the same four taps, with the flip and the
 *   turn folded into the tap address.  Rows go out as contiguous runs.  Runs are moved as aligned dwords and, at their two
 *   ends, byte by byte; no byte outside an image is read or written.
 * Bounds: B <= WM2F_PRE_MAX_IMAGES and sides <= WM2F_PRE_MAX_SIDE, else WM2F_EUNSUPPORTED.  WM2F_EINVAL: an image that
 * leaves the input or the output buffer, overlapping outputs, overlapping src and dst, vflip or affine outside {0, 1},
 * turns outside 0 .. 3, with affine = 1 a non-finite matrix entry (images) or a fixed-point term outside int32 (maps), a
 * fill byte outside 0 .. 255 or a fill id that does not fit the map's type. */
#define WM2F_ORIENT_DESC_LEN 22
int wm2f_orient_u8(const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, const int64_t* desc, int B,
                   void* stream);
int wm2f_orient_labels_u8(const uint8_t* src, int64_t src_elems, uint8_t* dst, int64_t dst_elems, const int64_t* desc,
                          int B, void* stream);
int wm2f_orient_labels_i32(const int32_t* src, int64_t src_elems, int32_t* dst, int64_t dst_elems, const int64_t* desc,
                           int B, void* stream);

/* ---- Simple Copy-Paste on device ------------------------------------------------------------
 * Instances of one image of a batch are cut out and pasted, shifted by whole pixels, onto another image of the same
 * batch (Ghiasi et al., CVPR 2021); nothing is blended.  pixels (B, C, H, W) float32, maps (B, H, W) int32.  A map value
 * in 0 .. 254 is an instance id; every other value (255, negative, above 255) is no instance: copied through, never
 * pasted, never counted.  All calls are out of place with respect to the batch: every image may be a source and a
 * destination in one call.
 *       desc   HOST int64 (B, WM2F_COPY_PASTE_DESC_LEN): source (-1: none, else another image of the batch), dy, dx,
 *              h, w (the destination's valid window, 0 <= h <= H, 0 <= w <= W).
 *       lut    DEVICE int32 (B, 256): lut[b][source id] = the id it is pasted as in image b (0 .. 254), or -1.  Entry 255
 *              and values outside 0 .. 254 count as -1; an image without source has no live entry.
 *       areas  DEVICE int32 (B, 3, 256): row 0 `before`, row 1 `after` (indexed by the id in the result), row 2
 *              `original` (indexed by the source id).
 * Paste rule.  Destination pixel (y, x) of image b takes source pixel (y - dy, x - dx) of image s = source when that
 * position lies inside the (H, W) frame, its id i has lut[b][i] >= 0, and y < h, x < w.  Then all C values are copied as
 * bit patterns and the map takes lut[b][i]; everywhere else the destination is copied.
 * min_visible = num / den (0 <= num <= den <= 1024); every comparison is int64.
 *   wm2f_copy_paste_select (step A, maps only): for every id i with lut_in[b][i] >= 0, original = its area in the whole
 *     source frame, landed = the number of its pixels (ys, xs) with ys + dy < h, xs + dx < w (and both >= 0).
 *     lut_out[b][i] = lut_in[b][i] when landed > 0 and landed den >= num original, else -1.  Writes row 2 of `areas`
 *     (0 for ids that were not selected).  `workspace`: B * 256 int32, cleared by the call.
 *   wm2f_copy_paste (step B): the paste with `lut` as it is.  before[b][i] = the number of pixels of the destination map
 *     equal to i, after[b][i] the same in the pasted map (i in 0 .. 254); writes rows 0 and 1 of `areas`.
 *   wm2f_copy_paste_prune (step C, maps only, in place on the pasted maps): every id with after > 0 and
 *     after den < num before is repainted to ignore_index (which must not be an id).  With num = 0 nothing is launched.
 * The destination's map and pixels are read once and written once; the source map is read where a source pixel can
 * arrive and the source pixels only where something is pasted; 16-byte accesses when W % 4 == 0 and the pointers are
 * 16-byte aligned (the source side when dx % 4 == 0 as well), one pixel per thread otherwise.  LUT and histograms live in
 * LDS and are flushed with integer atomics: the counts are exact and the same from run to run.  No call allocates,
 * keeps state or synchronises with the host.
 * Bounds: B <= 65535, sides <= WM2F_PRE_MAX_SIDE, else WM2F_EUNSUPPORTED.  WM2F_EINVAL: a source outside -1 .. B - 1 or
 * equal to its destination, a shift beyond +-65536, a window outside the frame, a bad fraction, in-place buffers. */
#define WM2F_COPY_PASTE_DESC_LEN 5
int wm2f_copy_paste_select(const int32_t* maps, const int32_t* lut_in, int32_t* lut_out, int32_t* areas, int32_t* workspace,
                           const int64_t* desc, int B, int H, int W, int64_t num, int64_t den, void* stream);
int wm2f_copy_paste(const float* pixels_in, const int32_t* maps_in, const int32_t* lut, float* pixels_out, int32_t* maps_out,
                    int32_t* areas, const int64_t* desc, int B, int C, int H, int W, void* stream);
int wm2f_copy_paste_prune(int32_t* maps, const int32_t* areas, int B, int H, int W, int64_t num, int64_t den,
                          int ignore_index, void* stream);

/* ---- connected components of class maps ------------------------------------------------
 * The cv2 steps of the reference's dataset loaders (datasets/pheno_bench/dataset.py:48-135, crop_weed
 * dataset_from_png_annotations.py:48-131): cv2.resize(INTER_NEAREST) of the mask, cv2.connectedComponents per class,
 * the instance map painted with ids 1, 2, ... in (class, component) order.
 * Two pixels join when they are 8-neighbours with the same nonzero class.  Components are numbered the way OpenCV's
 * block-based 8-connectivity labelling numbers them: by (class, first 2x2 block), where the first block of a component
 * is the minimum of (r >> 1) * ceil(W / 2) + (c >> 1) over its pixels.  The result does not depend on the schedule.
 * workspace: wm2f_ccl_workspace(H, W) bytes (-1 for a bad size): parent, class, slot, root list, each (H, W) int32,
 *     and a counter.
 * wm2f_ccl_label: class map of the (H, W) output: pixel (y, x) reads source pixel (ty[y], tx[x]) of the (src_H, src_W)
 *     map (ty / tx int32 device tables, clamped; both null = identity, then the sizes must agree) and maps it by mode:
 *       WM2F_CCL_VALUE   the value itself (src_dtype WM2F_U8, WM2F_U16 or WM2F_I32), 0 = background;
 *       WM2F_CCL_BINARY  1 where the value is nonzero;
 *       WM2F_CCL_RGB     (src_H, src_W, 3) uint8: 1 + the index of the first of the n_colors HOST rgb triples in
 *                        `colors` that equals the pixel, 0 if none (n_colors <= WM2F_CCL_MAX_COLORS).
 *     Then labels the components; count (1 int32) receives their number n (cleared on the stream first).
 * wm2f_ccl_keys: keys (n) int64 = class * 2^32 + first block of each component, in the workspace's root-list order;
 *     the keys are distinct.  The caller sorts them (ascending) into `order` (n int64 indices into that list).
 * wm2f_ccl_paint: the component at sorted position i gets id i + 1 (i + 2 from id 255 on when skip_255) and
 *     out (H, W) int32 = its id, `background` outside every component; comp_class (n) int32, if not null, = the class
 *     of the component at sorted position i.
 * wm2f_resize_nearest: dst (H, W) = src (src_H, src_W) pixels of elem_bytes (1, 2, 3 or 4) bytes at (ty[y], tx[x]). */
#define WM2F_CCL_VALUE 0
#define WM2F_CCL_BINARY 1
#define WM2F_CCL_RGB 2
#define WM2F_CCL_MAX_COLORS 16
int64_t wm2f_ccl_workspace(int H, int W);
int wm2f_ccl_label(const void* src, int mode, int src_dtype, int src_H, int src_W, const int32_t* ty, const int32_t* tx,
                   const uint8_t* colors, int n_colors, int H, int W, void* workspace, int32_t* count, void* stream);
int wm2f_ccl_keys(const void* workspace, int n, int H, int W, int64_t* keys, void* stream);
int wm2f_ccl_paint(void* workspace, const int64_t* order, int n, int H, int W, int skip_255, int background, int32_t* out,
                   int32_t* comp_class, void* stream);
int wm2f_resize_nearest(const void* src, int elem_bytes, int src_H, int src_W, const int32_t* ty, const int32_t* tx,
                        void* dst, int H, int W, void* stream);

/* ---- polygon rasterisation ------------------------------------------------------------------
 * cv2.fillPoly(img, pts, color) with the reference's arguments (int32 image, LINE_8, shift 0, no offset), for a
 * chain of calls painted in order: call k paints value values[k] over the union of its outline (8-connected
 * LineIterator lines, clipLine-clipped) and its scan fill (FillEdgeCollection: crossings of the active edges, sorted
 * and paired), all contours of one call sharing one edge table (even-odd).  A later call overwrites an earlier one;
 * pixels no call covers keep their value.  The result does not depend on the schedule.
 * Inputs are DEVICE int32 arrays:
 *   verts (n_verts, 2) x, y with |x|, |y| <= WM2F_POLY_MAX_COORD;
 *   contour_offsets (n_contours + 1): contour c is verts[contour_offsets[c] .. contour_offsets[c + 1]), non-empty,
 *     contour_offsets[0] = 0 and contour_offsets[n_contours] = n_verts;
 *   call_offsets (n_calls + 1): call k is contours [call_offsets[k], call_offsets[k + 1]), non-decreasing from 0 to
 *     n_contours;  values (n_calls);
 *   call_row0 (n_calls), item_offsets (n_calls + 1): the rows the scan fill visits, call k rows call_row0[k] ..
 *     call_row0[k] + item_offsets[k + 1] - item_offsets[k] - 1, each inside [0, H); item_offsets[0] = 0 and
 *     item_offsets[n_calls] = n_items.  Any range that holds every row where a vertex y0 <= row < vertex y1 of the
 *     call is correct (ops.fill_polygons uses [max(0, min y), min(H, max y) - 1]).
 * out (H, W) int32, painted in place.  workspace: wm2f_poly_workspace(H, W, n_verts) bytes (-1 for a bad size):
 * one 24-byte edge record per vertex and an (H, W) int32 rank map. */
#define WM2F_POLY_MAX_SIDE 16384
#define WM2F_POLY_MAX_COORD (1 << 24)
int64_t wm2f_poly_workspace(int H, int W, int n_verts);
int wm2f_poly_fill(int32_t* out, int H, int W, const int32_t* verts, int n_verts, const int32_t* contour_offsets,
                   int n_contours, const int32_t* call_offsets, const int32_t* values, const int32_t* call_row0,
                   const int32_t* item_offsets, int n_calls, int n_items, void* workspace, void* stream);

/* ---- run-length encoding and decoding of id maps -------------------------------------------
 * Scan order: `order` 0 flattens a (H, W) map row-major, v[y * W + x]; 1 column-major, v[x * H + y] (COCO's).
 * Slots: map (B, H, W) is WM2F_F32 (-1.0 background, otherwise an id by the rule of wm2f_labelmap_instance_stats),
 * WM2F_I32 or WM2F_U8; ids lie in [-1, N); slot 0 is id -1 and slot k + 1 is id k.  N <= WM2F_RLE_MAX_IDS.
 * Toggles: slot k toggles at position t of the flattened image v[0 .. HW) when
 *   - 0 < t < HW and exactly one of v[t - 1], v[t] has slot k, or
 *   - t == 0 and v[0] has slot k, or
 *   - t == HW and v[HW - 1] has slot k.
 * A slot's toggle list is every such t, ascending; its length is even; runs cross line ends (the first pixel of a line
 * is compared with the last pixel of the line before).  The runs of slot k are [t_0, t_1), [t_2, t_3), ...
 * wm2f_labelmap_toggle_counts: counts (B, N + 1) int32 <- the length of every slot's toggle list;
 *                         out_of_range (B) int32 <- the pixels whose value is outside [-1, N).  Such a pixel belongs to
 *                         no slot (its neighbours still toggle against it); a caller treats a non-zero word as an error.
 *                         workspace: wm2f_rle_workspace(B, H, W, N, order) bytes (-1 for a bad size), which the call
 *                         fills with the per-group prefixes the write launch needs: it must reach
 *                         wm2f_labelmap_toggles unchanged, with the same map and arguments.
 * wm2f_labelmap_toggles:   offsets (B * (N + 1) + 1) int32 DEVICE = the exclusive prefix sums of counts, image-major
 *                         then slot (CSR), the total last (< 2^31); positions (total) int32 <- every slot's toggle
 *                         list at offsets[b * (N + 1) + slot].  Every place is computed from the counts: no float and
 *                         no atomic takes part, and the result is bit-identical from run to run.  A position is stored
 *                         only inside its slot's range, whatever offsets and workspace hold.  Consumes the workspace.
 * Both read the map once, whatever N is.  Row-major: one wave per group of whole rows, 64 positions per step, ranks
 * by ballot and popcount per distinct slot of the step, cursors in LDS (4 B per slot).  Column-major: one lane per
 * column, a wave reading 64 adjacent pixels of a row per load; the workspace holds 4 B per (column, slot).
 * wm2f_rle_paint:          runs (R, 4) int32 DEVICE: (image, start, length, value), positions in scan order `order`;
 *                         out (B, H, W) int32, painted in place: value over [start, start + length), a later run over
 *                         an earlier one (painter's order, whatever the schedule); pixels no run covers keep their
 *                         value.  status (1) int32 DEVICE <- INT32_MAX, or the index of the first run with image
 *                         outside [0, B), start < 0, length < 0 or start + length > HW: then the WHOLE call is
 *                         refused and nothing is painted (a run is never clipped).  The call does not wait for the
 *                         device; the caller reads status.  workspace: wm2f_rle_paint_workspace(B, H, W) bytes, a rank
 *                         map.
 * H, W <= 16384, B <= 32, else WM2F_EUNSUPPORTED. */
#define WM2F_RLE_MAX_IDS 1024
int64_t wm2f_rle_workspace(int B, int H, int W, int N, int order);
int wm2f_labelmap_toggle_counts(const void* map, int dtype, int32_t* counts, int32_t* out_of_range, void* workspace,
                                int B, int H, int W, int N, int order, void* stream);
int wm2f_labelmap_toggles(const void* map, int dtype, const int32_t* offsets, int32_t* positions, void* workspace, int B,
                          int H, int W, int N, int order, void* stream);
int64_t wm2f_rle_paint_workspace(int B, int H, int W);
int wm2f_rle_paint(int32_t* out, const int32_t* runs, int R, int32_t* status, void* workspace, int B, int H, int W,
                   int order, void* stream);

/* ---- tracing id maps into polygons ---------------------------------------------------------
 * The inverse of wm2f_poly_fill.  map (B, H, W) is WM2F_F32 (-1.0 background), WM2F_I32 or WM2F_U8 as above; ids lie in
 * [-1, N), N <= WM2F_RLE_MAX_IDS; id -1 is never traced.  4 * B * H * W < 2^31 and B <= 4096, else WM2F_EUNSUPPORTED.
 * Edges: a side of a pixel (y, x) with id k >= 0 is a boundary side when the pixel across it has another value or lies
 *   outside the map.  Sides: 0 top, 1 right, 2 bottom, 3 left.  A boundary side is a directed unit edge on the corner
 *   lattice (x in [0, W], y in [0, H], y down): top (x, y) -> (x + 1, y), right (x + 1, y) -> (x + 1, y + 1), bottom
 *   (x + 1, y + 1) -> (x, y + 1), left (x, y + 1) -> (x, y); the segment lies on the right of the heading, so outer loops
 *   run clockwise on screen.  The key of an edge is 4 * (y * W + x) + side; edges are numbered by (image, key).
 * Successor: at the head vertex of an edge of heading d, with L the pixel ahead-left and R the pixel ahead-right: L has
 *   id k -> turn left (side (d + 3) % 4 of L); else R has id k -> straight (side d of R); else turn right (side
 *   (d + 1) % 4 of the edge's own pixel).  Left first makes a segment 8-connected at a saddle vertex.  Every edge has one
 *   successor and one predecessor: the edges of an id are disjoint closed loops.
 * Loops: a loop's leader is its edge of lowest key, rank 0; ranks grow along successors.  Loops are ordered by image, then
 *   id, then leader key.
 * Points, coords 0 (crack): an edge emits its tail vertex -- always, or with simplify only when its heading differs from
 *   its predecessor's.  Exact: the even-odd interior of an id's loops at pixel centres is the id's mask.
 * Points, coords 1 (pixel): an edge emits its own pixel (x, y) iff that pixel differs from its predecessor's pixel; a loop
 *   in which no edge does (round a single pixel) emits that pixel once, at its leader.  With simplify, a loop of more
 *   than two such points drops every point b whose cyclic neighbours a, c satisfy b - a == c - b.
 * A loop's point list starts at its emitting edge of lowest rank.
 * twice_area of a loop: the sum over its edges tail (xa, ya) -> head (xb, yb) of xa * yb - xb * ya; > 0 for an outer loop,
 *   < 0 for a hole, and an id's loops sum to twice its pixel count.
 * The chain (every array is DEVICE memory; no call waits for the device):
 * wm2f_trace_count:   counts (B + 1) int32 <- [E, the number of edges of the whole stack; then per image the pixels whose
 *                     value is outside [-1, N) (they are never traced; a caller treats a non-zero word as an error)].
 *                     workspace: wm2f_trace_workspace(B, H, W, N) bytes (-1 for a bad size): a word per pixel (the side
 *                     mask and the prefix of the edge count inside its block of 256 pixels) and a word per block.  It
 *                     must reach wm2f_trace_link unchanged, with the same map and arguments.
 * wm2f_trace_link:    E as read back from counts[0].  edge_workspace: wm2f_trace_edge_workspace(E) bytes, nine int32
 *                     arrays of E: key (4 * pixel index in the stack + side), next, prev, leader, rank, and four the
 *                     pointer jumping uses.  Fills key, next and prev.
 * wm2f_trace_rank:    leader and rank of every edge, by wm2f_trace_rounds(E) = max(1, ceil(log2 E)) launches of pointer
 *                     jumping along prev.
 * wm2f_trace_flags:   flag (E) int32 <- 1 where the edge emits a point under (coords, simplify); lead (E) int32 <- 1 at
 *                     leaders.  sum(lead) is the number of loops, sum(flag) of points.
 * wm2f_trace_loops:   lead_prefix (E) = the inclusive prefix sums of lead.  Loop j (leader order) stores
 *                     loop_key[j] = (image * N + id) << 32 | leader and loop_len[j] = its number of edges.
 * wm2f_trace_scatter: loop_place (n_loops): the place of loop j in (image, id, leader) order; loop_base (n_loops + 1): the
 *                     exclusive prefix sums of the lengths in that order.  Edge e goes to pos = loop_base[place] + rank:
 *                     flag_sorted[pos] <- flag[e], edge_sorted[pos] <- e, term_sorted[pos] <- its twice_area term.
 * wm2f_trace_emit:    flag_prefix (E) = the inclusive prefix sums of flag_sorted; points (P, 2) int32 (x, y) <- the point
 *                     of every flagged place at flag_prefix - 1.
 * No float and no atomic decides a place; every store is guarded by the range of its own array, whatever the tables
 * hold; the number of launches depends on the bit length of E alone. */
int64_t wm2f_trace_workspace(int B, int H, int W, int N);
int64_t wm2f_trace_edge_workspace(int64_t E);
int wm2f_trace_rounds(int64_t E);
int wm2f_trace_count(const void* map, int dtype, int32_t* counts, void* workspace, int B, int H, int W, int N,
                     void* stream);
int wm2f_trace_link(const void* map, int dtype, const void* workspace, void* edge_workspace, int E, int B, int H, int W,
                    int N, void* stream);
int wm2f_trace_rank(void* edge_workspace, int E, void* stream);
int wm2f_trace_flags(const void* edge_workspace, int32_t* flag, int32_t* lead, int E, int H, int W, int coords,
                     int simplify, void* stream);
int wm2f_trace_loops(const void* map, int dtype, const void* edge_workspace, const int32_t* lead_prefix,
                     int64_t* loop_key, int32_t* loop_len, int E, int n_loops, int B, int H, int W, int N, void* stream);
int wm2f_trace_scatter(const void* edge_workspace, const int32_t* flag, const int32_t* lead_prefix,
                       const int32_t* loop_place, const int32_t* loop_base, int32_t* flag_sorted, int32_t* edge_sorted,
                       int32_t* term_sorted, int E, int n_loops, int H, int W, void* stream);
int wm2f_trace_emit(const void* edge_workspace, const int32_t* flag_sorted, const int32_t* edge_sorted,
                    const int32_t* flag_prefix, int32_t* points, int E, int P, int H, int W, int coords, void* stream);

/* ---- merging the instances of overlapping tiles ---------------------------------------------
 * An image larger than the model's input is cut into T overlapping tiles of one size (th, tw); every tile is segmented
 * on its own; these calls decide which instances of neighbouring tiles are the same object, give them one id and write
 * one (H, W) id map.  tests/tile_merge_reference.py restates the contract in numpy.
 * Inputs (every array is DEVICE memory; no call waits for the device):
 *   tiles (T, th, tw): id maps, WM2F_F32 (-1.0 background: the post-processor's output) or WM2F_I32.  A value is an id
 *     by the rule of wm2f_labelmap_instance_stats (negative, fractional, not finite: no id; +-0 is id 0), and a value
 *     outside [0, n_ids[t]) is no id either.
 *   n_ids (T) int32, clamped to [0, N]; labels (T, N) int32.  Node g = t * N + i stands for instance i of tile t.
 *   geom (T, 6) int32: (oy, ox, cy0, cy1, cx0, cx1) -- the tile's origin in the image and its CELL, the half-open
 *     rectangle of output pixels it owns, in image coordinates.  The cells of a grid partition the image and each lies
 *     inside its tile (tiling.tile_windows: the cut between two neighbours is the midpoint of their overlap).
 *   pairs (P, 8) int32: (a, b, ay, ax, by, bx, h, w) -- tiles a < b whose windows intersect, and the intersection
 *     rectangle (h, w) at (ay, ax) of tile a and (by, bx) of tile b.
 * wm2f_tile_pair_counts:  hist (P, N+1, N+1) int32, overwritten: hist[p][i+1][j+1] = pixels of the rectangle with id i in
 *                         tile a and id j in tile b; row / column 0 is "no id" (the whole array is cleared first, 4 P (N+1)^2
 *                         bytes, and wm2f_tile_link reads it once).  area_a[i], the pixels of i inside the
 *                         rectangle, is a row sum; area_b[j] a column sum.  The tiles are read in place.  Bins live in
 *                         LDS while (N+1)^2 <= 16384 (N <= 127, 64 KiB) and are flushed once per workgroup; above that
 *                         every add is a global integer atomic.  A wave inside one id pair adds its lane count once; the
 *                         (none, none) bin is added once per workgroup.  Four pixels per lane when the rectangle's width
 *                         and tw are multiples of 4 and both row starts are 16-byte aligned, pixel by pixel otherwise,
 *                         with the same results.
 * wm2f_tile_owned_counts: owned (T, N) int32, overwritten: owned[t][i] = pixels of id i inside tile t's cell.
 * wm2f_tile_link:         LINK: i of tile a and j of tile b of pair p are the same object iff
 *                           inter = hist[p][i+1][j+1] > 0, labels[a][i] == labels[b][j] and
 *                           inter * den >= num * min(area_a[i], area_b[j])   (64-bit integers; equality links):
 *                         the intersection over the smaller of the two areas inside the overlap, so a view cut off by a
 *                         tile border still matches the whole view.  num >= 0, den >= 1.  Links are closed transitively
 *                         (union-find; the root of a set is its smallest node), so two instances of ONE tile may end
 *                         up in one set, joined through a neighbour.
 *                         NUMBERING: sets in which some node owns a pixel (owned > 0) are numbered 0, 1, ... in
 *                         ascending root order; remap (T, N) int32 <- the number of the node's set, -1 for a node of
 *                         a set that owns nothing and for i >= n_ids[t]; n_merged (1) int32 <- the number of sets.
 *                         workspace: wm2f_tile_merge_workspace(T, N, P) bytes (-1 for a bad size), no clearing needed.
 *                         Five launches (init, link, flatten + owner marks, numbering scan, remap): a phase that needs
 *                         every workgroup of the one before is its own launch.
 * wm2f_tile_compose:      out (H, W) int32, written once and inside the cells only (the cells must partition the image: a
 *                         pixel no cell covers is left as it was): pixel (y, x) of tile t's cell with local value v becomes
 *                         remap[t][v] when v is an id and -1 otherwise.  Inside every cell the output is the owner
 *                         tile's prediction, relabelled; an instance seen only where a neighbour owns the pixels, and
 *                         not linked, is not reported.  remap of the owner tile sits in LDS; four pixels per lane when
 *                         aligned as above.
 * All integer: no float and no float atomic takes part, every result is independent of the schedule and bit-identical
 * from run to run.  P == 0 (one tile, or no overlap) and N == 0 (out all -1) are legal.  Indices read from geom and pairs
 * are clipped to the arrays they address.  th, tw, H, W <= WM2F_TILE_MAX_SIDE, N <= WM2F_TILE_MAX_IDS,
 * T <= WM2F_TILE_MAX_TILES, P <= WM2F_TILE_MAX_PAIRS, else WM2F_EUNSUPPORTED. */
#define WM2F_TILE_MAX_SIDE 16384
#define WM2F_TILE_MAX_IDS 256
#define WM2F_TILE_MAX_TILES 1024
#define WM2F_TILE_MAX_PAIRS 16384
int64_t wm2f_tile_merge_workspace(int T, int N, int P);
int wm2f_tile_pair_counts(const void* tiles, int dtype, const int32_t* n_ids, const int32_t* pairs, int32_t* hist, int T,
                          int th, int tw, int N, int P, void* stream);
int wm2f_tile_owned_counts(const void* tiles, int dtype, const int32_t* n_ids, const int32_t* geom, int32_t* owned, int T,
                           int th, int tw, int N, void* stream);
int wm2f_tile_link(const int32_t* hist, const int32_t* pairs, const int32_t* labels, const int32_t* n_ids,
                   const int32_t* owned, int32_t* remap, int32_t* n_merged, void* workspace, int T, int N, int P, int num,
                   int den, void* stream);
int wm2f_tile_compose(const void* tiles, int dtype, const int32_t* n_ids, const int32_t* geom, const int32_t* remap,
                      int32_t* out, int T, int th, int tw, int N, int H, int W, void* stream);

/* ---- blending the class scores of overlapping tiles into one semantic map --------------------
 * The semantic counterpart of the merge above: tiles carry class SCORES, not ids, and where tiles overlap their scores
 * are blended under a feathering window before the argmax.  A view is one score grid per tile: the tiles as they are, or
 * the result computed on a flipped tile (test-time augmentation), which is read at the mirrored pixel.
 * tests/tile_blend_reference.py restates this contract in numpy, operation by operation.
 * Arguments (every array is DEVICE memory; the call does not wait for the device):
 *   scores (F, R * Cn, C, gh, gw) fp32: the (gh, gw) score grid of every class of every tile of every view; tiles are
 *     numbered row-major over R tile rows and Cn tile columns, all of size (th, tw).
 *   ys (R), xs (Cn) int32: the tile row / column origins in the image, ascending.
 *   flips (F) int32: bit 0 -- the view was computed on the horizontally flipped tile, bit 1 -- on the vertically flipped
 *     tile (other bits are ignored).
 *   seg (H, W) int32 and out_scores (C, H, W) fp32 or NULL, both 8-byte aligned, overwritten.
 * For output pixel (Y, X), in fp32 with every product, sum, difference and quotient below rounded on its own (no fused
 * multiply-add anywhere; the file is built with -ffp-contract=off):
 *   COVERING VIEWS  the covering rows are the r with ys[r] <= Y < ys[r] + th, the covering columns the c with
 *                   xs[c] <= X < xs[c] + tw; n = F * #rows * #columns.
 *   ORDER           views are visited with f ascending, then r ascending, then c ascending.
 *   WEIGHT          y = Y - ys[r], x = X - xs[c]; the integers wy = min(y + 1, th - y, ramp_y) and
 *                   wx = min(x + 1, tw - x, ramp_x); w = (float)(wy * wx) (an int32 product, converted once): a tent
 *                   that rises by 1 per pixel from each tile border and is capped at the ramp.
 *   SOLE VIEW       w = 1.0f when n == 1: a pixel that one view alone covers reproduces that tile's own sample.
 *   SAMPLE          v_k = the bilinear resize (align_corners = False) of class k's grid scores[f][r * Cn + c][k] to
 *                   (th, tw), taken at (sy, sx) = (bit 1 of flips[f] ? th - 1 - y : y, bit 0 ? tw - 1 - x : x) by the
 *                   function the semantic post-processing resizes with (grid_logit of csrc/postprocess_grid.h):
 *                     s = (float)gh / (float)th;  a = s * ((float)sy + 0.5f) - 0.5f;  a = a < 0 ? 0 : a;
 *                     y0 = min((int)a, gh - 1);  y1 = y0 + (y0 < gh - 1);  ly = min(max(a - (float)y0, 0), 1);
 *                     hy = 1 - ly; the same along x with gw, tw, sx -> x0, x1, lx, hx;
 *                     t0 = hx * p[y0][x0] + lx * p[y0][x1];  t1 = hx * p[y1][x0] + lx * p[y1][x1];
 *                     v = hy * t0 + ly * t1.
 *   ACCUMULATION    acc_k and wsum start at 0; per view acc_k = acc_k + w * v_k and wsum = wsum + w.
 *   OUTPUTS         seg = the first-max argmax over k of acc_k (k == 0 || acc_k > best, the rule of
 *                   wm2f_semantic_resize_argmax); out_scores[k] = acc_k / wsum, correctly rounded, and acc_k itself
 *                   when n == 1.
 *   UNCOVERED       n == 0: seg = -1 and out_scores = 0.  Every output pixel is written.
 * One launch, no workspace and no atomics: every result is bit-identical from run to run.  A lane owns two consecutive
 * pixels of a row and stores 8 bytes at a time when W is even, pixel by pixel otherwise, with the same values; classes
 * are held four at a time.  ys and xs need not be ascending for the result to follow the rules above, and no value in
 * them makes the kernel read outside scores.
 * F, R, Cn, C >= 1, ramp_y, ramp_x >= 1 and positive sizes, else WM2F_EINVAL; gh, gw, th, tw, H, W <= WM2F_TILE_MAX_SIDE
 * and R * Cn <= WM2F_TILE_MAX_TILES, else WM2F_EUNSUPPORTED. */
int wm2f_tile_blend(const void* scores, const int32_t* ys, const int32_t* xs, const int32_t* flips, int32_t* seg,
                    void* out_scores, int F, int R, int Cn, int C, int gh, int gw, int th, int tw, int ramp_y, int ramp_x,
                    int H, int W, void* stream);

/* ---- repairing id maps: small pieces, largest piece, holes -----------------------------------
 * A predicted id map paints thresholded masks over one another: an id often owns one plant-sized piece plus detached
 * specks, and plants have pinholes.  This call repairs a whole (B, H, W) stack in a fixed chain of launches, whatever
 * the number of instances; tests/clean_reference.py restates the contract with scipy.ndimage.label.
 * Input: map (B, H, W) is WM2F_F32, WM2F_I32 or WM2F_U8; which value is which id follows wm2f_labelmap_instance_stats
 *   (a float counts as the integer it equals, +-0 as 0; negative, fractional, not finite or >= 2^24: no id).  The
 *   instances are the ids 0 .. N-1; every other pixel is FREE (-1, no-id values, ids >= N such as a 255 ignore value).
 * Steps, in this order:
 *   1. PIECES.  Two pixels of one id join when they are 8-neighbours; a piece is a connected set of one id, its area
 *      its pixel count, its first pixel its smallest linear index y * W + x.
 *   2. keep.  WM2F_CLEAN_KEEP_ALL keeps every piece; WM2F_CLEAN_KEEP_LARGEST keeps per id and image the piece of
 *      greatest area only, among equal areas the one with the smallest first pixel.
 *   3. min_area (>= 0).  A piece still kept is dropped when its area < min_area (under KEEP_LARGEST an id whose
 *      largest piece is too small disappears).  Dropped pixels become free.
 *   4. fill_holes (0 / 1) with max_hole_area (< 0: no limit).  On the map after steps 2-3 free pixels join when they
 *      are 4-neighbours (the dual connectivity: a diagonal gap in an 8-connected ring does not leak).  A free
 *      component is a HOLE OF k when it touches no image border and every id pixel 4-adjacent to it carries the same
 *      id k; a hole of k with area <= max_hole_area is painted k.  Components that touch the border or are bounded by
 *      two or more ids stay free.  Holes are judged against the map after steps 2-3, never against partly filled
 *      output.  A speck of j inside plant i that step 3 dropped becomes (part of) a hole of i and is filled.
 *   5. relabel (0 / 1).  With 1 the ids that still own a pixel are renumbered 0 .. n'-1 in ascending old-id order.
 * Outputs: out (B, H, W), WM2F_I32 or WM2F_F32 (out_dtype), overwritten, must not overlap map: the pixel's final id, -1
 *   when free.  stats (B, N, 8) int64, overwritten:
 *     [area_in, pieces_in, pieces_kept, area_kept, holes_filled, pixels_filled, area_out, new_id],
 *   area_out = area_kept + pixels_filled; new_id is -1 for an id without a pixel in out and the old id when relabel = 0.
 *   n_out (B) int32: the number of ids that own a pixel in out.  stats may be NULL when N = 0.
 * With KEEP_ALL, min_area <= 1 and fill_holes = 0, out holds exactly the ids of map.
 * H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED; bad flags, a negative min_area, an unknown phase and
 * overlapping buffers are WM2F_EINVAL.  workspace: wm2f_labelmap_clean_workspace(B, H, W, N) bytes (-1 for a bad
 * size), 8-byte aligned, no clearing needed: 12 bytes per (image, id) and 20 bytes per pixel (id, union-find parent,
 * and at root pixels the area and the min / max adjacent id), each array rounded up to 16 bytes.  No call allocates,
 * keeps state or waits for the device.
 * phase: WM2F_CLEAN_ALL runs the chain; the other values run one part of it with the same arguments and workspace, in
 *   this order (the binding launches them one by one so that a kernel timer sees each):
 *   WM2F_CLEAN_PIECES  init; the 8-connected labelling: local (a 32 x 32 tile per workgroup, union-find in LDS whose
 *                      union links the larger root under the smaller by atomicMin -- a root is the smallest index of its
 *                      set, whatever the schedule -- and per tile root its pixel count in LDS), merge (device-scope
 *                      atomicMin across tile borders), flatten (every tile root points at its final root and adds its
 *                      tile's count there: one integer atomic per (tile, tile root), none per pixel).
 *   WM2F_CLEAN_CHOOSE  best: per piece one 64-bit atomicMax of area << 32 | (0xFFFFFFFF - first pixel) on its id's slot
 *                      (exact: H * W <= 2^28), with area_in and pieces_in; while N <= 1024 a workgroup gathers its 4096
 *                      pixels' pieces per id in LDS (20 B per id) and flushes the ids it saw, above that the pieces go to
 *                      the result directly; keep: a piece is kept iff its key equals that slot or KEEP_ALL is set,
 *                      and its area >= min_area.
 *   WM2F_CLEAN_HOLES   (nothing when fill_holes = 0) the same labelling code on the free pixels, 4-connected, which also
 *                      collects per component a border flag and the min and max of the 4-adjacent ids; then one add per
 *                      hole into holes_filled and pixels_filled.
 *   WM2F_CLEAN_PAINT   relabel (a workgroup per image scans area_out > 0 over the N ids into a table) and paint (16-byte
 *                      stores when W % 4 == 0 and out is 16-byte aligned, pixel by pixel otherwise, same results).
 * 12 kernel launches with holes, 8 without, at every N >= 1, B and size.  All integer, bit-identical from run to run. */
#define WM2F_CLEAN_KEEP_ALL 0
#define WM2F_CLEAN_KEEP_LARGEST 1
#define WM2F_CLEAN_ALL 0
#define WM2F_CLEAN_PIECES 1
#define WM2F_CLEAN_CHOOSE 2
#define WM2F_CLEAN_HOLES 3
#define WM2F_CLEAN_PAINT 4
int64_t wm2f_labelmap_clean_workspace(int B, int H, int W, int N);
int wm2f_labelmap_clean(const void* map, int dtype, void* out, int out_dtype, int64_t* stats, int32_t* n_out,
                        void* workspace, int B, int H, int W, int N, int keep, int64_t min_area, int fill_holes,
                        int64_t max_hole_area, int relabel, int phase, void* stream);

/* ---- splitting touching instances: a watershed of the interior distance -----------------------
 * Every route that makes instances ends in "one connected blob = one plant"; two plants whose leaves touch, or that one
 * query painted, are one instance.  This call parts them where the blob has a neck, for a whole (B, H, W) stack in a
 * fixed chain of launches whatever the number of instances, basins and images.  tests/split_reference.py restates the
 * rule in numpy.
 * Input: map (B, H, W) WM2F_F32, WM2F_I32 or WM2F_U8, ids by wm2f_labelmap_instance_stats' rule; the instances are the
 *   ids 0 .. N-1, every other pixel is background (as for wm2f_labelmap_clean).  d2 (B, H, W) int32: the output of
 *   wm2f_labelmap_distance for the same map (either border mode).
 * Definitions: lin(p) = y * W + x.  key(p) = (d2[p] << 32) | (0xFFFFFFFF - lin(p)), unsigned 64-bit, unique per pixel:
 *   the larger distance wins, among equal distances the earlier pixel in raster order.
 * ASCENT.  up(p) is the pixel of largest key among p and those of its 8 neighbours that carry p's id.  A pixel with
 *   up(p) = p is a PEAK.  Following up from an instance pixel ends at a peak (keys strictly increase); the pixels that
 *   end at one peak are a BASIN.
 * GROUPS.  A group is a set of basins of one id; at the start every basin is its own group.  A group's peak is the peak
 *   of largest key among its basins; peak_d2(G) and peak_lin(G) are that pixel's distance and position.
 * ROUNDS.  `rounds` synchronous rounds; every decision of a round reads the state at the round's start.
 *   1. For every 8-adjacent pair p, q of equal id in different groups the pass height is s = min(d2[p], d2[q]).
 *   2. A group G takes, over all such pairs it is part of, the largest (s << 32) | (0xFFFFFFFF - peak_lin(other group)):
 *      its highest pass, among equal passes the neighbour whose peak comes first in raster order: (s*, O).
 *   3. G is linked under O when key(peak O) > key(peak G) and
 *      (peak_d2(G) < min_peak_d2  or  s* * den^2 >= num^2 * peak_d2(G), in int64).
 *   4. After all decisions the groups are the trees of links.  Links go strictly up in peak key: no cycles, and a
 *      tree's root is its group's peak.
 *   A part merges into the higher neighbour across its highest pass when the neck is at least num / den of the part's
 *   own clearance, or when the part's clearance is below sqrt(min_peak_d2).
 * OUTPUT.  out (B, H, W) int32, -1 on background.  For each id k the group with the largest peak key keeps k; every
 *   other group gets N, N+1, ... in raster order of its peak pixel, over the whole image.  M is the size of the output
 *   id space: a group whose id would be >= M is not split off, its pixels keep k.
 *   info (B, M, 4) int32 per output id: [parent_id, peak_x, peak_y, peak_d2], parent_id = k for k itself and for the
 *   groups split off k; [-1, -1, -1, 0] for an id without a pixel.
 *   status (B, 4) int32: [ids wanted (N + extra groups, uncapped), basins at the start, links made in the last of the
 *   `rounds` rounds, rounds].  A non-zero third entry says that more rounds would have merged more; the result is
 *   still the defined result of `rounds` rounds.
 *   Disconnected pieces of one id are never adjacent, so they come out as separate instances.
 * Limits: H, W <= 16384, B <= 32, N <= M <= 4096, else WM2F_EUNSUPPORTED, reported before a pointer is looked at;
 *   1 <= rounds <= 32, 0 <= num <= den, 1 <= den <= 1024, min_peak_d2 >= 0, else WM2F_EINVAL.  out must not overlap map
 *   or d2.  workspace: wm2f_labelmap_split_workspace(B, H, W, M) bytes (-1 for a bad size), 16-byte aligned like info
 *   and status, no clearing needed: 16 bytes per pixel (id, forest pointer, and 8 bytes that hold a group's best pass
 *   during the rounds and the new ids after them), 8 per (image, id), 4 per 1024 pixels and 136 per image.
 * Kernels: init; ascent (decodes the map, up(p), counts the peaks); flatten (every pixel follows its pointer to the fixed
 *   point: the basins); per round pass (a pixel and its four forward neighbours, a 64-bit atomicMax into both groups'
 *   slots after a look at the slot), decide (a thread per group peak) and flatten, each returning at once when the
 *   round before linked nothing; keep (64-bit atomicMax per id), count, scan, assign (the extras in raster order) and
 *   paint.  8 + 3 * rounds launches.  Integer max and add atomics only: bit-identical from run to run.  No call
 *   allocates, keeps state or waits for the device. */
int64_t wm2f_labelmap_split_workspace(int B, int H, int W, int M);
int wm2f_labelmap_split(const void* map, int dtype, const int32_t* d2, int32_t* out, int32_t* info, int32_t* status,
                        void* workspace, int B, int H, int W, int N, int M, int num, int den, int min_peak_d2, int rounds,
                        void* stream);

/* ---- per-instance shape sums: moments, sides, border counts, convex hull ------------------------
 * What wm2f_labelmap_instance_stats does not say about an instance: how long, how ragged and how convex it is.  The
 * device returns exact integers; the float traits (axes, orientation, perimeter, solidity ...) are a few float64
 * operations on them (instances.shape_from_sums).  tests/shape_reference.py restates every rule in numpy / scipy.
 * Maps, ids / n_ids / N and "a value that is no listed id belongs to nothing" are wm2f_labelmap_instance_stats'.
 *
 * wm2f_labelmap_shape_stats: shape (B, N, 10) int64 per instance, x and y the pixel indices (point masses at pixel
 *   centres):  [0] area  [1] sum x  [2] sum y  [3] sum x^2  [4] sum y^2  [5] sum xy
 *   [6] sides: the pixel sides between a pixel of the instance and anything else, the outside of the image included (the
 *       length of the instance's crack contours);
 *   [7] p_straight  [8] p_diag  [9] p_mixed: a pixel of instance r is a BORDER pixel of r when one of its four
 *       neighbours is not r (outside the image is not r).  A border pixel with a border pixels of r among its four
 *       neighbours and b among its diagonal ones has the code 1 + 2a + 10b; codes 5, 7, 15, 17, 25, 27 count into
 *       p_straight, 21 and 33 into p_diag, 13 and 23 into p_mixed, every other code nowhere.  The 4-neighbourhood
 *       perimeter of skimage is p_straight + sqrt(2) p_diag + (1 + sqrt(2)) / 2 p_mixed; a lone pixel has 0.
 *   An id without a pixel has an all-zero row.  At the limits area <= 2^28 and x^2 < 2^28: every sum is below 2^57 and
 *   fits int64.  Three launches (clear, moments: one read of the map; border: a second read through 64 x 32 tiles with
 *   a halo of 2).  Accumulators are in LDS up to N = 1024 (52 KiB at that N for the moments), in the result above.
 *
 * wm2f_labelmap_hull: the convex hull of every instance's pixel SQUARES, that is of the corners (x, y), (x+1, y),
 *   (x, y+1), (x+1, y+1) of its pixels on the corner lattice [0, W] x [0, H] (the "crack" coordinates of the polygons).
 *   stats (B, N, 8): wm2f_labelmap_instance_stats of the same map and rows (the boxes).  hull (B, N, 3) int64:
 *   [n_vertices, area2, feret2]: the number of hull vertices, twice the hull's area (the shoelace sum, exact), the
 *   largest squared distance between two vertices; [0, 0, 0] for an id without a pixel; n_vertices = -1 for an instance
 *   the row table was too short for.
 *   The vertices are strictly convex (no collinear point is kept), start at the vertex with the smallest (y, then x)
 *   and go on towards increasing x: with y pointing down every consecutive cross product
 *   (b - a) x (c - b) = (bx - ax)(cy - by) - (by - ay)(cx - bx) is POSITIVE (clockwise on the screen).
 *   rows: the capacity of the row table, at least the sum of the box heights of all B N instances (at most B N H).
 *   workspace: wm2f_labelmap_hull_workspace(B, N, rows) bytes (-1 for a bad size), 8-byte aligned, no clearing:
 *   8 (B N + 1) for the instances' first rows, 8 per row for (xmin, xmax) of every (instance, row), 16 per row and 32
 *   per instance for the vertex slots -- instance i owns 2 (h_i + 2) points, more than the 2 (h_i + 1) a hull can have.
 *   The vertices stay in the workspace; wm2f_labelmap_hull_vertices copies them out.
 *   Four launches: scan of the box heights (one workgroup), table init, rows (one read of the map, atomicMin /
 *   atomicMax per run), chain (a wave per instance: Andrew's monotone chain down the right and the left side in
 *   int64 cross products, the shoelace sum, the largest distance by brute force).
 * wm2f_labelmap_hull_vertices: vertices (B, N, K, 2) int32 <- the first K vertices (x, y) of every instance from the
 *   workspace wm2f_labelmap_hull left (same stats, hull, rows), (-1, -1) past n_vertices.  One launch.
 * Limits: H, W <= 16384, B <= 32, N <= 4096, rows <= 2^30, K <= 2 (16384 + 2), else WM2F_EUNSUPPORTED, reported before
 *   a pointer is looked at; a size below 1, a null pointer, ids without n_ids or another dtype: WM2F_EINVAL.  Integer
 *   atomics only: bit-identical from run to run.  No call allocates, keeps state or waits for the device. */
int wm2f_labelmap_shape_stats(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids, int64_t* shape, int B,
                              int H, int W, int N, void* stream);
int64_t wm2f_labelmap_hull_workspace(int B, int N, int64_t rows);
int wm2f_labelmap_hull(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids, const int64_t* stats,
                       int64_t* hull, void* workspace, int64_t rows, int B, int H, int W, int N, void* stream);
int wm2f_labelmap_hull_vertices(const int64_t* stats, const int64_t* hull, const void* workspace, int64_t rows,
                                int32_t* vertices, int B, int H, int N, int K, void* stream);

/* ---- crop rows: the Hough vote of the voting pixels, instances against a set of lines -----------
 * Positions along a direction are integers in units of 2^-14 pixel.  A direction is a pair (c, s) = (rint(cos th 2^14),
 * rint(sin th 2^14)) with th in [0, pi), so s >= 0: th is the direction of the row NORMAL.  A pixel (x, y) -- indices,
 * not centres -- lies at rho = x c + y s + off with off = -min(0, c) (W - 1), which makes rho >= 0 over the image.  At
 * the limits every product is at most 2^28 and rho is below 2^29.  tests/rows_reference.py restates every rule in numpy.
 *
 * wm2f_labelmap_row_votes: map (B, H, W) fp32 / int32 / uint8, decoded as an id of [0, N) or nothing; vote (B, N) uint8:
 *   a pixel of id i votes when vote[b][i] != 0.  cs (T, 2) int32: the directions, taken as given (the host computes
 *   th_t = pi t / T; the kernel does no trigonometry).  A voting pixel's bin for direction t is
 *   (x c_t + y s_t + off_t) >> shift: bins of 2^(shift - 14) pixels, R = (((W + H - 2) << 14) >> shift) + 1 of them.
 *   acc (B, T, R) int32 <- the vote counts; energy (B, T) int64 <- the sum over the bins of acc^2 (below 2^44).  Both
 *   are written in full: no clearing needed.
 *   Three launches: clear; votes (64 x 64 pixel tiles, the voters compacted once, LDS histograms of 16 directions x 128
 *   bins, their non-zero bins added to acc by integer atomics; one read of the map when there are at least 2048 tiles,
 *   up to ceil(T / 16) reads of a small one); energy (a workgroup per row of acc).
 *   Limits: 1 <= T <= 1024, H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED; a size below 1 or a shift outside
 *   [14, 20]: WM2F_EINVAL; both are decided before a pointer is looked at.
 *
 * wm2f_labelmap_row_bands: map, ids / n_ids / N as wm2f_labelmap_instance_stats takes them.  line (B, 4) int32
 *   [c, s, off, K] per image; rho (B, Kmax) int32: the positions of the image's rows, ascending, the first K valid
 *   (K is clamped to [0, Kmax]; rho may be NULL when Kmax = 0); band >= 0: a half-width, same unit.
 *   A pixel is IN A BAND when |rho(p) - rho_k| <= band for the row k nearest to it; with K = 0 no pixel is.
 *   counts (B, N, 3) int64 per instance: [0] its pixels  [1] those in a band  [2] the sum of rho(p) over them (below
 *   2^58); an id without a pixel has an all-zero row.  zone (B, H, W) uint8, optional: 1 for a pixel in a band, 0
 *   otherwise, written for every pixel whatever its id.
 *   Two launches (clear; one read of the map, the row positions in LDS and a binary search per pixel).  Accumulators
 *   are in LDS up to N = 1024, in the result above.
 *   Limits: Kmax <= 1024, H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED, reported before a pointer is looked
 *   at; a size below 1, Kmax or band below 0, a null pointer, ids without n_ids or another dtype: WM2F_EINVAL.
 * Integer atomics only: bit-identical from run to run.  No call allocates, keeps state or waits for the device. */
int wm2f_labelmap_row_votes(const void* map, int dtype, const uint8_t* vote, const int32_t* cs, int32_t* acc,
                            int64_t* energy, int B, int H, int W, int N, int T, int shift, void* stream);
int wm2f_labelmap_row_bands(const void* map, int dtype, const int32_t* ids, const int32_t* n_ids, const int32_t* line,
                            const int32_t* rho, int64_t* counts, uint8_t* zone, int B, int H, int W, int N, int Kmax,
                            int band, void* stream);

/* ---- skeletons: parallel thinning of id maps, per-instance skeleton sums -------------------------
 * What the other per-instance calls do not say about a plant: how long its leaves and stems are, how many ends it has
 * and how wide its parts are.  tests/skeleton_reference.py restates every rule in numpy; no library's thinning is
 * claimed to give the same bytes.
 *
 * wm2f_labelmap_skeleton
 * Input: map (B, H, W) WM2F_F32, WM2F_I32 or WM2F_U8, ids by wm2f_labelmap_instance_stats' rule; the instances are the
 *   ids 0 .. N-1, every other pixel is background (as for wm2f_labelmap_clean).
 * State: an int32 map s, s[p] = id while p is alive, -1 otherwise.  At the start every instance pixel is alive.
 * Neighbours of a live pixel p of id k:  p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S, p7 = SW, p8 = W, p9 = NW (N is y - 1,
 *   E is x + 1).  pi = 1 iff that pixel is inside the image and alive with the same id k; another id counts as
 *   background, so all instances thin at once and never interact.
 * Deletion rule (Guo and Hall, CACM 32(3), 1989, algorithm A1: two sub-iterations):
 *   C  = (!p2 & (p3 | p4)) + (!p4 & (p5 | p6)) + (!p6 & (p7 | p8)) + (!p8 & (p9 | p2))
 *   N1 = (p9 | p2) + (p3 | p4) + (p5 | p6) + (p7 | p8)
 *   N2 = (p2 | p3) + (p4 | p5) + (p6 | p7) + (p8 | p9)
 *   N  = min(N1, N2)
 *   m0 = (p6 | p7 | !p9) & p8          (first sub-iteration)
 *   m1 = (p2 | p3 | !p5) & p4          (second sub-iteration)
 *   p is deleted in sub-iteration j  iff  C = 1 and 2 <= N <= 3 and mj = 0.
 *   A sub-iteration is synchronous: every decision reads the state at its start.  An iteration is sub-iteration 0, then
 *   sub-iteration 1.  The result is the state after `rounds` iterations.  An iteration that deletes nothing leaves a
 *   fixed point, so every later one deletes nothing either.
 * Output: out (B, H, W) int32: the skeleton as an id map again, -1 elsewhere.
 *   status (B, 4) int32: [skeleton pixels, iterations that deleted something, deletions in iteration `rounds`, rounds].
 *   A non-zero third entry says that `rounds` was too small; out is then still the defined result of exactly `rounds`
 *   iterations.  A solid shape settles in about (its largest half-width + 1) iterations.
 * per_launch: the iterations a launch runs on a tile held in LDS, 1, 2, 4 or 8; 0: the shipped default (4).  Every value
 *   gives the same bits.
 * Limits: H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED, reported before a pointer is looked at; a size
 *   below 1, rounds outside [1, 1024], another per_launch, a null pointer or another dtype: WM2F_EINVAL.  out must not
 *   overlap map.  workspace: wm2f_labelmap_skeleton_workspace(B, H, W) bytes (-1 for a bad size), 16-byte aligned, no
 *   clearing needed: one int32 plane and 8 KiB of counters per image.
 * Kernels: init (counters); ceil(rounds / per_launch) launches of thin; status.  A thin workgroup owns a 64 x 64 tile:
 *   it loads the tile and a halo of 2 per_launch pixels into LDS as int16 cells, runs its sub-iterations there
 *   (decisions into registers, a barrier, the writes, a barrier) and stores the owned tile; after sub-iteration t the
 *   cells at least t inside the loaded region are exact; after two sub-iterations in a row in which the workgroup
 *   deleted nothing its image is final and it goes on to the store.  The launches ping-pong between out and the workspace plane so
 *   that the last one writes out; the first decodes the map; the last runs only the iterations that remain.  From the
 *   third on, a launch returns at once when the launch before it deleted nothing in its image (that launch copied one
 *   plane to the other, so both hold the result).  Integer add atomics only, one per workgroup and counter:
 *   bit-identical from run to run.  No call allocates, keeps state, reads anything back or waits for the device.
 *
 * wm2f_labelmap_skeleton_stats: skel (B, H, W) int32, what wm2f_labelmap_skeleton wrote; d2 (B, H, W) int32, optional:
 *   wm2f_labelmap_distance of the ORIGINAL map; ids / n_ids / N as wm2f_labelmap_shape_stats takes them.  For a skeleton
 *   pixel p of id k, pi as above on skel, b = the number of pi that are 1, and X = the crossing number: the sum of
 *   !pi & p(i+1) around the cycle p2, p3, ..., p9, p2.  stats (B, N, 8) int64 per id:
 *   [0] skeleton pixels
 *   [1] orthogonal links: pairs of 4-adjacent skeleton pixels of the id, each pair once
 *   [2] diagonal links: pairs of diagonally adjacent skeleton pixels of the id, counted only when neither of the two
 *       pixels 4-adjacent to both is a skeleton pixel of that id (a staircase does not count its triangles twice)
 *   [3] tips: X = 1 and b <= 2      [4] junction pixels: X >= 3      [5] isolated pixels: b = 0
 *   [6] the sum of d2 over the skeleton pixels      [7] the largest d2 among them      (both 0 without d2)
 *   The skeleton's length is [1] + sqrt(2) [2]; 2 sqrt(d2) - 1 is the width of the part a skeleton pixel runs through.
 *   (Guo and Hall's C is 0 at the centre of a 4-connected "+", which is why junctions use X.)  An id without a skeleton
 *   pixel has an all-zero row.  Two launches (clear; one read of the map, a one-pixel stencil around skeleton pixels,
 *   one lane adding for its wave when the wave's skeleton pixels share an id).
 *   Limits as above with N >= 1; ids without n_ids: WM2F_EINVAL.  Integer add and max atomics: bit-identical. */
int64_t wm2f_labelmap_skeleton_workspace(int B, int H, int W);
int wm2f_labelmap_skeleton(const void* map, int dtype, int32_t* out, int32_t* status, void* workspace, int B, int H, int W,
                           int N, int rounds, int per_launch, void* stream);
int wm2f_labelmap_skeleton_stats(const int32_t* skel, const int32_t* d2, const int32_t* ids, const int32_t* n_ids,
                                 int64_t* stats, int B, int H, int W, int N, void* stream);

/* ---- skeleton graphs: spur pruning, branches and node clusters, per-instance graph sums ----------
 * A raw skeleton grows a side branch for every bump of a mask's boundary, and it has no structure.  These two calls
 * decompose a skeleton into branches and node clusters, delete the branches that are boundary noise, and sum the graph
 * per id.  tests/skeleton_graph_reference.py restates every rule in numpy (array passes, scipy.ndimage.label per key).
 *
 * Input: skel (B, H, W) int32, a skeleton map: an id in [0, N), anything else is dead (-1 after decoding).  Normally what
 *   wm2f_labelmap_skeleton wrote, but any int32 map is defined input.  d2 (B, H, W) int32: wm2f_labelmap_distance of the
 *   ORIGINAL map; a negative value counts as 0.
 * Pixel classes, for a live pixel p of id k, p2 .. p9 as above (same-id live neighbours inside the image):
 *   b = the number of pi that are 1;  X = the crossing number, the sum of !pi & p(i+1) around the ring p2 .. p9, p2.
 *   node pixel: b >= 3.   path pixel: b <= 2.
 *   free end: a path pixel with b <= 1, or with b = 2 and X = 1 (its two neighbours are adjacent to each other).
 *   Nodes go by b, not by X: with X >= 3 the path pixels around a T-junction stay 8-connected through their diagonals
 *   and the branches do not come apart.  With b >= 3 every component of path pixels is a chain or a closed ring.
 * Components: key = 2 k + [node].  A component is an 8-connected set of pixels of equal key: a BRANCH when its pixels are
 *   path pixels, a NODE CLUSTER when they are node pixels.  Its label is the smallest linear index y W + x among its
 *   pixels.
 * Branch record: P = its pixels; T = its free ends; a contact is a pair (path pixel of the branch, 8-adjacent node pixel
 *   of the same id); cmin / cmax = the smallest / largest label among the clusters of contacted node pixels; D = the
 *   largest d2 among contacted node pixels.
 * Spur: a branch with T >= 1, a contact, cmin = cmax, and P <= min_pixels or 256 P'^2 <= ratio_q^2 D in int64 with
 *   P' = min(P, 2^20).  ratio_q = round(16 ratio): "the branch is no longer than `ratio` times the half-width of the
 *   part it grows out of", which is how long a boundary-noise spur is; a leaf is many half-widths long.  Because
 *   cmin = cmax, everything adjacent to a deleted branch lies in one connected cluster, and a cluster is never deleted:
 *   the 8-connected pieces of every id survive, under simultaneous deletions too.  An isolated line (no contact) and a
 *   ring (T = 0) are never touched.  min_pixels = 0 and ratio_q = 0 delete no spur.
 *
 * wm2f_labelmap_skeleton_prune
 * One round: all spurs of the image are deleted at once, decided on the state at the round's start; then `rethin`
 *   iterations of wm2f_labelmap_skeleton's rule run on the result (they remove what is left of a node cluster, so the
 *   former junction becomes a thin pass-through).  The result is the state after `rounds` rounds, per image,
 *   unconditionally.  A round that changes nothing in an image leaves a fixed point of both steps.
 * Output: out (B, H, W) int32, the pruned skeleton as an id map, -1 elsewhere.  status (B, 4) int32:
 *   [pixels left, rounds that removed something, pixels removed in round `rounds`, pixels removed in all]; a non-zero
 *   third entry says that `rounds` was too few, and out is then still the defined result of exactly `rounds` rounds.
 * Limits: those of wm2f_labelmap_skeleton (WM2F_EUNSUPPORTED); a size below 1, min_pixels outside [0, 2^20], ratio_q
 *   outside [0, 1024], rounds outside [1, 64], rethin outside [1, 16] or a null pointer: WM2F_EINVAL; sizes before
 *   pointers, and all of them before a pointer is looked at.  out must not overlap skel or d2.  workspace:
 *   wm2f_labelmap_skeleton_prune_workspace(B, H, W) bytes (-1 for a bad size), 16-byte aligned, no clearing needed.
 * Kernels: per round local (classify and label inside 32 x 32 tiles), merge (tile borders), flatten, record (the branch
 *   records at the roots: integer add / min / max atomics, the counts once per wave where a wave's pixels share a root),
 *   delete, and the launches of wm2f_labelmap_skeleton; one clear before and a status kernel after: a fixed number of
 *   launches whatever the content.  The kernels of a round return at once for an image in which the round before
 *   removed nothing (per-image live counts in device memory; nothing is read back).  Bit-identical from run to run.
 *
 * wm2f_labelmap_skeleton_graph: one decomposition, nothing deleted.  ids / n_ids / N as wm2f_labelmap_skeleton_stats
 *   takes them; with a list, row r of image b is the raw id ids[b][r] and a pixel whose value is not listed is dead.
 *   labels (B, H, W) int32: -1 for a dead pixel, a path pixel's branch label, -2 - (cluster label) for a node pixel.
 *   sums (B, N, 8) int64 per id:
 *   [0] branches      [1] end branches (T >= 1 and a contact)      [2] node clusters      [3] node pixels
 *   [4] free ends     [5] P of the longest end branch              [6] P of the longest branch
 *   [7] closed branches (T = 0 and at most one contacted cluster)
 *   An id without a skeleton pixel has an all-zero row.  Limits as above with N >= 0 (sums may be null when N = 0); ids
 *   without n_ids: WM2F_EINVAL.  labels must not overlap skel.  workspace: wm2f_labelmap_skeleton_graph_workspace bytes,
 *   16-byte aligned.  Six launches: clear, the four of the decomposition, labels (one add per root). */
int64_t wm2f_labelmap_skeleton_prune_workspace(int B, int H, int W);
int wm2f_labelmap_skeleton_prune(const int32_t* skel, const int32_t* d2, int32_t* out, int32_t* status, void* workspace,
                                 int B, int H, int W, int N, int min_pixels, int ratio_q, int rounds, int rethin,
                                 void* stream);
int64_t wm2f_labelmap_skeleton_graph_workspace(int B, int H, int W);
int wm2f_labelmap_skeleton_graph(const int32_t* skel, const int32_t* ids, const int32_t* n_ids, int32_t* labels,
                                 int64_t* sums, void* workspace, int B, int H, int W, int N, void* stream);

/* ---- colour: per-instance sums of the picture under an id map, vegetation-index histogram and mask
 * A picture is (B, H, W, 3) uint8, packed, R G B per pixel, at any byte address.  An INDEX is I = a R + b G + c B with
 * integer coefficients, not all zero, |a| + |b| + |c| <= 32.  Its smallest value is Imin = -255 x (the sum of the
 * negative coefficients' magnitudes); it takes bins = 255 (|a| + |b| + |c|) + 1 values (at most 8161); a pixel's bin is
 * I - Imin.  The NORMALISED index of a pixel is q = floor(4096 I / (R + G + B)), 0 where R + G + B = 0: Q12 on the
 * chromatic coordinates, FLOOR division ((200, 1, 0) under (-1, 2, -1) gives -4035).  tests/color_reference.py restates
 * every rule in numpy with Python's //.
 *
 * wm2f_labelmap_color_stats: maps, ids / n_ids / N and "a value that is no listed id belongs to nothing" are
 *   wm2f_labelmap_instance_stats'.  thresholds (B) int32 on the device.  sums (B, N, 14) int64 per instance, over the
 *   pixels that carry its id:
 *   [0] area   [1..3] sum R, G, B   [4..6] sum R^2, G^2, B^2   [7..9] sum RG, RB, GB
 *   [10] n_on: pixels with I > thresholds[b]   [11] sum q (signed)
 *   [12] n_dark: pixels with max(R, G, B) < dark   [13] n_bright: pixels with max(R, G, B) >= bright
 *   An id without a pixel has an all-zero row.  At the limits (area <= 2^28) every sum stays below 2^45.
 *   hue (B, N, K) int64, or null (then K and min_chroma are not looked at): hue[b][r][k] counts the instance's pixels with
 *   chroma cr = mx - mn >= min_chroma whose integer hue h falls in bin h / (360 / K), mx and mn the largest and smallest
 *   of R, G, B.  h in [0, 360), with floor division, the cases in this order:
 *     mx == R: h = floor(60 (G - B) / cr), plus 360 when negative;   else mx == G: h = 120 + floor(60 (B - R) / cr);
 *     else: h = 240 + floor(60 (R - G) / cr).          (255, 0, 1) gives 359.
 *   This is the project's own integer hue; it is NOT Pillow's float HSV of wm2f_photometric_u8.
 *   Both results are cleared inside the call.  A memset per result and one launch whatever N.
 * wm2f_image_index_hist: hist (B, bins) int64, cleared inside the call: the count of every value of I over the picture.
 * wm2f_image_index_mask: mask (B, H, W) uint8 <- 1 where I > thresholds[b], else 0; counts (B) int64, cleared inside the
 *   call, <- the on-pixels.  One launch; 3 bytes read and 1 written per pixel.
 * Limits: H, W <= 16384, B <= 32, N <= 4096, else WM2F_EUNSUPPORTED; a size below 1, coefficients outside the rule above,
 *   dark or bright outside [0, 255], with hue K outside [1, 36] or not a divisor of 360 or min_chroma outside [1, 255],
 *   another map dtype, a null pointer, ids without n_ids: WM2F_EINVAL; sizes and scalars before pointers.  No float
 *   instruction, integer atomics only: bit-identical from run to run.  No call allocates, keeps state or waits. */
int wm2f_labelmap_color_stats(const uint8_t* image, const void* map, int dtype, const int32_t* ids, const int32_t* n_ids,
                              int ca, int cb, int cc, const int32_t* thresholds, int dark, int bright, int K,
                              int min_chroma, int64_t* sums, int64_t* hue, int B, int H, int W, int N, void* stream);
int wm2f_image_index_hist(const uint8_t* image, int ca, int cb, int cc, int64_t* hist, int B, int H, int W, void* stream);
int wm2f_image_index_mask(const uint8_t* image, int ca, int cb, int cc, const int32_t* thresholds, uint8_t* mask,
                          int64_t* counts, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WM2F_H */
