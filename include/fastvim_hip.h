/*
 * fastvim_hip.h -- C ABI of libfastvim_hip.so, the MI355X (gfx950) native kernel
 * library for the FastVim backbone hot path.
 *
 * Boundary rules:
 *   - extern "C", plain device pointers + sizes, no torch / C++ types;
 *   - every entry point enqueues work on `stream` (a hipStream_t) and returns
 *     immediately -- no host synchronisation, no allocation (graph-capture safe);
 *     the caller owns every buffer (in practice: the torch caching allocator);
 *   - return value: FV_OK (0) or a negative FV_ERR_* code; fv_last_error() gives
 *     the message (the Python host raises RuntimeError from it, mirroring the
 *     reference's TORCH_CHECK -> RuntimeError, selective_scan.cpp:235-305);
 *   - tensors are contiguous in the stated layout; `dtype` selects the storage
 *     type of activations (FV_F32 / FV_BF16 / FV_F16); all arithmetic is fp32.
 *
 * Each entry point cites the reference interface it replaces (paths relative to
 * the insitro/FastVim root).
 */
#ifndef FASTVIM_HIP_H
#define FASTVIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fv_stream_t; /* hipStream_t */

enum { FV_F32 = 0, FV_BF16 = 1, FV_F16 = 2 };
enum { FV_OK = 0, FV_ERR_INVALID = -1, FV_ERR_HIP = -2, FV_ERR_UNSUPPORTED = -3 };

const char* fv_last_error(void);
/* ABI version of this header; fv_version() returns the one the library was built with -- a caller compiled against
 * another value must not call anything else.  History:
 *   1  rounds 1-3.
 *   2  round 4 changed fv_mixer_scan_bwd_segments / fv_mixer_scan_bwd_seg_partials (a d_inner argument was inserted)
 *      without bumping the number; round 5 bumps it for that break, removes the opt-in fv_mixer_mid_fwd(_ok) and
 *      fv_gemm_bf16_addnorm_rw(_ok), and adds fv_mixer_scan_bwd_xproj(_ok), fv_mixer_conv_pool_bwd2(_ok),
 *      fv_chunk_rows_bf16.
 *   3  round 6 adds fv_mixer_conv_pool_bwd_dgrad(_ok, _blocks), fv_transpose_bf16_batched, fv_gemm_bf16_tn_grouped_wide8
 *      (nothing removed or changed).
 *      Later, still 3: fv_grad_sumsq_blocks, fv_grad_sumsq_partials and fv_adamw_flat_groups were ADDED (layer-wise lr
 *      decay and global-norm gradient clipping in the fused optimizer); no existing entry point changed, so the number
 *      stays.
 *      Later, still 3: fv_pack_weight_frags_batched, fv_mixer_conv_pool_bwd_dgrad_pk and
 *      fv_mixer_combine_out_proj_addnorm_pk were ADDED (projection weights streamed in MFMA fragment order); the plain
 *      entry points keep their signatures and the plain layout.
 *      Later, still 3: fv_pack_weight_frags_w2_batched and fv_mixer_conv_pool_bwd_dgrad_pk2 were ADDED (the second
 *      weight of the fused backward launch streamed in MFMA fragment order); no existing entry point changed --
 *      fv_pack_weight_frags_batched keeps the meaning of K and its checks.
 *      Later, still 3: fv_mix_batch, fv_patch_unfold_mix, fv_mixup_target and fv_label_ce were ADDED (batch Mixup /
 *      CutMix and the losses on integer labels).
 *      Later, still 3: fv_patch_unfold_chan, fv_chan_embed_table and fv_chan_embed_scatter were ADDED (hierarchical
 *      channel sampling of the channel models with the drawn subset in device memory).
 *      Later, still 3: fv_mixer_plan was ADDED (the launch plan of the mixer's row kernels, which now serve d_inner
 *      2048 and 2560: FastVim-L / -H).  fv_mixer_conv_pool_bwd2_ok is defined from it and therefore answers no
 *      for 1536 < d_inner <= 2048 that is not a multiple of 256 -- widths whose launch always failed -- and yes
 *      for the multiples of 256 up to 3072; no signature changed, so the number stays.
 *      Later, still 3: two preconditions were RELAXED, nothing added.  fv_patch_unfold and fv_patch_unfold_mix take any
 *      even patch width from 8 up (was: a multiple of 8; patch 14 of FastVim-H / MAE-H), and fv_mixer_combine_fwd / _bwd serve
 *      d_inner 2560 (and the other multiples of 512 from 1536 to 4096 that had no form) with tokens_per_patch > 1 when
 *      there is one patch column (the un-pooled geometry of the masked MAE encoders and the Vim mixer).
 *      Later, still 3: fv_bn1d_stats, fv_bn1d_apply, fv_bn1d_bwd, fv_sgd_flat, fv_lars_partials_per_segment,
 *      fv_lars_sumsq_partials and fv_lars_flat were ADDED (the linear-probe recipe: BatchNorm1d over pooled features,
 *      momentum SGD and LARS over the flat buffers).
 *      Later, still 3: fv_swap_params_ema and fv_eval_accumulate were ADDED (the validation step: the batch under the
 *      live and the EMA weights, metrics accumulated on the device).
 *      Later, still 3: fv_patch_unfold_u8, fv_patch_unfold_mix_u8 and fv_patch_unfold_chan_u8 were ADDED (8-bit image
 *      batches: the per-channel normalisation as a table lookup inside the patch unfold).
 *      Later, still 3: fv_random_erase, fv_patch_unfold_u8_re and fv_patch_unfold_mix_u8_re were ADDED (random erasing
 *      of the normalised image, with the boxes and the noise key in device memory); no existing entry point changed.
 *      Later, still 3: fv_mae_loss_ok, fv_mae_loss_fwd and fv_mae_loss_bwd were ADDED (the MAE reconstruction loss, from
 *      fp32 or uint8 images, fused into two launches forward and one backward); no existing entry point changed.
 *      Later, still 3: fv_mae_mask_plan, fv_tokens_gather, fv_mae_decoder_tokens_fwd and fv_mae_decoder_tokens_bwd were
 *      ADDED (the MAE masking plan from one launch, the permuted token copies, the decoder's input assembly); no existing
 *      entry point changed.
 *      Later, still 3: fv_pack_weight_frags_in_batched and fv_gemm_bf16_inproj_pk were ADDED (in_proj forward at
 *      d_model 192 with its weight streamed in MFMA fragment order); fv_gemm_bf16 is unchanged.
 *      Later, still 3: fv_resample_u8_ok, fv_resample_workspace_ints, fv_resample_coeffs and fv_resample_u8 were ADDED
 *      (bicubic resize, crop window and flip of uint8 images on the device, bit-exact to PIL); no existing entry point
 *      changed.
 *      Later, still 3: fv_randaug_ok, fv_randaug_workspace_bytes, fv_randaug_stats and fv_randaug_apply were ADDED
 *      (RandAugment of planar uint8 batches on the device, bit-exact to PIL); no existing entry point changed.
 *      Later, still 3: fv_jpeg_probe, fv_jpeg_entropy_decode, fv_jpeg_table_ints, fv_jpeg_idct and fv_jpeg_rgb were ADDED
 *      (JPEG decode split between a host entropy decoder and two device launches, byte-exact to PIL); no existing entry
 *      point changed.
 *      Later, still 3: fv_mae_noise and fv_mae_mask_plan_keyed were ADDED (the MAE masking noise as a function of a key
 *      block in device memory, and the masking plan of that noise without the noise tensor); fv_mae_mask_plan is
 *      unchanged.
 *      Later, still 3: fv_jpeg_entropy_decode_packed, fv_jpeg_packed_bound and fv_jpeg_idct_packed were ADDED (the packed
 *      coefficient form: a mask and the non-zero values per block); fv_jpeg_rgb also reads records of packed jobs; no
 *      signature changed.
 *      Later, still 3: fv_jpeg_index_bound, fv_jpeg_build_index, fv_jpeg_index_stage, fv_jpeg_stream_table_ints and
 *      fv_jpeg_huff were ADDED (device-side Huffman decoding from a per-file index: THE INDEX below); no existing entry
 *      point, record layout or default changed.
 *      Later, still 3: fv_cellaug_geom and fv_cellaug_filter were ADDED (the cell-image augmentation of the channel
 *      models' loader on planar uint8 planes: THE CELL RECORD below); no existing entry point changed.
 *      Later, still 3: fv_jpeg_sync_stage, fv_jpeg_sync_host, fv_jpeg_sync_table_ints and fv_jpeg_sync were ADDED (the
 *      entries fv_jpeg_huff starts from, found on the device without a sidecar index: ENTRIES MADE ON THE DEVICE below);
 *      no existing entry point, record layout or default changed.
 *      Later, still 3: fv_gemm_bf16_plan and fv_gemm_bf16_tn_grouped_plan were ADDED (the launch fv_gemm_bf16 and one launch
 *      of fv_gemm_bf16_tn_grouped(_ld) make, answered by the deciders the launches themselves ask: FV_GEMM_KIND_*,
 *      FV_GEMM_GROUPED_*); no existing entry point changed and every shape runs on the kernel it ran on.
 *      Later, still 3: fv_mae_encoder_tokens_cls_fwd, fv_mae_encoder_tokens_cls_bwd, fv_mae_decoder_tokens_cls_fwd and
 *      fv_mae_decoder_tokens_cls_bwd were ADDED (token assembly of the Vim MAE baseline, whose encoder carries a class token
 *      in the middle of the kept tokens and whose decoder carries it behind the grid); no existing entry point changed.
 *      Later, still 3: fv_vim_cls_tokens_fwd, fv_vim_cls_tokens_bwd, fv_add_norm_row_fwd and fv_add_norm_row_bwd were ADDED
 *      (the supervised Vim baseline: its class token put among the patch tokens with the position table, and its final
 *      add + norm of the class row alone); no existing entry point changed -- fv_add_norm_fwd / _bwd run the kernels they
 *      ran, whose bodies the row forms share.
 *      Later, still 3: fv_chan_cls_tokens_fwd and fv_chan_cls_tokens_bwd were ADDED (the ChannelVim baseline: its class
 *      token put among channel tokens that already carry their position rows -- rows moved, nothing added); no existing
 *      entry point changed: fv_vim_cls_tokens_* keep adding their table and writing fp32. */
#define FV_ABI_VERSION 3
int fv_version(void);

/* ------------------------------------------------------------------------
 * Selective scan, reference layout (B, D, L) with L contiguous.
 * Replaces pybind `selective_scan_cuda.fwd`
 *   (mamba-1p1p1/csrc/selective_scan/selective_scan.cpp:226-336, 494-497) and
 * `selective_scan_cuda.bwd` (selective_scan.cpp:338-492).
 *
 *   u, delta, z, out : (batch, dim, seqlen)            storage `dtype`
 *   A                : (dim, dstate)                   fp32
 *   B, C             : (batch, n_groups, dstate, seqlen) storage `dtype` if *_variable
 *                      else (dim, dstate) fp32
 *   D, delta_bias    : (dim) fp32, nullable
 *   last_state       : (batch, dim, dstate) fp32, nullable
 * out = (scan(u, softplus?(delta + delta_bias), A, B, C) + D*u) * silu(z)
 * ---------------------------------------------------------------------- */
int fv_selective_scan_fwd(const void* u, const void* delta, const float* A, const void* B,
                          const void* C, const float* D, const void* z, const float* delta_bias,
                          void* out, float* last_state, int batch, int dim, int seqlen, int dstate,
                          int n_groups, int B_variable, int C_variable, int delta_softplus,
                          int dtype, fv_stream_t stream);

/* Workspace (bytes) fv_selective_scan_bwd needs in `workspace`. */
size_t fv_selective_scan_bwd_workspace(int batch, int dim, int seqlen, int dstate, int n_groups,
                                       int B_variable, int C_variable);

/* Gradients.  du, ddelta, dz: storage `dtype`.  dA (dim,dstate), dD, ddelta_bias (dim): fp32.
 * dB, dC: fp32, (batch, n_groups, dstate, seqlen) if variable else (dim, dstate).
 * All gradient buffers are overwritten (no accumulation).  Deterministic: no float atomics. */
int fv_selective_scan_bwd(const void* u, const void* delta, const float* A, const void* B,
                          const void* C, const float* D, const void* z, const float* delta_bias,
                          const void* dout, void* du, void* ddelta, float* dA, float* dB, float* dC,
                          float* dD, void* dz, float* ddelta_bias, void* workspace, int batch, int dim,
                          int seqlen, int dstate, int n_groups, int B_variable, int C_variable,
                          int delta_softplus, int dtype, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Causal depthwise conv1d (+ SiLU), reference op layout (batch, dim, seqlen), seqlen contiguous.
 * Replaces `causal_conv1d_cuda.causal_conv1d_fwd(x, weight, bias, seq_idx=None, silu)` and
 * `causal_conv1d_cuda.causal_conv1d_bwd(x, weight, bias, dout, seq_idx=None, dx, silu) -> (dx, dw, dbias)`
 * of PyPI causal-conv1d 1.1.3.post1 (third-party, not vendored; pinned by the reference README.md:43 and
 * called at mamba_ssm/modules/mamba_simple_faster.py:274-285 and
 * mamba_ssm/ops/selective_scan_interface.py:496-498, 640-642, 751-753).
 *
 *   x, y, dy, dx : (batch, dim, seqlen) storage `dtype`;  weight (dim, width) fp32, width in 2..4;
 *   bias (dim) fp32, nullable;  silu != 0 applies SiLU to the output.
 *   y[b,d,l] = act(bias[d] + sum_k weight[d,k] * x[b,d,l-(width-1)+k])
 * Backward writes dx and per-(batch, dim) partials (batch, dim, 5) = [dw front-padded to 4 taps | dbias];
 * the caller sums them over batch with fv_reduce_partials (fixed order, deterministic).
 * ---------------------------------------------------------------------- */
int fv_causal_conv1d_fwd(const void* x, const float* weight, const float* bias, void* y, int batch, int dim,
                         int seqlen, int width, int silu, int dtype, fv_stream_t stream);
int fv_causal_conv1d_bwd(const void* x, const float* weight, const float* bias, const void* dy, void* dx,
                         float* partials, int batch, int dim, int seqlen, int width, int silu, int dtype,
                         fv_stream_t stream);

/* Expand + skip epilogue of the "compressed scan" fork: out[b,d,l] = yc[b,d,l/cf] + D[d]*u_full[b,d,l],
 * cf = seqlen / seqlen_compressed.  With fv_selective_scan_fwd on (u_compressed, delta, ...) this replaces
 * `faster_selective_scan_cuda.fwd(u, u_compressed, delta, A, B, C, D, z=None, delta_bias, softplus)`
 * (fastvim_kernel/mamba-1p1p1/csrc/selective_scan/selective_scan.cpp:216-360,
 *  selective_scan_fwd_kernel.cuh:68-299).  D nullable (then u_full may be null). */
int fv_scan_expand_skip_fwd(const void* yc, const void* u_full, const float* D, void* out, int batch, int dim,
                            int seqlen, int seqlen_compressed, int dtype, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused FastVim mixer "middle", channel-last (token-major) activations.
 * Together these replace the body of `Mamba.forward` between in_proj and out_proj
 *   (mamba-1p1p1/mamba_ssm/modules/mamba_simple_faster.py:270-444) and the fused autograd
 *   function `FastVim_MambaInnerFnNoOutProj_withoutZ`
 *   (mamba_ssm/ops/selective_scan_interface.py:452-776), which themselves call
 *   causal_conv1d_cuda.causal_conv1d_fwd/bwd (PyPI causal-conv1d 1.1.3.post1) and
 *   selective_scan_cuda.fwd/bwd.
 *
 * Layouts:  xz (batch, L, 2*d_inner)  [x | z] per token;  g, do (batch, L, d_inner);
 *           xc, yc, ... (2, batch, rows, d_inner)  [0] = forward direction, [1] = backward,
 *           both indexed by the pooled row in ORIGINAL order (no flips are materialised);
 *           x_dbl (2, batch*rows, dt_rank + 2*d_state) = [dt_low | B | C].
 * Token grid: the mixer's sequence position (i, j), i < rows, j < cols, is memory token
 *           i*tok_stride_row + j*tok_stride_col.  (cols, 1) = natural order; (1, rows) = the
 *           transposed grid odd layers see (models/fastvim.py:192-210) -- no copy is made.
 *           tokens_per_patch = t > 1 (channel-wise tokenization, Channel-First order,
 *           mamba_simple_channel_faster.py:242-256, 333-340): every grid cell holds t consecutive
 *           tokens, sequence position ((i*cols + j)*t + c), pooling groups (i, c), pooled tensors
 *           (2, batch, rows*t, d_inner), pooled index i*t + c; strides are in cells.
 * Conv weights are (d_inner, d_conv) fp32 (= conv1d.weight viewed "d 1 w -> d w").
 * ---------------------------------------------------------------------- */
/* Both depthwise convs + SiLU, the pooling over `cols` -> xc, and (skip != NULL) the D-weighted skip term
 * skip[b, token, :] = D*conv_f(x) + D_b*conv_b(x)  (batch, L, d_inner), memory token order, storage `dtype`
 * (mamba_simple_faster.py:356-358, 412-416): each conv+SiLU is evaluated once per forward pass.
 * pool_max != 0 (collapse_method="max", mamba_simple_faster.py:299-305): xc holds the row maxima and amax
 * (same shape and dtype as xc, nullable) receives the column of the first maximum, for the backward pass. */
int fv_mixer_conv_pool_fwd(const void* xz, const float* conv_w, const float* conv_b,
                           const float* conv_w_b, const float* conv_b_b, const float* D, const float* D_b,
                           void* xc, void* skip, void* amax, int batch, int rows, int cols, int tok_stride_row,
                           int tok_stride_col, int tokens_per_patch, int d_inner, int d_conv, int pool_max,
                           float scaling_factor, int dtype, fv_stream_t stream);

/* dt_proj + softplus + selective scan (A = -exp(A_log)) for both directions.  yc is fp32. */
int fv_mixer_scan_fwd(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias,
                      const float* A_log, const float* dt_w_b, const float* dt_bias_b,
                      const float* A_log_b, float* yc, int batch, int Lc, int d_inner, int dt_rank,
                      int d_state, int dtype, fv_stream_t stream);
/* Training form for long pooled lengths (Lc > 16, dt_rank <= 48): the forward launch also leaves the state entering
 * every 16-step chunk in `ckpt` (fv_mixer_scan_ckpt_floats() fp32; 0 = shape not covered, pass NULL), laid out
 * (2, batch, ceil(Lc/16), d_inner, d_state); fv_mixer_scan_bwd_ckpt(ckpt_given = 1) then skips its own forward sweep --
 * the states of the reference's forward kernel that its backward kernel re-derives (selective_scan_bwd_kernel.cuh:75-528
 * recomputes them chunk by chunk from `x`, the per-chunk running state saved by selective_scan_fwd_kernel.cuh:67-345). */
size_t fv_mixer_scan_ckpt_floats(int batch, int Lc, int d_inner, int d_state, int dt_rank);
int fv_mixer_scan_fwd_ckpt(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias,
                           const float* A_log, const float* dt_w_b, const float* dt_bias_b,
                           const float* A_log_b, float* yc, float* ckpt, int batch, int Lc, int d_inner, int dt_rank,
                           int d_state, int dtype, fv_stream_t stream);
/* Segment-parallel form for long sequences on few batch elements (the un-pooled Vim baseline at 2048 px: 16 385 steps,
 * batch 8; mamba_simple.py:210-255 -- the reference scans it with a parallel scan over L,
 * selective_scan_fwd_kernel.cuh:67-345): time is cut into fv_mixer_scan_fwd_segments() runs of whole 16-step chunks that
 * are scanned side by side -- states reached from zero, a serial combine over the segments, then the scan proper from the
 * true entry states (the recurrence is linear in the state).  seg_ws: fv_mixer_scan_fwd_seg_floats() fp32 of workspace
 * (0 = one segment: pass NULL, the call is fv_mixer_scan_fwd_ckpt).  yc / ckpt as there. */
int fv_mixer_scan_fwd_segments(int batch, int Lc, int d_inner, int dt_rank);
size_t fv_mixer_scan_fwd_seg_floats(int batch, int Lc, int d_inner, int d_state, int dt_rank);
int fv_mixer_scan_fwd_seg(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias,
                          const float* A_log, const float* dt_w_b, const float* dt_bias_b, const float* A_log_b,
                          float* yc, float* ckpt, float* seg_ws, int batch, int Lc, int d_inner, int dt_rank,
                          int d_state, int dtype, fv_stream_t stream);

/* x_proj + dt_proj + softplus + selective scan in ONE launch for short pooled lengths (Lc <= 16, bf16, dt_rank <= 48:
 * the 224 / 256 px grids): x_dbl (2, batch*Lc, dt_rank + 2*d_state) = xc @ x_proj_w2[dir]^T is computed on the matrix
 * cores inside the scan kernel (mamba_simple_faster.py:321-327 + 328-354), written out in bf16 for the backward pass and
 * consumed from LDS.  x_proj_w2: (2, dt_rank + 2*d_state, d_inner) bf16, both directions.  fv_mixer_xproj_scan_fwd_ok
 * tells whether a shape is covered (else: fv_mixer_xproj_fwd + fv_mixer_scan_fwd). */
int fv_mixer_xproj_scan_fwd_ok(int Lc, int d_inner, int dt_rank, int dtype);
int fv_mixer_xproj_scan_fwd(const void* xc, const void* x_proj_w2, const float* dt_w, const float* dt_bias,
                            const float* A_log, const float* dt_w_b, const float* dt_bias_b, const float* A_log_b,
                            void* x_dbl, float* yc, int batch, int Lc, int d_inner, int dt_rank, int d_state,
                            int dtype, fv_stream_t stream);

/* g = LayerNorm((yc_f + yc_b + skip) / 2) * silu(z), the scan outputs expanded over `cols`; ln_w == NULL
 * skips the norm (use_norm_after_ssm=False).  mean/rstd (batch*L) fp32 are saved for backward, which
 * rebuilds the normalised value from skip, yc, mean, rstd. */
int fv_mixer_combine_fwd(const void* xz, const void* skip, const float* yc, const float* ln_w,
                         const float* ln_b, float ln_eps, void* g, float* mean, float* rstd, int batch,
                         int rows, int cols, int tok_stride_row, int tok_stride_col, int tokens_per_patch,
                         int d_inner, int dtype, fv_stream_t stream);

/* ---- backward of the fused mixer middle --------------------------------------------
 * Number of persistent blocks a row-walking backward kernel launches (which = 0: combine_bwd,
 * 1: conv_pool_bwd); their `partials` buffers are (blocks, 2*d_inner) and (blocks, 12*d_inner) fp32. */
int fv_mixer_bwd_blocks(int batch, int rows, int d_inner, int tokens_per_patch, int which);

/* Launch plan of one of the mixer's four row-kernel families for a shape -- what the launchers themselves ask before
 * they launch (host code only, no HIP call: usable without a GPU).
 *   family: 0 fv_mixer_conv_pool_fwd, 1 fv_mixer_combine_fwd, 2 fv_mixer_combine_bwd, 3 fv_mixer_conv_pool_bwd(2)
 *   cols  : patch columns of a pooling row;  pool_max, dtype as in the launch
 *   plan[8] <- { form, vec, waves, slabs, row_groups, lds_bytes, takes_dxc2, 0 }
 *     form       0 unsupported (the launch returns an error), 1 generic tile / streaming kernel, 2 whole-row kernel
 *                (14 / 16 columns), 3 cell walker (tokens_per_patch 8, long dense rows), 4 wave-per-token kernel
 *     vec        channels per lane;  waves: channel waves of a block per row group;  slabs: blocks that cover d_inner
 *                (slabs * waves * 64 * vec == d_inner for a multiple of 64);  row_groups: pooling rows a block walks at
 *                a time (waves * row_groups * 64 threads);  lds_bytes: LDS of a block
 *     takes_dxc2 family 3: the form takes the second pooled-gradient addend of fv_mixer_conv_pool_bwd2 */
int fv_mixer_plan(int family, int batch, int rows, int cols, int tokens_per_patch, int d_inner, int pool_max, int dtype,
                  int* plan);

/* Adjoint of the LayerNorm + gate of fv_mixer_combine_fwd; the normalised value is rebuilt from the saved
 * skip, yc, mean, rstd.  dg: gradient wrt g.
 * Writes dz into the z half of dxz (batch, L, 2*d_inner), d_o (batch, L, d_inner) = gradient wrt the
 * averaged pre-norm value, dyc (batch, rows, d_inner) fp32 = 0.5 * sum_j d_o (gradient wrt BOTH
 * directions' scan outputs), and per-block partials [d ln_w (d_inner) | d ln_b (d_inner)]. */
int fv_mixer_combine_bwd(const void* dg, const void* xz, const void* skip, const float* yc,
                         const float* ln_w, const float* ln_b, const float* mean, const float* rstd,
                         void* dxz, void* d_o, float* dyc, float* partials, int batch, int rows, int cols, int tok_stride_row,
                         int tok_stride_col, int tokens_per_patch, int d_inner, int dtype, fv_stream_t stream);

/* Adjoint of fv_mixer_scan_fwd with the dt_proj adjoint fused in (replaces
 * selective_scan_cuda.bwd + the einsums of selective_scan_interface.py:698-723).
 *   dyc    (batch, Lc, d_inner) fp32          in
 *   dxc    (2, batch, Lc, d_inner) fp32       out: gradient wrt xc through the scan input u
 *   dx_dbl (fv_mixer_scan_bwd_chunks, 2, batch*Lc, dt_rank+2*d_state) fp32 out: sum over chunks
 *          = gradient wrt x_dbl
 *   ckpt   fv_mixer_scan_bwd_ckpt_floats() fp32 scratch
 *   partials (batch, 2, d_inner*(d_state + dt_rank + 1)): per-batch partials, per direction the
 *          segments [dA_log (d_inner*d_state) | d dt_proj.weight (d_inner*dt_rank) | d dt_proj.bias (d_inner)]
 *          (sum over batch with fv_reduce_partials). */
int fv_mixer_scan_bwd_chunks(int d_inner, int Lc, int dt_rank);
/* the same for a given batch: long pooled lengths pick the channel-chunk width by how many workgroups the launch has
 * (fv_mixer_scan_bwd_chunks answers for a large batch); size dx_dbl with this one */
int fv_mixer_scan_bwd_chunks_b(int batch, int d_inner, int Lc, int dt_rank);
/* rows of the `partials` buffer of fv_mixer_scan_bwd: (rows, 2, d_inner*(d_state + dt_rank + 1)) fp32 */
int fv_mixer_scan_bwd_partials(int batch, int Lc, int dt_rank);
size_t fv_mixer_scan_bwd_ckpt_floats(int batch, int Lc, int d_inner, int d_state, int dt_rank);
int fv_mixer_scan_bwd(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias,
                      const float* A_log, const float* dt_w_b, const float* dt_bias_b, const float* A_log_b,
                      const float* dyc, float* dxc, float* dx_dbl, float* ckpt, float* partials, int batch,
                      int Lc, int d_inner, int dt_rank, int d_state, int dtype, fv_stream_t stream);
/* Same with one output gradient per direction: dyc_per_direction != 0 -> dyc is (2, batch, Lc, d_inner).  The MAE
 * masked mixer needs it: its two branches gather different rows per token
 * (mamba_simple_masked_faster.py:281-283, 311-314), so their pooled gradients differ. */
int fv_mixer_scan_bwd_dir(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias,
                          const float* A_log, const float* dt_w_b, const float* dt_bias_b, const float* A_log_b,
                          const float* dyc, int dyc_per_direction, float* dxc, float* dx_dbl, float* ckpt,
                          float* partials, int batch, int Lc, int d_inner, int dt_rank, int d_state, int dtype,
                          fv_stream_t stream);
/* Same; ckpt_given != 0: `ckpt` holds the checkpoints written by fv_mixer_scan_fwd_ckpt for the same inputs (read, not
 * scratch).  Pooled lengths above 16 take the chunked kernel (16-step chunks, states of a chunk recomputed into
 * registers from its checkpoint); without given checkpoints it derives them with a forward sweep of its own. */
int fv_mixer_scan_bwd_ckpt(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias,
                           const float* A_log, const float* dt_w_b, const float* dt_bias_b, const float* A_log_b,
                           const float* dyc, int dyc_per_direction, float* dxc, float* dx_dbl, float* ckpt,
                           int ckpt_given, float* partials, int batch, int Lc, int d_inner, int dt_rank, int d_state,
                           int dtype, fv_stream_t stream);
/* Segment-parallel form of the same (long sequences on few batch elements, ckpt_given != 0 only: the un-pooled Vim baseline at
 * high resolution): the adjoint recurrence is linear in the adjoint state like the forward one in the state, so the
 * segments of fv_mixer_scan_fwd_seg are walked side by side here too -- adjoint states reached from zero, a serial combine
 * last segment to first, then the backward kernel proper per segment.  seg_ws: fv_mixer_scan_bwd_seg_floats() fp32 (0: one
 * segment, pass NULL); partials then has fv_mixer_scan_bwd_seg_partials() rows (one per batch element and segment). */
int fv_mixer_scan_bwd_segments(int batch, int Lc, int d_inner, int dt_rank);
size_t fv_mixer_scan_bwd_seg_floats(int batch, int Lc, int d_inner, int d_state, int dt_rank);
int fv_mixer_scan_bwd_seg_partials(int batch, int Lc, int d_inner, int dt_rank);
/* slices of dx_dbl (one per channel chunk) of the launch fv_mixer_scan_bwd_seg makes: with a segment workspace the
 * 64-channel workgroups of the segment-parallel form, without it fv_mixer_scan_bwd_chunks_b() */
int fv_mixer_scan_bwd_seg_chunks(int batch, int d_inner, int Lc, int dt_rank, int seg_ws_given);
int fv_mixer_scan_bwd_seg(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias, const float* A_log,
                          const float* dt_w_b, const float* dt_bias_b, const float* A_log_b, const float* dyc,
                          int dyc_per_direction, float* dxc, float* dx_dbl, float* ckpt, int ckpt_given, float* partials,
                          float* seg_ws, int batch, int Lc, int d_inner, int dt_rank, int d_state, int dtype,
                          fv_stream_t stream);

/* fv_mixer_scan_bwd for the short pooled lengths WITH the data half of the x_proj adjoint folded in (reference:
 * selective_scan_interface.py:679-696 + 726-734, `dx = dx_dbl @ x_proj.weight` added to the scan's d u).  Built for
 * Lc in {14, 16}, d_inner == 384 (two 192-channel chunks), dt_rank <= 12: ask fv_mixer_scan_bwd_xproj_ok.
 *   x_proj_w, x_proj_w_b (dt_rank + 2 * d_state, d_inner) fp32: the weights as stored
 *   x_proj_w2_bf16 (2, dt_rank + 2 * d_state, d_inner) bf16: the two, rounded -- required for bf16 storage, where the
 *        product is taken on the bf16 matrix cores from bf16(d x_dbl) and these (the operands of the reference's autocast
 *        backward); fp32 storage multiplies the fp32 weights exactly and ignores it (may be NULL)
 *   dxc  (2, batch, Lc, d_inner) fp32: d u through the scan + (this chunk's partial d x_dbl) @ Wx, own channels
 *   dxc2 (2, batch, Lc, d_inner) storage dtype: the same product for the OTHER chunk's channels; the total gradient of
 *        the pooled conv output is dxc + dxc2 (fv_mixer_conv_pool_bwd2 adds them)
 *   dx_dbl (2, 2, batch * Lc, W) fp32: per-chunk partial rows (fv_chunk_rows_bf16 sums them for the weight gradient)
 *   partials: fv_mixer_scan_bwd_partials() rows, as for fv_mixer_scan_bwd.  Deterministic. */
int fv_mixer_scan_bwd_xproj_ok(int batch, int Lc, int d_inner, int dt_rank, int dtype);
int fv_mixer_scan_bwd_xproj(const void* xc, const void* x_dbl, const float* dt_w, const float* dt_bias, const float* A_log,
                            const float* dt_w_b, const float* dt_bias_b, const float* A_log_b, const float* dyc,
                            const float* x_proj_w, const float* x_proj_w_b, const void* x_proj_w2_bf16, float* dxc,
                            void* dxc2, float* dx_dbl, float* partials, int batch, int Lc, int d_inner, int dt_rank,
                            int d_state, int dtype, fv_stream_t stream);
/* outs[j] (rows, WP) bf16 = sum over nchunks of partials[j] (nchunks, rows, width) fp32, WP = width rounded up to 8, pad
 * columns zero; up to 64 jobs of one shape in one launch (host arrays of device pointers).  The rows
 * fv_mixer_xproj_bwd2 publishes, bit for bit. */
int fv_chunk_rows_bf16(const float* const* partials, void* const* outs, int njobs, int nchunks, long rows, int width,
                       fv_stream_t stream);

/* ---- MAE masked mixer: kept tokens <-> pooling rows --------------------------
 * Replaces compute_row_means_constantdivide (index_add_ over the kept tokens, divide by cols;
 * mamba_simple_masked_faster.py:376-416) and the torch.gather that expands the scan output back to the kept tokens
 * (:281-283, 311-314), plus their adjoints -- the adjoint of one is the other.  Deterministic (no atomics).
 *   idx (2, batch, n_tokens) int32: pooling row of token t, per direction; values outside [0, rows) contribute /
 *       receive nothing.
 * fv_rows_segment_sum: out[dir][b][r][:] = scale * sum_{t : idx[dir][b][t] == r} in[dir][b][t][:]
 *   in  (2, batch, n_tokens, d_inner), or (batch, n_tokens, d_inner) shared by both directions when
 *       in_per_direction == 0;   out (2, batch, rows, d_inner).
 * fv_rows_gather: out[dir][b][t][:] = scale * in[dir][b][idx[dir][b][t]][:]
 *   in  (2, batch, rows, d_inner);   out (2, batch, n_tokens, d_inner).
 * dtypes FV_F32 / FV_BF16 per tensor; d_inner a multiple of 4. */
int fv_rows_segment_sum(const void* in, int in_dtype, int in_per_direction, const int* idx, void* out, int out_dtype,
                        int batch, int n_tokens, int rows, int d_inner, float scale, fv_stream_t stream);
int fv_rows_gather(const void* in, int in_dtype, const int* idx, void* out, int out_dtype, int batch, int n_tokens,
                   int rows, int d_inner, float scale, fv_stream_t stream);

/* Adjoint of fv_mixer_conv_pool_fwd plus the D-skip path: consumes d_o and the total gradient
 * wrt the pooled conv output dxc (2, batch, rows, d_inner) fp32; writes dx into the x half of
 * dxz and per-block partials [d conv_w (d_inner*4) | d conv_w_b (d_inner*4) | d conv_b | d conv_b_b |
 * dD | dD_b] (12*d_inner floats).  pool_max != 0: `amax` is the argmax tensor the forward wrote; the
 * pooled gradient goes to that column only (autograd of `.max(dim).values`, mamba_simple_faster.py:299-305). */
int fv_mixer_conv_pool_bwd(const void* xz, const void* d_o, const float* dxc, const float* conv_w,
                           const float* conv_b, const float* conv_w_b, const float* conv_b_b, const float* D,
                           const float* D_b, const void* amax, void* dxz, float* partials, int batch, int rows,
                           int cols, int tok_stride_row, int tok_stride_col, int tokens_per_patch, int d_inner,
                           int d_conv, int pool_max, float scaling_factor, int dtype, fv_stream_t stream);

/* Same, with the pooled gradient given as two addends: dxc (fp32) + dxc2 (storage dtype, nullable) -- the form
 * fv_mixer_scan_bwd_xproj produces.  dxc2 is taken by the whole-row kernel only: mean pooling, tokens_per_patch 1,
 * 14 or 16 columns, d_inner a multiple of 128 (fv_mixer_conv_pool_bwd2_ok). */
int fv_mixer_conv_pool_bwd2_ok(int rows, int cols, int tokens_per_patch, int d_inner, int pool_max);
int fv_mixer_conv_pool_bwd2(const void* xz, const void* d_o, const float* dxc, const void* dxc2, const float* conv_w,
                            const float* conv_b, const float* conv_w_b, const float* conv_b_b, const float* D,
                            const float* D_b, const void* amax, void* dxz, float* partials, int batch, int rows,
                            int cols, int tok_stride_row, int tok_stride_col, int tokens_per_patch, int d_inner,
                            int d_conv, int pool_max, float scaling_factor, int dtype, fv_stream_t stream);

/* out[i] (+)= sum_{s < n_partials} partials[s*n + i], fixed order (deterministic); accumulate != 0
 * adds into `out` (gradient accumulation straight into a parameter's .grad). */
int fv_reduce_partials(const float* partials, float* out, int n_partials, size_t n, int accumulate,
                       fv_stream_t stream);
/* Up to 208 such reductions in one launch (host arrays of device pointers / sizes; at most 65 535 partials of fewer
 * than 2^32 elements each; 96 until round 6). */
int fv_reduce_partials_multi(const float* const* partials, float* const* outs, const int* n_partials,
                             const size_t* ns, int njobs, int accumulate, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused (per-sample scale) + residual add + RMSNorm / LayerNorm over the last dim.
 * Replaces the Triton kernels behind rms_norm_fn / layer_norm_fn
 *   (mamba-1p1p1/mamba_ssm/ops/triton/layernorm.py:66-121 fwd, 210-304 bwd; host 124-191, 307-399).
 *   r = x * row_scale[row / rows_per_scale] + residual   (row_scale, residual nullable)
 *   residual_out = r (nullable);  y = norm(r) * weight (+ bias)
 * x, residual, y, residual_out: (M, N) with independent storage dtypes (FV_F32 / FV_BF16);
 * weight, bias: (N) fp32; mean (LayerNorm only), rstd: (M) fp32.  N % 4 == 0, N <= 2048.
 * ---------------------------------------------------------------------- */
int fv_add_norm_blocks(int M);   /* rows of the (blocks, N) partial_dw / partial_db buffers */
int fv_add_norm_fwd(const void* x, int x_dtype, const void* residual, int residual_dtype,
                    const float* weight, const float* bias, const float* row_scale, int rows_per_scale,
                    void* y, int y_dtype, void* residual_out, int residual_out_dtype, float* mean,
                    float* rstd, int M, int N, float eps, int is_rms_norm, fv_stream_t stream);
/* r: the saved residual_out.  dresidual_in = d r (nullable), dx = d r * row_scale (nullable);
 * partial_dw/partial_db: per-block partial sums, reduce with fv_reduce_partials. */
int fv_add_norm_bwd(const void* dy, int dy_dtype, const void* dresidual_out, int dresidual_out_dtype,
                    const void* r, int r_dtype, const float* weight, const float* mean, const float* rstd,
                    const float* row_scale, int rows_per_scale, void* dx, int dx_dtype, void* dresidual_in,
                    int dresidual_in_dtype, float* partial_dw, float* partial_db, int M, int N,
                    int is_rms_norm, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * LayerNorm over C with an NCHW side: the dense-prediction (detection / segmentation) kernels (csrc/chan_ln.hip).
 *
 * Feature tap (models/fastvim.py:682-690, outnorm_i + view(-1, H, W, C).permute(0, 3, 1, 2).contiguous()):
 *   x (B, L, C) token-major, FV_F32 / FV_BF16, L = H * W, token l = cell (l / W, l % W);
 *   y (B, C, L) fp32 = weight[c] * (x - mean) * rstd + bias[c], statistics over C in fp32; mean, rstd (B * L) fp32.
 *   C % 4 == 0, 4 <= C <= 1024; x, y, dy, dx, weight, bias 16-byte aligned (any L: plane bases may be unaligned).
 * Backward: dy (B, C, L) fp32 -> dx (B, L, C) in x's dtype; partial_dw / partial_db (fv_tap_ln_blocks(B, L), C):
 *   one row per workgroup, reduce with fv_reduce_partials.
 *
 * LN2d (detection/vitdet/simple_fpn.py:15-32): x, y, dy, dx contiguous (N, C, HW) of one dtype (FV_F32 / FV_BF16),
 *   y = weight[c] * (x - mean) * rstd + bias[c] with mean / rstd over C per (n, position), saved as (N * HW) fp32.
 *   1 <= C <= 1024, any HW >= 1; partial rows: (fv_ln2d_blocks(N, C, HW), C).
 * The *_blocks queries are host-only and return 0 for shapes the launches refuse.
 * ---------------------------------------------------------------------- */
int fv_tap_ln_blocks(int B, int L);
int fv_tap_ln_fwd(const void* x, int x_dtype, const float* weight, const float* bias, float* y, float* mean,
                  float* rstd, int B, int L, int C, float eps, fv_stream_t stream);
int fv_tap_ln_bwd(const float* dy, const void* x, int x_dtype, const float* weight, const float* mean,
                  const float* rstd, void* dx, float* partial_dw, float* partial_db, int B, int L, int C,
                  fv_stream_t stream);
int fv_ln2d_blocks(int N, int C, int HW);
int fv_ln2d_fwd(const void* x, int dtype, const float* weight, const float* bias, void* y, float* mean, float* rstd,
                int N, int C, int HW, float eps, fv_stream_t stream);
int fv_ln2d_bwd(const void* dy, const void* x, int dtype, const float* weight, const float* mean, const float* rstd,
                void* dx, float* partial_dw, float* partial_db, int N, int C, int HW, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * bf16 MFMA GEMM  C[M][N] = sum_k A(m,k) B(k,n) (+ bias[n]), fp32 accumulate.
 * Replaces the cuBLAS GEMMs behind in_proj / out_proj (mamba_simple_faster.py:189-193, 435-444),
 * the patch-embed Conv2d (models/fastvim.py:95, k == stride) and their autograd adjoints.
 *   a_k_slow = 0: A(m,k) = A[m*lda + k]      a_k_slow = 1: A(m,k) = A[k*lda + m]
 *   b_k_slow = 0: B(k,n) = B[n*ldb + k]      b_k_slow = 1: B(k,n) = B[k*ldb + n]
 *   (0,0) activations x weight^T;  (0,1) data gradient with the weight as stored;  (1,1) weight
 *   gradient X^T Y.  splits > 1 cuts K across grid.z and writes `splits` fp32 partials (stride
 *   M*ldc) for fv_reduce_partials.  C is bf16 (c_fp32 = 0) or fp32; bias (N) fp32 nullable.
 * ---------------------------------------------------------------------- */
int fv_gemm_bf16(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda,
                 long ldb, long ldc, int a_k_slow, int b_k_slow, int c_fp32, int splits, fv_stream_t stream);

/* The kernel fv_gemm_bf16 launches for these arguments, without launching it -- the answer of the ONE function the launch
 * itself asks (a test names the kernel it means and asserts it before it runs).  Returns FV_GEMM_KIND_*, or the negative
 * code with which fv_gemm_bf16 refuses the shape (pointers, their alignment and lda / ldb are not part of the question).
 * has_bias: a bias pointer would be given; rb_period > 0: the call is fv_gemm_bf16_rowbias with that period.  cus: the CU
 * count the rules that count workgroup rounds are asked for, 0 = the current device (256 where there is none).  tile_m /
 * tile_n / lds_dma (nullable) receive the tile's extents and whether the operands are staged by LDS-DMA (1) or through
 * registers (0).  A tuning build's extra tile shapes answer 100 + the value of their hook. */
enum {
  FV_GEMM_KIND_STREAM = 0,             /* persistent streaming kernel, 128 x 192 tiles of trimmed height */
  FV_GEMM_KIND_PHASED_TILE = 1,        /* phased 256 x 256 kernel, one workgroup per tile */
  FV_GEMM_KIND_PHASED_PERSISTENT = 2,  /* phased 256 x 256 kernel, one persistent workgroup per CU */
  FV_GEMM_KIND_WAVE8_256 = 3,          /* 256 x 256 tiles on eight waves */
  FV_GEMM_KIND_160x128 = 4,
  FV_GEMM_KIND_128x96 = 5,
  FV_GEMM_KIND_128x192 = 6,
  FV_GEMM_KIND_128x128 = 7             /* the only kind with both staging forms */
};
int fv_gemm_bf16_plan(int M, int N, int K, int a_k_slow, int b_k_slow, int c_fp32, int has_bias, int rb_period, long ldc,
                      int splits, int cus, int* tile_m, int* tile_n, int* lds_dma);

/* fp32-MFMA GEMM (v_mfma_f32_16x16x4_f32), batched:  C_b[M][N] = sum_k A_b(m,k) B_b(k,n) (+ bias[n]),  b < batch.
 * The projections in the reference's DEFAULT precision (fp32, imagenet_classification/train.py:17) -- F.linear / matmul /
 * bmm behind in_proj, x_proj, out_proj, patch embed, head and their adjoints (mamba_simple_faster.py:189-193, 321-327,
 * 435-444; models/fastvim.py:95, 537) -- and every shape fv_gemm_bf16 does not take (odd extents, unaligned rows).
 * Operand layouts as fv_gemm_bf16 (a_k_slow / b_k_slow); operands FV_F32 or FV_BF16 (widened exactly), C FV_F32 or
 * FV_BF16, fp32 accumulate in K order; any M, N, K, leading dimensions and alignment.  Batch b uses A + b*strideA,
 * B + b*strideB, C + b*strideC (elements): both scan directions of x_proj in one launch, or the K slices of a deterministic
 * split-K weight gradient (C = fp32 partials for fv_reduce_partials). */
int fv_gemm_f32(const void* A, int a_dtype, const void* B, int b_dtype, void* C, int c_dtype, const float* bias, int M,
                int N, int K, long lda, long ldb, long ldc, int a_k_slow, int b_k_slow, int batch, long strideA,
                long strideB, long strideC, fv_stream_t stream);

/* out_proj fused with the NEXT block's residual add + RMSNorm (mamba_simple_faster.py:435-444 followed by
 * models/fastvim.py:168-190 / layernorm.py:66-121):
 *   h = bf16_round(A W^T);  r = residual + row_scale[row / rows_per_scale] * h;  residual_out = r (fp32);
 *   rstd[row] = rsqrt(mean_n r^2 + eps);  y = bf16(r * rstd * norm_weight)
 * -- bit for bit fv_gemm_bf16 (bf16 C) followed by fv_add_norm_fwd (is_rms_norm), without writing and re-reading h.
 * A (M, K) bf16, W (N, K) bf16, residual / residual_out (M, N) fp32, row_scale nullable.  Built for N == 192 and
 * K % 64 == 0 (a workgroup owns whole rows); returns FV_ERR_UNSUPPORTED otherwise and the caller runs the two calls. */
int fv_gemm_bf16_addnorm(const void* A, const void* W, const float* residual, const float* norm_weight,
                         const float* row_scale, int rows_per_scale, void* y, float* residual_out, float* rstd, int M,
                         int N, int K, long lda, long ldw, float eps, fv_stream_t stream);

/* in_proj data gradient fused with the SAME block's RMSNorm + residual-add adjoint (mamba_simple_faster.py:189-193
 * backward followed by ops/triton/layernorm.py:210-304): d y = bf16_round(A W) (A (M, K) bf16 = d xz, W (K, N) bf16 =
 * in_proj.weight as stored); then exactly fv_add_norm_bwd(is_rms_norm) on it: d residual_in = rstd (d y w - xhat mean(d y
 * w xhat)) + d residual_out (fp32), d x = d residual_in * row_scale (bf16), partial_dw (fv_gemm_bf16_dgrad_addnorm_blocks(M),
 * N): per-workgroup sums of d y * xhat (reduce with fv_reduce_partials).  The data gradient itself never reaches HBM.
 * N == 192, K % 64 == 0; FV_ERR_UNSUPPORTED otherwise. */
int fv_gemm_bf16_dgrad_addnorm_blocks(int M);
int fv_gemm_bf16_dgrad_addnorm_bwd(const void* A, const void* W, const float* dresidual_out, const float* r,
                                   const float* rstd, const float* norm_weight, const float* row_scale,
                                   int rows_per_scale, void* dx, float* dresidual_in, float* partial_dw, int M, int N,
                                   int K, long lda, long ldw, fv_stream_t stream);

/* The same with a second GEMM phase: C2 (M, N2) bf16 = d x @ W2, W2 (N, N2) bf16 row-major -- the PREVIOUS block's out_proj
 * data gradient (d g = d x @ out_proj.weight), computed from the d x tile while it is still in LDS; bit-identical to
 * fv_gemm_bf16(b_k_slow = 1) on d x.  W2 null: no second phase.  N2 % 128 == 0. */
int fv_gemm_bf16_dgrad_addnorm_bwd2(const void* A, const void* W, const float* dresidual_out, const float* r,
                                    const float* rstd, const float* norm_weight, const float* row_scale,
                                    int rows_per_scale, void* dx, float* dresidual_in, float* partial_dw, int M, int N,
                                    int K, long lda, long ldw, const void* W2, void* C2, int N2, long ldw2,
                                    fv_stream_t stream);

/* fv_mixer_combine_fwd + fv_gemm_bf16_addnorm in ONE launch (round 5): the gated activations g of a block are produced
 * tile by tile inside the out_proj GEMM that also does the NEXT block's DropPath scale + residual add + RMSNorm
 * (reference: mamba_simple_faster.py:356, 412-414, 434-444; models/fastvim.py:168-190).  g (batch, L, 384) bf16, mean /
 * rstd_ln (batch * L) are written for the backward pass exactly as fv_mixer_combine_fwd writes them; y / residual_out /
 * rstd exactly as fv_gemm_bf16_addnorm does from that g.  Built for bf16, d_inner 384, d_model 192, tokens_per_patch 1
 * (fv_mixer_combine_out_proj_addnorm_ok); W (192, ldw) bf16 row-major = out_proj.weight. */
int fv_mixer_combine_out_proj_addnorm_ok(int batch, int rows, int cols, int tokens_per_patch, int d_inner, int d_model,
                                         int dtype);
int fv_mixer_combine_out_proj_addnorm(const void* xz, const void* skip, const float* yc, const float* ln_w,
                                      const float* ln_b, float ln_eps, void* g, float* mean, float* rstd_ln, int batch,
                                      int rows, int cols, int tok_stride_row, int tok_stride_col, const void* W, long ldw,
                                      const float* residual, const float* norm_weight, const float* row_scale,
                                      int rows_per_scale, void* y, float* residual_out, float* rstd, float eps,
                                      fv_stream_t stream);
/* The same launch with W given as the FRAGMENT-MAJOR copy of out_proj.weight (fv_pack_weight_frags_batched, K = 384;
 * ldw must be 384): every load of the weight stream reads 1 KiB contiguous.  Only load addresses differ: all outputs are
 * bit-identical to fv_mixer_combine_out_proj_addnorm on the plain weight. */
int fv_mixer_combine_out_proj_addnorm_pk(const void* xz, const void* skip, const float* yc, const float* ln_w,
                                         const float* ln_b, float ln_eps, void* g, float* mean, float* rstd_ln, int batch,
                                         int rows, int cols, int tok_stride_row, int tok_stride_col, const void* W,
                                         long ldw, const float* residual, const float* norm_weight,
                                         const float* row_scale, int rows_per_scale, void* y, float* residual_out,
                                         float* rstd, float eps, fv_stream_t stream);

/* fv_mixer_conv_pool_bwd2 + fv_gemm_bf16_dgrad_addnorm_bwd2 in ONE launch (round 6): the backward mirror of
 * fv_mixer_combine_out_proj_addnorm.  A workgroup owns four pooling rows of one image: it runs the conv + pool adjoint on
 * them (reference: FastVim_MambaInnerFnNoOutProj_withoutZ.backward, selective_scan_interface.py:607-776 -- causal_conv1d_bwd
 * of both directions, the mean-pool adjoint, the D-skip adjoint), writes the x half of dxz (batch, L, 768) once -- the
 * in_proj weight gradient reads it -- and keeps it in LDS as the A operand of the in_proj data gradient
 * `dxz @ in_proj.weight` (mamba_simple_faster.py:189-193; the z half of dxz, written by fv_mixer_combine_bwd, is read
 * here), whose epilogue is the block's residual add + RMSNorm adjoint (models/fastvim.py:168-190) and whose second phase
 * is the previous block's out_proj data gradient C2 = dx @ W2 -- arguments from `W_in_t` on as in
 * fv_gemm_bf16_dgrad_addnorm_bwd2, except that the weight is given TRANSPOSED: W_in_t (192, ldwt) bf16 row-major =
 * in_proj.weight^T (fv_transpose_bf16_batched), so that a lane's MFMA fragment is 16 contiguous bytes.
 * conv_partials (fv_mixer_conv_pool_bwd_dgrad_blocks(batch, rows), 12 * 384) and partial_dw (same row count, 192) are
 * per-workgroup partial rows for fv_reduce_partials: [dw | dw_b | db | db_b | dD | dD_b] as fv_mixer_conv_pool_bwd writes
 * them, and the norm weight's gradient.  dx / dresidual_in / C2 and the x half of dxz are bit-identical to the two
 * launches' (tests/test_convpool_dgrad_gpu.py); the parameter-gradient sums group rows differently (fp32 rounding).
 * Built for bf16, d_inner 384, d_model 192, cols 14 or 16, tokens_per_patch 1, mean pooling
 * (fv_mixer_conv_pool_bwd_dgrad_ok). */
int fv_mixer_conv_pool_bwd_dgrad_ok(int batch, int rows, int cols, int tokens_per_patch, int d_inner, int d_model,
                                    int pool_max, int dtype);
int fv_mixer_conv_pool_bwd_dgrad_blocks(int batch, int rows);
int fv_mixer_conv_pool_bwd_dgrad(const void* xz, const void* dskip, const float* dxc, const void* dxc2,
                                 const float* conv_w, const float* conv_b, const float* conv_w_b, const float* conv_b_b,
                                 const float* D, const float* D_b, void* dxz, float* conv_partials, int batch, int rows,
                                 int cols, int tok_stride_row, int tok_stride_col, float scaling, const void* W_in_t,
                                 long ldwt, const float* dresidual_out, const float* r, const float* rstd,
                                 const float* norm_weight, const float* row_scale, int rows_per_scale, void* dx,
                                 float* dresidual_in, float* partial_dw, const void* W2, void* C2, int N2, long ldw2,
                                 fv_stream_t stream);
/* The same launch with W_in_t given as the FRAGMENT-MAJOR copy of in_proj.weight^T (fv_pack_weight_frags_batched,
 * K = 768; ldwt must be 768).  Only load addresses differ: every output, the partial rows included, is bit-identical to
 * fv_mixer_conv_pool_bwd_dgrad on the plain transposed weight.  W2 stays plain. */
int fv_mixer_conv_pool_bwd_dgrad_pk(const void* xz, const void* dskip, const float* dxc, const void* dxc2,
                                    const float* conv_w, const float* conv_b, const float* conv_w_b,
                                    const float* conv_b_b, const float* D, const float* D_b, void* dxz,
                                    float* conv_partials, int batch, int rows, int cols, int tok_stride_row,
                                    int tok_stride_col, float scaling, const void* W_in_t, long ldwt,
                                    const float* dresidual_out, const float* r, const float* rstd,
                                    const float* norm_weight, const float* row_scale, int rows_per_scale, void* dx,
                                    float* dresidual_in, float* partial_dw, const void* W2, void* C2, int N2, long ldw2,
                                    fv_stream_t stream);
/* ... and with W2 given as the FRAGMENT-MAJOR copy of the previous block's out_proj.weight for the product in which its
 * rows are k (fv_pack_weight_frags_w2_batched).  W2 and C2 not null, N2 == 384, ldw2 == 384 (no row padding).  The second
 * phase then streams W2 from L2 into MFMA operand registers, each wave for 96 columns of C2 and all 64 tile rows; same
 * operands, k order and accumulation chains: every output is bit-identical to the two launches above. */
int fv_mixer_conv_pool_bwd_dgrad_pk2(const void* xz, const void* dskip, const float* dxc, const void* dxc2,
                                     const float* conv_w, const float* conv_b, const float* conv_w_b,
                                     const float* conv_b_b, const float* D, const float* D_b, void* dxz,
                                     float* conv_partials, int batch, int rows, int cols, int tok_stride_row,
                                     int tok_stride_col, float scaling, const void* W_in_t, long ldwt,
                                     const float* dresidual_out, const float* r, const float* rstd,
                                     const float* norm_weight, const float* row_scale, int rows_per_scale, void* dx,
                                     float* dresidual_in, float* partial_dw, const void* W2, void* C2, int N2, long ldw2,
                                     fv_stream_t stream);

/* dsts[j] (cols, rows) bf16 = srcs[j] (rows, cols)^T for up to 64 equal-shape matrices in one launch: the transposed
 * bf16 shadows of in_proj.weight that fv_mixer_conv_pool_bwd_dgrad reads (refreshed once per optimizer step). */
int fv_transpose_bf16_batched(const void* const* srcs, void* const* dsts, int njobs, int rows, int cols,
                              fv_stream_t stream);

/* Fragment-major copies of up to 64 weights in one launch.  srcs[j] is (192, K) bf16 with K contiguous, K = 384
 * (out_proj.weight as stored) or 768 (in_proj.weight^T); dsts[j] holds the same 192 K elements in 16-byte units:
 *   unit ((wv * K / 32 + ks) * 3 + nb) * 64 + lane  =  srcs[j][48 wv + 16 nb + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8)
 * (wv 0..3, ks 0..K/32-1, nb 0..2, lane 0..63) -- the MFMA operand lane `lane` of wave wv loads for column block nb at
 * k step ks in the _pk launches above.  Both sides 16-byte aligned, no aliasing.  Refreshed once per optimizer step. */
int fv_pack_weight_frags_batched(const void* const* srcs, void* const* dsts, int njobs, int K, fv_stream_t stream);

/* Fragment-major copies of up to 64 weights (192, 384) bf16 row-major whose ROWS are k (out_proj.weight as the operand of
 * its data gradient), in one launch; dsts[j] holds the same elements in 16-byte units:
 *   unit ((wv * 6 + ks) * 6 + nb) * 64 + lane  =  srcs[j][32 ks + 8 (lane >> 4) + j'][96 wv + 16 nb + (lane & 15)], j' = 0..7
 * (wv 0..3, ks 0..5, nb 0..5, lane 0..63) -- the MFMA operand lane `lane` of wave wv feeds for column block nb at k step
 * ks in the second phase of fv_mixer_conv_pool_bwd_dgrad_pk2.  dsts 16-byte aligned, no aliasing. */
int fv_pack_weight_frags_w2_batched(const void* const* srcs, void* const* dsts, int njobs, fv_stream_t stream);

/* Fragment-major copies of up to 64 weights (N, 192) bf16 row-major, N a multiple of 384, whose rows are OUTPUT COLUMNS of a
 * forward product (in_proj.weight), in one launch; dsts[j] holds the same elements in 16-byte units:
 *   unit (((p * 4 + wv) * 6 + ks) * 6 + nb) * 64 + lane  =  srcs[j][384 p + 96 wv + 16 nb + (lane & 15)][32 ks + 8 (lane >> 4) .. + 8)
 * (p 0..N/384-1, wv 0..3, ks 0..5, nb 0..5, lane 0..63) -- the MFMA operand lane `lane` of wave wv loads for column block nb
 * at k step ks of pass p in fv_gemm_bf16_inproj_pk.  Both sides 16-byte aligned, no aliasing. */
int fv_pack_weight_frags_in_batched(const void* const* srcs, void* const* dsts, int njobs, int N, fv_stream_t stream);

/* C (M, N) bf16 contiguous = A (M, 192) bf16 @ W^T with W (N, 192) given as W_pk, its fragment-major copy
 * (fv_pack_weight_frags_in_batched): one workgroup per tile of up to 64 rows, the tile in LDS, the weight streamed from L2
 * into MFMA operand registers.  Built for K == 192, N % 384 == 0, lda == K, 16-byte aligned operands, no bias: anything
 * else is an error (callers take fv_gemm_bf16).  rows_per_tile: 0 = the library's choice, 1..64 = rows of C per workgroup,
 * -1 = the rows dealt evenly over whole rounds of 2 x CU-count workgroups.  Same MFMA, operand order and k order as
 * fv_gemm_bf16: C is bit-identical to it, whatever rows_per_tile. */
int fv_gemm_bf16_inproj_pk(const void* A, const void* W_pk, void* C, int M, int N, int K, long lda, int rows_per_tile,
                           fv_stream_t stream);

/* fv_gemm_bf16_addnorm with a second GEMM phase: C2 (M, N2) bf16 = y @ W2^T, W2 (N2, N) bf16 row-major -- the block's
 * in_proj (mamba_simple_faster.py:189-193) computed from the normalised tile while it is still in LDS; bit-identical to
 * fv_gemm_bf16 on y.  W2 null: no second phase.  N2 % 128 == 0. */
int fv_gemm_bf16_addnorm2(const void* A, const void* W, const float* residual, const float* norm_weight,
                          const float* row_scale, int rows_per_scale, void* y, float* residual_out, float* rstd, int M,
                          int N, int K, long lda, long ldw, float eps, const void* W2, void* C2, int N2, long ldw2,
                          fv_stream_t stream);

/* Several weight gradients in one launch (queued until the end of the backward pass): problem i is
 * x_i (Kd_i, M_i)^T @ y_i (Kd_i, N_i) -> parts_i (splits_i, M_i, N_i) fp32 partials (sum with fv_reduce_partials);
 * the same arithmetic, tiling and fixed split order as fv_gemm_bf16(a_k_slow = b_k_slow = 1, c_fp32 = 1).
 * splits_i == -1: one K slice ADDED in place to the (M_i, N_i) fp32 matrix parts_i points at (the gradient itself; no
 * partial, nothing to reduce) -- for launches whose outputs are all multiples of 256 x 256 and at least 512 x 512, Kd_i a
 * multiple of 64 and >= 128; an error otherwise. */
int fv_gemm_bf16_tn_grouped(const void* const* x, const void* const* y, float* const* parts, const int* Kd,
                            const int* M, const int* N, const int* splits, int count, fv_stream_t stream);
/* Same with explicit row strides (elements) of x and y -- rows may be padded (ldx >= M, ldy >= N, multiples of 8; pad
 * elements must be finite): M and N then need not be multiples of 8.  ldx / ldy null: dense rows. */
int fv_gemm_bf16_tn_grouped_ld(const void* const* x, const void* const* y, float* const* parts, const int* Kd,
                               const int* M, const int* N, const int* ldx, const int* ldy, const int* splits, int count,
                               fv_stream_t stream);

/* Tile class the grouped launch runs an (M, N) weight gradient over Kd tokens on when every problem of the launch agrees:
 * 4 = 256 x 192 tiles, 5 = 192 x 256 tiles (eight waves; the d_model-384 outputs from 50 000 tokens on), 0 = not taken.  The
 * host groups problems per launch and picks their split-K factors by the same answer. */
int fv_gemm_bf16_tn_grouped_wide8(int M, int N, int Kd);

/* The plan of ONE launch of fv_gemm_bf16_tn_grouped_ld over these problems (1 .. 40 of them; the entry cuts a longer list
 * into balanced launches of at most 40), from the function the entry itself asks.  Arrays as the entry takes them (ldx /
 * ldy nullable).  Returns the tile class FV_GEMM_GROUPED_*, or the negative code with which the entry refuses the problems
 * on their shapes (splits = -1 off the phased form, a K that does not cut into whole tiles, ...).  lds_dma (nullable): 1 =
 * operands staged by LDS-DMA, 0 = through registers (128 x 128 only); phased (nullable): 1 = the phased 256 x 256 form. */
enum {
  FV_GEMM_GROUPED_128x128 = 0,
  FV_GEMM_GROUPED_128x192 = 1,
  FV_GEMM_GROUPED_192x128 = 2,
  FV_GEMM_GROUPED_256x256 = 3,         /* eight waves; phased when every slice has two K tiles or more */
  FV_GEMM_GROUPED_256x192 = 4,         /* eight waves: fv_gemm_bf16_tn_grouped_wide8 */
  FV_GEMM_GROUPED_192x256 = 5
};
int fv_gemm_bf16_tn_grouped_plan(const int* Kd, const int* M, const int* N, const int* ldx, const int* ldy,
                                 const int* splits, int count, int* lds_dma, int* phased);

/* x_proj of both directions, bf16: x_dbl (2, M, width) = xc (2, M, d_inner) @ x_proj_w2 (2, width, d_inner)^T, fp32
 * accumulate (mamba_simple_faster.py:321-327; the F.linear behind `self.x_proj` / `self.x_proj_b`).  M = batch*Lc,
 * width = dt_rank + 2*d_state <= 112, d_inner a multiple of 32. */
int fv_mixer_xproj_fwd(const void* xc, const void* x_proj_w2, void* x_dbl, int M, int d_inner, int width,
                       fv_stream_t stream);

/* Adjoint of x_proj for both directions, fused with the sum of the scan backward's chunk partials
 * (replaces the einsum/addmm chain of selective_scan_interface.py:698-734):
 *   dx_dbl = sum_c dx_dbl_partials[c];  dxc += dx_dbl @ W;  dW_partials[slice] = dx_dbl[slice]^T @ xc[slice].
 * dx_dbl_partials (nchunks, 2, M, width) fp32; xc (2, M, d_inner) storage dtype; W (width, d_inner) fp32;
 * dxc (2, M, d_inner) fp32 in/out; dW_partials (fv_mixer_xproj_bwd_slices(M), 2, width, d_inner) fp32.
 * Returns FV_ERR_UNSUPPORTED for a width that is not built (the host then uses library GEMMs). */
int fv_mixer_xproj_bwd_slices(int M);
int fv_mixer_xproj_bwd(const float* dx_dbl_partials, int nchunks, const void* xc, const float* x_proj_w,
                       const float* x_proj_w_b, float* dxc, float* dW_partials, int M, int d_inner, int width,
                       int dtype, fv_stream_t stream);
/* Same; `dx_dbl_bf16` (2, M, WP) bf16 with WP = width rounded up to 8 (pad columns zero), nullable, receives the
 * summed dx_dbl rows, and `dW_partials` may then be null: the weight gradient dx_dbl^T xc is left to a (grouped)
 * GEMM over exactly those bf16 rows -- what the reference's autocast backward multiplies
 * (selective_scan_interface.py:726-729). */
int fv_mixer_xproj_bwd2(const float* dx_dbl_partials, int nchunks, const void* xc, const float* x_proj_w,
                        const float* x_proj_w_b, float* dxc, float* dW_partials, void* dx_dbl_bf16, int M, int d_inner,
                        int width, int dtype, fv_stream_t stream);
/* The data half of fv_mixer_xproj_bwd2 (dW_partials == NULL; `dx_dbl_bf16` required) with the TRANSPOSED bf16 copy of both
 * weights, `x_proj_w_t_bf16` (2, d_inner, width): bf16(summed dx_dbl) @ bf16(weight) on the bf16 matrix cores, fp32
 * accumulate -- the operands of the reference's autocast backward (selective_scan_interface.py:726-734).  The product is
 * added to `dxc` (fp32, in place), or, with `dxc2_bf16` (2, M, d_inner) non-NULL, WRITTEN there in bf16 and `dxc` left alone
 * (the conv + pool adjoint then takes both: fv_mixer_conv_pool_bwd2).  Built where fv_mixer_xproj_bwd3_ok says so (bf16
 * storage, d_inner a multiple of 64 from 768 up, width 56 / 64 / 80 / 96 / 112); any other call, or a NULL transposed
 * weight, is fv_mixer_xproj_bwd2 with the fp32 weights (and refuses `dxc2_bf16`).  (Added in round 6; ABI version
 * unchanged: new symbols.) */
int fv_mixer_xproj_bwd3_ok(int M, int d_inner, int width, int dtype);
int fv_mixer_xproj_bwd3(const float* dx_dbl_partials, int nchunks, const void* xc, const float* x_proj_w,
                        const float* x_proj_w_b, const void* x_proj_w_t_bf16, float* dxc, void* dxc2_bf16,
                        void* dx_dbl_bf16, int M, int d_inner, int width, int dtype, fv_stream_t stream);

/* Soft-target cross-entropy, value and gradient in one call (replaces timm.loss.SoftTargetCrossEntropy as the
 * reference trainer uses it, imagenet_classification/supervised_imagenet.py:83, 109-115, and its autograd):
 *   loss_rows[b] = sum_c -target[b][c] * log_softmax(logits[b])[c];  loss[0] = mean_b loss_rows[b];
 *   dlogits[b][c] = (softmax(logits[b])[c] * sum_c' target[b][c'] - target[b][c]) / batch      (fp32)
 * logits (batch, classes) fp32 or bf16, target fp32; classes <= 2048.  Deterministic (fixed summation order). */
int fv_soft_target_ce(const void* logits, int logits_dtype, const float* target, float* loss_rows, float* loss,
                      float* dlogits, int batch, int classes, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Small memory-bound ops around the backbone (csrc/glue.hip): each replaces a string of library elementwise /
 * reduce launches of the reference step.
 * ---------------------------------------------------------------------- */
/* The k == stride patch-embed Conv2d (models/fastvim.py:95) as a GEMM: its A operand, unfolded and cast in one pass.
 *   out[b][gi*gw + gj][(c*ph + pi)*pw + pj] = img[b][c][gi*ph + pi][gj*pw + pj]
 * img (batch, chans, height, width), out (batch, gh*gw, chans*ph*pw); fp32 or bf16 each; pw even and at least 8 (a multiple of 8
 * takes 16-byte accesses throughout, any other even width places 2-element pairs and stores 16, 8 or 4 bytes at a
 * time, whichever the grid's chunk boundaries allow). */
int fv_patch_unfold(const void* img, int img_dtype, void* out, int out_dtype, int batch, int chans, int height,
                    int width, int ph, int pw, fv_stream_t stream);
/* fv_gemm_bf16(a_k_slow = b_k_slow = 0) with fp32 C = bf16_round(A B^T) + table[(m mod period)][n]: the patch
 * projection with conv bias and position embedding added in the epilogue (models/fastvim.py:95-101, 500) -- the
 * value an autocast F.linear followed by the fp32 add returns.  table (period, N) fp32. */
int fv_gemm_bf16_rowbias(const void* A, const void* B, float* C, const float* table, int period, int M, int N, int K,
                         long lda, long ldb, long ldc, fv_stream_t stream);
/* final_pool_type == "mean" (models/fastvim.py:529-531): out[b][d] = mean_l x[b][l][d] (fp32 sum, fixed order) and its
 * adjoint dx[b][l][d] = g[b][d] / tokens.  x (batch, tokens, dim), dim % 4 == 0, one dtype throughout. */
int fv_mean_pool_fwd(const void* x, void* out, int batch, int tokens, int dim, int dtype, fv_stream_t stream);
int fv_mean_pool_bwd(const void* g, void* dx, int batch, int tokens, int dim, int dtype, fv_stream_t stream);
/* Stochastic depth (timm DropPath, models/fastvim.py:175-178): table (mods, batch) holds U[0,1) draws on entry and
 * floor(keep[m] + U) * inv_keep[m] on return -- one row of per-sample scales per DropPath module. */
int fv_droppath_table(float* table, const float* keep, const float* inv_keep, int mods, int batch, fv_stream_t stream);
/* y[i] = x[i] * scale[0] (device scalar), cast to y_dtype: the loss gradient handed to the head. */
int fv_scale_cast(const float* x, const float* scale, void* y, int y_dtype, size_t n, fv_stream_t stream);
/* out[c] (+)= sum_r x[r][c], x (rows, cols) fp32 or bf16, fixed order: a bias gradient. */
int fv_column_sum(const void* x, int dtype, float* out, int rows, int cols, int accumulate, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Batch-mode Mixup / CutMix (timm.data.Mixup, mode='batch'; the first line of the reference's training_step,
 * imagenet_classification/supervised_imagenet.py:116-139) and the losses on integer labels (:80-92).
 *
 * Image b is mixed with image batch-1-b.  Everything below reads the augmentation's parameters from a MIX-PARAMETER
 * BLOCK in device memory -- 32 bytes, 16-byte aligned, laid out as `struct fv_mix_params` -- and takes none of them
 * as a launch argument: the host rewrites the block between two replays of a captured launch, and the replay mixes
 * with the new values.
 *   lam            fp32 weight of the image itself / of labels[b]
 *   one_minus_lam  fp32 rounding of the DOUBLE 1 - lam (what Python's `1. - lam` hands to torch), weight of the partner
 *   use_cutmix     0: mixup, out = fl(x * lam) + fl(x_partner * one_minus_lam), the two products rounded separately
 *                     to the storage type, then added (no fused multiply-add: that is torch's x.mul(lam).add_(
 *                     x.flip(0).mul_(1. - lam)) bit for bit); lam == 1 is a plain copy
 *                  1: cutmix, pixels with yl <= y < yh and xl <= x < xh come from the partner image, all others
 *                     from the image itself (an empty box is a plain copy); lam only weighs the labels
 *   yl, yh, xl, xh the box, in pixels
 * ---------------------------------------------------------------------- */
typedef struct fv_mix_params {
  float lam;
  float one_minus_lam;
  int32_t use_cutmix;
  int32_t yl, yh, xl, xh;
  int32_t reserved;
} fv_mix_params;

/* ------------------------------------------------------------------------
 * Random erasing (timm.data.random_erasing.RandomErasing with count 1, as every ImageNet and MAE fine-tune loader of
 * the reference applies it: after Normalize, before the batch-level Mixup).  Sample b has at most one box; inside it
 * every pixel of every channel is replaced.  Like the mix parameters, boxes and noise key live in an ERASE BLOCK in
 * device memory that the kernels read when they RUN -- 4 + 4 * batch int32, 16-byte aligned:
 *   [0] key0, [1] key1   the Philox key of this draw (the host derives it from its (seed, counter))
 *   [2] mode             FV_ERASE_CONST: write 0;  FV_ERASE_PIXEL: write a standard-normal value per (channel, y, x)
 *   [3] batch            number of box records that follow; a sample at or past it is not erased
 *   [4 + 4 b ..]         top, left, h, w of sample b, in pixels; h <= 0 (or w <= 0) means no erase
 * The noise at (b, c, y, x) is a function of (key0, key1, b, c, y, x) alone (csrc/erase_noise.h): Philox4x32-10 with
 * key (key0, key1) and counter (x >> 2, y, c, b); output words 0, 1 become pixels x & ~3 and (x & ~3) + 1 by Box-Muller
 * (cos, sin), words 2, 3 the next two; u1 = ((r >> 8) + 1) * 2^-24, u2 = (r' >> 8) * 2^-24.  Every kernel below writes
 * the same bits for the same key, whatever its load width, output type or workgroup shape.
 * ---------------------------------------------------------------------- */
#define FV_ERASE_CONST 0
#define FV_ERASE_PIXEL 1
/* out = x outside the boxes, 0 / noise inside; x, out (batch, chans, height, width) contiguous, of one dtype (fp32 or
 * bf16: the fp32 noise rounded once).  out == x is allowed (then only the boxes are touched); any other overlap is
 * not.  16-byte accesses where width and addresses allow, else 8, 4 or one element. */
int fv_random_erase(const void* x, void* out, int dtype, int batch, int chans, int height, int width, const void* erase,
                    fv_stream_t stream);

/* out[b] = mix(x[b], x[batch-1-b]), out of place; x, out (batch, chans, height, width) of one dtype (fp32 or bf16),
 * batch even.  One thread handles the same position of both images of a pair: the batch is read once and written
 * once. */
int fv_mix_batch(const void* x, void* out, int dtype, int batch, int chans, int height, int width, const void* mix,
                 fv_stream_t stream);
/* fv_patch_unfold of the mixed batch in one launch: the mixed image never exists in memory.  A workgroup unfolds the
 * same chunk of a patch row of both images of a pair; a pixel is mixed in the image's dtype exactly as fv_mix_batch
 * mixes it and rounded to out_dtype once, so out equals fv_patch_unfold(fv_mix_batch(img)) bit for bit.  Arguments
 * and limits of fv_patch_unfold; batch even. */
int fv_patch_unfold_mix(const void* img, int img_dtype, void* out, int out_dtype, int batch, int chans, int height,
                        int width, int ph, int pw, const void* mix, fv_stream_t stream);
/* The dense soft target timm.data.Mixup returns: target (batch, classes) fp32 =
 *   fl(y1 * lam) + fl(y2 * one_minus_lam),  y1 = one_hot(labels), y2 = one_hot(labels reversed along the batch),
 * one_hot with off = smoothing / classes elsewhere and on = 1 - smoothing + off at the label (both computed in double,
 * rounded to fp32).  labels (batch,) int64; a label outside [0, classes) marks no class. */
int fv_mixup_target(const int64_t* labels, float* target, int batch, int classes, double smoothing, const void* mix,
                    fv_stream_t stream);
/* fv_soft_target_ce on the target fv_mixup_target would write, built in registers from labels[b], labels[batch-1-b]
 * and the block: same row body, bit-identical loss_rows / loss / dlogits, no (batch, classes) target tensor.
 *   mix == NULL    no partner: the target is one_hot(labels) itself -- torch.nn.CrossEntropyLoss (mean reduction) with
 *                  smoothing == 0, timm.loss.LabelSmoothingCrossEntropy with smoothing > 0; batch may be odd
 *   dlogits        NULL: value only (validation)
 *   correct_rows, n_correct   NULL, or (batch,) / 1 int32: correct_rows[b] = (argmax_c logits[b][c] == labels[b]), the
 *                  first maximum on a tie, and their sum (fixed order) -- the validation step's top-1 count
 * classes <= 2048. */
int fv_label_ce(const void* logits, int logits_dtype, const int64_t* labels, const void* mix, double smoothing,
                float* loss_rows, float* loss, float* dlogits, int32_t* correct_rows, int32_t* n_correct, int batch,
                int classes, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Hierarchical channel sampling of the channel models (PatchEmbedPerChannel.forward,
 * models/channel_wise_tokenization/models_channel_mamba_faster.py:167-181): every training forward embeds a drawn
 * subset of n_sel of the image's chans_total channels.  The COUNT n_sel fixes every shape downstream and is a launch
 * argument; the INDICES are read from `sel`, n_sel int32 in device memory, when the kernel runs -- the host rewrites
 * them between two replays of a captured launch, like the mix-parameter block.  sel == NULL is the identity
 * (channels 0 .. n_sel-1: evaluation, hcs off).  An index outside [0, chans_total) is clamped into it by the gather
 * kernels and skipped by the scatter; the indices of a subset are distinct.
 * ---------------------------------------------------------------------- */
/* The per-channel patches of the shared Conv3d(1, D, (1, ph, pw)) projection (:117-125) as a GEMM operand, in
 * (row, col, channel) token order (:193-198), unfolded, gathered and cast in one pass:
 *   out[b][(p * n_sel + k)][pi*pw + pj] = img[b][sel[k]][gi*ph + pi][gj*pw + pj],
 *   p = gi*gw + gj, or gj*gh + gi with `colwise` (scanpath_type == "colwise", :193-194).
 * img (batch, chans_total, height, width), out (batch, gh*gw*n_sel, ph*pw); fp32 or bf16 each; pw % 8 == 0.  Every
 * byte of a selected channel is read once, an unselected channel is not touched, the gathered image never exists. */
int fv_patch_unfold_chan(const void* img, int img_dtype, void* out, int out_dtype, int batch, int chans_total,
                         int height, int width, int ph, int pw, const int32_t* sel, int n_sel, int colwise,
                         fv_stream_t stream);
/* The per-token table fv_gemm_bf16_rowbias adds (period = positions * n_sel), fp32, in exactly this association:
 *   table[p * n_sel + k][:] = (chan_table[sel[k]][:] + bias[:]) + pos[p][:]
 * chan_table (chans_total, dim) -- the channel embedding (:188-191); bias (dim) and pos (positions, dim) -- the conv
 * bias and x + repeat_interleave(pos_embed, n_sel, 1) (:626-627) -- may each be NULL (that term is left out). */
int fv_chan_embed_table(const float* chan_table, const float* bias, const float* pos, float* table, const int32_t* sel,
                        int n_sel, int chans_total, int positions, int dim, fv_stream_t stream);
/* The adjoint of the table's gather: d_table[sel[k]][:] += d_chan[k][:], d_chan (n_sel, dim), d_table (chans_total, dim),
 * fp32.  The rows of channels that were not drawn are not touched.  One thread owns an element: no atomics. */
int fv_chan_embed_scatter(const float* d_chan, float* d_table, const int32_t* sel, int n_sel, int chans_total, int dim,
                          fv_stream_t stream);

/* ------------------------------------------------------------------------
 * 8-bit images: the three patch unfolds above with the loader's per-channel normalisation (ToTensor + Normalize,
 * A.Normalize) as a table lookup.  img is uint8, (batch, chans, height, width) contiguous; table is fp32
 * (chans, 256) in device memory, read when the kernel runs, built by the HOST in the loader's own order of operations
 * (fastvim_amd/pixels.py) -- the kernels do no arithmetic on a pixel that a fast-math build could rewrite.  A pixel
 * becomes table[c][img] (c the SOURCE channel: sel[k] in the per-channel form) and from there on is treated exactly
 * as the float entry points treat an fp32 image, so for out_dtype fp32 and bf16
 *   fv_patch_unfold_u8(img, table)      == fv_patch_unfold(table[c][img] as an fp32 image)
 *   fv_patch_unfold_mix_u8(img, table)  == fv_patch_unfold_mix(...)   (mixed in fp32, products rounded separately)
 *   fv_patch_unfold_chan_u8(img, table) == fv_patch_unfold_chan(...)  (an index outside [0, chans_total) is clamped)
 * bit for bit.  Output layouts, sel / mix blocks and the limits on the patch shape are those of the float entry
 * points, with the table (1 KB per channel) sharing the workgroup's 64 KB of LDS with the staging tile.  Image rows
 * are loaded 16 bytes at a time where width, patch width and the image's base address allow, else 8, 4 or 2: the image
 * must be 2-byte aligned (4-byte for the per-channel form), table and out 16-byte aligned.
 * ---------------------------------------------------------------------- */
int fv_patch_unfold_u8(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                       int height, int width, int ph, int pw, fv_stream_t stream);
int fv_patch_unfold_mix_u8(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                           int height, int width, int ph, int pw, const void* mix, fv_stream_t stream);
int fv_patch_unfold_chan_u8(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans_total,
                            int height, int width, int ph, int pw, const int32_t* sel, int n_sel, int colwise,
                            fv_stream_t stream);
/* The two launches above with random erasing between the lookup and the placement / the mixing: `erase` is the erase
 * block described at fv_random_erase; in the pair launch each image of a pair is erased with its own box first and
 * mixed afterwards (loader, then training_step).  Bit for bit
 *   fv_patch_unfold_u8_re(img, table, erase)          == fv_patch_unfold(fv_random_erase(table[c][img]))
 *   fv_patch_unfold_mix_u8_re(img, table, mix, erase) == fv_patch_unfold_mix(fv_random_erase(table[c][img]), mix) */
int fv_patch_unfold_u8_re(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                          int height, int width, int ph, int pw, const void* erase, fv_stream_t stream);
int fv_patch_unfold_mix_u8_re(const uint8_t* img, const float* table, void* out, int out_dtype, int batch, int chans,
                              int height, int width, int ph, int pw, const void* mix, const void* erase,
                              fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused AdamW (decoupled weight decay, bias correction; torch.optim.AdamW semantics) over a flat fp32
 * parameter buffer, optionally updating an EMA copy (timm ModelEmaV2: ema = d*ema + (1-d)*p) and the
 * bf16 shadow weights in the same pass.  Replaces the optimizer + EMA + autocast casts of the
 * reference step (imagenet_classification/supervised_imagenet.py:134-147, 270-276).
 * decay_mask: one byte per element (1 = weight decay applies).  lr, step: device scalars (fp32);
 * step is incremented by the call.  grad_scale multiplies every gradient element as it is read: 1, or
 * 1 / world_size when `grads` holds the SUM over data-parallel ranks (the mean torch DDP produces,
 * imagenet_classification/train.py:34-43, without a pass of its own).  n % 4 == 0.
 * ---------------------------------------------------------------------- */
int fv_adamw_flat(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema,
                  void* shadow_bf16, const uint8_t* decay_mask, const float* lr, float* step, float beta1,
                  float beta2, float eps, float weight_decay, float ema_decay, float grad_scale, size_t n,
                  fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused optimizer with parameter groups and global-norm gradient clipping: the reference's fine-tune recipe
 * (mae/lr_decay.py:param_groups_lrd groups with an lr_scale each, mae/finetune_imagenet.py:148-151, 238-262;
 * gradient_clip_val of mae/config/finetune_FastVimH_448.yaml = torch.nn.utils.clip_grad_norm_ on the mean gradient).
 *
 * fv_grad_sumsq_blocks(n): host-side size query, G = number of workgroups = number of fp32 partials of the launch below,
 *   a pure function of n (1 <= G <= 1024; never of the device).
 * fv_grad_sumsq_partials: ONE launch; partials[b] = sum of grads[i]^2 over workgroup b's share of the RAW gradient (no
 *   grad_scale), accumulated in a fixed order (no atomics): same input, same bits.  n % 4 == 0, grads 16-byte aligned,
 *   partials holds G floats.
 * fv_adamw_flat_groups: the pass of fv_adamw_flat with
 *   group_ids    one byte per element (in place of decay_mask): row of group_table; padding elements carry 0
 *   group_table  n_groups rows (1 <= n_groups <= 256) of two floats (lr_scale, weight_decay), DEVICE memory: element
 *                update with lr_g = lr[0] * lr_scale, p *= 1 - lr_g * weight_decay, step size lr_g / bias_correction1
 *   partials     NULL, or the n_partials = fv_grad_sumsq_blocks(n) floats fv_grad_sumsq_partials wrote (16-byte aligned).
 *                Every workgroup sums them in one fixed order: total_norm = grad_scale * sqrt(sum)
 *   max_norm     NULL, or a device scalar (needs partials): clip_coef = min(1, max_norm / (total_norm + 1e-6)) and every
 *                gradient element is read as g * (grad_scale * clip_coef)
 *   stats        4 floats, required with partials: [total_norm, clip_coef, finite (0/1), skipped_steps].  The first three
 *                are written by the call; skipped_steps is a counter the call only ever increments (zero it once)
 *   skip_nonfinite  non-zero (needs partials): when the sum of squares is not finite the call leaves params, exp_avg,
 *                exp_avg_sq, ema, shadow and step untouched and adds 1 to skipped_steps
 * lr, step as for fv_adamw_flat.  n % 4 == 0.
 * ---------------------------------------------------------------------- */
int fv_grad_sumsq_blocks(size_t n);
int fv_grad_sumsq_partials(const float* grads, float* partials, size_t n, fv_stream_t stream);
int fv_adamw_flat_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema,
                         void* shadow_bf16, const uint8_t* group_ids, const float* group_table, int n_groups,
                         const float* lr, float* step, const float* partials, int n_partials, const float* max_norm,
                         float* stats, int skip_nonfinite, float beta1, float beta2, float eps, float ema_decay,
                         float grad_scale, size_t n, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * BatchNorm1d over pooled features (batch, dim), row-major, fp32 or bf16 -- the linear-probe head of the reference
 * (mae/linear_imagenet.py:39-53: Sequential(BatchNorm1d(dim, affine=False, eps=1e-6), head); a SyncBatchNorm under
 * mae/linear.py:41).  Statistics, running buffers (fp32) and the counter (int64) as in torch.nn.BatchNorm1d.  All
 * sums are taken in a fixed order (no atomics): same input, same bits.
 *
 * fv_bn1d_stats: table_row (2 dim + 1 floats) = [mean(dim) | M2(dim) | count]: per-column mean and centred sum of
 *   squares of THIS rank's rows, by exact passes (mean, then deviations from it), and the row count.
 * fv_bn1d_apply: training != 0: merges the `world` rows of `table` (row r at table + r (2 dim + 1)) in rank order with
 *   the parallel-variance formula, writes xhat = (x - mean) * rsqrt(M2 / n + eps) in the feature dtype, the merged mean
 *   and rstd (dim floats each, for fv_bn1d_bwd), and updates running_mean / running_var (nullable, together) with
 *   `momentum` -- the running variance from M2 / (n - 1) -- and num_batches_tracked (nullable) += 1: each by exactly
 *   one thread, so a replayed graph advances them once per replay.  training == 0: xhat from the running statistics
 *   (required), mean_out / rstd_out = what was used, no buffer touched, table unused.
 * fv_bn1d_bwd: training != 0: dx = rstd (dy - mean_b(dy) - xhat mean_b(dy xhat)) with xhat = (x - mean) rstd recomputed
 *   from x and the mean / rstd fv_bn1d_apply wrote -- the adjoint for ONE rank's batch statistics.  training == 0:
 *   dx = dy * rstd.  dy, x, dx share the feature dtype.
 * ---------------------------------------------------------------------- */
int fv_bn1d_stats(const void* x, int dtype, float* table_row, int batch, int dim, fv_stream_t stream);
int fv_bn1d_apply(const void* x, int dtype, const float* table, int world, float* running_mean, float* running_var,
                  int64_t* num_batches_tracked, void* xhat, float* mean_out, float* rstd_out, int batch, int dim,
                  float eps, float momentum, int training, fv_stream_t stream);
int fv_bn1d_bwd(const void* dy, const void* x, int dtype, const float* mean, const float* rstd, void* dx, int batch,
                int dim, int training, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Momentum SGD and LARS over the flat buffers of fv_adamw_flat (lr a device scalar; bf16 shadow refreshed in the same
 * pass, nullable): the linear-probe optimizers (mae/linear_imagenet.py:230 torch.optim.SGD(momentum=0.9); mae/lars.py).
 *
 * fv_sgd_flat: g' = g * grad_scale + weight_decay * p (where decay_mask[i] != 0); buf = momentum * buf + g';
 *   p -= lr * buf.  With a zero-initialised buf: torch.optim.SGD, dampening 0, no Nesterov.  n % 4 == 0.
 * LARS: `segments` is DEVICE memory, n_segments rows of three int64 (first element, element count, ndim > 1), one per
 *   parameter; a row that does not lie inside [0, n) is skipped.  P = fv_lars_partials_per_segment().
 * fv_lars_sumsq_partials: partials (n_segments x 2 x P floats): fixed-order partial sums of |p|^2 and of
 *   |g * grad_scale + weight_decay * p|^2 of every segment with ndim > 1.
 * fv_lars_flat: per segment with ndim > 1: finishes its partials, q = trust_coefficient |p| / |dp| when both norms are
 *   positive, else 1; dp = (g * grad_scale + weight_decay * p) * q.  Segments with ndim <= 1: dp = g * grad_scale
 *   (lars.py:29).  Then buf = momentum * buf + dp; p -= lr * buf.  norms: NULL, or n_segments x 3 floats written as
 *   [|p|, |dp|, q] ([0, 0, 1] for ndim <= 1).
 * ---------------------------------------------------------------------- */
int fv_sgd_flat(float* params, const float* grads, float* momentum_buf, void* shadow_bf16, const uint8_t* decay_mask,
                const float* lr, float momentum, float weight_decay, float grad_scale, size_t n, fv_stream_t stream);
int fv_lars_partials_per_segment(void);
int fv_lars_sumsq_partials(const float* params, const float* grads, const int64_t* segments, int n_segments,
                           float* partials, float weight_decay, float grad_scale, size_t n, fv_stream_t stream);
int fv_lars_flat(float* params, const float* grads, float* momentum_buf, void* shadow_bf16, const int64_t* segments,
                 int n_segments, const float* partials, const float* lr, float* norms, float momentum,
                 float weight_decay, float trust_coefficient, float grad_scale, size_t n, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * The validation step of the reference's supervised loops (imagenet_classification/supervised_imagenet.py:151-210,
 * mae/finetune_imagenet.py:165-221, cell_imaging/supervised.py:132-165): every batch through the live backbone and
 * through the EMA copy, loss and top-1 accuracy of each as epoch means.
 *
 * fv_swap_params_ema: ONE pass that exchanges params[i] and ema[i] (fp32, bit for bit, NaN payloads included) and writes
 *   shadow[i] = cast(new params[i]) in shadow_dtype (FV_BF16, FV_F16: round to nearest even, denormals kept, a NaN stays
 *   a NaN; FV_F32: a copy) -- the flat training state's weights become the EMA weights in place, and a second call puts
 *   all three buffers back.  No arithmetic on the values.  8 B read and 8 B + the shadow element written per element (18 B with bf16).
 *   n is arbitrary; the buffers need only the alignment of their element type: 16-byte accesses are used from the first
 *   element at which params, ema and the shadow are all aligned for them (the start of equally offset views of aligned
 *   allocations), single elements before it, for the tail, and throughout when no such element exists.
 *
 * fv_eval_accumulate: two launches that add one batch to an accumulator block.
 *   logits (batch, classes) fp32 or bf16; labels (batch,) int64; classes <= 2048
 *   n_valid      one int32 in DEVICE memory, read when the kernels run (a captured launch sees what the host wrote
 *                before the replay): only rows b < min(max(*n_valid, 0), batch) count.  The other rows' logits and
 *                labels are not read, whatever they hold.
 *   loss_rows, correct_rows   scratch, (batch,) fp32 / int32: for a counted row exactly what fv_label_ce(mix = NULL,
 *                smoothing = 0) writes there (same row body, bit-identical), for the other rows 0
 *   acc          the accumulator block, FV_EVAL_ACC_HEAD + 2 * classes 64-bit words, 8-byte aligned, zeroed by the caller
 *                at the start of an epoch:
 *                  word 0                       loss_sum, an fp64: += the sum of the counted rows' fp32 losses, taken in
 *                                               fp64 in one fixed order (no float atomics)
 *                  word 1                       n_seen, int64: += the number of counted rows
 *                  word 2                       n_correct, int64: += the counted rows whose arg-max is their label
 *                  words 3 .. 3 + classes       support[c], int64: += the counted rows with label c
 *                  words 3 + classes .. end     hit[c], int64: += those of them that are correct
 *                A counted row whose label is outside [0, classes) adds to n_seen only (its loss is 0, it is never correct
 *                and belongs to no class); no label value causes an access outside the block.  The same batches in the
 *                same order leave the same bytes.
 * ---------------------------------------------------------------------- */
#define FV_EVAL_ACC_HEAD 3
int fv_swap_params_ema(float* params, float* ema, void* shadow, int shadow_dtype, size_t n, fv_stream_t stream);
int fv_eval_accumulate(const void* logits, int logits_dtype, const int64_t* labels, const int32_t* n_valid,
                       float* loss_rows, int32_t* correct_rows, int64_t* acc, int batch, int classes, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * The MAE reconstruction loss (models/mae/models_mamba_faster_mae_vimdecoder.py:864-880, forward_loss): mean squared error
 * between the prediction and the (per-patch normalised) pixels, averaged over the removed patches.
 *
 *   img        (batch, 3, height, width), contiguous.  table == NULL: fp32 (the normalised images).  table != NULL: uint8,
 *              and a pixel is table[c][v]; table is the (3, 256) fp32 table of fv_patch_unfold_u8, 16-byte aligned
 *   pred       (batch, L, D) fp32 or bf16 (pred_dtype), contiguous; L = (height / patch) (width / patch), D = 3 patch^2;
 *              patch l = gy (width / patch) + gx, element j = (py patch + px) 3 + c is pixel (c, gy patch + py, gx patch + px)
 *   mask       (batch, L) fp32: 0 = kept, else the patch's weight (1 = removed)
 *   loss_rows  (batch, L) fp32 out: sum_j (pred[j] - target[j])^2 / D; exactly 0 where mask == 0
 *   row_stats  (batch, L, 2) fp32 out: (mean, rstd) of the patch, (0, 1) without norm_pix, (0, 0) where mask == 0
 *   out        2 floats out: out[0] = sum(loss_rows mask) / sum(mask), out[1] = sum(mask)
 * norm_pix != 0: mean = sum(t) / D, var = sum((t - mean)^2) / (D - 1) -- exact fp32 passes over the on-chip copy of the
 *   patch, the mean first (refined once by the sum of the residuals), never E[t^2] - mean^2: a constant patch has var 0
 *   and target 0 exactly --, target = (t - mean) rsqrt(var + 1e-6); norm_pix == 0: target = t.
 * A patch with mask == 0 is not read: neither its pixels nor its pred row, whatever they hold.
 *
 * fv_mae_loss_fwd: two launches (the rows, then one workgroup that sums loss_rows mask and mask in fp64 in a fixed order);
 *   no atomics: the same inputs give the same bits.
 * fv_mae_loss_bwd: one launch.  dpred[n, l, j] = g mask[n, l] 2 (pred - target) / (D sum_mask) in pred_dtype, with target
 *   recomputed from img and the row_stats of the forward call; exactly 0, with nothing read, where mask == 0.  g and
 *   sum_mask are single fp32 values in DEVICE memory (sum_mask: out + 1 of the forward call).
 * fv_mae_loss_ok: host code; 1 when both accept the shape: chans == 3, height == width, a multiple of patch, patch even
 *   in [8, 28], pred fp32 or bf16, batch L <= 131072.
 * Alignment: every buffer that of its element type only (uint8 images: none), the table 16 bytes; the kernels pick their
 *   access widths from the actual addresses.
 * Bit identity: a call with a table equals the call with table == NULL on the fp32 image table[c][img] in every output --
 *   loss_rows, row_stats, out, dpred.  The uint8 form only looks values up (no arithmetic on the byte).
 * sum(mask) == 0 is unspecified (0 / 0, as in the reference).
 * ---------------------------------------------------------------------- */
int fv_mae_loss_ok(int batch, int chans, int height, int width, int patch, int pred_dtype);
int fv_mae_loss_fwd(const void* img, const float* table, const void* pred, int pred_dtype, const float* mask,
                    float* loss_rows, float* row_stats, float* out, int batch, int height, int width, int patch,
                    int norm_pix, fv_stream_t stream);
int fv_mae_loss_bwd(const void* img, const float* table, const void* pred, int pred_dtype, const float* mask,
                    const float* row_stats, const float* sum_mask, const float* g, void* dpred, int batch, int height,
                    int width, int patch, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * MAE token bookkeeping (csrc/mae_tokens.hip): the masking plan of a step from ONE launch, the permuted row copies that
 * use it, and the decoder's input assembly.  B = batch, L = grid_h grid_w tokens, K = len_keep.
 *
 * fv_mae_mask_plan: one workgroup per sample.  noise (B, L) fp32.  rank[i] = #{j : noise[j] < noise[i], or equal and
 *   j < i} -- the stable ascending order; the K lowest-ranked tokens are kept.  All outputs are written by this launch:
 *   ids_keep        (B, K) int64   positions of the kept tokens, ascending
 *   ids_restore     (B, L) int64   kept token: its place among the kept ones; removed token: its rank
 *   mask            (B, L) fp32    1 = removed
 *   keep_index      (B, K) int32   = ids_keep
 *   restore_index   (B, L) int32   = ids_restore where < K, else -1
 *   row_index_even  (2, B, K) int32  [r, (grid_h - 1) - flip(r)], r = ids_keep / grid_w
 *   ids_keep_odd    (B, K) int64   the kept tokens' places (id % grid_w) grid_h + id / grid_w in the transposed grid, ascending
 *   order, inverse  (B, K) int64   ids_keep_odd[q] is the transposed place of kept token order[q]; inverse[order[q]] = q
 *   order_index, inverse_index  (B, K) int32  the same two
 *   row_index_odd   (2, B, K) int32  [r, (grid_w - 1) - flip(r)], r = ids_keep_odd / grid_h
 *   L <= FV_MAE_PLAN_MAX_TOKENS, 1 <= K <= L.  Finite noise is the contract.  The order is taken on the bit patterns
 *   (-0 == +0), so ANY input, NaN included, gives a permutation: every index written is in range and nothing is written
 *   outside the outputs; which tokens a NaN makes kept is unspecified.
 *
 * fv_tokens_gather: out[b, t, :] = in[b, index[b, t], :] for in (B, len_in, dim), index (B, len_out) int32, out
 *   (B, len_out, dim); an index outside [0, len_in) writes a zero row.  in / out: fp32 or bf16 each; the same type is a
 *   bit copy, different types one conversion (round to nearest even).  dim % 4 == 0.  With unique indices the adjoint is
 *   the gather by the inverse index, -1 where a row of `in` was not picked.
 *
 * fv_mae_decoder_tokens_fwd: out[b, l, :] = (r >= 0 ? x[b, r, :] : mask_token rounded to x_dtype) + pos_embed[l, :] with
 *   r = restore_index[b, l]; x (B, K, dim) fp32 or bf16, mask_token (dim) fp32, pos_embed (L, dim) fp32, out (B, L, dim)
 *   fp32: one fp32 rounding, of the sum.  dim % 4 == 0.
 * fv_mae_decoder_tokens_bwd: two launches.  dx[b, r, :] = dout[b, l, :] in x_dtype for the rows with r >= 0;
 *   dmask_token (dim) fp32 = the sum of the other rows of dout (B, L, dim) fp32, each rounded to x_dtype first, added in
 *   fp64 in a fixed order: a workgroup per FV_MAE_DECODER_ROWS_PER_BLOCK rows of (B L) writes one row of `partials`
 *   (n_partials = ceil(B L / FV_MAE_DECODER_ROWS_PER_BLOCK) rows of dim doubles, caller-allocated), a second launch adds
 *   those.  No atomics: the same inputs give the same bits.  restore_index must hold each of 0 .. K-1 once per sample (as
 *   fv_mae_mask_plan writes it) for every row of dx to be written.
 *
 * The KEY BLOCK: int32[4] in DEVICE memory, (k0, k1, step_lo, step_hi), read when the kernels RUN (a replayed graph takes
 *   the values of that moment).  The masking noise of sample b, token l is u = float(w >> 8) * 2^-24 -- exact, in [0, 1),
 *   24 bits like torch.rand -- with w = word (l & 3) of Philox4x32-10 under key (k0, k1) and counter (l >> 2, b, step_lo,
 *   step_hi); the rounds are those of the erase noise (fv_random_erase).
 * fv_mae_noise: noise (batch, len) fp32 = that u for every (b, l): one launch.
 * fv_mae_mask_plan_keyed: fv_mae_mask_plan of the noise of `block` with the noise made inside the launch -- no (B, L)
 *   tensor exists; same outputs, same limits, same stable order, and every output equal bit for bit to fv_mae_mask_plan
 *   on what fv_mae_noise(block, ., batch, grid_h grid_w) writes.
 * Alignment: every buffer that of its element type only.
 * ---------------------------------------------------------------------- */
#define FV_MAE_PLAN_MAX_TOKENS 1024
#define FV_MAE_DECODER_ROWS_PER_BLOCK 32
int fv_mae_mask_plan(const float* noise, long long* ids_keep, long long* ids_restore, float* mask, int* keep_index,
                     int* restore_index, int* row_index_even, long long* ids_keep_odd, long long* order, long long* inverse,
                     int* order_index, int* inverse_index, int* row_index_odd, int batch, int grid_h, int grid_w,
                     int len_keep, fv_stream_t stream);
int fv_mae_noise(const int32_t* block, float* noise, int batch, int len, fv_stream_t stream);
int fv_mae_mask_plan_keyed(const int32_t* block, long long* ids_keep, long long* ids_restore, float* mask, int* keep_index,
                           int* restore_index, int* row_index_even, long long* ids_keep_odd, long long* order,
                           long long* inverse, int* order_index, int* inverse_index, int* row_index_odd, int batch,
                           int grid_h, int grid_w, int len_keep, fv_stream_t stream);
int fv_tokens_gather(const void* in, int in_dtype, const int* index, void* out, int out_dtype, int batch, int len_in,
                     int len_out, int dim, fv_stream_t stream);
int fv_mae_decoder_tokens_fwd(const void* x, int x_dtype, const float* mask_token, const float* pos_embed,
                              const int* restore_index, float* out, int batch, int len, int len_keep, int dim,
                              fv_stream_t stream);
int fv_mae_decoder_tokens_bwd(const float* dout, const int* restore_index, void* dx, int x_dtype, double* partials,
                              int n_partials, float* dmask_token, int batch, int len, int len_keep, int dim,
                              fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Token assembly with a class token (csrc/mae_tokens_cls.hip): the Vim MAE baseline.  B = batch samples, L = len grid
 * tokens, K = len_keep kept ones, c = K / 2 the class token's place among the kept tokens; keep_index (B, K) and
 * restore_index (B, L) int32 as fv_mae_mask_plan writes them.  x_dtype FV_F32 or FV_BF16; dim % 4 == 0; B (L + 1) < 2^31.
 *
 * fv_mae_encoder_tokens_cls_fwd: out (B, K + 1, dim) in x_dtype from the UN-gathered x (B, L, dim) x_dtype:
 *   out[b, j] = x[b, keep_index[b, j]] for j < c, x[b, keep_index[b, j - 1]] for j > c (bit copies; a zero row where the
 *   index is outside [0, L)), and out[b, c] = cls_token + pos_embed[0], added in fp32 and rounded once to x_dtype.
 *   cls_token (dim) fp32; pos_embed fp32, of which only row 0 -- the class slot of the (L + 1, dim) table -- is read.
 * fv_mae_encoder_tokens_cls_bwd: two launches.  dx (B, L, dim) x_dtype, EVERY row written: row l takes
 *   dout[b, r + (r >= c)] with r = restore_index[b, l] where 0 <= r < K, zero elsewhere; dout (B, K + 1, dim) x_dtype.
 *   dcls_token (dim) fp32 = sum over b of dout[b, c, :], added in fp64 in the order b = 0 .. B-1, rounded once.
 * fv_mae_decoder_tokens_cls_fwd: out (B, L + 1, dim) fp32 from x (B, K + 1, dim) x_dtype:
 *   out[b, l] = (r >= 0 ? x[b, r + (r >= c)] : mask_token rounded to x_dtype) + pos_embed[1 + l] for l < L, and
 *   out[b, L] = x[b, c] + pos_embed[0]; mask_token (dim) fp32, pos_embed (L + 1, dim) fp32; one fp32 rounding, of the sum.
 * fv_mae_decoder_tokens_cls_bwd: two launches, the kernels of fv_mae_decoder_tokens_bwd.  dout (B, L + 1, dim) fp32;
 *   dx (B, K + 1, dim) x_dtype: row c takes dout[b, L], row r + (r >= c) takes dout[b, l] for the rows with r >= 0;
 *   dmask_token (dim) fp32 = the sum of the other rows l < L (the class row is no mask row), each rounded to x_dtype first,
 *   in fp64 in a fixed order: n_partials = ceil(B (L + 1) / FV_MAE_DECODER_ROWS_PER_BLOCK) rows of dim doubles,
 *   caller-allocated.  restore_index must hold each of 0 .. K-1 once per sample for every row of dx to be written.
 * No atomics, no host synchronisation: safe under stream capture; the same inputs give the same bits.
 * Alignment: every buffer that of its element type only.
 * ---------------------------------------------------------------------- */
int fv_mae_encoder_tokens_cls_fwd(const void* x, int x_dtype, const float* cls_token, const float* pos_embed,
                                  const int* keep_index, void* out, int batch, int len, int len_keep, int dim,
                                  fv_stream_t stream);
int fv_mae_encoder_tokens_cls_bwd(const void* dout, const int* restore_index, void* dx, int x_dtype, float* dcls_token,
                                  int batch, int len, int len_keep, int dim, fv_stream_t stream);
int fv_mae_decoder_tokens_cls_fwd(const void* x, int x_dtype, const float* mask_token, const float* pos_embed,
                                  const int* restore_index, float* out, int batch, int len, int len_keep, int dim,
                                  fv_stream_t stream);
int fv_mae_decoder_tokens_cls_bwd(const float* dout, const int* restore_index, void* dx, int x_dtype, double* partials,
                                  int n_partials, float* dmask_token, int batch, int len, int len_keep, int dim,
                                  fv_stream_t stream);

/* ------------------------------------------------------------------------
 * The class token of the supervised Vim baseline (csrc/vim_tokens.hip, csrc/norm.hip): B = batch samples, M = len patch
 * tokens, p = position of the class token among the M + 1 rows (0 <= p <= M).  y_dtype FV_F32 or FV_BF16; dim % 4 == 0;
 * B (M + 1) < 2^31.
 *
 * fv_vim_cls_tokens_fwd: out (B, M + 1, dim) fp32 from y (B, M, dim) y_dtype, the patch projection:
 *   out[b, j] = (j == p ? cls_token rounded to y_dtype : y[b, j - (j > p)]) + pos_embed[j], ONE fp32 add -- the values of
 *   `cat((x[:, :p], cls_token.expand(B, -1, -1).to(x.dtype), x[:, p:]), 1) + pos_embed`.  cls_token (dim) fp32,
 *   pos_embed (M + 1, dim) fp32.  A thread moves 16 bytes of y (8 for bf16 when dim % 8 != 0).
 * fv_vim_cls_tokens_bwd: ONE launch, one thread per (row j, vector of channels) walking b = 0 .. B-1.  dout (B, M + 1, dim)
 *   fp32; dy (B, M, dim) y_dtype: dy[b, i] = dout[b, i + (i >= p)] rounded to y_dtype (fp32: a bit copy);
 *   dpos_embed (M + 1, dim) fp32 = sum over b of dout[b, j, :], added in fp64 in that order, rounded once;
 *   dcls_token (dim) fp32 = the same sum of row p with every term rounded to y_dtype first (fp32: dpos_embed[p]).
 *
 * fv_add_norm_row_fwd: fv_add_norm_fwd of row `position` of every sample and of no other row.  hidden / residual
 *   (B, rows, N); row_scale (B) fp32 or NULL, one factor per sample; y (B, N), residual_out (B, N) -- the normalised
 *   input, which the backward reads -- mean (B, NULL for RMSNorm) and rstd (B) are packed.  The kernel bodies are those of
 *   fv_add_norm_fwd, chosen by N the same way: y, residual_out, mean and rstd equal that launch's rows b * rows + position
 *   bit for bit.
 * fv_add_norm_row_bwd: ONE launch writes ALL of dhidden and dresidual (B, rows, N) (dresidual may be NULL): row `position`
 *   of each sample from the norm's adjoint -- bit for bit the rows fv_add_norm_bwd writes for a dy that is zero outside
 *   those rows -- and zero everywhere else.  dy (B, N), r (B, N) = residual_out, mean, rstd as the forward left them.
 *   partial_dw / partial_db: (fv_add_norm_blocks(B), N) fp32, fixed-order sums over the B rows (reduce with
 *   fv_reduce_partials); partial_db NULL without a bias.
 * No atomics, no host synchronisation: safe under stream capture; the same inputs give the same bits.
 * Alignment: fv_vim_cls_tokens_*: every buffer that of its element type only; fv_add_norm_row_*: as fv_add_norm_*.
 * ---------------------------------------------------------------------- */
int fv_vim_cls_tokens_fwd(const void* y, int y_dtype, const float* cls_token, const float* pos_embed, float* out, int batch,
                          int len, int dim, int position, fv_stream_t stream);
int fv_vim_cls_tokens_bwd(const float* dout, void* dy, int y_dtype, float* dpos_embed, float* dcls_token, int batch, int len,
                          int dim, int position, fv_stream_t stream);
int fv_add_norm_row_fwd(const void* hidden, int hidden_dtype, const void* residual, int residual_dtype, const float* weight,
                        const float* bias, const float* row_scale, void* y, int y_dtype, void* residual_out,
                        int residual_out_dtype, float* mean, float* rstd, int batch, int rows, int position, int N, float eps,
                        int is_rms_norm, fv_stream_t stream);
int fv_add_norm_row_bwd(const void* dy, int dy_dtype, const void* r, int r_dtype, const float* weight, const float* mean,
                        const float* rstd, const float* row_scale, void* dhidden, int dhidden_dtype, void* dresidual,
                        int dresidual_dtype, float* partial_dw, float* partial_db, int batch, int rows, int position, int N,
                        int is_rms_norm, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * The class token of the ChannelVim baseline (csrc/chan_tokens.hip): B = batch samples, M = len channel tokens (P patches
 * times the channels of this forward pass; pos_embed is already in them), p = position of the class token among the
 * M + 1 rows (0 <= p <= M).  dtype FV_F32 or FV_BF16, of the tokens on BOTH sides; dim % 4 == 0; B (M + 1) < 2^31.
 *
 * fv_chan_cls_tokens_fwd: out (B, M + 1, dim) dtype from y (B, M, dim) dtype:
 *   out[b, j] = (j == p ? cls_token rounded to dtype : y[b, j - (j > p)]) -- the values of
 *   `cat((x[:, :p], cls_token.expand(B, -1, -1).to(x.dtype), x[:, p:]), 1)`.  The token rows are MOVED as bits: no
 *   arithmetic touches them (-0.0 stays -0.0).  cls_token (dim) fp32.  A thread moves 16 bytes (8 for bf16 when
 *   dim % 8 != 0).
 * fv_chan_cls_tokens_bwd: ONE launch.  dout (B, M + 1, dim) dtype; dy (B, M, dim) dtype: dy[b, i] = the bits of
 *   dout[b, i + (i >= p)], one thread per 16 bytes of dy (a full-grid copy); dcls_token (dim) fp32 = sum over
 *   b = 0 .. B-1 of dout[b, p, :], added in fp64 in that order, rounded once -- by dim / 4 (bf16, dim % 8 == 0: dim / 8)
 *   threads in the first workgroups of the same grid.
 * No atomics, no partial buffer, no host synchronisation: safe under stream capture; the same inputs give the same bits.
 * Alignment: every buffer 4 bytes.
 * ---------------------------------------------------------------------- */
int fv_chan_cls_tokens_fwd(const void* y, int dtype, const float* cls_token, void* out, int batch, int len, int dim,
                           int position, fv_stream_t stream);
int fv_chan_cls_tokens_bwd(const void* dout, void* dy, int dtype, float* dcls_token, int batch, int len, int dim,
                           int position, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-side geometry of the uint8 loaders: bicubic resize, crop window and horizontal flip of decoded 8-bit images,
 * bit for bit what PIL's `Image.resize(size, BICUBIC)` (ImagingResample, 8 bits per channel: horizontal pass, uint8
 * intermediate, vertical pass, integer coefficients of 22 fraction bits) followed by a crop and a flip computes --
 * the reference's RandomResizedCropAndInterpolation + RandomHorizontalFlip (mae/datasets_mae.py:83-99) and its
 * Resize + CenterCrop (datasets_supervised.py:254-262), in front of ToTensor / Normalize (fv_patch_unfold_u8).
 *
 *   pool   uint8, `pool_bytes` long: the decoded sources back to back, each H x W x 3 interleaved with packed rows
 *          (PIL's / numpy's layout); a source may start at ANY byte (rows of 3 w_src bytes have every alignment anyway).
 *   plan   (batch, FV_RESAMPLE_PLAN_INTS) int32 in DEVICE memory, read when the kernels RUN (a replayed graph takes the
 *          plan and the pool contents of that moment).  Per sample:
 *            [0] [1]  byte offset of the source in the pool, low and high 32 bits
 *            [2] [3]  h_src, w_src
 *            [4] [5]  o_h, o_w: the FULL output size of the resize
 *            [6] [7]  win_y, win_x: origin of the s_h x s_w window of it that is written
 *            [8]      flip != 0: out[.., x] = resized[.., win_x + s_w - 1 - x]
 *            [9..11]  unused, 0
 *   ws     int32 workspace of fv_resample_workspace_ints(batch, s_h, s_w) words, 4-byte aligned: per sample the x axis
 *          then the y axis, each (2 + FV_RESAMPLE_MAX_TAPS) rows of S words -- lo[S], cnt[S], then c[k][i].
 *   out    (batch, 3, s_h, s_w) uint8, planar, contiguous; any alignment (4-byte stores when it allows them).
 *
 * fv_resample_coeffs: one launch, a workgroup per (sample, axis): the window's filter bounds and integer coefficients
 *   in fp64 without contraction or fast-math -- PIL's precompute_coeffs + normalize_coeffs_8bpc.  A plan row that
 *   fv_resample_u8_ok refuses, or whose source does not lie inside the pool, gets cnt = 0 everywhere: the main launch
 *   then reads nothing of that sample and writes zeros.  (Callers check on the host first: fastvim_amd/resample.py.)
 * fv_resample_u8: one launch over (column tile, band of FV_RESAMPLE_BAND rows, sample); reads what fv_resample_coeffs
 *   wrote for the SAME plan, pool size and window size.  No atomics; the same inputs give the same bits.
 * fv_resample_u8_ok: host code, the range both serve -- batch in [1, 4096], s_h and s_w in [8, 1024], h_src and w_src
 *   in [1, 16384], o_h and o_w up to 65536, the window inside the output, and at most FV_RESAMPLE_MAX_TAPS filter taps
 *   per axis: h_src <= 16 o_h and w_src <= 16 o_w.
 * ---------------------------------------------------------------------- */
#define FV_RESAMPLE_PLAN_INTS 12
#define FV_RESAMPLE_MAX_TAPS 65
#define FV_RESAMPLE_BAND 16
int fv_resample_u8_ok(int batch, int s_h, int s_w, int h_src, int w_src, int o_h, int o_w, int win_y, int win_x);
long long fv_resample_workspace_ints(int batch, int s_h, int s_w);
int fv_resample_coeffs(const int* plan, long long pool_bytes, int* ws, int batch, int s_h, int s_w, fv_stream_t stream);
int fv_resample_u8(const void* pool, long long pool_bytes, const int* plan, const int* ws, void* out, int batch, int s_h,
                   int s_w, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-side RandAugment of a planar uint8 batch: one layer of timm's `RandAugment` (rand_augment_transform:
 * imagenet_classification/datasets_supervised.py:193-207) per pair of launches, bit for bit what PIL computes for the op
 * and argument the HOST drew (fastvim_amd/randaug.py).  Built without fast-math and with contraction off.
 *
 *   in, out  (batch, 3, s_h, s_w) uint8, planar, contiguous, distinct; any alignment.  `in` is only read.
 *   plan     (batch, num_layers, FV_RANDAUG_PLAN_INTS) int32 in DEVICE memory, 8-byte aligned, read when the kernels
 *            RUN (a replayed graph takes the plan of that moment).  The record of (sample, layer):
 *              [0]       kind, FV_RA_* below; a value outside them is FV_RA_COPY
 *              [1] [2]   arg0, arg1: SOLARIZE threshold | POSTERIZE bits kept | SOLARIZE_ADD addend, threshold
 *              [3]       the float32 bits of the blend factor (COLOR, CONTRAST, BRIGHTNESS, SHARPNESS)
 *              [4]       fill colour of AFFINE, R | G << 8 | B << 16
 *              [5]       unused, 0
 *              [6..17]   the six AFFINE coefficients (PIL's output-to-input map) as doubles, low word first
 *   ws       fv_randaug_workspace_bytes(batch) bytes: per sample a (3, 256) uint8 table.  fv_randaug_stats writes it
 *            for AUTOCONTRAST and EQUALIZE (the lookup table of each channel) and CONTRAST (byte 0: the mean grey
 *            value); fv_randaug_apply of the SAME layer reads it.
 *
 * fv_randaug_stats: one launch over (channel, sample), 256 threads.  Workgroups of samples whose op needs no statistic
 *   return at once.  Histograms are LDS integer atomics (order-independent); no global and no floating-point atomics.
 *     AUTOCONTRAST (ImageOps.autocontrast, cutoff 0): lo / hi the first / last non-empty bin; identity if hi <= lo, else
 *       fp64 scale = 255.0 / (hi - lo), offset = -lo * scale, lut[i] = clamp(trunc(i * scale + offset), 0, 255).
 *     EQUALIZE (ImageOps.equalize): integers; identity with at most one non-empty bin or step = (sum - last non-empty
 *       bin) / 255 == 0; else n = step / 2; lut[i] = min(n / step, 255); n += h[i].
 *     CONTRAST: int(sum of grey / (s_h * s_w) + 0.5) in fp64, grey = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16.
 * fv_randaug_apply: one launch over (tile of FV_RANDAUG_ROWS rows, sample), 256 threads; the kind is uniform in a
 *   workgroup.  COPY copies.  The table ops (AUTOCONTRAST, EQUALIZE from ws; INVERT, SOLARIZE, POSTERIZE, SOLARIZE_ADD,
 *   BRIGHTNESS and CONTRAST built in LDS from the record) are one lookup per byte.  COLOR and SHARPNESS are
 *   Image.blend(degenerate, image, factor) in float32: degenerate + factor * (image - degenerate), one multiply and one
 *   add, truncated for factors in [0, 1] and clipped otherwise; SHARPNESS's degenerate is ImageFilter.SMOOTH (borders
 *   copied, float32 weights k / 13, accumulator from 0.5, rows y + 1, y, y - 1).  AFFINE is Image.transform(size, AFFINE,
 *   m, BICUBIC, fillcolor) in fp64 (Geometry.c: bicubic_filter32RGB).  No atomics; the same inputs give the same bits.
 * fv_randaug_ok: host code, the range both serve -- batch in [1, 4096], s_h and s_w in [8, 1024], num_layers in
 *   [1, FV_RANDAUG_MAX_LAYERS].  `layer` is in [0, num_layers).
 * ---------------------------------------------------------------------- */
#define FV_RANDAUG_PLAN_INTS 18
#define FV_RANDAUG_MAX_LAYERS 4
#define FV_RANDAUG_WS_BYTES 768
#define FV_RANDAUG_ROWS 8
#define FV_RA_COPY 0
#define FV_RA_AUTOCONTRAST 1
#define FV_RA_EQUALIZE 2
#define FV_RA_INVERT 3
#define FV_RA_SOLARIZE 4
#define FV_RA_POSTERIZE 5
#define FV_RA_SOLARIZE_ADD 6
#define FV_RA_COLOR 7
#define FV_RA_CONTRAST 8
#define FV_RA_BRIGHTNESS 9
#define FV_RA_SHARPNESS 10
#define FV_RA_AFFINE 11
int fv_randaug_ok(int batch, int s_h, int s_w, int num_layers);
long long fv_randaug_workspace_bytes(int batch);
int fv_randaug_stats(const void* in, const int* plan, void* ws, int batch, int s_h, int s_w, int num_layers, int layer,
                     fv_stream_t stream);
int fv_randaug_apply(const void* in, void* out, const int* plan, const void* ws, int batch, int s_h, int s_w,
                     int num_layers, int layer, fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-side JPEG decode after host entropy decoding, byte for byte what libjpeg-turbo (PIL's
 * `Image.open(...).convert("RGB")`, the reference's datasets.ImageFolder loader) gives.  The serial part stays on the
 * HOST: marker parsing and Huffman decoding (csrc/jpeg_host.cpp, plain C++, no HIP; these two entry points touch no GPU
 * and keep no state -- any number of threads may call them; they report through their return value, not fv_last_error).
 * Everything per pixel runs on the device (csrc/jpeg.hip): dequantisation, the 8 x 8 inverse DCT, fancy chroma
 * upsampling and YCbCr -> RGB, written straight into the pixel pool fv_resample_u8 reads.
 *
 * Served (fv_jpeg_probe): SOF0, 8-bit precision, one interleaved scan of all components, Huffman coding, 8-bit
 * quantisation tables; one component, sampled 1x1 (FV_JPEG_GRAY), or three read as YCbCr with chroma sampled 1x1 and luma
 * 1x1 (FV_JPEG_444), 2x1 (FV_JPEG_422) or 2x2 (FV_JPEG_420).  Everything else is unserved with a FV_JPEG_R_* reason.
 *
 * fv_jpeg_probe(data, nbytes, info): info[FV_JPEG_INFO_INTS] = height, width, components, sampling class (-1 when
 *   unserved), served (0 / 1), reason, MCUs per row, MCU rows.  Returns FV_OK (also for an unserved file: the reason is the
 *   answer) or FV_ERR_INVALID for a null pointer.
 * fv_jpeg_entropy_decode(data, nbytes, window, coef_out, coef_capacity, record): window[4] = x0, y0, w, h is a rectangle
 *   of MCUs inside the image.  MCUs are decoded in file order up to the LAST one the window needs; the quantised
 *   coefficients of the blocks inside the window are written as int16 in NATURAL order, component after component, each a
 *   dense (h * v_i block rows, w * h_i block columns, 64) array starting at coef_out; `coef_capacity` counts int16
 *   ELEMENTS.  Byte stuffing, fill bytes, restart intervals (predictors reset, marker sequence checked), EOB and ZRL are
 *   handled.  Returns FV_OK or a FV_JPEG_E_* code; on an error the record and the coefficients are unspecified and must
 *   not be used (there is no partial result).  Reads only [data, data + nbytes), writes only coef_out[0 : coef_capacity]
 *   and record[0 : FV_JPEG_REC_INTS].  The record, int32:
 *     [0]        1: a JPEG job (0: none -- a sample staged as a decoded array)
 *     [1] [2]    image height, width          [3] components          [4] sampling class
 *     [5..8]     the window: x0, y0, w, h in MCUs
 *     [9..14]    per component the offset of its coefficients in ELEMENTS, low and high 32 bits -- relative to coef_out as
 *                the decoder writes them; the caller adds the offset of coef_out in the pool.  The component's sample
 *                plane lies at the same offset, in bytes, of the plane workspace.
 *     [15] [16]  elements written, low and high    [17] blocks written    [18] MCUs decoded
 *     [19..22]   CALLER: the crop top, left, height, width in image pixels (inside the window's interior: see jpeg.py)
 *     [23] [24]  CALLER: byte offset of the crop's h x w x 3 region in the pixel pool, low and high
 *     [25..31]   0
 *     [32..223]  the quantisation table of each component, 64 words, natural order
 *
 * The two launches read a TABLE in device memory when they RUN (a replayed graph takes the table, the coefficients and
 * the pools of that moment): `batch` records, then batch + 1 int32 prefix sums of the records' block counts, then
 * batch + 1 prefix sums of their pixel quads, ceil(crop h * crop w / 4) -- fv_jpeg_table_ints(batch) words.  Their grids
 * depend on the capacities only (each workgroup takes a contiguous share of the work the table states).  Every coefficient and plane access is checked against `coef_elems`
 * / `plane_bytes` and every pixel write against `pool_bytes`; a record that does not fit is skipped.  No atomics.
 * fv_jpeg_idct: every block: coefficient x table entry in 32-bit integers, jidctint's "islow" inverse DCT (CONST_BITS 13,
 *   PASS1_BITS 2; columns first, (v + 1024) >> 11; then rows, (v + 131072) >> 18), + 128, clamped to 0..255, into the
 *   component's plane (window-local pitch: block columns * 8).  8 lanes per block.  `planes` holds plane_bytes >=
 *   coef_elems bytes, 8-byte aligned; coef 16-byte aligned.
 * fv_jpeg_rgb: every pixel of every crop: luma, chroma upsampled as jdsample's fancy h2v1 / h2v2 upsamplers do over the
 *   TRUE plane sizes ceil(W / h_max) x ceil(H / v_max), jdcolor's 16-bit fixed-point conversion, three bytes into the
 *   pool (HWC, pitch 3 w).  A crop's region must start 4-byte aligned in a 4-byte aligned pool.
 * For coefficient values no encoder writes the pixel values are unspecified (32-bit wrap-around, not libjpeg's 64-bit
 * intermediates and masked range table); memory safety holds regardless.
 *
 * THE PACKED FORM (opt-in; the dense form above stays the default).  A block of a photograph is mostly zeros, and the
 * dense form sends all 64 coefficients of it over the link.  The packed form sends a 64-bit mask and the non-zero values.
 * A sample's blocks are numbered as the dense form numbers them: component after component, each row-major over its
 * (block rows, block columns) of the MCU window.  Per sample ONE contiguous piece of the coefficient pool holds
 *   headers  `blocks` headers of 16 bytes, the first 16-byte aligned; a header is four little-endian uint32 words:
 *              w0, w1   low and high word of a 64-bit mask: bit k (NATURAL order, k = 8 * row + column) is set exactly when
 *                       AC coefficient k is non-zero; bit 0 is always clear
 *              w2       bits 0..30: byte offset of the block's values relative to the sample's VALUE BASE, even;
 *                       bit 31 `wide`: set exactly when some AC value of the block lies outside -128 .. 127
 *              w3       low 16 bits: the DC coefficient as int16; high 16 bits 0
 *   values   directly behind the headers (value base = first header + 16 * blocks): per block its non-zero AC
 *            coefficients in ascending natural index, int8 each when `wide` is clear, little-endian int16 each when it is
 *            set.  Every block's values start at an even offset: a block with an odd number of value bytes is followed by
 *            one pad byte of 0 (so the bytes written are even).  A block with mask 0 has no values (its offset is where
 *            the next block's values start).
 * It is shaped for 8 lanes per block, lane r owning natural row r: lane r's coefficients are the set bits of mask byte r,
 * its first value is number popcount(mask & ((1 << 8 r) - 1)) of the block.  No zigzag table on the device, no scatter; a
 * DC-only block is mask == 0, known before any value is loaded.
 * fv_jpeg_packed_bound(blocks): the worst case of a sample, blocks * (16 + 126) bytes (0 for blocks < 0).
 * fv_jpeg_entropy_decode_packed(data, nbytes, window, out, out_capacity_bytes, record): parsing, window, early stop and
 *   error codes of fv_jpeg_entropy_decode; writes the headers at `out` (16-byte aligned, else FV_ERR_INVALID) and the
 *   values from out + 16 * blocks.  The capacity is checked as it goes: FV_JPEG_E_CAPACITY without a write at or beyond
 *   out + out_capacity_bytes.  On an error there is no partial result.  The record differs from the dense one in
 *     [0]        2: a packed JPEG job
 *     [9..14]    per component the byte offset of its PLANE, low and high: 64 x the blocks in front of it; the caller adds
 *                the sample's base in the plane workspace (a multiple of 8)
 *     [15] [16]  BYTES written, low and high
 *     [25] [26]  byte offset of the first header, [27] [28] of the value base, low and high -- relative to `out`; the
 *                caller adds the offset of `out` in the pool (a multiple of 16)
 *   and in nothing else (blocks, MCUs decoded and the quantisation tables included).
 * fv_jpeg_idct_packed(pool, pool_bytes, table, planes, plane_bytes, batch, stream): fv_jpeg_idct on records with [0] == 2
 *   (others are skipped, as fv_jpeg_idct skips these): same table, same contiguous share of blocks per workgroup, a grid
 *   from min(pool_bytes / 16, plane_bytes / 64) alone, the same planes bit for bit.  Every header and value access is
 *   checked against `pool_bytes` (values against its whole 4-byte words: they are read as aligned words) and every plane
 *   store against `plane_bytes`; a record or a block that does not fit is skipped.  No atomics.  `pool` 16-byte aligned, `planes` 8.  fv_jpeg_rgb reads planes only and takes the records of
 *   either form.
 *
 * THE INDEX (opt-in; nothing above changes).  Huffman decoding is serial only because nobody knows where MCU n starts in
 * the bit stream and what the DC predictors are there.  A file that is read every epoch is decoded once on the host into
 * a sidecar index that records both for every GROUP -- S = segment_mcus consecutive MCUs of one MCU row, the last group
 * of a row shorter -- and from then on the device decodes each group on its own, one lane per group
 * (csrc/jpeg_huff_core.h is the decoder, the same text on host and device), and the host only copies bytes.  A crop
 * touches only the groups that meet its MCU window.  Indexed: what fv_jpeg_probe serves, without a restart interval
 * (FV_JPEG_R_RESTART) and with one pair of Huffman tables for both chroma components (FV_JPEG_R_CHROMA_TABLES), in a
 * file of less than 2^31 bytes.  The index is one little-endian blob of 32-bit words:
 *     [0]        FV_JPEG_INDEX_MAGIC          [1] FV_JPEG_INDEX_VERSION
 *     [2] [3]    bytes of the file, low and high     [4] [5] FNV-1a 64-bit hash of the file's bytes, low and high
 *     [6] [7]    image height, width          [8] sampling class          [9] components
 *     [10] [11]  MCUs per row, MCU rows       [12] S        [13] groups per row, ceil([10] / S)       [14] groups, [13] * [11]
 *     [16] [17]  offset of the first entropy-coded byte, low and high       [15], [18..31] 0
 *     [32..223]  the quantisation table of each component, 64 words, natural order: words [32..223] of the record
 *     [224..1647] four Huffman tables of 356 words -- DC of component 0, DC of the chroma components, AC of component 0,
 *                AC of chroma (a one-component file repeats its own) -- each as the device reads it:
 *                  words 0..255    512 uint16: index = the next 9 bits of the stream; length << 8 | symbol of a code of at
 *                                  most 9 bits, 0 for a longer one
 *                  words 256..273  maxcode[0..17], int32: the largest code of each length, -1: none; [17] = 2^31 - 1
 *                  words 274..290  valoff[0..16], int32: index of the first symbol of a length minus its first code
 *                  word 291        symbols                words 292..355  the symbols, bytes
 *     [1648 ..]  one ENTRY of four words per group, in file order (MCU row after MCU row), then one more, the END SENTINEL
 *                (the position behind the last MCU): byte, bit, DC predictors of components 0 and 1 as int16 in the low
 *                and high half, predictor of component 2 as int16 in the low half
 *   An entry's position is that of the group's first bit in the byte-stuffed stream: `byte` is the offset IN THE FILE of
 *   the data byte that holds it, `bit` (0..7, the most significant first) the bits of that byte that belong to the group
 *   before.  It moves over whole stuffed bytes -- a data 0xFF and its stuffed 0x00 are one step -- so it never rests on a
 *   stuffed 0x00; the end sentinel may rest on the marker that ends the scan.  The predictors are those before the group.
 * fv_jpeg_index_bound(mcus_x, mcus_y, segment_mcus): the bytes of an index, FV_JPEG_INDEX_HEAD_BYTES + 16 * (groups + 1);
 *   0 outside 1 <= mcus <= 8192 per axis, 1 <= segment_mcus <= 65536.
 * fv_jpeg_build_index(data, nbytes, segment_mcus, out, out_capacity_bytes): host, no state.  Returns the bytes written, or
 *   a negative code and an unspecified `out`: FV_JPEG_E_UNSERVED for a file that is not indexed -- the first int32 of `out`
 *   then holds the FV_JPEG_R_* reason (out_capacity_bytes >= 4) -- FV_JPEG_E_CAPACITY, or the decoder's code for a stream
 *   it gives up on (fill bytes inside the scan are among them: FV_JPEG_E_TRUNCATED).  Such files keep
 *   fv_jpeg_entropy_decode.
 * fv_jpeg_index_stage(data, nbytes, index, index_bytes, window, verify, pool, pool_capacity_bytes, pool_used, coef_base,
 *   record, stream_record): host, no state, no Huffman code decoded.  Checks the index against the file -- magic, version
 *   and the header's consistency (FV_JPEG_E_INDEX_FORMAT), nbytes and, with `verify`, the hash (FV_JPEG_E_INDEX_FILE), the
 *   window (FV_JPEG_E_WINDOW), and that every entry it will use, the one behind each row's last group included, lies
 *   inside the scan with bit <= 7 and in file order (FV_JPEG_E_INDEX_ENTRY) -- then appends to the host stream pool `pool`
 *   (16-byte aligned) from the next multiple of 16 at or above *pool_used: the four tables, the entries of the groups
 *   that meet the window (row after row of the window, `group columns` per row), and the bytes of the file from the
 *   first of those groups to two bytes past the start of the group behind the last (clamped to the file), zero-padded to
 *   16.  FV_JPEG_E_CAPACITY without a write if that does not fit; *pool_used is advanced.  Writes the ordinary dense record
 *   ([0] = 1; [18] = the MCUs fv_jpeg_entropy_decode would have decoded; [19..24] are the caller's as ever) whose
 *   component offsets are `coef_base` (elements, a multiple of 8: where the caller reserved the window's coefficients)
 *   plus the decoder's, and the STREAM RECORD, FV_JPEG_STREAM_REC_INTS int32:
 *     [0]        1: an indexed job (0: none)          [1] sampling class
 *     [2..5]     the window: x0, y0, w, h in MCUs     [6] MCUs per row of the image      [7] S
 *     [8] [9]    the first group column the window meets, and how many
 *     [10..15]   per component the offset of its coefficients in the coefficient pool, elements, low and high
 *     [16] [17]  byte offset of the tables in the stream pool, [18] [19] of the entries, [20] [21] of the file bytes
 *     [22]       file bytes staged       [23] offset in the file of the first of them
 *     [24]       DEVICE: the status, 0 or the FV_JPEG_ST_* of a lane that gave up        [25..31] 0
 * fv_jpeg_stream_table_ints(batch): the words of the STREAM TABLE in device memory: `batch` stream records, then
 *   batch + 1 int32 prefix sums of the records' lanes ([9] * [5], 0 for a record with [0] == 0).
 * fv_jpeg_huff(stream_pool, stream_bytes, stream_table, coef, coef_elems, batch, stream): in front of fv_jpeg_idct.  One
 *   lane per group: it finds its sample by a search over the prefix sums, decodes the group's MCUs from its entry and
 *   writes all 64 coefficients, zeros included, of every block inside the window where fv_jpeg_entropy_decode would have
 *   put them; blocks outside the window are decoded and dropped.  Every block of a window belongs to exactly one lane: no
 *   memset, no atomics, and a replay never sees stale coefficients.  The grid is from stream_bytes alone (a lane needs a
 *   16-byte entry).  Every table, entry and stream read is checked against stream_bytes (the stream against the staged
 *   range; beyond it and from a marker on the reader delivers zero bits), every store against coef_elems, and every loop
 *   is bounded independently of the stream: a corrupt stream or index gives unspecified coefficients and a non-zero
 *   status word ([24], a plain store), never a hang or an access out of range.  stream_pool and coef 16-byte aligned.
 *
 * ENTRIES MADE ON THE DEVICE (opt-in; nothing above changes).  A file without a sidecar index: the device finds the group
 * starts itself.  A baseline Huffman stream re-synchronises -- a decoder started at a wrong bit soon falls into step with
 * the true one -- so the scan is cut into SUBSEQUENCES of `subseq_bytes` bytes of the file (a boundary that falls on a
 * stuffed 0x00 lies one byte later), each is decoded from its first bit with (block 0, a DC code next), and then again
 * from its predecessor's exit state until a round changes nothing; an INVALID exit state -- a speculative decode that met a
 * bad code or a run past 63 -- is not handed on, its successor keeps its own state meanwhile.  Subsequence 0 starts from the scan's true start, so
 * after round i subsequence i is right: the fixed point is the serial decoder's, whether or not the stream synchronised.
 * A prefix sum over the subsequences' MCU counts and DC sums gives every MCU start its number and predictors, and the
 * starts the window needs are written as ENTRIES of THE INDEX, where fv_jpeg_huff reads them.  csrc/jpeg_sync_core.h is the
 * decoder, one text for host and device.  Served: what fv_jpeg_build_index serves.
 * fv_jpeg_sync_stage(data, nbytes, window, segment_mcus, subseq_bytes, max_scan_bytes, pool, pool_capacity_bytes, pool_used,
 *   scratch_capacity_records, scratch_used, coef_base, record, stream_record, job): host, no state, no Huffman code
 *   decoded.  Parses the markers; refuses what fv_jpeg_build_index refuses -- FV_JPEG_E_UNSERVED with job[0] = 0 and the
 *   FV_JPEG_R_* reason in job[1] (restart intervals and separate chroma table pairs among them), FV_JPEG_E_TRUNCATED for
 *   fill bytes inside the scan and for an empty scan -- FV_JPEG_E_WINDOW, and a scan (from the first entropy-coded byte to
 *   the first 0xFF that no 0x00 follows) of more than min(max_scan_bytes, 2^26) bytes: FV_JPEG_E_SCAN_SIZE.  subseq_bytes:
 *   a power of two in [16, 1024] (a symbol is at most 31 bits: 16 bytes always hold a symbol start); segment_mcus as S
 *   above.  Appends to the host stream pool from the next multiple of 16 at or above *pool_used: the four tables, a
 *   RESERVED region of 16 bytes per group that meets the window, filled with 0xFF -- an entry nobody wrote has bit > 7,
 *   and fv_jpeg_huff's lane returns FV_JPEG_ST_RECORD for it -- and the whole scan, zero-padded to 16; takes
 *   ceil(scan bytes / subseq_bytes) records of the scratch buffer from *scratch_used on -- at most FV_JPEG_SYNC_MAX_SUBSEQS,
 *   a longer scan is FV_JPEG_E_SCAN_SIZE too: the cap bounds the rounds of a launch.  FV_JPEG_E_CAPACITY if either does
 *   not fit: then nothing is written and the counters stay; on success both counters are advanced.  Writes the dense record and the stream record
 *   fv_jpeg_index_stage writes ([22] the scan's bytes, [23] its offset in the file), and the SYNC JOB,
 *   FV_JPEG_SYNC_JOB_INTS int32:
 *     [0]        1: a job (0: none)        [1] sampling class        [2..5] the window: x0, y0, w, h in MCUs
 *     [6]        MCUs per row of the image [7] S                     [8] [9] first group column the window meets, how many
 *     [10] [11]  byte offset of the scan in the stream pool, low and high       [12] its bytes      [13] its offset in the file
 *     [14]       the bit of the first byte the scan starts at (0)     [15] subseq_bytes      [16] subsequences
 *     [17] [18]  byte offset of the entry region in the stream pool, [19] [20] of the tables
 *     [21] [22]  the first scratch record of the job                  [23] MCU rows of the image
 *     [24]       DEVICE: the status -- 0, FV_JPEG_ST_SYNC_JOB (a job that does not fit its buffers: nothing was read) or
 *                FV_JPEG_ST_SYNC_LOST (the MCU starts in front of the first exit state that stays INVALID -- a bad code, a run
 *                past 63, the end of the data -- do not reach the last group start the window needs: no entry was written)
 *     [25]       DEVICE: the rounds that changed a state
 *     [26..28]   fv_jpeg_sync_host ONLY (the device leaves them 0), what speculation was worth, over all subsequences but
 *                the last: speculative exit states that were INVALID where the final one is not, those that were valid but
 *                not the final one, and the longest run of the former          [29..31] 0
 * fv_jpeg_sync_table_ints(batch): the words of the SYNC TABLE in device memory: `batch` sync jobs.
 * fv_jpeg_sync(stream_pool, stream_bytes, sync_table, scratch, scratch_bytes, batch, stream): in front of fv_jpeg_huff.
 *   One workgroup per sample, a grid of `batch`; a slot without a job returns at once.  `scratch`: FV_JPEG_SYNC_REC_BYTES
 *   per subsequence, contents unspecified before and after.  Writes the entries of the groups the window needs into the
 *   reserved region of the stream pool, each by exactly one lane, and words [24] [25] of the job.  Every job word is
 *   checked against stream_bytes and scratch_bytes, every stream read against the staged scan, every loop is bounded by
 *   the job's byte and subsequence counts; plain stores, no atomics: a corrupt stream gives a status, or entries that are
 *   the serial decoder's up to the damage, never a hang or an access out of range.  stream_pool and scratch 16-byte aligned.
 * fv_jpeg_sync_host(pool, pool_bytes, job, scratch, scratch_records): host; the same passes and rounds over one job, one
 *   subsequence after the other, on the HOST stream pool: fills the entry region and words [24] [25] as the device does.
 * ---------------------------------------------------------------------- */
#define FV_JPEG_INFO_INTS 8
#define FV_JPEG_REC_INTS 224
#define FV_JPEG_444 0
#define FV_JPEG_422 1
#define FV_JPEG_420 2
#define FV_JPEG_GRAY 3
#define FV_JPEG_R_OK 0
#define FV_JPEG_R_PROGRESSIVE 1
#define FV_JPEG_R_ARITHMETIC 2
#define FV_JPEG_R_PRECISION 3
#define FV_JPEG_R_COMPONENTS 4
#define FV_JPEG_R_COLOUR 5
#define FV_JPEG_R_SAMPLING 6
#define FV_JPEG_R_SCANS 7
#define FV_JPEG_R_TABLES16 8
#define FV_JPEG_R_MALFORMED 9
#define FV_JPEG_R_FRAME 10
#define FV_JPEG_E_UNSERVED (-10)
#define FV_JPEG_E_TRUNCATED (-11)
#define FV_JPEG_E_CODE (-12)
#define FV_JPEG_E_RUN (-13)
#define FV_JPEG_E_RESTART (-14)
#define FV_JPEG_E_CAPACITY (-15)
#define FV_JPEG_E_WINDOW (-16)
int fv_jpeg_probe(const void* data, long long nbytes, int* info);
int fv_jpeg_entropy_decode(const void* data, long long nbytes, const int* window, int16_t* coef_out,
                           long long coef_capacity, int* record);
long long fv_jpeg_table_ints(int batch);
int fv_jpeg_idct(const void* coef, long long coef_elems, const int* table, void* planes, long long plane_bytes, int batch,
                 fv_stream_t stream);
int fv_jpeg_rgb(const void* planes, long long plane_bytes, const int* table, void* pool, long long pool_bytes, int batch,
                fv_stream_t stream);
long long fv_jpeg_packed_bound(long long blocks);
int fv_jpeg_entropy_decode_packed(const void* data, long long nbytes, const int* window, void* out,
                                  long long out_capacity_bytes, int* record);
int fv_jpeg_idct_packed(const void* pool, long long pool_bytes, const int* table, void* planes, long long plane_bytes,
                        int batch, fv_stream_t stream);
#define FV_JPEG_INDEX_MAGIC 0x58494A46u
#define FV_JPEG_INDEX_VERSION 1
#define FV_JPEG_INDEX_HEAD_BYTES 6592
#define FV_JPEG_STREAM_REC_INTS 32
#define FV_JPEG_R_RESTART 11
#define FV_JPEG_R_CHROMA_TABLES 12
#define FV_JPEG_E_INDEX_FORMAT (-17)
#define FV_JPEG_E_INDEX_FILE (-18)
#define FV_JPEG_E_INDEX_ENTRY (-19)
#define FV_JPEG_ST_CODE 1
#define FV_JPEG_ST_RUN 2
#define FV_JPEG_ST_CAPACITY 3
#define FV_JPEG_ST_RECORD 4
long long fv_jpeg_index_bound(int mcus_x, int mcus_y, int segment_mcus);
long long fv_jpeg_build_index(const void* data, long long nbytes, int segment_mcus, void* out, long long out_capacity_bytes);
int fv_jpeg_index_stage(const void* data, long long nbytes, const void* index, long long index_bytes, const int* window,
                        int verify, void* pool, long long pool_capacity_bytes, long long* pool_used, long long coef_base,
                        int* record, int* stream_record);
long long fv_jpeg_stream_table_ints(int batch);
int fv_jpeg_huff(const void* stream_pool, long long stream_bytes, int* stream_table, void* coef, long long coef_elems,
                 int batch, fv_stream_t stream);
#define FV_JPEG_SYNC_JOB_INTS 32
#define FV_JPEG_SYNC_REC_BYTES 32
#define FV_JPEG_SYNC_MAX_SUBSEQS 16384
#define FV_JPEG_E_SCAN_SIZE (-20)
#define FV_JPEG_ST_SYNC_JOB 5
#define FV_JPEG_ST_SYNC_LOST 6
int fv_jpeg_sync_stage(const void* data, long long nbytes, const int* window, int segment_mcus, int subseq_bytes,
                       long long max_scan_bytes, void* pool, long long pool_capacity_bytes, long long* pool_used,
                       long long scratch_capacity_records, long long* scratch_used, long long coef_base, int* record,
                       int* stream_record, int* job);
int fv_jpeg_sync_host(void* pool, long long pool_bytes, int* job, void* scratch, long long scratch_records);
long long fv_jpeg_sync_table_ints(int batch);
int fv_jpeg_sync(void* stream_pool, long long stream_bytes, int* sync_table, void* scratch, long long scratch_bytes, int batch,
                 fv_stream_t stream);

/* ------------------------------------------------------------------------
 * Device-side cell-image augmentation: the pixel work of the reference's CellAugmentation(is_train=True)
 * (cell_imaging/transformations/cell.py:104-149) in front of A.Normalize (fv_patch_unfold_chan_u8): pad + crop, one of
 * {horizontal flip, vertical flip, rotation by any angle}, defocus, coarse dropout.  The host draws and turns every draw
 * into numbers (fastvim_amd/cellaug.py); the device applies them.  The arithmetic below is the contract; it is restated in
 * numpy at tests/cellaug_ref.py.
 *
 *   pool   uint8, `pool_bytes` long: the sources back to back, each (channels, H, W) planar with packed rows; a source
 *          may start at any byte (fastvim_amd/cellaug.py starts each on a 16-byte boundary).
 *   plan   (batch, FV_CELLAUG_PLAN_INTS) int32 in DEVICE memory, 8-byte aligned, read when the kernels RUN.
 *          THE CELL RECORD, per sample:
 *            [0] [1]      byte offset of the source in the pool, low and high 32 bits
 *            [2] [3]      H, W of the source, each in [1, 4096]
 *            [4] [5]      oy, ox: crop pixel (y, x) is src[c][y - oy][x - ox] inside the source and 0 outside
 *                         (oy = pad_top - crop_top, likewise ox; |oy|, |ox| <= 8192)
 *            [6]          geometry: FV_CELLAUG_NONE, _HFLIP (out[y][x] = crop[y][S-1-x]), _VFLIP (crop[S-1-y][x]), _ROTATE
 *            [7]          defocus != 0: correlate with the kernel at [24..104]
 *            [8]          number of holes, 0 .. FV_CELLAUG_MAX_HOLES
 *            [9..11]      unused, 0
 *            [12..23]     m0 .. m5, six fp64 (low word first): the INVERSE (destination to source) affine map of a
 *                         rotation, sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5
 *            [24..104]    the 9 x 9 defocus kernel, fp32 bits, row-major
 *            [105..107]   unused, 0
 *            [108..171]   the holes, four words each: y1, x1, y2, x2 (y2, x2 exclusive) in output coordinates
 *            [172..175]   unused, 0
 *   out    (batch, channels, S, S) uint8, planar, contiguous; 4-byte stores when S % 4 == 0 and the buffers allow them.
 *
 * fv_cellaug_geom: pool -> out.  A rotation is the fixed-point scheme of an 8-bit bilinear warpAffine; after the fp64
 *   products (no contraction) everything is integer:
 *     adelta[x] = rint(m0 x 1024), bdelta[x] = rint(m3 x 1024)
 *     X0[y] = rint((m1 y + m2) 1024) + 16,  Y0[y] = rint((m4 y + m5) 1024) + 16
 *     X = (X0 + adelta) >> 5, sx = X >> 5, fx = X & 31; the same for Y
 *     taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1), each index reflected (REFLECT_101: 2 1 | 0 1 2 ..) within the
 *     S x S crop and only then mapped to the source; weights (32-fy)(32-fx)32, (32-fy)fx 32, fy(32-fx)32, fy fx 32
 *     out = (sum w p + 16384) >> 15
 * fv_cellaug_filter: in -> out, both (batch, channels, S, S) and not overlapping.  With defocus, out = clamp(rint(acc), 0,
 *   255) where acc runs over the 81 taps in row-major order, skipping weights that are exactly 0, in fp32 with the product
 *   and the add rounded separately (no FMA), borders REFLECT_101; without, a copy.  Then 0 inside each hole.
 * Both serve batch in [1, 4096], channels in [1, 16], S in [8, 512].  A record outside the ranges above, or whose source
 * does not lie inside the pool, reads nothing and gives zeros.  No atomics; every output byte has one owner.
 * ---------------------------------------------------------------------- */
#define FV_CELLAUG_PLAN_INTS 176
#define FV_CELLAUG_TAPS 9
#define FV_CELLAUG_MAX_HOLES 16
#define FV_CELLAUG_NONE 0
#define FV_CELLAUG_HFLIP 1
#define FV_CELLAUG_VFLIP 2
#define FV_CELLAUG_ROTATE 3
int fv_cellaug_geom(const void* pool, long long pool_bytes, const int* plan, void* out, int batch, int channels, int size,
                    fv_stream_t stream);
int fv_cellaug_filter(const void* in, const int* plan, void* out, int batch, int channels, int size, fv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTVIM_HIP_H */
