/*
 * xvector_hip.h -- C ABI of libxvector_hip.so: the MI355X (gfx950) x-vector extraction hot path.
 *
 * This is the drop-in boundary for ONE path of BUTSpeechFIT/x-vector-kaldi-tf: the forward pass that
 * Model.make_embedding (local/tf/models.py:356-432) evaluates once per utterance chunk through
 * sess.run(embed_layer-0/scores) (local/tf/models.py:414).  The reference has no native code and no
 * FFI; what it binds for this path are the stock TensorFlow ops listed next to each entry point
 * below.  A maintainer replaces the sess.run call by these calls (see INTEGRATION.md for the ctypes
 * stub); the Python twin in x-vector-kaldi-tf_amd/local/tf/models.py does exactly that.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (e.g. a torch-ROCm tensor's data_ptr);
 *    the library never allocates, frees or synchronises; work is enqueued on `stream`
 *    (hipStream_t passed as void*; NULL = the null stream).
 *  - return value: 0 on success, otherwise a hipError_t / negative argument-error code;
 *    xv_last_error() returns a thread-local message.  No exceptions cross the ABI.
 *  - arithmetic: three GEMM arithmetics behind the same fp32-in / fp32-out contraction, all accumulating in fp32:
 *      *_f32      exact IEEE fp32 (f32-input MFMA: exact fp32 products) -- the reference's own arithmetic;
 *      *_bf16x3   every operand split x = hi + lo into two bf16, a product formed as hi*hi + hi*lo + lo*hi on the bf16 matrix
 *                 cores (16x the f32-MFMA rate; the dropped lo*lo term is ~2^-16 relative): ~5e-6 relative L2 on the x-vector;
 *      *_f16bf8   hi = fp16(x), the two cross terms through ONE block-scaled e5m2 MFMA at twice the 16-bit rate (csrc/xv_split8.h):
 *                 ~1.3e-5.  This is what the host side runs BY DEFAULT for the hidden frame-level layers (layer 0 and the segment
 *                 FCs stay bf16x3) -- per checkpoint, after an accuracy probe admitted it (xvector_amd/engine.py select_model;
 *                 DESIGN.md 5.1); a model whose f16bf8 results drift from bf16x3 runs as bf16x3, then as f32.
 *    All are inside the 1e-4 parity bar against the fp64 oracle.  Pooling, epilogues and the chunk average are fp32 in all three.
 *
 * Ragged batch layout ("packed rows with gaps")
 *    A batch of utterance chunks is ONE row-major matrix x[R, C].  Chunk b owns rows
 *    [row_start[b], row_start[b]+row_len[b]).  Between consecutive chunks (and before the first /
 *    after the last) the caller leaves >= G all-zero "gap" rows, G = max over layers of
 *    (K-1)*dilation/2.  Because the gaps are zero, a temporal tap that reaches past a chunk's own
 *    first/last frame reads zeros -- exactly tf.nn.conv1d's per-utterance SAME padding at batch 1
 *    (local/tf/models.py:60,410) -- with no per-tap bounds logic in the kernel.  row_valid[R]
 *    (1 = frame, 0 = gap) lets each layer's epilogue write zeros back into the gap rows, so the
 *    invariant holds for the next layer.  Rows outside [0,R) read as zero and are never written.
 */
#ifndef XVECTOR_HIP_H_
#define XVECTOR_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XV_ACT_NONE 0
#define XV_ACT_RELU 1   /* tf.nn.relu            local/tf/models.py:64   */
#define XV_ACT_LRELU 2  /* tf.nn.leaky_relu      local/tf/models.py:912  (alpha[0]) */
#define XV_ACT_PRELU 3  /* tf_block.prelu        local/tf/tf_block.py:38-47 (alpha[Cout]) */

#define XV_ERR_BAD_ARG (-1)
#define XV_ERR_UNSUPPORTED (-2)

/* Library / ABI version (increments whenever an entry point is added or changed; currently 44). */
int xv_version(void);
/* Thread-local description of the last non-zero return. */
const char *xv_last_error(void);
/* Process-wide launch tuning (no TF counterpart; the analogue of the session's ConfigProto knobs,
 * local/tf/models.py:361-363).  Results do not depend on any of these.
 *   XV_TUNE_TILE_ROWS  rows per workgroup tile of the bf16x3 / f16bf8 GEMMs with split-format input: 128 (4 waves, two
 *                      workgroups per CU), 256 (8 waves, one per CU), 512 / 1024 (f16bf8: the 256 x 256 tile on the 32 x 32 /
 *                      16 x 16 MFMA shapes where the shape allows it, else as 0; bf16x3: as 256), 0 = built-in choice.
 *   XV_TUNE_FP32_GEMM  form of the exact-fp32 GEMM where several exist (bit-identical results): 1 = register-staged (tdnn_gemm_kernel),
 *                      2 = fed by LDS-DMA on 32-channel slabs (tdnn_gemm_dma_kernel), 3 = as 2 with the K = 1 layers on 16-channel
 *                      slabs, three workgroups per CU (tdnn_gemm_k1_kernel), 0 = built-in choice (3).
 *   XV_TUNE_FIRST_TILES  16-frame tiles per wave of the first-layer kernel (xv_tdnn_first_*): 1..4096, 0 = spread the rows evenly
 *                      over one workgroup per CU (tests use small values to walk through several groups of tiles on small inputs). */
#define XV_TUNE_TILE_ROWS 1
#define XV_TUNE_FIRST_TILES 2
#define XV_TUNE_FP32_GEMM 3
int xv_set_tuning(int key, int value);

/* One-off weight re-layout.  TF stores a conv kernel as w[K, Cin, Cout] == row-major [K*Cin, Cout]
 * (local/tf/models.py:56-57) and an FC weight as w[In, Out] (local/tf/models.py:83); the GEMM kernel
 * wants each output channel's reduction vector contiguous: wp[Cout][K*Cin].  kred = K*Cin (or In). */
int xv_pack_weights_f32(const float *w, int kred, int cout, float *wp, void *stream);

/* Fold tf.nn.batch_normalization's inference form (local/tf/tf_block.py:25-26, epsilon 1e-3 from
 * tf_block.py:9) into a per-channel affine:  scale = gamma*rsqrt(var+eps), shift = beta - mean*scale. */
int xv_fold_bn_f32(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                   int c, float *scale, float *shift, void *stream);

/* Move a producer layer's BN shift into its consumer (one-off at load; see tap_bias of xv_tdnn_layer_f16bf8).  w[K, Cin, Cout]
 * are the consumer's fp32 weights, shift[Cin] the producer's:
 *     tap_bias[t][o] = sum_c shift[c] * w[t][c][o]          ([K][Cout]; may be NULL when only the sum is wanted, e.g. K = 1)
 *     bias_full[o]   = bias[o] + sum_t tap_bias[t][o]       (bias may be NULL = 0)
 * accumulated in fp64 in a fixed order (taps, then input channels, ascending) and rounded to fp32 once. */
int xv_fold_shift_taps_f32(const float *w, const float *shift, const float *bias, int K, int cin, int cout, float *tap_bias,
                           float *bias_full, void *stream);

/* Frame-level TDNN layer over a whole ragged batch.  Replaces, per layer,
 *   tf.nn.conv1d(stride 1, SAME) / tf.nn.convolution(dilation_rate)  local/tf/models.py:60, :579-580
 *   + tf.nn.bias_add (:61) + relu|leaky_relu|prelu (:64, :912, tf_block.py:38-47)
 *   + batch_norm_wrapper eval branch (tf_block.py:25-26).
 *     z[r,o]  = bias[o] + sum_{k<K} sum_{c<Cin} x[r + (k-(K-1)/2)*dilation, c] * w[k,c,o]
 *     y[r,o]  = row_valid[r] ? act(z)*bn_scale[o] + bn_shift[o] : 0
 *   x[R,Cin] with row stride ldx; wp = xv_pack_weights_f32(w) i.e. [Cout][K*Cin];
 *   bn_scale/bn_shift may be NULL (identity); act_alpha: [1] for LRELU, [Cout] for PRELU;
 *   row_valid may be NULL (all rows valid); y_preact (row stride ldy) may be NULL, else receives z.
 *   K odd, (K-1)*dilation <= 8.  Implicit-im2col GEMM on v_mfma_f32_32x32x2_f32. */
int xv_tdnn_layer_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias,
                      const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha,
                      int K, int dilation, int cout, const uint8_t *row_valid, float *y, int ldy,
                      float *y_preact, void *stream);

/* The FIRST frame-level layer (models.py:54-67 on the feature rows) as a K = 1 GEMM over OVERLAPPING rows.  The packed feature rows
 * x[R, ldx] lie back to back (ldx = the feature dimension padded to a multiple of 4, padding columns zero), so the K-tap window
 * of frame r IS the contiguous span of K * ldx floats that starts at x + (r - (K-1)/2) * ldx: no im2col, no taps -- the exact-fp32
 * GEMM kernels read "row r" from there (DMA-fed: rows before the buffer or past its end read as zeros through the buffer
 * descriptor's range check).  wp = xv_pack_weights_rows_f32(w[K,Cin,Cout]): [Cout][roundup32(K * ldx)] floats with w[k][c][o] at
 * column k * ldx + c and zeros elsewhere (xv_packed_weights_rows_f32_floats; 0 = unsupported: K odd, Cin <= ldx, ldx % 4 == 0).
 * Same products as xv_tdnn_layer_f32, summed in another order (tap-major): not bit-identical to it; used by the "fp32tc" path.
 * x, y and the per-column parameters 16-byte aligned; gap rows must be zero as everywhere (dilation 1 only). */
size_t xv_packed_weights_rows_f32_floats(int K, int cin, int ldx, int cout);
int xv_pack_weights_rows_f32(const float *w, int K, int cin, int ldx, int cout, float *wp, void *stream);
int xv_tdnn_layer_rows_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias, const float *bn_scale,
                           const float *bn_shift, int act_kind, const float *act_alpha, int K, int cout, const uint8_t *row_valid,
                           float *y, int ldy, void *stream);

/* ---- "fp32tc": the wide-context layers with fewer multiplications (Toom-Cook F(2, K) over time; csrc/xv_toom.hip) -------------
 * Same layer as xv_tdnn_layer_f32 (models.py:54-67) for K in {3, 5, 7} (the default topology's layers 1 and 2, models.py:28 -- 74 % of
 * the network's multiplications; the dilated class's K = 3 layers, models.py:545-548,579-585): two output rows are formed from K + 1
 * products of TRANSFORMED input rows and TRANSFORMED taps instead of 2 K products (0.67 / 0.60 / 0.57 of the MFMA work), exact fp32
 * products, fp32 accumulation.  Not bit-identical to xv_tdnn_layer_f32 (another rounding, same accuracy class), hence its own
 * entry points.
 *   wp = xv_pack_weights_toom_f32(w[K,Cin,Cout]): [Cout][(K+1)*Cin] floats (xv_packed_weights_toom_f32_floats; 0 = unsupported);
 *   xv_toom_supported: K in {3,5,7}, dilation 1..8, Cin % 32 == 0, Cout % 4 == 0; the layer call additionally needs 16-byte aligned
 *   x / y rows and per-column parameters (else XV_ERR_UNSUPPORTED: use xv_tdnn_layer_f32).
 * xv_tdnn_layer_toom_dilated_f32: tf.nn.convolution(dilation_rate = d) (models.py:579-585) as d independent undilated problems over
 * the rows sub, sub + d, sub + 2 d, ... (one launch); its row pairs are rows (r, r + d) with floor(r / d) even.
 * Row pairs sit on fixed global rows: chunks should start on multiples of 2 d rows (then a chunk's bits do not depend on its
 * neighbours); xv_tdnn_layer_toom_f32 is the d = 1 call. */
int xv_toom_supported(int K, int dilation, int cin, int cout);
size_t xv_packed_weights_toom_f32_floats(int K, int cin, int cout);
int xv_pack_weights_toom_f32(const float *w, int K, int cin, int cout, float *wp, void *stream);
int xv_tdnn_layer_toom_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias, const float *bn_scale,
                           const float *bn_shift, int act_kind, const float *act_alpha, int K, int cout, const uint8_t *row_valid,
                           float *y, int ldy, void *stream);
int xv_tdnn_layer_toom_dilated_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias, const float *bn_scale,
                                   const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                                   const uint8_t *row_valid, float *y, int ldy, void *stream);

/* ---- bf16x3 split-precision twins (same contraction, fp32-class accuracy, bf16 matrix cores) ----------------
 *
 * Tensor formats for xv_tdnn_layer_bf16x3:
 *   XV_FMT_F32    row-major fp32, row stride ld (Cin, ld multiples of 4, 16-byte aligned).
 *   XV_FMT_SPLIT  "split" activations: for row r and 32-channel slab s, 128 bytes at
 *                 ((r * ceil(C/32) + s) * 128): 8 slots of 16 B; logical slot t = plane*4 + (k>>3) holds channels
 *                 s*32 + 8*(k>>3) .. +7 of plane hi (0) / lo (1) as bf16; it is stored at physical slot
 *                 t ^ ((r>>1)&7).  value = float(hi) + float(lo).  Same bytes/element as fp32.  The halo tile of a
 *                 layer is then a linear global->LDS DMA.  A split INPUT buffer must be readable (and finite, e.g.
 *                 zero) for rows [-XV_SPLIT_PAD_BEFORE, R + XV_SPLIT_PAD_AFTER) around the pointer to row 0;
 *                 channels >= C inside the last slab are written as zero by the producing layer.
 *   xv_split_row_bytes(C) = ceil(C/32)*128.  xv_split_encode_f32 / xv_split_decode_f32 convert fp32 rows <-> split
 *   (tooling and tests; the layers read/write the format directly).
 * Weights: xv_pack_weights_bf16x3 turns TF's w[K,Cin,Cout] into xv_packed_weights_bf16x3_bytes(K,Cin,Cout) bytes of
 *   16 KB tiles, one per (128-column tile, 32-channel slab, tap) in K-loop order, each [hi 128x64 B][lo 128x64 B]. */
#define XV_FMT_F32 0
#define XV_FMT_SPLIT 1
#define XV_SPLIT_PAD_BEFORE 8
#define XV_SPLIT_PAD_AFTER 264
size_t xv_packed_weights_bf16x3_bytes(int K, int cin, int cout);
int xv_pack_weights_bf16x3(const float *w, int K, int cin, int cout, void *wt, void *stream);
/* The tiles of n layers in ONE launch, each in one or both orientations (the training step re-packs every weight after every
 * optimizer step): wt_fwd[i] = xv_pack_weights_bf16x3 of w[i][K, cin, cout] with cin padded by zero rows to cin_pad[i]
 * (xv_packed_weights_bf16x3_bytes(K, cin_pad, cout) bytes); wt_bwd[i] = the operand of the input-gradient GEMM,
 * w'[k, o, c] = w[K-1-k, c, o] as [K, cout, cin_pad] (xv_packed_weights_bf16x3_bytes(K, cout, cin_pad) bytes) -- what
 * tf.gradients builds for conv1d / xw_plus_b (local/tf/models.py:112).  Either destination of a layer may be NULL. */
int xv_pack_weights_bf16x3_many(int n, const float *const *w, const int32_t *K, const int32_t *cin, const int32_t *cin_pad,
                                const int32_t *cout, void *const *wt_fwd, void *const *wt_bwd, void *stream);
size_t xv_split_row_bytes(int channels);
int xv_split_encode_f32(const float *x, int64_t R, int c, int ldx, void *xs, void *stream);
int xv_split_decode_f32(const void *xs, int64_t R, int c, float *x, int ldx, void *stream);
/* Same semantics as xv_tdnn_layer_f32; x / y in the given formats (ldx / ldy used for XV_FMT_F32 only); y may be
 * NULL when only y_preact (always fp32 rows, stride ldpre) is wanted. */
int xv_tdnn_layer_bf16x3(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                         const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation,
                         int cout, const uint8_t *row_valid, void *y, int y_format, int ldy, float *y_preact, int ldpre,
                         void *stream);
/* The same layer with fp32 rows out, and the column sums of that output for free: the epilogue also leaves, per 128-row tile,
 * [sum_rows y | sum_rows y * sum_r] in double in `workspace` (xv_col_sums_workspace_bytes(R, cout) bytes; merged by
 * xv_col_sums_merge_f32 / xv_bn_act_backward_parts_f32).  The training step calls it as the input-gradient GEMM of a layer
 * (tf.gradients of conv1d, local/tf/models.py:112): y = dL/dh of the layer below, sum_r = that layer's activation output,
 * and the two sums are what its BN backward starts from -- no separate pass over y.  cout % 8 == 0. */
int xv_tdnn_layer_bf16x3_sums(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                              const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K,
                              int dilation, int cout, const uint8_t *row_valid, float *y, int ldy, const float *sum_r,
                              int ld_sum_r, void *workspace, void *stream);
/* xv_tdnn_layer_bf16x3 (fp32 rows out, optional y_preact) whose epilogue also leaves, per 128-row tile, [sum_rows y | sum_rows y^2]
 * in double in `workspace` (xv_col_sums_workspace_bytes(R, cout) bytes): the batch moments tf.layers.batch_normalization(training=
 * True) takes of the layer's activation output (local/tf/models.py:66-68) without a pass over it -- xv_bn_moments_fold_f32 turns
 * them into mean / var / the folded affine.  cout % 8 == 0. */
int xv_tdnn_layer_bf16x3_moments(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                                 const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K,
                                 int dilation, int cout, const uint8_t *row_valid, float *y, int ldy, float *y_preact, int ldpre,
                                 void *workspace, void *stream);
/* Last frame-level layer fused with the first half of statistics pooling (models.py:66-76 / 482-486 in one pass):
 * the same GEMM as xv_tdnn_layer_bf16x3, but instead of storing y[R, Cout] the epilogue reduces every block of 8
 * consecutive rows (global rows 8i..8i+7, valid rows only) to per-channel (mean, M2 = sum (v-mean)^2) and writes
 *     block_stats[ceil(R/8)][2][Cout]  fp32   (xv_block_stats_bytes(R, Cout) bytes, 16-byte aligned)
 * -- a quarter of the bytes of y, and y is never re-read.  Every chunk must START ON A ROW THAT IS A MULTIPLE OF 8 (gap
 * rows pad up to it), so that a block never mixes two chunks and the result does not depend on batch composition.
 * xv_stats_pool_blocks_f32 merges the blocks of each chunk in order (fp64) into out[B, 2*Cout] = [mean | sqrt(var+eps)],
 * the same quantity as xv_stats_pool_f32; a chunk whose row_start is not a multiple of 8, or whose row_len is <= 0, yields NaN. */
size_t xv_block_stats_bytes(int64_t R, int cout);
int xv_tdnn_layer_pool_bf16x3(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                              const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K,
                              int dilation, int cout, const uint8_t *row_valid, float *block_stats, void *stream);
int xv_stats_pool_blocks_f32(const float *block_stats, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                             float eps, float *out, void *stream);
/* The same fused last layer in the exact-fp32 arithmetic (xv_tdnn_layer_f32's GEMM with the block-statistics epilogue: the
 * 4 * Cout bytes per frame of y are neither written nor re-read).  x / wp as for xv_tdnn_layer_f32; needs Cout % 4 == 0 and
 * 16-byte aligned bias / bn_scale / bn_shift / per-channel act_alpha. */
int xv_tdnn_layer_pool_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias, const float *bn_scale,
                           const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                           const uint8_t *row_valid, float *block_stats, void *stream);

/* The FIRST frame-level layer (frame_level_info_layer-0: conv1d over the MFCC rows, models.py:54-67) as a kernel built around
 * its output stream: the im2col operand of a wave's 16 frames is formed in registers straight from the fp32 feature rows, the
 * weights of 128 output channels stay in LDS for a strip of 512 frames, and the epilogue writes XV_FMT_SPLIT rows directly from
 * the accumulators.  Same contraction and epilogue as xv_tdnn_layer_bf16x3 with x in XV_FMT_F32 and y in XV_FMT_SPLIT.
 * x[R, ldx]: rows of ceil8(Cin) floats (columns >= Cin zero), ldx % 8 == 0, 32-byte aligned; wt = xv_pack_first_bf16x3(w[K,Cin,Cout]).
 * Supported: K odd, K*ceil8(Cin) <= 128, (K-1)*dilation <= 8, Cout % 32 == 0, Cout <= 512 (xv_packed_first_bf16x3_bytes
 * returns 0 otherwise; the general kernel takes those shapes). */
size_t xv_packed_first_bf16x3_bytes(int K, int cin, int cout);
int xv_pack_first_bf16x3(const float *w, int K, int cin, int cout, void *wt, void *stream);
int xv_tdnn_first_bf16x3(const float *x, int64_t R, int cin, int ldx, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, void *y, void *stream);

/* The last TWO frame-level layers and the first half of statistics pooling in one launch, for topologies whose last two
 * layers have no temporal context (kernel size 1: models.py:28 [5,5,7,1,1], :545 [5,3,3,1,1]):
 *     h = bn1(act(x . w1 + b1))          frame_level_info_layer-(n-2)   models.py:54-67
 *     y = bn2(act(h . w2 + b2))          frame_level_info_layer-(n-1)
 *     block_stats = per-8-row (mean, M2) of y, as xv_tdnn_layer_pool_bf16x3 writes them (merge: xv_stats_pool_blocks_f32)
 * h never exists in memory: a wave keeps its 16 frames x Cmid of h in registers, produced by the first GEMM directly in
 * the operand layout of the second (v_mfma_f32_16x16x32_bf16, bf16x3 arithmetic).  x: XV_FMT_SPLIT rows (same padding
 * contract as xv_tdnn_layer_bf16x3).  wt = xv_pack_pair_bf16x3(w1[Cin,Cmid], w2[Cmid,Cout]) (TF's [in, out] order;
 * xv_packed_pair_bf16x3_bytes bytes, 0 = unsupported shape).  Supported: Cmid == 512, Cin % 32 == 0, Cout % 64 == 0,
 * Cout <= 2048 (else XV_ERR_UNSUPPORTED: run the two layers separately).  Chunks must start on rows that are multiples of
 * 8, as for xv_tdnn_layer_pool_bf16x3.  act_alpha1 / act_alpha2: [1] for LRELU, [Cmid] / [Cout] for PRELU. */
size_t xv_packed_pair_bf16x3_bytes(int cin, int cmid, int cout);
int xv_pack_pair_bf16x3(const float *w1, const float *w2, int cin, int cmid, int cout, void *wt, void *stream);
int xv_tdnn_pair_pool_bf16x3(const void *x, int64_t R, int cin, int cmid, int cout, const void *wt, const float *bias1,
                             const float *bn_scale1, const float *bn_shift1, const float *act_alpha1, const float *bias2,
                             const float *bn_scale2, const float *bn_shift2, const float *act_alpha2, int act_kind,
                             const uint8_t *row_valid, float *block_stats, void *stream);

/* ---- f16bf8 split-precision twins of the hidden frame-level layers --------------------------------------------------
 *
 * The same layer (models.py:54-76) with every product formed as
 *     x*w = xh*wh + 2^-11 (xl8*wh8 + xh8*wl8)      xh = fp16(x), xl8 = bf8(2^11 (x - xh)), xh8 = bf8(x)   (bf8 = e5m2)
 * i.e. one v_mfma_f32_32x32x16_f16 and one block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (K = 64 holds both cross terms
 * of a 32-channel slab; the 2^-11 is its E8M0 scale operand) per three bf16 MFMAs of the bf16x3 arithmetic; fp32
 * accumulation, fp32 epilogue.  Accuracy on the full network: 1.1e-5 relative L2 against fp64 (bf16x3: 5e-6).
 *   XV_FMT_SPLIT8  the XV_FMT_SPLIT geometry (128 bytes per row and 32-channel slab, same padding contract, same
 *                  xv_split_row_bytes, physical slot = logical slot ^ ((r>>1)&7)) with logical slot g (0..3) = fp16 hi of
 *                  channels 8g..8g+7 and slot 4+g = [8 x xl8 | 8 x xh8] of the same channels.
 * Range: values are clamped to +-57344 (largest finite e5m2; fp16 ends at 65504) when a layer WRITES this format; every
 * writer takes `status` (device int32, may be NULL) and ORs bit 0 into it when it had to clamp -- the caller then repeats
 * the batch in the bf16x3 arithmetic (fp32 range).  Activations of a BN-normalised network are O(1..100).
 * Weights: xv_pack_weights_f16bf8 -> xv_packed_weights_f16bf8_bytes(K,Cin,Cout) bytes of 16 KB tiles in the order of
 *   xv_pack_weights_bf16x3, each [fp16 plane 128x64 B][8-bit plane 128x64 B, slot g = 8 x wh8 | 8 x wl8]; |w| > 57344 clamps.
 * xv_tdnn_layer_f16bf8: x in XV_FMT_SPLIT8; y in XV_FMT_F32 (row stride ldy), XV_FMT_SPLIT (to feed a bf16x3 consumer such
 *   as xv_tdnn_pair_pool_bf16x3) or XV_FMT_SPLIT8; K in {1,3,5,7}, 2 <= (K-1)*dilation <= 8 for K > 1.
 * xv_tdnn_layer_pool_f16bf8: the xv_tdnn_layer_pool_bf16x3 contract (block statistics instead of y).
 * tap_bias (both; NULL = none; K > 1, Cout % 8 == 0, 16-byte aligned -- else XV_ERR_UNSUPPORTED): a per-row bias.  When the
 *   producer of x stored scale * act(z + b) without its BN shift (so that a ReLU's zeros stay zero bits in x), the shift's share
 *   of this layer is the constant tap_bias[t][o] (xv_fold_shift_taps_f32) for every tap t that falls on a frame, and nothing
 *   for a tap that falls on a gap row (row_valid == 0) or outside [0, R), where SAME padding reads zeros:
 *     z[r,o] = bias[o] - sum_{t missing at r} tap_bias[t][o] + sum_t sum_c x[r + (t-(K-1)/2)*dilation, c] * w[t,c,o]
 *   with bias = the layer's own bias + sum_t tap_bias[t] (bias_full of xv_fold_shift_taps_f32).
 * xv_tdnn_first_f16bf8: xv_tdnn_first_bf16x3 (bf16x3 arithmetic on the fp32 feature rows, same packed weights) writing
 *   XV_FMT_SPLIT8 rows.  xv_split8_encode_f32 / xv_split8_decode_f32: tooling and tests (decode returns hi + xl8 / 2^11). */
#define XV_FMT_SPLIT8 2
size_t xv_packed_weights_f16bf8_bytes(int K, int cin, int cout);
int xv_pack_weights_f16bf8(const float *w, int K, int cin, int cout, void *wt, void *stream);
int xv_split8_encode_f32(const float *x, int64_t R, int c, int ldx, void *xs, int32_t *status, void *stream);
int xv_split8_decode_f32(const void *xs, int64_t R, int c, float *x, int ldx, void *stream);
int xv_tdnn_layer_f16bf8(const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, const float *tap_bias, void *y, int y_format, int ldy, int32_t *status,
                         void *stream);
int xv_tdnn_layer_pool_f16bf8(const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                              const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                              const uint8_t *row_valid, const float *tap_bias, float *block_stats, void *stream);
int xv_tdnn_first_f16bf8(const float *x, int64_t R, int cin, int ldx, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, void *y, int32_t *status, void *stream);

/* xv_tdnn_pair_pool_bf16x3 in the f16bf8 arithmetic: x in XV_FMT_SPLIT8, wt = xv_pack_pair_f16bf8(w1, w2)
 * (xv_packed_pair_f16bf8_bytes bytes, 0 = unsupported: Cmid == 512, Cin % 32 == 0, Cout % 64 == 0, Cout <= 4096), same
 * block_stats contract.  A pair of waves shares 32 frames: each wave keeps HALF of the intermediate's channels in registers
 * (so it streams half of both layers' weights through its fragment reads) and the two partial sums of the second GEMM meet in
 * LDS.  `status` (may be NULL): bit 0 is ORed in when the intermediate activation had to be clamped to +-57344. */
size_t xv_packed_pair_f16bf8_bytes(int cin, int cmid, int cout);
int xv_pack_pair_f16bf8(const float *w1, const float *w2, int cin, int cmid, int cout, void *wt, void *stream);
int xv_tdnn_pair_pool_f16bf8(const void *x, int64_t R, int cin, int cmid, int cout, const void *wt, const float *bias1,
                             const float *bn_scale1, const float *bn_shift1, const float *act_alpha1, const float *bias2,
                             const float *bn_scale2, const float *bn_shift2, const float *act_alpha2, int act_kind,
                             const uint8_t *row_valid, float *block_stats, int32_t *status, void *stream);

/* xv_tdnn_pair_pool_f16bf8 with the cross terms of the SECOND layer in block-scaled e2m3 (6-bit elements, one power-of-two scale
 * per 16 channels of a frame / of a weight column: csrc/xv_split6.h) at half the matrix cycles of the bf8 form.  Same x, same
 * arguments, same status semantics, same supported shapes; wt = xv_pack_pair_f16mx6(w1, w2) (xv_packed_pair_f16mx6_bytes bytes;
 * the first layer's stages are byte for byte those of xv_pack_pair_f16bf8). */
size_t xv_packed_pair_f16mx6_bytes(int cin, int cmid, int cout);
int xv_pack_pair_f16mx6(const float *w1, const float *w2, int cin, int cmid, int cout, void *wt, void *stream);
int xv_tdnn_pair_pool_f16mx6(const void *x, int64_t R, int cin, int cmid, int cout, const void *wt, const float *bias1,
                             const float *bn_scale1, const float *bn_shift1, const float *act_alpha1, const float *bias2,
                             const float *bn_scale2, const float *bn_shift2, const float *act_alpha2, int act_kind,
                             const uint8_t *row_valid, float *block_stats, int32_t *status, void *stream);

/* A hidden layer with its cross terms in block-scaled e2m3 (csrc/xv_split6.h), fed by another layer's epilogue.
 *   XV_FMT_SPLIT6  the XV_FMT_SPLIT8 geometry (128 bytes per row and 32-channel slab, same row stride, padding contract and
 *                  slot swizzle).  Logical slots 0-3: fp16 hi, bit for bit XV_FMT_SPLIT8's.  Slots 4-7: two e2m3 blocks, block c =
 *                  channels 16c..16c+15 of the slab, 32 six-bit elements [2^11 lo | clamp(v)] under one power-of-two scale:
 *                  slot 4+c = dwords 0-3 of block c, slot 6+c = [dword 4 | dword 5 | E8M0 byte - 11, zero-extended | 0] (the 2^-11
 *                  of the cross terms rides in the byte).  All-zero bytes are a row of zeros.  Clamp and `status` as XV_FMT_SPLIT8.
 * Writers: xv_tdnn_layer_f16bf8 / xv_tdnn_layer_f16mx6 with y_format = XV_FMT_SPLIT6 where they run the 16 x 16 MFMA form of the
 *   256 x 256 tile (an even number of slabs, K in {3,5,7}, Cout % 256 == 0; else XV_ERR_UNSUPPORTED), xv_tdnn_first_f16mx6, and
 *   xv_split6_encode_f32 (tooling and tests; xv_split6_decode_f32 returns hi + lo_q / 2^11 and, where cq is not NULL, the
 *   dequantised second operand c_q, both with row stride ldx).  Every writer stores the rows xv_split6_encode_f32 stores for the
 *   same fp32 values, bit for bit.
 * xv_tdnn_first_f16mx6: xv_tdnn_first_f16bf8 (same arguments, packed weights, shapes -- else XV_ERR_UNSUPPORTED -- and `status`)
 *   writing XV_FMT_SPLIT6 rows: the producer of a layer 1 that runs xv_tdnn_layer_f16mx6.
 * xv_tdnn_layer_f16mx6: xv_tdnn_layer_f16bf8's arguments and semantics with x in XV_FMT_SPLIT6 and wt = xv_pack_weights_f16mx6
 *   (the 16 KB tiles and fp16 planes of xv_pack_weights_f16bf8; the 8-bit plane holds the blocks [clamp(w) | 2^11 lo] of each
 *   column's channels 16c..16c+15 at the same positions, byte unshifted).  The 16 x 16 MFMA form of the 256 x 256 tile only: an
 *   even number of 32-channel slabs, K in {3,5,7}, Cout % 256 == 0, y not XV_FMT_F32 -- else XV_ERR_UNSUPPORTED. */
#define XV_FMT_SPLIT6 3
size_t xv_packed_weights_f16mx6_bytes(int K, int cin, int cout);
int xv_pack_weights_f16mx6(const float *w, int K, int cin, int cout, void *wt, void *stream);
int xv_split6_encode_f32(const float *x, int64_t R, int c, int ldx, void *xs, int32_t *status, void *stream);
int xv_split6_decode_f32(const void *xs, int64_t R, int c, float *x, float *cq, int ldx, void *stream);
int xv_tdnn_layer_f16mx6(const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, const float *tap_bias, void *y, int y_format, int ldy, int32_t *status,
                         void *stream);
int xv_tdnn_first_f16mx6(const float *x, int64_t R, int cin, int ldx, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, void *y, int32_t *status, void *stream);

/* xv_fc_f32 twin: fp32 rows in, fp32 rows out; wt = xv_pack_weights_bf16x3(w, 1, In, Out). */
int xv_fc_bf16x3(const float *x, int nrows, int in_dim, const void *wt, const float *bias, const float *bn_scale,
                 const float *bn_shift, int act_kind, const float *act_alpha, int out_dim, float *y, float *y_preact, void *stream);

/* Statistics pooling.  Replaces tf.nn.moments(h, 1) + tf.sqrt(var + 1e-5) + tf.concat
 * (local/tf/models.py:16,75-76):  out[b] = [ mean_t h[t,:]  ||  sqrt(mean_t (h-mean)^2 + eps) ]
 * over the rows of chunk b.  h[R,C] row stride ldh, C % 4 == 0; out[B, 2C].
 * Chunks longer than `split_rows` rows are reduced by several workgroups; `workspace` must then hold
 * xv_stats_pool_workspace_bytes(C, B, max_len, split_rows) bytes (may be NULL when that is 0).
 * ldh must be a multiple of 4 and >= C (XV_ERR_BAD_ARG otherwise; the same holds for xv_chunk_moments_f32 and
 * xv_attention_pool_f32).  A chunk with row_len <= 0 has no statistics: its row of out is NaN, in the direct and in the split path
 * (as xv_stats_pool_blocks_f32 writes it); its row_start is not read and the other chunks are not affected. */
size_t xv_stats_pool_workspace_bytes(int c, int nchunks, int max_len, int split_rows);
int xv_stats_pool_f32(const float *h, int64_t ldh, int c, const int32_t *row_start, const int32_t *row_len,
                      int nchunks, int max_len, int split_rows, float eps, float *out, void *workspace,
                      void *stream);

/* Segment-level affine.  Replaces tf.nn.xw_plus_b (local/tf/models.py:86) and, for the path to
 * embed_layer-1, the relu + batch_norm between the two (local/tf/models.py:88-89):
 *     z = x[B,In] . w + bias ;  y_preact <- z (the x-vector when this is embed_layer-0) ;
 *     y <- act(z)*bn_scale + bn_shift   (skipped when y == NULL)
 *   wp = xv_pack_weights_f32(w[In,Out]) i.e. [Out][In]. */
int xv_fc_f32(const float *x, int nrows, int in_dim, const float *wp, const float *bias, const float *bn_scale,
              const float *bn_shift, int act_kind, const float *act_alpha, int out_dim, float *y,
              float *y_preact, void *stream);

/* xv_fc_f32 for a SKINNY problem (a training minibatch's segment level: 64 rows x 3072 -> 512): with <= 128 rows there are only a few
 * output tiles, and each would walk all In / 32 slabs one after the other.  The slabs are dealt to groups of workgroups that write
 * raw partial sums to `workspace` (xv_fc_splitk_workspace_bytes bytes; 0 = the shape is not skinny and the call IS xv_fc_f32), a
 * second kernel adds the groups in order (deterministic) and applies bias / activation / BN.  Same arguments as xv_fc_f32. */
size_t xv_fc_splitk_workspace_bytes(int nrows, int in_dim, int out_dim);
int xv_fc_splitk_f32(const float *x, int nrows, int in_dim, const float *wp, const float *bias, const float *bn_scale,
                     const float *bn_shift, int act_kind, const float *act_alpha, int out_dim, float *y, float *y_preact, void *workspace,
                     void *stream);

/* Length-weighted average of chunk embeddings.  Replaces the NumPy lines local/tf/models.py:398,
 * 418-421 with the same float32 operation order (product, sum in chunk order, one division):
 *   out[u] = ( sum_{i in [seg_start[u], seg_start[u+1])} float(chunk_len[i]) * e[i] ) / float(sum len). */
int xv_chunk_average_f32(const float *e, const int32_t *seg_start, const int32_t *chunk_len, int nutts, int dim,
                         float *out, void *stream);

/* ---- training step (reference Model.train_one_iteration, local/tf/models.py:216-305) ----------
 * The forward GEMMs and the input-gradient GEMMs are xv_tdnn_layer_f32 / xv_fc_f32 (dgrad = the same kernel with the
 * taps flipped and Cin/Cout swapped in the weights); the entry points below add the rest.  fp32 storage, reductions
 * accumulate in fp64.  Workspaces are caller-provided device buffers. */

/* Per-chunk (mean, BIASED variance) over the rows of each chunk: out[B, 2C] = [mean || var].  Same kernel and arguments
 * as xv_stats_pool_f32 (ldh >= C, NaN for an empty chunk) without the sqrt(var+eps).  With xv_merge_moments_f32 this is tf.nn.moments over all frames of
 * the minibatch (local/tf/tf_block.py:19). */
int xv_chunk_moments_f32(const float *h, int64_t ldh, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                         int max_len, int split_rows, float *out, void *workspace, void *stream);
int xv_merge_moments_f32(const float *chunk_mean_var, const int32_t *row_len, int nchunks, int c, float *mean, float *var,
                         void *stream);
/* y[r,:] = row_valid[r] ? x[r,:]*scale + shift : 0   (batch-norm with batch statistics folded by xv_fold_bn_f32).  x / y may be
 * column slices of wider buffers: ldx >= c and ldy >= c, else XV_ERR_BAD_ARG. */
int xv_rows_affine_f32(const float *x, int ldx, int64_t R, int c, const float *scale, const float *shift,
                       const uint8_t *row_valid, float *y, int ldy, void *stream);
/* The same with a second copy of y in the bf16 split activation format (XV_FMT_SPLIT; y_split = row 0 of a buffer with the format's
 * padding rows, c % 32 == 0; NULL = xv_rows_affine_f32): the training step's K = 1 layers then take the DMA-fed GEMM. */
int xv_rows_affine_split_f32(const float *x, int ldx, int64_t R, int c, const float *scale, const float *shift,
                             const uint8_t *row_valid, float *y, int ldy, void *y_split, void *stream);
/* Weight gradient of a TDNN/FC layer: dw[k,ci,co] = sum_r x[r + (k-(K-1)/2)*dilation, ci] * dz[r, co]  (TF layout
 * [K,Cin,Cout]; rows outside [0,R) read as zero; gap rows of x and dz are zero by contract).  x / dz may be column slices of wider
 * buffers (ldx >= cin, lddz >= cout, else XV_ERR_BAD_ARG); K odd. */
size_t xv_wgrad_workspace_bytes(int64_t R, int cin, int cout, int K);
int xv_wgrad_f32(const float *x, int ldx, const float *dz, int lddz, int64_t R, int cin, int cout, int K, int dilation,
                 float *dw, void *workspace, void *stream);
/* The same gradient in the bf16x3 arithmetic of xv_tdnn_layer_bf16x3 (operands split hi + lo while they are staged, three bf16
 * MFMAs per product, fp32 accumulate; ~5e-6 relative): what `--train-precision bf16x3` runs.  Same arguments, same workspace,
 * same deterministic split merge; falls back to xv_wgrad_f32 when R * ld * 4 >= 2^31 (32-bit buffer offsets). */
int xv_wgrad_bf16x3(const float *x, int ldx, const float *dz, int lddz, int64_t R, int cin, int cout, int K, int dilation,
                    float *dw, void *workspace, void *stream);
/* xv_wgrad_bf16x3 that also leaves db[co] = sum_r dz[r, co], the bias gradient of the same layer (models.py:61 under minimize()): the
 * workgroups of tap 0 / input tile 0 sum the dz rows they stream anyway (fp32 inside a 16-row step, double across steps and row
 * splits, merged in split order: deterministic) -- no separate pass over dz (xv_col_sums_f32).  workspace: xv_wgrad_bias_workspace_bytes
 * (always required).  No fp32 fallback: XV_ERR_UNSUPPORTED when R * ld * 4 >= 2^31. */
size_t xv_wgrad_bias_workspace_bytes(int64_t R, int cin, int cout, int K);
int xv_wgrad_bias_bf16x3(const float *x, int ldx, const float *dz, int lddz, int64_t R, int cin, int cout, int K, int dilation,
                         float *dw, float *db, void *workspace, void *stream);
/* sum_a[c] = sum_r a[r,c];  sum_ab[c] = sum_r a[r,c]*b[r,c]  (b, sum_ab may be NULL).  lda >= c, and ldb >= c when b is given, else
 * XV_ERR_BAD_ARG.  Rows are read 16 bytes at a time only when lda, ldb are multiples of 4 and a, b are 16-byte aligned; any 4-byte
 * aligned pointer and any ld >= c are accepted. */
size_t xv_col_sums_workspace_bytes(int64_t R, int c);
int xv_col_sums_f32(const float *a, int lda, const float *b, int ldb, int64_t R, int c, float *sum_a, float *sum_ab,
                    void *workspace, void *stream);
/* Batch-norm backward through the activation (closed form): given dh = dL/d(BN output), r = activation output, the
 * batch statistics and sum_dh = sum_r dh, sum_dh_r = sum_r dh*r, writes dgamma, dbeta and dz = dL/d(pre-activation)
 * (gap rows zero).  coef_ws: 3*c floats.  act_kind: NONE / RELU / LRELU(act_alpha).  dh, r and dz share the row stride ld >= c (else
 * XV_ERR_BAD_ARG; the same for the _split and _parts forms below). */
int xv_bn_act_backward_f32(const float *dh, const float *r, int ld, int64_t R, int c, const float *sum_dh,
                           const float *sum_dh_r, const float *mean, const float *var, const float *gamma, float eps,
                           float n_frames, int act_kind, float act_alpha, const uint8_t *row_valid, float *dgamma,
                           float *dbeta, float *coef_ws, float *dz, void *stream);
/* The same with a second copy of dz in the bf16 split activation format (dz_split as y_split above; NULL = the plain form). */
int xv_bn_act_backward_split_f32(const float *dh, const float *r, int ld, int64_t R, int c, const float *sum_dh,
                                 const float *sum_dh_r, const float *mean, const float *var, const float *gamma, float eps,
                                 float n_frames, int act_kind, float act_alpha, const uint8_t *row_valid, float *dgamma,
                                 float *dbeta, float *coef_ws, float *dz, void *dz_split, void *stream);
/* The same from the PARTIAL column sums a producer left in `sums_workspace` (xv_col_sums_workspace_bytes(R, c) bytes: per 128 rows
 * [sum dh | sum dh*r] in double -- written by xv_tdnn_layer_bf16x3_sums, the input-gradient GEMM that produced dh): merge and
 * coefficients in one launch, no pass over dh for the sums.  tf.gradients of tf.layers.batch_normalization(training=True),
 * local/tf/models.py:66-68,109-113. */
int xv_bn_act_backward_parts_f32(const float *dh, const float *r, int ld, int64_t R, int c, const void *sums_workspace,
                                 const float *mean, const float *var, const float *gamma, float eps, float n_frames,
                                 int act_kind, float act_alpha, const uint8_t *row_valid, float *dgamma, float *dbeta,
                                 float *coef_ws, float *dz, void *dz_split, void *stream);
/* Batch moments + BN fold from the partial sums of xv_tdnn_layer_bf16x3_moments, one launch: mean = S1 / n_frames,
 * var = S2 / n_frames - mean^2 (biased: tf.nn.moments), scale = gamma / sqrt(var + eps), shift = beta - mean * scale (the
 * operations of xv_fold_bn_f32).  Replaces xv_chunk_moments_f32 + xv_merge_moments_f32 + xv_fold_bn_f32 of a training forward. */
int xv_bn_moments_fold_f32(const void *sums_workspace, int64_t R, int c, float n_frames, const float *gamma, const float *beta,
                           float eps, float *mean, float *var, float *scale, float *shift, void *stream);
/* Merge of such partial sums alone: sum_a[c], sum_ab[c] (sum_ab may be NULL) -- what xv_col_sums_f32 returns for the same rows. */
int xv_col_sums_merge_f32(const void *sums_workspace, int64_t R, int c, float *sum_a, float *sum_ab, void *stream);
/* Backward of [statistics pooling -> BN -> activation] of the LAST frame-level layer in two launches: the gradient that reaches
 * h = BN(r) comes from the pooling alone (local/tf/models.py:75-76), so the BN backward's column sums follow from per-chunk numbers
 * (pooled = [mu | sig], dpooled, chunk_moments = xv_chunk_moments_f32 of r: [mean | biased var] per chunk) and dh is formed on the
 * fly, never stored.  Writes dgamma, dbeta, dz (gap rows and rows outside every chunk zero) and optionally dz in the split format.
 * ld >= c, else XV_ERR_BAD_ARG; at most 65535 chunks.  Every chunk is required to have row_len >= 1.  A chunk with row_len <= 0 is
 * tolerated as follows: it adds nothing to dgamma, dbeta and the coefficients (its pooled row, NaN from xv_stats_pool_f32, is not
 * read for them), it owns no frame, and the rows from its row_start up to the next chunk's are zeroed like gap rows. */
int xv_pool_bn_act_backward_f32(const float *h, const float *r, int ld, int c, const int32_t *row_start, const int32_t *row_len,
                                int nchunks, int64_t R, const float *pooled, const float *dpooled, const float *chunk_moments,
                                const float *mean, const float *var, const float *gamma, float eps, float n_frames,
                                int act_kind, float act_alpha, float *dgamma, float *dbeta, float *coef_ws, float *dz,
                                void *dz_split, void *stream);
/* tf.layers.batch_normalization(training=True) of a SMALL matrix (1 .. 1024 rows, every row a sample: the segment-level layers of
 * a training step, local/tf/models.py:88-91) in one launch each way.  Forward: batch mean / biased variance into mean, var, and
 * y = x * scale + shift with the fold of xv_fold_bn_f32 (what xv_chunk_moments_f32 + xv_merge_moments_f32 + xv_fold_bn_f32 +
 * xv_rows_affine_f32 do in four).  Backward: dgamma, dbeta and dz through the activation (NONE / RELU / LRELU), as xv_col_sums_f32
 * + xv_bn_act_backward_f32. */
int xv_bn_small_forward_f32(const float *x, int ldx, int nrows, int c, const float *gamma, const float *beta, float eps, float *mean,
                            float *var, float *y, int ldy, void *stream);
int xv_bn_small_backward_f32(const float *dh, const float *r, int ld, int nrows, int c, const float *mean, const float *var,
                             const float *gamma, float eps, int act_kind, float act_alpha, float *dgamma, float *dbeta, float *dz,
                             void *stream);
/* Gradient of statistics pooling: dh[t,c] = dmu[c]/T + dsig[c]*(h[t,c]-mu[c])/(T*sig[c]); dh gap rows are zeroed (all R * ldh floats of
 * dh are written).  ldh >= c and R > 0, else XV_ERR_BAD_ARG.  Every chunk is required to have row_len >= 1; a chunk with
 * row_len <= 0 writes nothing (its rows stay zero). */
int xv_pool_backward_f32(const float *h, int ldh, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                         int64_t R, const float *pooled, const float *dpooled, float *dh, void *stream);
/* tf.nn.softmax_cross_entropy_with_logits + reduce_mean + accuracy (local/tf/models.py:106-117):
 * loss_acc[0] = mean loss, loss_acc[1] = accuracy; dlogits (may be NULL) = (softmax - onehot)/nrows.  row_ws: 2*nrows. */
int xv_softmax_ce_f32(const float *logits, const int32_t *labels, int nrows, int nclasses, float *loss_acc, float *row_ws,
                      float *dlogits, void *stream);
/* tf.train.AdamOptimizer dense update with lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) computed by the caller. */
int xv_adam_f32(float *param, const float *grad, float *m, float *v, int64_t n, float lr_t, float beta1, float beta2, float eps,
                void *stream);
/* y += a*x and out[0] = sum x^2: the L2 penalty of the ModelL2Loss* classes, beta*(0.1|1)*tf.nn.l2_loss(w)
 * (local/tf/models.py:811-842): gradient g += beta*coef*w, loss += beta*coef*sumsq/2.  xv_sumsq_f32 reduces in two
 * stages (fp64 partials in `workspace`, xv_sumsq_workspace_bytes(n) bytes, 8-byte aligned, added in a fixed order). */
int xv_axpy_f32(float *y, const float *x, float a, int64_t n, void *stream);
size_t xv_sumsq_workspace_bytes(int64_t n);
int xv_sumsq_f32(const float *x, int64_t n, float *out, void *workspace, void *stream);
/* tf.nn.dropout(x, keep_prob) in place on x[R, C] (models.py:70-72, 92-94): element (r, c) is kept (and scaled by
 * 1/keep_prob) iff the top 32 bits of splitmix64(seed ^ 0x9E3779B97F4A7C15*(r*C + c + 1)) < keep_prob*2^32, else zeroed.
 * Stateless: the same call on the gradient buffer is the backward pass.  keep_prob == 1 is a no-op. */
int xv_dropout_f32(float *x, int ldx, int64_t R, int c, uint64_t seed, float keep_prob, void *stream);
/* Index arrays of a training minibatch in the packed-rows layout (B chunks of T frames, `gap` zero rows in front of, between and
 * behind them; rows >= gap + B (T + gap)): row_start[B], row_len[B], row_valid[rows] -- generated on the device (a host copy of
 * them is a host synchronisation, and a run meets a new length in most of its first few hundred steps). */
int xv_minibatch_layout(int B, int T, int gap, int64_t rows, int32_t *row_start, int32_t *row_len, uint8_t *row_valid, void *stream);
/* A training minibatch src[B, T, F] (float16 when src_is_f16, else float32; DEVICE pointer like everything else) -> the packed
 * rows-with-gaps matrix dst[rows, in_dim] of the header comment: chunk b at rows gap + b*(T+gap), all other rows and the columns
 * F..in_dim-1 zero; rows >= gap + B*(T+gap).  Replaces the feed_dict hand-over of models.py:255-262 (the egs hold float16). */
int xv_pack_minibatch_f32(const void *src, int src_is_f16, int B, int T, int F, int gap, int in_dim, float *dst, int64_t rows,
                          void *stream);

/* PReLU backward (tf_block.py:38-47): on entry dr = dL/d(activation output), z = pre-activation; on exit
 * dr = dL/dz = dr * (z > 0 ? 1 : alpha[c]) and z = dr_in * min(z, 0), whose column sums (xv_col_sums_f32) are dL/dalpha. */
int xv_prelu_backward_f32(float *dr, float *z, int ld, int64_t R, int c, const float *alpha, void *stream);

/* moving = moving*decay + batch*(1-decay)   (local/tf/tf_block.py:20-21). */
int xv_ema_f32(float *moving, const float *batch, int n, float decay, void *stream);

/* ---- additive-margin softmax head (build-defined: BASELINE configs[4] asks for it, the reference has no margin head) ----
 * logits[b, j] = scale * (cos(x_b, w_j) - margin * [j == label_b]),  cos = <x/||x||, w_j/||w_j||>   (Wang et al. 2018).
 * xv_l2_normalize_rows_f32: y = x / max(||x||, 1e-12) per row, norm[r] = ||x_r||;  _backward: dx = (dy - y<y,dy>) / norm;
 * xv_am_margin_f32 applies margin and scale in place to the cosine matrix (which xv_fc_* computes from the normalised
 * operands); the loss is xv_softmax_ce_f32 on the result. */
int xv_l2_normalize_rows_f32(const float *x, int ldx, int nrows, int c, float *y, int ldy, float *norm, void *stream);
int xv_l2_normalize_backward_f32(const float *dy, const float *y, const float *norm, int nrows, int c, float *dx, void *stream);
int xv_am_margin_f32(float *cosines, const int32_t *labels, int nrows, int nclasses, float scale, float margin, void *stream);

/* ---- self-attentive statistics pooling (ModelL2LossWithoutDropoutLReluAttention, local/tf/models.py:1036-1052) -------
 * The last frame-level layer has 2*C channels, h = [h1 | h2].  With u = h1.W + b (one more K=1 xv_tdnn_layer_* call):
 *   xv_attention_scores_f32   scores[r] = sum_c v[c]*tanh(u[r,c])            (models.py:1045-1046; fp64 row sums);
 *                             nonlin (optional, [R, ldn]) receives tanh(u) for the training backward
 *   xv_attention_softmax_f32  att[rows of chunk b] = softmax(scores[rows of chunk b])   (models.py:1046)
 *   xv_attention_pool_f32     out[b] = [ m | sqrt(max(q,0) + eps) ],  m = sum_t att[t] h2[t,:],  q = sum_t att[t] h2[t,:]^2 - m^2
 *                             (models.py:1048-1050; products and sums in fp64).  Chunks longer than split_rows rows are
 *                             reduced by several workgroups through `workspace`
 *                             (xv_attention_pool_workspace_bytes bytes, 8-byte aligned; may be NULL when that is 0).
 * Gap rows of scores / att are never read or written.  A chunk with row_len <= 0: xv_attention_softmax_f32 writes nothing for it,
 * xv_attention_pool_f32 sets its row of out to NaN (direct and split path); ldh >= C as for xv_stats_pool_f32. */
int xv_attention_scores_f32(const float *u, int64_t ldu, int64_t R, int c, const float *v, float *scores, float *nonlin,
                            int64_t ldn, void *stream);
int xv_attention_softmax_f32(const float *scores, const int32_t *row_start, const int32_t *row_len, int nchunks, float *att,
                             void *stream);
size_t xv_attention_pool_workspace_bytes(int c, int nchunks, int max_len, int split_rows);
int xv_attention_pool_f32(const float *h, int64_t ldh, int c, const float *att, const int32_t *row_start, const int32_t *row_len,
                          int nchunks, int max_len, int split_rows, float eps, float *out, void *workspace, void *stream);
/* Backward of the three steps above (training step of the attention class):
 *   xv_attention_pool_backward_f32     dh[t,c] = att[t] (g1[c] + 2 h[t,c] g2[c]),  datt[t] = sum_c h[t,c] g1[c] + h[t,c]^2 g2[c]
 *                                      with g2 = dsd/(2 sd), g1 = dm - 2 m g2, [m | sd] = pooled, [dm | dsd] = dpooled
 *   xv_attention_softmax_backward_f32  dscores[t] = att[t] (datt[t] - sum_tau att[tau] datt[tau])   per chunk
 *   xv_attention_scores_backward_f32   du[r,c] = dscores[r] v[c] (1 - n[r,c]^2);  nonlin (= n = tanh(u)) is OVERWRITTEN with
 *                                      dscores[r] n[r,c], whose column sums are dv (xv_col_sums_f32); rows outside every
 *                                      chunk must carry dscores = 0. */
int xv_attention_pool_backward_f32(const float *h, int64_t ldh, int c, const float *att, const int32_t *row_start,
                                   const int32_t *row_len, int nchunks, int max_len, const float *pooled, const float *dpooled,
                                   float *dh, int64_t lddh, float *datt, void *stream);
int xv_attention_softmax_backward_f32(const float *att, const float *datt, const int32_t *row_start, const int32_t *row_len,
                                      int nchunks, float *dscores, void *stream);
int xv_attention_scores_backward_f32(float *nonlin, int64_t ldn, const float *dscores, const float *v, int64_t R, int c, float *du,
                                     int64_t lddu, void *stream);

/* ---- feature front-end -------------------------------------------------------------------------------
 * Sliding-window cepstral mean normalisation + VAD frame selection, i.e. what
 *   apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ... | select-voiced-frames ...
 * (local/tf/extract_xvectors.sh:68) do in front of extract_embedding.py, as one scatter kernel.
 *   x[sum T, F]  raw features of n_utts utterances back to back (utt_start[u], utt_len[u] in rows; max_len = max utt_len)
 *   dst_row[t]   per INPUT row: row of y that receives the normalised frame, or -1 to drop it (unvoiced / not in a chunk)
 *   y[., ldy]    destination (e.g. the packed batch buffer); only columns [0, F) of the addressed rows are written
 * Window rule and arithmetic (double-precision window sums) follow Kaldi's SlidingWindowCmn; min_window only matters
 * when center == 0 (Kaldi default 100). */
int xv_cmn_sliding_scatter_f32(const float *x, int ldx, int feat_dim, const int32_t *utt_start, const int32_t *utt_len,
                               int n_utts, int max_len, int cmn_window, int center, int min_window, const int32_t *dst_row,
                               float *y, int ldy, void *stream);

/* ---- PLDA / cosine scoring back-end ------------------------------------------------------------
 * What stage 9 of the recipe does with ivector-subtract-global-mean | transform-vec | ivector-normalize-length |
 * ivector-plda-scoring, for the part that scales with the data.  The PLDA log-likelihood ratio (Kaldi Plda::LogLikelihoodRatio)
 * is a dot product of length K = 2d plus a per-enrolment constant r:
 *   enrolment row [ (a/v) z , 1/v - 1/w ],  test row [ t , -t^2/2 ],  r = -1/2 sum a^2 z^2/v + 1/2 sum (log w - log v),
 *   a = n psi/(n psi + 1), v = 1 + psi/(n psi + 1), w = 1 + psi   (n = the enrolment vector's utterance count).
 * xv_backend_prepare_f32  operand rows out[N, ldo] (and r[N]) from raw vectors x[N, D] (ldx):
 *     y = lda (x - mean) + lda_offset        lda [dim, D] (ld_lda) exact-fp32 MFMA; NULL: y = x - mean (dim == D); mean NULL: 0;
 *                                            lda_offset NULL: 0
 *     length_norm: y *= sqrt(dim) / |y|      (ivector-normalize-length; a zero vector is left as it is)
 *     z = P (y - m), z *= sqrt(dim / sum_k z_k^2 / (psi_k + 1/n))    (Plda::TransformIvector; n = num_utts[row], NULL: 1);
 *                                            plda_transform [dim, dim] row-major, plda_mean [dim], plda_psi [dim]: all three
 *                                            or none (NULL: z = y)
 *     side XV_SIDE_PLAIN   out = z (K = dim)            XV_SIDE_ENROL  out = enrolment row (K = 2 dim), r written
 *          XV_SIDE_TEST    out = test row (K = 2 dim)   XV_SIDE_COSINE out = z / |z| (K = dim)
 *   Columns [K, ldo) are written with zeros: ldo is the operand width Kpad of the scorers, a multiple of XV_BACKEND_KSTEP.
 *   r (may be NULL) receives the row's constant: it is WRITTEN on every side, as exactly 0 on the sides that have none
 *   (PLAIN, TEST, COSINE).  ENROL / TEST need the PLDA.
 *   Arithmetic the tests rely on: both products (lda (x - mean) and P (y - m)) are fmaf chains per output element, k ascending
 *   from 0 with a zero start, one fp32 rounding of x - mean (y - m) in front and lda_offset added after the chain; without an
 *   lda, y = x - mean is that one subtraction.  A zero vector stays exactly zero through either length norm and the cosine
 *   packing (its scale is taken as 1: no NaN).  The output bits do not depend on ldx, ld_lda, ldo or the other rows.
 *   D <= 2048 and dim <= 256, else XV_ERR_UNSUPPORTED; ld_lda >= D, dim == D without an lda, ldo >= K and a multiple of
 *   XV_BACKEND_KSTEP, all three PLDA arrays or none, else XV_ERR_BAD_ARG.  A refused call launches nothing.
 * xv_score_matrix_f32  scores[e, t] (ld_scores) = sum_{k < kpad} E[e, k] T[t, k] + r[e]   (r NULL: + 0) for every
 *   e < n_enrol, t < n_test, on the exact-fp32 MFMA.  Fixed summation order: one fp32 accumulator per score, k ascending from 0,
 *   no split-K, r added after the dot product.  E, T: row stride ldk (a multiple of 4 floats, 16-byte aligned), kpad a multiple
 *   of XV_BACKEND_KSTEP, <= 1024 (else XV_ERR_UNSUPPORTED).
 * xv_score_pairs_f32  scores[i] = the same expression for the trial (e_idx[i], t_idx[i]), as an fmaf chain k ascending from 0:
 *   bit-identical to the cell of xv_score_matrix_f32, whatever the other trials of the list.
 * xv_score_blocks_f32  block-diagonal self-scoring of ragged groups of rows (diarization: every recording's sub-segments against
 *   each other).  E, T [n_rows, ldk] and r [n_rows] (may be NULL) as for xv_score_matrix_f32.  Device tables:
 *   grp_row0 [n_groups + 1] (int32 prefix sums: group g is rows [grp_row0[g], grp_row0[g + 1]), n_g >= 1 of them) and grp_score0
 *   [n_groups] (int64 element offsets into scores, multiples of 4).  Group g's n_g x n_g matrix lies at scores + grp_score0[g] with
 *   row stride ld_g = (n_g + 3) & ~3; its cell (i, j) = sum_k E[row0 + i, k] T[row0 + j, k] + r[row0 + i] holds the SAME BITS as the
 *   cell xv_score_matrix_f32 writes for those two rows (one tile body serves both).  Columns [n_g, ld_g) and everything between
 *   the blocks are not written.  max_n: an upper bound of every n_g (it sizes the grid: tiles x groups, workgroups past a group's
 *   own tiles exit); scores_elems: the elements of scores.  One launch per 65535 groups, no synchronisation.
 *   A group out of contract (n_g < 1, n_g > max_n, rows outside [0, n_rows), an offset that is negative or no multiple of 4, a
 *   block of n_g * ld_g elements past scores_elems) is skipped whole: nothing is read or written for it, and the device word
 *   *status receives 1.  The caller zeroes *status and reads it back with the results.
 *   XV_ERR_BAD_ARG, nothing launched: a NULL pointer (r excepted), n_groups, max_n, n_rows or scores_elems below 1, kpad / ldk /
 *   alignment as for xv_score_matrix_f32 (scores 16-byte aligned too), misaligned tables.  kpad > 1024: XV_ERR_UNSUPPORTED.
 * xv_topk_row_stats_f32  AS-norm cohort statistics: for each row i < n_rows of scores (row i = scores[i*ld .. i*ld + n_cols)),
 *   mean[i] and std[i] = the mean and the POPULATION standard deviation (divisor top_n) of the top_n largest values of the row,
 *   taken as a multiset (ties at the threshold are counted by multiplicity).  Exact selection: an MSB-first radix select on
 *   order-preserving uint32 keys, no approximation.  Every NaN, of either sign, ranks above +inf, so a row holding a NaN yields
 *   NaN statistics.  Sums in fp64 (the variance centred on the mean), rounded to fp32 once.  A row's bits depend on its values,
 *   n_cols and top_n only: not on the other rows, n_rows or ld.  Columns [n_cols, ld) are never read; nothing past n_rows is
 *   written.  Requires 1 <= top_n <= n_cols <= ld, ld a multiple of 4 and scores 16-byte aligned (else XV_ERR_BAD_ARG). */
#define XV_BACKEND_KSTEP 8
#define XV_SIDE_PLAIN 0
#define XV_SIDE_ENROL 1
#define XV_SIDE_TEST 2
#define XV_SIDE_COSINE 3
int xv_backend_prepare_f32(const float *x, int64_t ldx, int n_rows, int dim_in, const int32_t *num_utts, const float *mean,
                           const float *lda, int64_t ld_lda, const float *lda_offset, int dim, int length_norm,
                           const float *plda_transform, const float *plda_mean, const float *plda_psi, int side, float *out,
                           int64_t ldo, float *r, void *stream);
int xv_score_matrix_f32(const float *e, const float *t, int64_t ldk, int kpad, int n_enrol, int n_test, const float *r,
                        float *scores, int64_t ld_scores, void *stream);
int xv_score_blocks_f32(const float *e, const float *t, int64_t ldk, int kpad, int n_rows, const float *r, const int32_t *grp_row0,
                        const int64_t *grp_score0, int n_groups, int max_n, float *scores, int64_t scores_elems, int32_t *status,
                        void *stream);
int xv_score_pairs_f32(const float *e, const float *t, int64_t ldk, int kpad, const int32_t *e_idx, const int32_t *t_idx,
                       int64_t n_trials, const float *r, float *scores, void *stream);
int xv_topk_row_stats_f32(const float *scores, int64_t ld, int n_rows, int n_cols, int top_n, float *mean, float *std,
                          void *stream);

/* ---- moments for PLDA adaptation (ivector-adapt-plda, stage 10; csrc/xv_moments.hip) --------------------
 * xv_moment_stats_f64  sum[j] = sum_i x[i, j] and outer[j, k] = sum_i x[i, j] x[i, k] over the rows i < n_rows of x (row stride
 *   ldx) for j, k < dim, in fp64: the fp32 inputs are widened (exact), the products go through v_mfma_f64_16x16x4_f64 (a product
 *   of two fp32 values is exact in fp64) and every accumulation is fp64.
 *   Fixed order: rows are cut into slabs of XV_MOMENT_SLAB rows; each slab is accumulated with its rows ascending (four rows
 *   per MFMA) into a partial held in the workspace, and a second launch adds the partials in slab order.  No floating-point
 *   atomics.  The output bits depend on the values, n_rows and dim only: not on ldx, ld_outer, the stream or what ran before.
 *   Only the 16 x 16 tiles on or above the diagonal are computed and the rest is mirrored: outer is exactly symmetric.
 *   Columns [dim, ldx) of x are never read; nothing outside sum[0, dim) and outer[j * ld_outer + k], j, k < dim, is written.
 *   1 <= dim <= 256, else XV_ERR_UNSUPPORTED.  n_rows >= 1, ldx >= dim, ld_outer >= dim, x 16-byte aligned and ldx a multiple
 *   of 4, a workspace of at least xv_moment_stats_workspace_bytes(n_rows, dim) bytes, else XV_ERR_BAD_ARG (nothing is launched).
 * xv_moment_stats_workspace_bytes  the bytes of that workspace (0 for arguments xv_moment_stats_f64 refuses). */
#define XV_MOMENT_SLAB 2048
int xv_moment_stats_f64(const float *x, int64_t ldx, int64_t n_rows, int dim, double *sum, double *outer, int64_t ld_outer,
                        void *workspace, size_t workspace_bytes, void *stream);
size_t xv_moment_stats_workspace_bytes(int64_t n_rows, int dim);

/* ---- clustering for PLDA adaptation (csrc/xv_cluster.hip) ---------------------------------------------------
 * xv_ahc_average_f64  average-linkage agglomerative clustering of n items from their n x n similarity matrix (the PLDA scores
 *   of the unlabelled in-domain vectors against themselves, xv_score_matrix_f32).  The semantics are fixed completely, so that
 *   any implementation gives the same bits:
 *   Input: the similarity of items i < j is (double)scores[i * ld + j].  Only the strict upper triangle is read: the diagonal, the
 *     lower triangle and columns [n, ld) never are.
 *   State: every cluster lives in the slot of its smallest member; size[c] is an integer; T[c, e] is the fp64 sum of the
 *     similarities between the members of c and of e, and T[i, j] starts as the widened score.
 *   Step: avg(c, e) = T[c, e] / (double)(size[c] * size[e]), the integer product formed in int64, the division one IEEE fp64
 *     division.  Among the live pairs c < e the largest avg is taken, ties to the lexicographically smallest (c, e).  Stop if the
 *     cluster count equals min_clusters or if !(avg >= threshold) (a threshold of -inf: down to min_clusters).  Otherwise
 *     (merge_a, merge_b, merge_score)[m] = (c, e, avg); for every other live k, T[k, c] = T[c, k] = T[c, k] + T[e, k] (one fp64
 *     addition, the operands in that order); then size[c] += size[e], and e dies.
 *   Output (device memory): *n_merges = the number of merges; labels[i] = the slot of i's cluster (its smallest member).  Entries
 *     [*n_merges, n - 1) of the three merge arrays are not written, nor is anything past labels[n).
 *   Determinism: no floating-point atomics; each row's best partner is cached and re-scanned only when it can have changed, which
 *     cannot change the answer because avg is a pure function of T and the sizes.  The bits depend on the values, n, threshold and
 *     min_clusters only: not on ld, the stream, the workspace contents or what ran before.
 *   The merges run in one workgroup: launches of up to 256 merges chained in stream order behind a device-side "done"
 *     word; the call enqueues ceil((n - min_clusters) / 256) + 3 launches and does NOT synchronise the stream or read anything back.
 *   n = 1 is valid (0 merges, label 0).  XV_ERR_BAD_ARG, with nothing launched: n < 1, ld < n, ld not a multiple of 4 or scores
 *     not 16-byte aligned, min_clusters outside [1, n], a NaN threshold, a NULL or misaligned output, a workspace that is missing,
 *     not 8-byte aligned or smaller than xv_ahc_average_workspace_bytes(n).  n > XV_AHC_MAX_N: XV_ERR_UNSUPPORTED.  For non-finite
 *     scores the result is unspecified, but the call terminates and writes only inside its outputs.
 * xv_ahc_average_workspace_bytes  the bytes of that workspace: the fp64 n x n state plus O(n) bookkeeping, 8 n^2 + 24 n + 64
 *   (0 for an n xv_ahc_average_f64 refuses). */
#define XV_AHC_MAX_N 32768
int xv_ahc_average_f64(const float *scores, int64_t ld, int n, double threshold, int min_clusters, int32_t *merge_a,
                       int32_t *merge_b, double *merge_score, int32_t *n_merges, int32_t *labels, void *workspace,
                       size_t workspace_bytes, void *stream);
size_t xv_ahc_average_workspace_bytes(int n);

/* ---- diarization: one clustering problem per recording (csrc/xv_cluster.hip) ------------------------------
 * xv_ahc_average_batch_f64  n_groups independent xv_ahc_average_f64 problems in ONE launch, one workgroup per group.  Per-group
 *   inputs, all in device memory: grp_row0 [n_groups + 1] and grp_score0 [n_groups] as for xv_score_blocks_f32 (group g's score
 *   block at scores + grp_score0[g], row stride (n_g + 3) & ~3, only its strict upper triangle is read); grp_ws0 [n_groups]
 *   (int64 byte offsets into the workspace, multiples of 8, each slice xv_ahc_average_batch_workspace_bytes(n_g) bytes);
 *   threshold [n_groups] (fp64); min_clusters [n_groups] (int32).
 *   Semantics: those of xv_ahc_average_f64 above, word for word.  Group g's merges, merge scores, n_merges[g] and labels are
 *     bit-identical to a single-problem call on its block; slot indices are local to the group.  They do not depend on the other
 *     groups, the group's position in the batch, the workspace contents or what ran before.
 *   Outputs need no tables of their own: merge_a, merge_b, merge_score have n_rows entries, group g owns
 *     [grp_row0[g], grp_row0[g] + n_g - 1) and only the first n_merges[g] of those are written; labels [n_rows] holds group g's
 *     labels at grp_row0[g] + i; n_merges [n_groups].
 *   Structure: a group's init, first row caches, merges and labels all run inside its workgroup, between s_barriers; no
 *     cooperative launch, no grid barrier, no workgroup waits on another, no floating-point atomics.  The merge loop is bounded
 *     by construction (m < n_g - min_clusters), so non-finite scores cannot make it spin (their result is unspecified).  The call
 *     enqueues one launch and does NOT synchronise.  Workgroups tend to start in group order (speed alone depends on it) and
 *     a large group runs much longer than a small one: the CALLER puts large groups first, so that the longest do not start last.
 *   XV_ERR_BAD_ARG, nothing launched: a NULL or misaligned pointer (scores 16 bytes; grp_score0, grp_ws0, threshold, merge_score
 *     and the workspace 8; the rest 4), n_groups, n_rows or scores_elems below 1, max_n < 1, workspace_bytes of 0.
 *     max_n > XV_AHC_BATCH_MAX_N: XV_ERR_UNSUPPORTED.
 *   Device side: a group that breaks its contract (n_g outside [1, max_n], rows outside [0, n_rows), a score block as refused by
 *     xv_score_blocks_f32, min_clusters outside [1, n_g], a NaN threshold, a workspace slice that is negative, misaligned or
 *     ends past workspace_bytes) is skipped whole: nothing of it is read or written, and *status receives 1.  The caller zeroes
 *     *status and reads it back with the results.
 * xv_ahc_average_batch_workspace_bytes  the bytes of ONE group's slice, 8 n^2 + 24 n + 64 (0 for n outside
 *   [1, XV_AHC_BATCH_MAX_N]). */
#define XV_AHC_BATCH_MAX_N 4096
int xv_ahc_average_batch_f64(const float *scores, int64_t scores_elems, const int32_t *grp_row0, const int64_t *grp_score0,
                             const int64_t *grp_ws0, const double *threshold, const int32_t *min_clusters, int n_groups, int max_n,
                             int n_rows, int32_t *merge_a, int32_t *merge_b, double *merge_score, int32_t *n_merges, int32_t *labels,
                             int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t xv_ahc_average_batch_workspace_bytes(int n);

/* ---- diarization: per-recording PCA and the PLDA projected into it (csrc/xv_pca.hip) -----------------------
 * What ivector-plda-scoring-dense --target-energy does per recording (EstPca, TransformIvectors, Plda::ApplyTransform).  The rule
 * below was written down from memory of Kaldi's source, not checked against it: the rule AS WRITTEN HERE is the contract.
 * xv_pca_plda_groups_f64  for every group g (rows [grp_row0[g], grp_row0[g + 1]) of y [n_rows, ldy] fp32, n_g >= 1 of them; the
 *   rows are the vectors after mean subtraction, LDA and length normalisation), all in fp64, one workgroup per group:
 *   1. C = (1/n) sum_i y_i y_i^T - m m^T, m = (1/n) sum_i y_i; every sum runs over the rows in ascending order.
 *   2. The eigenpairs of C.  Eigenvalues descending, ties to the smaller column index of the iteration; every eigenvector's
 *      sign is chosen so that its first component of largest magnitude is positive.
 *   3. total = sum of the eigenvalues (descending order); k = the smallest count with (l_1 + .. + l_k) / total > target_energy
 *      (k = dim if none); p_g = min(k + 1, dim) -- Kaldi's loop steps once past the count it summed.
 *   4. A_g [p_g, dim] = the first p_g eigenvectors as rows.  Vectors are projected WITHOUT centring: u = A_g y.
 *   5. With the global model (mean mu, transform P, psi) and within = P^-1 P^-T, between = P^-1 diag(psi) P^-T (formed by the
 *      caller): mu_g = A_g mu, W_g = A_g within A_g^T, B_g = A_g between A_g^T; W_g = L L^T (Cholesky), T1 = L^-1, the eigenpairs of
 *      T1 B_g T1^T descending (V), P_g = V^T T1, psi_g = max(eigenvalue, 0).
 *   Outputs (device memory): grp_dim [n_groups] int32 = p_g; grp_info [n_groups] int32: 0 = PCA applied, 1 = fallback for energy,
 *     2 = fallback for non-convergence; eigvals [n_groups, dim]: the eigenvalues of C, descending (zeros when info is 1 by a
 *     non-finite or non-positive trace, or when the PCA's own iteration did not converge); pca [n_groups, dim, dim] (may be
 *     NULL: not written): rows < p_g hold A_g; grp_psi [n_groups, dim]: psi_g in the first p_g entries; grp_map
 *     [n_groups, dim, dim]: rows < p_g hold M_g = P_g A_g; grp_off [n_groups, dim]: c_g = -P_g mu_g in the first p_g entries.
 *     So z = M_g y + c_g.  Rows and entries at p_g and beyond are not written.
 *   Fallback: total (or the trace of C) not finite or not > 0 (one vector, identical vectors): info 1; an eigen-iteration that
 *     does not converge within XV_PCA_MAX_SWEEPS sweeps, or a W_g that is not positive definite: info 2.  Such a group holds the
 *     global model: p_g = dim, grp_map = transform and grp_psi = psi as exact copies, grp_off[i] = -(sum_k P[i, k] mu[k]) with
 *     rounded products added in ascending k from a zero start, pca = the identity.
 *   Eigen-solver: cyclic Jacobi in a fixed rotation order, a round-robin tournament over m = dim rounded up to even players (the
 *     circle method: step r < m - 1 pairs (m - 1, r) and ((r + k) mod (m - 1), (r - k) mod (m - 1)), 0 < k < m / 2; a pair
 *     holding the index dim, for odd dim, sits out).  The disjoint rotations of a step are applied together.  At the head of
 *     every sweep the iteration stops as converged if max_{i != j} |a_ij| <= 2^-58 max_i |a_ii|; at most XV_PCA_MAX_SWEEPS sweeps
 *     run.  One device function serves the dim x dim problem of step 2 and the p_g x p_g problem of step 5.
 *   Determinism: no floating-point atomics, every value has one writer and every sum one order; the bits of a group's outputs
 *     depend on its own rows, dim, target_energy and the model only: not on the other groups, the group's position, the
 *     workspace contents or what ran before.  The iterate lives in LDS (dim * (dim + 1) doubles, 129 KiB at dim 128: small
 *     problems share a CU), the accumulated eigenvectors in the group's workspace slice.  No cooperative launch, no workgroup
 *     waits on another, every loop is bounded by construction.  One launch; the call does NOT synchronise.
 *   XV_ERR_BAD_ARG, nothing launched: n_groups, n_rows or dim below 1, ldy < dim, a target_energy outside (0, 1] or NaN, a NULL
 *     pointer (pca excepted) or a misaligned one (fp64 arrays and the workspace 8 bytes, the rest 4), a workspace smaller than
 *     xv_pca_plda_groups_workspace_bytes(n_groups, dim).  dim > XV_PCA_MAX_DIM: XV_ERR_UNSUPPORTED.
 *   Device side: a group with n_g < 1 or rows outside [0, n_rows) is skipped whole: nothing of it is read or written, and
 *     *status receives 1.  The caller zeroes *status and reads it back with the results.
 * xv_pca_plda_groups_workspace_bytes  the bytes of that workspace, n_groups * 4 * dim^2 * 8 (0 for arguments the call refuses).
 * xv_backend_prepare_groups_f32  the grouped twin of xv_backend_prepare_f32's PLDA stage: for every row of y [n_rows, ldy] in
 *   group g (the tables above; max_n: an upper bound of every n_g, it sizes the grid), with p = grp_dim[g]:
 *     z_i = sum_k (float)M_g[i, k] y[k] + (float)c_g[i], i < p   (an fmaf chain, k ascending from a zero start, c added after it)
 *     z *= sqrt(p / sum_i z_i^2 / ((float)psi_g[i] + 1))          (Plda::TransformIvector, one utterance; a zero sum: scale 1)
 *     side XV_SIDE_ENROL: the enrolment row of xv_backend_prepare_f32 with n = 1 and psi_g in columns [0, 2 p), r written;
 *          XV_SIDE_TEST:  the test row in columns [0, 2 p), r (may be NULL) written as exactly 0.
 *   Columns [2 p, ldo) receive exact zeros, so xv_score_blocks_f32 scores these rows unchanged with kpad = ldo.  The bits of a
 *   row depend on its values and its group's tables only, not on ldy, ldo or the other rows.
 *   XV_ERR_BAD_ARG, nothing launched: a side other than ENROL / TEST, counts below 1, ldy < dim, ldo < 2 dim or no multiple of
 *     XV_BACKEND_KSTEP, a NULL (r excepted) or misaligned pointer.  dim > XV_PCA_MAX_DIM: XV_ERR_UNSUPPORTED.
 *   Device side: a group with n_g outside [1, max_n], rows outside [0, n_rows) or grp_dim outside [1, dim] is skipped whole and
 *     *status receives 1. */
#define XV_PCA_MAX_DIM 128
#define XV_PCA_MAX_SWEEPS 30
int xv_pca_plda_groups_f64(const float *y, int64_t ldy, int n_rows, const int32_t *grp_row0, int n_groups, int dim,
                           double target_energy, const double *mean, const double *within, const double *between,
                           const double *transform, const double *psi, int32_t *grp_dim, int32_t *grp_info, double *eigvals,
                           double *pca, double *grp_psi, double *grp_map, double *grp_off, int32_t *status, void *workspace,
                           size_t workspace_bytes, void *stream);
size_t xv_pca_plda_groups_workspace_bytes(int n_groups, int dim);
int xv_backend_prepare_groups_f32(const float *y, int64_t ldy, int n_rows, const int32_t *grp_row0, int n_groups, int max_n, int dim,
                                  const int32_t *grp_dim, const double *grp_psi, const double *grp_map, const double *grp_off,
                                  int side, float *out, int64_t ldo, float *r, int32_t *status, void *stream);

/* ---- diarization: VBx resegmentation of every recording's vectors (csrc/xv_vbx.hip) -------------------------
 * A variational-Bayes HMM over the x-vector sequence of one recording (Landini et al., "Bayesian HMM clustering of x-vector
 * sequences"): one state per speaker, speaker means drawn from the PLDA's between-class prior, initialised from a clustering's
 * labels; speakers the data do not support fade out.  The rule below was written down from memory of BUT's VBx.py / vbhmm.py, not
 * checked against them: the rule AS WRITTEN HERE is the contract.
 * xv_vbx_groups_f64  for every group g (rows [grp_row0[g], grp_row0[g + 1]) of y [n_rows, ldy] fp32, T = n_g >= 1 of them, the
 *   rows after mean subtraction, LDA and length normalisation; D = dim), one workgroup per group, all arithmetic in fp64.
 *   Inputs of a group: its rows, visited in time order through row_of_t (int32 [n_rows]; entry grp_row0[g] + t is the row index,
 *     local to the group, of the group's t-th vector in time; a permutation of [0, n_g); NULL = the identity); an initial label
 *     l in [0, S) per ROW (init_label [n_rows], indexed like y); S = grp_spk[g], 1 <= S <= max_spk <= XV_VBX_MAX_SPK; the global
 *     PLDA mu = plda_mean [D], P = transform [D, D], Phi = psi [D]; the scalars Fa = fa > 0, Fb = fb > 0 (both finite), loopP =
 *     loop_prob in [0, 1), smooth = init_smoothing >= 0 (finite), max_iters in [1, XV_VBX_MAX_ITERS], eps = epsilon (any value but
 *     NaN; -inf: never stop early).  y_t below is the row of the t-th vector in time, l_t its initial label.
 *   1. z_t = P (y_t - mu) (no length scaling: this is not Plda::TransformIvector); rho_t = z_t o sqrt(Phi);
 *      G_t = -1/2 (sum_d z_td^2 + D ln 2 pi).
 *   2. gamma_ts = e^smooth / (e^smooth + S - 1) for s = l_t and 1 / (e^smooth + S - 1) otherwise; pi_s = 1 / S.
 *   3. Iteration i = 0, 1, ...:
 *        N_s = sum_t gamma_ts;  invL_sd = 1 / (1 + (Fa/Fb) N_s Phi_d);  alpha_sd = (Fa/Fb) invL_sd sum_t gamma_ts rho_td
 *        l_ts = Fa (sum_d rho_td alpha_sd - 1/2 sum_d (invL_sd + alpha_sd^2) Phi_d + G_t);  m_t = max_s l_ts;  b_ts = exp(l_ts - m_t)
 *        forward:  v_0s = pi_s b_0s;  v_ts = (loopP a_{t-1,s} + (1 - loopP) pi_s) b_ts, t >= 1;  c_t = sum_s v_ts;  a_ts = v_ts / c_t
 *                  (the transition loopP I + (1 - loopP) 1 pi^T, used in its structure: a step costs O(S))
 *        backward: beta_{T-1,s} = 1;  w_s = b_{t+1,s} beta_{t+1,s};  beta_ts = (loopP w_s + (1 - loopP) sum_j pi_j w_j) / c_{t+1}
 *        gamma_ts = a_ts beta_ts
 *        ELBO_i = sum_t (ln c_t + m_t) + (Fb/2) sum_sd (ln invL_sd - invL_sd - alpha_sd^2 + 1)
 *        pi'_s = gamma_0s + (1 - loopP) pi_s sum_{t >= 1} b_ts beta_ts / c_t;  pi = pi' / sum_s pi'_s
 *                  (pi_s = 0 is legal: no logarithm of pi is taken anywhere)
 *        stop after this iteration if i > 0 and ELBO_i - ELBO_{i-1} < eps, or at max_iters.
 *   4. label_t = argmax_s gamma_ts, ties to the smallest s: a slot of the initial labelling (the caller renumbers).
 *   Outputs (device memory), per ROW like y: labels [n_rows] int32; gamma [n_rows, max_spk] (may be NULL: not written), columns
 *     < S; per group: pi [n_groups, max_spk], entries < S; elbo [n_groups, max_iters]: ELBO_0 .. of the iterations that ran, the
 *     entries past grp_iters[g] are not written; grp_iters [n_groups]; grp_info [n_groups].
 *   Fallback: a c_t, an ELBO or a pi normaliser that is zero or not finite (a NaN in a row, a negative psi) gives info 2: the
 *     group's labels are then its initial labels, its other outputs are unspecified but lie inside its own slices.  Otherwise
 *     info 0.  Every loop is bounded by T, S, D and max_iters, whatever the values.
 *   Structure: z / rho are formed once into the group's workspace slice; the two products of an iteration, sum_t gamma_ts rho_td
 *     and sum_d rho_td alpha_sd, and z itself run on v_mfma_f64_16x16x4_f64, their 16 x 16 output tiles dealt to the workgroup's
 *     waves, each tile one chain over its whole summation index in ascending groups of 4; the forward and backward chains run in
 *     one wave, one lane per speaker (hence the cap of 64), with one cross-lane butterfly sum (xor 1, 2, 4, ... below the power of
 *     two that holds S) and one division per step and no exp / log inside; a, b, beta and c live in LDS when (3 S + 1) T doubles
 *     fit, in the workspace slice otherwise, with the same bits either way.
 *   Determinism: no floating-point atomics, every sum has one order; the bits of a group's outputs depend on its own rows,
 *     labels, time order, S, the model and the scalars only: not on the other groups, its position in the batch, ldy, max_spk
 *     (beyond the layout of gamma and pi), the workspace contents or what ran before.  Bit equality with a host evaluation is not
 *     claimed: exp and log differ by library.  No cooperative launch, no workgroup waits on another.  One launch; the call does
 *     NOT synchronise.
 *   XV_ERR_BAD_ARG, nothing launched: n_groups, n_rows or dim below 1, ldy < dim, max_spk outside [1, XV_VBX_MAX_SPK], max_iters
 *     outside [1, XV_VBX_MAX_ITERS], a scalar outside its range above or NaN, a NULL pointer (row_of_t and gamma excepted) or a
 *     misaligned one (fp64 arrays and the workspace 8 bytes, the rest 4), a workspace smaller than
 *     xv_vbx_groups_workspace_bytes(n_rows, n_groups, dim, max_spk).  dim > XV_PCA_MAX_DIM: XV_ERR_UNSUPPORTED.
 *   Device side: a group with n_g < 1, rows outside [0, n_rows), grp_spk outside [1, max_spk], an initial label outside [0, S) or
 *     a row_of_t entry outside [0, n_g) is skipped whole: nothing of it is written, nothing of its rows is read, and *status
 *     receives 1.  The caller zeroes *status and reads it back with the results.
 * xv_vbx_groups_workspace_bytes  the bytes of that workspace, 8 (n_rows (dp + 3 + 3 max_spk) + n_groups 2 max_spk dp) with dp =
 *   dim rounded up to a multiple of 4 (0 for arguments the call refuses). */
#define XV_VBX_MAX_SPK 64
#define XV_VBX_MAX_ITERS 100
int xv_vbx_groups_f64(const float *y, int64_t ldy, int n_rows, const int32_t *grp_row0, int n_groups, int dim,
                      const int32_t *row_of_t, const int32_t *init_label, const int32_t *grp_spk, int max_spk,
                      const double *plda_mean, const double *transform, const double *psi, double fa, double fb, double loop_prob,
                      double init_smoothing, int max_iters, double epsilon, int32_t *labels, double *gamma, double *pi, double *elbo,
                      int32_t *grp_iters, int32_t *grp_info, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
size_t xv_vbx_groups_workspace_bytes(int n_rows, int n_groups, int dim, int max_spk);

/* Stage 1 of the recipe: MFCC features and the energy VAD (compute-mfcc-feats / compute-vad; csrc/xv_mfcc.hip).
 * xv_mfcc_f32  MFCC rows of n_utts utterances in one launch.  samples: every utterance's samples back to back, int16
 *   (sample_format 0) or fp32 (1); utterance u has utt_samples[u] samples from element utt_offset[u], its frames go to rows
 *   utt_row0[u] .. utt_row0[u] + frames(u) - 1 of feats [total_rows, ld_feats] (utt_row0 non-decreasing: the prefix sum of the
 *   frame counts, which the host forms with the geometry below), and utt_key[u] keys its dither noise.
 *   Geometry: frames(n) = snip_edges ? (n < frame_length ? 0 : 1 + (n - frame_length) / frame_shift)
 *                                    : (n + frame_shift / 2) / frame_shift;
 *   frame t starts at t * frame_shift (snip) or t * frame_shift + frame_shift / 2 - frame_length / 2; indices outside [0, n) are
 *   reflected (s < 0 -> -s - 1, s >= n -> 2n - 1 - s) until they land inside.
 *   Per frame: + dither * N(0,1) per sample (Philox4x32-10 keyed on utt_key, counter (sample, frame lo, frame hi, 0), Box-Muller),
 *   - the mean if remove_dc, raw log energy, pre-emphasis, window[frame_length], zero padding to padded_length, power spectrum
 *   of bins 0 .. padded/2 - 1 (radix-2 FFT with twiddle = exp(-2 pi i k / padded) as (re, im) fp32 pairs, k < padded/2),
 *   log-mel b = log(max(sum_j mel_w[b * mel_ld + j] * P[mel_first[b] + j], FLT_EPSILON)) for j < mel_len[b],
 *   feats[c] = sum_b lifter_dct[c * num_bins + b] * logmel[b]; with use_energy, c0 := the log energy (raw_energy: after DC
 *   removal, else after the window), floored at log(energy_floor) when energy_floor > 0.  logmel (NULL: not written) receives
 *   the log-mel energies [total_rows, ld_logmel].  Rows that no utterance's frames cover are not written.  A frame's bits depend
 *   on its utterance's samples, key and the tables only.  padded_length must be a power of two in [128, 1024] and num_bins
 *   <= 128 (else XV_ERR_UNSUPPORTED); frame_length <= padded_length, num_ceps <= num_bins, mel_first[b] + mel_len[b] <=
 *   padded_length / 2 (the caller's tables).
 * xv_vad_energy_f32  compute-vad on ragged utterances: utterance u is rows utt_row0[u] .. + n_frames[u] - 1 of feats (row
 *   stride ld; column 0 = the log energy is the only one read).  thr = energy_threshold + energy_mean_scale * sum_t c0[t] / T
 *   with the sum in fp64 in a fixed order; out[utt_row0[u] + t] = 1.0f when #{t2 in [t - ctx, t + ctx] n [0, T) : c0[t2] > thr}
 *   >= float(den) * proportion_threshold (den = the in-range frames), else 0.0f.  One workgroup per utterance: a decision does not
 *   depend on the other utterances of the launch. */
int xv_mfcc_f32(const void *samples, int sample_format, const int64_t *utt_offset, const int64_t *utt_samples,
                const int64_t *utt_row0, const uint64_t *utt_key, int n_utts, int64_t total_rows, const float *window,
                const int32_t *mel_first, const int32_t *mel_len, const float *mel_w, int num_bins, int mel_ld,
                const float *lifter_dct, int num_ceps, const float *twiddle, int frame_length, int frame_shift, int padded_length,
                int snip_edges, float dither, float preemph_coeff, int remove_dc, int use_energy, int raw_energy,
                float energy_floor, float *feats, int64_t ld_feats, float *logmel, int64_t ld_logmel, void *stream);
int xv_vad_energy_f32(const float *feats, int64_t ld, const int64_t *utt_row0, const int32_t *n_frames, int n_utts,
                      float energy_threshold, float energy_mean_scale, int frames_context, float proportion_threshold, float *out,
                      void *stream);

/* Stage 2 of the recipe: wav-reverberate on the GPU (reverberation, additive noise, level, trim / repeat, the int16 write;
 * csrc/xv_augment.hip).  One evaluation level of many ragged utterances is six launches in this order:
 * power, conv, gains, mix, level, write.  sig: an int16 sample pool holding every input and noise; taps: an fp32 pool of
 * impulse responses (already scaled by 1/32768); y: an fp64 scratch pool (the waveform between the steps).  Utterance u is described by
 * utt[XV_AUG_UTT_FIELDS * u + XV_AUG_*] (int64), noise reference r by refs[XV_AUG_REF_FIELDS * r + XV_AUG_REF_*].
 * xv_augment_power_f64  segment s = segments[4s ..] = (off, len, tile0, ntiles), a run of sig; tile t = tiles[2t ..] = (segment,
 *   i0), i0 a multiple of 16384: tile_sumsq[t] = the fp64 sum of sig[off + i]^2 over i in [i0, min(i0 + 16384, len)); the tiles
 *   of segment s are tile_sumsq[tile0 .. tile0 + ntiles) in order (ntiles = 0 for an empty segment).
 * xv_augment_conv_f64  job j = jobs[5j ..] = (x_off, N, h_off, L, y_off): the full linear convolution of x = sig[x_off .. + N)
 *   with h = taps[h_off .. + L), exact products summed in fp64; output n < N + L - 1 goes to y[y_off + n]
 *   (y_off < 0: not written).  Tile t = tiles[2t ..] = (job, n0) covers outputs n0 .. n0 + 2047 (n0 a multiple of 2048) and
 *   writes tile_sumsq[t] = the fp64 sum of their squares.
 * xv_augment_gains_f32  with S(s) = the sum of power_sumsq over segment s's tiles, in order: per utterance utt_out[4u] = P0 =
 *   S(X_SEG) / N; utt_out[4u + 1] = E = (sum of conv_sumsq over EARLY_TILE0 .. + EARLY_NTILES) / EARLY_LEN, or P0 when
 *   EARLY_NTILES = 0; per reference: ref_power[r] = Pn = S(NOISE_SEG) / NOISE_LEN (0 when NOISE_LEN = 0), ref_scale[r] =
 *   fp32(sqrt(10^(-snr_r / 10) E / Pn)), 0 when Pn = 0.
 * xv_augment_mix_f64  tile t = (utt, n0), n0 a multiple of 1024: for n < Y_LEN, v = y[Y_OFF + n] (RIR != 0) or sig[X_OFF + n];
 *   then for each reference in order, v = v + ref_scale * sig[NOISE_OFF + n - OFFSET] where 0 <= n - OFFSET < NOISE_LEN (fp64,
 *   the product exact); y[Y_OFF + n] = v; tile_sumsq[t] = sum v^2 (fp64).
 * xv_augment_level_f32  utt_out[4u + 2] = P1 = (sum of mix_sumsq over MIX_TILE0 .. + MIX_NTILES) / Y_LEN; utt_out[4u + 3] =
 *   the level: utt_param[2u] (volume) when > 0, else fp32(sqrt(P0 / P1)) when utt_param[2u + 1] != 0 and P1 > 0, else 1.
 * xv_augment_write  tile t = (utt, m0), m0 a multiple of 1024: for m < M, v = trunc(y[Y_OFF + SHIFT + (m mod N)] * level) (fp64),
 *   saturated to [-32768, 32767] (clipped[u] += 1 when saturated), to out[OUT_OFF + m] as int16 (sample_format 0) or fp32 (1).
 *   SHIFT + N <= Y_LEN is the caller's.  Nothing outside the described rows is written. */
#define XV_AUG_UTT_FIELDS 16
#define XV_AUG_X_OFF 0
#define XV_AUG_N 1
#define XV_AUG_Y_OFF 2
#define XV_AUG_Y_LEN 3
#define XV_AUG_RIR 4
#define XV_AUG_EARLY_TILE0 5
#define XV_AUG_EARLY_NTILES 6
#define XV_AUG_EARLY_LEN 7
#define XV_AUG_REF0 8
#define XV_AUG_NREF 9
#define XV_AUG_SHIFT 10
#define XV_AUG_M 11
#define XV_AUG_OUT_OFF 12
#define XV_AUG_MIX_TILE0 13
#define XV_AUG_MIX_NTILES 14
#define XV_AUG_X_SEG 15
#define XV_AUG_REF_FIELDS 4
#define XV_AUG_REF_NOISE_OFF 0
#define XV_AUG_REF_NOISE_LEN 1
#define XV_AUG_REF_OFFSET 2
#define XV_AUG_REF_NOISE_SEG 3
int xv_augment_power_f64(const int16_t *sig, const int64_t *segments, const int64_t *tiles, int64_t n_tiles, double *tile_sumsq,
                         void *stream);
int xv_augment_conv_f64(const int16_t *sig, const float *taps, const int64_t *jobs, const int64_t *tiles, int64_t n_tiles, double *y,
                        double *tile_sumsq, void *stream);
int xv_augment_gains_f32(const int64_t *utt, int n_utts, const int64_t *refs, const float *ref_snr, const int64_t *segments,
                         const double *power_sumsq, const double *conv_sumsq, double *utt_out, double *ref_power, float *ref_scale,
                         void *stream);
int xv_augment_mix_f64(const int16_t *sig, const int64_t *utt, const int64_t *refs, const float *ref_scale, const int64_t *tiles,
                       int64_t n_tiles, double *y, double *tile_sumsq, void *stream);
int xv_augment_level_f32(const int64_t *utt, int n_utts, const double *utt_param, const double *mix_sumsq, double *utt_out,
                         void *stream);
int xv_augment_write(const double *y, const int64_t *utt, const double *utt_out, const int64_t *tiles, int64_t n_tiles, void *out,
                     int sample_format, unsigned long long *clipped, void *stream);

/* ---- training examples: stages 3-5 of the recipe -----------------------------------------------------------
 * What run.sh stage 3 (apply-cmvn-sliding | select-voiced-frames | copy-feats), local/tf/get_egs.sh and create_tar_files.py do to
 * the features, without the intermediate no-silence copy: raw MFCC rows + VAD decisions in, packed float16 [B, T, F] members out.
 * xv_vad_compact_i32  vad[n_frames]: the VAD values of n_utts utterances back to back (utt_start[u], utt_len[u] in frames;
 *   non-zero = voiced).  voiced_count[u] = number of voiced frames of u (the utt2num_frames of the *_no_sil set);
 *   voiced_row[utt_start[u] + j] = frame index inside u of its j-th voiced frame, j < voiced_count[u] (the other entries are left
 *   alone; voiced_row has n_frames entries).  A segmented prefix sum without atomics: bit-identical on every run.  An utterance
 *   whose span leaves [0, n_frames) gets voiced_count 0 and nothing else is touched for it.
 * xv_egs_chunks_f16   x[x_rows, ldx]: the raw rows of the same utterances; chunk c is chunk_len[c] consecutive VOICED frames of
 *   utterance chunk_utt[c] from voiced frame chunk_first[c] on (the numbering of a ranges file).  For j < chunk_len[c], with
 *   t = voiced_row[utt_start[u] + chunk_first[c] + j]:
 *       y[chunk_dst[c] + j feat_dim + f] = half_rne(float(double(x[t][f]) - sum_{ws <= s < we} double(x[s][f]) / (we - ws)))
 *   [ws, we) is the window of xv_cmn_sliding_scatter_f32 around RAW frame t (CMN precedes the selection), the sum is taken in
 *   double precision, the conversion to half rounds to nearest even from the float (overflow: inf, NaN stays NaN).  chunk_dst
 *   counts halves from y (a packed [B, T, F] member is chunk_dst = member + slot T F); chunks may differ in length
 *   (max_chunk_len = the longest), overlap in their sources and come in any order.  A row whose voiced index lies outside
 *   [0, voiced_count[u]), whose utterance is out of range or whose halves would leave [0, y_elems) is skipped: no read, no write. */
int xv_vad_compact_i32(const float *vad, const int32_t *utt_start, const int32_t *utt_len, int n_utts, int64_t n_frames,
                       int32_t *voiced_count, int32_t *voiced_row, void *stream);
int xv_egs_chunks_f16(const float *x, int ldx, int feat_dim, int64_t x_rows, const int32_t *utt_start, const int32_t *utt_len,
                      int n_utts, const int32_t *voiced_count, const int32_t *voiced_row, const int32_t *chunk_utt,
                      const int32_t *chunk_first, const int32_t *chunk_len, const int64_t *chunk_dst, int n_chunks, int max_chunk_len,
                      int cmn_window, int center, int min_window, void *y, int64_t y_elems, void *stream);

/* ---- the extractor's destination-row plan made on the device (csrc/xv_rowplan.hip) ---------------------------
 * What Extractor.submit_raw computes on the host for xv_cmn_sliding_scatter_f32 (libxvector_host.so: one pass over every frame),
 * from VAD decisions that already lie in device memory.  Utterances are addressed as in xv_vad_compact_i32 (utt_start[u],
 * utt_len[u] in frames of a buffer of n_frames rows); they may come in any order and leave gaps.  Integers only, no atomics: the
 * same bits on every run.  An utterance whose span leaves [0, n_frames) is skipped: nothing is read or written for it (its
 * voiced_count is 0).  Entries of rank / dst_row outside the listed spans are never written.
 * xv_voiced_rank_i32  for frame t < utt_len[u], p = utt_start[u] + t: rank[p] = number of voiced frames (vad != 0) of u before t
 *   when vad[p] != 0, else -1; voiced_count[u] = number of voiced frames of u (= xv_vad_compact_i32's).  vad == NULL: every
 *   frame is voiced (rank[p] = t, voiced_count[u] = utt_len[u]).
 * xv_chunk_row_plan_i32  the voiced frames of utterance i, counted from 0, fall into chunks of chunk_size[i] frames; the first
 *   chunks_kept[i] of them exist and chunk k of the utterance is chunk first_chunk[i] + k of the window, of which this batch
 *   holds chunks [b0, b1), chunk c at row row_start[c - b0] of the packed batch (row_start: b1 - b0 entries).  With v = rank[p]:
 *   dst_row[p] = -1 when v < 0 or chunk_size[i] <= 0; else with k = v / size, r = v % size, cid = first_chunk[i] + k:
 *   dst_row[p] = row_start[cid - b0] + r when k < chunks_kept[i] and b0 <= cid < b1, else -1 (an unvoiced frame, a dropped tail,
 *   a chunk of another batch).  The device twin of xv_raw_row_plan (csrc/xv_host.cpp), indexed by feature row.
 * Both: n_utts == 0 returns 0 and launches nothing; a NULL output or a negative n_utts / n_frames is XV_ERR_BAD_ARG. */
int xv_voiced_rank_i32(const float *vad, const int32_t *utt_start, const int32_t *utt_len, int n_utts, int64_t n_frames,
                       int32_t *rank, int32_t *voiced_count, void *stream);
int xv_chunk_row_plan_i32(const int32_t *rank, const int32_t *utt_start, const int32_t *utt_len, const int32_t *chunk_size,
                          const int32_t *chunks_kept, const int32_t *first_chunk, int n_utts, int64_t n_frames, int32_t b0,
                          int32_t b1, const int32_t *row_start, int32_t *dst_row, void *stream);

/* ---- compressed feature output: Kaldi CompressedMatrix payloads (csrc/xv_compress.hip) ------------------------
 * What compute-mfcc-feats --compress=true / copy-feats --compress=true do with CompressedMatrix::CopyFromMat (kAutomaticMethod),
 * restated; the format contract and the error bounds of DESIGN.md §8.10 are claimed, byte equality with Kaldi's own writer is not.
 * All arithmetic is fp32 unless (double) is shown; no fused multiply-add is formed, division is IEEE, subnormals are kept.
 * For a matrix m[T, C], T >= 1:
 *     gmin = min(m); gmax = max(m)        (exact; of a zero extreme, -0.0 is the minimum and +0.0 the maximum when both occur)
 *     if gmax == gmin: gmax = (float)((double)gmin + (1.0 + fabs((double)gmin)))
 *     grange = gmax - gmin
 *     U16(v): f = (v - gmin) / grange; f = min(max(f, 0), 1); (int)trunc((double)(f * 65535.0f) + 0.499)
 *     F16(q): gmin + (grange * 1.52590218966964e-05f) * (float)q
 *     (int) of a double that is not finite or lies outside int: INT_MIN, as the x86 conversion gives (a zero-width segment).
 *     payload = {float gmin, float grange, int32 T, int32 C}, little endian, then
 *     T <= 8 (token "CM2 "): U16(m[t, c]) as uint16, row-major;
 *     T  > 8 (token "CM "), q = T / 4, s = column c sorted ascending:
 *         p0 = min(U16(s[0]), 65532)              p25  = min(max(U16(s[q]), p0 + 1), 65533)
 *         p75 = min(max(U16(s[3 q]), p25 + 1), 65534)   p100 = max(U16(s[T - 1]), p75 + 1)
 *         C x {uint16 p0, p25, p75, p100}, then C x T bytes column-major, with P* = F16(p*):
 *         v < P25: b = clamp(      (int)trunc((double)(((v - P0 ) / (P25  - P0 )) *  64.0f) + 0.5),   0,  64)
 *         v < P75: b = clamp( 64 + (int)trunc((double)(((v - P25) / (P75  - P25)) * 128.0f) + 0.5),  64, 192)
 *         else   : b = clamp(192 + (int)trunc((double)(((v - P75) / (P100 - P75)) *  63.0f) + 0.5), 192, 255)
 * xv_cm_payload_bytes  16 + (rows > 8 ? 8 cols + rows cols : 2 rows cols); 0 for rows == 0 (such a matrix stays a plain record).
 * xv_cm_encode_f32  utterances addressed as in xv_vad_energy_f32: utterance u is rows utt_row0[u] .. + n_frames[u] - 1 of feats,
 *   row stride ld >= n_cols.  Its payload goes to out + out_offset[u] (each offset a multiple of 16, out 16-byte aligned, the
 *   ranges disjoint: the caller's); no byte outside [out_offset[u], out_offset[u] + xv_cm_payload_bytes(T_u, n_cols)) is written,
 *   nothing for T_u = 0.  status[u] = 0, 1 when the utterance holds a NaN or an infinity (or gmax - gmin overflows), or 2 when T_u n_cols >= 2^31 (the frame
 *   counts live on the device); with a non-zero status the payload bytes are unspecified, every other utterance is unaffected.
 *   The bytes of an utterance depend on its values, T and n_cols only: not on the batch, ld or the offsets.
 *   1 <= n_cols <= 128 and n_utts n_cols < 2^31, else XV_ERR_UNSUPPORTED.  Three launches (range, column statistics by an exact
 *   radix select, elements) that leave their results in the payload itself: no workspace.  Enqueues and returns. */
int64_t xv_cm_payload_bytes(int rows, int cols);
int xv_cm_encode_f32(const float *feats, int64_t ld, const int64_t *utt_row0, const int32_t *n_frames, int n_utts, int n_cols,
                     const int64_t *out_offset, uint8_t *out, int32_t *status, void *stream);

/* ---- sample-rate conversion in front of the MFCC kernel (csrc/xv_resample.hip) -------------------------------
 * What compute-mfcc-feats does with --allow-downsample / --allow-upsample: Kaldi's ResampleWaveform (LinearResample, a
 * Hann-windowed sinc with 6 zeros and a cutoff of 0.99 of the lower Nyquist frequency, applied once to the whole wave),
 * restated.  The algorithm below is what is claimed; bit equality with Kaldi's binary (a BLAS dot product) is not.
 * For a rate pair fi -> fo (positive integers, fi != fo): g = gcd(fi, fo), Ui = fi / g, Uo = fo / g.  Output o = u Uo + p
 * (0 <= p < Uo) of a wave x[0 .. n) is
 *     k0 = first[p] + u Ui;   y[o] = sum_j w[p][j] x[k0 + j]   over j < ntaps[p] with 0 <= k0 + j < n
 * as ONE fp32 accumulator from 0.0f, acc = fmaf(w, x, acc), j ascending; a tap outside the wave is skipped.  x is the int16
 * sample converted to fp32 or the fp32 sample; y stays fp32.  The tables of a pair (first, ntaps: Uo int32 each; w: Uo rows of
 * `row` floats, row = the longest tap count, the rest of a row unused) are the caller's (xvector_amd/resample.py forms them in
 * fp64 as Kaldi's LinearResample::SetIndexesAndWeights does and rounds to fp32).
 * xv_resample_num_output  the number of outputs for n input samples: with tick = lcm(fi, fo), L = n (tick / fi), 0 when L <= 0,
 *   else last = L / (tick / fo), less one when that division is exact, and the count is last + 1 (int64 throughout).
 *   -1 for a non-positive rate or fi == fo.  A host function.
 * xv_resample_f32  n_utts ragged utterances of any mix of rate pairs in one launch.  in: every utterance's samples back to back,
 *   int16 (in_format 0) or fp32 (1); utterance u has in_samples[u] samples from element in_offset[u], uses table utt_table[u]
 *   and its outputs o < out_samples[u] go to out[out_offset[u] + o]; nothing else of out is written.  out_samples[u] may not
 *   exceed what xv_resample_num_output gives (the caller's: the kernel does not re-derive it; a smaller count is a prefix).
 *   tables: n_tables descriptors of XV_RS_TAB_FIELDS int64 each IN HOST MEMORY (they travel as a kernel argument, at most
 *   XV_RS_MAX_TABLES per launch): UI, UO, ROW, PHASE_OFF (table t's first and ntaps are first[PHASE_OFF ..] and
 *   ntaps[PHASE_OFF ..], Uo entries each), W_OFF (its weights are w[W_OFF + p ROW + j]) and SPAN (the most input samples the
 *   XV_RS_OUT_TILE consecutive outputs of a tile reach over, from the first tap of the first to the last tap of the last; it
 *   sizes the LDS staging buffer, and first[p] + u Ui and the row ends must be non-decreasing in o).  first, ntaps, w, the
 *   per-utterance arrays and tiles are device memory.  tiles: [n_tiles, 2] int64 = (utterance, first output), the first output
 *   a multiple of XV_RS_OUT_TILE; every output is covered by exactly one tile (the host's list).  A sample's bits depend on
 *   its own wave and table only.  XV_ERR_BAD_ARG: a null pointer, a negative count, an in_format other than 0 / 1, a
 *   descriptor with a non-positive UI / UO / ROW / SPAN or a negative offset.  XV_ERR_UNSUPPORTED: ROW > XV_RS_MAX_ROW, UO >
 *   XV_RS_MAX_UO, n_tables > XV_RS_MAX_TABLES, more than 2^31 - 1 tiles, or a SPAN beyond the LDS of a CU (32760 samples: a
 *   rate ratio above ~31).  A refused call launches nothing; n_tiles == 0 returns 0 and launches nothing. */
#define XV_RS_OUT_TILE 1024
#define XV_RS_MAX_TABLES 8
#define XV_RS_MAX_ROW 1024
#define XV_RS_MAX_UO 4096
#define XV_RS_TAB_FIELDS 6
#define XV_RS_UI 0
#define XV_RS_UO 1
#define XV_RS_ROW 2
#define XV_RS_PHASE_OFF 3
#define XV_RS_W_OFF 4
#define XV_RS_SPAN 5
int64_t xv_resample_num_output(int64_t n, int rate_in, int rate_out);
int xv_resample_f32(const void *in, int in_format, const int64_t *in_offset, const int64_t *in_samples, const int64_t *out_offset,
                    const int64_t *out_samples, const int64_t *utt_table, int n_utts, const int64_t *tables, int n_tables,
                    const int32_t *first, const int32_t *ntaps, const float *w, const int64_t *tiles, int64_t n_tiles, float *out,
                    void *stream);

/* ---- NIST SPHERE audio decoded in front of the MFCC kernel (csrc/xv_sphere.hip) --------------------------------
 * What `sph2pipe -f wav -p [-c N] x.sph |` does for an uncompressed file: the expansion of 8-bit G.711 codes to 16-bit linear
 * PCM (or a byte swap of 16-bit PCM) and the choice of one channel.  The formulas below, exact integer arithmetic, are what is
 * claimed (they give ITU-T G.711's tables); equality with the sph2pipe binary is not.  For a code byte b (0 .. 255):
 *     mu-law:  u = ~b;  t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);  y = (u & 128) ? 132 - t : t - 132
 *     A-law:   a = b ^ 0x55;  t = (a & 15) << 4;  s = (a >> 4) & 7;  t += s ? 0x108 : 8;  if (s > 1) t <<= s - 1;
 *              y = (a & 128) ? t : -t
 *     PCM16:   y = b0 | b1 << 8 (little-endian) or b0 << 8 | b1 (big-endian), as a signed 16-bit value
 * xv_wave_decode  n_utts ragged utterances of any mix of codings in one launch.  raw: raw_bytes bytes of device memory holding
 *   the data regions of the files as they lie on disk.  Utterance u is described by utt[XV_DEC_FIELDS * u + XV_DEC_*] (int64,
 *   device): sample s < N is the code at byte RAW_OFF + s STRIDE + CH_OFF of raw (STRIDE: the bytes of a frame, 1, 2 or 4;
 *   CH_OFF: the chosen channel's place in it, CH_OFF + width <= STRIDE with width 2 for PCM16 and 1 for G.711) and goes to
 *   out[OUT_OFF + s] as int16 (sample_format 0) or as that value in fp32 (1; exact), the formats of xv_mfcc_f32 and
 *   xv_augment_write.  Two utterances may read the same bytes (the two channels of one file).  Nothing of out outside
 *   [OUT_OFF, OUT_OFF + N) is written, whatever the offsets' alignment.  The two reserved fields are zero.
 *   tiles: [n_tiles, 2] int64 (device) = (utterance, o0), o0 a multiple of XV_DEC_TILE: with h = OUT_OFF mod 8 the tile makes the
 *   samples s with o0 <= s + h < o0 + XV_DEC_TILE (tiles are cut at 16-byte boundaries of out, not of the utterance), so an
 *   utterance takes ceil((N + h) / XV_DEC_TILE) tiles; every sample is covered by exactly one tile (the host's list).
 *   raw and out must be 16-byte aligned.  The kernel cannot see how long out is, and the descriptors are device memory: the
 *   caller checks that every span lies inside raw and out and that CODING, STRIDE and CH_OFF are in range before the call
 *   (xvector_amd/hiplib.py wave_decode does, refusing with XV_ERR_BAD_ARG); a workgroup that meets a descriptor outside these
 *   rules, or a span leaving raw, writes nothing.  XV_ERR_BAD_ARG: a null pointer, a negative count, a sample_format other than
 *   0 / 1, a misaligned raw or out.  XV_ERR_UNSUPPORTED: more than 2^31 - 1 tiles.  A refused call launches nothing; n_tiles == 0
 *   returns 0 and launches nothing.  Enqueues and returns. */
#define XV_DEC_TILE 4096
#define XV_DEC_FIELDS 8
#define XV_DEC_RAW_OFF 0
#define XV_DEC_N 1
#define XV_DEC_STRIDE 2
#define XV_DEC_CH_OFF 3
#define XV_DEC_CODING 4
#define XV_DEC_OUT_OFF 5
#define XV_DEC_PCM16_LE 0
#define XV_DEC_PCM16_BE 1
#define XV_DEC_ULAW 2
#define XV_DEC_ALAW 3
int xv_wave_decode(const uint8_t *raw, int64_t raw_bytes, const int64_t *utt, int n_utts, const int64_t *tiles, int64_t n_tiles,
                   void *out, int sample_format, void *stream);

/* ---- sliding-window extraction: the packed rows of overlapping sub-segments (csrc/xv_subseg.hip) --------------
 * xv_cmn_sliding_scatter_f32 indexed by OUTPUT row, so that one frame may go to several rows: the fp32, packed-row sibling of
 * xv_egs_chunks_f16.  x[x_rows, ldx]: the raw rows of n_utts utterances (utt_start[u], utt_len[u] in rows; any order, gaps
 * allowed).  Chunk c is chunk_len[c] consecutive VOICED frames of utterance u = chunk_utt[c] from voiced frame chunk_first[c] on
 * and goes to rows chunk_row[c] .. chunk_row[c] + chunk_len[c] - 1 of y[y_rows, ldy] (e.g. a zero-filled packed batch).  For
 * j < chunk_len[c], with t = voiced_row[utt_start[u] + chunk_first[c] + j] (voiced_count, voiced_row: xv_vad_compact_i32's, voiced_row
 * with x_rows entries; BOTH NULL: every frame is voiced, t = chunk_first[c] + j):
 *     y[(chunk_row[c] + j) ldy + f] = float(double(x[utt_start[u] + t][f]) - sum_{ws <= s < we} double(x[utt_start[u] + s][f]) / (we - ws))
 * for f < feat_dim; [ws, we) is the window of xv_cmn_sliding_scatter_f32 around RAW frame t (CMN precedes the selection), the
 * sum is taken in double precision.  Only columns [0, feat_dim) of the addressed rows are written: gap rows and padding columns
 * keep their contents.  Chunks may overlap in their sources, come in any order and differ in length (max_chunk_len = the
 * longest; rows of a chunk past it are not made).  Chunks whose destination rows overlap are the caller's error (both write).
 * A row is skipped -- no read, no write -- when its utterance is out of range or its span leaves [0, x_rows), its voiced index
 * lies outside [0, voiced_count[u]), its t outside [0, utt_len[u]), or its destination row outside [0, y_rows).
 * n_chunks == 0 returns 0 and launches nothing.  XV_ERR_BAD_ARG before any launch: a NULL required pointer, exactly one of
 * voiced_count / voiced_row NULL, a negative count, feat_dim <= 0, cmn_window <= 0, min_window <= 0, ldx < feat_dim, ldy < feat_dim.
 * No atomics: the same bits on every run.  Enqueues and returns. */
int xv_cmn_sliding_gather_f32(const float *x, int ldx, int feat_dim, int64_t x_rows, const int32_t *utt_start, const int32_t *utt_len,
                              int n_utts, const int32_t *voiced_count, const int32_t *voiced_row, const int32_t *chunk_utt,
                              const int32_t *chunk_first, const int32_t *chunk_len, const int32_t *chunk_row, int n_chunks,
                              int max_chunk_len, int cmn_window, int center, int min_window, float *y, int ldy, int64_t y_rows,
                              void *stream);

/* ---- speech segments from VAD decisions on the device (csrc/xv_segment.hip) ------------------------------------
 * What Kaldi's diarization recipes do with compute_vad_decision.sh + diarization/vad_to_segments.sh, for decisions that never leave
 * the card.  The rule is this project's own and this text is its contract.  An utterance has T frames and decisions v[t]; a frame
 * is voiced iff v[t] != 0 (NaN counts as voiced, as in xv_vad_compact_i32).  Parameters, all in frames: max_gap G >= 0, min_len
 * M >= 1, pad P >= 0 with 2 P <= G, max_len L = 0 (no splitting) or L >= 2 M.  Four steps, in this order:
 *   1. close  a maximal unvoiced run [a, b) with a > 0, b < T and b - a <= G becomes voiced (leading and trailing silence is
 *             never closed);
 *   2. drop   of the maximal voiced runs [a, b) of the result, those with b - a >= M are kept;
 *   3. pad    a kept run becomes [max(a - P, 0), min(b + P, T)) (2 P <= G: kept runs never touch after padding);
 *   4. split  a run of n > L frames (L > 0) becomes k = ceil(n / L) pieces, piece i = [a + floor(i n / k), a + floor((i + 1) n / k)).
 * The segments of the utterance are the pieces in increasing order.  Every piece has at least M and (L > 0) at most L frames, and
 * their number is at most xv_vad_segments_capacity(T, G, M, L) = (T + G + 1) / (M + G + 1) + (L ? T / L : 0), integer division
 * (a host function; -1 for T < 0 or parameters outside the ranges above).
 * xv_vad_segments_i32  vad[n_frames]; utterances are addressed as in xv_vad_compact_i32 (utt_start[u], utt_len[u] in frames; any
 *   order, gaps allowed).  seg_count[u] = the FULL number of segments of u; segment i of u goes to seg_first[seg_off[u] + i] (its
 *   first frame, counted inside u) and seg_len[seg_off[u] + i], and an entry is written only while i < seg_cap[u] and
 *   0 <= seg_off[u] + i < n_slots: a count above the capacity tells the caller its bound was wrong.  Nothing else is written
 *   anywhere.  An utterance whose span leaves [0, n_frames), or with T == 0, gets count 0.  n_utts == 0 returns 0 and launches
 *   nothing.  XV_ERR_BAD_ARG before any launch: a NULL pointer (workspace may be NULL when no bytes are needed), a negative
 *   count, parameters outside the ranges above, workspace_bytes < xv_vad_segments_workspace_bytes(n_frames) (0 for the tiled walk
 *   of this implementation).  One workgroup of XV_SEG_TILE threads per utterance walks it XV_SEG_TILE frames at a time and carries
 *   the last voiced frame, the open run and the output index across tiles.  Integers only, no atomics: the same bits on every
 *   run.  Enqueues and returns. */
#define XV_SEG_TILE 256
int xv_vad_segments_i32(const float *vad, const int32_t *utt_start, const int32_t *utt_len, int n_utts, int64_t n_frames,
                        int max_gap, int min_len, int pad, int max_len, const int32_t *seg_off, const int32_t *seg_cap,
                        int64_t n_slots, int32_t *seg_count, int32_t *seg_first, int32_t *seg_len, void *workspace,
                        size_t workspace_bytes, void *stream);
size_t xv_vad_segments_workspace_bytes(int64_t n_frames);
int64_t xv_vad_segments_capacity(int64_t T, int max_gap, int min_len, int max_len);

#ifdef __cplusplus
}
#endif
#endif /* XVECTOR_HIP_H_ */
