/*
 * ita_mi355x.h -- C ABI of libita_mi355x.so, the MI355X (gfx950) replacement for the
 * reference's ITA custom-dispatch plugin.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes (no torch / HIP types in
 * the signatures; a stream is passed as `void*` holding a hipStream_t, NULL = default stream)
 * and -- except the two drop-in symbols whose reference prototype is `void` -- returns an
 * ita_status.  All file:line citations are relative to the reference repository.
 *
 * Boundary being replaced
 *   samples/inference_udp_FPGA_custom_dispatch/plugin/ITA_dispatch.c:17-27   ITASelfAttention_workgroup
 *   samples/inference_udp_FPGA_custom_dispatch/plugin/ITA_dispatch.c:31-57   ..._workgroup_expanded
 *   samples/inference_udp_FPGA_custom_dispatch/plugin/ITA_spec.mlir:6-9,21-33 2 bindings, 0 constants, 1 workgroup
 *   samples/inference_udp_FPGA_custom_dispatch/main.cpp:171-201               module.main_graph 5-in / 3-out
 *   tests/export_onnx_for_FPGA.py:71-80                                       I/O names of main_graph
 */
#ifndef ITA_MI355X_H_
#define ITA_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITA_MI355X_ABI_VERSION 1

typedef struct ita_context* ita_handle;

typedef enum ita_status {
  ITA_OK = 0,
  ITA_ERR_INVALID_ARG = -1,
  ITA_ERR_BAD_BLOB = -2,      /* magic / bounds / missing tensor */
  ITA_ERR_NO_WEIGHTS = -3,    /* compute call before ita_load_weights */
  ITA_ERR_UNSUPPORTED = -4,   /* dims or a head count the kernels, or this entry point, are not built for */
  ITA_ERR_HIP = -5,           /* a HIP runtime call failed; see ita_error_string */
  ITA_ERR_NO_DEVICE = -6,
  ITA_ERR_NOT_BOUND = -7      /* drop-in symbol called without ita_bind_dispatch */
} ita_status;

typedef enum ita_image_dtype { ITA_IMAGE_F32 = 0, ITA_IMAGE_U8 = 1 } ita_image_dtype;
typedef enum ita_dispatch_dtype { ITA_DISPATCH_F16 = 0, ITA_DISPATCH_F32 = 1 } ita_dispatch_dtype;

/* ---- lifetime --------------------------------------------------------------------------- */
int ita_abi_version(void);
/* Creates a context on HIP device `device_ordinal` (-1: the calling thread's current device). */
int ita_create(ita_handle* out, int device_ordinal);
int ita_destroy(ita_handle h);
/* Uploads an "ITAW0001" blob (ita_weights.h) from host memory; replaces any earlier weights.
 * Dims: E in {64, 128}, S = 128, P = 192, F = 256, H (attention heads) in {1, 2, 3, 4, 6}; H > 1 for an all-int8
 * (ITAW0001) blob only -- ITAW0002 and ITAW0003 blobs run with one head.  Anything else: ITA_ERR_UNSUPPORTED.
 * A layer with H > 1 runs on the block kernels (ita_mha_kernel<E, H>, then the FFN block) behind the stand-alone tokenizer;
 * every entry point below serves it except those that need the one-head stream kernel, which return
 * ITA_ERR_UNSUPPORTED before any launch: ita_mha_q8, ita_mha_long_q8, ita_mha_long_int8, ita_mha_long_int8_taps,
 * ita_mha_long_int8_stats, ita_mha_long_int8_hist, ita_mha_long_int8_propagate, ita_encoder_layer_long, ita_debug_encoder_stamps, ita_vitlstm_forward_slots (and ita_mha_long_f32 / ita_mha_long_f32_stats / ita_mha_long_f32_propagate / ita_encoder_layer_long_f32, which take
 * float layers only).
 * The reference pre-loads weights into the accelerator out of band
 * (docs/HOW-TO-run-the-full-project-workflow.md:55); this is that step. */
int ita_load_weights(ita_handle h, const void* blob, size_t nbytes);
/* The structural check ita_load_weights runs first (ita_weights.h: ita_blob_validate): header, table bounds, and the exact
 * dtype / byte size of every tensor the loader knows, derived from E / P / F / num_layers.  Host only, needs no GPU.
 * bad_name32 (char[32], may be NULL) receives the offending tensor's name. */
int ita_validate_blob(const void* blob, size_t nbytes, char* bad_name32);
/* Pre-sizes the internal workspace for batches up to max_batch so that the compute calls below allocate nothing, and
 * PINS it: after ita_reserve a larger batch is an error (ITA_ERR_INVALID_ARG) instead of a silent reallocation -- HIP
 * graphs captured over this handle and ita_vitlstm_front / _back pairs hold raw pointers into the workspace.  Call
 * ita_reserve again (it synchronises the device) to move to a larger size.  Without any ita_reserve the compute calls
 * grow the workspace on demand (an implicit device synchronisation; refused inside a stream capture).
 *
 * Concurrency: a handle owns ONE workspace and one set of profiling state -- at most one call may be in flight per
 * handle at a time, on one stream (calls on the same stream are ordered and safe).  Use one handle per stream or per
 * thread; the weights are small (about 25 MB with the derived buffers). */
int ita_reserve(ita_handle h, int max_batch);
int ita_get_dims(ita_handle h, int* E, int* S, int* P, int* F, int* H, int* num_layers);

/* ---- errors ------------------------------------------------------------------------------ */
int ita_last_error(void);                 /* status of the calling thread's last failing call */
const char* ita_error_string(void);       /* human readable detail for ita_last_error()        */

/* ---- hot path: device pointers, asynchronous on `stream` ---------------------------------- */

/* ITASelfAttention_QAT.forward (models/ITA/QAT/layers.py:101-127): x (B,128,E) f32 -> y (B,128,E)
 * f32 = dequantised out_proj, with the blob's H heads of P / H features.  layer < num_layers. */
int ita_mha_int8(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, void* stream);

/* As above, also writing the per-stage integer tensors (any pointer may be NULL):
 * x_q (B,128,E) s8, Q/K/V (B,128,P) s8, logits (B,H,128,128) s8, probs (B,H,128,128) u8 (H from ita_get_dims: one
 * 128 x 128 map per head, (B,128,128) at H = 1), ctx (B,128,P) s8 (heads concatenated), out_q (B,128,E) s8.  Used by the parity tests
 * (the reference hooks the same tensors: tests/export_and_validation_W_B.py:25-102). */
typedef struct ita_mha_taps {
  int8_t *x_q, *Q, *K, *V, *logits;
  uint8_t* probs;
  int8_t *ctx, *out_q;
} ita_mha_taps;
int ita_mha_int8_taps(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch,
                      const ita_mha_taps* taps, void* stream);

/* The same block at the accelerator's own boundary: int8 codes in (what `quant` produces, layers.py:103), int8 out_proj
 * codes out (what `dequant` consumes, layers.py:125) -- x_q, out_q (B,128,E) s8 device pointers.  This is the form
 * SURVEY.md section 8(d) prices BASELINE config 2 on (32 KiB of HBM traffic per E = 128 frame instead of 128 KiB).
 * Equal, byte for byte, to the x_q -> out_q taps of ita_mha_int8_taps. */
int ita_mha_q8(ita_handle h, int layer, const int8_t* x_q_dev, int8_t* out_q_dev, int batch, void* stream);

/* The same block on LONG token sequences: x_q, out_q (B, seq_len, E) s8 with seq_len a multiple of 128 in [128, 65536],
 * batch <= 65535, E = 64 or 128 --
 * BASELINE config 5 as it is worded (480 x 720 input, 64x patch-token blow-up: seq_len = 8192).  Same arithmetic as above
 * (layers.py:106-123, ITA_softmax.py:51-61 over a row of seq_len logits); the logits are never materialised: three sweeps over
 * the key tiles per query tile (row maximum, row sum, probabilities -> A.V), Q K^T recomputed in each.  Its Q / K / V^T
 * workspace (3 x 192 bytes per token) belongs to the handle and grows on demand (not inside a stream capture). */
int ita_mha_long_q8(ita_handle h, int layer, const int8_t* x_q_dev, int8_t* out_q_dev, int batch, int seq_len, void* stream);
/* The long form of ita_mha_int8: x, y (B, seq_len, E) f32, y = attn(x) -- x quantised as ita_mha_int8 quantises it, the
 * out_proj codes of ita_mha_long_q8 dequantised.  Shape limits, workspace and refusals of ita_mha_long_q8. */
int ita_mha_long_int8(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, int seq_len, void* stream);
/* ita_mha_long_int8 with the stage tensors and, for chosen query rows, the attention rows read out: y is what
 * ita_mha_long_int8 writes, bit for bit, and every tap is the value the long kernels compute with (the taps kernels are
 * the production kernels' bodies plus stores).  Device pointers, natural row-major layouts, any of them may be NULL:
 * x_q, out_q (B, seq_len, E) s8 (16-byte aligned); Q, K, V, ctx (B, seq_len, P) s8 (4-byte aligned).  rows: a HOST array of n_rows strictly increasing token
 * indices in [0, seq_len), the same query rows of every frame; for each, logits (s8, clamped as the softmax reads them) and
 * probs (u8: the reference's attn_weights) (B, n_rows, seq_len), 4-byte aligned, row_max (B, n_rows) s8 and row_sum (B, n_rows) s32 (the row's
 * maximum logit and the sum of 256 >> (max - logit) the probabilities are divided by).  taps == NULL: all-null taps.
 * Refusals, all before any launch, outputs and taps untouched: whatever ita_mha_long_int8 refuses, with the same status
 * (a float-attention layer: its flash kernel keeps no row probabilities, ita_mha_long_f32_taps reads it out); ITA_ERR_INVALID_ARG for n_rows outside
 * [0, 1024], n_rows > 0 without rows, rows not strictly increasing or out of range, a row-indexed pointer (logits,
 * probs, row_max, row_sum) with n_rows == 0, a misaligned tap, and for a call inside a stream capture (the row table
 * is rebuilt on the host and copied to the handle's device table on `stream` in every call that gives rows). */
typedef struct ita_mha_long_taps {
  int8_t *x_q, *Q, *K, *V, *ctx, *out_q;  /* (B,S,E) / (B,S,P) s8, any may be NULL */
  const int* rows;                         /* HOST array, strictly increasing token indices in [0, seq_len) */
  int n_rows;                              /* 0 .. 1024 */
  int8_t* logits; uint8_t* probs;          /* (B, n_rows, seq_len) */
  int8_t* row_max; int* row_sum;           /* (B, n_rows) */
} ita_mha_long_taps;
int ita_mha_long_int8_taps(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, int seq_len,
                           const ita_mha_long_taps* taps, void* stream);
/* Row and column statistics of the WHOLE seq_len x seq_len probability matrix of ita_mha_long_int8 (H = 1), which is never
 * held: x (B, seq_len, E) f32 is read only, there is no y.  Per query row i (all (B, seq_len), device pointers, any may be
 * NULL): row_max s8 and row_sum s32 as ita_mha_long_taps has them, row_mass s32 = sum_j p[i, j] (256 if the integer
 * softmax lost nothing, 0 for a row it killed), row_nnz s32 = #{j : p[i, j] > 0}.  Per key column j: col_mass s32 =
 * sum_i p[i, j] ("attention received", at most 255 * 65 536), col_nnz s32 = #{i : p[i, j] > 0}.  Equal, bit for bit, to
 * attention_stats_ref.py.  The production projection launch, then one sweep kernel that repeats the three Q K^T sweeps
 * and reduces the probabilities instead of multiplying them with V; the column arrays are zeroed on `stream` (a small kernel:
 * a captured call is kernel nodes only) and added to with integer atomics, so the result does not depend on the order of arrival.  Refusals, all before any
 * launch or memset, outputs untouched: whatever ita_mha_long_int8 refuses, with the same status; ITA_ERR_INVALID_ARG for
 * a NULL x_dev or stats, all six pointers NULL, or an s32 output that is not 4-byte aligned.  Workspace of
 * ita_mha_long_q8: once it holds the call there is no host synchronisation and no allocation, the call may be captured. */
typedef struct ita_mha_long_stats {
  int8_t* row_max; int* row_sum; int* row_mass; int* row_nnz;   /* (batch, seq_len) each, may be NULL */
  int* col_mass; int* col_nnz;                                    /* (batch, seq_len) each, may be NULL */
} ita_mha_long_stats;
int ita_mha_long_int8_stats(ita_handle h, int layer, const float* x_dev, int batch, int seq_len,
                            const ita_mha_long_stats* stats, void* stream);
/* Histograms of the WHOLE seq_len x seq_len matrix of ita_mha_long_int8 (H = 1) in front of and behind its integer softmax,
 * which is never held: the health of the quantisation, where the statistics above describe the attention map.  x (B,
 * seq_len, E) f32 is read only, there is no y.  With acc the int32 Q K^T accumulator (it has no bias term), raw = rne(f32(acc)
 * * f32(ml)), logits = clamp(raw, -128, 127) and p the u8 probabilities, per frame (device pointers, any may be NULL):
 *   logits (B, 256) s64: bin c + 128 = #{(i, j) : logits[i, j] = c};  logits_out (B, 2) s64: #{raw < -128}, #{raw > 127}, what
 *   the clamp changed;  acc_range (B, 2) s32: minimum and maximum of acc, that is, which ml would fit;  shifts (B, 256) s64:
 *   bin s = #{(i, j) : max_j' logits[i, j'] - logits[i, j] = s} (the softmax resolves 0 .. 15 only);  probs (B, 256) s64: bin
 *   v = #{(i, j) : p[i, j] = v}.  Every histogram of a frame sums to seq_len^2 (2^32 at seq_len = 65 536: no 32-bit word holds a frame's
 *   total).  Equal, bit for bit, to attention_hist_ref.py.
 * The production projection launch, then one kernel of two Q K^T sweeps (csrc/ita_long_hist_kernel.h) that counts in LDS
 * and adds to the outputs with integer atomics, so the result does not depend on the order of arrival: the same bytes on every
 * call.  The outputs are set to zero on `stream` first, by a small kernel: a captured call is kernel nodes only.
 * Refusals, all before any launch, outputs untouched: whatever ita_mha_long_int8 refuses, with the same status and words (a
 * float-attention layer, H > 1, a shape outside the limits); ITA_ERR_INVALID_ARG for a NULL x_dev or hist, a bad layer, all
 * five pointers NULL, an s64 output off an 8-byte boundary or acc_range off a 4-byte boundary.  Workspace of
 * ita_mha_long_q8: once it holds the call there is no host synchronisation and no allocation, the call may be captured. */
typedef struct ita_mha_long_hist {
  int64_t *logits, *shifts, *probs;   /* (batch, 256) each, may be NULL */
  int64_t *logits_out;                /* (batch, 2), may be NULL */
  int32_t *acc_range;                 /* (batch, 2), may be NULL */
} ita_mha_long_hist;
int ita_mha_long_int8_hist(ita_handle h, int layer, const float* x_dev, int batch, int seq_len,
                           const ita_mha_long_hist* hist, void* stream);
/* Weighted column sums of the WHOLE seq_len x seq_len probability matrix of ita_mha_long_int8 (H = 1), which is never held:
 *     out[b, r, j] = sum_i w[b, r, i] * p[b, i, j]      w s8 (B, n_w, seq_len), out s32 (B, n_w, seq_len), 1 <= n_w <= 64
 * with p[b, i, j] the u8 probability of query i for key j, the bits of ita_mha_long_taps' probs.  col_mass of
 * ita_mha_long_int8_stats is w = all ones, a probability row is w = one-hot.  The result is exact (equal to
 * attention_propagate_ref.py); the same input gives the same bytes on every call (no atomics).  Range: every partial sum
 * the kernel forms is 128 sum_i w + sum_{i < n} w (p - 128), with |sum w (p - 128)| and |128 sum w| each at most
 * 128 * 128 * seq_len, so it and the result fit s32 for ANY s8 weight at seq_len <= 32 768, and at seq_len = 65 536 for
 * weights in [-127, 127] (127 * 128 * 65 536 < 2^30 each).  The weights are not scanned: beyond that bound the sums wrap.
 * x (B, seq_len, E) f32 is read only; w and out must not overlap each other or x.  Launches: the production projection,
 * ita_long_stats_kernel for the row maximum and row sum of every query (into the workspace), a small kernel that packs them
 * per token, sums the weight rows and permutes w into MFMA operand images, and ita_long_prop_kernel, the transposed sweep
 * (csrc/ita_long_prop_kernel.h).  Workspace: ita_mha_long_q8's plus, per 128-token tile, 1664 + 2048 ceil(n_w / 16) bytes
 * and 256 bytes per frame; once it holds the call there is no host synchronisation and no allocation, the call may be
 * captured and is kernel nodes only.  Refusals, all before any launch, out untouched: whatever ita_mha_long_int8 refuses,
 * with the same status; ITA_ERR_INVALID_ARG for a NULL x_dev, w_dev or out_dev, a bad layer, n_w outside [1, 64], w_dev
 * off a 4-byte boundary or out_dev off a 16-byte boundary. */
int ita_mha_long_int8_propagate(ita_handle h, int layer, const float* x_dev, int batch, int seq_len,
                                const int8_t* w_dev, int n_w, int32_t* out_dev, void* stream);
/* The long form of ita_encoder_layer: y = LN2(x1 + ffn(x1)), x1 = LN1(x + attn(x)) on (B, seq_len, E) f32 rows; x_dev may
 * equal y_dev.  Attention + residual + LN1 are the two long launches (x1 goes to y), the FFN + residual + LN2 then run in
 * place on y, 128 rows per block (ita_ffn_int8's kernel: the FFN is per token).  Shape limits, workspace and refusals of
 * ita_mha_long_q8; in addition a float-FFN layer (ITAW0002 blob: ita_encoder_layer_long_f32 runs it) is ITA_ERR_UNSUPPORTED and a blob without the layer's
 * norm parameters ITA_ERR_BAD_BLOB -- all before any launch. */
int ita_encoder_layer_long(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, int seq_len, void* stream);

/* ITAFeedForward_QAT.forward (models/ITA/QAT/layers.py:61-75). */
int ita_ffn_int8(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, void* stream);
typedef struct ita_ffn_taps { int8_t *x_q, *h, *out_q; } ita_ffn_taps;
int ita_ffn_int8_taps(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch,
                      const ita_ffn_taps* taps, void* stream);

/* FFN kind of a loaded layer: ITA_FFN_INT8 (ITAW0001 blob, ita_ffn_int8) or ITA_FFN_F32 (ITAW0002 blob: the
 * attention-only QAT graph, models/ITA_single_layer_upsample_shuffle/QAT_only_attn/model.py, whose FFN, residual and
 * LayerNorm2 are float32).  ita_ffn_int8 / _taps on an F32 layer, ita_ffn_f32 on an INT8 layer and the drop-in
 * ITAFeedForward_workgroup bound to an F32 layer fail with ITA_ERR_UNSUPPORTED. */
enum { ITA_FFN_INT8 = 0, ITA_FFN_F32 = 1 };
int ita_get_ffn_kind(ita_handle h, int layer, int* kind);
/* the float32 FFN of layer `layer` alone (no residual, no LayerNorm): y = fc2(relu(fc1(x) + b1)) + b2, (B,128,E) f32,
 * bit-identical to two ascending-k fmaf chains per output started from the bias (E = 64, and E = 128 for an ITAW0003 blob) */
int ita_ffn_f32(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, void* stream);
/* Attention kind of a loaded layer: ITA_ATTN_INT8 (ITAW0001 / ITAW0002 blob, ita_mha_int8) or ITA_ATTN_F32 (ITAW0003
 * blob: the float graph, models/ITA_single_layer_upsample_shuffle/model.py, nothing quantised).  ita_mha_int8 / _taps,
 * ita_mha_q8, ita_mha_long_q8, ita_mha_long_int8, ita_encoder_layer_long, ita_debug_encoder_stamps and the drop-in
 * ITASelfAttention_workgroup on an F32 layer, and
 * ita_mha_f32 / ita_mha_long_f32 / ita_mha_long_f32_taps / ita_mha_long_f32_stats / ita_mha_long_f32_propagate on an INT8 layer, fail with ITA_ERR_UNSUPPORTED; each message names the
 * sibling entry (ita_mha_long_int8 <-> ita_mha_long_f32, ita_mha_long_int8_taps <-> ita_mha_long_f32_taps,
 * ita_mha_long_int8_stats <-> ita_mha_long_f32_stats; ita_mha_long_f32_propagate names ita_mha_long_int8_propagate,
 * ita_encoder_layer_long <-> ita_encoder_layer_long_f32). */
enum { ITA_ATTN_INT8 = 0, ITA_ATTN_F32 = 1 };
int ita_get_attn_kind(ita_handle h, int layer, int* kind);
/* the float32 attention block of layer `layer` alone (no residual, no LayerNorm), ITASelfAttention.forward
 * (models/ITA/layers.py:67-88): y = out_proj(softmax(Q K^T) V), Q / K / V = x W^T + b, one head, no 1/sqrt(d);
 * (B,128,E) f32, E = 64 or 128 (the E = 128 float graph, models/ITA_upsample_shuffle/model.py, has no fusion tail).  A
 * frame's result does not depend on the batch it runs in. */
int ita_mha_f32(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, void* stream);
/* The long form of ita_mha_f32: x, y (B, seq_len, E) f32, y = attn(x) over rows of seq_len keys, for a float-attention
 * layer (ITAW0003 blob).  seq_len a multiple of 128 in [128, 65536], batch <= 65535, E = 64 or 128; anything else, and an
 * int8-attention layer (ITAW0001 / ITAW0002 blob: ita_mha_long_int8 runs it), is ITA_ERR_UNSUPPORTED before any launch.
 * One sweep over the key tiles with a running row maximum and sum (exp-softmax is associative); the logits are never
 * materialised.  Its K / V workspace (2 x 768 bytes per token, shared with ita_mha_long_q8's) belongs to the handle and
 * grows on demand (not inside a stream capture: ITA_ERR_INVALID_ARG).  A frame's result does not depend on the batch it
 * runs in; x_dev may equal y_dev. */
int ita_mha_long_f32(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, int seq_len, void* stream);
/* ita_mha_long_f32 with the stage tensors and, for chosen query rows, the attention rows read out -- the float sibling of
 * ita_mha_long_int8_taps: y is what ita_mha_long_f32 writes, bit for bit, and every tap is the f32 register value the two
 * launches compute with (the taps kernels are the production kernels' bodies plus stores).  Device pointers, natural
 * row-major layouts, any of them may be NULL: Q, K, V (B, seq_len, P): the projections' accumulators; ctx (B, seq_len, P):
 * the context after the multiplication by 1 / row_sum, out_proj's operand.  rows: a HOST array of n_rows strictly
 * increasing token indices in [0, seq_len), the same query rows of every frame; for each, logits (B, n_rows, seq_len): the
 * sweep's Q K^T row before the exponential; row_max (B, n_rows): the final running maximum; row_sum (B, n_rows): the
 * final running sum, whose reciprocal scales the context; probs (B, n_rows, seq_len).  The flash sweep never holds a
 * probability, so probs is DEFINED from the three production values, by a small elementwise launch behind the attention:
 *     probs = ita_expf(logits - row_max) * (1.0f / row_sum)
 * one subtraction, the library's exp (oracle: ita_oracle_expf), one division and one multiplication, each a separately
 * rounded f32 operation.  Q, K, V, ctx, logits and probs must be 16-byte aligned, row_max and row_sum 4-byte.
 * taps == NULL: all-null taps.  Refusals, all before any launch, outputs and taps untouched: whatever ita_mha_long_f32
 * refuses, with the same status (an int8-attention layer: ita_mha_long_int8_taps reads it out); ITA_ERR_INVALID_ARG for
 * n_rows outside [0, 1024], n_rows > 0 without rows, rows not strictly increasing or out of range, a row-indexed pointer
 * (logits, probs, row_max, row_sum) with n_rows == 0, a misaligned tap, and for a call inside a stream capture (the row
 * table is rebuilt on the host and copied to the handle's device table on `stream` in every call that gives rows).
 * The struct has a tag and no typedef name -- that identifier is the entry's -- so callers write
 * `struct ita_mha_long_f32_taps`. */
struct ita_mha_long_f32_taps {
  float *Q, *K, *V, *ctx;        /* (B, seq_len, P) f32, natural row-major, any may be NULL */
  const int* rows;               /* HOST array, strictly increasing token indices in [0, seq_len) */
  int n_rows;                    /* 0 .. 1024 */
  float *logits, *probs;         /* (B, n_rows, seq_len) */
  float *row_max, *row_sum;      /* (B, n_rows) */
};
int ita_mha_long_f32_taps(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, int seq_len,
                          const struct ita_mha_long_f32_taps* taps, void* stream);
/* Row and column statistics of the WHOLE seq_len x seq_len probability matrix of ita_mha_long_f32, which is never held --
 * the float sibling of ita_mha_long_int8_stats: x (B, seq_len, E) f32 is read only, there is no y.  With s, m and l the
 * logits, the final running maximum and the final row sum of the production sweep, the probability is the one
 * ita_mha_long_f32_taps defines, p[i, j] = ita_expf(s[i, j] - m[i]) * (1.0f / l[i]), each operation rounded on its own.
 * Per query row i (all (B, seq_len), device pointers, any may be NULL): row_max f32 = m[i] and row_sum f32 = l[i], bit
 * for bit the taps' values; row_gap f32 = sum_j p[i, j] * (m[i] - s[i, j]) >= 0 (the row's entropy is log(row_sum) +
 * row_gap); row_nnz s32 = #{j : p[i, j] >= p_min}.  Per key column j: col_mass f32 = sum_i p[i, j] ("attention
 * received"; a frame's column masses add up to about seq_len), col_nnz s32 = #{i : p[i, j] >= p_min}.
 * The f32 sums are taken in one fixed order (csrc/ita_long_f32_stats_kernel.h; no floating-point atomics): the same input
 * gives the same bits on every call, and a frame's result does not depend on the batch it runs in.  The production
 * projection launch, one kernel that runs the production sweep for m and l and a second sweep that recomputes the logits
 * and reduces p, and for the columns a reduction of the query tiles' partial sums: kernel launches only, so the call
 * may be captured once the workspace holds it.  Workspace: ita_mha_long_f32's, plus 2 x 4 x seq_len bytes per
 * 128-token tile when a column statistic is asked for; it grows on demand (not inside a stream capture:
 * ITA_ERR_INVALID_ARG).  A call that asks for row statistics only launches no column reduction and stores no partials.
 * Refusals, all before any launch, outputs untouched: whatever ita_mha_long_f32 refuses, with the same status (an
 * int8-attention layer: ita_mha_long_int8_stats reads it out); ITA_ERR_INVALID_ARG for a NULL x_dev or stats, all six
 * pointers NULL, an output that is not 4-byte aligned, and p_min that is NaN, <= 0 or > 1.
 * As with ita_mha_long_f32_taps the struct has a tag and no typedef name -- that identifier is the entry's. */
struct ita_mha_long_f32_stats {
  float* row_max; float* row_sum; float* row_gap; int* row_nnz;   /* (batch, seq_len) each, may be NULL */
  float* col_mass; int* col_nnz;                                    /* (batch, seq_len) each, may be NULL */
};
int ita_mha_long_f32_stats(ita_handle h, int layer, const float* x_dev, int batch, int seq_len, float p_min,
                           const struct ita_mha_long_f32_stats* stats, void* stream);
/* Weighted column sums of the WHOLE seq_len x seq_len probability matrix of ita_mha_long_f32, which is never held -- the
 * float sibling of ita_mha_long_int8_propagate:
 *     out[b, r, j] = sum_i w[b, r, i] * p[b, i, j]      w f32 (B, n_w, seq_len), out f32 (B, n_w, seq_len), 1 <= n_w <= 64
 * with p[b, i, j] = ita_expf(s - m) * (1.0f / l) the probability ita_mha_long_f32_taps defines, each operation rounded on
 * its own; s, m and l are the production sweep's bits.  col_mass of ita_mha_long_f32_stats is w = all ones up to the order
 * of the additions, a probability row is w = one-hot.  x (B, seq_len, E) f32 is read only; w and out must not overlap each
 * other or x.  The weights are not scanned: non-finite weights give non-finite sums.
 * Numerical contract.  The f32 sums are taken in one fixed order (csrc/ita_long_f32_prop_kernel.h: fmaf chains of the 64
 * queries of a unit from zero, the units' blocks added in ascending order; no atomics).  Bit-exact: a one-hot weight row
 * gives the bits of the taps' probability row (0 * p adds +0); a weight row gives the same bits whether it is row 0 of an
 * n_w = 1 call or row 37 of an n_w = 64 call; the same input gives the same bits on every call, in any batch position, and
 * alone.  Against the kernels' own probabilities P (the taps' probs of all rows) summed in float64:
 *     |out - sum_i w P| <= gamma_(S+2) * sum_i |w| P,   gamma_n = n u / (1 - n u),  u = 2^-24
 * (any fixed-order f32 sum of S terms, one rounding for a product, one to spare: derived, not measured).  Against float64
 * from the parameters the project's rule holds per case: 3 * e_torch + 4 ulp32(max |truth|), e_torch the error of torch's
 * CPU f32 w @ softmax(q k^T) on the same inputs.
 * Launches: one projection launch that writes the K image and a Q image in the same layout (no V), ita_lf32_stats_kernel
 * for the row maximum and row sum of every query (rows only, into the workspace), and ita_lf32_prop_kernel, the transposed
 * sweep: kernel launches only.  Workspace: ita_mha_long_f32's plus 8 bytes per token; it grows on demand (not inside a
 * stream capture: ITA_ERR_INVALID_ARG); once it holds the call there is no host synchronisation and no allocation, and
 * the call may be captured.  Shape limits of ita_mha_long_f32.  Refusals, all before any launch, out untouched: whatever
 * ita_mha_long_f32 refuses, with the same status (an int8-attention layer: ITA_ERR_UNSUPPORTED, the message names
 * ita_mha_long_int8_propagate); ITA_ERR_INVALID_ARG for a NULL x_dev, w_dev or out_dev, a bad layer, n_w outside [1, 64],
 * w_dev or out_dev off a 16-byte boundary. */
int ita_mha_long_f32_propagate(ita_handle h, int layer, const float* x_dev, int batch, int seq_len,
                               const float* w_dev, int n_w, float* out_dev, void* stream);
/* The long form of ita_encoder_layer for a layer with a float FFN: y = LN2(x1 + ffn(x1)), x1 = LN1(x + attn(x)) on
 * (B, seq_len, E) f32 rows; x_dev may equal y_dev.  Attention + residual + LN1 are the two launches of ita_mha_long_f32
 * (ITAW0003 blob) or of ita_mha_long_int8 (ITAW0002 blob, with that entry's refusals); the float FFN + residual + LN2
 * then run in place on y (ita_ffn_f32's kernel: the FFN is per token).  Shape limits and workspace as above; an int8-FFN
 * layer (ITAW0001 blob: ita_encoder_layer_long runs it) is ITA_ERR_UNSUPPORTED and a blob without the layer's norm
 * parameters ITA_ERR_BAD_BLOB -- all before any launch. */
int ita_encoder_layer_long_f32(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, int seq_len, void* stream);
/* One encoder layer as the model wires it (QAT/model.py:100-113):
 * y = LN2(x1 + ffn(x1)),  x1 = LN1(x + mha(x)).  x_dev and y_dev may alias.
 * A float-FFN layer (ITA_FFN_F32) runs ffn, the residual and LN2 in float32 (QAT_only_attn/model.py:76-88); a
 * float-attention layer (ITA_ATTN_F32) also mha, the residual and LN1 (model.py:96-106). */
int ita_encoder_layer(ita_handle h, int layer, const float* x_dev, float* y_dev, int batch, void* stream);

/* OverlapPatchMerging (models/ITA/QAT/layers.py:39-45): image (B,60,90) -> tokens (B,128,E).
 * ITA_IMAGE_F32: pixels already scaled to [0,1] (the reference host's float(pixel) / 255.0f, main.cpp:168-169).
 * ITA_IMAGE_U8: the 8-bit wire codes as they arrive (main.cpp:37,166); the division by 255 is folded, with the 1/256 of
 * the exact integer bilinear blend, into the conv weights -- the same linear map rounded once per weight, so the tokens
 * of the two forms agree to ~1e-6, not bit for bit (oracle/ita_oracle.c: ita_oracle_tokenizer_u8 / ita_oracle_tokenizer). */
int ita_tokenizer(ita_handle h, const void* image_dev, int image_dtype, float* tokens_dev, int batch, void* stream);

/* refine_inputs' resize (QAT/model.py:29-30: F.interpolate(..., mode='bilinear', align_corners=False)) as a stage of its
 * own, for frames as a camera or a data set delivers them: `batch` frames of height x width pixels of pixel_dtype, row r
 * of frame b at src_dev + (b * frame_stride + r * row_stride) PIXELS (a cropped view of a larger buffer is passed as it
 * is) -> frames_dev (batch,60,90) f32, contiguous, ready for ITA_IMAGE_F32.  Pixel value before blending: u8
 * f32(code) / 255.0f (main.cpp:118,125), u16 min(f32(code) * depth_scale, 1.0f), f32 as is.  The result equals
 * ingest_ref.py: ingest_reference bit for bit (every operation a separately rounded float32 operation).
 * Reads only the pixels [base, base + (height-1) * row_stride + width) of each frame, whatever the alignment of base;
 * writes only the batch * 5400 floats.  Stream-ordered, no allocation, no host synchronisation; needs no weights.
 * ITA_ERR_INVALID_ARG before any launch: a null pointer, a bad dtype, height or width outside [1, 4096], row_stride <
 * width, frame_stride < (height-1) * row_stride + width, a stride above 2^40 pixels, batch < 1, src_dev not aligned to
 * its pixel size, frames_dev not aligned to 4 bytes, and for u16 a depth_scale that is not finite and positive (it is
 * ignored for u8 and f32). */
typedef enum ita_pixel_dtype { ITA_PIXEL_U8 = 0, ITA_PIXEL_U16 = 1, ITA_PIXEL_F32 = 2 } ita_pixel_dtype;
int ita_ingest(ita_handle h, const void* src_dev, int pixel_dtype, int height, int width, long long row_stride,
               long long frame_stride, float depth_scale, float* frames_dev, int batch, void* stream);

/* OverlapPatchMerging(in, out, 7, 2, 3, output_size) (models/ITA/QAT/layers.py:39-45) for ANY frame size and token grid: the
 * way from a camera frame into the long-sequence path (ita_mha_long_int8, ita_encoder_layer_long, ita_fusion_tail_large;
 * BASELINE config 5: 480 x 720 -> 64 x 128 = 8192 tokens).  `batch` frames of height x width pixels, addressed and valued
 * as ita_ingest addresses and values them (strides in pixels; u8 f32(code) / 255.0f, u16 min(f32(code) * depth_scale,
 * 1.0f), f32 as is) -> tokens_dev (batch, tok_h * tok_w, E) f32, token (oy, ox) in row oy * tok_w + ox:
 *   conv 7x7, stride 2, zero padding 3 -> CH x CW = ((height-1)/2 + 1) x ((width-1)/2 + 1)
 *   bilinear CH x CW -> tok_h x tok_w, align_corners = False (up- or down-sampling), LayerNorm over E.
 * Conv and resize are linear, so the four bilinear neighbours are blended on the 7 x 7 input patches first and one
 * ascending 49-step fmaf chain per token and channel, started from the bias, follows: the conv map is never written.  The
 * result equals tokenizer_long_ref.py (blend_patches, then the chain and the LayerNorm) bit for bit, and at 60 x 90 -> 8 x
 * 16 on f32 frames it equals ita_tokenizer(ITA_IMAGE_F32) bit for bit.
 * Reads only the pixels [base, base + (height-1) * row_stride + width) of each frame, whatever the alignment of base;
 * writes only the batch * tok_h * tok_w * E floats.  Stream-ordered, no allocation, no host synchronisation.  Needs loaded
 * weights (ITA_ERR_NO_WEIGHTS) of any blob kind and head count: every blob carries the tokenizer's parameters.
 * ITA_ERR_INVALID_ARG before any launch: the argument faults of ita_ingest (tokens_dev must be aligned to 16 bytes).
 * ITA_ERR_UNSUPPORTED before any launch: tok_h < 1, tok_w not a positive multiple of 16, tok_h * tok_w not a multiple of
 * 128 or above 65536, batch > 65535. */
int ita_tokenizer_long(ita_handle h, const void* src_dev, int pixel_dtype, int height, int width, long long row_stride,
                       long long frame_stride, float depth_scale, int tok_h, int tok_w, float* tokens_dev, int batch,
                       void* stream);

/* The reference HOST's resize as a stage in front of the graph, for hosts that decode camera frames: `batch` u8 frames of
 * height x width, row r of frame b at src_dev + b * frame_stride + r * row_stride (strides in pixels = bytes; a cropped
 * view of a larger buffer is passed as it is) -> wire_dev (batch,60,90) u8, contiguous: the wire frames ITA_IMAGE_U8
 * takes.  It is what stbir_resize_uint8_linear(src, width, height, 0, dst, 90, 60, 0, 1 channel) computes in the reference's
 * replay host (samples/inference_trainingset_custom_dispatch/main.cpp:117-128): stb_image_resize2's default filters --
 * Mitchell on an axis that shrinks, Catmull-Rom on one that grows or keeps its size -- edge clamp, pixel f32(code) *
 * 3.9215689e-03f, code = trunc(clamp(y * 255 + 0.5)).  The result equals ingest_wire_ref.py: ingest_wire_reference bit
 * for bit; that definition is within 1 code of stb's own output, and differs from it only where y * 255 + 0.5 lies
 * within 1e-3 of an integer (tests/golden/resize_stb_*.npz).  A 60 x 90 source comes out unchanged.
 * ita_ingest_wire_prepare builds and uploads the two filter tables of a source size; the handle keeps the last eight
 * sizes.  ita_ingest_wire on a prepared size is stream-ordered, allocates nothing and does not synchronise; on another
 * size it prepares first (allocation, synchronous copies), which is refused with ITA_ERR_INVALID_ARG on a stream that is
 * being captured.  Reads only [base, base + (height-1) * row_stride + width) of each frame, whatever the alignment of
 * base; writes only the batch * 5400 bytes.  Needs no weights.
 * ITA_ERR_INVALID_ARG before any launch: a null pointer, height or width outside [1, 4096], row_stride < width,
 * frame_stride < (height-1) * row_stride + width, a stride above 2^40, batch < 1.
 * ita_resize_table: one axis of those tables on the host (no GPU, no handle): n0[n_out], count[n_out] and
 * coeff[n_out][coeff_width] (zero padded), output o = sum_j coeff[o][j] * source[n0[o] + j]; *width_out = the widest
 * count (ITA_ERR_INVALID_ARG, with *width_out set, if coeff_width is smaller).  Equals ingest_wire_ref.py: resize_tables
 * bit for bit. */
int ita_ingest_wire_prepare(ita_handle h, int height, int width);
int ita_ingest_wire(ita_handle h, const uint8_t* src_dev, int height, int width, long long row_stride,
                    long long frame_stride, uint8_t* wire_dev, int batch, void* stream);
int ita_resize_table(int n_in, int n_out, int* n0, int* count, float* coeff, int coeff_width, int* width_out);

/* Fusion tail (QAT/model.py:116-121): x (B,128,E) -> (B,9,16,32) flattened, row stride 4608. */
int ita_fusion_tail(ita_handle h, const float* x_dev, float* feat_dev, int batch, void* stream);

/* module.main_graph with a leading batch (main.cpp:171-201; tests/export_onnx_for_FPGA.py:71-80):
 *   image (B,1,60,90) f32 or u8 wire frames, additional_data (B,1), quat_data (B,4),
 *   hidden_in_h / hidden_in_c (3,B,128)  ->  output (B,3), hidden_out_h / hidden_out_c (3,B,128).
 * hidden_out_* may alias hidden_in_* (in-place state).  optional float taps (may be NULL): tokens/x1/x2 (B,128,E),
 * feat (B,4608), dec (B,512). */
typedef struct ita_forward_taps { float *tokens, *x1, *x2, *feat, *dec; } ita_forward_taps;
int ita_vitlstm_forward(ita_handle h, const void* image_dev, int image_dtype, const float* additional_data_dev,
                        const float* quat_data_dev, const float* hidden_in_h_dev, const float* hidden_in_c_dev,
                        float* output_dev, float* hidden_out_h_dev, float* hidden_out_c_dev, int batch,
                        const ita_forward_taps* taps, void* stream);

/* The part of the graph behind the encoder on its own (QAT/model.py:116-130): x2 (B,128,64) f32 = the last LayerNorm2
 * output -> fusion tail -> decoder -> cat -> 3 LSTM layers -> fc, in the arithmetic ita_set_tail_mode selects. */
int ita_vitlstm_tail(ita_handle h, const float* x2_dev, const float* additional_data_dev, const float* quat_data_dev,
                     const float* hidden_in_h_dev, const float* hidden_in_c_dev, float* output_dev,
                     float* hidden_out_h_dev, float* hidden_out_c_dev, int batch, void* stream);

/* The same graph cut in two, for software pipelining ACROSS time steps.  A time step's image-only part
 * (tokenizer, encoder, folded tail GEMM) does not depend on the LSTM state, so step t+1's front can run on
 * one stream while step t's back (LSTM layers + fc, small latency-bound kernels) runs on another:
 *     front(t)  on stream F: image -> gate partials in internal buffer `buf` (0 .. ITA_PART_BUFFERS-1)
 *     back(t)   on stream B: partials[buf] + (h, c) -> velocity, new (h, c); must wait for front(t)
 * The caller orders them with events: back(t) after front(t); front(t') after back(t) when it reuses t's
 * buffer.  With buf = t % ITA_PART_BUFFERS the front stream does not wait for the back stream inside a window of
 * ITA_PART_BUFFERS steps.  Measured at 128 frames per step: front alone 32.6 us, back alone 17.3 us, one stream 50 us,
 * two streams 43 us (HIP graph of 8 steps, or ita_vitlstm_pipelined) -- the GPU overlaps about 7 of the 17 us.
 * front + back on one stream equals ita_vitlstm_forward.  Needs tail mode 1. */
#define ITA_PART_BUFFERS 8
int ita_vitlstm_front(ita_handle h, const void* image_dev, int image_dtype, int batch, int buf, void* stream);
/* the same, and records `encoder_done_event` (a hipEvent_t, may be NULL) on `stream` between the encoder and the
 * folded GEMM.  The encoder kernel owns every CU (one persistent workgroup each, all of LDS and VGPRs): small
 * kernels launched next to it only delay some of its workgroups.  Making back(t) wait for this event of front(t+1)
 * puts the LSTM kernels of step t next to the GEMM of step t+1, which leaves room for them. */
int ita_vitlstm_front_ev(ita_handle h, const void* image_dev, int image_dtype, int batch, int buf, void* stream,
                         void* encoder_done_event);
/* The front cut once more, for a THREE-stage pipeline: encoder(t+2) | folded GEMM(t+1) | LSTM + fc(t) on three streams.
 * ita_vitlstm_encode writes the encoder output planes into plane set `plane_set` (0 or 1), ita_vitlstm_fold multiplies
 * that set into partial buffer `buf`; encode + fold on one stream with plane_set 0 equals ita_vitlstm_front.  The caller
 * orders them with events: fold(t) after encode(t); encode(t') after fold(t) when it reuses t's plane set; back(t) after
 * fold(t); fold(t') after back(t) when it reuses t's partial buffer.  Measured from one HIP graph of 8 steps
 * (host.PipelinedSteps): 128 frames per step 38.2 us against 43.0 us for the two-stage form, 64 frames 36.1 / 39.7, one frame
 * 31.7 / 34.0. */
int ita_vitlstm_encode(ita_handle h, const void* image_dev, int image_dtype, int batch, int plane_set, void* stream);
int ita_vitlstm_fold(ita_handle h, int batch, int plane_set, int buf, void* stream);
int ita_vitlstm_back(ita_handle h, const float* additional_data_dev, const float* quat_data_dev,
                     const float* hidden_in_h_dev, const float* hidden_in_c_dev, float* output_dev,
                     float* hidden_out_h_dev, float* hidden_out_c_dev, int batch, int buf, void* stream);
/* n_steps consecutive time steps of the same `batch` streams, pipelined by this library on the caller's two (distinct,
 * non-default) streams: front(t+1) on stream_front overlaps back(t) on stream_back, ordered with events; the state
 * ping-pongs between state_h/state_c (3,batch,128; in: the incoming state, out: the state after the last step) and an
 * internal copy, so no step updates it in place.  image[t] / additional_data[t] / quat_data[t] / output[t] are HOST arrays
 * of n_steps device pointers.  Joins on stream_front: work enqueued there afterwards sees every output.  The calling
 * thread enqueues about six launches per step; it returns without waiting for the GPU. */
int ita_vitlstm_pipelined(ita_handle h, const void* const* image_dev, int image_dtype, const float* const* additional_data_dev,
                          const float* const* quat_data_dev, float* state_h_dev, float* state_c_dev, float* const* output_dev,
                          int batch, int n_steps, void* stream_front, void* stream_back);

/* Time as a dimension: n_steps consecutive steps of `batch` independent streams whose frames are all known up front
 * (offline replay), in one call on one stream.  Only the LSTM head depends on the previous step, so the image-only part
 * (tokenizer, encoder, folded GEMM) of a chunk of steps runs as ONE batch of Tc * batch frames, and the recurrence of
 * those Tc steps as ONE launch (ita_lstm_seq_kernel: the head kernel with a time loop, weights and cell state resident,
 * steps handed over between its workgroups in-kernel).  Tc = max(1, workspace frames / batch): ita_reserve(n_steps *
 * batch) gives one chunk; the result does not depend on the chunking.  Equal to n_steps calls of ita_vitlstm_forward,
 * bit for bit.  Arrays are time-major:
 *   image_dev (n_steps, batch, 60, 90) u8 or f32, additional_data_dev (n_steps, batch), quat_data_dev (n_steps, batch, 4),
 *   output_dev (n_steps, batch, 3);  state_h_dev / state_c_dev (3, batch, 128): in the state before step 0, out the state
 *   after the last step (updated in place);  lengths_dev (batch) int or NULL = all n_steps: stream b takes part in the
 *   steps t < lengths[b] only (0 <= lengths[b] <= n_steps) -- behind them its state is kept and its output rows are not
 *   written.
 * Stream-ordered, no host synchronisation, no allocation once the workspace holds `batch` frames.  Needs tail mode 1
 * (ITA_ERR_UNSUPPORTED otherwise, before any launch); refused between ita_profile_begin and ita_profile_end.
 * ita_head_status reports a timed-out in-kernel wait of this call as it does for the step path.
 * Uses (overwrites) partial buffer 0 and plane set 0 of the front / back form: an ita_vitlstm_front(buf 0) whose
 * ita_vitlstm_back has not run yet is lost, and ita_vitlstm_back(buf 0) after this call is refused until a new front. */
int ita_vitlstm_sequence(ita_handle h, const void* image_dev, int image_dtype, const float* additional_data_dev,
                         const float* quat_data_dev, float* state_h_dev, float* state_c_dev, const int* lengths_dev,
                         float* output_dev, int n_steps, int batch, void* stream);

/* Serving form of the same graph: the LSTM state of `num_slots` independent streams lives in two
 * persistent device arrays state_h / state_c of shape (3, num_slots, 128); frame b of the batch belongs to
 * stream slot_idx[b] (device int array, all distinct within one call) and updates that stream's state
 * in place.  This is how the reference host carries (h, c) from frame to frame (main.cpp:143-148,217-221),
 * generalised from one stream to many.  Needs tail mode 1. */
int ita_vitlstm_forward_slots(ita_handle h, const void* image_dev, int image_dtype, const float* additional_data_dev,
                              const float* quat_data_dev, float* state_h_dev, float* state_c_dev,
                              const int* slot_idx_dev, int num_slots, float* output_dev, int batch, void* stream);

/* Arithmetic of the float tail (fusion conv, decoder, LSTM) inside ita_vitlstm_forward:
 *   1 (default)  fusion conv, decoder and LSTM layer 0's input projection folded into one matrix at load
 *                time; all tail GEMMs on f16 MFMA with split-precision (hi+lo) operands: within 1e-5 of the
 *                f32 graph (task tolerance 1e-4).  The decoder output is never materialised: taps->dec is
 *                left untouched in this mode.
 *   0            the f32 kernels in the CPU oracle's operation order: equal to the oracle bit for bit.
 * hidden_out_* may alias hidden_in_* in both modes. */
int ita_set_tail_mode(ita_handle h, int mode);

/* Device status of the LSTM head of tail mode 1, which runs its three layers and the fc in one launch whose workgroups
 * wait for each other (bounded waits).  *status = 0, or ITA_HEAD_TIMEOUT when a wait timed out since the last query: the
 * outputs of that call are then invalid.  Waits for the device; a non-zero status is cleared and the head re-armed. */
#define ITA_HEAD_TIMEOUT 1
int ita_head_status(ita_handle h, int* status);

/* ---- per-stage timing (bench.py's roofline leg) -------------------------------------------- */
/* Between ita_profile_begin and ita_profile_end every ita_vitlstm_forward call records HIP
 * events on ITS OWN stream around each stage; ita_profile_end synchronises them and returns
 * the summed device time per stage in milliseconds and the number of forwards covered.
 * Stages: 0 tokenizer, 1 int8 MHA (+LN1), 2 int8 FFN (+LN2), 3 fusion tail, 4 decoder GEMM,
 * 5 LSTM + fc.  At most max_forwards calls are recorded (later ones run unprofiled). */
#define ITA_NUM_STAGES 6
int ita_profile_begin(ita_handle h, int max_forwards);
/* Sampled form: only every `every_n`-th forward is instrumented and, when only_stage >= 0, only the two
 * events around that stage are recorded.  An event in the stream costs a ~5 us pipeline bubble (the next
 * kernel can no longer be launched under the previous one's tail), so this is what a throughput
 * measurement uses inside its timed region.  With only_stage = 1 (fused encoder kernel) stage 2 reads 0. */
int ita_profile_begin_sampled(ita_handle h, int max_forwards, int every_n, int only_stage);
int ita_profile_end(ita_handle h, double* stage_ms, int* n_forwards);

/* ---- fusion tail on large token grids (BASELINE config 5) ----------------
 * The layers of models/ITA_single_layer_upsample_shuffle/QAT/model.py:116-121 -- PixelShuffle(2) ||
 * Upsample(x2, bilinear, align_corners=True) -> cat -> Conv2d(5E/4 -> out_ch, 3, padding 1) -- on a
 * tok_h x tok_w token grid (models/ITA_upsample_shuffle/model.py:70-79 declares them with E = 128 and
 * 48 outputs):  x_dev (B, tok_h*tok_w, E) f32 -> out_dev (B, out_ch, 2 tok_h, 2 tok_w) f32.
 * ita_fusion_tail_load takes HOST pointers (conv weight (out_ch, 5E/4, 3, 3), bias (out_ch)), once;
 * it is independent of ita_load_weights; a later call on the same handle replaces the weights, E
 * and out_ch included.  Needs E % 16 == 0, out_ch <= 64, tok_h % 4 == 0, tok_w % 16 == 0,
 * batch <= 65535 (ITA_ERR_UNSUPPORTED otherwise; a refused load leaves the loaded tail in place).
 * Split-precision f16 MFMA: the weights are scaled by a power of two before their f16 hi / lo split
 * (any weight magnitude, exactly), the tokens are split AS THEY COME.  The accuracy claim -- within
 * 2e-5 of the largest output magnitude of the f32 oracle and of a float64 evaluation -- therefore
 * holds for a window of token magnitudes, tested at tokens ~ N(0,1) * 2^p for p = -6 ... +12:
 *   above it, a token or bilinear blend with |value| > 65504 overflows the f16 hi plane (inf, then
 *   NaN, in the output; N(0,1) * 2^14 does);
 *   below it, the lo plane sinks into the f16 subnormals and loses bits: the result stays finite
 *   and the error grows as the tokens shrink -- measured (zero bias, relative to the largest
 *   output) 1.2e-6 at p = -6, 1.9e-5 to 2.3e-5 at p = -10, 7.2e-5 to 7.9e-5 at p = -12, as an
 *   emulation that keeps f16 subnormals predicts: the MFMA does not flush them. */
int ita_fusion_tail_load(ita_handle h, const float* conv_w_host, const float* conv_b_host, int E, int out_ch);
int ita_fusion_tail_large(ita_handle h, const float* x_dev, float* out_dev, int batch, int tok_h, int tok_w,
                          void* stream);

/* Diagnostic: one encoder layer (E = 64) with in-kernel s_memtime stamps, taken by waves 0 and 4 of every
 * workgroup over its first 8 frames, 16 slots each: stamps[((block * 8 + frame) * 2 + wave / 4) * 16 + slot],
 * a u64 device buffer of min(batch, #CUs) * 256 entries.  Slots: 0 frame start, 1 projections done, 2 past the
 * K/V^T barrier, 3 logits, 4 softmax, 5 A.V, 6 past the second barrier, 7 out_proj + LayerNorm1, 8 fc1,
 * 11 fc2 + LayerNorm2 + store; with image_u8_dev (tokenizer fused in front, x_dev unused) 9 and 10: patch blend
 * and conv + LayerNorm of the NEXT frame.  Not used by the product path. */
int ita_debug_encoder_stamps(ita_handle h, int layer, const float* x_dev, const void* image_u8_dev, float* y_dev,
                             int batch, unsigned long long* stamps_dev, void* stream);

/* Diagnostic / test entry: IntegerApproximatedSoftmax (models/ITA/QAT/ITA_softmax.py:51-61) alone, through the same
 * device function and register layout the encoder kernel uses between QK^T and A.V: int8 logits (rows,128) -> u8
 * probabilities (rows,128), both device pointers.  Needs no weights. */
int ita_debug_softmax_rows(ita_handle h, const int8_t* logits_dev, uint8_t* probs_dev, int rows, void* stream);

/* Diagnostic / test entries: which requantisation form a layer runs (read-only).
 * ita_debug_fast_site_ok: host only, no handle: 1 when ita_load_weights' proof admits the single-rounding form for a
 * site with this multiplier (no accumulator value rounds differently once and twice after the clamp), else 0 --
 * also for a multiplier outside (0, 1) or below 130 / 4e6.
 * ita_debug_layer_forms: fast_sites = the ITA_SITE_* mask (bit 0..5: Q, K, V, logits, context, out_proj) of the sites
 * that passed; a stream kernel runs the single-rounding instantiation only when all six did (mask 63).  It is 0 for a
 * layer without stream images.  stream_images = ITA_FORMS_* bits: the attention image (ita_mha_int8 without taps,
 * ita_mha_q8, the long-sequence entries), the whole-layer image (ita_encoder_layer; needs an int8 FFN and both
 * LayerNorms in the blob), the whole-layer image with the tokenizer in front.  Without the attention image the layer
 * runs on the block kernels (stream_range_ok refused it, or H > 1). */
enum { ITA_FORMS_ATTN_IMAGE = 1, ITA_FORMS_LAYER_IMAGE = 2, ITA_FORMS_TOK_IMAGE = 4 };
int ita_debug_fast_site_ok(float mult);
int ita_debug_layer_forms(ita_handle h, int layer, unsigned* fast_sites, int* stream_images);

/* Diagnostic / test entries: the fused requantisation form.  A site's accumulators start at an
 * integer pattern C near 0x4B400000 and one fma(C + sum, mult, K) replaces un-bias, scale and round.
 * ita_debug_fused_site: host only: the load-time search.  1 and *C, *K when a base within 2^18 of 0x4B400000 passes the
 * enumeration of every accumulator value of the clamp range against the reference's two roundings; else 0 (also for a
 * multiplier outside (0, 1) or below 130 / 4e6, or a K outside [2^23, 2^24)).
 * ita_debug_fused_check: the enumeration alone on a given C; form 0: int8 codes, 1: the logits' 16-bit travel form, clamped
 * as the integer softmax clamps it, 2: fc1's ReLU form (codes 0 .. 127); *K (may be null) receives the K it used.
 * ita_debug_layer_fused: fused_sites = bits 0..5 (Q, K, V, logits, context, fc1; 6, 7: see below) proven for this layer and left on by the
 * environment variable ITA_FUSED_SITES (a mask ANDed onto the proven sites when the weights are loaded); fused = 1 when
 * the stream kernels run the fused instantiation (bits 0..4 all set, and fast_sites == 63), 2 when the whole-layer
 * flavours run fc1's fused ReLU form as well (bit 5), else 0; C6 / K6 (may be null): the six bases and constants of bits 0..5
 * (those of bits 6 and 7 are reachable only through ita_debug_layer_dequant). */
int ita_debug_fused_site(float mult, int* C, float* K);
int ita_debug_fused_check(float mult, int form, int C, float* K);
int ita_debug_layer_fused(ita_handle h, int layer, unsigned* fused_sites, int* fused, int* C6, float* K6);
/* The fused dequantise form of the two block outputs, out_proj and fc2 (fused_sites bits 6 and 7): t = fma(C + sum, mult, K),
 * K = 1.5 * 2^23 - round(C mult), then t - 1.5 * 2^23, the clamp to [-128, 127] and the scale.
 * ita_debug_fused_check form 3 is its enumeration on a given C.
 * ita_debug_dequant_site: host only: the search with the base kept within dmax (capped at 2^18) of 0x4B400000.
 * ita_debug_layer_dequant: fused_dq = 1 when the whole-layer flavours of this layer run the form at both sites (bits 6 and 7
 * proven and left on, on top of fused == 2); C2 / K2 (may be null): the bases and constants of out_proj and fc2 (the
 * default base when the form does not run). */
int ita_debug_dequant_site(float mult, int dmax, int* C, float* K);
int ita_debug_layer_dequant(ita_handle h, int layer, int* fused_dq, int* C2, float* K2);
/* Test entry: the first set of f16 hi / lo planes of x2 that the encoder hands to the folded GEMM, rows [0, B) of ld_planes
 * halves each (B within the reserved workspace).  fill != 0: set every byte of those rows, padding included, to fill & 0xff;
 * fill == 0: copy them to the device buffers hi and lo (B * ld_planes halves each).  *ld_planes (may be null) is the row stride. */
int ita_debug_x2_planes(ita_handle h, int fill, void* hi, void* lo, int B, int* ld_planes, void* stream);

/* ---- wire format of the reference's UDP host (ita_wire.h), exported for bindings and tests ------- */
/* frame_out: [desired_velocity, position_x, quat w, x, y, z]; returns 0, or -1 on a short packet */
int ita_wire_unpack_packet(const uint8_t* packet, size_t nbytes, int quat_stride_bug, float* frame_out);
/* main.cpp:381-417: clip x, normalise, scale by desired velocity, near-start x override */
void ita_wire_postprocess(const float* raw3, float desired_velocity, float position_x, float* out3);

/* ---- drop-in symbols of the reference plugin ---------------------------------------------- */

/* Selects the context/layer the two `void` symbols below run, and the element type of their
 * host buffers (the reference's C side says uint16 'float16_t', ITA_dispatch.c:7, its MLIR side
 * says f32, ITA_spec.mlir:30-33; both are supported). */
int ita_bind_dispatch(ita_handle h, int layer, int dispatch_dtype);

/* Same symbol and prototype as ITA_dispatch.c:17-19.  input/output are HOST buffers of
 * 1 x 128 x E elements (E = 128 in ITA_spec.mlir); the body is the full int8 attention block
 * instead of the reference's 16 384-element copy.  Synchronous.  Errors: ita_last_error(). */
void ITASelfAttention_workgroup(const uint16_t* input, uint16_t* output);
/* The 10-argument expanded-memref form (ITA_dispatch.c:31-41): base/aligned/offset/size/stride x 2 */
void ITASelfAttention_workgroup_expanded(const uint16_t* binding0, const uint16_t* binding0_aligned,
                                         size_t binding0_offset, size_t binding0_size, size_t binding0_stride,
                                         uint16_t* binding1, uint16_t* binding1_aligned, size_t binding1_offset,
                                         size_t binding1_size, size_t binding1_stride);
/* FFN twin for the `abs` marker (models/ITA/export/ITA_ONNX.py:35-38), same buffer convention. */
void ITAFeedForward_workgroup(const uint16_t* input, uint16_t* output);

#ifdef __cplusplus
}
#endif
#endif /* ITA_MI355X_H_ */
