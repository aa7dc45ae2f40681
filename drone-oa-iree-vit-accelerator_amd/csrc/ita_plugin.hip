// ita_plugin.hip -- C ABI (include/ita_mi355x.h) over the gfx950 kernels.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off
//        -I include  csrc/ita_plugin.hip -o csrc/libita_mi355x.so
// (the iree_runtime_plugin.cmake equivalent is plugin/ita_runtime_plugin.cmake).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <atomic>
#include <functional>
#include <thread>
#include <vector>

#include "../../include/ita_mi355x.h"
#include "../../include/ita_weights.h"
#include "../../include/ita_wire.h"
#include "ita_f16x3_kernels.h"
#include "ita_lstm_seq_kernel.h"
#include "ita_f32_kernels.h"
#include "ita_int8_kernels.h"
#include "ita_stream_kernel.h"
#include "ita_long_attn_kernel.h"
#include "ita_ffn_f32_kernel.h"
#include "ita_attn_f32_kernel.h"
#include "ita_ingest_kernel.h"

namespace {

thread_local int tl_err = ITA_OK;
thread_local std::string tl_msg;

int fail(int code, const std::string& msg) {
  tl_err = code;
  tl_msg = msg;
  return code;
}
#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(ITA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
  } while (0)

constexpr int K0P = 672;    // exact-f32 path: LSTM layer-0 concat width 517 + 128 = 645, padded to a multiple of 32
constexpr int K0S = 144;    // f16x3 path, LSTM layer 0 remainder: [h_in0 (128) | desvel | quat (4) | 0 pad]
// K of the folded GEMM = 128 tokens x E channels (8192 for ITAViTLSTM, 16384 for the E = 128 graph without a fusion
// tail); row stride of the x2 / Wfold planes = K + 64: a power-of-two stride (16 KB) would put
                                     // every row of a K tile on the same L2 channel
constexpr int NSPLIT = 8;   // split-K of the folded GEMM (1024 x 512 x 8192 -> 256 workgroups)

struct Layer {
  const int8_t *wq, *wk, *wv, *wo, *w1, *w2;
  const int32_t *bq, *bk, *bv, *bo, *b1, *b2;
  float ascal[ITA_A_NSCAL], fscal[ITA_F_NSCAL];
  const float *n1w, *n1b, *n2w, *n2b;
  // float32 FFN of an ITAW0002 blob (the attention-only graph), device pointers; the int8 FFN fields are then null
  bool ffn_f32 = false;
  const float *w1f = nullptr, *b1f = nullptr, *w2f = nullptr, *b2f = nullptr;
  float *w1p = nullptr, *w2p = nullptr;   // E = 128: B-fragment images of W1 / W2 (ita_ffn_f32_frag_image), owned
  // float32 attention of an ITAW0003 blob (the float graph), device pointers; the int8 attention fields are then null
  bool attn_f32 = false;
  const float *wqf = nullptr, *wkf = nullptr, *wvf = nullptr, *bqf = nullptr, *bkf = nullptr, *bvf = nullptr,
              *wof = nullptr, *bof = nullptr;
  // LDS images of the stream kernels (ita_stream_kernel.h), device copies: whole layer, whole layer with the
  // tokenizer in front (layer 0 of the E = 64 model), attention block only
  char *simg_enc = nullptr, *simg_tok = nullptr, *simg_mha = nullptr;
  unsigned fast_sites = 0;   // ITA_SITE_* bits: requantisation sites proven equal under single rounding (fast_site_ok)
};

}  // namespace

struct ita_context {
  int device = 0;
  int num_cus = 256;
  bool loaded = false;
  ita_blob_header hdr{};
  std::vector<char> hblob;
  char* dblob = nullptr;
  std::vector<Layer> layers;
  // float layers (device pointers into dblob)
  const float *tail_b = nullptr, *dec_w = nullptr, *dec_b = nullptr, *fc_w = nullptr, *fc_b = nullptr;
  // derived device buffers
  float* tail_wT = nullptr;
  char* tok_simg = nullptr;                // LDS images of ita_tok_stream_kernel: [u8 frames (conv weights x 1/65280) | f32 frames]
  size_t tok_simg_bytes = 0;               // size of one of the two
  float* wcat[3] = {nullptr, nullptr, nullptr};
  float* bsum[3] = {nullptr, nullptr, nullptr};
  // split-precision (f16 hi/lo) tail: folded tail+decoder matrix and LSTM weights, pre-scaled
  int kfold = 8192, ldfold = 8192 + 64;    // K and plane row stride of the folded GEMM (see the constants above)
  int tail_mode = 1;                       // 1: folded f16x3 GEMMs (default), 0: exact f32 kernels
  bool folded = false;
  _Float16 *foldf_hi = nullptr, *foldf_lo = nullptr;   // G0 once more as B... MFMA fragments [16][K/16][64][8], for batches of <= 32 frames
  _Float16 *fold_hi = nullptr, *fold_lo = nullptr;   // [512][LDFOLD]: G0 = W_ih0[:, :512] . Wfold, rows in permuted gate order
  float* fold_bias = nullptr;                        // [512] gate-major: W_ih0[:, :512] . dec(tail(0)) + b_ih0 + b_hh0
  float fold_inv_scale = 1.0f;
  _Float16 *lw_hi[3] = {nullptr, nullptr, nullptr}, *lw_lo[3] = {nullptr, nullptr, nullptr};   // [512][K0S | 256 | 256]
  float lw_inv_scale[3] = {1.0f, 1.0f, 1.0f};
  // workspace of the f16x3 path
  _Float16 *x2_hi = nullptr, *x2_lo = nullptr, *c1_hi = nullptr, *c1_lo = nullptr,
           *c2_hi = nullptr, *c2_lo = nullptr;
  float* part = nullptr;
  // the LSTM head's meeting words (ita_lstm_head_kernel): [0] device error word, then one arrival counter per 32-frame
  // tile every ITA_HEAD_CNT_STRIDE words; zeroed at allocation, re-armed in-kernel by each tile's last workgroup and by
  // ita_head_status
  unsigned* head_sync = nullptr;
  size_t head_sync_bytes = 0;
  char* seq_ho = nullptr;       // ita_lstm_seq_kernel's hand-off buffers: ITA_SEQ_TILE bytes per 32-stream tile
  // workspace
  int cap = 0;
  bool ws_reserved = false;     // ita_reserve was called: the workspace is pinned (see ensure_workspace)
  int front_cap[ITA_PART_BUFFERS] = {};   // workspace capacity when ita_vitlstm_front filled partial buffer i
  float *bufA = nullptr, *bufB = nullptr, *cat0 = nullptr, *cat1 = nullptr, *cat2 = nullptr, *gates = nullptr,
        *feat = nullptr;
  // per-stage profiling (ita_profile_begin / _end)
  bool prof = false;
  int prof_max = 0, prof_n = 0;
  int prof_every = 1, prof_stage = -1, prof_calls = 0;   // sample every n-th forward; -1 = all stages, else one stage
  std::vector<hipEvent_t> prof_ev;   // per recorded forward: 1 + 1 + 2*L + 3 events
  std::vector<hipEvent_t> pipe_ev;   // ita_vitlstm_pipelined: front-done / back-done rings + fork/join
  float* pipe_h = nullptr;           // ita_vitlstm_pipelined: second copy of (h, c), 2 x (3, pipe_cap, 128)
  int pipe_cap = 0;
  // fusion tail on large token grids (ita_fusion_tail_load / _large, BASELINE config 5)
  _Float16 *tl_hi = nullptr, *tl_lo = nullptr;   // [chunks][9][nt*16][32]
  _Float16 *tu_hi = nullptr, *tu_lo = nullptr;   // upsample branch by linearity (ita_tail_up_kernel): [9][4][3][64][8], E = 128 only
  _Float16 *ts_hi = nullptr, *ts_lo = nullptr;   // its phase 2, the pixel-shuffle channels: [9][48][32] (48 rows whatever out_ch is)
  float* tl_bias = nullptr;
  float tl_inv_scale = 1.0f;
  int tl_E = 0, tl_CO = 0, tl_nt = 0, tl_nchunk = 0;
  // long-sequence attention (ita_mha_long_q8): Q fragments, K / V^T images, column sums; grown on demand
  char* long_ws = nullptr;
  size_t long_ws_bytes = 0;
  // staging for the host-buffer drop-in symbols
  float *dsp_in = nullptr, *dsp_out = nullptr;
  std::vector<float> dsp_host;
};

namespace {

std::mutex g_bind_mu;
ita_handle g_bound = nullptr;
int g_bound_layer = 0;
int g_bound_dtype = ITA_DISPATCH_F16;

template <typename T>
const T* dptr(ita_context* c, const char* name, bool required, bool* ok) {
  const ita_blob_entry* e = ita_blob_find(c->hblob.data(), c->hblob.size(), name);
  if (!e) {
    if (required) *ok = false;
    return nullptr;
  }
  return (const T*)(c->dblob + e->offset);
}
template <typename T>
const T* hptr(ita_context* c, const char* name) {
  const ita_blob_entry* e = ita_blob_find(c->hblob.data(), c->hblob.size(), name);
  return e ? (const T*)(c->hblob.data() + e->offset) : nullptr;
}

void free_weights(ita_context* c) {
  for (Layer& L : c->layers) {
    char** im[] = {&L.simg_enc, &L.simg_tok, &L.simg_mha};
    for (char** q : im) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
    }
    float** fim[] = {&L.w1p, &L.w2p};
    for (float** q : fim) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
    }
  }
  if (c->dblob) (void)hipFree(c->dblob);
  if (c->tail_wT) (void)hipFree(c->tail_wT);
  if (c->tok_simg) (void)hipFree(c->tok_simg);
  c->tok_simg = nullptr;
  for (int l = 0; l < 3; ++l) {
    if (c->wcat[l]) (void)hipFree(c->wcat[l]);
    if (c->bsum[l]) (void)hipFree(c->bsum[l]);
    c->wcat[l] = c->bsum[l] = nullptr;
  }
  void* extra[] = {c->foldf_hi, c->foldf_lo, c->fold_hi, c->fold_lo, c->fold_bias, c->lw_hi[0], c->lw_lo[0], c->lw_hi[1], c->lw_lo[1],
                   c->lw_hi[2], c->lw_lo[2]};
  for (void* q : extra)
    if (q) (void)hipFree(q);
  c->fold_hi = c->fold_lo = c->foldf_hi = c->foldf_lo = nullptr;
  c->fold_bias = nullptr;
  for (int l = 0; l < 3; ++l) c->lw_hi[l] = c->lw_lo[l] = nullptr;
  c->folded = false;
  c->dblob = nullptr;
  c->tail_wT = nullptr;
  c->loaded = false;
}

void free_workspace(ita_context* c) {
  float** bufs[] = {&c->bufA, &c->bufB, &c->cat0, &c->cat1, &c->cat2, &c->gates, &c->feat};
  for (float** b : bufs) {
    if (*b) (void)hipFree(*b);
    *b = nullptr;
  }
  _Float16** hb[] = {&c->x2_hi, &c->x2_lo, &c->c1_hi, &c->c1_lo, &c->c2_hi, &c->c2_lo};
  for (_Float16** b : hb) {
    if (*b) (void)hipFree(*b);
    *b = nullptr;
  }
  if (c->part) (void)hipFree(c->part);
  c->part = nullptr;
  if (c->head_sync) (void)hipFree(c->head_sync);
  c->head_sync = nullptr;
  c->head_sync_bytes = 0;
  if (c->seq_ho) (void)hipFree(c->seq_ho);
  c->seq_ho = nullptr;
  c->cap = 0;
  for (int& fc : c->front_cap) fc = 0;
}

// Growth frees and reallocates every buffer, so it is only allowed while nothing can still reference the old ones:
// never after an explicit ita_reserve (HIP graphs and front/back pairs keep raw pointers into the workspace), and never
// on a stream that is being captured.
int ensure_workspace(ita_context* c, int B, hipStream_t s = nullptr) {
  if (B <= c->cap) return ITA_OK;
  if (c->ws_reserved)
    return fail(ITA_ERR_INVALID_ARG, "batch exceeds the workspace pinned by ita_reserve; call ita_reserve(max_batch) again while idle");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return fail(ITA_ERR_INVALID_ARG, "the workspace cannot grow inside a stream capture; call ita_reserve first");
  free_workspace(c);
  const size_t E = (size_t)c->hdr.E;
  HIPCHK(hipMalloc(&c->bufA, sizeof(float) * B * 128 * E));
  HIPCHK(hipMalloc(&c->bufB, sizeof(float) * B * 128 * E));
  HIPCHK(hipMalloc(&c->feat, sizeof(float) * (size_t)B * 4608));
  HIPCHK(hipMalloc(&c->cat0, sizeof(float) * (size_t)B * K0P));
  HIPCHK(hipMalloc(&c->cat1, sizeof(float) * (size_t)B * 256));
  HIPCHK(hipMalloc(&c->cat2, sizeof(float) * (size_t)B * 256));
  HIPCHK(hipMalloc(&c->gates, sizeof(float) * (size_t)B * 512));
  HIPCHK(hipMalloc(&c->x2_hi, 2 * 2 * (size_t)B * c->ldfold));   // two sets of planes: ita_vitlstm_encode / _fold ping-pong
  HIPCHK(hipMalloc(&c->x2_lo, 2 * 2 * (size_t)B * c->ldfold));
  HIPCHK(hipMalloc(&c->c1_hi, 2 * (size_t)((B + 31) / 32 * 32) * 256));   // fragment order, whole 32-frame tiles
  HIPCHK(hipMalloc(&c->c1_lo, 2 * (size_t)((B + 31) / 32 * 32) * 256));   // fragment order, whole 32-frame tiles
  HIPCHK(hipMalloc(&c->c2_hi, 2 * (size_t)((B + 31) / 32 * 32) * 256));   // fragment order, whole 32-frame tiles
  HIPCHK(hipMalloc(&c->c2_lo, 2 * (size_t)((B + 31) / 32 * 32) * 256));   // fragment order, whole 32-frame tiles
  HIPCHK(hipMalloc(&c->part, ITA_PART_BUFFERS * sizeof(float) * (size_t)NSPLIT * B * 512));   // ita_vitlstm_front/back
  c->head_sync_bytes = sizeof(unsigned) * ITA_HEAD_CNT_STRIDE * ((size_t)1 + (B + 31) / 32);
  HIPCHK(hipMalloc(&c->head_sync, c->head_sync_bytes));
  HIPCHK(hipMemset(c->head_sync, 0, c->head_sync_bytes));
  HIPCHK(hipMalloc(&c->seq_ho, (size_t)ITA_SEQ_TILE * ((B + 31) / 32)));   // 3 KB per frame, whether or not the sequence form is used
  HIPCHK(hipDeviceSynchronize());
  c->cap = B;
  return ITA_OK;
}

template <typename K>
int set_lds(K kernel, int bytes) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return ITA_OK;
}

int check(ita_handle h, int batch, bool need_weights = true) {
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (batch <= 0) return fail(ITA_ERR_INVALID_ARG, "batch must be positive");
  if (need_weights && !h->loaded) return fail(ITA_ERR_NO_WEIGHTS, "ita_load_weights has not been called");
  HIPCHK(hipSetDevice(h->device));
  return ITA_OK;
}

ItaMhaArgs mha_args(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, const ita_mha_taps* t) {
  const Layer& L = c->layers[layer];
  ItaMhaArgs a{};
  a.x = x; a.y = y;
  a.wq = L.wq; a.wk = L.wk; a.wv = L.wv; a.wo = L.wo;
  a.bq = L.bq; a.bk = L.bk; a.bv = L.bv; a.bo = L.bo;
  a.inv_sx = L.ascal[ITA_A_INV_SX]; a.mq = L.ascal[ITA_A_MQ]; a.mk = L.ascal[ITA_A_MK]; a.mv = L.ascal[ITA_A_MV];
  a.ml = L.ascal[ITA_A_ML]; a.mc = L.ascal[ITA_A_MC]; a.mo = L.ascal[ITA_A_MO]; a.so = L.ascal[ITA_A_SO];
  a.ln_w = L.n1w; a.ln_b = L.n1b;
  a.B = B; a.fuse_ln = fuse ? 1 : 0;
  if (t) {
    a.t_xq = t->x_q; a.t_Q = t->Q; a.t_K = t->K; a.t_V = t->V; a.t_logits = t->logits; a.t_probs = t->probs;
    a.t_ctx = t->ctx; a.t_out = t->out_q;
  }
  return a;
}

struct StreamIo;
int launch_stream(ita_context* c, int layer, int mode, bool fuse_ln, const StreamIo& io, int B, hipStream_t s);
int launch_mha_stream(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s);

// the attention block: without taps on the stream kernel (weights resident in LDS, activations chained through
// registers); with taps, or for a layer without an LDS image, on the tile-phased kernel that can expose every tensor
int launch_mha(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, const ita_mha_taps* t,
               hipStream_t s) {
  if (c->layers[layer].attn_f32)
    return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): ita_mha_f32 runs it");
  if (fuse && !c->layers[layer].n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
  if (!t && c->layers[layer].simg_mha) return launch_mha_stream(c, layer, x, y, B, fuse, s);
  const ItaMhaArgs a = mha_args(c, layer, x, y, B, fuse, t);
  const int grid = B < c->num_cus ? B : c->num_cus;
  if (c->hdr.E == 64) {
    hipLaunchKernelGGL(ita_mha_kernel<64>, dim3(grid), dim3(512), ItaMhaLds<64>::TOTAL, s, a);
  } else {
    hipLaunchKernelGGL(ita_mha_kernel<128>, dim3(grid), dim3(512), ItaMhaLds<128>::TOTAL, s, a);
  }
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

int launch_ffn(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, const ita_ffn_taps* t,
               hipStream_t s, _Float16* y_hi = nullptr, _Float16* y_lo = nullptr) {
  const Layer& L = c->layers[layer];
  if (L.ffn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's FFN is float32 (ITAW0002 blob): ita_ffn_f32 runs it");
  if (fuse && !L.n2w) return fail(ITA_ERR_BAD_BLOB, "norm2 parameters missing from the blob");
  ItaFfnArgs a{};
  a.x = x; a.y = y; a.w1 = L.w1; a.w2 = L.w2; a.b1 = L.b1; a.b2 = L.b2;
  a.inv_sx = L.fscal[ITA_F_INV_SX]; a.m1 = L.fscal[ITA_F_M1]; a.m2 = L.fscal[ITA_F_M2]; a.s2 = L.fscal[ITA_F_S2];
  a.ln_w = L.n2w; a.ln_b = L.n2b; a.B = B; a.fuse_ln = fuse ? 1 : 0;
  if (t) { a.t_xq = t->x_q; a.t_h = t->h; a.t_out = t->out_q; }
  a.y_hi = y_hi; a.y_lo = y_lo; a.ld_planes = c->ldfold;
  const int grid = B < 2 * c->num_cus ? B : 2 * c->num_cus;
  if (c->hdr.E == 64) {
    hipLaunchKernelGGL(ita_ffn_kernel<64>, dim3(grid), dim3(512), ItaFfnLds<64>::TOTAL, s, a);
  } else {
    hipLaunchKernelGGL(ita_ffn_kernel<128>, dim3(grid), dim3(512), ItaFfnLds<128>::TOTAL, s, a);
  }
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

// the float32 FFN (ita_ffn_f32_kernel.h) of an ITAW0002 layer, fuse: + residual + LayerNorm2
int launch_ffn_f32(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s,
                   _Float16* y_hi = nullptr, _Float16* y_lo = nullptr, const float* h0_src = nullptr, float* h0_dst = nullptr,
                   const int* slots = nullptr) {
  const Layer& L = c->layers[layer];
  if (!L.ffn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's FFN is int8 (ITAW0001 blob): ita_ffn_int8 runs it");
  if (c->hdr.E != 64 && !L.w1p) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN of an ITAW0002 blob is built for E = 64");
  if (fuse && !L.n2w) return fail(ITA_ERR_BAD_BLOB, "norm2 parameters missing from the blob");
  ItaFfnF32Args a{};
  a.x = x; a.y = y; a.w1 = L.w1f; a.b1 = L.b1f; a.w2 = L.w2f; a.b2 = L.b2f; a.ln_w = L.n2w; a.ln_b = L.n2b;
  a.B = B; a.fuse_ln = fuse ? 1 : 0;
  a.y_hi = y_hi; a.y_lo = y_lo; a.ld_planes = c->ldfold;
  a.h0_src = h0_src; a.h0_dst = h0_dst; a.slots = slots;
  const int cap = 2 * c->num_cus;
  if (c->hdr.E == 64) {
    const int ntile = B * (128 / ItaFfnF32Lds<64>::TT);
    hipLaunchKernelGGL(ita_ffn_f32_kernel<64>, dim3(ntile < cap ? ntile : cap), dim3(256), ItaFfnF32Lds<64>::TOTAL, s, a);
  } else {   // E = 128: the weights stream as fragment images (66 KB of LDS: two workgroups per CU)
    a.w1 = L.w1p; a.w2 = L.w2p;
    const int ntile = B * (128 / ItaFfnF32Lds<128>::TT);
    hipLaunchKernelGGL(ita_ffn_f32_kernel<128>, dim3(ntile < cap ? ntile : cap), dim3(256), ItaFfnF32Lds<128>::TOTAL, s, a);
  }
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

// the float32 attention block (ita_attn_f32_kernel.h) of an ITAW0003 layer, fuse: + residual + LayerNorm1
int launch_attn_f32(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s) {
  const Layer& L = c->layers[layer];
  if (!L.attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is int8 (ITAW0001 / ITAW0002 blob): ita_mha_int8 runs it");
  if (fuse && !L.n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
  ItaAttnF32Args a{};
  a.x = x; a.y = y;
  a.wq = L.wqf; a.wk = L.wkf; a.wv = L.wvf; a.bq = L.bqf; a.bk = L.bkf; a.bv = L.bvf; a.wo = L.wof; a.bo = L.bof;
  a.ln_w = L.n1w; a.ln_b = L.n1b; a.B = B; a.fuse_ln = fuse ? 1 : 0;
  // 130 KB (E = 64) / 96 KB (E = 128) of LDS: one workgroup per CU, frames in a grid stride
  if (c->hdr.E == 64)
    hipLaunchKernelGGL(ita_attn_f32_kernel<64>, dim3(B < c->num_cus ? B : c->num_cus), dim3(512), ItaAttnF32Lds<64>::TOTAL, s, a);
  else
    hipLaunchKernelGGL(ita_attn_f32_kernel<128>, dim3(B < c->num_cus ? B : c->num_cus), dim3(512), ItaAttnF32Lds<128>::TOTAL, s, a);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

// ---- stream kernels (ita_stream_kernel.h): the LDS image a workgroup copies verbatim at start-up.
// Natural-k matrices (Wq, Wk, Wv, W1) are chunk-major [k/16][row][16].  The block output projections (Wo, fc2)
// consume activations that were packed four 16-feature tiles at a time straight from MFMA accumulators:
// fragment ks of lane (token, kq) holds, at byte 4j+i, feature 16(4ks+j) + 4kq + i -- so chunk 4ks+kq of their
// image holds those input features, and image row 16et + rho is output channel (E/4)(rho>>2) + 4et + (rho&3),
// which hands lane (token, kq) its own channels (E/4)kq + 4et + i.
struct StreamHostParams {
  const int8_t *wq, *wk, *wv, *wo, *w1, *w2;
  const int32_t *bq, *bk, *bv, *bo, *b1, *b2;
  const float *n1w, *n1b, *n2w, *n2b, *tlw, *tlb, *conv_w, *conv_b;
};

// The integer conv tables of the u8 tokenizer (ita_stream_kernel.h: ItaTokTab; definition: oracle/ita_oracle.c
// ita_oracle_tok_quant_weights / ita_oracle_tokenizer_u8): per channel 23-bit fixed-point weights Wq = rne(w * 2^e), e = 22 -
// exponent(max |w|), split into balanced bytes w0, w1 and the remainder w2, laid out as int8 MFMA A fragments.
template <int E>
void build_tok_tab(const float* conv_w, const float* conv_b, char* tab) {
  using T = ItaTokTab<E>;
  int32_t* ti = (int32_t*)(tab + T::TI);
  float* ts = (float*)(tab + T::TS);
  std::vector<int8_t> dig((size_t)E * 49 * 3);
  for (int c = 0; c < E; ++c) {
    float mx = 0.0f;
    for (int k = 0; k < 49; ++k) mx = fmaxf(mx, fabsf(conv_w[(size_t)c * 49 + k]));
    int e = 0;
    if (mx > 0.0f) {
      int ex;
      (void)frexpf(mx, &ex);
      e = 22 - ex;
    }
    long long s0 = 0, s1 = 0, s2 = 0;
    for (int k = 0; k < 49; ++k) {
      const int32_t W = (int32_t)rintf(ldexpf(conv_w[(size_t)c * 49 + k], e));
      const int32_t w0 = ((W + 128) & 255) - 128, W1r = (W - w0) >> 8;
      const int32_t w1 = ((W1r + 128) & 255) - 128, w2 = (W1r - w1) >> 8;
      dig[((size_t)c * 49 + k) * 3 + 0] = (int8_t)w0; dig[((size_t)c * 49 + k) * 3 + 1] = (int8_t)w1; dig[((size_t)c * 49 + k) * 3 + 2] = (int8_t)w2;
      s0 += w0; s1 += w1; s2 += w2;
    }
    // the kernel feeds a ^ 0x80 = a - 128: S0 = S0' + 128 sum w0, S1 = S1' + 128 (sum w1 + sum w0), ... (L = S0 + 256 S1, H = S2 + 256 S3)
    ti[c] = (int32_t)(128 * s0 + 256 * 128 * (s1 + s0));
    ti[E + c] = (int32_t)(128 * (s2 + s1) + 256 * 128 * s2);
    const float sc = ldexpf(1.0f, -e) / 65280.0f;
    ts[c] = sc; ts[E + c] = 65536.0f * sc; ts[2 * E + c] = conv_b[c];
  }
  for (int ct = 0; ct < T::NCT; ++ct)
    for (int j = 0; j < 3; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        const int rho = lane & 15, kq = lane >> 4, ch = (E / 4) * (rho >> 2) + 4 * ct + (rho & 3);
        for (int b = 0; b < 16; ++b) {
          const int t = 4 * b + kq;        // slot b of k-group kq <-> tap 4 b + kq (the lane that blends it); taps >= 49: zero
          tab[T::TW + ((ct * 3 + j) * 64 + lane) * 16 + b] = t < 49 ? (char)dig[((size_t)ch * 49 + t) * 3 + j] : 0;
        }
      }
}

template <int E, bool FFN, bool TOK>
int build_stream_image(const StreamHostParams& p, char** d_out) {
  using L = ItaStreamLds<E, FFN, TOK>;
  constexpr int P = 192, F = 256;
  std::vector<char> im(L::GIMAGE, 0);   // (E = 128 with FFN: fc1 / fc2 weights lie behind the LDS part)
  auto natural = [&](int off, const int8_t* w, int rows, int kb) {
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < kb; ++k) im[off + (((k >> 4) * rows + r) << 4) + (k & 15)] = (char)w[(size_t)r * kb + k];
  };
  auto fragment = [&](int off, const int8_t* w, int nks, int kb) {   // w: [E][kb], kb = 64 * nks
    for (int ks = 0; ks < nks; ++ks)
      for (int kq = 0; kq < 4; ++kq)
        for (int et = 0; et < E / 16; ++et)
          for (int rho = 0; rho < 16; ++rho) {
            const int ch = (E / 4) * (rho >> 2) + 4 * et + (rho & 3);
            for (int j = 0; j < 4; ++j)
              for (int i = 0; i < 4; ++i)
                im[off + (((4 * ks + kq) * E + et * 16 + rho) << 4) + 4 * j + i] =
                    (char)w[(size_t)ch * kb + (4 * ks + j) * 16 + 4 * kq + i];
          }
  };
  natural(L::WQ, p.wq, P, E); natural(L::WK, p.wk, P, E); natural(L::WV, p.wv, P, E);
  fragment(L::WO, p.wo, 3, P);
  int32_t* bias = (int32_t*)(im.data() + L::BIAS);
  memcpy(bias, p.bq, P * 4); memcpy(bias + P, p.bk, P * 4); memcpy(bias + 2 * P, p.bv, P * 4);
  memcpy(bias + 3 * P, p.bo, E * 4);
  float* ln = (float*)(im.data() + L::LNP);
  if (p.n1w && p.n1b) { memcpy(ln, p.n1w, E * 4); memcpy(ln + E, p.n1b, E * 4); }
  auto bias_accumulators = [&]() {   // accumulators start at ITA_ACC_BIAS + bias (ita_device.h: scale_clamp_b)
    for (int i = 0; i < L::NBIAS; ++i) bias[i] = (int32_t)((uint32_t)bias[i] + (uint32_t)ITA_ACC_BIAS);
  };
  if constexpr (FFN) {
    natural(L::W12G ? L::GW1 : L::W1, p.w1, F, E);
    fragment(L::W12G ? L::GW2 : L::W2, p.w2, 4, F);
    memcpy(bias + 3 * P + E, p.b1, F * 4); memcpy(bias + 3 * P + E + F, p.b2, E * 4);
    memcpy(ln + 2 * E, p.n2w, E * 4); memcpy(ln + 3 * E, p.n2b, E * 4);
  }
  if constexpr (TOK) {
    memcpy(ln + 4 * E, p.tlw, E * 4); memcpy(ln + 5 * E, p.tlb, E * 4);
    build_tok_tab<E>(p.conv_w, p.conv_b, im.data() + L::CW);
    int32_t* tap = (int32_t*)(im.data() + L::TAP);
    for (int t = 0; t < 52; ++t) tap[t] = t < 49 ? (t / 7) * 96 + (t % 7) : 0;
  }
  bias_accumulators();
  {
    int32_t* vb4 = (int32_t*)(im.data() + L::VB4);
    for (int d = 0; d < P; ++d)
      for (int i = 0; i < 4; ++i) vb4[4 * d + i] = bias[2 * P + d];
  }
  HIPCHK(hipMalloc(d_out, im.size()));
  HIPCHK(hipMemcpy(*d_out, im.data(), im.size(), hipMemcpyHostToDevice));
  return ITA_OK;
}

// The stream kernels read an int32 accumulator as the float 1.5 * 2^23 + sum, which is exact while |sum| < 2^22.
// Worst case of a Linear row: sum_k |w| * 128 + |bias| (inputs are int8 codes).  QK^T (192 * 128 * 128) and A.V
// (<= 255 * 128) are inside the range by construction.  A blob outside it runs on the block kernels instead.
bool stream_range_ok(const StreamHostParams& p, int E, bool ffn, const float* ascal, const float* fscal) {
  // ... and the requantised value travels as a 16-bit integer between the rounding and the u8 saturation
  // (ita_device.h: rq_pack16_v3), so |acc * mult| + 128 has to stay below 2^15 as well: same worst case times the multiplier.
  auto rows_ok = [](const int8_t* w, const int32_t* b, int rows, int k, float mult) {
    if (!(mult > 0.0f)) return false;
    for (int r = 0; r < rows; ++r) {
      long long sum = 0;
      for (int i = 0; i < k; ++i) sum += w[(size_t)r * k + i] < 0 ? -(long long)w[(size_t)r * k + i] : w[(size_t)r * k + i];
      const long long bb = b[r] < 0 ? -(long long)b[r] : b[r];
      if (sum * 128 + bb >= (1ll << 22)) return false;
      if ((double)(sum * 128 + bb) * (double)mult >= 32000.0) return false;
    }
    return true;
  };
  if (!(ascal[ITA_A_ML] > 0.0f) || 192.0 * 128 * 128 * (double)ascal[ITA_A_ML] >= 32000.0) return false;   // Q K^T
  // A V: the integer softmax's probabilities sum to at most 255 per row (each is floor(num * 255 / sum(num))), so |sum p v| <= 255 * 128
  if (!(ascal[ITA_A_MC] > 0.0f) || 255.0 * 128 * (double)ascal[ITA_A_MC] >= 32000.0) return false;
  return rows_ok(p.wq, p.bq, 192, E, ascal[ITA_A_MQ]) && rows_ok(p.wk, p.bk, 192, E, ascal[ITA_A_MK]) &&
         rows_ok(p.wv, p.bv, 192, E, ascal[ITA_A_MV]) && rows_ok(p.wo, p.bo, E, 192, ascal[ITA_A_MO]) &&
         (!ffn || (rows_ok(p.w1, p.b1, 256, E, fscal[ITA_F_M1]) && rows_ok(p.w2, p.b2, E, 256, fscal[ITA_F_M2])));
}

// Single-rounding permission of one requantisation site.  The reference computes rne(fl(acc * m)) -- two roundings; the
// fast form of the stream kernels computes fl(acc * m + magic) in one fused multiply-add -- one rounding.  They can differ
// only for an accumulator value whose exact product lies within half an ulp of a rounding tie without being one.  The set of
// accumulator values that matter is small (|acc * m| below the clamp range: a few hundred thousand integers), so it is
// simply enumerated, on the host, in the arithmetic the GPU instructions perform (IEEE f32 multiply, add and fma; this file
// is compiled with -ffp-contract=off): a site is fast only if no value differs after the clamp.
bool fast_site_ok(float m) {
  if (!(m > 0.0f) || !(m < 1.0f)) return false;
  const double lim = 130.0 / (double)m;
  if (lim > 4.0e6) return false;   // outside the biased-float accumulator range: not a stream-kernel blob anyway
  const long long A = (long long)lim + 2;
  auto code = [](float t) {        // low 16 bits of the pattern = r + 128 (two's complement), then the u8 saturation
    unsigned u;
    memcpy(&u, &t, 4);
    const int v = (int)(int16_t)(u & 0xffffu);
    return v < 0 ? 0 : v > 255 ? 255 : v;
  };
  for (long long a = -A; a <= A; ++a) {
    const float x = (float)a;
    const float y = x * m;
    if (code(y + ITA_MAGIC128_F) != code(fmaf(x, m, ITA_MAGIC128_F))) return false;
  }
  return true;
}
unsigned fast_sites_of(const float* ascal) {
  unsigned mask = 0;
  const int idx[6] = {ITA_A_MQ, ITA_A_MK, ITA_A_MV, ITA_A_ML, ITA_A_MC, ITA_A_MO};
  for (int i = 0; i < 6; ++i)
    if (fast_site_ok(ascal[idx[i]])) mask |= 1u << i;   // bit order = ITA_SITE_Q, _K, _V, _L, _C, _O
  return mask;
}

struct StreamIo {
  const int8_t* xq = nullptr;   // int8 in / int8 out attention block (mode 2)
  int8_t* yq = nullptr;
  const float* x = nullptr;
  float* y = nullptr;
  _Float16 *y_hi = nullptr, *y_lo = nullptr;
  float* x1_tap = nullptr;
  unsigned long long* stamps = nullptr;
  const float* h0_src = nullptr;
  float* h0_dst = nullptr;
  const int* slots = nullptr;
  const void* img = nullptr;   // u8 wire frames: tokenizer fused in front (x unused)
  float* tok_tap = nullptr;
};

// mode 0: whole encoder layer; 1: attention block only (fuse_ln: + residual + LayerNorm1)
int launch_stream(ita_context* c, int layer, int mode, bool fuse_ln, const StreamIo& io, int B, hipStream_t s) {
  const Layer& L = c->layers[layer];
  if (L.attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): it has no int8 stream kernel");
  ItaStreamArgs a{};
  a.x = io.x; a.y = io.y; a.y_hi = io.y_hi; a.y_lo = io.y_lo; a.ld_planes = c->ldfold; a.x1_tap = io.x1_tap;
  a.inv_sx = L.ascal[ITA_A_INV_SX]; a.mq = L.ascal[ITA_A_MQ]; a.mk = L.ascal[ITA_A_MK]; a.mv = L.ascal[ITA_A_MV];
  a.ml = L.ascal[ITA_A_ML]; a.mc = L.ascal[ITA_A_MC]; a.mo = L.ascal[ITA_A_MO]; a.so = L.ascal[ITA_A_SO];
  a.f_inv_sx = L.fscal[ITA_F_INV_SX]; a.m1 = L.fscal[ITA_F_M1]; a.m2 = L.fscal[ITA_F_M2]; a.s2 = L.fscal[ITA_F_S2];
  a.B = B; a.fuse_ln = fuse_ln ? 1 : 0;
  a.stamps = io.stamps; a.h0_src = io.h0_src; a.h0_dst = io.h0_dst; a.slots = io.slots;
  a.img = io.img; a.tok_tap = io.tok_tap; a.xq = io.xq; a.yq = io.yq;
  a.fast_sites = L.fast_sites;
  const int grid = B < c->num_cus ? B : c->num_cus;
  const bool fast = L.fast_sites == ITA_SITES_ALL;   // the single-rounding instantiation: all six sites proven (fast_site_ok)
#define ITA_LAUNCH_STREAM(E_, FFN_, TOK_, IO8_)                                                                                   \
  do {                                                                                                                            \
    if (fast) hipLaunchKernelGGL((ita_stream_kernel<E_, FFN_, TOK_, false, IO8_, true>), dim3(grid), dim3(512),                     \
                                 (ItaStreamLds<E_, FFN_, (TOK_) != 0>::TOTAL), s, a);                                              \
    else hipLaunchKernelGGL((ita_stream_kernel<E_, FFN_, TOK_, false, IO8_, false>), dim3(grid), dim3(512),                         \
                            (ItaStreamLds<E_, FFN_, (TOK_) != 0>::TOTAL), s, a);                                                   \
  } while (0)
  if (mode == 2) {
    if (!L.simg_mha) return fail(ITA_ERR_UNSUPPORTED, "this layer has no attention image (accumulator range)");
    a.image = L.simg_mha;
    if (c->hdr.E == 64) ITA_LAUNCH_STREAM(64, false, 0, true);
    else ITA_LAUNCH_STREAM(128, false, 0, true);
  } else if (mode == 1) {
    if (!L.simg_mha) return fail(ITA_ERR_BAD_BLOB, "attention image missing");
    if (fuse_ln && !L.n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
    a.image = L.simg_mha;
    if (c->hdr.E == 64) ITA_LAUNCH_STREAM(64, false, 0, false);
    else ITA_LAUNCH_STREAM(128, false, 0, false);
  } else if (io.img) {
    if (!L.simg_tok) return fail(ITA_ERR_BAD_BLOB, "tokenizer / LayerNorm parameters missing from the blob");
    a.image = L.simg_tok;
    if (io.stamps) hipLaunchKernelGGL((ita_stream_kernel<64, true, 1, true>), dim3(grid), dim3(512), (ItaStreamLds<64, true, true>::TOTAL), s, a);
    else ITA_LAUNCH_STREAM(64, true, 1, false);
  } else {
    if (!L.simg_enc) return fail(ITA_ERR_BAD_BLOB, "LayerNorm parameters missing from the blob");
    a.image = L.simg_enc;
    if (c->hdr.E == 128) {   // attention + FFN of an E = 128 layer in one launch; fc1 / fc2 weights are read from the global image
      if (io.stamps) return fail(ITA_ERR_UNSUPPORTED, "phase stamps are built for the E = 64 encoder");
      ITA_LAUNCH_STREAM(128, true, 0, false);
    } else if (io.stamps) hipLaunchKernelGGL((ita_stream_kernel<64, true, 0, true>), dim3(grid), dim3(512), (ItaStreamLds<64, true, false>::TOTAL), s, a);
    else ITA_LAUNCH_STREAM(64, true, 0, false);
  }
#undef ITA_LAUNCH_STREAM
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

int launch_mha_stream(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s) {
  StreamIo io;
  io.x = x; io.y = y;
  return launch_stream(c, layer, 1, fuse, io, B, s);
}

// One encoder layer: the stream kernel (ita_stream_kernel.h) when the layer has an LDS image -- E = 64 and every
// accumulator provably inside the biased-float range (stream_range_ok) -- else the two block kernels through bufB.
// A float-FFN layer (ITAW0002) is always two launches: the attention block with the fused residual + LayerNorm1 into bufB
// (stream kernel mode 1, or ita_mha_kernel for a layer without an attention image), then ita_ffn_f32_kernel; `mid`, when
// given, runs between the two (the profiler's stage-2 mark).  A float layer (ITAW0003) is the same two launches with
// ita_attn_f32_kernel as the first.
int launch_encoder(ita_context* c, int layer, const float* x, float* y, _Float16* y_hi, _Float16* y_lo, float* x1_tap,
                   int B, hipStream_t s, unsigned long long* stamps = nullptr, const float* h0_src = nullptr,
                   float* h0_dst = nullptr, const int* slots = nullptr, const void* img = nullptr,
                   float* tok_tap = nullptr, const std::function<int()>* mid = nullptr) {
  const Layer& L = c->layers[layer];
  if (!L.n1w || !L.n2w) return fail(ITA_ERR_BAD_BLOB, "LayerNorm parameters missing from the blob");
  if (L.ffn_f32) {
    if (img || stamps) return fail(ITA_ERR_UNSUPPORTED, "a float-FFN layer runs behind the stand-alone tokenizer, without stamps");
    if (c->hdr.E != 64 && !L.w1p) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN of an ITAW0002 blob is built for E = 64");
    int rc = ensure_workspace(c, B, s);
    if (rc) return rc;
    if ((rc = L.attn_f32 ? launch_attn_f32(c, layer, x, c->bufB, B, true, s)
                         : launch_mha(c, layer, x, c->bufB, B, true, nullptr, s))) return rc;
    if (x1_tap) HIPCHK(hipMemcpyAsync(x1_tap, c->bufB, sizeof(float) * (size_t)B * 128 * c->hdr.E, hipMemcpyDeviceToDevice, s));
    if (mid && (rc = (*mid)())) return rc;
    return launch_ffn_f32(c, layer, c->bufB, y, B, true, s, y_hi, y_lo, h0_src, h0_dst, slots);
  }
  if (img ? L.simg_tok != nullptr : L.simg_enc != nullptr) {
    StreamIo io;
    io.x = x; io.y = y; io.y_hi = y_hi; io.y_lo = y_lo; io.x1_tap = x1_tap; io.stamps = stamps;
    io.h0_src = h0_src; io.h0_dst = h0_dst; io.slots = slots; io.img = img; io.tok_tap = tok_tap;
    return launch_stream(c, layer, 0, false, io, B, s);
  }
  if (img) return fail(ITA_ERR_INVALID_ARG, "launch_encoder: frames need the tokenizer image");
  // (everything that can refuse is checked before the first launch: no partial work is left behind an error)
  if (h0_dst && slots) return fail(ITA_ERR_UNSUPPORTED, "slot-indexed state needs the stream kernel (this blob's accumulator range rules it out)");
  int rc = ensure_workspace(c, B, s);
  if (rc) return rc;
  if ((rc = launch_mha(c, layer, x, c->bufB, B, true, nullptr, s))) return rc;
  if (x1_tap) HIPCHK(hipMemcpyAsync(x1_tap, c->bufB, sizeof(float) * (size_t)B * 128 * c->hdr.E, hipMemcpyDeviceToDevice, s));
  if (h0_dst)   // the side copy the stream kernel makes for the LSTM
    HIPCHK(hipMemcpyAsync(h0_dst, h0_src, sizeof(float) * (size_t)B * 128, hipMemcpyDeviceToDevice, s));
  return launch_ffn(c, layer, c->bufB, y, B, true, nullptr, s, y_hi, y_lo);
}

// frames into the E = 64 model: the tokenizer runs inside the first encoder layer's kernel
// (ITA_SPLIT_TOKENIZER=1 keeps the separate ita_tok_stream_kernel launch, for comparison)
bool fuse_tokenizer(const ita_context* c, int image_dtype) {
  static const bool split = getenv("ITA_SPLIT_TOKENIZER") != nullptr;
  // f32 frames go through the stand-alone tokenizer: the stream kernel's private pixel windows are sized for bytes
  return !split && image_dtype == ITA_IMAGE_U8 && !c->layers.empty() && c->layers[0].simg_tok;
}

int launch_tokenizer(ita_context* c, const void* img, int dtype, float* tokens, int B, hipStream_t s) {
  // (the image exists when the blob has the conv weights and bias and the LayerNorm: ita_load_weights)
  if (!c->tok_simg) return fail(ITA_ERR_BAD_BLOB, "tokenizer parameters missing from the blob");
  const bool u8 = dtype == ITA_IMAGE_U8;
  ItaTokStreamArgs ta{c->tok_simg + (u8 ? 0 : c->tok_simg_bytes), img, tokens, B};
  const int g = B < 2 * c->num_cus ? B : 2 * c->num_cus;   // 35 KB of LDS, <= 128 registers: two workgroups per CU
  if (c->hdr.E == 64) {
    if (u8) hipLaunchKernelGGL((ita_tok_stream_kernel<64, true>), dim3(g), dim3(512), (ItaTokStreamLds<64, true>::TOTAL), s, ta);
    else hipLaunchKernelGGL((ita_tok_stream_kernel<64, false>), dim3(g), dim3(512), (ItaTokStreamLds<64, false>::TOTAL), s, ta);
  } else {
    if (u8) hipLaunchKernelGGL((ita_tok_stream_kernel<128, true>), dim3(g), dim3(512), (ItaTokStreamLds<128, true>::TOTAL), s, ta);
    else hipLaunchKernelGGL((ita_tok_stream_kernel<128, false>), dim3(g), dim3(512), (ItaTokStreamLds<128, false>::TOTAL), s, ta);
  }
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

int launch_tail(ita_context* c, const float* x, float* feat, int ld, int B, hipStream_t s) {
  if (!c->tail_wT) return fail(ITA_ERR_BAD_BLOB, "fusion-tail parameters missing from the blob");
  if (c->hdr.E != 64) return fail(ITA_ERR_UNSUPPORTED, "fusion tail is built for E = 64 (ITAViTLSTM)");
  ItaTailArgs a{x, c->tail_wT, c->tail_b, feat, ld, B};
  const int grid = B < 2 * c->num_cus ? B : 2 * c->num_cus;
  hipLaunchKernelGGL(ita_tail_kernel<64>, dim3(grid), dim3(256), ita_tail_lds_bytes<64>(), s, a);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

int launch_gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N,
                int K, hipStream_t s) {
  if (N % 64 || K % 32) return fail(ITA_ERR_UNSUPPORTED, "gemm needs N % 64 == 0 and K % 32 == 0");
  ItaGemmArgs g{A, lda, W, ldw, bias, C, ldc, M, N, K};
  hipLaunchKernelGGL(ita_gemm_f32_kernel, dim3(N / 64, (M + 31) / 32), dim3(256), 0, s, g);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

template <int NT, int WAVES, int TPS>
int launch_tail_big_w(const ItaTailBigArgs& a, hipStream_t s) {
  // the attribute is per DEVICE: one bit per ordinal (a process-wide flag left the second GPU's context without it).
  // Lock-free on the launch path: the mutex is only taken by the first launch on a device.
  static std::mutex mu;
  static std::atomic<uint64_t> attr_set{0};
  auto kern = ita_tail_big_kernel<NT, WAVES, TPS>;
  constexpr int lds_bytes = ItaTailBigLds<NT, WAVES, TPS>::TOTAL;
  {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
      std::lock_guard<std::mutex> g(mu);
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
      attr_set.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(kern, dim3(2 * a.TW / 32, 2 * a.TH / (2 * WAVES), a.B), dim3(64 * WAVES), lds_bytes, s, a);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}
// 16-row tiles on 8 waves with a whole chunk's weights resident when the map height allows (measured best:
// 0.61 ms for 32 frames of BASELINE config 5); else 8-row tiles on 4 waves with a third of the chunk's taps
// resident (70 KB of LDS, two workgroups per CU: 0.66 ms).
template <int NT>
int launch_tail_big(const ItaTailBigArgs& a, hipStream_t s) {
  if ((2 * a.TH) % 16 != 0) return launch_tail_big_w<NT, 4, 3>(a, s);
  return launch_tail_big_w<NT, 8, 9>(a, s);
}

template <int BM, int BN, int WM, int WN>
int launch_gemm_split(const _Float16* a_hi, const _Float16* a_lo, int lda, const _Float16* w_hi, const _Float16* w_lo,
                      int ldw, float* out, int M, int N, int K, int nsplit, hipStream_t s, const _Float16* wf_hi = nullptr,
                      const _Float16* wf_lo = nullptr) {
  if (N % BN || K % (64 * nsplit)) return fail(ITA_ERR_UNSUPPORTED, "split gemm shape");
  static const int dbg = getenv("ITA_GEMM_DBG") ? atoi(getenv("ITA_GEMM_DBG")) : 0;
  ItaGemmSplitArgs g{a_hi, a_lo, lda, w_hi, w_lo, ldw, out, M, N, K, nsplit, dbg, wf_hi, wf_lo};
  if (M <= 32 && N % 32 == 0 && wf_hi && wf_lo) {   // one M tile: one wave per 32 x 32 tile and K slice
    hipLaunchKernelGGL(ita_gemm_f16x3_tiny_kernel, dim3(N / 32, 1, nsplit), dim3(64), 0, s, g);
    HIPCHK(hipGetLastError());
    return ITA_OK;
  }
  if (M <= 256 && N % 32 == 0) {   // a few M tiles: four-wave workgroups share the staging, same arithmetic
    // M tiles per workgroup: up to four (128 frames: 128 workgroups).  Fewer tiles per workgroup fill the chip -- MT = ceil(M / 64)
    // gives 256 workgroups from 64 frames on and the kernel alone gets 1.4-2.9 us faster (64 / 128 frames, one stream) -- but in
    // the three-branch graph schedule that bench.py uses at these sizes a 256-workgroup GEMM leaves no CU to the LSTM branch
    // and the step gets SLOWER (128 frames: 36.6 -> 38.3 us).  Per output element the arithmetic does not depend on MT.
    const int mt = M >= 128 ? 4 : (M + 31) / 32;
    const dim3 grid((N / 32) * nsplit, (M + 32 * mt - 1) / (32 * mt));
    switch (mt) {
      case 1: hipLaunchKernelGGL(ita_gemm_f16x3_small_kernel<1>, grid, dim3(256), ita_gemm_small_lds(1), s, g); break;
      case 2: hipLaunchKernelGGL(ita_gemm_f16x3_small_kernel<2>, grid, dim3(256), ita_gemm_small_lds(2), s, g); break;
      case 3: hipLaunchKernelGGL(ita_gemm_f16x3_small_kernel<3>, grid, dim3(256), ita_gemm_small_lds(3), s, g); break;
      default: hipLaunchKernelGGL(ita_gemm_f16x3_small_kernel<4>, grid, dim3(256), ita_gemm_small_lds(4), s, g); break;
    }
    HIPCHK(hipGetLastError());
    return ITA_OK;
  }
  constexpr int lds_bytes = ItaGemmSplitLds<BM, BN>::TOTAL;
  auto kern = ita_gemm_f16x3_kernel<BM, BN, WM, WN>;
  hipLaunchKernelGGL(kern, dim3((N / BN) * ((M + BM - 1) / BM) * nsplit), dim3(64 * WM * WN), lds_bytes, s, g);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

uint16_t float_to_half(float f);
float half_to_float(uint16_t hbits);

// hi/lo f16 planes of w * 2^e, e chosen so that max|w| * 2^e lies in [512, 1024)
int split_upload(const std::vector<float>& w, _Float16** d_hi, _Float16** d_lo, float* inv_scale) {
  float mx = 0.0f;
  for (float v : w) mx = fabsf(v) > mx ? fabsf(v) : mx;
  int e = 0;
  if (mx > 0.0f) {
    int ex;
    frexpf(mx, &ex);       // mx = m * 2^ex, m in [0.5, 1)
    e = 10 - ex;
  }
  const float sc = ldexpf(1.0f, e);
  *inv_scale = ldexpf(1.0f, -e);
  std::vector<uint16_t> hi(w.size()), lo(w.size());
  for (size_t i = 0; i < w.size(); ++i) {
    const float v = w[i] * sc;
    hi[i] = float_to_half(v);
    lo[i] = float_to_half(v - half_to_float(hi[i]));
  }
  HIPCHK(hipMalloc(d_hi, w.size() * 2));
  HIPCHK(hipMalloc(d_lo, w.size() * 2));
  HIPCHK(hipMemcpy(*d_hi, hi.data(), w.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(*d_lo, lo.data(), w.size() * 2, hipMemcpyHostToDevice));
  return ITA_OK;
}

int launch_tail(ita_context* c, const float* x, float* feat, int ld, int B, hipStream_t s);
int launch_gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N,
                int K, hipStream_t s);

// Folds PixelShuffle/Upsample/concat/conv3x3 and the decoder Linear into Wfold[512][K] (K = 128 E) by pushing unit
// impulses through the exact f32 kernels (bias-free), and dec(tail(0)) as the bias.  Without a fusion tail
// (models/ITA/QAT/model.py:80-81: the decoder reads the flattened tokens) Wfold is the decoder matrix itself.
int build_fold(ita_context* c) {
  const int CH = 1024, KFOLD = c->kfold, LDFOLD = c->ldfold;
  const bool has_tail = c->hdr.has_tail != 0;
  float *imp = nullptr, *feat = nullptr, *mt = nullptr, *zero = nullptr;
  HIPCHK(hipMalloc(&imp, sizeof(float) * (size_t)(has_tail ? CH : 512) * KFOLD));
  HIPCHK(hipMalloc(&feat, sizeof(float) * (size_t)CH * 4608));
  HIPCHK(hipMalloc(&mt, sizeof(float) * (size_t)KFOLD * 512));
  HIPCHK(hipMalloc(&zero, sizeof(float) * 16));
  HIPCHK(hipMemset(zero, 0, sizeof(float) * 16));
  int rc = ITA_OK;
  std::vector<float> hmt((size_t)KFOLD * 512), hb(512);
  if (has_tail) {
    const float* real_cb = c->tail_b;
    c->tail_b = zero;                       // bias-free pass: column i of Wfold = dec_nobias(tail_nobias(e_i))
    for (int c0 = 0; c0 < KFOLD && !rc; c0 += CH) {
      const size_t n = (size_t)CH * KFOLD;
      hipLaunchKernelGGL(ita_impulse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, imp, CH, KFOLD, c0);
      if ((rc = launch_tail(c, imp, feat, 4608, CH, nullptr))) break;
      rc = launch_gemm(feat, 4608, c->dec_w, 4608, nullptr, mt + (size_t)c0 * 512, 512, CH, 512, 4608, nullptr);
    }
    c->tail_b = real_cb;
    if (!rc) {
      // bias' = dec(tail(0)) with the real biases
      HIPCHK(hipMemset(imp, 0, sizeof(float) * KFOLD));
      if (!(rc = launch_tail(c, imp, feat, 4608, 1, nullptr)))
        rc = launch_gemm(feat, 4608, c->dec_w, 4608, c->dec_b, imp, 512, 1, 512, 4608, nullptr);
    }
    if (!rc) {
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipMemcpy(hb.data(), imp, 512 * sizeof(float), hipMemcpyDeviceToHost));
    }
  } else {
    // Wfold^T[k][n] = dec_w[n][k]: transposed on the host (once, at load time); bias' = the decoder bias
    const float *dw = hptr<float>(c, "dec.w"), *db = hptr<float>(c, "dec.b");
    for (int n = 0; n < 512; ++n)
      for (int k = 0; k < KFOLD; ++k) hmt[(size_t)k * 512 + n] = dw[(size_t)n * KFOLD + k];
    HIPCHK(hipMemcpy(mt, hmt.data(), hmt.size() * sizeof(float), hipMemcpyHostToDevice));
    memcpy(hb.data(), db, 512 * sizeof(float));
  }
  if (!rc) {
    // one fold further: the decoder output feeds only LSTM layer 0, so
    //   G0^T[k][j] = sum_n Wfold^T[k][n] * W_ih0[j][n]        (wcat[0] holds W_ih0 in its first 517 columns)
    // computed with the exact f32 GEMM; the buffer that held the impulses is reused for the result
    rc = launch_gemm(mt, 512, c->wcat[0], K0P, nullptr, imp, 512, KFOLD, 512, 512, nullptr);
  }
  if (!rc) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(hmt.data(), imp, hmt.size() * sizeof(float), hipMemcpyDeviceToHost));
  }
  (void)hipFree(imp); (void)hipFree(feat); (void)hipFree(mt); (void)hipFree(zero);
  if (rc) return rc;
  // rows of the GEMM weight in the permuted gate order r' = ut*32 + gate*8 + u (ita_lstm_head_kernel)
  std::vector<float> wf((size_t)512 * LDFOLD, 0.0f);
  for (int rp = 0; rp < 512; ++rp) {
    const int j = ((rp >> 3) & 3) * 128 + (rp >> 5) * 8 + (rp & 7);
    for (int k = 0; k < KFOLD; ++k) wf[(size_t)rp * LDFOLD + k] = hmt[(size_t)k * 512 + j];
  }
  if ((rc = split_upload(wf, &c->fold_hi, &c->fold_lo, &c->fold_inv_scale))) return rc;
  {
    // the same values in fragment order for ita_gemm_f16x3_tiny_kernel (same scale: max |w| is the same)
    std::vector<float> wfr((size_t)512 * KFOLD);
    for (int nt = 0; nt < 16; ++nt)
      for (int st = 0; st < KFOLD / 16; ++st)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j)
            wfr[(((size_t)nt * (KFOLD / 16) + st) * 64 + lane) * 8 + j] =
                wf[(size_t)(nt * 32 + (lane & 31)) * LDFOLD + st * 16 + 8 * (lane >> 5) + j];
    float inv2 = 0.0f;
    if ((rc = split_upload(wfr, &c->foldf_hi, &c->foldf_lo, &inv2))) return rc;
    if (inv2 != c->fold_inv_scale) return fail(ITA_ERR_UNSUPPORTED, "fragment copy of the folded weights got a different scale");
  }
  // bias'' = W_ih0[:, :512] . bias' + b_ih0 + b_hh0   (gate-major order)
  const float *wih0 = hptr<float>(c, "lstm.w_ih0"), *bih0 = hptr<float>(c, "lstm.b_ih0"), *bhh0 = hptr<float>(c, "lstm.b_hh0");
  std::vector<float> b2(512);
  for (int j = 0; j < 512; ++j) {
    double acc = (double)bih0[j] + (double)bhh0[j];
    for (int n = 0; n < 512; ++n) acc += (double)wih0[(size_t)j * 517 + n] * (double)hb[n];
    b2[j] = (float)acc;
  }
  HIPCHK(hipMalloc(&c->fold_bias, 512 * sizeof(float)));
  HIPCHK(hipMemcpy(c->fold_bias, b2.data(), 512 * sizeof(float), hipMemcpyHostToDevice));
  c->folded = true;
  return ITA_OK;
}

int dispatch_host(const uint16_t* in, uint16_t* out, bool ffn);

}  // namespace

// =============================================================================== C ABI
namespace {
template <typename T>
int launch_ingest(ita_context* c, const void* src, int H, int W, long long row_stride, long long frame_stride,
                  float depth_scale, float* frames, int batch, hipStream_t s) {
  const float scale_y = (float)H / (float)ITA_INGEST_H, scale_x = (float)W / (float)ITA_INGEST_W;   // host IEEE divisions
  const int row_bytes = W * (int)sizeof(T);
  if (W >= 2 * ITA_INGEST_W && row_bytes <= ITA_INGEST_ROW_BYTES) {
    const long long items = (long long)batch * (ITA_INGEST_H / 4);
    const int grid = (int)std::min<long long>(items, (long long)c->num_cus * 8);
    hipLaunchKernelGGL(ita_ingest_rows_kernel<T>, dim3(grid), dim3(256), ita_ingest_rows_lds_total(row_bytes), s,
                       (const T*)src, H, W, row_stride, frame_stride, scale_y, scale_x, depth_scale, frames, batch);
  } else {
    const long long blocks = ((long long)batch * ITA_INGEST_H * ITA_INGEST_W + 255) / 256;
    const int grid = (int)std::min<long long>(blocks, (long long)c->num_cus * 8);
    hipLaunchKernelGGL(ita_ingest_gather_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)src, H, W, row_stride,
                       frame_stride, scale_y, scale_x, depth_scale, frames, batch);
  }
  HIPCHK(hipGetLastError());
  return ITA_OK;
}
}  // namespace

extern "C" {

int ita_abi_version(void) { return ITA_MI355X_ABI_VERSION; }
int ita_last_error(void) { return tl_err; }
const char* ita_error_string(void) { return tl_msg.c_str(); }

int ita_create(ita_handle* out, int device_ordinal) {
  if (!out) return fail(ITA_ERR_INVALID_ARG, "out is null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ITA_ERR_NO_DEVICE, "no HIP device visible");
  int dev = device_ordinal;
  if (dev < 0) HIPCHK(hipGetDevice(&dev));
  if (dev >= n) return fail(ITA_ERR_INVALID_ARG, "device ordinal out of range");
  HIPCHK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  ita_context* c = new ita_context();
  c->device = dev;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  int rc = ITA_OK;
  if ((rc = set_lds(ita_mha_kernel<64>, ItaMhaLds<64>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_attn_f32_kernel<64>, ItaAttnF32Lds<64>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_attn_f32_kernel<128>, ItaAttnF32Lds<128>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_ffn_f32_kernel<128>, ItaFfnF32Lds<128>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_mha_kernel<128>, ItaMhaLds<128>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_ffn_kernel<64>, ItaFfnLds<64>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_ffn_kernel<128>, ItaFfnLds<128>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_tok_stream_kernel<64, true>, ItaTokStreamLds<64, true>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_tok_stream_kernel<128, true>, ItaTokStreamLds<128, true>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_tok_stream_kernel<64, false>, ItaTokStreamLds<64, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_tok_stream_kernel<128, false>, ItaTokStreamLds<128, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_tail_kernel<64>, ita_tail_lds_bytes<64>()))) { delete c; return rc; }
  if ((rc = set_lds(ita_tail_up_kernel, ItaTailUpLds::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_long_proj_kernel<false>, ItaStreamLds<128, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_long_proj_kernel<true>, ItaStreamLds<128, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_long_attn_kernel<false>, ItaLongLds::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_long_attn_kernel<true>, ItaLongLds::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, true, 1, false, false, true>, ItaStreamLds<64, true, true>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, true, 0, false, false, true>, ItaStreamLds<64, true, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, false, 0, false, false, true>, ItaStreamLds<64, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<128, false, 0, false, false, true>, ItaStreamLds<128, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<128, true, 0, false, false, true>, ItaStreamLds<128, true, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, false, 0, false, true, true>, ItaStreamLds<64, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<128, false, 0, false, true, true>, ItaStreamLds<128, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, true, 1>, ItaStreamLds<64, true, true>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, true, 0>, ItaStreamLds<64, true, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, true, 1, true>, ItaStreamLds<64, true, true>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, true, 0, true>, ItaStreamLds<64, true, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, false, 0>, ItaStreamLds<64, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<128, false, 0>, ItaStreamLds<128, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<128, true, 0>, ItaStreamLds<128, true, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<64, false, 0, false, true>, ItaStreamLds<64, false, false>::TOTAL))) { delete c; return rc; }
  if ((rc = set_lds(ita_stream_kernel<128, false, 0, false, true>, ItaStreamLds<128, false, false>::TOTAL))) { delete c; return rc; }
  {
    auto k1 = ita_gemm_f16x3_kernel<128, 128, 2, 4>;
    constexpr int b1 = ItaGemmSplitLds<128, 128>::TOTAL;
    if ((rc = set_lds(k1, b1))) { delete c; return rc; }
    if ((rc = set_lds(ita_gemm_f16x3_small_kernel<1>, ita_gemm_small_lds(1)))) { delete c; return rc; }
    if ((rc = set_lds(ita_gemm_f16x3_small_kernel<2>, ita_gemm_small_lds(2)))) { delete c; return rc; }
    if ((rc = set_lds(ita_gemm_f16x3_small_kernel<3>, ita_gemm_small_lds(3)))) { delete c; return rc; }
    if ((rc = set_lds(ita_gemm_f16x3_small_kernel<4>, ita_gemm_small_lds(4)))) { delete c; return rc; }
  }
  *out = c;
  return ITA_OK;
}

static void free_tail_large(ita_context* c);

int ita_destroy(ita_handle h) {
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  {
    std::lock_guard<std::mutex> g(g_bind_mu);
    if (g_bound == h) g_bound = nullptr;
  }
  (void)hipSetDevice(h->device);
  free_weights(h);
  free_workspace(h);
  for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->pipe_ev) (void)hipEventDestroy(e);
  if (h->pipe_h) (void)hipFree(h->pipe_h);
  if (h->long_ws) (void)hipFree(h->long_ws);
  if (h->dsp_in) (void)hipFree(h->dsp_in);
  if (h->dsp_out) (void)hipFree(h->dsp_out);
  free_tail_large(h);
  delete h;
  return ITA_OK;
}

int ita_load_weights(ita_handle h, const void* blob, size_t nbytes) {
  if (!h || !blob) return fail(ITA_ERR_INVALID_ARG, "null argument");
  const int ffn_kind = nbytes < sizeof(ita_blob_header) ? -1 : ita_blob_ffn_kind(blob, nbytes);
  const int attn_kind = nbytes < sizeof(ita_blob_header) ? -1 : ita_blob_attn_kind(blob, nbytes);
  if (ffn_kind < 0 || attn_kind < 0) return fail(ITA_ERR_BAD_BLOB, "not an ITAW0001 / ITAW0002 / ITAW0003 blob");
  HIPCHK(hipSetDevice(h->device));
  ita_blob_header hdr;
  memcpy(&hdr, blob, sizeof hdr);
  if (hdr.n_tensors < 0 || sizeof(hdr) + (size_t)hdr.n_tensors * sizeof(ita_blob_entry) > nbytes)
    return fail(ITA_ERR_BAD_BLOB, "tensor table exceeds the blob");
  if ((hdr.E != 64 && hdr.E != 128) || hdr.S != 128 || hdr.P != 192 || hdr.F != 256 || hdr.H != 1 ||
      hdr.num_layers < 1 || hdr.num_layers > 16)
    return fail(ITA_ERR_UNSUPPORTED, "kernels are built for E in {64,128}, S=128, P=192, F=256, H=1");
  // the float graph (ITAW0003) runs at E = 64 with its fusion tail, and at E = 128 without one (ITA_upsample_shuffle)
  if (attn_kind == 1 && hdr.E != 64 && hdr.has_tail)
    return fail(ITA_ERR_UNSUPPORTED, "the float32 graph's fusion tail (ITAW0003) is built for E = 64; at E = 128 it runs without one");
  if (attn_kind == 0 && ffn_kind == 1 && hdr.E != 64) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN (ITAW0002) is built for E = 64");
  {
    const ita_blob_entry* e = (const ita_blob_entry*)((const char*)blob + sizeof(hdr));
    for (int i = 0; i < hdr.n_tensors; ++i)
      if (e[i].offset < 0 || e[i].nbytes < 0 || (size_t)e[i].offset + (size_t)e[i].nbytes > nbytes ||
          (e[i].offset & 15))
        return fail(ITA_ERR_BAD_BLOB, "tensor out of bounds or misaligned");
  }
  {
    char bad[32];
    const int v = ita_blob_validate(blob, nbytes, bad);
    if (v) return fail(ITA_ERR_BAD_BLOB, std::string(v == -2 ? "required tensor missing: " : v == -3 ? "tensor has the wrong dtype or size: " : "malformed blob ") + bad);
  }
  free_weights(h);
  free_workspace(h);
  h->hdr = hdr;
  h->hblob.assign((const char*)blob, (const char*)blob + nbytes);
  HIPCHK(hipMalloc(&h->dblob, nbytes));
  HIPCHK(hipMemcpy(h->dblob, blob, nbytes, hipMemcpyHostToDevice));
  bool ok = true;
  h->layers.assign(hdr.num_layers, Layer{});
  char nm[40];
  auto expect = [&](const char* name, size_t bytes) {
    const ita_blob_entry* e = ita_blob_find(h->hblob.data(), h->hblob.size(), name);
    if (e && (size_t)e->nbytes != bytes) ok = false;
  };
  const size_t E = hdr.E, P = hdr.P, F = hdr.F;
  for (int i = 0; i < hdr.num_layers; ++i) {
    Layer& L = h->layers[i];
#define NM(fmt) (snprintf(nm, sizeof nm, fmt, i), nm)
    if (attn_kind == 1) {   // float32 attention (sizes checked by ita_blob_validate)
      L.attn_f32 = true;
      L.wqf = dptr<float>(h, NM("attn%d.wqf"), true, &ok); L.wkf = dptr<float>(h, NM("attn%d.wkf"), true, &ok);
      L.wvf = dptr<float>(h, NM("attn%d.wvf"), true, &ok); L.bqf = dptr<float>(h, NM("attn%d.bqf"), true, &ok);
      L.bkf = dptr<float>(h, NM("attn%d.bkf"), true, &ok); L.bvf = dptr<float>(h, NM("attn%d.bvf"), true, &ok);
      L.wof = dptr<float>(h, NM("attn%d.wof"), true, &ok); L.bof = dptr<float>(h, NM("attn%d.bof"), true, &ok);
    } else {
      expect(NM("attn%d.wq"), P * E); expect(NM("attn%d.wo"), E * P); expect(NM("attn%d.bq"), P * 4);
      expect(NM("attn%d.bo"), E * 4); expect(NM("attn%d.scal"), ITA_A_NSCAL * 4);
      L.wq = dptr<int8_t>(h, NM("attn%d.wq"), true, &ok); L.wk = dptr<int8_t>(h, NM("attn%d.wk"), true, &ok);
      L.wv = dptr<int8_t>(h, NM("attn%d.wv"), true, &ok); L.wo = dptr<int8_t>(h, NM("attn%d.wo"), true, &ok);
      L.bq = dptr<int32_t>(h, NM("attn%d.bq"), true, &ok); L.bk = dptr<int32_t>(h, NM("attn%d.bk"), true, &ok);
      L.bv = dptr<int32_t>(h, NM("attn%d.bv"), true, &ok); L.bo = dptr<int32_t>(h, NM("attn%d.bo"), true, &ok);
      const float* as = hptr<float>(h, NM("attn%d.scal"));
      if (!as) { ok = false; break; }
      memcpy(L.ascal, as, sizeof L.ascal);
    }
    if (ffn_kind == 1) {   // float32 FFN (sizes checked by ita_blob_validate)
      L.ffn_f32 = true;
      L.w1f = dptr<float>(h, NM("ffn%d.w1f"), true, &ok); L.b1f = dptr<float>(h, NM("ffn%d.b1f"), true, &ok);
      L.w2f = dptr<float>(h, NM("ffn%d.w2f"), true, &ok); L.b2f = dptr<float>(h, NM("ffn%d.b2f"), true, &ok);
      const float *w1 = hptr<float>(h, NM("ffn%d.w1f")), *w2 = hptr<float>(h, NM("ffn%d.w2f"));
      if (E == 128 && w1 && w2) {   // ita_ffn_f32_kernel<128> streams W1 / W2 as B-fragment images
        std::vector<float> img(F * E);
        float** dst[2] = {&L.w1p, &L.w2p};
        for (int m = 0; m < 2; ++m) {
          if (m == 0) ita_ffn_f32_frag_image(w1, (int)F, (int)E, img.data());
          else ita_ffn_f32_frag_image(w2, (int)E, (int)F, img.data());
          if (hipMalloc(dst[m], img.size() * sizeof(float)) != hipSuccess ||
              hipMemcpy(*dst[m], img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            free_weights(h);
            return fail(ITA_ERR_HIP, "uploading the float32 FFN fragment images failed");
          }
        }
      }
    } else {
      expect(NM("ffn%d.w1"), F * E); expect(NM("ffn%d.w2"), E * F); expect(NM("ffn%d.scal"), ITA_F_NSCAL * 4);
      L.w1 = dptr<int8_t>(h, NM("ffn%d.w1"), true, &ok); L.w2 = dptr<int8_t>(h, NM("ffn%d.w2"), true, &ok);
      L.b1 = dptr<int32_t>(h, NM("ffn%d.b1"), true, &ok); L.b2 = dptr<int32_t>(h, NM("ffn%d.b2"), true, &ok);
      const float* fs = hptr<float>(h, NM("ffn%d.scal"));
      if (!fs) { ok = false; break; }
      memcpy(L.fscal, fs, sizeof L.fscal);
    }
    L.n1w = dptr<float>(h, NM("norm1_%d.w"), false, &ok); L.n1b = dptr<float>(h, NM("norm1_%d.b"), false, &ok);
    L.n2w = dptr<float>(h, NM("norm2_%d.w"), false, &ok); L.n2b = dptr<float>(h, NM("norm2_%d.b"), false, &ok);
#undef NM
  }
  if (!ok) { free_weights(h); return fail(ITA_ERR_BAD_BLOB, "a required block tensor is missing or mis-sized"); }
  h->tail_b = dptr<float>(h, "tail.conv_b", false, &ok);
  h->dec_w = dptr<float>(h, "dec.w", false, &ok); h->dec_b = dptr<float>(h, "dec.b", false, &ok);
  h->fc_w = dptr<float>(h, "fc.w", false, &ok); h->fc_b = dptr<float>(h, "fc.b", false, &ok);
  for (int i = 0; i < hdr.num_layers; ++i) {
    Layer& L = h->layers[i];
    if (L.attn_f32) continue;   // no int8 attention: no stream images (ita_attn_f32_kernel + ita_ffn_f32_kernel)
    StreamHostParams sp{};
#define NM(fmt) (snprintf(nm, sizeof nm, fmt, i), nm)
    sp.wq = hptr<int8_t>(h, NM("attn%d.wq")); sp.wk = hptr<int8_t>(h, NM("attn%d.wk")); sp.wv = hptr<int8_t>(h, NM("attn%d.wv"));
    sp.wo = hptr<int8_t>(h, NM("attn%d.wo")); sp.w1 = hptr<int8_t>(h, NM("ffn%d.w1")); sp.w2 = hptr<int8_t>(h, NM("ffn%d.w2"));
    sp.bq = hptr<int32_t>(h, NM("attn%d.bq")); sp.bk = hptr<int32_t>(h, NM("attn%d.bk")); sp.bv = hptr<int32_t>(h, NM("attn%d.bv"));
    sp.bo = hptr<int32_t>(h, NM("attn%d.bo")); sp.b1 = hptr<int32_t>(h, NM("ffn%d.b1")); sp.b2 = hptr<int32_t>(h, NM("ffn%d.b2"));
    sp.n1w = hptr<float>(h, NM("norm1_%d.w")); sp.n1b = hptr<float>(h, NM("norm1_%d.b"));
    sp.n2w = hptr<float>(h, NM("norm2_%d.w")); sp.n2b = hptr<float>(h, NM("norm2_%d.b"));
#undef NM
    sp.tlw = hptr<float>(h, "tok.ln_w"); sp.tlb = hptr<float>(h, "tok.ln_b");
    sp.conv_w = hptr<float>(h, "tok.conv_w"); sp.conv_b = hptr<float>(h, "tok.conv_b");
    int rc2 = ITA_OK;
    // a float-FFN layer gets the attention image only: its FFN is ita_ffn_f32_kernel (no simg_enc / simg_tok)
    const bool lns = !L.ffn_f32 && sp.n1w && sp.n1b && sp.n2w && sp.n2b && stream_range_ok(sp, hdr.E, true, L.ascal, L.fscal);
    if (!stream_range_ok(sp, hdr.E, false, L.ascal, L.fscal)) continue;   // no images: this layer runs on the block kernels
    L.fast_sites = fast_sites_of(L.ascal);
    if (hdr.E == 64) {
      rc2 = build_stream_image<64, false, false>(sp, &L.simg_mha);
      if (!rc2 && lns) rc2 = build_stream_image<64, true, false>(sp, &L.simg_enc);
      if (!rc2 && lns && i == 0 && sp.tlw && sp.tlb && sp.conv_w && sp.conv_b) rc2 = build_stream_image<64, true, true>(sp, &L.simg_tok);
    } else {
      rc2 = build_stream_image<128, false, false>(sp, &L.simg_mha);
      if (!rc2 && lns) rc2 = build_stream_image<128, true, false>(sp, &L.simg_enc);
    }
    if (rc2) { free_weights(h); return rc2; }
  }
  if (const float* cw = hptr<float>(h, "tok.conv_w")) {
    const int Ei = hdr.E;
    const float *cb = hptr<float>(h, "tok.conv_b"), *lw = hptr<float>(h, "tok.ln_w"), *lb = hptr<float>(h, "tok.ln_b");
    if (cb && lw && lb && (Ei == 64 || Ei == 128)) {   // the LDS images of ita_tok_stream_kernel<E, U8>
      // [0]: u8 frames (integer conv tables), [1]: f32 frames (f32 MFMA A fragments); each padded to the larger of the two
      const int nct = Ei / 16;
      const size_t one8 = Ei == 64 ? (size_t)ItaTokStreamLds<64, true>::IMAGE : (size_t)ItaTokStreamLds<128, true>::IMAGE;
      const size_t onef = Ei == 64 ? (size_t)ItaTokStreamLds<64, false>::IMAGE : (size_t)ItaTokStreamLds<128, false>::IMAGE;
      const size_t one = ((one8 > onef ? one8 : onef) + 15) & ~(size_t)15;
      std::vector<char> im(2 * one, 0);
      {
        char* b0 = im.data();
        memcpy(b0, lw, Ei * 4); memcpy(b0 + Ei * 4, lb, Ei * 4);
        int off_tap;
        if (Ei == 64) { build_tok_tab<64>(cw, cb, b0 + ItaTokStreamLds<64, true>::CW); off_tap = ItaTokStreamLds<64, true>::TAP; }
        else { build_tok_tab<128>(cw, cb, b0 + ItaTokStreamLds<128, true>::CW); off_tap = ItaTokStreamLds<128, true>::TAP; }
        int32_t* tap = (int32_t*)(b0 + off_tap);
        for (int t = 0; t < 52; ++t) tap[t] = t < 49 ? (t / 7) * 96 + (t % 7) : 0;
      }
      {
        char* b0 = im.data() + one;
        const int off_cw = 2 * Ei * 4, off_cb = off_cw + 13 * nct * 64 * 4, off_tap = off_cb + Ei * 4;
        memcpy(b0, lw, Ei * 4); memcpy(b0 + Ei * 4, lb, Ei * 4);
        float* cwf = (float*)(b0 + off_cw);
        for (int st = 0; st < 13; ++st)
          for (int ct = 0; ct < nct; ++ct)
            for (int lane = 0; lane < 64; ++lane) {
              const int t = 4 * st + (lane >> 4), rho = lane & 15, ch = (Ei / 4) * (rho >> 2) + 4 * ct + (rho & 3);
              cwf[(st * nct + ct) * 64 + lane] = t < 49 ? cw[(size_t)ch * 49 + t] : 0.0f;
            }
        memcpy(b0 + off_cb, cb, Ei * 4);
        int32_t* tap = (int32_t*)(b0 + off_tap);
        for (int t = 0; t < 52; ++t) tap[t] = t < 49 ? (t / 7) * 96 + (t % 7) : 0;
      }
      h->tok_simg_bytes = one;
      HIPCHK(hipMalloc(&h->tok_simg, im.size()));
      HIPCHK(hipMemcpy(h->tok_simg, im.data(), im.size(), hipMemcpyHostToDevice));
    }
  }
  // derived: conv3x3 weights re-laid [c][ky][kx][o -> 12] so one tap's 9 output weights are contiguous
  if (const float* cw = hptr<float>(h, "tail.conv_w")) {
    const int cin = hdr.E / 4 + hdr.E;
    std::vector<float> wT((size_t)cin * 9 * 12, 0.0f);
    for (int o = 0; o < 9; ++o)
      for (int c = 0; c < cin; ++c)
        for (int k = 0; k < 9; ++k) wT[((size_t)c * 9 + k) * 12 + o] = cw[((size_t)o * cin + c) * 9 + k];
    HIPCHK(hipMalloc(&h->tail_wT, wT.size() * sizeof(float)));
    HIPCHK(hipMemcpy(h->tail_wT, wT.data(), wT.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  // derived: LSTM [W_ih | W_hh] concatenated along k (layer 0 zero padded to K0P), b_ih + b_hh
  if (hptr<float>(h, "lstm.w_ih0")) {
    for (int l = 0; l < 3; ++l) {
      char a[32], b[32], ci[32], d[32];
      snprintf(a, sizeof a, "lstm.w_ih%d", l); snprintf(b, sizeof b, "lstm.w_hh%d", l);
      snprintf(ci, sizeof ci, "lstm.b_ih%d", l); snprintf(d, sizeof d, "lstm.b_hh%d", l);
      const float *wih = hptr<float>(h, a), *whh = hptr<float>(h, b), *bih = hptr<float>(h, ci), *bhh = hptr<float>(h, d);
      if (!wih || !whh || !bih || !bhh) { free_weights(h); return fail(ITA_ERR_BAD_BLOB, "incomplete LSTM parameters"); }
      const int in = l == 0 ? 517 : 128, kp = l == 0 ? K0P : 256;
      std::vector<float> wc((size_t)512 * kp, 0.0f), bs(512);
      for (int j = 0; j < 512; ++j) {
        memcpy(&wc[(size_t)j * kp], wih + (size_t)j * in, sizeof(float) * in);
        memcpy(&wc[(size_t)j * kp + in], whh + (size_t)j * 128, sizeof(float) * 128);
        bs[j] = bih[j] + bhh[j];
      }
      HIPCHK(hipMalloc(&h->wcat[l], wc.size() * sizeof(float)));
      HIPCHK(hipMemcpy(h->wcat[l], wc.data(), wc.size() * sizeof(float), hipMemcpyHostToDevice));
      HIPCHK(hipMalloc(&h->bsum[l], 512 * sizeof(float)));
      HIPCHK(hipMemcpy(h->bsum[l], bs.data(), 512 * sizeof(float), hipMemcpyHostToDevice));
      // split-precision planes, rows permuted to r' = ut*32 + gate*8 + u so that one MFMA tile holds
      // i,f,g,o of 8 units.  Layers 1, 2: the concatenated [W_ih | W_hh].  Layer 0: only what the folded
      // GEMM does not cover, [W_hh0 (128) | W_ih0[:,512] (desvel) | W_ih0[:,513:517] (quat) | 0] (K0S wide).
      const int kf = l == 0 ? K0S : 256;
      std::vector<float> wf((size_t)512 * kf, 0.0f);
      for (int rp = 0; rp < 512; ++rp) {
        const int j = ((rp >> 3) & 3) * 128 + (rp >> 5) * 8 + (rp & 7);
        if (l == 0) {
          memcpy(&wf[(size_t)rp * kf], whh + (size_t)j * 128, sizeof(float) * 128);
          memcpy(&wf[(size_t)rp * kf + 128], wih + (size_t)j * 517 + 512, sizeof(float) * 5);
        } else {
          memcpy(&wf[(size_t)rp * kf], &wc[(size_t)j * kp], sizeof(float) * 256);
        }
      }
      // ... and stored as the A fragments the LSTM kernels load: [ut][k-range][k-step][lane (row r, k half h)][8]
      const int nsw = l == 0 ? 1 : 4, nss = l == 0 ? kf / 16 : 4;   // k-ranges (one per wave) x k-steps of 16
      std::vector<float> wfrag(wf.size());
      for (int ut = 0; ut < 16; ++ut)
        for (int kw = 0; kw < nsw; ++kw)
          for (int st = 0; st < nss; ++st)
            for (int lane = 0; lane < 64; ++lane)
              for (int j = 0; j < 8; ++j)
                wfrag[((((size_t)ut * nsw + kw) * nss + st) * 64 + lane) * 8 + j] =
                    wf[(size_t)(ut * 32 + (lane & 31)) * kf + (kw * nss + st) * 16 + 8 * (lane >> 5) + j];
      int rc2 = split_upload(wfrag, &h->lw_hi[l], &h->lw_lo[l], &h->lw_inv_scale[l]);
      if (rc2) { free_weights(h); return rc2; }
    }
  }
  h->loaded = true;
  h->kfold = 128 * hdr.E;
  h->ldfold = h->kfold + 64;
  if (((hdr.has_tail && hdr.E == 64 && h->tail_wT) || !hdr.has_tail) && h->dec_w && h->lw_hi[0]) {
    int rc2 = build_fold(h);
    if (rc2) { free_weights(h); return rc2; }
  }
  return ITA_OK;
}

int ita_validate_blob(const void* blob, size_t nbytes, char* bad_name32) {
  const int v = ita_blob_validate(blob, nbytes, bad_name32);
  if (v) return fail(ITA_ERR_BAD_BLOB, std::string("blob validation failed (") + std::to_string(v) + ")");
  return ITA_OK;
}

int ita_reserve(ita_handle h, int max_batch) {
  int rc = check(h, max_batch);
  if (rc) return rc;
  h->ws_reserved = false;          // an explicit reserve may move the workspace: the caller vouches that nothing is in flight
  if (max_batch > h->cap) HIPCHK(hipDeviceSynchronize());
  rc = ensure_workspace(h, max_batch);
  h->ws_reserved = rc == ITA_OK;
  return rc;
}

int ita_get_dims(ita_handle h, int* E, int* S, int* P, int* F, int* H, int* num_layers) {
  if (!h || !h->loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (E) *E = h->hdr.E;
  if (S) *S = h->hdr.S;
  if (P) *P = h->hdr.P;
  if (F) *F = h->hdr.F;
  if (H) *H = h->hdr.H;
  if (num_layers) *num_layers = h->hdr.num_layers;
  return ITA_OK;
}

int ita_mha_int8_taps(ita_handle h, int layer, const float* x, float* y, int batch, const ita_mha_taps* taps,
                      void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !y || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  return launch_mha(h, layer, x, y, batch, false, taps, (hipStream_t)stream);
}
int ita_mha_int8(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  return ita_mha_int8_taps(h, layer, x, y, batch, nullptr, stream);
}

int ita_mha_long_q8(ita_handle h, int layer, const int8_t* x_q, int8_t* out_q, int batch, int seq_len, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x_q || !out_q || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  if (h->layers[layer].attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): no int8 long attention");
  if (h->hdr.E != 128) return fail(ITA_ERR_UNSUPPORTED, "long-sequence attention is built for E = 128 (models/ITA, models/ITA_upsample_shuffle)");
  if (seq_len < 128 || seq_len % 128 || seq_len > 65536 || batch > 65535)
    return fail(ITA_ERR_UNSUPPORTED, "seq_len must be a multiple of 128 in [128, 65536], batch <= 65535");
  const Layer& L = h->layers[layer];
  if (!L.simg_mha) return fail(ITA_ERR_UNSUPPORTED, "this layer has no attention image (accumulator range)");
  // the logits of a long row still fit the 16-bit travel format: same bound as stream_range_ok (per key, not per row)
  hipStream_t s = (hipStream_t)stream;
  const size_t ntile = (size_t)batch * (seq_len / 128);
  const size_t need = ntile * (3 * 24576 + 192 * 4);
  if (need > h->long_ws_bytes) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(ITA_ERR_INVALID_ARG, "the long-attention workspace cannot grow inside a stream capture; run one call first");
    HIPCHK(hipDeviceSynchronize());
    if (h->long_ws) (void)hipFree(h->long_ws);
    h->long_ws = nullptr; h->long_ws_bytes = 0;
    HIPCHK(hipMalloc(&h->long_ws, need));
    h->long_ws_bytes = need;
  }
  ItaLongArgs a{};
  a.image = L.simg_mha; a.xq = x_q; a.yq = out_q;
  a.qfrag = h->long_ws; a.kimg = a.qfrag + ntile * 24576; a.vimg = a.kimg + ntile * 24576;
  a.csum = (int*)(a.vimg + ntile * 24576);
  a.mq = L.ascal[ITA_A_MQ]; a.mk = L.ascal[ITA_A_MK]; a.mv = L.ascal[ITA_A_MV]; a.ml = L.ascal[ITA_A_ML];
  a.mc = L.ascal[ITA_A_MC]; a.mo = L.ascal[ITA_A_MO];
  a.B = batch; a.S = seq_len;
  const bool fast = L.fast_sites == ITA_SITES_ALL;
  const int pg = ntile < (size_t)h->num_cus ? (int)ntile : h->num_cus;
  if (fast) hipLaunchKernelGGL(ita_long_proj_kernel<true>, dim3(pg), dim3(512), (ItaStreamLds<128, false, false>::TOTAL), s, a);
  else hipLaunchKernelGGL(ita_long_proj_kernel<false>, dim3(pg), dim3(512), (ItaStreamLds<128, false, false>::TOTAL), s, a);
  HIPCHK(hipGetLastError());
  if (fast) hipLaunchKernelGGL(ita_long_attn_kernel<true>, dim3(seq_len / 128, batch), dim3(512), ItaLongLds::TOTAL, s, a);
  else hipLaunchKernelGGL(ita_long_attn_kernel<false>, dim3(seq_len / 128, batch), dim3(512), ItaLongLds::TOTAL, s, a);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

int ita_mha_q8(ita_handle h, int layer, const int8_t* x_q, int8_t* out_q, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x_q || !out_q || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  StreamIo io;
  io.xq = x_q; io.yq = out_q;
  return launch_stream(h, layer, 2, false, io, batch, (hipStream_t)stream);
}

int ita_ffn_int8_taps(ita_handle h, int layer, const float* x, float* y, int batch, const ita_ffn_taps* taps,
                      void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !y || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  return launch_ffn(h, layer, x, y, batch, false, taps, (hipStream_t)stream);
}
int ita_ffn_int8(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  return ita_ffn_int8_taps(h, layer, x, y, batch, nullptr, stream);
}

int ita_get_ffn_kind(ita_handle h, int layer, int* kind) {
  if (!h || !h->loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!kind || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  *kind = h->layers[layer].ffn_f32 ? ITA_FFN_F32 : ITA_FFN_INT8;
  return ITA_OK;
}

int ita_ffn_f32(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !y || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  return launch_ffn_f32(h, layer, x, y, batch, false, (hipStream_t)stream);
}

static_assert(ITA_HEAD_ERR_TIMEOUT == ITA_HEAD_TIMEOUT, "one error code, two names");
int ita_head_status(ita_handle h, int* status) {
  int rc = check(h, 1, false);
  if (rc) return rc;
  if (!status) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  *status = 0;
  if (!h->head_sync) return ITA_OK;
  unsigned v = 0;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&v, h->head_sync, sizeof(v), hipMemcpyDeviceToHost));
  if (v) {   // a timed-out workgroup left its tile's counter short: zero the error word and every counter
    HIPCHK(hipMemset(h->head_sync, 0, h->head_sync_bytes));
    HIPCHK(hipDeviceSynchronize());
  }
  *status = (int)v;
  return ITA_OK;
}

int ita_get_attn_kind(ita_handle h, int layer, int* kind) {
  if (!h || !h->loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!kind || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  *kind = h->layers[layer].attn_f32 ? ITA_ATTN_F32 : ITA_ATTN_INT8;
  return ITA_OK;
}

int ita_mha_f32(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !y || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  return launch_attn_f32(h, layer, x, y, batch, false, (hipStream_t)stream);
}

int ita_encoder_layer(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !y || layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  return launch_encoder(h, layer, x, y, nullptr, nullptr, nullptr, batch, (hipStream_t)stream);
}

int ita_debug_encoder_stamps(ita_handle h, int layer, const float* x, const void* image_u8, float* y, int batch,
                             unsigned long long* stamps, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if ((!x && !image_u8) || !y || !stamps || layer < 0 || layer >= h->hdr.num_layers)
    return fail(ITA_ERR_INVALID_ARG, "bad argument");
  if (h->layers[layer].attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): no stream kernel, no stamps");
  if (image_u8 ? !h->layers[layer].simg_tok : !h->layers[layer].simg_enc)
    return fail(ITA_ERR_UNSUPPORTED, "this layer does not run on the stream kernel");
  return launch_encoder(h, layer, x, y, nullptr, nullptr, nullptr, batch, (hipStream_t)stream, stamps, nullptr, nullptr,
                        nullptr, image_u8);
}

#ifdef ITA_UP_STAMP
// diagnostic build only: the phase stamps of the last ita_tail_up_kernel launch ([workgroup][wave 0 | 4][8] x u64)
int ita_debug_tail_up_stamps(unsigned long long* host_dst, int count) {
  if (hipDeviceSynchronize() != hipSuccess) return ITA_ERR_HIP;
  return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(ita_up_stamp_buf), sizeof(unsigned long long) * (size_t)count) == hipSuccess ? ITA_OK : ITA_ERR_HIP;
}
#endif
int ita_debug_softmax_rows(ita_handle h, const int8_t* logits, uint8_t* probs, int rows, void* stream) {
  int rc = check(h, rows, false);
  if (rc) return rc;
  if (!logits || !probs) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  hipLaunchKernelGGL(ita_softmax_rows_kernel, dim3((rows + 15) / 16), dim3(64), 0, (hipStream_t)stream, logits, probs, rows);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

int ita_tokenizer(ita_handle h, const void* image, int image_dtype, float* tokens, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!image || !tokens || (image_dtype != ITA_IMAGE_F32 && image_dtype != ITA_IMAGE_U8))
    return fail(ITA_ERR_INVALID_ARG, "bad pointer or image dtype");
  return launch_tokenizer(h, image, image_dtype, tokens, batch, (hipStream_t)stream);
}

int ita_ingest(ita_handle h, const void* src, int pixel_dtype, int height, int width, long long row_stride,
               long long frame_stride, float depth_scale, float* frames, int batch, void* stream) {
  // every argument is judged before the handle is used and before any HIP call
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (!src || !frames) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (pixel_dtype != ITA_PIXEL_U8 && pixel_dtype != ITA_PIXEL_U16 && pixel_dtype != ITA_PIXEL_F32)
    return fail(ITA_ERR_INVALID_ARG, "pixel_dtype must be ITA_PIXEL_U8, ITA_PIXEL_U16 or ITA_PIXEL_F32");
  if (height < 1 || height > ITA_INGEST_MAX_DIM || width < 1 || width > ITA_INGEST_MAX_DIM)
    return fail(ITA_ERR_INVALID_ARG, "height and width must be in [1, 4096]");
  if (batch < 1) return fail(ITA_ERR_INVALID_ARG, "batch must be positive");
  if (row_stride < width || frame_stride < (long long)(height - 1) * row_stride + width)
    return fail(ITA_ERR_INVALID_ARG, "row_stride < width, or frame_stride < (height - 1) * row_stride + width (strides are in pixels)");
  if (row_stride > (1ll << 40) || frame_stride > (1ll << 40))
    return fail(ITA_ERR_INVALID_ARG, "stride out of range");
  const size_t px = pixel_dtype == ITA_PIXEL_U8 ? 1 : pixel_dtype == ITA_PIXEL_U16 ? 2 : 4;
  if ((uintptr_t)src % px || (uintptr_t)frames % sizeof(float))
    return fail(ITA_ERR_INVALID_ARG, "src must be aligned to its pixel size, frames to 4 bytes");
  if (pixel_dtype == ITA_PIXEL_U16 && !(depth_scale > 0.0f && depth_scale <= 3.402823466e38f))
    return fail(ITA_ERR_INVALID_ARG, "depth_scale must be finite and positive");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  switch (pixel_dtype) {
    case ITA_PIXEL_U8: return launch_ingest<uint8_t>(h, src, height, width, row_stride, frame_stride, depth_scale, frames, batch, s);
    case ITA_PIXEL_U16: return launch_ingest<uint16_t>(h, src, height, width, row_stride, frame_stride, depth_scale, frames, batch, s);
    default: return launch_ingest<float>(h, src, height, width, row_stride, frame_stride, depth_scale, frames, batch, s);
  }
}

int ita_fusion_tail(ita_handle h, const float* x, float* feat, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !feat) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  return launch_tail(h, x, feat, 4608, batch, (hipStream_t)stream);
}

static void free_tail_large(ita_context* c) {
  if (c->tl_hi) (void)hipFree(c->tl_hi);
  if (c->tl_lo) (void)hipFree(c->tl_lo);
  if (c->tl_bias) (void)hipFree(c->tl_bias);
  if (c->tu_hi) (void)hipFree(c->tu_hi);
  if (c->tu_lo) (void)hipFree(c->tu_lo);
  if (c->ts_hi) (void)hipFree(c->ts_hi);
  if (c->ts_lo) (void)hipFree(c->ts_lo);
  c->tu_hi = c->tu_lo = c->ts_hi = c->ts_lo = nullptr;
  c->tl_hi = c->tl_lo = nullptr;
  c->tl_bias = nullptr;
  c->tl_E = c->tl_CO = c->tl_nt = c->tl_nchunk = 0;
}

int ita_fusion_tail_load(ita_handle h, const float* conv_w, const float* conv_b, int E, int out_ch) {
  int rc = check(h, 1, false);
  if (rc) return rc;
  if (!conv_w || !conv_b) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (E <= 0 || E % 16 || out_ch <= 0 || out_ch > 64) return fail(ITA_ERR_UNSUPPORTED, "needs E % 16 == 0 and out_ch <= 64");
  free_tail_large(h);
  const int CIN = E / 4 + E, nchunk = (CIN + 31) / 32, nt = (out_ch + 15) / 16, cop = nt * 16;
  // same scaling rule as split_upload: max |w| * 2^e in [512, 1024) keeps the lo halves normal in f16
  float mx = 0.0f;
  for (size_t i = 0; i < (size_t)out_ch * CIN * 9; ++i) mx = fabsf(conv_w[i]) > mx ? fabsf(conv_w[i]) : mx;
  int e = 0;
  if (mx > 0.0f) { int ex; frexpf(mx, &ex); e = 10 - ex; }
  const float sc = ldexpf(1.0f, e);
  std::vector<uint16_t> hi((size_t)nchunk * 9 * cop * 32, 0), lo(hi.size(), 0);
  for (int co = 0; co < out_ch; ++co)
    for (int c = 0; c < CIN; ++c)
      for (int tap = 0; tap < 9; ++tap) {
        const float v = conv_w[((size_t)co * CIN + c) * 9 + tap] * sc;
        const size_t d = (((size_t)(c / 32) * 9 + tap) * cop + co) * 32 + (c % 32);
        hi[d] = float_to_half(v);
        lo[d] = float_to_half(v - half_to_float(hi[d]));
      }
  std::vector<float> bias(cop < 48 ? 48 : cop, 0.0f);
  memcpy(bias.data(), conv_b, sizeof(float) * out_ch);
  if (E == 128 && out_ch <= 48) {
    // the 128 upsampled channels (conv input channels 32..159) as A fragments of v_mfma_f32_16x16x32_f16:
    // [tap][k-step j][N tile nt][lane (row = lane & 15 -> output channel 16 nt + row, k = 32 j + 8 (lane >> 4) + o(e))][e],
    // o(e) = 4 (e & 1) + (e >> 1): the element order of the kernel's token fragments (dword p of a fragment = the channel pair
    // of pixel-shuffle parity p)
    std::vector<uint16_t> uh((size_t)9 * 4 * 3 * 64 * 8, 0), ul(uh.size(), 0);
    for (int tap = 0; tap < 9; ++tap)
      for (int j = 0; j < 4; ++j)
        for (int nt2 = 0; nt2 < 3; ++nt2)
          for (int lane = 0; lane < 64; ++lane)
            for (int e2 = 0; e2 < 8; ++e2) {
              const int co = 16 * nt2 + (lane & 15), c = 32 + 32 * j + 8 * (lane >> 4) + 4 * (e2 & 1) + (e2 >> 1);
              if (co >= out_ch) continue;
              const float v = conv_w[((size_t)co * CIN + c) * 9 + tap] * sc;
              const size_t d = ((((size_t)tap * 4 + j) * 3 + nt2) * 64 + lane) * 8 + e2;
              uh[d] = float_to_half(v);
              ul[d] = float_to_half(v - half_to_float(uh[d]));
            }
    std::vector<uint16_t> sh((size_t)9 * 48 * 32, 0), sl(sh.size(), 0);
    for (int co = 0; co < out_ch; ++co)
      for (int c = 0; c < 32; ++c)
        for (int tap = 0; tap < 9; ++tap) {
          const float v = conv_w[((size_t)co * CIN + c) * 9 + tap] * sc;
          const size_t d = ((size_t)tap * 48 + co) * 32 + c;
          sh[d] = float_to_half(v);
          sl[d] = float_to_half(v - half_to_float(sh[d]));
        }
    HIPCHK(hipMalloc(&h->ts_hi, sh.size() * 2));
    HIPCHK(hipMalloc(&h->ts_lo, sl.size() * 2));
    HIPCHK(hipMemcpy(h->ts_hi, sh.data(), sh.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->ts_lo, sl.data(), sl.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&h->tu_hi, uh.size() * 2));
    HIPCHK(hipMalloc(&h->tu_lo, ul.size() * 2));
    HIPCHK(hipMemcpy(h->tu_hi, uh.data(), uh.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tu_lo, ul.data(), ul.size() * 2, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMalloc(&h->tl_hi, hi.size() * 2));
  HIPCHK(hipMalloc(&h->tl_lo, lo.size() * 2));
  HIPCHK(hipMalloc(&h->tl_bias, bias.size() * sizeof(float)));
  HIPCHK(hipMemcpy(h->tl_hi, hi.data(), hi.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->tl_lo, lo.data(), lo.size() * 2, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->tl_bias, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  h->tl_inv_scale = ldexpf(1.0f, -e);
  h->tl_E = E; h->tl_CO = out_ch; h->tl_nt = nt; h->tl_nchunk = nchunk;
  return ITA_OK;
}

int ita_fusion_tail_large(ita_handle h, const float* x, float* out, int batch, int tok_h, int tok_w, void* stream) {
  int rc = check(h, batch, false);
  if (rc) return rc;
  if (!x || !out) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (!h->tl_hi) return fail(ITA_ERR_NO_WEIGHTS, "ita_fusion_tail_load has not been called");
  if (tok_h < 4 || tok_w < 16 || (2 * tok_h) % 8 || (2 * tok_w) % 32 || batch > 65535)
    return fail(ITA_ERR_UNSUPPORTED, "needs tok_h % 4 == 0, tok_w % 16 == 0, batch <= 65535");
  ItaTailBigArgs a{x, h->tl_hi, h->tl_lo, h->tl_bias, h->tl_inv_scale, out, batch, h->tl_E, tok_h, tok_w, h->tl_CO, h->tl_nchunk, 0};
  hipStream_t s = (hipStream_t)stream;
  // E = 128: the upsampled channels (4/5 of the contraction) by linearity on the low-resolution tokens (ita_tail_up_kernel),
  // the pixel-shuffle channels (= chunk 0 of the implicit GEMM) in phase 2 of the same kernel.  Needs whole 16 x 32 tiles and
  // every tile's source region inside 10 x 18 tokens (same float expressions as the kernel; true for every x2 grid tried,
  // checked instead of assumed).  Every other shape runs on ita_tail_big_kernel.
  if (h->tu_hi && (2 * tok_h) % 16 == 0 && (2 * tok_w) % 32 == 0) {
    const int OH = 2 * tok_h, OW = 2 * tok_w;
    auto span_ok = [](int T, int O, int tile, int lim) {
      const float sc = (float)(T - 1) / (float)(O - 1);
      auto src = [&](int q) { int i = (int)(sc * (float)q); return i > T - 1 ? T - 1 : i; };
      for (int t0 = 0; t0 < O; t0 += tile) {
        const int lo = src(t0 - 1 < 0 ? 0 : t0 - 1), hq = src(t0 + tile > O - 1 ? O - 1 : t0 + tile);
        if (hq + (hq < T - 1 ? 1 : 0) - lo > lim - 1) return false;
        // the pixel-shuffle halo takes its tokens (q >> 1) from the same region
        const int q0 = t0 - 1 < 0 ? 0 : t0 - 1, q1 = t0 + tile > O - 1 ? O - 1 : t0 + tile;
        if ((q0 >> 1) < lo || (q1 >> 1) - lo > lim - 1) return false;
      }
      return true;
    };
    if (span_ok(tok_h, OH, 16, ItaTailUpLds::RH) && span_ok(tok_w, OW, 32, ItaTailUpLds::RW)) {
      ItaTailUpArgs u{x, h->tu_hi, h->tu_lo, h->ts_hi, h->ts_lo, h->tl_bias, h->tl_inv_scale, out, batch, tok_h, tok_w, h->tl_CO};
      const long ntiles = (long)(OW / 32) * (OH / 16) * batch;      // persistent: one workgroup per CU, tiles dealt round robin
      hipLaunchKernelGGL(ita_tail_up_kernel, dim3((unsigned)(ntiles < h->num_cus ? ntiles : h->num_cus)), dim3(512), ItaTailUpLds::TOTAL, s, u);
      HIPCHK(hipGetLastError());
      return ITA_OK;
    }
  }
  switch (h->tl_nt) {
    case 1: return launch_tail_big<1>(a, s);
    case 2: return launch_tail_big<2>(a, s);
    case 3: return launch_tail_big<3>(a, s);
    default: return launch_tail_big<4>(a, s);
  }
}

// the LSTM head behind the folded GEMM: layers 0, 1, 2 and the fc in one launch (ita_lstm_head_kernel), reading the
// GEMM's split-K partials `part`.  State rows are slots[b] (else b) of (3, rows, 128) arrays with layer stride lstride;
// h_out / c_out may alias h_in / c_in.
static int launch_lstm_head(ita_context* h, const float* part, const float* desvel, const float* quat, const float* h_in,
                            const float* c_in, float* h_out, float* c_out, size_t lstride, float* vel, int B,
                            const int* slots, hipStream_t s) {
  ItaLstmHeadArgs p{part, h->fold_inv_scale, h->lw_hi[0], h->lw_lo[0], h->lw_inv_scale[0], h->fold_bias,
                    h->lw_hi[1], h->lw_lo[1], h->lw_hi[2], h->lw_lo[2], h->lw_inv_scale[1], h->lw_inv_scale[2],
                    h->bsum[1], h->bsum[2], desvel, quat, h_in, c_in, h_out, c_out, lstride,
                    h->c1_hi, h->c1_lo, h->c2_hi, h->c2_lo, h->fc_w, h->fc_b, vel, h->head_sync + ITA_HEAD_CNT_STRIDE, h->head_sync, B, slots};
  hipLaunchKernelGGL(ita_lstm_head_kernel<NSPLIT>, dim3(16 * ((B + 31) / 32)), dim3(256), 0, s, p);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}

// x2_in != null: start behind the encoder from a given (B,128,E) activation (ita_vitlstm_tail); image is then unused
static int forward_impl(ita_handle h, const void* image, int image_dtype, const float* desvel, const float* quat,
                        const float* h_in, const float* c_in, float* vel, float* h_out, float* c_out, int batch,
                        const ita_forward_taps* taps, void* stream, const int* slots, int state_rows,
                        const float* x2_in = nullptr) {
  int rc = check(h, batch);
  if (rc) return rc;
  if ((!image && !x2_in) || !desvel || !quat || !h_in || !c_in || !vel || !h_out || !c_out)
    return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (image_dtype != ITA_IMAGE_F32 && image_dtype != ITA_IMAGE_U8) return fail(ITA_ERR_INVALID_ARG, "bad image dtype");
  if (!h->dec_w || !h->wcat[0] || !h->fc_w || (h->hdr.has_tail && !h->tail_wT))
    return fail(ITA_ERR_BAD_BLOB, "blob holds no decoder / LSTM (/ fusion tail) parameters");
  if (h->hdr.has_tail && h->hdr.E != 64) return fail(ITA_ERR_UNSUPPORTED, "the fusion tail is built for E = 64 (ITAViTLSTM)");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = batch;
  const size_t tokb = sizeof(float) * (size_t)B * 128 * h->hdr.E;
  const bool fast = h->tail_mode == 1 && h->folded;
  if (slots && !fast) return fail(ITA_ERR_UNSUPPORTED, "slot-indexed state needs tail mode 1");
  const size_t lstride = (size_t)(slots ? state_rows : batch) * 128;   // layer stride of the (3, rows, 128) state
  const int ev_per_fwd = 5 + 2 * h->hdr.num_layers;
  hipEvent_t* ev = nullptr;
  if (h->prof && h->prof_n < h->prof_max && (h->prof_calls++ % h->prof_every) == 0)
    ev = &h->prof_ev[(size_t)h->prof_n * ev_per_fwd];
  // an event in the stream costs a pipeline bubble of ~5 us (the next kernel cannot be launched
  // under the tail of the previous one), so in single-stage mode only that stage's two marks are recorded
  int evi = 0, m_lo = 0, m_hi = ev_per_fwd - 1;
  if (h->prof_stage >= 0) {
    const int L2 = 2 * h->hdr.num_layers;
    const int lo[ITA_NUM_STAGES] = {0, 1, 1, 1 + L2, 2 + L2, 3 + L2}, hi[ITA_NUM_STAGES] = {1, 1 + L2, 1 + L2, 2 + L2, 3 + L2, 4 + L2};
    m_lo = lo[h->prof_stage]; m_hi = hi[h->prof_stage];
  }
#define MARK() do { if (ev && (h->prof_stage < 0 || evi == m_lo || evi == m_hi)) HIPCHK(hipEventRecord(ev[evi], s)); ++evi; } while (0)
  MARK();
  const bool fused_tok = !x2_in && fuse_tokenizer(h, image_dtype);
  if (slots && !x2_in) {   // refuse before the first launch: the slot-indexed form is served by the stream kernel only
    const Layer& LL = h->layers.back();
    if (!LL.ffn_f32 && !((fused_tok && h->hdr.num_layers == 1) ? LL.simg_tok : LL.simg_enc))
      return fail(ITA_ERR_UNSUPPORTED, "slot-indexed state needs the stream kernel (this blob's accumulator range rules it out)");
  }
  if (x2_in) {
    HIPCHK(hipMemcpyAsync(h->bufA, x2_in, tokb, hipMemcpyDeviceToDevice, s));
    if (fast) {
      const size_t n = (size_t)B * 128 * h->hdr.E;
      hipLaunchKernelGGL(ita_split_planes_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, s, h->bufA, h->x2_hi,
                         h->x2_lo, 128 * h->hdr.E, h->ldfold, B);
      HIPCHK(hipGetLastError());
    }
  } else if (!fused_tok && (rc = launch_tokenizer(h, image, image_dtype, h->bufA, B, s))) return rc;
  MARK();
  if (!x2_in && !fused_tok && taps && taps->tokens) HIPCHK(hipMemcpyAsync(taps->tokens, h->bufA, tokb, hipMemcpyDeviceToDevice, s));
  for (int l = 0; l < (x2_in ? 0 : h->hdr.num_layers); ++l) {
    const bool last = l == h->hdr.num_layers - 1;
    const bool planes = fast && last;
    float* yout = (planes && !(taps && taps->x2)) ? nullptr : h->bufA;
    bool marked = false;   // a float-FFN layer records the attention / FFN boundary between its two launches
    const std::function<int()> mid = [&]() -> int { MARK(); marked = true; return ITA_OK; };
    // one encoder layer, in place on bufA
    if ((rc = launch_encoder(h, l, h->bufA, yout, planes ? h->x2_hi : nullptr, planes ? h->x2_lo : nullptr,
                             (taps && last) ? taps->x1 : nullptr, B, s, nullptr, nullptr, nullptr, slots,
                             (fused_tok && l == 0) ? image : nullptr,
                             (fused_tok && l == 0 && taps) ? taps->tokens : nullptr, &mid))) return rc;
    if (!marked) MARK();
    MARK();
  }
  if (x2_in) { MARK(); MARK(); }
  if (taps && taps->x2) HIPCHK(hipMemcpyAsync(taps->x2, h->bufA, tokb, hipMemcpyDeviceToDevice, s));
  if (fast) {
    // folded tail+decoder: dec = x2 . Wfold^T + bias'   (x2 planes were written by the last FFN)
    if ((rc = launch_gemm_split<128, 128, 2, 4>(h->x2_hi, h->x2_lo, h->ldfold, h->fold_hi, h->fold_lo, h->ldfold, h->part, B,
                                                512, h->kfold, NSPLIT, s, h->foldf_hi, h->foldf_lo))) return rc;
    MARK();
    MARK();
    if ((rc = launch_lstm_head(h, h->part, desvel, quat, h_in, c_in, h_out, c_out, lstride, vel, B, slots, s))) return rc;
    MARK();
  } else {
    if (h->hdr.has_tail) {
      if ((rc = launch_tail(h, h->bufA, h->feat, 4608, B, s))) return rc;
      MARK();
      if (taps && taps->feat)
        HIPCHK(hipMemcpyAsync(taps->feat, h->feat, sizeof(float) * (size_t)B * 4608, hipMemcpyDeviceToDevice, s));
      // decoder writes straight into the LSTM layer-0 concat buffer (columns 0..511)
      if ((rc = launch_gemm(h->feat, 4608, h->dec_w, 4608, h->dec_b, h->cat0, K0P, B, 512, 4608, s))) return rc;
    } else {   // no fusion tail: the decoder reads the flattened tokens, (B,128,E) as it stands in bufA
      MARK();
      if ((rc = launch_gemm(h->bufA, h->kfold, h->dec_w, h->kfold, h->dec_b, h->cat0, K0P, B, 512, h->kfold, s))) return rc;
    }
    MARK();
    if (taps && taps->dec)
      HIPCHK(hipMemcpy2DAsync(taps->dec, 512 * sizeof(float), h->cat0, K0P * sizeof(float), 512 * sizeof(float), B,
                              hipMemcpyDeviceToDevice, s));
    {
      ItaLstmPrepArgs p{desvel, quat, h_in, h->cat0, h->cat1, h->cat2, K0P, B};
      hipLaunchKernelGGL(ita_lstm_prep_kernel, dim3(B), dim3(256), 0, s, p);
      HIPCHK(hipGetLastError());
    }
    float* cats[3] = {h->cat0, h->cat1, h->cat2};
    const int kp[3] = {K0P, 256, 256};
    for (int l = 0; l < 3; ++l) {
      if ((rc = launch_gemm(cats[l], kp[l], h->wcat[l], kp[l], h->bsum[l], h->gates, 512, B, 512, kp[l], s))) return rc;
      ItaLstmPointArgs p{h->gates, c_in + (size_t)l * B * 128, h_out + (size_t)l * B * 128, c_out + (size_t)l * B * 128,
                         l < 2 ? cats[l + 1] : nullptr, 256, B};
      hipLaunchKernelGGL(ita_lstm_point_kernel, dim3((B * 128 + 255) / 256), dim3(256), 0, s, p);
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(ita_fc_kernel, dim3((B * 3 + 63) / 64), dim3(64), 0, s, h_out + (size_t)2 * B * 128, h->fc_w,
                       h->fc_b, vel, B);
    HIPCHK(hipGetLastError());
    MARK();
  }
#undef MARK
  if (ev) ++h->prof_n;
  return ITA_OK;
}

int ita_vitlstm_forward(ita_handle h, const void* image, int image_dtype, const float* desvel, const float* quat,
                        const float* h_in, const float* c_in, float* vel, float* h_out, float* c_out, int batch,
                        const ita_forward_taps* taps, void* stream) {
  return forward_impl(h, image, image_dtype, desvel, quat, h_in, c_in, vel, h_out, c_out, batch, taps, stream, nullptr, 0);
}

int ita_vitlstm_tail(ita_handle h, const float* x2, const float* desvel, const float* quat, const float* h_in,
                     const float* c_in, float* vel, float* h_out, float* c_out, int batch, void* stream) {
  if (!x2) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  // (both graph families: with the fusion tail E = 64 -- forward_impl checks --, without it the decoder reads x2 itself)
  return forward_impl(h, nullptr, ITA_IMAGE_F32, desvel, quat, h_in, c_in, vel, h_out, c_out, batch, nullptr, stream, nullptr, 0, x2);
}

// ---- two-stage form for software pipelining across time steps -------------------------------------
// parts: 1 = tokenizer + encoder into the x2 planes `xbuf`, 2 = folded GEMM from planes `xbuf` into partial buffer `buf`
static int front_impl(ita_handle h, const void* image, int image_dtype, int batch, int buf, void* stream,
                      void* encoder_done_event, int xbuf = 0, int parts = 3) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (((parts & 1) && !image) || buf < 0 || buf >= ITA_PART_BUFFERS || xbuf < 0 || xbuf > 1)
    return fail(ITA_ERR_INVALID_ARG, "null image, buf not in [0, ITA_PART_BUFFERS) or plane set not 0 / 1");
  if ((parts & 1) && image_dtype != ITA_IMAGE_F32 && image_dtype != ITA_IMAGE_U8) return fail(ITA_ERR_INVALID_ARG, "bad image dtype");
  if (!(h->tail_mode == 1 && h->folded)) return fail(ITA_ERR_UNSUPPORTED, "front/back form needs tail mode 1 and a full ITAViTLSTM blob");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream))) return rc;
  if (parts & 2) h->front_cap[buf] = h->cap;
  hipStream_t s = (hipStream_t)stream;
  _Float16* const xh = h->x2_hi + (size_t)xbuf * h->cap * h->ldfold;
  _Float16* const xl = h->x2_lo + (size_t)xbuf * h->cap * h->ldfold;
  // sampled single-stage profiling (ita_profile_begin_sampled with only_stage 0, 1 or 3) also works here
  const int L2 = 2 * h->hdr.num_layers, per = 5 + L2;
  hipEvent_t* ev = nullptr;
  if (h->prof && h->prof_stage >= 0 && h->prof_n < h->prof_max && (h->prof_calls++ % h->prof_every) == 0)
    ev = &h->prof_ev[(size_t)h->prof_n * per];
  auto mark = [&](int stage, bool end) -> int {
    if (ev && h->prof_stage == stage) {
      const int lo[ITA_NUM_STAGES] = {0, 1, 1, 1 + L2, 2 + L2, 3 + L2}, hi[ITA_NUM_STAGES] = {1, 1 + L2, 1 + L2, 2 + L2, 3 + L2, 4 + L2};
      HIPCHK(hipEventRecord(ev[end ? hi[stage] : lo[stage]], s));
    }
    return ITA_OK;
  };
  if (parts & 1) {
    if ((rc = mark(0, false))) return rc;
    const bool fused_tok = fuse_tokenizer(h, image_dtype);
    if (!fused_tok && (rc = launch_tokenizer(h, image, image_dtype, h->bufA, batch, s))) return rc;
    if ((rc = mark(0, true)) || (rc = mark(1, false))) return rc;
    for (int l = 0; l < h->hdr.num_layers; ++l) {
      const bool last = l == h->hdr.num_layers - 1;
      if ((rc = launch_encoder(h, l, h->bufA, last ? nullptr : h->bufA, last ? xh : nullptr, last ? xl : nullptr,
                               nullptr, batch, s, nullptr, nullptr, nullptr, nullptr, (fused_tok && l == 0) ? image : nullptr,
                               nullptr))) return rc;
    }
    if ((rc = mark(1, true))) return rc;
    if (encoder_done_event) HIPCHK(hipEventRecord((hipEvent_t)encoder_done_event, s));
  }
  if (parts & 2) {
    if ((rc = mark(3, false))) return rc;
    float* part = h->part + (size_t)buf * NSPLIT * h->cap * 512;
    if ((rc = launch_gemm_split<128, 128, 2, 4>(xh, xl, h->ldfold, h->fold_hi, h->fold_lo, h->ldfold, part, batch, 512,
                                                h->kfold, NSPLIT, s, h->foldf_hi, h->foldf_lo))) return rc;
    if ((rc = mark(3, true))) return rc;
  }
  if (ev && (h->prof_stage == 0 || h->prof_stage == 1 || h->prof_stage == 3)) ++h->prof_n;
  return ITA_OK;
}

int ita_vitlstm_front(ita_handle h, const void* image, int image_dtype, int batch, int buf, void* stream) {
  return front_impl(h, image, image_dtype, batch, buf, stream, nullptr);
}

int ita_vitlstm_front_ev(ita_handle h, const void* image, int image_dtype, int batch, int buf, void* stream,
                         void* encoder_done_event) {
  return front_impl(h, image, image_dtype, batch, buf, stream, encoder_done_event);
}

int ita_vitlstm_encode(ita_handle h, const void* image, int image_dtype, int batch, int plane_set, void* stream) {
  return front_impl(h, image, image_dtype, batch, 0, stream, nullptr, plane_set, 1);
}

int ita_vitlstm_fold(ita_handle h, int batch, int plane_set, int buf, void* stream) {
  return front_impl(h, nullptr, ITA_IMAGE_U8, batch, buf, stream, nullptr, plane_set, 2);
}

int ita_vitlstm_back(ita_handle h, const float* desvel, const float* quat, const float* h_in, const float* c_in, float* vel,
                     float* h_out, float* c_out, int batch, int buf, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!desvel || !quat || !h_in || !c_in || !vel || !h_out || !c_out || buf < 0 || buf >= ITA_PART_BUFFERS)
    return fail(ITA_ERR_INVALID_ARG, "null pointer or buf not in [0, ITA_PART_BUFFERS)");
  if (!(h->tail_mode == 1 && h->folded)) return fail(ITA_ERR_UNSUPPORTED, "front/back form needs tail mode 1 and a full ITAViTLSTM blob");
  if (batch > h->cap || h->front_cap[buf] != h->cap)
    return fail(ITA_ERR_INVALID_ARG, "ita_vitlstm_front has not filled this buffer for the current workspace (reserve before front)");
  hipStream_t s = (hipStream_t)stream;
  const int B = batch;
  const size_t lstride = (size_t)B * 128;
  const float* part = h->part + (size_t)buf * NSPLIT * h->cap * 512;
  // h_out may alias h_in: the head kernel reads all of h_in before any h_out element is written
  return launch_lstm_head(h, part, desvel, quat, h_in, c_in, h_out, c_out, lstride, vel, B, nullptr, s);
}

// n consecutive time steps, software-pipelined from the host: front(t+1) on stream_front while back(t) is on stream_back
int ita_vitlstm_pipelined(ita_handle h, const void* const* image, int image_dtype, const float* const* desvel,
                          const float* const* quat, float* state_h, float* state_c, float* const* vel, int batch, int n_steps,
                          void* stream_front, void* stream_back) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!image || !desvel || !quat || !state_h || !state_c || !vel || n_steps <= 0 || !stream_front || !stream_back ||
      stream_front == stream_back)
    return fail(ITA_ERR_INVALID_ARG, "null argument, n_steps <= 0, or the two streams are not two distinct non-default streams");
  if (h->prof)   // two host threads would write the one profiling state of this handle
    return fail(ITA_ERR_INVALID_ARG, "ita_vitlstm_pipelined cannot run between ita_profile_begin and ita_profile_end");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream_front))) return rc;
  hipStream_t sf = (hipStream_t)stream_front, sb = (hipStream_t)stream_back;
  const size_t nstate = (size_t)3 * batch * 128;
  if (h->pipe_cap < batch) {   // the second copy of the state, so that no step updates its state in place
    if (h->pipe_h) (void)hipFree(h->pipe_h);
    h->pipe_h = nullptr; h->pipe_cap = 0;
    HIPCHK(hipMalloc(&h->pipe_h, 2 * nstate * sizeof(float)));
    h->pipe_cap = batch;
  }
  while ((int)h->pipe_ev.size() < 2 * ITA_PART_BUFFERS + 1) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->pipe_ev.push_back(e);
  }
  hipEvent_t* evf = h->pipe_ev.data();                       // front(t) done, ring of ITA_PART_BUFFERS
  hipEvent_t* evb = h->pipe_ev.data() + ITA_PART_BUFFERS;    // back(t) done
  float* sh[2] = {state_h, h->pipe_h};
  float* sc[2] = {state_c, h->pipe_h + nstate};
  // the back stream starts after what the caller has already put on the front stream (the state it hands over)
  HIPCHK(hipEventRecord(h->pipe_ev[2 * ITA_PART_BUFFERS], sf));
  HIPCHK(hipStreamWaitEvent(sb, h->pipe_ev[2 * ITA_PART_BUFFERS], 0));
  // Two host threads, one per stream: a step is about six kernel launches and three event calls, 31-37 us of host time
  // when one thread issues them all -- about what the GPU needs for a 128-frame step.  The calling thread issues
  // the fronts, a helper the backs; they hand over "event t has been recorded / waited for" through two counters,
  // because hipStreamWaitEvent must come after the hipEventRecord it refers to in HOST order.
  std::atomic<int> fronts_recorded{0}, backs_recorded{0}, abort_flag{0};
  int rc_back = ITA_OK;
  std::string msg_back;     // the helper's error text (its fail() writes ITS thread-local message)
  auto back_body = [&]() {
    if (hipSetDevice(h->device) != hipSuccess) {   // a new thread starts on device 0
      rc_back = fail(ITA_ERR_HIP, "hipSetDevice (back stream's host thread)");
      msg_back = tl_msg;
      abort_flag.store(1, std::memory_order_relaxed);
      return;
    }
    for (int t = 0; t < n_steps; ++t) {
      const int buf = t % ITA_PART_BUFFERS;
      while (fronts_recorded.load(std::memory_order_acquire) <= t) {
        if (abort_flag.load(std::memory_order_relaxed)) return;
        std::this_thread::yield();
      }
      if (hipStreamWaitEvent(sb, evf[buf], 0) != hipSuccess) { rc_back = fail(ITA_ERR_HIP, "hipStreamWaitEvent (back stream)"); break; }
      if ((rc_back = ita_vitlstm_back(h, desvel[t], quat[t], sh[t & 1], sc[t & 1], vel[t], sh[(t + 1) & 1], sc[(t + 1) & 1], batch,
                                      buf, sb)))
        break;
      if (hipEventRecord(evb[buf], sb) != hipSuccess) { rc_back = fail(ITA_ERR_HIP, "hipEventRecord (back stream)"); break; }
      backs_recorded.store(t + 1, std::memory_order_release);
    }
    if (rc_back) {
      msg_back = tl_msg;
      abort_flag.store(1, std::memory_order_relaxed);
    }
  };
  std::thread back_thread;
  try {
    back_thread = std::thread(back_body);
  } catch (const std::exception& e) {   // std::system_error must not escape through the C ABI
    return fail(ITA_ERR_HIP, std::string("ita_vitlstm_pipelined: cannot start the back stream's host thread: ") + e.what());
  }
  for (int t = 0; t < n_steps && !rc; ++t) {
    const int buf = t % ITA_PART_BUFFERS;
    if (t >= ITA_PART_BUFFERS) {   // front(t) overwrites what back(t - NB) read
      while (backs_recorded.load(std::memory_order_acquire) <= t - ITA_PART_BUFFERS && !abort_flag.load(std::memory_order_relaxed))
        std::this_thread::yield();
      if (abort_flag.load(std::memory_order_relaxed)) break;
      if (hipStreamWaitEvent(sf, evb[buf], 0) != hipSuccess) { rc = fail(ITA_ERR_HIP, "hipStreamWaitEvent (front stream)"); break; }
    }
    if ((rc = ita_vitlstm_front(h, image[t], image_dtype, batch, buf, sf))) break;
    if (hipEventRecord(evf[buf], sf) != hipSuccess) { rc = fail(ITA_ERR_HIP, "hipEventRecord (front stream)"); break; }
    fronts_recorded.store(t + 1, std::memory_order_release);
  }
  if (rc) abort_flag.store(1, std::memory_order_relaxed);
  back_thread.join();
  if (rc) return rc;
  if (rc_back) return fail(rc_back, "ita_vitlstm_pipelined, back stream's host thread: " + msg_back);
  if (n_steps & 1) {   // an odd number of steps leaves the state in the internal copy
    HIPCHK(hipMemcpyAsync(state_h, sh[1], nstate * sizeof(float), hipMemcpyDeviceToDevice, sb));
    HIPCHK(hipMemcpyAsync(state_c, sc[1], nstate * sizeof(float), hipMemcpyDeviceToDevice, sb));
  }
  // join: everything is complete in stream_front's order
  HIPCHK(hipEventRecord(h->pipe_ev[2 * ITA_PART_BUFFERS], sb));
  HIPCHK(hipStreamWaitEvent(sf, h->pipe_ev[2 * ITA_PART_BUFFERS], 0));
  return ITA_OK;
}

// T time steps of `batch` streams in one call: the image-only part of a chunk of steps runs as ONE batch of Tc * batch
// frames (time-major rows), the recurrence of those Tc steps as one ita_lstm_seq_kernel launch; the state is carried in
// state_h / state_c from chunk to chunk.  One stream, no host synchronisation, no allocation once the workspace holds
// `batch` frames.  (Running the fronts of later chunks ahead on a second stream was built and measured: slower at every
// shape with more than one chunk, profiles/r05_sequence_overlap_ab.txt.)
int ita_vitlstm_sequence(ita_handle h, const void* image, int image_dtype, const float* desvel, const float* quat,
                         float* state_h, float* state_c, const int* lengths, float* vel, int n_steps, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!image || !desvel || !quat || !state_h || !state_c || !vel) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (n_steps <= 0) return fail(ITA_ERR_INVALID_ARG, "n_steps must be positive");
  if (image_dtype != ITA_IMAGE_F32 && image_dtype != ITA_IMAGE_U8) return fail(ITA_ERR_INVALID_ARG, "bad image dtype");
  if (!(h->tail_mode == 1 && h->folded)) return fail(ITA_ERR_UNSUPPORTED, "the sequence form needs tail mode 1 and a full ITAViTLSTM blob");
  if (h->prof) return fail(ITA_ERR_INVALID_ARG, "ita_vitlstm_sequence cannot run between ita_profile_begin and ita_profile_end");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = batch, Tc = h->cap / B;   // >= 1: the workspace holds at least B frames
  const size_t frame_bytes = (size_t)60 * 90 * (image_dtype == ITA_IMAGE_U8 ? 1 : sizeof(float));
  for (int t0 = 0; t0 < n_steps; t0 += Tc) {
    const int n = std::min(Tc, n_steps - t0);
    const size_t row0 = (size_t)t0 * B;
    if ((rc = front_impl(h, (const char*)image + row0 * frame_bytes, image_dtype, n * B, 0, stream, nullptr))) return rc;
    ItaLstmSeqArgs p{h->part, h->fold_inv_scale, h->lw_hi[0], h->lw_lo[0], h->lw_inv_scale[0], h->fold_bias,
                     h->lw_hi[1], h->lw_lo[1], h->lw_hi[2], h->lw_lo[2], h->lw_inv_scale[1], h->lw_inv_scale[2],
                     h->bsum[1], h->bsum[2], desvel + row0, quat + row0 * 4, state_h, state_c, lengths, t0, h->seq_ho,
                     h->fc_w, h->fc_b, vel + row0 * 3, h->head_sync + ITA_HEAD_CNT_STRIDE, h->head_sync, B, n};
    hipLaunchKernelGGL(ita_lstm_seq_kernel<NSPLIT>, dim3(16 * ((B + 31) / 32)), dim3(256), 0, s, p);
    HIPCHK(hipGetLastError());
  }
  h->front_cap[0] = 0;   // partial buffer 0 holds time-major rows of several steps: not something ita_vitlstm_back may read
  return ITA_OK;
}

int ita_vitlstm_forward_slots(ita_handle h, const void* image, int image_dtype, const float* desvel, const float* quat,
                              float* state_h, float* state_c, const int* slot_idx, int num_slots, float* vel, int batch,
                              void* stream) {
  if (!slot_idx || num_slots < batch) return fail(ITA_ERR_INVALID_ARG, "slot_idx null or fewer slots than frames");
  return forward_impl(h, image, image_dtype, desvel, quat, state_h, state_c, vel, state_h, state_c, batch, nullptr, stream,
                      slot_idx, num_slots);
}

int ita_profile_begin(ita_handle h, int max_forwards) { return ita_profile_begin_sampled(h, max_forwards, 1, -1); }

int ita_profile_begin_sampled(ita_handle h, int max_forwards, int every_n, int only_stage) {
  int rc = check(h, 1);
  if (rc) return rc;
  if (max_forwards <= 0 || max_forwards > 4096) return fail(ITA_ERR_INVALID_ARG, "max_forwards out of range");
  if (every_n < 1 || only_stage < -1 || only_stage >= ITA_NUM_STAGES) return fail(ITA_ERR_INVALID_ARG, "bad sampling arguments");
  h->prof_every = every_n;
  h->prof_stage = only_stage;
  h->prof_calls = 0;
  const size_t need = (size_t)max_forwards * (5 + 2 * h->hdr.num_layers);
  while (h->prof_ev.size() < need) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    h->prof_ev.push_back(e);
  }
  h->prof = true;
  h->prof_max = max_forwards;
  h->prof_n = 0;
  return ITA_OK;
}

int ita_profile_end(ita_handle h, double* stage_ms, int* n_forwards) {
  if (!h || !stage_ms || !n_forwards) return fail(ITA_ERR_INVALID_ARG, "null argument");
  HIPCHK(hipSetDevice(h->device));
  h->prof = false;
  const int L = h->hdr.num_layers, per = 5 + 2 * L;
  for (int i = 0; i < ITA_NUM_STAGES; ++i) stage_ms[i] = 0.0;
  for (int f = 0; f < h->prof_n; ++f) {
    hipEvent_t* ev = &h->prof_ev[(size_t)f * per];
    HIPCHK(hipEventSynchronize(ev[h->prof_stage >= 0 ? (h->prof_stage == 0 ? 1 : (h->prof_stage <= 2 ? 1 + 2 * L : h->prof_stage - 1 + 2 * L)) : per - 1]));
    auto dt = [&](int a, int b, double* acc) -> int {
      float ms = 0.0f;
      HIPCHK(hipEventElapsedTime(&ms, ev[a], ev[b]));
      *acc += ms;
      return ITA_OK;
    };
    int rc;
    if (h->prof_stage >= 0) {     // single-stage mode: only that stage's two marks exist
      const int lo[ITA_NUM_STAGES] = {0, 1, 1, 1 + 2 * L, 2 + 2 * L, 3 + 2 * L}, hi[ITA_NUM_STAGES] = {1, 1 + 2 * L, 1 + 2 * L, 2 + 2 * L, 3 + 2 * L, 4 + 2 * L};
      if ((rc = dt(lo[h->prof_stage], hi[h->prof_stage], &stage_ms[h->prof_stage]))) return rc;
      continue;
    }
    if ((rc = dt(0, 1, &stage_ms[0]))) return rc;
    for (int l = 0; l < L; ++l) {
      if ((rc = dt(1 + 2 * l, 2 + 2 * l, &stage_ms[1]))) return rc;
      if ((rc = dt(2 + 2 * l, 3 + 2 * l, &stage_ms[2]))) return rc;
    }
    if ((rc = dt(1 + 2 * L, 2 + 2 * L, &stage_ms[3]))) return rc;
    if ((rc = dt(2 + 2 * L, 3 + 2 * L, &stage_ms[4]))) return rc;
    if ((rc = dt(3 + 2 * L, 4 + 2 * L, &stage_ms[5]))) return rc;
  }
  *n_forwards = h->prof_n;
  h->prof_n = 0;
  return ITA_OK;
}

int ita_wire_unpack_packet(const uint8_t* packet, size_t nbytes, int quat_stride_bug, float* frame_out) {
  ita_wire_frame f;
  if (!frame_out || ita_wire_unpack(packet, nbytes, quat_stride_bug, &f)) return fail(ITA_ERR_INVALID_ARG, "short packet");
  frame_out[0] = f.desired_velocity; frame_out[1] = f.position_x;
  for (int i = 0; i < 4; ++i) frame_out[2 + i] = f.quaternion[i];
  return ITA_OK;
}
void ita_wire_postprocess(const float* raw3, float desired_velocity, float position_x, float* out3) {
  ita_wire_final_velocity(raw3, desired_velocity, position_x, out3);
}

int ita_set_tail_mode(ita_handle h, int mode) {
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (mode != 0 && mode != 1) return fail(ITA_ERR_INVALID_ARG, "mode must be 0 (exact f32) or 1 (folded f16x3)");
  h->tail_mode = mode;
  return ITA_OK;
}

int ita_bind_dispatch(ita_handle h, int layer, int dispatch_dtype) {
  if (!h || !h->loaded) return fail(ITA_ERR_NO_WEIGHTS, "bind needs a context with weights");
  if (layer < 0 || layer >= h->hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "layer out of range");
  if (dispatch_dtype != ITA_DISPATCH_F16 && dispatch_dtype != ITA_DISPATCH_F32)
    return fail(ITA_ERR_INVALID_ARG, "bad dispatch dtype");
  std::lock_guard<std::mutex> g(g_bind_mu);
  g_bound = h;
  g_bound_layer = layer;
  g_bound_dtype = dispatch_dtype;
  return ITA_OK;
}

void ITASelfAttention_workgroup(const uint16_t* input, uint16_t* output) { (void)dispatch_host(input, output, false); }
void ITAFeedForward_workgroup(const uint16_t* input, uint16_t* output) { (void)dispatch_host(input, output, true); }

void ITASelfAttention_workgroup_expanded(const uint16_t* b0, const uint16_t* b0_aligned, size_t b0_offset, size_t,
                                         size_t, uint16_t* b1, uint16_t* b1_aligned, size_t b1_offset, size_t,
                                         size_t) {
  // memref descriptor: data = aligned + offset (elements); the reference falls back base -> aligned
  const uint16_t* in = b0_aligned ? b0_aligned : b0;
  uint16_t* out = b1_aligned ? b1_aligned : b1;
  if (!in || !out) { fail(ITA_ERR_INVALID_ARG, "null binding"); return; }
  size_t esz;
  {
    std::lock_guard<std::mutex> g(g_bind_mu);
    esz = g_bound_dtype == ITA_DISPATCH_F16 ? 2 : 4;
  }
  in = (const uint16_t*)((const char*)in + b0_offset * esz);
  out = (uint16_t*)((char*)out + b1_offset * esz);
  (void)dispatch_host(in, out, false);
}

}  // extern "C"

namespace {

float half_to_float(uint16_t hbits) {
  const uint32_t sign = (uint32_t)(hbits & 0x8000u) << 16;
  uint32_t exp = (hbits >> 10) & 0x1fu, man = hbits & 0x3ffu, out;
  if (exp == 0) {
    if (man == 0) out = sign;
    else {
      exp = 127 - 15 + 1;
      while (!(man & 0x400u)) { man <<= 1; --exp; }
      out = sign | (exp << 23) | ((man & 0x3ffu) << 13);
    }
  } else if (exp == 31) out = sign | 0x7f800000u | (man << 13);
  else out = sign | ((exp + 127 - 15) << 23) | (man << 13);
  float f;
  memcpy(&f, &out, 4);
  return f;
}
uint16_t float_to_half(float f) {   // round to nearest even
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  const uint32_t absx = x & 0x7fffffffu;
  if (absx >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (absx > 0x7f800000u ? 0x200u : 0));
  if (absx >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);            // overflow -> inf
  if (absx < 0x33000001u) return sign;                                    // underflow -> 0
  int exp = (int)(absx >> 23) - 127 + 15;
  uint32_t man = (absx & 0x7fffffu) | 0x800000u;
  int shift = 13;
  if (exp <= 0) { shift += 1 - exp; exp = 0; }
  uint32_t hm = man >> shift;
  const uint32_t rem = man & ((1u << shift) - 1), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (hm & 1))) ++hm;
  uint32_t outv = exp > 0 ? (((uint32_t)exp << 10) + (hm - 0x400u)) : hm;   // mantissa carry bumps the exponent
  return (uint16_t)(sign | outv);
}

// Host-buffer entry used by the reference's `void` symbols: 1 x 128 x E activation in, same out.
int dispatch_host(const uint16_t* in, uint16_t* out, bool ffn) {
  std::lock_guard<std::mutex> g(g_bind_mu);
  ita_context* c = g_bound;
  if (!c) return fail(ITA_ERR_NOT_BOUND, "ita_bind_dispatch has not been called");
  if (!in || !out) return fail(ITA_ERR_INVALID_ARG, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)128 * c->hdr.E;
  if (!c->dsp_in) {
    HIPCHK(hipMalloc(&c->dsp_in, n * sizeof(float)));
    HIPCHK(hipMalloc(&c->dsp_out, n * sizeof(float)));
    c->dsp_host.resize(n);
  }
  const float* src = (const float*)in;
  if (g_bound_dtype == ITA_DISPATCH_F16) {
    for (size_t i = 0; i < n; ++i) c->dsp_host[i] = half_to_float(in[i]);
    src = c->dsp_host.data();
  }
  HIPCHK(hipMemcpy(c->dsp_in, src, n * sizeof(float), hipMemcpyHostToDevice));
  int rc = ffn ? launch_ffn(c, g_bound_layer, c->dsp_in, c->dsp_out, 1, false, nullptr, nullptr)
               : launch_mha(c, g_bound_layer, c->dsp_in, c->dsp_out, 1, false, nullptr, nullptr);
  if (rc) return rc;
  if (g_bound_dtype == ITA_DISPATCH_F16) {
    HIPCHK(hipMemcpy(c->dsp_host.data(), c->dsp_out, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = float_to_half(c->dsp_host[i]);
  } else {
    HIPCHK(hipMemcpy(out, c->dsp_out, n * sizeof(float), hipMemcpyDeviceToHost));
  }
  tl_err = ITA_OK;
  return ITA_OK;
}

}  // namespace
