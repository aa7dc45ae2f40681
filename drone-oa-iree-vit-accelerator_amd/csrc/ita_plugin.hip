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
#include <thread>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/ita_mi355x.h"
#include "../../include/ita_weights.h"
#include "../../include/ita_wire.h"
#include "ita_f16x3_kernels.h"
#include "ita_lstm_head_kernel.h"
#include "ita_lstm_seq_kernel.h"
#include "ita_f32_kernels.h"
#include "ita_int8_kernels.h"
#include "ita_stream_kernel.h"
#include "ita_long_attn_kernel.h"
#include "ita_long_stats_kernel.h"
#include "ita_long_hist_kernel.h"
#include "ita_long_prop_kernel.h"
#include "ita_ffn_f32_kernel.h"
#include "ita_attn_f32_kernel.h"
#include "ita_long_f32_kernel.h"
#include "ita_long_f32_stats_kernel.h"
#include "ita_long_f32_prop_kernel.h"
#include "ita_ingest_kernel.h"
#include "ita_ingest_wire_kernel.h"
#include "ita_tokenizer_long_kernel.h"

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

// Every kernel launch of the plugin goes through launch / launch_lds.  Bytes is the kernel's dynamic LDS: what launch
// starts it with, and the most launch_lds may start it with.  Instantiating a launch with Bytes > 0 puts {kernel, Bytes}
// on a process-wide list during static initialisation, and ita_create raises the dynamic-LDS limit of every listed kernel
// on its device: a kernel that can be launched is registered by construction, on every device that has a handle, before
// its first launch (which may sit inside a stream capture).
struct LdsKernel { const void* kernel; int bytes; };
std::vector<LdsKernel>& lds_kernels() {
  static std::vector<LdsKernel> list;
  return list;
}
template <auto Kernel, int Bytes>
struct LdsListed {
  static inline const bool yes = (lds_kernels().push_back({reinterpret_cast<const void*>(Kernel), Bytes}), true);
};

constexpr int LDS_PER_CU = 160 * 1024;   // gfx950

template <auto Kernel, int Bytes, typename... Args>
int launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args&... args) {
  // An instantiation that asks for more than a CU has could never launch (hipFuncSetAttribute refuses it, and ita_create
  // would fail for every caller): it fails the build here instead of a user's call.
  static_assert(Bytes <= LDS_PER_CU, "this kernel instantiation asks for more LDS than a gfx950 CU has");
  if constexpr (Bytes > 0)
    (void)LdsListed<Kernel, Bytes>::yes;   // the ODR-use that instantiates the member, nothing at run time
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
  HIPCHK(hipGetLastError());
  return ITA_OK;
}
template <auto Kernel, int Bytes = 0, typename... Args>
int launch(dim3 grid, dim3 block, hipStream_t s, const Args&... args) {
  return launch_lds<Kernel, Bytes>(grid, block, Bytes, s, args...);
}

// f(std::integral_constant<int, 64 or 128>): the compile-time split over the two embedding widths
template <typename F>
int with_E(int E, F&& f) {
  return E == 64 ? f(std::integral_constant<int, 64>{}) : f(std::integral_constant<int, 128>{});
}

constexpr int K0P = 672;    // exact-f32 path: LSTM layer-0 concat width 517 + 128 = 645, padded to a multiple of 32
constexpr int K0S = 144;    // f16x3 path, LSTM layer 0 remainder: [h_in0 (128) | desvel | quat (4) | 0 pad]
// K of the folded GEMM = 128 tokens x E channels (8192 for ITAViTLSTM, 16384 for the E = 128 graph without a fusion
// tail); row stride of the x2 / Wfold planes = K + 64: a power-of-two stride (16 KB) would put every row of a K tile on
// the same L2 channel (Weights::kfold, Weights::ldfold)
constexpr int NSPLIT = 8;   // split-K of the folded GEMM (1024 x 512 x 8192 -> 256 workgroups)

// Owner of one device allocation.  Move-only; converts to T* so that kernel-argument structs and launch sites read as
// they would with a raw pointer.  Sizes are in elements.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p = o.p; o.p = nullptr; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  hipError_t alloc(size_t n) {
    reset();
    return hipMalloc(&p, n * sizeof(T));
  }
  hipError_t upload(const T* host, size_t n) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
  }
  operator T*() const { return p; }
};

// ---- the exact-f32 fusion tail and GEMM: the forward's tail mode 0, and what the fold is computed with at load time
int launch_tail(int num_cus, int E, const float* wT, const float* bias, const float* x, float* feat, int ld, int B,
                hipStream_t s) {
  if (!wT) return fail(ITA_ERR_BAD_BLOB, "fusion-tail parameters missing from the blob");
  if (E != 64) return fail(ITA_ERR_UNSUPPORTED, "fusion tail is built for E = 64 (ITAViTLSTM)");
  ItaTailArgs a{x, wT, bias, feat, ld, B};
  const int grid = B < 2 * num_cus ? B : 2 * num_cus;
  return launch<ita_tail_kernel<64>, ita_tail_lds_bytes<64>()>(dim3(grid), dim3(256), s, a);
}

int launch_gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N,
                int K, hipStream_t s) {
  if (N % 64 || K % 32) return fail(ITA_ERR_UNSUPPORTED, "gemm needs N % 64 == 0 and K % 32 == 0");
  ItaGemmArgs g{A, lda, W, ldw, bias, C, ldc, M, N, K};
  return launch<ita_gemm_f32_kernel>(dim3(N / 64, (M + 31) / 32), dim3(256), s, g);
}

}  // namespace

#include "ita_weights_load.h"

namespace {

// Everything ensure_workspace allocates, for `cap` frames.
struct Workspace {
  int cap = 0;
  int front_cap[ITA_PART_BUFFERS] = {};   // workspace capacity when ita_vitlstm_front filled partial buffer i
  DevBuf<float> bufA, bufB, cat0, cat1, cat2, gates, feat;
  // the f16x3 path
  DevBuf<_Float16> x2_hi, x2_lo, c1_hi, c1_lo, c2_hi, c2_lo;
  DevBuf<float> part;
  // the LSTM head's meeting words (ita_lstm_head_kernel): [0] device error word, then one arrival counter per 32-frame
  // tile every ITA_HEAD_CNT_STRIDE words; zeroed at allocation, re-armed in-kernel by each tile's last workgroup and by
  // ita_head_status
  DevBuf<unsigned> head_sync;
  size_t head_sync_bytes = 0;
  DevBuf<char> seq_ho;          // ita_lstm_seq_kernel's hand-off buffers: ITA_SEQ_TILE bytes per 32-stream tile
};

// What ita_fusion_tail_load builds: the fusion tail on large token grids (ita_fusion_tail_large, BASELINE config 5)
struct TailLarge {
  DevBuf<_Float16> hi, lo;         // [chunks][9][nt*16][32]
  DevBuf<_Float16> up_hi, up_lo;   // upsample branch by linearity (ita_tail_up_kernel): [9][4][3][64][8], E = 128 only
  DevBuf<_Float16> ps_hi, ps_lo;   // its phase 2, the pixel-shuffle channels: [9][48][32] (48 rows whatever out_ch is)
  DevBuf<float> bias;
  float inv_scale = 1.0f;
  int E = 0, CO = 0, nt = 0, nchunk = 0;
};

// The device tables of one source size of ita_ingest_wire (ita_ingest_wire_prepare)
struct WireSize {
  int H = 0, W = 0;                // 0: the slot is free
  DevBuf<int> idx;                 // n0y[60] | cnty[60] | n0x[90] | cntx[90]
  DevBuf<float> coeff;             // wy[60][ldy] | wx transposed [ldx][90]
  ItaWireTables dev{};
  int span[3] = {};                // source rows the widest band of 4 / 8 / 12 output rows needs (the staged kernel's LDS)
};
constexpr int ITA_WIRE_SIZES = 8;

}  // namespace

// Device memory is grouped by lifetime: `w` per ita_load_weights, `ws` per workspace capacity, `tl` per
// ita_fusion_tail_load; what follows them lives as long as the handle.  Assigning a fresh value releases a group.
struct ita_context {
  int device = 0;
  int num_cus = 256;
  Weights w;
  Workspace ws;
  bool ws_reserved = false;     // ita_reserve was called: the workspace is pinned (see ensure_workspace); a load keeps it
  TailLarge tl;
  int tail_mode = 1;            // 1: folded f16x3 GEMMs (default), 0: exact f32 kernels
  // per-stage profiling (ita_profile_begin / _end)
  bool prof = false;
  int prof_max = 0, prof_n = 0;
  int prof_every = 1, prof_stage = -1, prof_calls = 0;   // sample every n-th forward; -1 = all stages, else one stage
  std::vector<hipEvent_t> prof_ev;   // per recorded forward: 1 + 1 + 2*L + 3 events
  std::vector<hipEvent_t> pipe_ev;   // ita_vitlstm_pipelined: front-done / back-done rings + fork/join
  DevBuf<float> pipe_h;              // ita_vitlstm_pipelined: second copy of (h, c), 2 x (3, pipe_cap, 128)
  int pipe_cap = 0;
  // long-sequence attention (ita_mha_long_q8): Q fragments, K / V^T images, column sums; the float entries' K / V images
  // and, behind them, ita_mha_long_f32_stats' column partials; grown on demand
  DevBuf<char> long_ws;
  size_t long_ws_bytes = 0;
  // ita_mha_long_int8_taps: the row table (token -> output row, or -1), ITA_LONG_MAX_SEQ entries, and its host copy
  DevBuf<int> long_rows;
  std::vector<int> long_rows_host;
  // ita_mha_long_f32_taps: row_max | row_sum of a call that asks for probs without them, 2 x batch x n_rows; grown on demand
  DevBuf<float> long_rowstat;
  size_t long_rowstat_n = 0;
  // staging for the host-buffer drop-in symbols
  DevBuf<float> dsp_in, dsp_out;
  std::vector<float> dsp_host;
  // ita_ingest_wire: the last ITA_WIRE_SIZES source sizes prepared; a new one beyond that replaces the oldest
  WireSize wire[ITA_WIRE_SIZES];
  int wire_next = 0;
};

namespace {

std::mutex g_bind_mu;
ita_handle g_bound = nullptr;
int g_bound_layer = 0;
int g_bound_dtype = ITA_DISPATCH_F16;

bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// Frees and reallocates every buffer of the workspace, for B frames
int grow_workspace(ita_context* c, int B) {
  c->ws = Workspace{};
  Workspace& ws = c->ws;
  const size_t E = (size_t)c->w.hdr.E, nb = (size_t)B, ntile = (nb + 31) / 32;
  HIPCHK(ws.bufA.alloc(nb * 128 * E));
  HIPCHK(ws.bufB.alloc(nb * 128 * E));
  HIPCHK(ws.feat.alloc(nb * 4608));
  HIPCHK(ws.cat0.alloc(nb * K0P));
  HIPCHK(ws.cat1.alloc(nb * 256));
  HIPCHK(ws.cat2.alloc(nb * 256));
  HIPCHK(ws.gates.alloc(nb * 512));
  HIPCHK(ws.x2_hi.alloc(2 * nb * c->w.ldfold));   // two sets of planes: ita_vitlstm_encode / _fold ping-pong
  HIPCHK(ws.x2_lo.alloc(2 * nb * c->w.ldfold));
  for (DevBuf<_Float16>* b : {&ws.c1_hi, &ws.c1_lo, &ws.c2_hi, &ws.c2_lo})
    HIPCHK(b->alloc(ntile * 32 * 256));           // fragment order, whole 32-frame tiles
  HIPCHK(ws.part.alloc(ITA_PART_BUFFERS * (size_t)NSPLIT * nb * 512));   // ita_vitlstm_front/back
  ws.head_sync_bytes = sizeof(unsigned) * ITA_HEAD_CNT_STRIDE * (1 + ntile);
  HIPCHK(ws.head_sync.alloc(ITA_HEAD_CNT_STRIDE * (1 + ntile)));
  HIPCHK(hipMemset(ws.head_sync, 0, ws.head_sync_bytes));
  HIPCHK(ws.seq_ho.alloc((size_t)ITA_SEQ_TILE * ntile));   // 3 KB per frame, whether or not the sequence form is used
  HIPCHK(hipDeviceSynchronize());
  ws.cap = B;
  return ITA_OK;
}

// Growth is only allowed while nothing can still reference the old buffers: never after an explicit ita_reserve (HIP
// graphs and front/back pairs keep raw pointers into the workspace), and never on a stream that is being captured.
int ensure_workspace(ita_context* c, int B, hipStream_t s) {
  if (B <= c->ws.cap) return ITA_OK;
  if (c->ws_reserved)
    return fail(ITA_ERR_INVALID_ARG, "batch exceeds the workspace pinned by ita_reserve; call ita_reserve(max_batch) again while idle");
  if (capturing(s))
    return fail(ITA_ERR_INVALID_ARG, "the workspace cannot grow inside a stream capture; call ita_reserve first");
  return grow_workspace(c, B);
}

int check(ita_handle h, int batch, bool need_weights = true) {
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (batch <= 0) return fail(ITA_ERR_INVALID_ARG, "batch must be positive");
  if (need_weights && !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "ita_load_weights has not been called");
  HIPCHK(hipSetDevice(h->device));
  return ITA_OK;
}

// check(), then what every per-layer entry point asks of its activation pointers and layer index
int check_layer_io(ita_handle h, int layer, const void* x, const void* y, int batch) {
  if (int rc = check(h, batch)) return rc;
  if (!x || !y || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  return ITA_OK;
}

ItaMhaArgs mha_args(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, const ita_mha_taps* t) {
  const Layer& L = c->w.layers[layer];
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

// event indices of a profiling stage's first and last mark among the events of one recorded forward
struct StageMarks { int lo, hi; };
StageMarks stage_marks(int num_layers, int stage) {
  const int L2 = 2 * num_layers;
  const int lo[ITA_NUM_STAGES] = {0, 1, 1, 1 + L2, 2 + L2, 3 + L2}, hi[ITA_NUM_STAGES] = {1, 1 + L2, 1 + L2, 2 + L2, 3 + L2, 4 + L2};
  return {lo[stage], hi[stage]};
}

// The profiling marks of one call between ita_profile_begin and ita_profile_end: the call's slice of prof_ev (null when
// the call is not sampled), the selected stage and the index of the next mark.  An event in the stream costs a pipeline
// bubble of ~5 us (the next kernel cannot be launched under the tail of the previous one), so in single-stage mode only
// that stage's two marks are recorded.
struct StageRecorder {
  ita_context* h;
  hipStream_t s;
  hipEvent_t* ev = nullptr;
  int stage, lo, hi;     // the marks that close the count: the selected stage's two, or (all stages) the first and the last
  int next = 0;          // mark(): a whole forward numbers its marks as it goes
  unsigned seen = 0;     // bit 0: lo was recorded, bit 1: hi
  // events of one recorded forward: forward start, tokenizer end, two per layer, tail, decoder, LSTM + fc
  static int events_per_forward(const ita_context* h) { return 5 + 2 * h->w.hdr.num_layers; }

  // all_stages_too: the call runs every stage (a front half is sampled in single-stage mode only)
  StageRecorder(ita_context* h_, hipStream_t s_, bool all_stages_too) : h(h_), s(s_), stage(h_->prof_stage) {
    const int per = events_per_forward(h);
    const StageMarks m = stage >= 0 ? stage_marks(h->w.hdr.num_layers, stage) : StageMarks{0, per - 1};
    lo = m.lo;
    hi = m.hi;
    if (h->prof && (all_stages_too || stage >= 0) && h->prof_n < h->prof_max && (h->prof_calls++ % h->prof_every) == 0)
      ev = &h->prof_ev[(size_t)h->prof_n * per];
  }
  int record(int i) {
    HIPCHK(hipEventRecord(ev[i], s));
    seen |= (i == lo ? 1u : 0u) | (i == hi ? 2u : 0u);
    return ITA_OK;
  }
  int mark() {   // the next mark of a whole forward
    const int i = next++;
    return ev && (stage < 0 || i == lo || i == hi) ? record(i) : ITA_OK;
  }
  int mark(int st, bool end) {   // a front half: the start or end mark of stage st, when that is the selected stage
    return ev && stage == st ? record(end ? hi : lo) : ITA_OK;
  }
  // the slot counts as a forward only when both closing marks were recorded in this call
  void finish() { if (ev && seen == 3u) ++h->prof_n; }
};

// What one encoder layer (launch_encoder) or one stream-kernel launch (launch_stream) reads and writes
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
  StageRecorder* mid = nullptr;   // launch_encoder: marks the attention / FFN boundary of a layer that runs as two launches
};

// the stream kernel's instantiations without stamps; `fast` picks the single-rounding one (all six sites proven: fast_site_ok),
// `fused` the one-fma one (a.image then holds the layer's own accumulator bases: Layer::fused)
template <int E, bool FFN, int TOK, bool IO8>
int launch_stream_kernel(bool fast, int fused, dim3 grid, hipStream_t s, const ItaStreamArgs& a) {
  constexpr int lds = ItaStreamLds<E, FFN, TOK != 0>::TOTAL;
  if constexpr (FFN) {
    if (fused == 3) return launch<ita_stream_kernel<E, FFN, TOK, false, IO8, true, 3>, lds>(grid, dim3(512), s, a);
    if (fused == 2) return launch<ita_stream_kernel<E, FFN, TOK, false, IO8, true, 2>, lds>(grid, dim3(512), s, a);
  }
  if (fused) return launch<ita_stream_kernel<E, FFN, TOK, false, IO8, true, 1>, lds>(grid, dim3(512), s, a);
  return fast ? launch<ita_stream_kernel<E, FFN, TOK, false, IO8, true>, lds>(grid, dim3(512), s, a)
              : launch<ita_stream_kernel<E, FFN, TOK, false, IO8, false>, lds>(grid, dim3(512), s, a);
}

// mode 0: whole encoder layer; 1: attention block only (fuse_ln: + residual + LayerNorm1)
int launch_stream(ita_context* c, int layer, int mode, bool fuse_ln, const StreamIo& io, int B, hipStream_t s) {
  const Layer& L = c->w.layers[layer];
  if (L.attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): it has no int8 stream kernel");
  ItaStreamArgs a{};
  a.x = io.x; a.y = io.y; a.y_hi = io.y_hi; a.y_lo = io.y_lo; a.ld_planes = c->w.ldfold; a.x1_tap = io.x1_tap;
  a.inv_sx = L.ascal[ITA_A_INV_SX]; a.mq = L.ascal[ITA_A_MQ]; a.mk = L.ascal[ITA_A_MK]; a.mv = L.ascal[ITA_A_MV];
  a.ml = L.ascal[ITA_A_ML]; a.mc = L.ascal[ITA_A_MC]; a.mo = L.ascal[ITA_A_MO]; a.so = L.ascal[ITA_A_SO];
  a.f_inv_sx = L.fscal[ITA_F_INV_SX]; a.m1 = L.fscal[ITA_F_M1]; a.m2 = L.fscal[ITA_F_M2]; a.s2 = L.fscal[ITA_F_S2];
  a.B = B; a.fuse_ln = fuse_ln ? 1 : 0;
  a.stamps = io.stamps; a.h0_src = io.h0_src; a.h0_dst = io.h0_dst; a.slots = io.slots;
  a.img = io.img; a.tok_tap = io.tok_tap; a.xq = io.xq; a.yq = io.yq;
  a.fast_sites = L.fast_sites;
  const dim3 grid(B < c->num_cus ? B : c->num_cus), block(512);
  const bool fast = L.fast_sites == ITA_SITES_ALL;
  // the fused form: its own images, and the constants of its five sites
  // (2: fc1 as well, 3: and the dequantise sites out_proj and fc2 -- the whole-layer flavours, the others launch 1)
  const int fused = (L.fused && !io.stamps) ? (L.fused_dq ? 3 : L.fused_relu ? 2 : 1) : 0;
  if (fused) {
    a.mkq = {a.mq, L.fused_k[0]}; a.mkk = {a.mk, L.fused_k[1]}; a.mkv = {a.mv, L.fused_k[2]}; a.mkl = {a.ml, L.fused_k[3]};
    a.mkc = {a.mc, L.fused_k[4]}; a.mk1 = {a.m1, L.fused_k[5]}; a.mko = {a.mo, L.fused_k[6]}; a.mk2 = {a.m2, L.fused_k[7]};
    a.c_l = L.fused_c[3]; a.c_c = L.fused_c[4];
  }
  if (mode == 2) {
    if (!L.simg_mha) return fail(ITA_ERR_UNSUPPORTED, "this layer has no attention image (accumulator range, or more than one head)");
    a.image = fused ? L.fimg_mha : L.simg_mha;
    return with_E(c->w.hdr.E, [&](auto e) { return launch_stream_kernel<decltype(e)::value, false, 0, true>(fast, fused, grid, s, a); });
  }
  if (mode == 1) {
    if (!L.simg_mha) return fail(ITA_ERR_BAD_BLOB, "attention image missing");
    if (fuse_ln && !L.n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
    a.image = fused ? L.fimg_mha : L.simg_mha;
    return with_E(c->w.hdr.E, [&](auto e) { return launch_stream_kernel<decltype(e)::value, false, 0, false>(fast, fused, grid, s, a); });
  }
  if (io.img) {
    if (!L.simg_tok) return fail(ITA_ERR_BAD_BLOB, "tokenizer / LayerNorm parameters missing from the blob");
    a.image = fused ? L.fimg_tok : L.simg_tok;
    if (io.stamps) return launch<ita_stream_kernel<64, true, 1, true>, ItaStreamLds<64, true, true>::TOTAL>(grid, block, s, a);
    return launch_stream_kernel<64, true, 1, false>(fast, fused, grid, s, a);
  }
  if (!L.simg_enc) return fail(ITA_ERR_BAD_BLOB, "LayerNorm parameters missing from the blob");
  a.image = fused ? L.fimg_enc : L.simg_enc;
  if (c->w.hdr.E == 128) {   // attention + FFN of an E = 128 layer in one launch; fc1 / fc2 weights are read from the global image
    if (io.stamps) return fail(ITA_ERR_UNSUPPORTED, "phase stamps are built for the E = 64 encoder");
    return launch_stream_kernel<128, true, 0, false>(fast, fused, grid, s, a);
  }
  if (io.stamps) return launch<ita_stream_kernel<64, true, 0, true>, ItaStreamLds<64, true, false>::TOTAL>(grid, block, s, a);
  return launch_stream_kernel<64, true, 0, false>(fast, fused, grid, s, a);
}

int launch_mha_stream(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s) {
  StreamIo io;
  io.x = x; io.y = y;
  return launch_stream(c, layer, 1, fuse, io, B, s);
}

// the attention block: without taps on the stream kernel (weights resident in LDS, activations chained through
// registers); with taps, or for a layer without an LDS image (accumulator range, or H > 1 heads), on the tile-phased
// kernel that can expose every tensor and is instantiated per head count
int launch_mha(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, const ita_mha_taps* t,
               hipStream_t s) {
  if (c->w.layers[layer].attn_f32)
    return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): ita_mha_f32 runs it");
  if (fuse && !c->w.layers[layer].n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
  if (!t && c->w.layers[layer].simg_mha) return launch_mha_stream(c, layer, x, y, B, fuse, s);
  const ItaMhaArgs a = mha_args(c, layer, x, y, B, fuse, t);
  const int grid = B < c->num_cus ? B : c->num_cus;
  return with_E(c->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    switch (c->w.hdr.H) {   // (check_blob admits these five)
      case 1: return launch<ita_mha_kernel<E, 1>, ItaMhaLds<E>::TOTAL>(dim3(grid), dim3(512), s, a);
      case 2: return launch<ita_mha_kernel<E, 2>, ItaMhaLds<E>::TOTAL>(dim3(grid), dim3(512), s, a);
      case 3: return launch<ita_mha_kernel<E, 3>, ItaMhaLds<E>::TOTAL>(dim3(grid), dim3(512), s, a);
      case 4: return launch<ita_mha_kernel<E, 4>, ItaMhaLds<E>::TOTAL>(dim3(grid), dim3(512), s, a);
      case 6: return launch<ita_mha_kernel<E, 6>, ItaMhaLds<E>::TOTAL>(dim3(grid), dim3(512), s, a);
    }
    return fail(ITA_ERR_UNSUPPORTED, "the attention kernel is built for H in {1,2,3,4,6}");
  });
}

int launch_ffn(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, const ita_ffn_taps* t,
               hipStream_t s, _Float16* y_hi = nullptr, _Float16* y_lo = nullptr) {
  const Layer& L = c->w.layers[layer];
  if (L.ffn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's FFN is float32 (ITAW0002 blob): ita_ffn_f32 runs it");
  if (fuse && !L.n2w) return fail(ITA_ERR_BAD_BLOB, "norm2 parameters missing from the blob");
  ItaFfnArgs a{};
  a.x = x; a.y = y; a.w1 = L.w1; a.w2 = L.w2; a.b1 = L.b1; a.b2 = L.b2;
  a.inv_sx = L.fscal[ITA_F_INV_SX]; a.m1 = L.fscal[ITA_F_M1]; a.m2 = L.fscal[ITA_F_M2]; a.s2 = L.fscal[ITA_F_S2];
  a.ln_w = L.n2w; a.ln_b = L.n2b; a.B = B; a.fuse_ln = fuse ? 1 : 0;
  if (t) { a.t_xq = t->x_q; a.t_h = t->h; a.t_out = t->out_q; }
  a.y_hi = y_hi; a.y_lo = y_lo; a.ld_planes = c->w.ldfold;
  const int grid = B < 2 * c->num_cus ? B : 2 * c->num_cus;
  return with_E(c->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    return launch<ita_ffn_kernel<E>, ItaFfnLds<E>::TOTAL>(dim3(grid), dim3(512), s, a);
  });
}

// the float32 FFN (ita_ffn_f32_kernel.h) of an ITAW0002 layer, fuse: + residual + LayerNorm2
int launch_ffn_f32(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s,
                   _Float16* y_hi = nullptr, _Float16* y_lo = nullptr, const float* h0_src = nullptr, float* h0_dst = nullptr,
                   const int* slots = nullptr) {
  const Layer& L = c->w.layers[layer];
  if (!L.ffn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's FFN is int8 (ITAW0001 blob): ita_ffn_int8 runs it");
  if (c->w.hdr.E != 64 && !L.w1p) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN of an ITAW0002 blob is built for E = 64");
  if (fuse && !L.n2w) return fail(ITA_ERR_BAD_BLOB, "norm2 parameters missing from the blob");
  ItaFfnF32Args a{};
  a.x = x; a.y = y; a.w1 = L.w1f; a.b1 = L.b1f; a.w2 = L.w2f; a.b2 = L.b2f; a.ln_w = L.n2w; a.ln_b = L.n2b;
  a.B = B; a.fuse_ln = fuse ? 1 : 0;
  a.y_hi = y_hi; a.y_lo = y_lo; a.ld_planes = c->w.ldfold;
  a.h0_src = h0_src; a.h0_dst = h0_dst; a.slots = slots;
  if (c->w.hdr.E != 64) { a.w1 = L.w1p; a.w2 = L.w2p; }   // E = 128: the weights stream as fragment images (66 KB of LDS: two workgroups per CU)
  const int cap = 2 * c->num_cus;
  return with_E(c->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    const int ntile = B * (128 / ItaFfnF32Lds<E>::TT);
    return launch<ita_ffn_f32_kernel<E>, ItaFfnF32Lds<E>::TOTAL>(dim3(ntile < cap ? ntile : cap), dim3(256), s, a);
  });
}

// the float32 attention block (ita_attn_f32_kernel.h) of an ITAW0003 layer, fuse: + residual + LayerNorm1
int launch_attn_f32(ita_context* c, int layer, const float* x, float* y, int B, bool fuse, hipStream_t s) {
  const Layer& L = c->w.layers[layer];
  if (!L.attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is int8 (ITAW0001 / ITAW0002 blob): ita_mha_int8 runs it");
  if (fuse && !L.n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
  ItaAttnF32Args a{};
  a.x = x; a.y = y;
  a.wq = L.wqf; a.wk = L.wkf; a.wv = L.wvf; a.bq = L.bqf; a.bk = L.bkf; a.bv = L.bvf; a.wo = L.wof; a.bo = L.bof;
  a.ln_w = L.n1w; a.ln_b = L.n1b; a.B = B; a.fuse_ln = fuse ? 1 : 0;
  // 130 KB (E = 64) / 96 KB (E = 128) of LDS: one workgroup per CU, frames in a grid stride
  return with_E(c->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    return launch<ita_attn_f32_kernel<E>, ItaAttnF32Lds<E>::TOTAL>(dim3(B < c->num_cus ? B : c->num_cus), dim3(512), s, a);
  });
}

// One encoder layer: the stream kernel (ita_stream_kernel.h) when the layer has an LDS image -- one head and every
// accumulator provably inside the biased-float range (stream_range_ok) -- else the two block kernels through bufB.
// A float-FFN layer (ITAW0002) is always two launches: the attention block with the fused residual + LayerNorm1 into bufB
// (stream kernel mode 1, or ita_mha_kernel for a layer without an attention image), then ita_ffn_f32_kernel; io.mid,
// when given, takes its next mark between the two (the profiler's stage-2 mark).  A float layer (ITAW0003) is the same
// two launches with ita_attn_f32_kernel as the first.
int launch_encoder(ita_context* c, int layer, const StreamIo& io, int B, hipStream_t s) {
  const Layer& L = c->w.layers[layer];
  if (!L.n1w || !L.n2w) return fail(ITA_ERR_BAD_BLOB, "LayerNorm parameters missing from the blob");
  const size_t x1_bytes = sizeof(float) * (size_t)B * 128 * c->w.hdr.E;
  if (L.ffn_f32) {
    if (io.img || io.stamps) return fail(ITA_ERR_UNSUPPORTED, "a float-FFN layer runs behind the stand-alone tokenizer, without stamps");
    if (c->w.hdr.E != 64 && !L.w1p) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN of an ITAW0002 blob is built for E = 64");
    int rc = ensure_workspace(c, B, s);
    if (rc) return rc;
    if ((rc = L.attn_f32 ? launch_attn_f32(c, layer, io.x, c->ws.bufB, B, true, s)
                         : launch_mha(c, layer, io.x, c->ws.bufB, B, true, nullptr, s))) return rc;
    if (io.x1_tap) HIPCHK(hipMemcpyAsync(io.x1_tap, c->ws.bufB, x1_bytes, hipMemcpyDeviceToDevice, s));
    if (io.mid && (rc = io.mid->mark())) return rc;
    return launch_ffn_f32(c, layer, c->ws.bufB, io.y, B, true, s, io.y_hi, io.y_lo, io.h0_src, io.h0_dst, io.slots);
  }
  if (io.img ? L.simg_tok != nullptr : L.simg_enc != nullptr) return launch_stream(c, layer, 0, false, io, B, s);
  if (io.img) return fail(ITA_ERR_INVALID_ARG, "launch_encoder: frames need the tokenizer image");
  // (everything that can refuse is checked before the first launch: no partial work is left behind an error)
  if (io.h0_dst && io.slots) return fail(ITA_ERR_UNSUPPORTED, "slot-indexed state needs the stream kernel (this blob's accumulator range or head count rules it out)");
  int rc = ensure_workspace(c, B, s);
  if (rc) return rc;
  if ((rc = launch_mha(c, layer, io.x, c->ws.bufB, B, true, nullptr, s))) return rc;
  if (io.x1_tap) HIPCHK(hipMemcpyAsync(io.x1_tap, c->ws.bufB, x1_bytes, hipMemcpyDeviceToDevice, s));
  if (io.h0_dst)   // the side copy the stream kernel makes for the LSTM
    HIPCHK(hipMemcpyAsync(io.h0_dst, io.h0_src, sizeof(float) * (size_t)B * 128, hipMemcpyDeviceToDevice, s));
  return launch_ffn(c, layer, c->ws.bufB, io.y, B, true, nullptr, s, io.y_hi, io.y_lo);
}

// frames into the E = 64 model: the tokenizer runs inside the first encoder layer's kernel
// (ITA_SPLIT_TOKENIZER=1 keeps the separate ita_tok_stream_kernel launch, for comparison)
bool fuse_tokenizer(const ita_context* c, int image_dtype) {
  static const bool split = getenv("ITA_SPLIT_TOKENIZER") != nullptr;
  // f32 frames go through the stand-alone tokenizer: the stream kernel's private pixel windows are sized for bytes
  return !split && image_dtype == ITA_IMAGE_U8 && !c->w.layers.empty() && c->w.layers[0].simg_tok;
}

int launch_tokenizer(ita_context* c, const void* img, int dtype, float* tokens, int B, hipStream_t s) {
  // (the image exists when the blob has the conv weights and bias and the LayerNorm: ita_load_weights)
  if (!c->w.tok_simg) return fail(ITA_ERR_BAD_BLOB, "tokenizer parameters missing from the blob");
  const bool u8 = dtype == ITA_IMAGE_U8;
  ItaTokStreamArgs ta{c->w.tok_simg + (u8 ? 0 : c->w.tok_simg_bytes), img, tokens, B};
  const int g = B < 2 * c->num_cus ? B : 2 * c->num_cus;   // 35 KB of LDS, <= 128 registers: two workgroups per CU
  return with_E(c->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    return u8 ? launch<ita_tok_stream_kernel<E, true>, ItaTokStreamLds<E, true>::TOTAL>(dim3(g), dim3(512), s, ta)
              : launch<ita_tok_stream_kernel<E, false>, ItaTokStreamLds<E, false>::TOTAL>(dim3(g), dim3(512), s, ta);
  });
}

template <int NT, int WAVES, int TPS>
int launch_tail_big_w(const ItaTailBigArgs& a, hipStream_t s) {
  return launch<ita_tail_big_kernel<NT, WAVES, TPS>, ItaTailBigLds<NT, WAVES, TPS>::TOTAL>(
      dim3(2 * a.TW / 32, 2 * a.TH / (2 * WAVES), a.B), dim3(64 * WAVES), s, a);
}
// 16-row tiles on 8 waves with a whole chunk's weights resident when the map height allows (measured best:
// 0.61 ms for 32 frames of BASELINE config 5); else 8-row tiles on 4 waves with a third of the chunk's taps
// resident (70 KB of LDS, two workgroups per CU: 0.66 ms).  More than 48 output channels (NT = 4) always take the
// 8-row form (76256 bytes, still two workgroups per CU; the map height is a multiple of 8 by ita_fusion_tail_large's
// own check): <4, 8, 9> would need 166752 bytes, more than a CU has.
template <int NT>
int launch_tail_big(const ItaTailBigArgs& a, hipStream_t s) {
  if constexpr (NT < 4)
    if ((2 * a.TH) % 16 == 0) return launch_tail_big_w<NT, 8, 9>(a, s);
  return launch_tail_big_w<NT, 4, 3>(a, s);
}

template <int BM, int BN, int WM, int WN>
int launch_gemm_split(const _Float16* a_hi, const _Float16* a_lo, int lda, const _Float16* w_hi, const _Float16* w_lo,
                      int ldw, float* out, int M, int N, int K, int nsplit, hipStream_t s, const _Float16* wf_hi = nullptr,
                      const _Float16* wf_lo = nullptr) {
  if (N % BN || K % (64 * nsplit)) return fail(ITA_ERR_UNSUPPORTED, "split gemm shape");
  static const int dbg = getenv("ITA_GEMM_DBG") ? atoi(getenv("ITA_GEMM_DBG")) : 0;
  ItaGemmSplitArgs g{a_hi, a_lo, lda, w_hi, w_lo, ldw, out, M, N, K, nsplit, dbg, wf_hi, wf_lo};
  if (M <= 32 && N % 32 == 0 && wf_hi && wf_lo)   // one M tile: one wave per 32 x 32 tile and K slice
    return M <= 16 ? launch<ita_gemm_f16x3_tiny_kernel<1>>(dim3(N / 32, 1, nsplit), dim3(64), s, g)
                   : launch<ita_gemm_f16x3_tiny_kernel<2>>(dim3(N / 32, 1, nsplit), dim3(64), s, g);
  if (M <= 256 && N % 32 == 0) {   // a few M tiles: four-wave workgroups share the staging, same arithmetic
    // M tiles per workgroup: up to four (128 frames: 128 workgroups).  Fewer tiles per workgroup fill the chip -- MT = ceil(M / 64)
    // gives 256 workgroups from 64 frames on and the kernel alone gets 1.4-2.9 us faster (64 / 128 frames, one stream) -- but in
    // the three-branch graph schedule that bench.py uses at these sizes a 256-workgroup GEMM leaves no CU to the LSTM branch
    // and the step gets SLOWER (128 frames: 36.6 -> 38.3 us).  Per output element the arithmetic does not depend on MT.
    const int mt = M >= 128 ? 4 : (M + 31) / 32;
    const dim3 grid((N / 32) * nsplit, (M + 32 * mt - 1) / (32 * mt));
    switch (mt) {
      case 1: return launch<ita_gemm_f16x3_small_kernel<1>, ita_gemm_small_lds(1)>(grid, dim3(256), s, g);
      case 2: return launch<ita_gemm_f16x3_small_kernel<2>, ita_gemm_small_lds(2)>(grid, dim3(256), s, g);
      case 3: return launch<ita_gemm_f16x3_small_kernel<3>, ita_gemm_small_lds(3)>(grid, dim3(256), s, g);
      default: return launch<ita_gemm_f16x3_small_kernel<4>, ita_gemm_small_lds(4)>(grid, dim3(256), s, g);
    }
  }
  return launch<ita_gemm_f16x3_kernel<BM, BN, WM, WN>, ItaGemmSplitLds<BM, BN>::TOTAL>(
      dim3((N / BN) * ((M + BM - 1) / BM) * nsplit), dim3(64 * WM * WN), s, g);
}

template <typename T>
int launch_ingest(ita_context* c, const void* src, int H, int W, long long row_stride, long long frame_stride,
                  float depth_scale, float* frames, int batch, hipStream_t s) {
  const float scale_y = (float)H / (float)ITA_INGEST_H, scale_x = (float)W / (float)ITA_INGEST_W;   // host IEEE divisions
  const int row_bytes = W * (int)sizeof(T);
  if (W >= 2 * ITA_INGEST_W && row_bytes <= ITA_INGEST_ROW_BYTES) {
    const long long items = (long long)batch * (ITA_INGEST_H / 4);
    const int grid = (int)std::min<long long>(items, (long long)c->num_cus * 8);
    // (at most ITA_INGEST_ROW_BYTES a row: within the LDS any kernel may ask for, nothing to register)
    return launch_lds<ita_ingest_rows_kernel<T>, 0>(dim3(grid), dim3(256), ita_ingest_rows_lds_total(row_bytes), s, (const T*)src, H, W,
                                                    row_stride, frame_stride, scale_y, scale_x, depth_scale, frames, batch);
  }
  const long long blocks = ((long long)batch * ITA_INGEST_H * ITA_INGEST_W + 255) / 256;
  const int grid = (int)std::min<long long>(blocks, (long long)c->num_cus * 8);
  return launch<ita_ingest_gather_kernel<T>>(dim3(grid), dim3(256), s, (const T*)src, H, W, row_stride, frame_stride, scale_y, scale_x,
                                             depth_scale, frames, batch);
}

// the source frames ita_ingest and ita_ingest_wire accept; no handle and no HIP call is involved
static_assert(ITA_INGEST_MAX_DIM == 4096 && ITA_WIRE_MAX_DIM == 4096, "one size rule, one message");
int check_frames(int height, int width, long long row_stride, long long frame_stride, int batch) {
  if (height < 1 || height > 4096 || width < 1 || width > 4096) return fail(ITA_ERR_INVALID_ARG, "height and width must be in [1, 4096]");
  if (batch < 1) return fail(ITA_ERR_INVALID_ARG, "batch must be positive");
  if (row_stride < width || frame_stride < (long long)(height - 1) * row_stride + width)
    return fail(ITA_ERR_INVALID_ARG, "row_stride < width, or frame_stride < (height - 1) * row_stride + width (strides are in pixels)");
  if (row_stride > (1ll << 40) || frame_stride > (1ll << 40)) return fail(ITA_ERR_INVALID_ARG, "stride out of range");
  return ITA_OK;
}

// whether every 16-token tile of a token row needs at most ITA_TOK_LONG_WIN_W pixel columns: from 2 x0 - 3 of its first token
// to 2 (x0 + xp) + 3 of its last (x0 and x0 + xp do not decrease along a row).  The kernel's own function on the host: the
// same float expressions give the same integers.
bool tok_long_window_fits(float scale_x, int CW, int tok_w) {
  for (int ox = 0; ox < tok_w; ox += 16) {
    int xf, xl, pf, pl;
    float l;
    bilinear_src_dev(ox, scale_x, CW, xf, pf, l);
    bilinear_src_dev(ox + 15, scale_x, CW, xl, pl, l);
    if (2 * (xl + pl - xf) + 7 > ITA_TOK_LONG_WIN_W) return false;
  }
  return true;
}

// ita_tokenizer_long's launch: persistent 512-thread workgroups, each round takes eight consecutive (frame, 16-token tile) items
template <typename T>
int launch_tokenizer_long(ita_context* c, const void* src, int H, int W, long long row_stride, long long frame_stride,
                          float depth_scale, int tok_h, int tok_w, float* tokens, int batch, hipStream_t s) {
  const int CH = (H - 1) / 2 + 1, CW = (W - 1) / 2 + 1;
  ItaTokLongArgs a{c->w.tok_simg + c->w.tok_simg_bytes, src, tokens, row_stride, frame_stride,
                   (float)CH / (float)tok_h, (float)CW / (float)tok_w,   // host IEEE divisions: the oracle's bilinear_src scales
                   depth_scale, H, W, CH, CW, tok_h, tok_w, batch};
  const long long rounds = (long long)batch * (tok_h * tok_w / 128);
  const int g = (int)std::min<long long>(rounds, 2ll * c->num_cus);   // <= 65 KB of LDS, <= 128 registers: two workgroups per CU
  const bool win = tok_long_window_fits(a.scale_x, CW, tok_w);
  return with_E(c->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    return win ? launch<ita_tok_long_kernel<E, T, true>, ItaTokLongLds<E, true>::TOTAL>(dim3(g), dim3(512), s, a)
               : launch<ita_tok_long_kernel<E, T, false>, ItaTokLongLds<E, false>::TOTAL>(dim3(g), dim3(512), s, a);
  });
}

WireSize* find_wire(ita_context* c, int H, int W) {
  for (WireSize& w : c->wire)
    if (w.H == H && w.W == W) return &w;
  return nullptr;
}

// Builds and uploads the two tables of a source size.  Allocates and copies synchronously: not for a captured stream.
int prepare_wire(ita_context* c, int H, int W, WireSize** out) {
  if (WireSize* w = find_wire(c, H, W)) {
    if (out) *out = w;
    return ITA_OK;
  }
  ItaResizeAxis ay, ax;
  if (!ita_resize_axis(H, ITA_WIRE_H, ay) || !ita_resize_axis(W, ITA_WIRE_W, ax))
    return fail(ITA_ERR_INVALID_ARG, "no resize table for this source size");
  WireSize* slot = nullptr;
  for (WireSize& w : c->wire)
    if (!slot && w.H == 0) slot = &w;
  if (!slot) {
    slot = &c->wire[c->wire_next];
    c->wire_next = (c->wire_next + 1) % ITA_WIRE_SIZES;
    HIPCHK(hipDeviceSynchronize());   // a launch still in flight may read the tables that go
  }
  *slot = WireSize{};
  std::vector<int> idx;
  for (const std::vector<int>* v : {&ay.n0, &ay.count, &ax.n0, &ax.count}) idx.insert(idx.end(), v->begin(), v->end());
  std::vector<float> coeff(ay.coeff);
  coeff.resize(ay.coeff.size() + ax.coeff.size());   // wx transposed: [ldx][90]
  for (int ox = 0; ox < ITA_WIRE_W; ++ox)
    for (int j = 0; j < ax.width; ++j) coeff[ay.coeff.size() + (size_t)j * ITA_WIRE_W + ox] = ax.coeff[(size_t)ox * ax.width + j];
  WireSize w;
  HIPCHK(w.idx.upload(idx.data(), idx.size()));
  HIPCHK(w.coeff.upload(coeff.data(), coeff.size()));
  w.dev.n0y = w.idx;
  w.dev.cnty = w.idx + ITA_WIRE_H;
  w.dev.n0x = w.idx + 2 * ITA_WIRE_H;
  w.dev.cntx = w.idx + 2 * ITA_WIRE_H + ITA_WIRE_W;
  w.dev.wy = w.coeff;
  w.dev.wx = w.coeff + ay.coeff.size();
  w.dev.ldy = ay.width;
  w.dev.ldx = ax.width;
  for (int b = 0; b < 3; ++b)
    for (int oy0 = 0, rows = 4 * (b + 1); oy0 < ITA_WIRE_H; oy0 += rows) {
      int first = H, end = 0;
      for (int oy = oy0; oy < std::min(oy0 + rows, ITA_WIRE_H); ++oy) {
        first = std::min(first, ay.n0[oy]);
        end = std::max(end, ay.n0[oy] + ay.count[oy]);
      }
      w.span[b] = std::max(w.span[b], end - first);
    }
  w.H = H;
  w.W = W;
  *slot = std::move(w);
  if (out) *out = slot;
  return ITA_OK;
}

// ita_load_weights without its cleanup: any non-zero return leaves h->w half built
int load_weights(ita_context* h, const void* blob, size_t nbytes) {
  ita_blob_header hdr;
  BlobKinds kinds;
  int rc = check_blob(blob, nbytes, &hdr, &kinds);
  if (rc) return rc;
  // the old weights and the workspace go before the new blob is uploaded: no two models resident at once
  h->w = Weights{};
  h->ws = Workspace{};
  Weights& w = h->w;
  w.hdr = hdr;
  w.hblob.assign((const char*)blob, (const char*)blob + nbytes);
  HIPCHK(w.dblob.upload((const char*)blob, nbytes));
  if ((rc = bind_layers(w, kinds)) || (rc = build_stream_images(w)) || (rc = build_tokenizer_images(w)) ||
      (rc = build_tail_weights(w)) || (rc = build_lstm_weights(w)))
    return rc;
  w.loaded = true;
  w.kfold = 128 * hdr.E;
  w.ldfold = w.kfold + 64;
  if (((hdr.has_tail && hdr.E == 64 && w.tail_wT) || !hdr.has_tail) && w.dec_w && w.lw_hi[0]) rc = build_fold(w, h->num_cus);
  return rc;
}

// Host-buffer entry used by the reference's `void` symbols: 1 x 128 x E activation in, same out.
int dispatch_host(const uint16_t* in, uint16_t* out, bool ffn) {
  std::lock_guard<std::mutex> g(g_bind_mu);
  ita_context* c = g_bound;
  if (!c) return fail(ITA_ERR_NOT_BOUND, "ita_bind_dispatch has not been called");
  if (!in || !out) return fail(ITA_ERR_INVALID_ARG, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)128 * c->w.hdr.E;
  if (!c->dsp_in) {
    HIPCHK(c->dsp_in.alloc(n));
    HIPCHK(c->dsp_out.alloc(n));
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

// =============================================================================== C ABI
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
  std::unique_ptr<ita_context> c(new ita_context());
  c->device = dev;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  for (const LdsKernel& k : lds_kernels())   // every kernel a launch can start with dynamic LDS, on this device
    HIPCHK(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
  *out = c.release();
  return ITA_OK;
}

int ita_destroy(ita_handle h) {
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  {
    std::lock_guard<std::mutex> g(g_bind_mu);
    if (g_bound == h) g_bound = nullptr;
  }
  (void)hipSetDevice(h->device);   // the handle's buffers are released on its device
  for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->pipe_ev) (void)hipEventDestroy(e);
  delete h;
  return ITA_OK;
}

int ita_load_weights(ita_handle h, const void* blob, size_t nbytes) {
  if (!h || !blob) return fail(ITA_ERR_INVALID_ARG, "null argument");
  HIPCHK(hipSetDevice(h->device));
  const int rc = load_weights(h, blob, nbytes);
  if (rc) h->w = Weights{};   // the one cleanup point: a failed load leaves the handle unloaded
  return rc;
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
  if (max_batch > h->ws.cap) {
    HIPCHK(hipDeviceSynchronize());
    rc = grow_workspace(h, max_batch);
  }
  h->ws_reserved = rc == ITA_OK;
  return rc;
}

int ita_get_dims(ita_handle h, int* E, int* S, int* P, int* F, int* H, int* num_layers) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (E) *E = h->w.hdr.E;
  if (S) *S = h->w.hdr.S;
  if (P) *P = h->w.hdr.P;
  if (F) *F = h->w.hdr.F;
  if (H) *H = h->w.hdr.H;
  if (num_layers) *num_layers = h->w.hdr.num_layers;
  return ITA_OK;
}

int ita_mha_int8_taps(ita_handle h, int layer, const float* x, float* y, int batch, const ita_mha_taps* taps,
                      void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  return launch_mha(h, layer, x, y, batch, false, taps, (hipStream_t)stream);
}
int ita_mha_int8(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  return ita_mha_int8_taps(h, layer, x, y, batch, nullptr, stream);
}

namespace {

// the sequence lengths and batches every long-sequence entry point, int8 or float, takes (ITA_ERR_UNSUPPORTED)
int check_long_shape(int batch, int seq_len) {
  if (seq_len < 128 || seq_len % 128 || seq_len > 65536 || batch > 65535)
    return fail(ITA_ERR_UNSUPPORTED, "seq_len must be a multiple of 128 in [128, 65536], batch <= 65535");
  return ITA_OK;
}

// the refusals every long-sequence int8 entry point shares (ITA_ERR_UNSUPPORTED, before any launch)
int check_long(const Layer& L, int batch, int seq_len, bool taps = false) {
  if (L.attn_f32)
    return fail(ITA_ERR_UNSUPPORTED, taps ? "this layer's attention is float32 (ITAW0003 blob): its flash kernel keeps no row probabilities, there are no taps "
                                            "here: ita_mha_long_f32_taps reads a float layer out"
                                          : "this layer's attention is float32 (ITAW0003 blob): no int8 long attention");
  if (int rc = check_long_shape(batch, seq_len)) return rc;
  if (!L.simg_mha) return fail(ITA_ERR_UNSUPPORTED, "this layer has no attention image (accumulator range, or more than one head)");
  return ITA_OK;
}

// The taps' own refusals (ITA_ERR_INVALID_ARG)
constexpr int ITA_LONG_MAX_ROWS = 1024, ITA_LONG_MAX_SEQ = 65536;
// the chosen rows of either long taps entry (ita_mha_long_taps, ita_mha_long_f32_taps: the same four row-indexed taps)
// row_ptr: is any of logits, probs, row_max, row_sum given
int check_long_rows(const int* rows, int n_rows, bool row_ptr, int seq_len) {
  if (n_rows < 0 || n_rows > ITA_LONG_MAX_ROWS) return fail(ITA_ERR_INVALID_ARG, "n_rows must be in [0, 1024]");
  if (n_rows > 0 && !rows) return fail(ITA_ERR_INVALID_ARG, "n_rows > 0 without rows");
  for (int i = 0; i < n_rows; ++i)
    if (rows[i] < 0 || rows[i] >= seq_len || (i > 0 && rows[i] <= rows[i - 1]))
      return fail(ITA_ERR_INVALID_ARG, "rows must be strictly increasing token indices in [0, seq_len)");
  if (n_rows == 0 && row_ptr)
    return fail(ITA_ERR_INVALID_ARG, "logits, probs, row_max and row_sum are per chosen row: n_rows is 0");
  return ITA_OK;
}
bool misaligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) != 0; }

int check_long_taps(const ita_mha_long_taps& t, int seq_len, hipStream_t s) {
  if (int rc = check_long_rows(t.rows, t.n_rows, t.logits || t.probs || t.row_max || t.row_sum, seq_len)) return rc;
  if (misaligned(t.x_q, 16) || misaligned(t.out_q, 16) || misaligned(t.Q, 4) || misaligned(t.K, 4) || misaligned(t.ctx, 4) ||
      misaligned(t.logits, 4) || misaligned(t.probs, 4) || misaligned(t.row_sum, 4))
    return fail(ITA_ERR_INVALID_ARG, "x_q and out_q must be 16-byte aligned; Q, K, ctx, logits, probs and row_sum 4-byte aligned");
  if (capturing(s))
    return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_int8_taps cannot run inside a stream capture (its row table is rebuilt on the host)");
  return ITA_OK;
}

// The handle's row table for a taps call that gives rows: token -> output row, or -1; the copy has left the host vector
// when the wait returns
int upload_long_rows(ita_context* h, const int* rows, int n_rows, int seq_len, hipStream_t s) {
  if (!h->long_rows) HIPCHK(h->long_rows.alloc(ITA_LONG_MAX_SEQ));
  h->long_rows_host.assign((size_t)seq_len, -1);
  for (int i = 0; i < n_rows; ++i) h->long_rows_host[rows[i]] = i;
  HIPCHK(hipMemcpyAsync(h->long_rows, h->long_rows_host.data(), (size_t)seq_len * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return ITA_OK;
}

// The handle's long-attention workspace (int8 and float entries share the buffer) at `need` bytes: it grows outside a
// stream capture only (a captured graph keeps raw pointers into it), behind a device synchronisation
int ensure_long_ws(ita_context* h, size_t need, hipStream_t s) {
  if (need <= h->long_ws_bytes) return ITA_OK;
  if (capturing(s))
    return fail(ITA_ERR_INVALID_ARG, "the long-attention workspace cannot grow inside a stream capture; run one call first");
  HIPCHK(hipDeviceSynchronize());
  h->long_ws_bytes = 0;
  HIPCHK(h->long_ws.alloc(need));
  h->long_ws_bytes = need;
  return ITA_OK;
}

// The int8 workspace of ntile tiles of 128 tokens (Q fragments, K and V^T images, column sums), and the two long kernels'
// arguments over it (the I/O pointers and fuse_ln are the caller's to set)
constexpr size_t long_int8_ws(size_t ntile) { return ntile * (3 * 24576 + 192 * 4); }
ItaLongArgs long_args(ita_context* h, const Layer& L, size_t ntile, int batch, int seq_len) {
  ItaLongArgs a{};
  a.image = L.simg_mha;
  a.qfrag = h->long_ws; a.kimg = a.qfrag + ntile * 24576; a.vimg = a.kimg + ntile * 24576;
  a.csum = (int*)(a.vimg + ntile * 24576);
  a.mq = L.ascal[ITA_A_MQ]; a.mk = L.ascal[ITA_A_MK]; a.mv = L.ascal[ITA_A_MV]; a.ml = L.ascal[ITA_A_ML];
  a.mc = L.ascal[ITA_A_MC]; a.mo = L.ascal[ITA_A_MO];
  a.inv_sx = L.ascal[ITA_A_INV_SX]; a.so = L.ascal[ITA_A_SO];
  a.B = batch; a.S = seq_len;
  return a;
}

// What the long-sequence entry points share: the refusals, the workspace, the two launches.
// Int8 form: xq -> yq.  F32 form (x non-null): x -> y, with fuse_ln + residual + LayerNorm1; with taps (f32 form only)
// the taps kernels run instead: the same bodies and the stores of ita_mha_long_taps.
int launch_long(ita_context* h, int layer, const int8_t* xq, int8_t* yq, const float* x, float* y, bool fuse_ln, int batch,
                int seq_len, hipStream_t s, const ita_mha_long_taps* taps = nullptr) {
  const Layer& L = h->w.layers[layer];
  if (int rc = check_long(L, batch, seq_len, taps != nullptr)) return rc;
  if (fuse_ln && !L.n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
  if (taps)
    if (int rc = check_long_taps(*taps, seq_len, s)) return rc;
  // the logits of a long row still fit the 16-bit travel format: same bound as stream_range_ok (per key, not per row)
  const size_t ntile = (size_t)batch * (seq_len / 128);
  if (int rc = ensure_long_ws(h, long_int8_ws(ntile), s)) return rc;
  ItaLongArgs a = long_args(h, L, ntile, batch, seq_len);
  a.xq = xq; a.yq = yq; a.x = x; a.y = y; a.fuse_ln = fuse_ln ? 1 : 0;
  const bool fast = L.fast_sites == ITA_SITES_ALL;
  const dim3 proj_grid(ntile < (size_t)h->num_cus ? (int)ntile : h->num_cus), attn_grid(seq_len / 128, batch);
  ItaLongTapArgs tp{};
  if (taps) {
    tp.xq = taps->x_q; tp.Q = taps->Q; tp.K = taps->K; tp.V = taps->V; tp.ctx = taps->ctx; tp.outq = taps->out_q;
    tp.logits = taps->logits; tp.probs = taps->probs; tp.row_max = taps->row_max; tp.row_sum = taps->row_sum;
    tp.n_rows = taps->n_rows;
    if (taps->n_rows > 0) {
      if (int rc = upload_long_rows(h, taps->rows, taps->n_rows, seq_len, s)) return rc;
      tp.rowidx = h->long_rows;
    }
  }
  auto run = [&](auto e, auto f32, auto fst) {
    constexpr int E = decltype(e)::value;
    constexpr bool F32 = decltype(f32)::value, FAST = decltype(fst)::value;
    if constexpr (F32) {
      if (taps) {
        if (int rc = launch<ita_long_proj_taps_kernel<FAST, E>, ItaStreamLds<E, false, false>::TOTAL>(proj_grid, dim3(512), s, a, tp)) return rc;
        return launch<ita_long_attn_taps_kernel<FAST, E>, ItaLongLds::TOTAL>(attn_grid, dim3(512), s, a, tp);
      }
    }
    if (int rc = launch<ita_long_proj_kernel<FAST, E, F32>, ItaStreamLds<E, false, false>::TOTAL>(proj_grid, dim3(512), s, a)) return rc;
    return launch<ita_long_attn_kernel<FAST, E, F32>, ItaLongLds::TOTAL>(attn_grid, dim3(512), s, a);
  };
  return with_E(h->w.hdr.E, [&](auto e) {
    if (x) return fast ? run(e, std::true_type{}, std::true_type{}) : run(e, std::true_type{}, std::false_type{});
    return fast ? run(e, std::false_type{}, std::true_type{}) : run(e, std::false_type{}, std::false_type{});
  });
}

}  // namespace

int ita_mha_long_q8(ita_handle h, int layer, const int8_t* x_q, int8_t* out_q, int batch, int seq_len, void* stream) {
  if (int rc = check_layer_io(h, layer, x_q, out_q, batch)) return rc;
  return launch_long(h, layer, x_q, out_q, nullptr, nullptr, false, batch, seq_len, (hipStream_t)stream);
}

int ita_mha_long_int8(ita_handle h, int layer, const float* x, float* y, int batch, int seq_len, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  return launch_long(h, layer, nullptr, nullptr, x, y, false, batch, seq_len, (hipStream_t)stream);
}

int ita_mha_long_int8_taps(ita_handle h, int layer, const float* x, float* y, int batch, int seq_len,
                           const ita_mha_long_taps* taps, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  const ita_mha_long_taps none{};
  return launch_long(h, layer, nullptr, nullptr, x, y, false, batch, seq_len, (hipStream_t)stream, taps ? taps : &none);
}

namespace {
// The output refusals of the two statistics entries (ITA_ERR_INVALID_ARG): all six outputs null, or one of those stored as
// 32-bit words (out[first_word] and the ones behind it) off a 4-byte boundary; the entry gives its own two messages
int check_long_stats_outputs(const void* const (&out)[6], int first_word, const char* all_null, const char* unaligned) {
  if (std::none_of(out, out + 6, [](const void* p) { return p != nullptr; })) return fail(ITA_ERR_INVALID_ARG, all_null);
  if (std::any_of(out + first_word, out + 6, [](const void* p) { return misaligned(p, 4); })) return fail(ITA_ERR_INVALID_ARG, unaligned);
  return ITA_OK;
}
}  // namespace

// The production projection launch (f32 form), then ita_long_stats_kernel over its workspace: no y, no A.V, no out_proj
int ita_mha_long_int8_stats(ita_handle h, int layer, const float* x, int batch, int seq_len, const ita_mha_long_stats* st,
                            void* stream) {
  if (int rc = check(h, batch)) return rc;
  if (!x || !st || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  const Layer& L = h->w.layers[layer];
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_long(L, batch, seq_len)) return rc;
  if (int rc = check_long_stats_outputs({st->row_max, st->row_sum, st->row_mass, st->row_nnz, st->col_mass, st->col_nnz}, 1,   // row_max: int8
                                        "ita_mha_long_int8_stats: all six outputs are null",
                                        "row_sum, row_mass, row_nnz, col_mass and col_nnz must be 4-byte aligned")) return rc;
  const size_t ntile = (size_t)batch * (seq_len / 128);
  if (int rc = ensure_long_ws(h, long_int8_ws(ntile), s)) return rc;
  ItaLongArgs a = long_args(h, L, ntile, batch, seq_len);
  a.x = x;
  ItaLongStatsArgs sa{};
  sa.qfrag = a.qfrag; sa.kimg = a.kimg; sa.ml = a.ml; sa.B = batch; sa.S = seq_len;
  sa.row_max = st->row_max; sa.row_sum = st->row_sum; sa.row_mass = st->row_mass; sa.row_nnz = st->row_nnz;
  sa.col_mass = st->col_mass; sa.col_nnz = st->col_nnz;
  // the kernel ADDS into the column arrays: they are zeroed on the stream first, by a kernel (inside a stream capture the
  // call is kernel nodes only)
  if (sa.col_mass || sa.col_nnz) {
    const size_t n = (size_t)batch * seq_len, blocks = (n + 255) / 256;
    if (int rc = launch<ita_long_stats_zero_kernel>(dim3(blocks < 2048 ? (int)blocks : 2048), dim3(256), s, sa.col_mass, sa.col_nnz, n))
      return rc;
  }
  const bool fast = L.fast_sites == ITA_SITES_ALL;
  const dim3 proj_grid(ntile < (size_t)h->num_cus ? (int)ntile : h->num_cus), grid(seq_len / 128, batch);
  auto run = [&](auto e, auto fst) {
    constexpr int E = decltype(e)::value;
    constexpr bool FAST = decltype(fst)::value;
    if (int rc = launch<ita_long_proj_kernel<FAST, E, true>, ItaStreamLds<E, false, false>::TOTAL>(proj_grid, dim3(512), s, a)) return rc;
    return launch<ita_long_stats_kernel<FAST>, ItaLongStatsLds::TOTAL>(grid, dim3(512), s, sa);
  };
  return with_E(h->w.hdr.E, [&](auto e) { return fast ? run(e, std::true_type{}) : run(e, std::false_type{}); });
}

// The production projection launch (f32 form), then ita_long_hist_kernel over its workspace (ita_long_hist_kernel.h): two
// sweeps, no y.  The kernel ADDS into the outputs: they are set to zero (the range to INT_MAX, INT_MIN) on the stream first,
// by a kernel (inside a stream capture the call is kernel nodes only)
int ita_mha_long_int8_hist(ita_handle h, int layer, const float* x, int batch, int seq_len, const ita_mha_long_hist* hist,
                           void* stream) {
  if (int rc = check(h, batch)) return rc;
  if (!x || !hist || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  const Layer& L = h->w.layers[layer];
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_long(L, batch, seq_len)) return rc;
  if (!hist->logits && !hist->shifts && !hist->probs && !hist->logits_out && !hist->acc_range)
    return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_int8_hist: all five outputs are null");
  if (misaligned(hist->logits, 8) || misaligned(hist->shifts, 8) || misaligned(hist->probs, 8) || misaligned(hist->logits_out, 8) ||
      misaligned(hist->acc_range, 4))
    return fail(ITA_ERR_INVALID_ARG, "logits, shifts, probs and logits_out must be 8-byte aligned, acc_range 4-byte aligned");
  const size_t ntile = (size_t)batch * (seq_len / 128);
  if (int rc = ensure_long_ws(h, long_int8_ws(ntile), s)) return rc;
  ItaLongArgs a = long_args(h, L, ntile, batch, seq_len);
  a.x = x;
  ItaLongHistArgs ha{};
  ha.qfrag = a.qfrag; ha.kimg = a.kimg; ha.ml = a.ml; ha.B = batch; ha.S = seq_len;
  ha.logits = (unsigned long long*)hist->logits; ha.shifts = (unsigned long long*)hist->shifts;
  ha.probs = (unsigned long long*)hist->probs; ha.logits_out = (unsigned long long*)hist->logits_out;
  ha.acc_range = hist->acc_range;
  if (int rc = launch<ita_long_hist_zero_kernel>(dim3(batch), dim3(256), s, ha)) return rc;
  const bool fast = L.fast_sites == ITA_SITES_ALL;
  const dim3 proj_grid(ntile < (size_t)h->num_cus ? (int)ntile : h->num_cus), grid(seq_len / 128, batch);
  auto run = [&](auto e, auto fst) {
    constexpr int E = decltype(e)::value;
    constexpr bool FAST = decltype(fst)::value;
    if (int rc = launch<ita_long_proj_kernel<FAST, E, true>, ItaStreamLds<E, false, false>::TOTAL>(proj_grid, dim3(512), s, a)) return rc;
    return launch<ita_long_hist_kernel<FAST>, ItaLongHistLds::TOTAL>(grid, dim3(512), s, ha);
  };
  return with_E(h->w.hdr.E, [&](auto e) { return fast ? run(e, std::true_type{}) : run(e, std::false_type{}); });
}

// out = w . P (ita_long_prop_kernel.h): the production projection launch, ita_long_stats_kernel for the row maximum and row
// sum of every query (into the workspace: no column arrays, so no zero launch), the prep kernel, the transposed sweep
int ita_mha_long_int8_propagate(ita_handle h, int layer, const float* x, int batch, int seq_len, const int8_t* w, int n_w,
                                int32_t* out, void* stream) {
  if (int rc = check(h, batch)) return rc;
  if (!x || !w || !out || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  const Layer& L = h->w.layers[layer];
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_long(L, batch, seq_len)) return rc;
  if (n_w < 1 || n_w > 64) return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_int8_propagate: n_w must be in [1, 64]");
  if (misaligned(w, 4) || misaligned(out, 16))
    return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_int8_propagate: w_dev must be 4-byte aligned, out_dev 16-byte aligned");
  const size_t ntile = (size_t)batch * (seq_len / 128), ng = (size_t)(n_w + 15) / 16;
  // behind the int8 workspace: row-parameter images, weight images, row_sum, 128 * weight row sums, row_max
  const size_t base = long_int8_ws(ntile), rowp = ntile * 1024, wimg = ntile * ng * 2048, rsum = ntile * 128 * 4,
               wsum = (size_t)batch * 64 * 4, rmax = ntile * 128;
  if (int rc = ensure_long_ws(h, base + rowp + wimg + rsum + wsum + rmax, s)) return rc;
  ItaLongArgs a = long_args(h, L, ntile, batch, seq_len);
  a.x = x;
  char* p = a.qfrag + base;
  ItaLongPropPrepArgs pa{};
  pa.rowp = p; pa.wimg = p + rowp;
  int* row_sum = (int*)(p + rowp + wimg);
  pa.wsum = (int*)(p + rowp + wimg + rsum);
  int8_t* row_max = (int8_t*)(p + rowp + wimg + rsum + wsum);
  pa.row_max = row_max; pa.row_sum = row_sum; pa.w = w; pa.B = batch; pa.S = seq_len; pa.n_w = n_w;
  ItaLongStatsArgs sa{};
  sa.qfrag = a.qfrag; sa.kimg = a.kimg; sa.ml = a.ml; sa.B = batch; sa.S = seq_len;
  sa.row_max = row_max; sa.row_sum = row_sum;
  ItaLongPropArgs ka{};
  ka.qfrag = a.qfrag; ka.kimg = a.kimg; ka.rowp = pa.rowp; ka.wimg = pa.wimg; ka.wsum = pa.wsum; ka.ml = a.ml;
  ka.B = batch; ka.S = seq_len; ka.n_w = n_w; ka.out = out;
  const bool fast = L.fast_sites == ITA_SITES_ALL;
  const dim3 proj_grid(ntile < (size_t)h->num_cus ? (int)ntile : h->num_cus), grid(seq_len / 128, batch);
  const dim3 prep_grid(seq_len / 128 + 16 * (int)ng, batch);
  auto run = [&](auto e, auto fst) {
    constexpr int E = decltype(e)::value;
    constexpr bool FAST = decltype(fst)::value;
    if (int rc = launch<ita_long_proj_kernel<FAST, E, true>, ItaStreamLds<E, false, false>::TOTAL>(proj_grid, dim3(512), s, a)) return rc;
    if (int rc = launch<ita_long_stats_kernel<FAST>, ItaLongStatsLds::TOTAL>(grid, dim3(512), s, sa)) return rc;
    if (int rc = launch<ita_long_prop_prep_kernel>(prep_grid, dim3(512), s, pa)) return rc;
    return launch<ita_long_prop_kernel<FAST>, ItaLongPropLds::TOTAL>(grid, dim3(512), s, ka);
  };
  return with_E(h->w.hdr.E, [&](auto e) { return fast ? run(e, std::true_type{}) : run(e, std::false_type{}); });
}

// x1 = LN1(x + attn(x)) into y by the two long launches, then the FFN block + residual + LN2 in place on y: the FFN is per
// token, so the (batch * seq_len / 128) blocks of 128 rows are its "frames"
int ita_encoder_layer_long(ita_handle h, int layer, const float* x, float* y, int batch, int seq_len, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  const Layer& L = h->w.layers[layer];
  // (everything that can refuse is checked before the first launch: no partial work is left behind an error)
  if (int rc = check_long(L, batch, seq_len)) return rc;
  if (L.ffn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's FFN is float32 (ITAW0002 blob): no long-sequence encoder layer");
  if (!L.n1w || !L.n2w) return fail(ITA_ERR_BAD_BLOB, "LayerNorm parameters missing from the blob");
  if (int rc = launch_long(h, layer, nullptr, nullptr, x, y, true, batch, seq_len, (hipStream_t)stream)) return rc;
  return launch_ffn(h, layer, y, y, batch * (seq_len / 128), true, nullptr, (hipStream_t)stream);
}

namespace {

// the refusals every long float entry point shares (ITA_ERR_UNSUPPORTED, before any launch); int8_layer: what to say of
// an int8-attention layer, naming the sibling entry
int check_long_f32(const Layer& L, int batch, int seq_len, const char* int8_layer) {
  if (!L.attn_f32) return fail(ITA_ERR_UNSUPPORTED, int8_layer);
  return check_long_shape(batch, seq_len);
}

// The float32 long attention (ita_long_f32_kernel.h) of an ITAW0003 layer: the refusals, the workspace (the int8 long
// path's buffer, grown the same way: K and V fragment images, 192 KB per 128-token tile), the two launches.  With taps
// (ita_mha_long_f32_taps) the taps kernels run instead, the same bodies and the stores of ItaLongF32TapArgs, and behind
// them the probabilities' elementwise launch.
int launch_long_f32(ita_context* h, int layer, const float* x, float* y, bool fuse_ln, int batch, int seq_len, hipStream_t s,
                    const struct ita_mha_long_f32_taps* taps = nullptr) {
  const Layer& L = h->w.layers[layer];
  if (int rc = check_long_f32(L, batch, seq_len,
                              taps ? "this layer's attention is int8 (ITAW0001 / ITAW0002 blob): ita_mha_long_int8_taps reads it out"
                                   : "this layer's attention is int8 (ITAW0001 / ITAW0002 blob): ita_mha_long_int8 runs it")) return rc;
  if (fuse_ln && !L.n1w) return fail(ITA_ERR_BAD_BLOB, "norm1 parameters missing from the blob");
  if (taps) {   // the taps' own refusals (ITA_ERR_INVALID_ARG)
    if (int rc = check_long_rows(taps->rows, taps->n_rows, taps->logits || taps->probs || taps->row_max || taps->row_sum, seq_len))
      return rc;
    if (misaligned(taps->Q, 16) || misaligned(taps->K, 16) || misaligned(taps->V, 16) || misaligned(taps->ctx, 16) ||
        misaligned(taps->logits, 16) || misaligned(taps->probs, 16) || misaligned(taps->row_max, 4) || misaligned(taps->row_sum, 4))
      return fail(ITA_ERR_INVALID_ARG, "Q, K, V, ctx, logits and probs must be 16-byte aligned; row_max and row_sum 4-byte aligned");
    if (capturing(s))
      return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_f32_taps cannot run inside a stream capture (its row table is rebuilt on the host)");
  }
  const size_t ntile = (size_t)batch * (seq_len / 128);
  const size_t img = ntile * 2 * ItaLongF32Lds::UNIT;
  if (int rc = ensure_long_ws(h, 2 * img, s)) return rc;
  ItaLongF32Args a{};
  a.x = x; a.y = y;
  a.wq = L.wqf; a.wk = L.wkf; a.wv = L.wvf; a.bq = L.bqf; a.bk = L.bkf; a.bv = L.bvf; a.wo = L.wof; a.bo = L.bof;
  a.ln_w = L.n1w; a.ln_b = L.n1b;
  a.kimg = (f32x4*)(char*)h->long_ws; a.vimg = (f32x4*)((char*)h->long_ws + img);
  a.B = batch; a.S = seq_len; a.fuse_ln = fuse_ln ? 1 : 0;
  const size_t cap = 2 * (size_t)h->num_cus;
  const dim3 proj_grid((unsigned)(ntile < cap ? ntile : cap)), attn_grid(seq_len / 128, batch);
  if (!taps)
    return with_E(h->w.hdr.E, [&](auto e) {
      constexpr int E = decltype(e)::value;
      if (int rc = launch<ita_lf32_proj_kernel<E>>(proj_grid, dim3(512), s, a)) return rc;
      return launch<ita_lf32_attn_kernel<E>, ItaLongF32Lds::TOTAL>(attn_grid, dim3(512), s, a);
    });
  ItaLongF32TapArgs tp{};
  tp.Q = taps->Q; tp.K = taps->K; tp.V = taps->V; tp.ctx = taps->ctx;
  tp.n_rows = taps->n_rows;
  const size_t nrow = (size_t)batch * taps->n_rows;
  if (taps->n_rows > 0) {
    if (int rc = upload_long_rows(h, taps->rows, taps->n_rows, seq_len, s)) return rc;
    tp.rowidx = h->long_rows;
    // the sweep's logits go to the caller's buffer, or where the probabilities will stand (turned in place below)
    tp.logits = taps->logits ? taps->logits : taps->probs;
    tp.row_max = taps->row_max; tp.row_sum = taps->row_sum;
    if (taps->probs && !(taps->row_max && taps->row_sum)) {   // the probabilities need both: the handle's own pair
      if (2 * nrow > h->long_rowstat_n) {
        HIPCHK(hipDeviceSynchronize());
        h->long_rowstat_n = 0;
        HIPCHK(h->long_rowstat.alloc(2 * nrow));
        h->long_rowstat_n = 2 * nrow;
      }
      if (!tp.row_max) tp.row_max = h->long_rowstat;
      if (!tp.row_sum) tp.row_sum = h->long_rowstat + nrow;
    }
  }
  return with_E(h->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (int rc = launch<ita_lf32_proj_taps_kernel<E>>(proj_grid, dim3(512), s, a, tp)) return rc;
    if (int rc = launch<ita_lf32_attn_taps_kernel<E>, ItaLongF32Lds::TOTAL>(attn_grid, dim3(512), s, a, tp)) return rc;
    if (!taps->probs) return (int)ITA_OK;
    return launch<ita_lf32_probs_kernel>(dim3((unsigned)nrow), dim3(256), s, (const float*)tp.logits, taps->probs,
                                         (const float*)tp.row_max, (const float*)tp.row_sum, seq_len);
  });
}

}  // namespace

int ita_mha_long_f32(ita_handle h, int layer, const float* x, float* y, int batch, int seq_len, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  return launch_long_f32(h, layer, x, y, false, batch, seq_len, (hipStream_t)stream);
}

int ita_mha_long_f32_taps(ita_handle h, int layer, const float* x, float* y, int batch, int seq_len,
                          const struct ita_mha_long_f32_taps* taps, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  const struct ita_mha_long_f32_taps none{};
  return launch_long_f32(h, layer, x, y, false, batch, seq_len, (hipStream_t)stream, taps ? taps : &none);
}

// The production projection launch, then ita_lf32_stats_kernel over its K image and, for the columns, the reduction of the
// query tiles' partials (ita_long_f32_stats_kernel.h): no y, no P.V, no out_proj.  The workspace is the float long
// workspace (K and V images: the projection kernel writes both) and behind it the partials, (B, S/128, S) f32 and s32,
// of a call that asks for a column statistic.
int ita_mha_long_f32_stats(ita_handle h, int layer, const float* x, int batch, int seq_len, float p_min,
                           const struct ita_mha_long_f32_stats* st, void* stream) {
  // the argument rules come first: they need neither the handle's contents nor the device
  if (!h || !x || !st) return fail(ITA_ERR_INVALID_ARG, "null handle, x_dev or stats");
  if (int rc = check_long_stats_outputs({st->row_max, st->row_sum, st->row_gap, st->row_nnz, st->col_mass, st->col_nnz}, 0,
                                        "ita_mha_long_f32_stats: all six outputs are null", "every output must be 4-byte aligned")) return rc;
  if (!(p_min > 0.0f && p_min <= 1.0f)) return fail(ITA_ERR_INVALID_ARG, "p_min must be in (0, 1]");   // NaN fails both
  if (int rc = check(h, batch)) return rc;
  if (layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad layer");
  const Layer& L = h->w.layers[layer];
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_long_f32(L, batch, seq_len,
                              "this layer's attention is int8 (ITAW0001 / ITAW0002 blob): ita_mha_long_int8_stats reads it out")) return rc;
  const size_t nqt = (size_t)seq_len / 128, ntile = (size_t)batch * nqt;
  const size_t img = ntile * 2 * ItaLongF32Lds::UNIT, part = ntile * seq_len * 4;
  const bool cols = st->col_mass || st->col_nnz;
  if (int rc = ensure_long_ws(h, 2 * img + (cols ? 2 * part : 0), s)) return rc;
  ItaLongF32Args a{};
  a.x = x;
  a.wk = L.wkf; a.wv = L.wvf; a.bk = L.bkf; a.bv = L.bvf;
  a.kimg = (f32x4*)(char*)h->long_ws; a.vimg = (f32x4*)((char*)h->long_ws + img);
  a.B = batch; a.S = seq_len;
  ItaLongF32StatsArgs sa{};
  sa.x = x; sa.wq = L.wqf; sa.bq = L.bqf; sa.kimg = a.kimg;
  sa.B = batch; sa.S = seq_len; sa.p_min = p_min;
  sa.row_max = st->row_max; sa.row_sum = st->row_sum; sa.row_gap = st->row_gap; sa.row_nnz = st->row_nnz;
  if (st->col_mass) sa.part_mass = (float*)((char*)h->long_ws + 2 * img);
  if (st->col_nnz) sa.part_nnz = (int*)((char*)h->long_ws + 2 * img + part);
  const size_t cap = 2 * (size_t)h->num_cus;
  const dim3 proj_grid((unsigned)(ntile < cap ? ntile : cap)), grid(seq_len / 128, batch);
  return with_E(h->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (int rc = launch<ita_lf32_proj_kernel<E>>(proj_grid, dim3(512), s, a)) return rc;
    if (int rc = launch<ita_lf32_stats_kernel<E>, ItaLongF32Lds::TOTAL>(grid, dim3(512), s, sa)) return rc;
    if (!cols) return (int)ITA_OK;
    const size_t n = (size_t)batch * seq_len, blocks = (n + 255) / 256;
    return launch<ita_lf32_colsum_kernel>(dim3(blocks < 4096 ? (unsigned)blocks : 4096u), dim3(256), s, (const float*)sa.part_mass,
                                          (const int*)sa.part_nnz, st->col_mass, st->col_nnz, (int)nqt, seq_len, n);
  });
}

// out = w . P (ita_long_f32_prop_kernel.h): the K and Q images in one projection launch, ita_lf32_stats_kernel for the row
// maximum and row sum of every query (rows only: sweep 1, into the workspace), the transposed sweep.  The workspace is the
// float long workspace (the Q image stands where the V image does) and behind it row_max and row_sum, (B, S) f32 each.
int ita_mha_long_f32_propagate(ita_handle h, int layer, const float* x, int batch, int seq_len, const float* w, int n_w,
                               float* out, void* stream) {
  if (int rc = check(h, batch)) return rc;
  if (!x || !w || !out || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  const Layer& L = h->w.layers[layer];
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_long_f32(L, batch, seq_len,
                              "this layer's attention is int8 (ITAW0001 / ITAW0002 blob): ita_mha_long_int8_propagate propagates through it")) return rc;
  if (n_w < 1 || n_w > 64) return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_f32_propagate: n_w must be in [1, 64]");
  if (misaligned(w, 16) || misaligned(out, 16))
    return fail(ITA_ERR_INVALID_ARG, "ita_mha_long_f32_propagate: w_dev and out_dev must be 16-byte aligned");
  const size_t ntile = (size_t)batch * (seq_len / 128);
  const size_t img = ntile * 2 * ItaLongF32Lds::UNIT, rows = (size_t)batch * seq_len * 4;
  if (int rc = ensure_long_ws(h, 2 * img + 2 * rows, s)) return rc;
  char* ws = (char*)h->long_ws;
  ItaLongF32PropProjArgs pa{};
  pa.x = x; pa.wk = L.wkf; pa.bk = L.bkf; pa.wq = L.wqf; pa.bq = L.bqf;
  pa.kimg = (f32x4*)ws; pa.qimg = (f32x4*)(ws + img);
  pa.B = batch; pa.S = seq_len;
  ItaLongF32StatsArgs sa{};
  sa.x = x; sa.wq = L.wqf; sa.bq = L.bqf; sa.kimg = pa.kimg;
  sa.B = batch; sa.S = seq_len; sa.p_min = 1.0f;
  sa.row_max = (float*)(ws + 2 * img); sa.row_sum = (float*)(ws + 2 * img + rows);
  ItaLongF32PropArgs ka{};
  ka.kimg = pa.kimg; ka.qimg = pa.qimg; ka.row_max = sa.row_max; ka.row_sum = sa.row_sum;
  ka.w = w; ka.out = out; ka.B = batch; ka.S = seq_len; ka.n_w = n_w;
  const size_t cap = 2 * (size_t)h->num_cus;
  const dim3 proj_grid((unsigned)(ntile < cap ? ntile : cap)), grid(seq_len / 128, batch);
  return with_E(h->w.hdr.E, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (int rc = launch<ita_lf32_projkq_kernel<E>>(proj_grid, dim3(512), s, pa)) return rc;
    if (int rc = launch<ita_lf32_stats_kernel<E>, ItaLongF32Lds::TOTAL>(grid, dim3(512), s, sa)) return rc;
    return launch<ita_lf32_prop_kernel, ItaLongF32PropLds::TOTAL>(grid, dim3(512), s, ka);
  });
}

// The long form of launch_encoder's float-FFN branch: x1 = LN1(x + attn(x)) into y by the float long launches (ITAW0003)
// or the int8 long launches (ITAW0002), then the float FFN block + residual + LN2 in place on y, whose kernel reads a
// 32-row tile (and prefetches its own next one) before it stores that tile and touches no other workgroup's rows
int ita_encoder_layer_long_f32(ita_handle h, int layer, const float* x, float* y, int batch, int seq_len, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  const Layer& L = h->w.layers[layer];
  // (everything that can refuse is checked before the first launch: no partial work is left behind an error)
  if (!L.ffn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's FFN is int8 (ITAW0001 blob): ita_encoder_layer_long runs it");
  if (h->w.hdr.E != 64 && !L.w1p) return fail(ITA_ERR_UNSUPPORTED, "the float32 FFN of an ITAW0002 blob is built for E = 64");
  if (!L.attn_f32)
    if (int rc = check_long(L, batch, seq_len)) return rc;
  if (!L.n1w || !L.n2w) return fail(ITA_ERR_BAD_BLOB, "LayerNorm parameters missing from the blob");
  if (int rc = L.attn_f32 ? launch_long_f32(h, layer, x, y, true, batch, seq_len, (hipStream_t)stream)
                          : launch_long(h, layer, nullptr, nullptr, x, y, true, batch, seq_len, (hipStream_t)stream)) return rc;
  return launch_ffn_f32(h, layer, y, y, batch * (seq_len / 128), true, (hipStream_t)stream);
}

int ita_mha_q8(ita_handle h, int layer, const int8_t* x_q, int8_t* out_q, int batch, void* stream) {
  if (int rc = check_layer_io(h, layer, x_q, out_q, batch)) return rc;
  StreamIo io;
  io.xq = x_q; io.yq = out_q;
  return launch_stream(h, layer, 2, false, io, batch, (hipStream_t)stream);
}

int ita_ffn_int8_taps(ita_handle h, int layer, const float* x, float* y, int batch, const ita_ffn_taps* taps,
                      void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  return launch_ffn(h, layer, x, y, batch, false, taps, (hipStream_t)stream);
}
int ita_ffn_int8(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  return ita_ffn_int8_taps(h, layer, x, y, batch, nullptr, stream);
}

int ita_get_ffn_kind(ita_handle h, int layer, int* kind) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!kind || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  *kind = h->w.layers[layer].ffn_f32 ? ITA_FFN_F32 : ITA_FFN_INT8;
  return ITA_OK;
}

int ita_ffn_f32(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  return launch_ffn_f32(h, layer, x, y, batch, false, (hipStream_t)stream);
}

static_assert(ITA_HEAD_ERR_TIMEOUT == ITA_HEAD_TIMEOUT, "one error code, two names");
int ita_head_status(ita_handle h, int* status) {
  int rc = check(h, 1, false);
  if (rc) return rc;
  if (!status) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  *status = 0;
  if (!h->ws.head_sync) return ITA_OK;
  unsigned v = 0;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(&v, h->ws.head_sync, sizeof(v), hipMemcpyDeviceToHost));
  if (v) {   // a timed-out workgroup left its tile's counter short: zero the error word and every counter
    HIPCHK(hipMemset(h->ws.head_sync, 0, h->ws.head_sync_bytes));
    HIPCHK(hipDeviceSynchronize());
  }
  *status = (int)v;
  return ITA_OK;
}

int ita_get_attn_kind(ita_handle h, int layer, int* kind) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!kind || layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  *kind = h->w.layers[layer].attn_f32 ? ITA_ATTN_F32 : ITA_ATTN_INT8;
  return ITA_OK;
}

int ita_mha_f32(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  return launch_attn_f32(h, layer, x, y, batch, false, (hipStream_t)stream);
}

int ita_encoder_layer(ita_handle h, int layer, const float* x, float* y, int batch, void* stream) {
  if (int rc = check_layer_io(h, layer, x, y, batch)) return rc;
  StreamIo io;
  io.x = x; io.y = y;
  return launch_encoder(h, layer, io, batch, (hipStream_t)stream);
}

int ita_debug_encoder_stamps(ita_handle h, int layer, const float* x, const void* image_u8, float* y, int batch,
                             unsigned long long* stamps, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if ((!x && !image_u8) || !y || !stamps || layer < 0 || layer >= h->w.hdr.num_layers)
    return fail(ITA_ERR_INVALID_ARG, "bad argument");
  if (h->w.layers[layer].attn_f32) return fail(ITA_ERR_UNSUPPORTED, "this layer's attention is float32 (ITAW0003 blob): no stream kernel, no stamps");
  if (image_u8 ? !h->w.layers[layer].simg_tok : !h->w.layers[layer].simg_enc)
    return fail(ITA_ERR_UNSUPPORTED, "this layer does not run on the stream kernel");
  StreamIo io;
  io.x = x; io.y = y; io.stamps = stamps; io.img = image_u8;
  return launch_encoder(h, layer, io, batch, (hipStream_t)stream);
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
  return launch<ita_softmax_rows_kernel>(dim3((rows + 15) / 16), dim3(64), (hipStream_t)stream, logits, probs, rows);
}

int ita_debug_fast_site_ok(float mult) { return fast_site_ok(mult) ? 1 : 0; }
int ita_debug_fused_site(float mult, int* C, float* K) {
  if (!C || !K) return 0;
  return fused_site(mult, ITA_MAGIC128_F, ITA_FUSED_DMAX, C, K) ? 1 : 0;
}
int ita_debug_fused_check(float mult, int form, int C, float* K) {
  float k = 0.0f;
  const int ok = fused_site_check(mult, form == 1 ? ITA_MAGIC32K_F : (form == 2 || form == 3) ? ITA_MAGIC_F : ITA_MAGIC128_F, C, &k, form == 3) ? 1 : 0;
  if (K) *K = k;
  return ok;
}
int ita_debug_layer_fused(ita_handle h, int layer, unsigned* fused_sites, int* fused, int* C6, float* K6) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!fused_sites || !fused || layer < 0 || layer >= h->w.hdr.num_layers)
    return fail(ITA_ERR_INVALID_ARG, "ita_debug_layer_fused: null output or layer out of range");
  const Layer& L = h->w.layers[layer];
  *fused_sites = L.fused_sites;
  *fused = L.fused ? (L.fused_relu ? 2 : 1) : 0;
  for (int i = 0; i < 6; ++i) {
    if (C6) C6[i] = L.fused_c[i];
    if (K6) K6[i] = L.fused_k[i];
  }
  return ITA_OK;
}

int ita_debug_dequant_site(float mult, int dmax, int* C, float* K) {
  if (!C || !K) return 0;
  return fused_site(mult, ITA_MAGIC_F, dmax, C, K, true) ? 1 : 0;
}
int ita_debug_layer_dequant(ita_handle h, int layer, int* fused_dq, int* C2, float* K2) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!fused_dq || layer < 0 || layer >= h->w.hdr.num_layers)
    return fail(ITA_ERR_INVALID_ARG, "ita_debug_layer_dequant: null output or layer out of range");
  const Layer& L = h->w.layers[layer];
  *fused_dq = L.fused_dq ? 1 : 0;
  for (int i = 0; i < 2; ++i) {
    if (C2) C2[i] = L.fused_c[6 + i];
    if (K2) K2[i] = L.fused_k[6 + i];
  }
  return ITA_OK;
}

int ita_debug_x2_planes(ita_handle h, int fill, void* hi, void* lo, int B, int* ld_planes, void* stream) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (ld_planes) *ld_planes = h->w.ldfold;
  if (B <= 0 || B > h->ws.cap || !h->ws.x2_hi || !h->ws.x2_lo)
    return fail(ITA_ERR_INVALID_ARG, "ita_debug_x2_planes: batch beyond the reserved workspace, or no planes");
  const size_t bytes = (size_t)B * h->w.ldfold * sizeof(_Float16);
  hipStream_t s = (hipStream_t)stream;
  if (fill) {
    HIPCHK(hipMemsetAsync(h->ws.x2_hi, fill & 0xff, bytes, s));
    HIPCHK(hipMemsetAsync(h->ws.x2_lo, fill & 0xff, bytes, s));
    return ITA_OK;
  }
  if (!hi || !lo) return fail(ITA_ERR_INVALID_ARG, "ita_debug_x2_planes: null output");
  HIPCHK(hipMemcpyAsync(hi, h->ws.x2_hi, bytes, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(lo, h->ws.x2_lo, bytes, hipMemcpyDeviceToDevice, s));
  return ITA_OK;
}

int ita_debug_layer_forms(ita_handle h, int layer, unsigned* fast_sites, int* stream_images) {
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "no weights loaded");
  if (!fast_sites || !stream_images || layer < 0 || layer >= h->w.hdr.num_layers)
    return fail(ITA_ERR_INVALID_ARG, "bad pointer or layer");
  const Layer& L = h->w.layers[layer];
  *fast_sites = L.fast_sites;
  *stream_images = (L.simg_mha ? ITA_FORMS_ATTN_IMAGE : 0) | (L.simg_enc ? ITA_FORMS_LAYER_IMAGE : 0) |
                       (L.simg_tok ? ITA_FORMS_TOK_IMAGE : 0);
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
  if (int rc = check_frames(height, width, row_stride, frame_stride, batch)) return rc;
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

int ita_tokenizer_long(ita_handle h, const void* src, int pixel_dtype, int height, int width, long long row_stride,
                       long long frame_stride, float depth_scale, int tok_h, int tok_w, float* tokens, int batch, void* stream) {
  // every argument is judged before the handle's weights are looked at and before any HIP call
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (!src || !tokens) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (pixel_dtype != ITA_PIXEL_U8 && pixel_dtype != ITA_PIXEL_U16 && pixel_dtype != ITA_PIXEL_F32)
    return fail(ITA_ERR_INVALID_ARG, "pixel_dtype must be ITA_PIXEL_U8, ITA_PIXEL_U16 or ITA_PIXEL_F32");
  if (int rc = check_frames(height, width, row_stride, frame_stride, batch)) return rc;
  const size_t px = pixel_dtype == ITA_PIXEL_U8 ? 1 : pixel_dtype == ITA_PIXEL_U16 ? 2 : 4;
  if ((uintptr_t)src % px || (uintptr_t)tokens % 16)
    return fail(ITA_ERR_INVALID_ARG, "src must be aligned to its pixel size, tokens to 16 bytes");
  if (pixel_dtype == ITA_PIXEL_U16 && !(depth_scale > 0.0f && depth_scale <= 3.402823466e38f))
    return fail(ITA_ERR_INVALID_ARG, "depth_scale must be finite and positive");
  if (tok_h < 1 || tok_w < 16 || tok_w % 16 || tok_w > 65536 || (long long)tok_h * tok_w % 128 || (long long)tok_h * tok_w > 65536 ||
      batch > 65535)
    return fail(ITA_ERR_UNSUPPORTED, "needs tok_h >= 1, tok_w % 16 == 0, tok_h * tok_w a multiple of 128 up to 65536, batch <= 65535");
  if (!h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "ita_load_weights has not been called");
  // (the image exists when the blob has the conv weights and bias and the LayerNorm: ita_load_weights)
  if (!h->w.tok_simg) return fail(ITA_ERR_BAD_BLOB, "tokenizer parameters missing from the blob");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  // sampled single-stage profiling (ita_profile_begin_sampled with only_stage 0, the tokenizer) also works here
  StageRecorder rec(h, s, false);
  int rc = rec.mark(0, false);
  if (rc) return rc;
  switch (pixel_dtype) {
    case ITA_PIXEL_U8: rc = launch_tokenizer_long<uint8_t>(h, src, height, width, row_stride, frame_stride, depth_scale, tok_h, tok_w, tokens, batch, s); break;
    case ITA_PIXEL_U16: rc = launch_tokenizer_long<uint16_t>(h, src, height, width, row_stride, frame_stride, depth_scale, tok_h, tok_w, tokens, batch, s); break;
    default: rc = launch_tokenizer_long<float>(h, src, height, width, row_stride, frame_stride, depth_scale, tok_h, tok_w, tokens, batch, s);
  }
  if (rc || (rc = rec.mark(0, true))) return rc;
  rec.finish();
  return ITA_OK;
}

int ita_resize_table(int n_in, int n_out, int* n0, int* count, float* coeff, int coeff_width, int* width_out) {
  if (!n0 || !count || !coeff || !width_out || coeff_width < 1) return fail(ITA_ERR_INVALID_ARG, "null pointer or coeff_width < 1");
  ItaResizeAxis t;
  if (!ita_resize_axis(n_in, n_out, t)) return fail(ITA_ERR_INVALID_ARG, "n_in must be in [1, 4096], n_out in [1, 4096]");
  *width_out = t.width;
  if (t.width > coeff_width) return fail(ITA_ERR_INVALID_ARG, "coeff_width is smaller than the table's width (see width_out)");
  for (int o = 0; o < n_out; ++o) {
    n0[o] = t.n0[o];
    count[o] = t.count[o];
    for (int j = 0; j < coeff_width; ++j) coeff[(size_t)o * coeff_width + j] = j < t.width ? t.coeff[(size_t)o * t.width + j] : 0.0f;
  }
  return ITA_OK;
}

int ita_ingest_wire_prepare(ita_handle h, int height, int width) {
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (height < 1 || height > ITA_WIRE_MAX_DIM || width < 1 || width > ITA_WIRE_MAX_DIM)
    return fail(ITA_ERR_INVALID_ARG, "height and width must be in [1, 4096]");
  HIPCHK(hipSetDevice(h->device));
  return prepare_wire(h, height, width, nullptr);
}

int ita_ingest_wire(ita_handle h, const uint8_t* src, int height, int width, long long row_stride, long long frame_stride,
                    uint8_t* wire, int batch, void* stream) {
  // every argument is judged before the handle is used and before any HIP call
  if (!h) return fail(ITA_ERR_INVALID_ARG, "null handle");
  if (!src || !wire) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_frames(height, width, row_stride, frame_stride, batch)) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  WireSize* w = find_wire(h, height, width);
  if (!w) {
    if (capturing(s))
      return fail(ITA_ERR_INVALID_ARG, "this source size has no tables yet and they cannot be built inside a stream capture; call ita_ingest_wire_prepare first");
    const int rc = prepare_wire(h, height, width, &w);
    if (rc) return rc;
  }
  // bands of 12, 8 or 4 output rows with their source rows staged in LDS, the tallest that fits; else bands of 4 read
  // from global memory
  int rows = 4, span = 0;
  if (row_stride % 4 == 0)
    for (int b = 2; b >= 0 && !span; --b)
      if (ita_wire_lds_bytes(width, w->span[b]) <= ITA_WIRE_STAGED_LDS_MAX) {
        rows = 4 * (b + 1);
        span = w->span[b];
      }
  const long long items = (long long)batch * ((ITA_WIRE_H + rows - 1) / rows);
  const int grid = (int)std::min<long long>(items, (long long)h->num_cus * 8);
  const int lds = ita_wire_lds_bytes(width, span);
  // (the unstaged forms hold four W-float rows: within the LDS any kernel may ask for, nothing to register)
  auto run = [&](auto dwords, auto staged) {
    constexpr bool DWORDS = decltype(dwords)::value, STAGED = decltype(staged)::value;
    return launch_lds<ita_ingest_wire_kernel<DWORDS, STAGED>, STAGED ? ITA_WIRE_STAGED_LDS_MAX : 0>(
        dim3(grid), dim3(256), lds, s, src, height, width, row_stride, frame_stride, w->dev, wire, batch, rows, span);
  };
  if (span) return run(std::true_type{}, std::true_type{});
  if (row_stride % 4 == 0) return run(std::true_type{}, std::false_type{});
  return run(std::false_type{}, std::false_type{});
}

int ita_fusion_tail(ita_handle h, const float* x, float* feat, int batch, void* stream) {
  int rc = check(h, batch);
  if (rc) return rc;
  if (!x || !feat) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  return launch_tail(h->num_cus, h->w.hdr.E, h->w.tail_wT, h->w.tail_b, x, feat, 4608, batch, (hipStream_t)stream);
}

int ita_fusion_tail_load(ita_handle h, const float* conv_w, const float* conv_b, int E, int out_ch) {
  int rc = check(h, 1, false);
  if (rc) return rc;
  if (!conv_w || !conv_b) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (E <= 0 || E % 16 || out_ch <= 0 || out_ch > 64) return fail(ITA_ERR_UNSUPPORTED, "needs E % 16 == 0 and out_ch <= 64");
  h->tl = TailLarge{};   // the old tail goes first; the new one is built aside and moved in whole, or not at all
  TailLarge tl;
  const int CIN = E / 4 + E, nchunk = (CIN + 31) / 32, nt = (out_ch + 15) / 16, cop = nt * 16;
  const int e = split_scale_exp(max_abs_of(conv_w, (size_t)out_ch * CIN * 9));   // one scale for every packing below
  const float sc = ldexpf(1.0f, e);
  auto upload = [](const std::vector<uint16_t>& v, DevBuf<_Float16>& d) { return d.upload((const _Float16*)v.data(), v.size()); };
  std::vector<uint16_t> hi((size_t)nchunk * 9 * cop * 32, 0), lo(hi.size(), 0);
  for (int co = 0; co < out_ch; ++co)
    for (int c = 0; c < CIN; ++c)
      for (int tap = 0; tap < 9; ++tap) {
        const size_t d = (((size_t)(c / 32) * 9 + tap) * cop + co) * 32 + (c % 32);
        split_half(conv_w[((size_t)co * CIN + c) * 9 + tap] * sc, &hi[d], &lo[d]);
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
              const size_t d = ((((size_t)tap * 4 + j) * 3 + nt2) * 64 + lane) * 8 + e2;
              split_half(conv_w[((size_t)co * CIN + c) * 9 + tap] * sc, &uh[d], &ul[d]);
            }
    std::vector<uint16_t> sh((size_t)9 * 48 * 32, 0), sl(sh.size(), 0);
    for (int co = 0; co < out_ch; ++co)
      for (int c = 0; c < 32; ++c)
        for (int tap = 0; tap < 9; ++tap) {
          const size_t d = ((size_t)tap * 48 + co) * 32 + c;
          split_half(conv_w[((size_t)co * CIN + c) * 9 + tap] * sc, &sh[d], &sl[d]);
        }
    HIPCHK(upload(sh, tl.ps_hi));
    HIPCHK(upload(sl, tl.ps_lo));
    HIPCHK(upload(uh, tl.up_hi));
    HIPCHK(upload(ul, tl.up_lo));
  }
  HIPCHK(upload(hi, tl.hi));
  HIPCHK(upload(lo, tl.lo));
  HIPCHK(tl.bias.upload(bias.data(), bias.size()));
  tl.inv_scale = ldexpf(1.0f, -e);
  tl.E = E; tl.CO = out_ch; tl.nt = nt; tl.nchunk = nchunk;
  h->tl = std::move(tl);
  return ITA_OK;
}

int ita_fusion_tail_large(ita_handle h, const float* x, float* out, int batch, int tok_h, int tok_w, void* stream) {
  int rc = check(h, batch, false);
  if (rc) return rc;
  if (!x || !out) return fail(ITA_ERR_INVALID_ARG, "null pointer");
  if (!h->tl.hi) return fail(ITA_ERR_NO_WEIGHTS, "ita_fusion_tail_load has not been called");
  if (tok_h < 4 || tok_w < 16 || (2 * tok_h) % 8 || (2 * tok_w) % 32 || batch > 65535)
    return fail(ITA_ERR_UNSUPPORTED, "needs tok_h % 4 == 0, tok_w % 16 == 0, batch <= 65535");
  ItaTailBigArgs a{x, h->tl.hi, h->tl.lo, h->tl.bias, h->tl.inv_scale, out, batch, h->tl.E, tok_h, tok_w, h->tl.CO, h->tl.nchunk, 0};
  hipStream_t s = (hipStream_t)stream;
  // E = 128: the upsampled channels (4/5 of the contraction) by linearity on the low-resolution tokens (ita_tail_up_kernel),
  // the pixel-shuffle channels (= chunk 0 of the implicit GEMM) in phase 2 of the same kernel.  Needs whole 16 x 32 tiles and
  // every tile's source region inside 10 x 18 tokens (same float expressions as the kernel; true for every x2 grid tried,
  // checked instead of assumed).  Every other shape runs on ita_tail_big_kernel.
  if (h->tl.up_hi && (2 * tok_h) % 16 == 0 && (2 * tok_w) % 32 == 0) {
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
      ItaTailUpArgs u{x, h->tl.up_hi, h->tl.up_lo, h->tl.ps_hi, h->tl.ps_lo, h->tl.bias, h->tl.inv_scale, out, batch, tok_h, tok_w, h->tl.CO};
      const long ntiles = (long)(OW / 32) * (OH / 16) * batch;      // persistent: one workgroup per CU, tiles dealt round robin
      return launch<ita_tail_up_kernel, ItaTailUpLds::TOTAL>(dim3((unsigned)(ntiles < h->num_cus ? ntiles : h->num_cus)), dim3(512), s, u);
    }
  }
  switch (h->tl.nt) {
    case 1: return launch_tail_big<1>(a, s);
    case 2: return launch_tail_big<2>(a, s);
    case 3: return launch_tail_big<3>(a, s);
    default: return launch_tail_big<4>(a, s);
  }
}

// what the LSTM head and its sequence form read of the model, and the GEMM's split-K partials `part`
static ItaLstmModelArgs lstm_model_args(const ita_context* h, const float* part) {
  const auto& w = h->w;
  ItaLstmModelArgs m;
  m.part = part;          m.inv_fold_scale = w.fold_inv_scale;
  m.w0_hi = w.lw_hi[0];   m.w0_lo = w.lw_lo[0];   m.inv_wscale0 = w.lw_inv_scale[0];
  m.bias0 = w.fold_bias;
  m.w1_hi = w.lw_hi[1];   m.w1_lo = w.lw_lo[1];   m.inv_wscale1 = w.lw_inv_scale[1];
  m.w2_hi = w.lw_hi[2];   m.w2_lo = w.lw_lo[2];   m.inv_wscale2 = w.lw_inv_scale[2];
  m.bsum1 = w.bsum[1];    m.bsum2 = w.bsum[2];
  return m;
}
// both kernels' grid: sixteen workgroups (unit tiles) per tile of 32 frames / streams
static dim3 lstm_grid(int B) { return dim3(16 * ((B + 31) / 32)); }

// the LSTM head behind the folded GEMM: layers 0, 1, 2 and the fc in one launch (ita_lstm_head_kernel), reading the
// GEMM's split-K partials `part`.  State rows are slots[b] (else b) of (3, rows, 128) arrays with layer stride lstride;
// h_out / c_out may alias h_in / c_in.
static int launch_lstm_head(ita_context* h, const float* part, const float* desvel, const float* quat, const float* h_in,
                            const float* c_in, float* h_out, float* c_out, size_t lstride, float* vel, int B,
                            const int* slots, hipStream_t s) {
  ItaLstmHeadArgs p{lstm_model_args(h, part), desvel, quat, h_in, c_in, h_out, c_out, lstride,
                    h->ws.c1_hi, h->ws.c1_lo, h->ws.c2_hi, h->ws.c2_lo, h->w.fc_w, h->w.fc_b, vel, h->ws.head_sync + ITA_HEAD_CNT_STRIDE, h->ws.head_sync, B, slots};
  return launch<ita_lstm_head_kernel<NSPLIT>>(lstm_grid(B), dim3(256), s, p);
}

// its sequence form (ita_lstm_seq_kernel): n steps of B streams from partial buffer 0, whose row t * B + b is stream b's
// frame of step t; desvel, quat and vel point at the first of these steps, which is step t0 of the sequence `lengths` counts
static int launch_lstm_seq(ita_context* h, const float* desvel, const float* quat, float* state_h, float* state_c,
                           const int* lengths, int t0, float* vel, int B, int n, hipStream_t s) {
  ItaLstmSeqArgs p{lstm_model_args(h, h->ws.part), desvel, quat, state_h, state_c, lengths, t0, h->ws.seq_ho,
                   h->w.fc_w, h->w.fc_b, vel, h->ws.head_sync + ITA_HEAD_CNT_STRIDE, h->ws.head_sync, B, n};
  return launch<ita_lstm_seq_kernel<NSPLIT>>(lstm_grid(B), dim3(256), s, p);
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
  if (!h->w.dec_w || !h->w.wcat[0] || !h->w.fc_w || (h->w.hdr.has_tail && !h->w.tail_wT))
    return fail(ITA_ERR_BAD_BLOB, "blob holds no decoder / LSTM (/ fusion tail) parameters");
  if (h->w.hdr.has_tail && h->w.hdr.E != 64) return fail(ITA_ERR_UNSUPPORTED, "the fusion tail is built for E = 64 (ITAViTLSTM)");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = batch;
  const size_t tokb = sizeof(float) * (size_t)B * 128 * h->w.hdr.E;
  const bool fast = h->tail_mode == 1 && h->w.folded;
  if (slots && !fast) return fail(ITA_ERR_UNSUPPORTED, "slot-indexed state needs tail mode 1");
  const size_t lstride = (size_t)(slots ? state_rows : batch) * 128;   // layer stride of the (3, rows, 128) state
  StageRecorder rec(h, s, true);
  if ((rc = rec.mark())) return rc;
  const bool fused_tok = !x2_in && fuse_tokenizer(h, image_dtype);
  if (slots && !x2_in) {   // refuse before the first launch: the slot-indexed form is served by the stream kernel only
    const Layer& LL = h->w.layers.back();
    if (!LL.ffn_f32 && !((fused_tok && h->w.hdr.num_layers == 1) ? LL.simg_tok : LL.simg_enc))
      return fail(ITA_ERR_UNSUPPORTED, "slot-indexed state needs the stream kernel (this blob's accumulator range or head count rules it out)");
  }
  if (x2_in) {
    HIPCHK(hipMemcpyAsync(h->ws.bufA, x2_in, tokb, hipMemcpyDeviceToDevice, s));
    if (fast) {
      const size_t n = (size_t)B * 128 * h->w.hdr.E;
      if ((rc = launch<ita_split_planes_kernel>(dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), s, h->ws.bufA, h->ws.x2_hi,
                                                h->ws.x2_lo, 128 * h->w.hdr.E, h->w.ldfold, B))) return rc;
    }
  } else if (!fused_tok && (rc = launch_tokenizer(h, image, image_dtype, h->ws.bufA, B, s))) return rc;
  if ((rc = rec.mark())) return rc;
  if (!x2_in && !fused_tok && taps && taps->tokens) HIPCHK(hipMemcpyAsync(taps->tokens, h->ws.bufA, tokb, hipMemcpyDeviceToDevice, s));
  for (int l = 0; l < (x2_in ? 0 : h->w.hdr.num_layers); ++l) {
    const bool last = l == h->w.hdr.num_layers - 1;
    const bool planes = fast && last;
    StreamIo io;   // one encoder layer, in place on bufA
    io.x = h->ws.bufA;
    io.y = (planes && !(taps && taps->x2)) ? nullptr : h->ws.bufA;
    if (planes) { io.y_hi = h->ws.x2_hi; io.y_lo = h->ws.x2_lo; }
    if (taps && last) io.x1_tap = taps->x1;
    io.slots = slots;
    if (fused_tok && l == 0) { io.img = image; io.tok_tap = taps ? taps->tokens : nullptr; }
    io.mid = &rec;   // a layer of two launches records the attention / FFN boundary between them
    const int mid_mark = rec.next;
    if ((rc = launch_encoder(h, l, io, B, s))) return rc;
    if (rec.next == mid_mark && (rc = rec.mark())) return rc;
    if ((rc = rec.mark())) return rc;
  }
  if (x2_in && ((rc = rec.mark()) || (rc = rec.mark()))) return rc;
  if (taps && taps->x2) HIPCHK(hipMemcpyAsync(taps->x2, h->ws.bufA, tokb, hipMemcpyDeviceToDevice, s));
  if (fast) {
    // folded tail+decoder: dec = x2 . Wfold^T + bias'   (x2 planes were written by the last FFN)
    if ((rc = launch_gemm_split<128, 128, 2, 4>(h->ws.x2_hi, h->ws.x2_lo, h->w.ldfold, h->w.fold_hi, h->w.fold_lo, h->w.ldfold, h->ws.part, B,
                                                512, h->w.kfold, NSPLIT, s, h->w.foldf_hi, h->w.foldf_lo))) return rc;
    if ((rc = rec.mark()) || (rc = rec.mark())) return rc;
    if ((rc = launch_lstm_head(h, h->ws.part, desvel, quat, h_in, c_in, h_out, c_out, lstride, vel, B, slots, s))) return rc;
    if ((rc = rec.mark())) return rc;
  } else {
    if (h->w.hdr.has_tail) {
      if ((rc = launch_tail(h->num_cus, h->w.hdr.E, h->w.tail_wT, h->w.tail_b, h->ws.bufA, h->ws.feat, 4608, B, s))) return rc;
      if ((rc = rec.mark())) return rc;
      if (taps && taps->feat)
        HIPCHK(hipMemcpyAsync(taps->feat, h->ws.feat, sizeof(float) * (size_t)B * 4608, hipMemcpyDeviceToDevice, s));
      // decoder writes straight into the LSTM layer-0 concat buffer (columns 0..511)
      if ((rc = launch_gemm(h->ws.feat, 4608, h->w.dec_w, 4608, h->w.dec_b, h->ws.cat0, K0P, B, 512, 4608, s))) return rc;
    } else {   // no fusion tail: the decoder reads the flattened tokens, (B,128,E) as it stands in bufA
      if ((rc = rec.mark())) return rc;
      if ((rc = launch_gemm(h->ws.bufA, h->w.kfold, h->w.dec_w, h->w.kfold, h->w.dec_b, h->ws.cat0, K0P, B, 512, h->w.kfold, s))) return rc;
    }
    if ((rc = rec.mark())) return rc;
    if (taps && taps->dec)
      HIPCHK(hipMemcpy2DAsync(taps->dec, 512 * sizeof(float), h->ws.cat0, K0P * sizeof(float), 512 * sizeof(float), B,
                              hipMemcpyDeviceToDevice, s));
    ItaLstmPrepArgs prep{desvel, quat, h_in, h->ws.cat0, h->ws.cat1, h->ws.cat2, K0P, B};
    if ((rc = launch<ita_lstm_prep_kernel>(dim3(B), dim3(256), s, prep))) return rc;
    float* cats[3] = {h->ws.cat0, h->ws.cat1, h->ws.cat2};
    const int kp[3] = {K0P, 256, 256};
    for (int l = 0; l < 3; ++l) {
      if ((rc = launch_gemm(cats[l], kp[l], h->w.wcat[l], kp[l], h->w.bsum[l], h->ws.gates, 512, B, 512, kp[l], s))) return rc;
      ItaLstmPointArgs p{h->ws.gates, c_in + (size_t)l * B * 128, h_out + (size_t)l * B * 128, c_out + (size_t)l * B * 128,
                         l < 2 ? cats[l + 1] : nullptr, 256, B};
      if ((rc = launch<ita_lstm_point_kernel>(dim3((B * 128 + 255) / 256), dim3(256), s, p))) return rc;
    }
    if ((rc = launch<ita_fc_kernel>(dim3((B * 3 + 63) / 64), dim3(64), s, h_out + (size_t)2 * B * 128, h->w.fc_w, h->w.fc_b, vel, B,
                                    (const int*)nullptr))) return rc;   // (rows in order: no slots)
    if ((rc = rec.mark())) return rc;
  }
  rec.finish();
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
  if (!(h->tail_mode == 1 && h->w.folded)) return fail(ITA_ERR_UNSUPPORTED, "front/back form needs tail mode 1 and a full ITAViTLSTM blob");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream))) return rc;
  if (parts & 2) h->ws.front_cap[buf] = h->ws.cap;
  hipStream_t s = (hipStream_t)stream;
  _Float16* const xh = h->ws.x2_hi + (size_t)xbuf * h->ws.cap * h->w.ldfold;
  _Float16* const xl = h->ws.x2_lo + (size_t)xbuf * h->ws.cap * h->w.ldfold;
  // sampled single-stage profiling (ita_profile_begin_sampled with only_stage 0, 1 or 3) also works here
  StageRecorder rec(h, s, false);
  if (parts & 1) {
    if ((rc = rec.mark(0, false))) return rc;
    const bool fused_tok = fuse_tokenizer(h, image_dtype);
    if (!fused_tok && (rc = launch_tokenizer(h, image, image_dtype, h->ws.bufA, batch, s))) return rc;
    if ((rc = rec.mark(0, true)) || (rc = rec.mark(1, false))) return rc;
    for (int l = 0; l < h->w.hdr.num_layers; ++l) {
      const bool last = l == h->w.hdr.num_layers - 1;
      StreamIo io;
      io.x = h->ws.bufA;
      if (last) { io.y_hi = xh; io.y_lo = xl; } else io.y = h->ws.bufA;
      if (fused_tok && l == 0) io.img = image;
      if ((rc = launch_encoder(h, l, io, batch, s))) return rc;
    }
    if ((rc = rec.mark(1, true))) return rc;
    if (encoder_done_event) HIPCHK(hipEventRecord((hipEvent_t)encoder_done_event, s));
  }
  if (parts & 2) {
    if ((rc = rec.mark(3, false))) return rc;
    float* part = h->ws.part + (size_t)buf * NSPLIT * h->ws.cap * 512;
    if ((rc = launch_gemm_split<128, 128, 2, 4>(xh, xl, h->w.ldfold, h->w.fold_hi, h->w.fold_lo, h->w.ldfold, part, batch, 512,
                                                h->w.kfold, NSPLIT, s, h->w.foldf_hi, h->w.foldf_lo))) return rc;
    if ((rc = rec.mark(3, true))) return rc;
  }
  rec.finish();
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
  if (!(h->tail_mode == 1 && h->w.folded)) return fail(ITA_ERR_UNSUPPORTED, "front/back form needs tail mode 1 and a full ITAViTLSTM blob");
  if (batch > h->ws.cap || h->ws.front_cap[buf] != h->ws.cap)
    return fail(ITA_ERR_INVALID_ARG, "ita_vitlstm_front has not filled this buffer for the current workspace (reserve before front)");
  hipStream_t s = (hipStream_t)stream;
  const int B = batch;
  const size_t lstride = (size_t)B * 128;
  const float* part = h->ws.part + (size_t)buf * NSPLIT * h->ws.cap * 512;
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
    h->pipe_cap = 0;
    HIPCHK(h->pipe_h.alloc(2 * nstate));
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
  if (!(h->tail_mode == 1 && h->w.folded)) return fail(ITA_ERR_UNSUPPORTED, "the sequence form needs tail mode 1 and a full ITAViTLSTM blob");
  if (h->prof) return fail(ITA_ERR_INVALID_ARG, "ita_vitlstm_sequence cannot run between ita_profile_begin and ita_profile_end");
  if ((rc = ensure_workspace(h, batch, (hipStream_t)stream))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int B = batch, Tc = h->ws.cap / B;   // >= 1: the workspace holds at least B frames
  const size_t frame_bytes = (size_t)60 * 90 * (image_dtype == ITA_IMAGE_U8 ? 1 : sizeof(float));
  for (int t0 = 0; t0 < n_steps; t0 += Tc) {
    const int n = std::min(Tc, n_steps - t0);
    const size_t row0 = (size_t)t0 * B;
    if ((rc = front_impl(h, (const char*)image + row0 * frame_bytes, image_dtype, n * B, 0, stream, nullptr))) return rc;
    if ((rc = launch_lstm_seq(h, desvel + row0, quat + row0 * 4, state_h, state_c, lengths, t0, vel + row0 * 3, B, n, s))) return rc;
  }
  h->ws.front_cap[0] = 0;   // partial buffer 0 holds time-major rows of several steps: not something ita_vitlstm_back may read
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
  const size_t need = (size_t)max_forwards * StageRecorder::events_per_forward(h);
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
  const int L = h->w.hdr.num_layers, per = StageRecorder::events_per_forward(h);
  for (int i = 0; i < ITA_NUM_STAGES; ++i) stage_ms[i] = 0.0;
  for (int f = 0; f < h->prof_n; ++f) {
    hipEvent_t* ev = &h->prof_ev[(size_t)f * per];
    HIPCHK(hipEventSynchronize(ev[h->prof_stage >= 0 ? stage_marks(L, h->prof_stage).hi : per - 1]));
    auto dt = [&](int a, int b, double* acc) -> int {
      float ms = 0.0f;
      HIPCHK(hipEventElapsedTime(&ms, ev[a], ev[b]));
      *acc += ms;
      return ITA_OK;
    };
    int rc;
    if (h->prof_stage >= 0) {     // single-stage mode: only that stage's two marks exist
      const StageMarks m = stage_marks(L, h->prof_stage);
      if ((rc = dt(m.lo, m.hi, &stage_ms[h->prof_stage]))) return rc;
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
  if (!h || !h->w.loaded) return fail(ITA_ERR_NO_WEIGHTS, "bind needs a context with weights");
  if (layer < 0 || layer >= h->w.hdr.num_layers) return fail(ITA_ERR_INVALID_ARG, "layer out of range");
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
