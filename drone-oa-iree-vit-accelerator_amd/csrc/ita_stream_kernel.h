// ita_stream_kernel.h -- the ITA encoder layer as eight wave-private token streams per CU.
//
//   x1 = LayerNorm1(x + ITASelfAttention_QAT(x));  y = LayerNorm2(x1 + ITAFeedForward_QAT(x1))
//   (reference models/ITA_single_layer_upsample_shuffle/QAT/model.py:100-113,
//    models/ITA/QAT/layers.py:39-45,61-75,101-127, models/ITA/QAT/ITA_softmax.py:51-61)
//
// Same arithmetic, bit for bit, as ita_mha_kernel + ita_ffn_kernel (ita_int8_kernels.h) and the CPU
// oracle; what is different is who owns what.  One persistent 512-thread workgroup per CU; wave w owns
// tokens 16w .. 16w+15 of the current frame (token row w of the 8 x 16 grid) from the pixels to the
// LayerNorm2 output.  Lane (qi = lane & 15, kq = lane >> 4) holds channels (E/4)kq .. (E/4)kq + E/4 - 1 of
// token 16w + qi in f32 registers for the residuals.
//
// Every GEMM of the layer is a 16x16x64 int8 MFMA with the WEIGHTS as the A operand (read from a
// resident LDS image) and the wave's OWN activations as the B operand, taken from registers: the C
// layout of that MFMA (lane = token column, four consecutive feature rows) packs, four tiles at a time,
// into exactly one B fragment of the next GEMM -- the integer sum does not care which k a fragment byte
// is, only that the weight image uses the same slot -> k mapping, and that mapping is baked into the
// image at load time (ita_plugin.hip: build_stream_image).  So x_q, Q, the context, the FFN hidden layer
// and both block outputs never touch LDS; only K and V^T do, because every wave needs every key.
// Two barriers per frame (K/V^T complete; K/V^T free again) instead of eight, and no token of a frame
// ever waits for another wave's tile.
//
// LDS (E = 64, fused tokenizer): weight image 80 KB + biases/LayerNorm 5.3 KB + conv weights 13.3 KB
// (f32 MFMA fragments) | K 24 KB | V^T 24 KB | column sums | eight private 9 x 96 byte windows of the next
// frame = 161 744 B of the CU's 160 KB (163 840).  E = 128 (no tokenizer; fc1 / fc2 weights stay in global memory): 158 464 B.
#pragma once
#include "ita_int8_kernels.h"
#include "ita_tokenizer_kernel.h"

struct ItaStreamArgs {
  const char* image;      // device copy of the LDS image (ItaStreamLds<...>::IMAGE bytes, built at load time)
  const float* x;         // (B,128,E) tokens (TOK == 0)
  float* y;               // (B,128,E) f32 output, may be null when planes are given
  _Float16 *y_hi, *y_lo;  // optional f16 hi/lo planes of y, row stride ld_planes per frame
  int ld_planes;
  float* x1_tap;          // optional (B,128,E): LayerNorm1 output
  float inv_sx, mq, mk, mv, ml, mc, mo, so;      // attention scalars (ita_weights.h)
  float f_inv_sx, m1, m2, s2;                    // FFN scalars
  int B;
  int fuse_ln;            // attention-only form: y = fuse_ln ? LayerNorm1(x + attn(x)) : attn(x)
  // diagnostic only (null in production): waves 0 and 4 of each workgroup store s_memtime at the phase
  // boundaries of the first 8 frames: stamps[((block * 8 + frame) * 2 + (wave >> 2)) * 16 + slot]
  unsigned long long* stamps;
  // optional side copy for the LSTM that follows: layer-0 hidden state of frame b (row slots[b] or b of h0_src) ->
  // h0_dst[b].  Layer 0 reads whole rows of h while other workgroups overwrite parts of the same row when the state
  // is updated in place; the staged copy removes that race.
  const float* h0_src;
  float* h0_dst;
  const int* slots;
  // int8 in / int8 out form of the attention block (IO8: the accelerator-native boundary):
  const int8_t* xq;       // (B,128,E) quantised block input
  int8_t* yq;             // (B,128,E) out_proj codes (no dequantisation, no residual)
  const void* img;        // (B,60,90) u8 wire frames (TOK == 1)
  float* tok_tap;         // optional (B,128,E): the tokens
  // bit s set: requantisation site s may use the single-rounding form (one v_pk_fma_f32 instead of multiply + magic add):
  // ita_load_weights has enumerated every accumulator value of the site's clamp range and found the two forms equal.
  // Informational inside the kernel: the launcher picks the FAST instantiation when all six bits are set.
  unsigned fast_sites;
  // the FUSED instantiation (the launcher picks it when every fused site of the layer is proven, ita_weights_load.h:
  // fused_site): the logits' and the column sums' accumulator bases C_L, C_C; each site's K_site = magic - round(C_site m_site)
  // is the second half of its mk* pair below.  The bases of Q, K and V are in the image's biases.  Unused by the other instantiations.
  int c_l, c_c;
  // Each site's {multiplier, K} as one 8-byte kernel argument: it arrives as an aligned SGPR pair, the operand of the
  // site's v_pk_fma_f32 (ita_device.h: ITA_PK_MK).  k1: fc1's fused ReLU form (FUSED >= 2; its base is in the image's b1);
  // ko, k2: out_proj's and fc2's fused dequantise form (FUSED == 3; bases in bo and b2)
  f32x2 mkq, mkk, mkv, mkl, mkc, mk1, mko, mk2;
};
enum { ITA_SITE_Q = 1, ITA_SITE_K = 2, ITA_SITE_V = 4, ITA_SITE_L = 8, ITA_SITE_C = 16, ITA_SITE_O = 32, ITA_SITES_ALL = 63,
       ITA_SITES_FUSED = 31 /* the sites the fused instantiation changes: all but out_proj */,
       ITA_SITE_FC1 = 32 /* in the FUSED mask only (the fast mask's bit 5 is out_proj): fc1's fused ReLU form */,
       ITA_SITE_DQ_O = 64, ITA_SITE_DQ_FC2 = 128 /* FUSED mask only: the fused dequantise form of out_proj and fc2 */,
       ITA_SITES_DQ = 192 };

#define ITA_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)

template <int E, bool FFN, bool TOK>
struct ItaStreamLds {
  static constexpr int S = 128, P = 192, F = 256;
  // ---- image: copied verbatim from global memory once per workgroup
  static constexpr int WQ = 0;                       // int8 [E/16][192][16]  chunk-major, natural k
  static constexpr int WK = WQ + P * E;
  static constexpr int WV = WK + P * E;
  static constexpr int WO = WV + P * E;              // int8 [12][E][16]     fragment order (see build_stream_image)
  // E = 128: attention weights (98 KB) + K / V^T (49 KB) fill the LDS, so fc1 / fc2 (64 KB) stay in GLOBAL memory (the image
  // continues behind the part that is copied to LDS) and are read as fragments, L2-resident, once per frame
  static constexpr bool W12G = FFN && E > 64;
  static constexpr int W1 = WO + E * P;              // int8 [E/16][256][16] natural k
  static constexpr int W2 = W1 + ((FFN && !W12G) ? F * E : 0);  // int8 [16][E][16]     fragment order
  static constexpr int BIAS = W2 + ((FFN && !W12G) ? E * F : 0);   // int32: bq | bk | bv | bo | b1 | b2
  static constexpr int NBIAS = 3 * P + E + (FFN ? F + E : 0);
  static constexpr int LNP = BIAS + NBIAS * 4;       // f32: n1w | n1b | n2w | n2b | tok_lnw | tok_lnb
  static constexpr int NLN = 2 * E + (FFN ? 2 * E : 0) + (TOK ? 2 * E : 0);
  static constexpr int CW = LNP + NLN * 4;           // integer conv tables (ItaTokTab<E>): weight byte planes | init sums | scales, bias
  static constexpr int TAP = CW + (TOK ? ItaTokTab<E>::BYTES : 0);   // int32 [52]: window offset ky * 96 + kx of tap t (0 for t >= 49)
  static constexpr int VB4 = TAP + (TOK ? 52 * 4 : 0);          // int32 [192][4]: bv replicated (V accumulators start per COLUMN)
  static constexpr int IMAGE = VB4 + P * 16;
  static constexpr int GW1 = IMAGE, GW2 = GW1 + F * E;               // W12G: offsets in the global image
  static constexpr int GIMAGE = W12G ? GW2 + E * F : IMAGE;          // bytes of the device image
  // ---- built / used at run time
  static constexpr int K = IMAGE;                    // int8 [12][128][16]  fragment order
  static constexpr int VT = K + S * P;               // int8 [8][192][16]   V^T, keys permuted (ita_int8_kernels.h)
  static constexpr int COLSUM = VT + P * S;          // int32 [2][192]: 128 * column sums of V, per frame parity
  static constexpr int IMG = COLSUM + 2 * P * 4;     // u8 [8 waves][9][96]: rows 2*y0-3 .. 2*y0+5 of the next frame, 3 zero columns each side
  static constexpr int IMG_WAVE = ITA_TOK_U8_WIN;
  static constexpr int TOTAL = IMG + (TOK ? 8 * IMG_WAVE : 0);
  static_assert(IMAGE % 16 == 0 && K % 16 == 0 && IMG % 16 == 0, "16-byte alignment");
  static_assert(TOTAL <= 160 * 1024, "LDS budget");
};

// ITA_ABLATE (diagnostic builds only, results are wrong): 1 no requantisation VALU, 2 no int8 MFMA, 4 no tokenizer,
// 8 no LDS operand reads, 16 no LayerNorm, 32 no softmax, 64 no barriers, 128 no h0 copy / output stores, 256 one plane store,
// 512 no window reads in the tokenizer's blend, 1024 no conv tiles -- what remains is timed against the full kernel to see what
// a frame's time is made of.  (The default, 0, is set in ita_device.h: layernorm_q16 there and the blend in ita_tokenizer_kernel.h have hooks.)
__device__ __forceinline__ i32x4 mfma16(i32x4 a, i32x4 b, i32x4 c) {
  if constexpr (ITA_ABLATE & 2) return c;   // (operand loads become dead code too)
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ i32x4 sfrag(const char* lds, int off) {
  if constexpr (ITA_ABLATE & 8) return (i32x4){off, off, off, off};
  return *(const i32x4*)(lds + off);
}

// Integer softmax (models/ITA/QAT/ITA_softmax.py:51-61) of the 16 rows a wave holds as packed signed 16-bit logit pairs
// -- lane (qi, kq): w[2kt + j] = {logit, logit'} of keys 16kt + 4kq + 2j, +1 of row qi -- entirely on v_pk_*_16, two keys
// per VALU op:  shift = max - x,  num = 256 >> shift,  inv = floor(255 * 2^16 / sum),  y = (num * inv) >> 16 = (inv >> 8)
// >> shift.  Out: the A.V MFMA's B fragments, pf[kb] byte 4t+i = (y - 128) of key 64kb + 16t + 4kq + i (the u8
// probabilities ride a signed MFMA as p - 128; the 128 * colsum(V) term restores them).
typedef short ita_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short ita_u16x2 __attribute__((ext_vector_type(2)));
// The logits arrive UNCLAMPED and biased, u = rne(acc * m) + 32768 (order-preserving u16, lg8_v3); the reference's clamp to
// [-128, 127] happens here at no cost:  m' = clamp(max, -128, 127);  shift = m' - clamp(x)  =  min(max(m' - x, 0), m' + 128)
// -- the saturating unsigned subtraction is the max(., 0) (x above the clamped maximum), and the row-wise cap
// min(m' + 128, 15) covers both x below -128 and the 15 beyond which every shift gives 0.
__device__ __forceinline__ void ita_softmax_packed16(const ita_u16x2 (&w)[16], i32x4 (&pf)[2]) {
  typedef ita_u16x2 u16x2;
  u16x2 m2 = w[0];
#pragma unroll
  for (int j = 1; j < 16; ++j) m2 = __builtin_elementwise_max(m2, w[j]);
  int m = max1632_i(max((int)m2.x, (int)m2.y));
  m = min(max(m, 32768 - 128), 32768 + 127);
  const u16x2 mm = {(unsigned short)m, (unsigned short)m};
  const unsigned short capv = (unsigned short)min(m - (32768 - 128), 15);   // 256 >> s and inv_hi >> s are both 0 from s = 9 on
  const u16x2 cap = {capv, capv};
  const u16x2 one = {256, 256};
  u16x2 sh[16], sum2 = {0, 0};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    sh[j] = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[j]), cap);
    sum2 += one >> sh[j];
  }
  int sum = sum1632_i((int)sum2.x + (int)sum2.y);   // <= 16 * 256 per half: no 16-bit overflow
  sum = max(sum, 1);
  const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;   // <= 255: sum >= 256
  const u16x2 iv = {(unsigned short)inv_hi, (unsigned short)inv_hi};
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int kt = 4 * kb + t;
      const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv >> sh[2 * kt]));
      const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv >> sh[2 * kt + 1]));
      pf[kb][t] = (int)(__builtin_amdgcn_perm(p23, p01, 0x06040200u) ^ 0x80808080u);
    }
}

// Test entry for that function alone: rows of int8 logits (R,128) -> u8 probabilities, 16 rows per wave in exactly the
// register layout the encoder kernel has them in.  Lets the parity tests feed chosen rows (all equal, one-hot, the
// shift 8 / 9 boundary, +-127 / -128) through the GPU formulation, which otherwise only ever sees what QK^T produces.
__global__ __launch_bounds__(64) void ita_softmax_rows_kernel(const int8_t* __restrict__ logits, uint8_t* __restrict__ probs, int rows) {
  const int lane = threadIdx.x, qi = lane & 15, kq = lane >> 4;
  const int row = min((int)blockIdx.x * 16 + qi, rows - 1);
  ita_u16x2 w[16];
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const int v = *(const int*)(logits + (size_t)row * 128 + 16 * kt + 4 * kq);
    w[2 * kt] = (ita_u16x2){(unsigned short)((int)(int8_t)v + 32768), (unsigned short)((int)(int8_t)(v >> 8) + 32768)};
    w[2 * kt + 1] = (ita_u16x2){(unsigned short)((int)(int8_t)(v >> 16) + 32768), (unsigned short)((int)(int8_t)(v >> 24) + 32768)};
  }
  i32x4 pf[2];
  ita_softmax_packed16(w, pf);
  if ((int)blockIdx.x * 16 + qi < rows) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        *(unsigned*)(probs + (size_t)row * 128 + 64 * kb + 16 * t + 4 * kq) = (unsigned)pf[kb][t] ^ 0x80808080u;
  }
}

// ---- software pipeline pieces.  One "group" = four 16-feature output tiles of this wave's 16 tokens.  Its LDS
// operands (weight fragments + the accumulator initialisers) are fetched one step ahead of its MFMAs, and its
// requantisation runs one step behind them, so neither the LDS latency nor the MFMA latency is ever waited for:
//     step g:  load(g+1) | mfma(g) | epilogue(g-1)
template <int N>
struct ItaFr {
  i32x4 w[N];   // weight fragments, tile-major: w[t * (N/4) + k-step]
};
// natural-k chunk-major image [E/16][ROWS][16]; the accumulators start from bias rows 16(tile0+t) + 4kq .. +3
template <int NK, int ROWS>
__device__ __forceinline__ void ld_nat(ItaFr<4 * NK>& f, i32x4 (&acc)[4], const char* img, const int* lds_bias, int tile0,
                                       int qi, int kq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = *(const i32x4*)(lds_bias + (tile0 + t) * 16 + 4 * kq);
#pragma unroll
    for (int c = 0; c < NK; ++c) f.w[t * NK + c] = sfrag(img, ((NK * kq + c) * ROWS + (tile0 + t) * 16 + qi) << 4);
  }
}
// the same image read as the B operand (V projection: roles swapped, column = feature qi): bias is per column
template <int NK, int ROWS>
__device__ __forceinline__ void ld_natv(ItaFr<4 * NK>& f, i32x4 (&acc)[4], const char* img, const int* lds_bias, int tile0,
                                        int qi, int kq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = *(const i32x4*)(lds_bias + ((tile0 + t) * 16 + qi) * 4);   // replicated table: one 16-byte read, no splat
#pragma unroll
    for (int c = 0; c < NK; ++c) f.w[t * NK + c] = sfrag(img, ((NK * kq + c) * ROWS + (tile0 + t) * 16 + qi) << 4);
  }
}
// one k-step (four tiles) of a fragment-order image [4*NKS][E][16] of a block output projection (out_proj, fc2):
// row 16 et + rho <-> channel (E/4)(rho>>2) + 4 et + (rho&3), so that lane (qi, kq) receives its own channels
// (E/4)kq + 4 et + i; and its MFMAs
struct ItaF4 { i32x4 w[4]; };
template <int E>
__device__ __forceinline__ void ld_frg_ks(ItaF4& f, const char* img, int et0, int ks, int qi, int kq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) f.w[t] = sfrag(img, ((4 * ks + kq) * E + (et0 + t) * 16 + qi) << 4);
}
__device__ __forceinline__ void mm_ks(const ItaF4& f, const i32x4& x, i32x4 (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = mfma16(f.w[t], x, acc[t]);
}
template <int E>
__device__ __forceinline__ void ld_obias(i32x4 (&acc)[4], const int* lds_bias, int et0, int kq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = *(const i32x4*)(lds_bias + (E / 4) * kq + 4 * (et0 + t));
}
// acc[t] += sum_k  W-fragment x activation fragment   (SWAP: the activations are the A operand)
template <int NKS, bool SWAP>
__device__ __forceinline__ void mm_group(const ItaFr<4 * NKS>& f, const i32x4 (&x)[NKS], i32x4 (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      acc[t] = SWAP ? mfma16(x[ks], f.w[t * NKS + ks], acc[t]) : mfma16(f.w[t * NKS + ks], x[ks], acc[t]);
}
// requantise four tiles and pack them: ONE B fragment of the next GEMM (byte 4t+i <-> row 4kq+i of tile t).
// fast (wave-uniform): this site's multiplier passed the load-time single-rounding proof (ita_device.h: rq_pack16_v3);
// RELU: fc1, clamp to [0, 127].
// FUSED: the accumulators started at the site's own base and kf is its K (one fma per pair, ita_device.h)
template <bool RELU = false, bool FUSED = false>
__device__ __forceinline__ i32x4 rq_group(const i32x4 (&acc)[4], float mult, bool fast, float kf = 0.0f) {
  if constexpr (ITA_ABLATE & 1) return acc[0] ^ acc[1] ^ acc[2] ^ acc[3];
  if constexpr (RELU && FUSED) return rq_pack16_v3<ITA_RQ_FUSED_RELU>(acc, mult, kf);
  if constexpr (RELU) return rq_pack16_v3<ITA_RQ_RELU>(acc, mult);
  if constexpr (FUSED) return rq_pack16_v3<ITA_RQ_FUSED>(acc, mult, kf);
  if (fast) return rq_pack16_v3<ITA_RQ_FAST>(acc, mult);
  return rq_pack16_v3<ITA_RQ_EXACT>(acc, mult);
}
// block output: d[4t+i] = dequantised int8 code of channel (E/4)kq + 4(et0+t) + i
// FUSED: the accumulators started at the site's own base and kf is its K (ita_device.h: dq16_fused)
template <bool FUSED = false>
__device__ __forceinline__ void dq_group(const i32x4 (&acc)[4], float mult, float scale, float (&d)[16], float kf = 0.0f) {
  if constexpr (ITA_ABLATE & 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = __int_as_float(acc[i >> 2][i & 3]);
    return;
  }
  if constexpr (FUSED) dq16_fused(acc, mult, kf, scale, d);
  else dq16_b(acc, mult, scale, d);
}
// the same, and the codes it scaled: c[4t+i] = d[4t+i] / scale as integers in [-128, 127] (the long taps kernel stores them)
__device__ __forceinline__ void dq_group_codes(const i32x4 (&acc)[4], float mult, float scale, float (&d)[16], float (&c)[16]) {
  dq16_b(acc, mult, scale, d, c);
}

// E = 64 plane stores with the lane exchange: p0 / p1 are the lane's two 16-byte pieces of its 32
// bytes of a plane row; v_permlane16_swap trades p0 of the odd 16-lane rows for p1 of the even ones, after which the first
// store holds bytes [0, 16) of the pair's 64 in the even lane and [16, 32) in the odd one (pa = the lane's own offset, less 16
// in the odd lane), and the second store the next 32 the same way.  Written through, the launch's WRITE_SIZE falls from twice
// the payload to the payload, and the launch is not slower for the 10 more VALU per wave (profiles/encoder_dequant_fused_ab.txt).
__device__ __forceinline__ void plane_store_xchg(__amdgpu_buffer_rsrc_t f, int pa, u32x4 p0, u32x4 p1) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const auto r = __builtin_amdgcn_permlane16_swap(p0[c], p1[c], false, false);
    p0[c] = r[0]; p1[c] = r[1];
  }
  ita_store16<true>(f, pa, p0);
  ita_store16<true>(f, pa + 32, p1);
}
// (amdgpu_waves_per_eu(2, 2): the workgroup owns the CU's LDS, so two waves per SIMD is all there will ever be -- without
// it the scheduler trades instruction-level parallelism for registers it has no use for: the LDS size is dynamic)
// FAST: every requantisation site of this layer passed the load-time single-rounding proof (ita_plugin.hip: fast_site_ok).
// A compile-time switch, two instantiations: as a run-time flag per site the two forms sit side by side in the frame loop
// and the ~40 uniform branches per frame cost more than the shorter form saves (measured: 56.7 us against 56.5 for the
// round-2 form, 54.0 with the fast form compiled in, 55.3 with the exact one).
// FUSED (implies FAST at the out_proj site of the int8 I/O form, the only one it leaves alone): Q, K, V, logits and context
// run the one-fma form on accumulators started at per-site bases, chosen and proven at load time; FUSED == 2: fc1 runs the
// fused ReLU form as well (its own proof); FUSED == 3: out_proj and fc2 run the fused dequantise form on top of that (their
// own proofs, both or neither).  A template argument for the same reason.
template <int E, bool FFN, int TOK, bool STAMP = false, bool IO8 = false, bool FAST = false, int FUSED = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void ita_stream_kernel(const ItaStreamArgs a) {
  static_assert(!IO8 || (!FFN && TOK == 0), "int8 I/O is the attention block's form");
  static_assert(FUSED == 0 || FUSED == 1 || ((FUSED == 2 || FUSED == 3) && FFN), "the fused ReLU and dequantise forms are the whole layer's");
  static_assert(FUSED == 0 || FAST, "the fused instantiation keeps the fast form at out_proj");
  using L = ItaStreamLds<E, FFN, TOK != 0>;
  constexpr int S = 128, P = 192, F = 256, EC = E / 4, NK = E / 64, NTE = E / 16;
  static_assert(!TOK || (E == 64 && FFN), "the fused tokenizer is built for the ITAViTLSTM shape");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keep it (and what derives from it) in SGPRs
  const int qi0 = lane & 15, kq0 = lane >> 4;   // E = 64: the handful of LDS bases derived from these stay hoisted
  const int* bias = (const int*)(lds + L::BIAS);
  const int *l_bq = bias, *l_bk = bias + P, *l_bo = bias + 3 * P, *l_b1 = bias + 3 * P + E,
            *l_b2 = bias + 3 * P + E + F;
  const float* lnp = (const float*)(lds + L::LNP);
  int* colsum = (int*)(lds + L::COLSUM);
  // per-site single-rounding permission (ItaStreamArgs::fast_sites, proven at load time): wave-uniform scalars
  auto site_fast = [&](unsigned bit) {
#ifdef ITA_FORCE_SITES   // counting builds (tools/valu_budget.py): one form per site at compile time
    return ((unsigned)(ITA_FORCE_SITES) & bit) != 0;
#endif
    (void)bit;
    return FAST;
  };
#define fq site_fast(ITA_SITE_Q)
#define fk site_fast(ITA_SITE_K)
#define fv site_fast(ITA_SITE_V)
#define fl site_fast(ITA_SITE_L)
#define fc site_fast(ITA_SITE_C)
#define fo site_fast(ITA_SITE_O)
  // accumulator bases of the two sites whose accumulators do not start from the image's biases (wave-uniform)
  const int base_l = FUSED ? a.c_l : ITA_ACC_BIAS, base_c = FUSED ? a.c_c : ITA_ACC_BIAS;

  // waves 4-7 were dispatched second and lose every VALU arbitration against their SIMD partner (MI355X guide,
  // "Two waves per SIMD", item 4): static priority evens the pair out
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  int fi = 0;
#define ITA_SSTAMP(ph)                                                                                  \
  do {                                                                                                  \
    if (STAMP && a.stamps && (tid & 255) == 0 && fi < 8)                                                      \
      a.stamps[(((size_t)blockIdx.x * 8 + fi) * 2 + (wave >> 2)) * 16 + (ph)] = __builtin_amdgcn_s_memtime(); \
  } while (0)

  // ---- fused tokenizer: the u8 window and conv functions of ita_tokenizer_kernel.h, placed between the phases of the int8
  // blocks by the frame loop: fetch a phase early, fill after B2, blend + the four tiles + LayerNorm after the output stores.
  // Everything per-lane in them is derived from an OPAQUE copy of the lane id taken once per frame (ol), see there.
  unsigned tk_d[5] = {0, 0, 0, 0, 0};
  i32x4 tk_a0, tk_a1;
  float tk_out[16];
  auto tok_fetch = [&](int fb, int ol) { tok_u8_fetch(a.img, fb, wave, ol, tk_d); };
  auto tok_fill = [&](int ol) { tok_u8_fill(lds + L::IMG, wave, ol, tk_d); };
  auto tok_blend = [&](int ol) { tok_u8_blend(lds + L::IMG, (const int*)(lds + L::TAP), wave, ol, tk_a0, tk_a1); };
  // one 16-channel tile of the conv: six int8 MFMAs + the float recombination, placed between the phases of the int8
  // blocks by the caller
  auto tok_step = [&](int ct, int ol) {
    if constexpr (ITA_ABLATE & 1024) { tk_out[4 * ct] = __int_as_float(tk_a0[ct]); return; }
    float o4[4];
    tok_u8_tile<E>(lds + L::CW, ct, ol, ol >> 4, tk_a0, tk_a1, o4);
#pragma unroll
    for (int i = 0; i < 4; ++i) tk_out[4 * ct + i] = o4[i];
  };
  auto tok_finish = [&](int fb, bool store_tap, float (&xr)[EC], int ol) {
    const int qi = ol & 15, kq = ol >> 4, token = wave * 16 + qi;
#pragma unroll
    for (int i = 0; i < 16; ++i) xr[i] = tk_out[i];
    layernorm_q16<E>(xr, lnp + 4 * E, lnp + 5 * E, EC * kq);
    if (a.tok_tap && store_tap) {
      float* o = a.tok_tap + ((size_t)fb * S + token) * E + EC * kq;
#pragma unroll
      for (int i = 0; i < EC; i += 4) *(f32x4*)(o + i) = (f32x4){xr[i], xr[i + 1], xr[i + 2], xr[i + 3]};
    }
  };

  // diagnostic: s_memrealtime (100 MHz, one clock for the whole chip) at kernel entry [12], prologue end [13], exit [14]
  if (STAMP && a.stamps && (tid & 255) == 0)
    a.stamps[(((size_t)blockIdx.x * 8) * 2 + (wave >> 2)) * 16 + 12] = __builtin_amdgcn_s_memrealtime();
  // ---- once per workgroup.  Order matters (it is 10+ % of a 4-frame launch): with the fused tokenizer the first frame's
  // pixels are requested after the image (see below).
  float xr[EC];
  i32x4 xq_cur[NK];       // IO8: this lane's k-slots of the block input, as they stand in memory
  f32x4 h0_cur = {0.0f, 0.0f, 0.0f, 0.0f};
  int h0_row_next = 0;
  {
    int ol = lane;
    asm volatile("" : "+v"(ol));
    if constexpr (IO8) {
      const int8_t* xrow = a.xq + ((size_t)blockIdx.x * S + wave * 16 + (ol & 15)) * E + EC * (ol >> 4);
#pragma unroll
      for (int c = 0; c < NK; ++c) xq_cur[c] = *(const i32x4*)(xrow + 16 * c);
    } else if constexpr (TOK == 0) {
      ld_tok_items<E>(a.x + ((size_t)blockIdx.x * S + wave * 16 + (ol & 15)) * E, ol >> 4, xr);   // transposed where it is first used
    }
    if (a.h0_dst && tid < 32) {
      const size_t row = a.slots ? (size_t)a.slots[blockIdx.x] : (size_t)blockIdx.x;
      h0_cur = *(const f32x4*)(a.h0_src + row * 128 + 4 * tid);
    }
    constexpr int T0 = L::LNP / 16, NT = (L::IMAGE - L::LNP) / 16, NTJ = (NT + 511) / 512;   // tables: LayerNorm, conv, taps
    constexpr int NW = L::LNP / 16, NWJ = (NW + 511) / 512;                                     // weights + biases
    static_assert(L::LNP % 16 == 0, "");
    i32x4 vt[NTJ], vw[NWJ];
#pragma unroll
    for (int j = 0; j < NTJ; ++j) {
      const int p = tid + 512 * j;
      vt[j] = (i32x4){0, 0, 0, 0};
      if (p < NT) vt[j] = *(const i32x4*)(a.image + (size_t)(T0 + p) * 16);
    }
#pragma unroll
    for (int j = 0; j < NWJ; ++j) {
      const int p = tid + 512 * j;
      vw[j] = (i32x4){0, 0, 0, 0};
      if (p < NW) vw[j] = *(const i32x4*)(a.image + (size_t)p * 16);
    }
    // Loads return in order.  The image (tables, weights) is L2-resident after the first workgroups, the first frame's pixels come
    // from HBM: requested LAST, the 100 KB of the image reach LDS while the pixels are still on their way, and the tokenizer of the
    // first frame is the only thing left between their arrival and the frame loop (pixels first, with the weights parked in
    // registers until the tokenizer was done, put the weights' LDS stores behind it)
    if constexpr (TOK != 0) tok_fetch(blockIdx.x, ol);
    if (tid < 2 * P) colsum[tid] = base_c;
#pragma unroll
    for (int j = 0; j < NTJ; ++j) {
      const int p = tid + 512 * j;
      if (p < NT) *(i32x4*)(lds + (T0 + p) * 16) = vt[j];
    }
#pragma unroll
    for (int j = 0; j < NWJ; ++j) {
      const int p = tid + 512 * j;
      if (p < NW) *(i32x4*)(lds + p * 16) = vw[j];
    }
    if constexpr (TOK != 0) tok_fill(ol);
    lds_barrier();   // tables, weights, biases and column-sum bases in place
    if constexpr (TOK != 0) {
      tok_blend(ol);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) tok_step(ct, ol);
      tok_finish(blockIdx.x, true, xr, ol);
    }
    if constexpr (TOK == 0 && !IO8) tok_items_transpose<E>(xr);   // the first frame's rows were fetched as items (ld_tok_items)
  }
  if (STAMP && a.stamps && (tid & 255) == 0)
    a.stamps[(((size_t)blockIdx.x * 8) * 2 + (wave >> 2)) * 16 + 13] = __builtin_amdgcn_s_memrealtime();

  for (int b = blockIdx.x; b < a.B; b += gridDim.x, ++fi) {
    int ol = lane;
    asm volatile("" : "+v"(ol));   // see the tokenizer above: its per-lane values are re-derived each frame
    // E = 128 holds twice the activations in registers: there the LDS bases are re-derived per frame as well
    const int qi = E > 64 ? (ol & 15) : qi0, kq = E > 64 ? (ol >> 4) : kq0, token = wave * 16 + qi;
    const int nb = b + gridDim.x;
    const bool more = nb < a.B;   // (uniform) the next frame exists: its tokenizer pieces run between this frame's phases
    int* cs = colsum + (fi & 1) * P;
    ITA_SSTAMP(0);
    // ---------------- quantise: this lane's E/4 channels are its k-slots of the B fragment(s)
    i32x4 xf[NK];
#pragma unroll
    for (int c = 0; c < NK; ++c) {
      if constexpr (IO8) {
        xf[c] = xq_cur[c];
      } else {
        unsigned p4[4];
        q_pack16(&xr[16 * c], a.inv_sx, p4);
        xf[c] = (i32x4){(int)p4[0], (int)p4[1], (int)p4[2], (int)p4[3]};
      }
    }
    // side copy of the LSTM layer-0 state row (see ItaStreamArgs): the row was requested a phase ago -- a load waited
    // for here would hold wave 0, and with it the whole workgroup's next barrier, for a full memory latency
    if (!(ITA_ABLATE & 128) && a.h0_dst && tid < 32) {
      *(f32x4*)(a.h0_dst + (size_t)b * 128 + 4 * ol) = h0_cur;   // (tid < 32: tid == ol; the opaque copy keeps the address out of the loop-invariant set)
      if (nb < a.B) h0_row_next = a.slots ? a.slots[nb] : nb;
    }

    // ---------------- projections, nine groups: Q0-2 (stay in registers), K0-2 and V0-2 (this wave's 16 rows of the
    // K image / 16 columns of the V^T image)
    i32x4 qf[3];
    {
      ItaFr<4 * NK> fr[2];
      i32x4 ac[3][4];
      auto load = [&](int g, ItaFr<4 * NK>& f, i32x4 (&acc)[4]) {
        const int mat = g / 3, t0 = 4 * (g - 3 * mat);
        if (mat == 0) ld_nat<NK, P>(f, acc, lds + L::WQ, l_bq, t0, qi, kq);
        else if (mat == 1) ld_nat<NK, P>(f, acc, lds + L::WK, l_bk, t0, qi, kq);
        else ld_natv<NK, P>(f, acc, lds + L::WV, (const int*)(lds + L::VB4), t0, qi, kq);
      };
      auto epilogue = [&](int g, const i32x4 (&acc)[4]) {
        const int mat = g / 3, gg = g - 3 * mat;
        if (mat == 0) {
          qf[gg] = rq_group<false, FUSED != 0>(acc, FUSED ? a.mkq.x : a.mq, fq, a.mkq.y);
        } else if (mat == 1) {
          *(i32x4*)(lds + L::K + (((4 * gg + kq) * S + token) << 4)) = rq_group<false, FUSED != 0>(acc, FUSED ? a.mkk.x : a.mk, fk, a.mkk.y);
        } else {
          // V with the roles swapped (A = tokens, B = weights): lane (feature qi, kq) holds keys 16w + 4kq + i of
          // feature 16 dt + qi -- one dword of the V^T slot (key block w>>2, k-group kq), at word w&3
          const i32x4 p4 = rq_group<false, FUSED != 0>(acc, FUSED ? a.mkv.x : a.mv, fv, a.mkv.y);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int d = (4 * gg + t) * 16 + qi;
            *(int*)(lds + L::VT + (((((wave >> 2) * 4 + kq) * P) + d) << 4) + 4 * (wave & 3)) = p4[t];
            // column sum of the requantised codes for the unsigned-probability offset, kept pre-multiplied by 128
            atomicAdd(&cs[d], __builtin_amdgcn_sdot4(p4[t], 0x01010101, 0, false) << 7);
          }
        }
      };
      // (three accumulator sets: group g+1's start from its bias while g computes and g-1 is requantised)
      load(0, fr[0], ac[0]);
#pragma unroll
      for (int g = 0; g < 9; ++g) {
        if (g + 1 < 9) load(g + 1, fr[(g + 1) & 1], ac[(g + 1) % 3]);
        if (g < 6) mm_group<NK, false>(fr[g & 1], xf, ac[g % 3]);
        else mm_group<NK, true>(fr[g & 1], xf, ac[g % 3]);
        if (g > 0) epilogue(g - 1, ac[(g - 1) % 3]);
        ITA_SCHED_BARRIER();   // keep the step's loads ahead of the next step's MFMAs
      }
      epilogue(8, ac[8 % 3]);
    }
    ITA_SSTAMP(1);
    if constexpr (!(ITA_ABLATE & 64)) lds_barrier();   // B1: K, V^T and the column sums of this frame are complete
    ITA_SSTAMP(2);

    // next frame's input: issued now, consumed after the attention phase
    if (!(ITA_ABLATE & 128) && a.h0_dst && tid < 32 && nb < a.B)
      h0_cur = *(const f32x4*)(a.h0_src + (size_t)h0_row_next * 128 + 4 * ol);
    float xn[EC];
    i32x4 xq_nxt[NK];
    if constexpr (TOK != 0) {
      if (nb < a.B) tok_fetch(nb, ol);
    } else if constexpr (IO8) {
      const int8_t* xnrow = a.xq + ((size_t)min(nb, a.B - 1) * S + token) * E + EC * kq;
#pragma unroll
      for (int c = 0; c < NK; ++c) xq_nxt[c] = *(const i32x4*)(xnrow + 16 * c);
    } else {
      ld_tok_items<E>(a.x + ((size_t)min(nb, a.B - 1) * S + token) * E, kq, xn);   // items; transposed at the end of the frame
    }

    // ---------------- attention for this wave's 16 queries: logits and probabilities stay in registers
    i32x4 cf[3];
    constexpr int EG = NTE / 4;   // groups of four output tiles of a block output projection
    ItaF4 ob[2];
    i32x4 oa[4];
    {
      // logits as packed signed 16-bit pairs: the integer softmax then runs on v_pk_*_16, two keys per
      // VALU op.  w[2kt + j] = {logit 4kt+2j, logit 4kt+2j+1} of keys 16kt + 4kq + ...
      typedef ita_u16x2 u16x2;
      u16x2 w[16];
      struct KFr { i32x4 w[6]; } kfr[2];   // two key tiles x three k-steps
      ItaF4 vb[2];
      i32x4 va[3][4];
      auto ldk = [&](int p, KFr& f) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int ks = 0; ks < 3; ++ks) f.w[t * 3 + ks] = sfrag(lds + L::K, ((4 * ks + kq) * S + (2 * p + t) * 16 + qi) << 4);
      };
      // A.V step st = (feature group dg = st >> 1, key block kb = st & 1): four V^T fragments; the accumulators of a
      // feature group start from 128 * column sum
      auto ldv = [&](int st, ItaF4& f) {
        const int dg = st >> 1, kb = st & 1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          f.w[t] = sfrag(lds + L::VT, (((kb * 4 + kq) * P) + (4 * dg + t) * 16 + qi) << 4);
          if (kb == 0) va[dg][t] = *(const i32x4*)(cs + (4 * dg + t) * 16 + 4 * kq);
        }
      };
      i32x4 la[2][2];
      auto mmk = [&](const KFr& f, i32x4 (&acc)[2]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          acc[t] = (i32x4){base_l, base_l, base_l, base_l};
#pragma unroll
          for (int ks = 0; ks < 3; ++ks) acc[t] = mfma16(f.w[t * 3 + ks], qf[ks], acc[t]);
        }
      };
      auto epil = [&](int p, const i32x4 (&acc)[2]) {
        // low 16 bits = rne(logit) + 32768, unclamped: the softmax clamps (ita_softmax_packed16)
        unsigned w4[4];
        if constexpr (FUSED) lg8_v3<ITA_RQ_FUSED>(acc, a.mkl.x, w4, a.mkl.y);
        else if (fl) lg8_v3<ITA_RQ_FAST>(acc, a.ml, w4);
        else lg8_v3<ITA_RQ_EXACT>(acc, a.ml, w4);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int j = 0; j < 2; ++j) w[2 * (2 * p + t) + j] = __builtin_bit_cast(u16x2, w4[2 * t + j]);
      };
      ldk(0, kfr[0]);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p + 1 < 4) ldk(p + 1, kfr[(p + 1) & 1]);
        else ldv(0, vb[0]);
        mmk(kfr[p & 1], la[p & 1]);
        if (p > 0) epil(p - 1, la[(p - 1) & 1]);
        ITA_SCHED_BARRIER();   // keep the step's loads ahead of the next step's MFMAs
      }
      epil(3, la[1]);
      ITA_SSTAMP(3);
      i32x4 pf[2];
      if constexpr (ITA_ABLATE & 32) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int t = 0; t < 4; ++t) pf[kb][t] = __builtin_bit_cast(int, w[2 * (4 * kb + t)]);
      } else {
        ita_softmax_packed16(w, pf);
      }
      ITA_SSTAMP(4);
      // A.V with uint8 probabilities on a signed MFMA: (p - 128) * v summed + 128 * colsum(v)
#pragma unroll
      for (int st = 0; st < 6; ++st) {
        if (st + 1 < 6) ldv(st + 1, vb[(st + 1) & 1]);
        mm_ks(vb[st & 1], pf[st & 1], va[st >> 1]);
        if (st == 3) cf[0] = rq_group<false, FUSED != 0>(va[0], FUSED ? a.mkc.x : a.mc, fc, a.mkc.y);
        ITA_SCHED_BARRIER();   // keep the step's loads ahead of the next step's MFMAs
      }
      ITA_SSTAMP(5);
      if constexpr (!(ITA_ABLATE & 64)) lds_barrier();   // B2: every wave is done with K, V^T and this frame's column sums
      ITA_SSTAMP(6);
      if (tid < P) cs[tid] = base_c;   // this parity is next accumulated after the NEXT frame's B2
      ld_frg_ks<E>(ob[0], lds + L::WO, 0, 0, qi, kq);
      ld_obias<E>(oa, l_bo, 0, kq);
      // the next frame's pixel window, before this frame's global stores (one in-order vmcnt for loads and stores)
      if constexpr (TOK != 0) { if (more) tok_fill(ol); }
      cf[1] = rq_group<false, FUSED != 0>(va[1], FUSED ? a.mkc.x : a.mc, fc, a.mkc.y);
      ld_frg_ks<E>(ob[1], lds + L::WO, 0, 1, qi, kq);
      mm_ks(ob[0], cf[0], oa);
      cf[2] = rq_group<false, FUSED != 0>(va[2], FUSED ? a.mkc.x : a.mc, fc, a.mkc.y);
    }

    // ---------------- out_proj + residual + LayerNorm1 (k-step 0 of the first group is already in flight)
    const char* w1p = lds + L::W1;   // fc1 / fc2 weights: LDS image, or (E = 128) the global image behind it
    const char* w2p = lds + L::W2;
    if constexpr (L::W12G) { w1p = a.image + L::GW1; w2p = a.image + L::GW2; }
    float x1[EC];
    ItaFr<4 * NK> ffr[2];
    i32x4 fa[3][4];
#pragma unroll
    for (int eg = 0; eg < EG; ++eg) {
      // k-steps 3 eg + ks; fragments are fetched one k-step ahead
#pragma unroll
      for (int ks = (eg == 0 ? 1 : 0); ks < 3; ++ks) {
        const int cur = (3 * eg + ks) & 1;
        if (ks + 1 < 3) ld_frg_ks<E>(ob[cur ^ 1], lds + L::WO, 4 * eg, ks + 1, qi, kq);
        else if (eg + 1 < EG) ld_frg_ks<E>(ob[cur ^ 1], lds + L::WO, 4 * (eg + 1), 0, qi, kq);
        else if constexpr (FFN) ld_nat<NK, F>(ffr[0], fa[0], w1p, l_b1, 0, qi, kq);
        mm_ks(ob[cur], cf[ks], oa);
        ITA_SCHED_BARRIER();   // keep the step's loads ahead of the next step's MFMAs
      }
      if constexpr (IO8) {   // the int8 codes themselves: 16 channels of this lane's token, one 16-byte store
        *(i32x4*)(a.yq + ((size_t)b * S + token) * E + EC * kq + 16 * eg) = rq_group(oa, a.mo, fo);
        if (eg + 1 < EG) ld_obias<E>(oa, l_bo, 4 * (eg + 1), kq);
        continue;
      }
      float d[16];
      dq_group<FUSED == 3>(oa, FUSED == 3 ? a.mko.x : a.mo, a.so, d, a.mko.y);
      if (eg + 1 < EG) ld_obias<E>(oa, l_bo, 4 * (eg + 1), kq);
#pragma unroll
      for (int j = 0; j < 16; ++j) x1[16 * eg + j] = (FFN || a.fuse_ln) ? xr[16 * eg + j] + d[j] : d[j];
    }
    if constexpr (IO8) {
#pragma unroll
      for (int c = 0; c < NK; ++c) xq_cur[c] = xq_nxt[c];
      continue;
    }
    if (FFN || a.fuse_ln) layernorm_q16<E>(x1, lnp, lnp + E, EC * kq);
    if (a.x1_tap) {
      float* o = a.x1_tap + ((size_t)b * S + token) * E + EC * kq;
#pragma unroll
      for (int i = 0; i < EC; i += 4) *(f32x4*)(o + i) = (f32x4){x1[i], x1[i + 1], x1[i + 2], x1[i + 3]};
    }
    ITA_SSTAMP(7);

    float yv[EC];
    if constexpr (FFN) {
      // ---------------- FFN: fc1 + ReLU (hidden layer = four B fragments in registers) -> fc2 -> LayerNorm2.
      // fc2's k-step ks consumes hidden fragment ks: its MFMAs are issued one step behind fc1's epilogue.
      i32x4 x1f[NK];
#pragma unroll
      for (int c = 0; c < NK; ++c) {
        unsigned p4[4];
        q_pack16(&x1[16 * c], a.f_inv_sx, p4);
        x1f[c] = (i32x4){(int)p4[0], (int)p4[1], (int)p4[2], (int)p4[3]};
      }
      i32x4 hf[4], ya[4];
      ItaF4 wb[2];
      ld_obias<E>(ya, l_b2, 0, kq);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (g + 1 < 4) ld_nat<NK, F>(ffr[(g + 1) & 1], fa[(g + 1) % 3], w1p, l_b1, 4 * (g + 1), qi, kq);
        if (g >= 1) ld_frg_ks<E>(wb[(g - 1) & 1], w2p, 0, g - 1, qi, kq);
        mm_group<NK, false>(ffr[g & 1], x1f, fa[g % 3]);
        if (g >= 2) mm_ks(wb[(g - 2) & 1], hf[g - 2], ya);
        if (g >= 1) hf[g - 1] = rq_group<true, FUSED >= 2>(fa[(g - 1) % 3], FUSED >= 2 ? a.mk1.x : a.m1, false, a.mk1.y);
        ITA_SCHED_BARRIER();   // keep the step's loads ahead of the next step's MFMAs
      }
      ld_frg_ks<E>(wb[1], w2p, 0, 3, qi, kq);
      mm_ks(wb[0], hf[2], ya);
      hf[3] = rq_group<true, FUSED >= 2>(fa[3 % 3], FUSED >= 2 ? a.mk1.x : a.m1, false, a.mk1.y);
      mm_ks(wb[1], hf[3], ya);
      ITA_SSTAMP(8);
      {
        float d[16];
        dq_group<FUSED == 3>(ya, FUSED == 3 ? a.mk2.x : a.m2, a.s2, d, a.mk2.y);
#pragma unroll
        for (int j = 0; j < 16; ++j) yv[j] = x1[j] + d[j];
      }
      // E = 128: the second half of the output channels, from the same hidden fragments
#pragma unroll
      for (int eg = 1; eg < EG; ++eg) {
        ld_obias<E>(ya, l_b2, 4 * eg, kq);
        ld_frg_ks<E>(wb[0], w2p, 4 * eg, 0, qi, kq);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          if (ks + 1 < 4) ld_frg_ks<E>(wb[(ks + 1) & 1], w2p, 4 * eg, ks + 1, qi, kq);
          mm_ks(wb[ks & 1], hf[ks], ya);
          ITA_SCHED_BARRIER();
        }
        float d[16];
        dq_group<FUSED == 3>(ya, FUSED == 3 ? a.mk2.x : a.m2, a.s2, d, a.mk2.y);
#pragma unroll
        for (int j = 0; j < 16; ++j) yv[16 * eg + j] = x1[16 * eg + j] + d[j];
      }
      layernorm_q16<E>(yv, lnp + 2 * E, lnp + 3 * E, EC * kq);
    } else {
#pragma unroll
      for (int i = 0; i < EC; ++i) yv[i] = x1[i];
    }
    {
      // Both outputs are read by the next launch, from other XCDs: write-through stores (ita_device.h) on a resource per
      // frame, so the byte offsets stay below 32 KB (f32 rows: 64 KB) at any batch size.  The planes of E = 128 stay plain:
      // a lane's 64 bytes of a row leave as four stores 64 bytes apart, quarter lines that cost that launch +8 us written
      // through (E = 64: half lines, -0.9 us; DESIGN.md section 4, profiles/handover_ab.txt)
      constexpr bool PLANES_WT = E == 64;
      float* y_f32 = a.y;
      _Float16* y_hi = a.y_hi;
      // (opaque copies: the two null tests are then scalar compares here, per frame, instead of two lane masks held in SGPR pairs
      // across the frame loop -- the four SGPRs the resource needs; without them E = 64 with the tokenizer spills two SGPRs)
      asm volatile("" : "+s"(y_f32), "+s"(y_hi));
      if (y_f32) st_tok_quarter_next<E>(ita_rsrc(y_f32 + (size_t)b * S * E), token, kq, yv);
      if (!(ITA_ABLATE & 128) && y_hi) {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        h8 vh[EC / 8], vl[EC / 8];
#pragma unroll
        for (int i = 0; i < EC; ++i) {
          const _Float16 hh = (_Float16)yv[i];
          vh[i >> 3][i & 7] = hh;
          vl[i >> 3][i & 7] = (_Float16)(yv[i] - (float)hh);
        }
        const int po = token * E + EC * kq;   // halves from the frame's row on
        if constexpr (ITA_ABLATE & 256) {   // values stay live, one 2-byte store instead of two 16-byte ones
#pragma unroll
          for (int i = 0; i < EC / 8; ++i)
            a.y_hi[(size_t)b * a.ld_planes + po + 8 * i] = vh[i][0] + vh[i][1] + vh[i][2] + vh[i][3] + vh[i][4] + vh[i][5] + vh[i][6] + vh[i][7] + vl[i][0] + vl[i][1] + vl[i][2] + vl[i][3] + vl[i][4] + vl[i][5] + vl[i][6] + vl[i][7];
        } else {
          // one plane after the other: one resource (four SGPRs) live at a time
          const __amdgpu_buffer_rsrc_t f_hi = ita_rsrc(y_hi + (size_t)b * a.ld_planes);
          if constexpr (PLANES_WT) {
            // lanes kq and kq ^ 1 (16 apart) exchange a 16-byte piece, the even one's second against the odd one's first: a
            // store instruction then covers 32 contiguous bytes per lane pair, two runs per token row instead of four
            const int pa = po * 2 - 16 * (kq & 1);
            plane_store_xchg(f_hi, pa, __builtin_bit_cast(u32x4, vh[0]), __builtin_bit_cast(u32x4, vh[1]));
            const __amdgpu_buffer_rsrc_t f_lo = ita_rsrc(a.y_lo + (size_t)b * a.ld_planes);
            plane_store_xchg(f_lo, pa, __builtin_bit_cast(u32x4, vl[0]), __builtin_bit_cast(u32x4, vl[1]));
          } else {
#pragma unroll
            for (int i = 0; i < EC / 8; ++i) ita_store16<PLANES_WT>(f_hi, (po + 8 * i) * 2, __builtin_bit_cast(u32x4, vh[i]));
            const __amdgpu_buffer_rsrc_t f_lo = ita_rsrc(a.y_lo + (size_t)b * a.ld_planes);
#pragma unroll
            for (int i = 0; i < EC / 8; ++i) ita_store16<PLANES_WT>(f_lo, (po + 8 * i) * 2, __builtin_bit_cast(u32x4, vl[i]));
          }
        }
      }
    }
    ITA_SSTAMP(11);
    // ---------------- the next frame's tokens: blend and the four conv tiles (each: six int8 MFMAs + 24 VALU + 8 LDS reads) here,
    // after LayerNorm2 and the output stores, where the kernel has registers to spare -- nothing of the tokenizer is live across
    // the FFN (246 VGPRs).  Measured on one box, encoder launch of 1024 frames: round-2 kernel 58.4 us, this placement 52.1; the
    // blend after B2 52.5, the four tiles right after the blend in front of out_proj 52.9, the tiles spread over the out_proj /
    // fc1 steps +1.5 (~20 more live registers at the kernel's tightest point: 7 spilled).  Those placements were removed.
    if constexpr (TOK != 0 && !(ITA_ABLATE & 4)) {
      if (more) {
        tok_blend(ol);   // (the window written after B2 is still in LDS: private to this wave)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) tok_step(ct, ol);
        tok_finish(nb, true, xr, ol);
      }
    } else {
      tok_items_transpose<E>(xn);
#pragma unroll
      for (int i = 0; i < EC; ++i) xr[i] = xn[i];
    }
  }
  if (STAMP && a.stamps && (tid & 255) == 0)
    a.stamps[(((size_t)blockIdx.x * 8) * 2 + (wave >> 2)) * 16 + 14] = __builtin_amdgcn_s_memrealtime();
#undef ITA_SSTAMP
#undef fq
#undef fk
#undef fv
#undef fl
#undef fc
#undef fo
}
