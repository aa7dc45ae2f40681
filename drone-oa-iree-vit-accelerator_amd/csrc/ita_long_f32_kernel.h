// ita_long_f32_kernel.h -- ITASelfAttention (float32, true softmax) on LONG token sequences: S a multiple of 128, E = 64 or
// 128, P = 192, one head.  The long form of ita_attn_f32_kernel.h, as ita_long_attn_kernel.h is the long form of the int8
// stream kernel:
//     y = attn(x) = out_proj(softmax(Q K^T) V),  or with fuse_ln  y = LayerNorm1(x + attn(x)),   Q / K / V = x W^T + b
//
// A row of S logits cannot stay in registers, but exp-softmax is associative (the integer softmax of the int8 path is
// not): ONE sweep over the key tiles with a running row maximum m and a running row sum l.  Per 64-key unit and query:
//     s = K q;   m' = max(m, max s);   l = l e^(m - m') + sum e^(s - m');   ctx = ctx e^(m - m') + sum e^(s - m') v;   m = m'
// and after the last unit ctx / l.  m starts at -inf and the first unit's e^(-inf - m') is ita_expf's clamp e^-87 times the
// zero l and ctx: exact zeros, and e^(-inf - (-inf)) is never formed because m' is a finite logit.  No 1 / sqrt(d): the
// reference has none, |logit| reaches the hundreds, and nothing but the subtraction of m' keeps e^s inside f32.
//
// Numerics as in ita_attn_f32_kernel.h: v_mfma_f32_16x16x4_f32 (an exact fmaf chain per output), projection accumulators
// seeded with the bias, ita_expf -- except that Q, K, V and the logits are BLOCK sums: the 16 products of one k group
// (four MFMAs) are chained from zero and the block is then added to the running total, as a blocked GEMM sums.  One chain
// of 128 or 192 roundings at the magnitude of the growing sum leaves q, k and a logit of magnitude 100 .. 400 several ulp
// off, and exp turns that into the whole output error where two keys nearly tie; the block form's roundings are mostly at
// the magnitude of a block.  Against float64 on the dominant-key inputs of tests/test_gpu_long_f32.py, as a multiple of
// the error of torch's CPU f32 attention: one chain 0.72 .. 3.22 (mean 1.4), block sums 0.20 .. 1.87 (mean 0.6), both
// measured on the GPU and reproduced by a CPU emulation of the chains; a correctly rounded q, k and logit 0.02 .. 0.28.  The GEMM chain is that kernel's, every accumulator the next
// GEMM's operand fragment:
//   Q^T = Wq x^T      D lane (token, slot) holds Q[token][16 ft + 4 slot + r]     -> B operand of S^T, in registers
//   K^T = Wk x^T      same layout                                                  -> A operand of S^T, image in the workspace
//   S^T = K Q^T       D lane (query, slot) holds S[query][16 kt + 4 slot + r]     -> running softmax, then B operand of ctx^T
//   V   = x Wv^T      D lane (feature, slot) holds V[16 kt + 4 slot + r][feature] -> A operand of ctx^T, image in the workspace
//   ctx^T = V^T P^T   D lane (query, slot) holds ctx[query][16 ft + 4 slot + r]   -> B operand of out^T, in registers
//   out^T = Wo ctx^T  D lane (query, slot) holds out[query][16 et + 4 slot + r]   -> + x, rows through LDS, LayerNorm1
//
//   ita_lf32_proj_kernel<E> : persistent, one 128-token tile at a time, no LDS: wave w projects its 16 tokens to K and V
//                             and stores the accumulators as they are, 1 KB per wave and feature tile -- the f32x4
//                             fragment images of the S = 128 kernel, cut into 64-key units [12 ft][4 kt][64 lanes]
//                             (48 KB) so that a unit is one contiguous piece for the attention kernel's LDS-DMA
//   ita_lf32_attn_kernel<E> : one workgroup per (query tile, frame), 8 waves, wave w owns 16 queries.  Q for the
//                             workgroup's own tile is computed in the prologue (128 x E x 192 MAC against the 2 x 128 x
//                             S x 192 of the sweeps; the workspace holds K and V only).  K units arrive by LDS-DMA into
//                             a two-slot ring, V units into one slot, requested at the top of a step and waited for
//                             behind that step's S^T and softmax: two barriers per unit, as sweep 3 of the int8 kernel.
//
// LDS: 3 x 48 KB = 144 KB, one workgroup per CU.  Two per CU would need 128 registers per lane, and Q (48), the context
// accumulators (48), a unit's logits (16) and two block sums (32) are more than that: the kernel runs at two
// waves per SIMD, where one wave's softmax VALU work runs beside the other's MFMAs.
// Aliasing: y may be x.  The projection launch reads all of x and writes the workspace only; in the attention launch a wave
// reads nothing of x but its own 16 rows (its Q in the prologue, its residual), each before it stores them.
//
// Roofline: 2 x 2 x B x S^2 x 192 flop for the two sweeps' GEMMs: 32 x 8192 -> 1.65 TFLOP, >= 10.5 ms at 157.3 TF.
//
// Taps (ita_mha_long_f32_taps): both kernel bodies are function templates with a TAPS switch, as in ita_long_attn_kernel.h;
// the production kernels are the bodies with TAPS = false, ita_lf32_proj_taps_kernel / ita_lf32_attn_taps_kernel those with
// TAPS = true.  Under `if constexpr (TAPS)` there are stores only, of the registers the launches compute with: K and V (the
// projection's accumulators), Q (the prologue's), ctx (after the multiplication by 1 / l), and for the query rows the row
// table (S int32: output index or -1) selects the sweep's logits s at their natural key index, the final running maximum
// m and the final row sum l.  The sweep never holds a probability e^(s - m_final) / l: ita_lf32_probs_kernel forms
// ita_expf(logit - row_max) * (1.0f / row_sum) from those three stored values behind the attention launch.
#pragma once
#include "ita_attn_f32_kernel.h"

struct ItaLongF32Args {
  const float* x;                 // (B, S, E) f32 tokens
  float* y;                       // (B, S, E) f32: fuse_ln ? LayerNorm1(x + attn(x)) : attn(x); may alias x
  const float *wq, *wk, *wv;      // [P][E] (nn.Linear [out][in])
  const float *bq, *bk, *bv;      // [P]
  const float *wo, *bo;           // [E][P], [E]
  const float *ln_w, *ln_b;       // LayerNorm1 affine
  f32x4* kimg;                    // workspace (B, S/64) units [12][4][64] f32x4: K^T fragments
  f32x4* vimg;                    // workspace (B, S/64) units [12][4][64] f32x4: V fragments
  int B, S;
  int fuse_ln;
};

// what the taps kernels store besides (any pointer may be null; plain vector stores)
struct ItaLongF32TapArgs {
  float *K, *V;               // projection launch: (B, S, P), natural [token][feature]
  float *Q, *ctx;             // attention launch: (B, S, P)
  const int* rowidx;          // S entries, the same for every frame: output index of a chosen query row, or -1; null: no rows
  int n_rows;
  float* logits;              // (B, n_rows, S): the sweep's s, before it becomes e^(s - m)
  float *row_max, *row_sum;   // (B, n_rows): the final m, the final l after the cross-lane add
};

struct ItaLongF32Lds {
  static constexpr int NFT = 12, NKT = 4;                  // feature tiles, 16-key tiles of a 64-key unit
  static constexpr int UNIT_F4 = NFT * NKT * 64;           // f32x4 per unit
  static constexpr int UNIT = UNIT_F4 * 16;                // 49152 bytes
  static constexpr int K = 0, V = 2 * UNIT;                // K: two-slot ring; V: one slot
  static constexpr int TOTAL = 3 * UNIT;                   // 147456 bytes
  // after the last unit the x + out rows [128][E + 4] overlay the K ring (every wave is behind the last step's second
  // barrier when the first row is written, and the K ring is read before that barrier only)
  static_assert(128 * (128 + 4) * 4 <= 2 * UNIT, "the x + out rows overlay the K ring");
};

template <int E, bool TAPS>
__device__ __forceinline__ void ita_lf32_proj_body(const ItaLongF32Args& a, const ItaLongF32TapArgs& tp) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel k groups");
  using L = ItaLongF32Lds;
  constexpr int S = 128, NFT = L::NFT, NG = E / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;
  const int ntile = a.B * (a.S / 128);
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    // x fragments of the wave's tokens: lane (token col, slot), group g holds x[16 wave + col][16 g + 4 slot + 0..3]
    const float* xsrc = a.x + ((size_t)tile * S + 16 * wave + col) * E + 4 * slot;
    f32x4 xf[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) xf[g] = *(const f32x4*)(xsrc + 16 * g);
    // the wave's 16 tokens are key tile wave & 3 of unit 2 tile + wave / 4
    const size_t dst = ((size_t)(2 * tile + (wave >> 2)) * NFT * L::NKT + (wave & 3)) * 64 + lane;
    f32x4 *kd = a.kimg + dst, *vd = a.vimg + dst;

    // K^T: rows = features 16 ft + 4 slot + r, column = token col
#pragma unroll
    for (int ft = 0; ft < NFT; ft += 2) {
      f32x4 ka[2];
      const float* wkr[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        ka[u] = *(const f32x4*)(a.bk + 16 * (ft + u) + 4 * slot);
        wkr[u] = a.wk + ita_opaque((16 * (ft + u) + col) * E + 4 * slot);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 w0 = *(const f32x4*)(wkr[0] + 16 * g), w1 = *(const f32x4*)(wkr[1] + 16 * g);
        f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};   // block sum (header): 16 products from zero, then onto the total
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[r], xf[g][r], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[r], xf[g][r], t1, 0, 0, 0);
        }
        ka[0] += t0;
        ka[1] += t1;
      }
      kd[ft * L::NKT * 64] = ka[0];
      kd[(ft + 1) * L::NKT * 64] = ka[1];
      if constexpr (TAPS) {   // the same accumulators at K[token 16 wave + col][16 ft + 4 slot + 0..3]
        if (tp.K) {
          float* kr = tp.K + ((size_t)tile * S + 16 * wave + col) * 192 + 4 * slot;
          *(f32x4*)(kr + 16 * ft) = ka[0];
          *(f32x4*)(kr + 16 * (ft + 1)) = ka[1];
        }
      }
    }
    // V: lane (feature 16 ft + col, slot) holds V[16 wave + 4 slot + r][feature]
#pragma unroll
    for (int ft = 0; ft < NFT; ft += 2) {
      f32x4 va[2];
      const float* wvr[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float bv = a.bv[16 * (ft + u) + col];
        va[u] = (f32x4){bv, bv, bv, bv};
        wvr[u] = a.wv + ita_opaque((16 * (ft + u) + col) * E + 4 * slot);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 w0 = *(const f32x4*)(wvr[0] + 16 * g), w1 = *(const f32x4*)(wvr[1] + 16 * g);
        f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xf[g][r], w0[r], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xf[g][r], w1[r], t1, 0, 0, 0);
        }
        va[0] += t0;
        va[1] += t1;
      }
      vd[ft * L::NKT * 64] = va[0];
      vd[(ft + 1) * L::NKT * 64] = va[1];
      if constexpr (TAPS) {   // element r is token 16 wave + 4 slot + r of feature 16 ft + col
        if (tp.V) {
          float* vr = tp.V + ((size_t)tile * S + 16 * wave + 4 * slot) * 192 + col;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            vr[r * 192 + 16 * ft] = va[0][r];
            vr[r * 192 + 16 * (ft + 1)] = va[1][r];
          }
        }
      }
    }
  }
}
template <int E>
__global__ __launch_bounds__(512) void ita_lf32_proj_kernel(const ItaLongF32Args a) {
  ita_lf32_proj_body<E, false>(a, ItaLongF32TapArgs{});
}
template <int E>
__global__ __launch_bounds__(512) void ita_lf32_proj_taps_kernel(const ItaLongF32Args a, const ItaLongF32TapArgs tp) {
  ita_lf32_proj_body<E, true>(a, tp);
}

// What ita_lf32_attn_body and ita_lf32_stats_kernel (ita_long_f32_stats_kernel.h) share.  The statistics' row_max and
// row_sum are the production bits because both kernels run these functions and nothing else up to m and l.  (stage is a
// lambda in each kernel: DESIGN section 4, "Long attention, shared".)
// Q^T of a wave's 16 queries: rows = features 16 ft + 4 slot + r, column = query col; xsrc is the lane's x row at channel
// 4 slot.  A rolled loop (unrolled, its independent block sums take more registers than a lane has) that parks the tiles
// at qs (the lane's own place in LDS, stride 64 f32x4 per feature tile); each lane reads back what it wrote itself
template <int E>
__device__ __forceinline__ void ita_lf32_q_prologue(const float* xsrc, const float* wq, const float* bq, int col, int slot,
                                                    f32x4* qs, f32x4 (&q)[ItaLongF32Lds::NFT]) {
  constexpr int NFT = ItaLongF32Lds::NFT, NG = E / 16;
  f32x4 xf[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) xf[g] = *(const f32x4*)(xsrc + 16 * g);
#pragma unroll 1
  for (int ft = 0; ft < NFT; ft += 2) {
    f32x4 qa[2];
    const float* wqr[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      qa[u] = *(const f32x4*)(bq + 16 * (ft + u) + 4 * slot);
      wqr[u] = wq + (16 * (ft + u) + col) * E + 4 * slot;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const f32x4 w0 = *(const f32x4*)(wqr[0] + 16 * g), w1 = *(const f32x4*)(wqr[1] + 16 * g);
      f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[r], xf[g][r], t0, 0, 0, 0);
        t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[r], xf[g][r], t1, 0, 0, 0);
      }
      qa[0] += t0;
      qa[1] += t1;
    }
    qs[ft * 64] = qa[0];
    qs[(ft + 1) * 64] = qa[1];
  }
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) q[ft] = qs[ft * 64];
}
// S^T = K Q^T of the 64-key unit at kb: tile kt, lane (query col, slot) holds S[query][16 kt + 4 slot + r].  Block sums:
// the 16 features of tile ft are chained from zero (t) and the block goes onto the logit one step later, behind the next
// tile's MFMAs; the fragments of tile ft + 1 load while tile ft computes (the steps are kept apart: interleaved, the twelve
// independent blocks take more registers than a lane has)
__device__ __forceinline__ void ita_lf32_logits(const f32x4* kb, int lane, const f32x4 (&q)[ItaLongF32Lds::NFT],
                                                f32x4 (&s)[ItaLongF32Lds::NKT]) {
  constexpr int NFT = ItaLongF32Lds::NFT, NKT = ItaLongF32Lds::NKT;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) s[kt] = (f32x4){0, 0, 0, 0};
  f32x4 kf[2][NKT], t[2][NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) kf[0][kt] = kb[kt * 64 + lane];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    if (ft + 1 < NFT) {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) kf[(ft + 1) & 1][kt] = kb[((ft + 1) * NKT + kt) * 64 + lane];
    }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) t[ft & 1][kt] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
        t[ft & 1][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[ft & 1][kt][r], q[ft][r], t[ft & 1][kt], 0, 0, 0);
    if (ft > 0) {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) s[kt] += t[(ft - 1) & 1][kt];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) s[kt] += t[(NFT - 1) & 1][kt];
}
// The running maximum over a unit's 64 keys of query col (16 in the lane, the rest in lanes col + 16 slot): m becomes
// mn = max(m, max s), which is returned, and down = e^(m - mn) rescales what was summed under the old m (first unit: the
// clamp's e^-87, times zeros)
__device__ __forceinline__ float ita_lf32_running_max(const f32x4 (&s)[ItaLongF32Lds::NKT], float& m, float& down) {
  float mt = s[0][0];
#pragma unroll
  for (int kt = 0; kt < ItaLongF32Lds::NKT; ++kt)
#pragma unroll
    for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[kt][r]);
  mt = fmaxf(mt, __int_as_float(xor16_i(__float_as_int(mt))));
  mt = fmaxf(mt, __int_as_float(xor32_i(__float_as_int(mt))));
  const float mn = fmaxf(m, mt);
  down = ita_expf(m - mn);
  m = mn;
  return mn;
}
// the four slot lanes' shares of a query's sum, (v0 + v1) + (v2 + v3): the same bits in all four lanes
__device__ __forceinline__ float ita_lf32_sum_slots(float v) {
  v = v + __int_as_float(xor16_i(__float_as_int(v)));
  return v + __int_as_float(xor32_i(__float_as_int(v)));
}

template <int E, bool TAPS>
__device__ __forceinline__ void ita_lf32_attn_body(const ItaLongF32Args& a, const ItaLongF32TapArgs& tp) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel groups");
  using L = ItaLongF32Lds;
  constexpr int P = 192, XS = E + 4, NFT = L::NFT, NKT = L::NKT, NG = E / 16, EC = E / 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, slot = lane >> 4;
  const int t0 = 16 * wave;   // this wave's queries inside the tile
  const int nu = a.S / 64, qt = blockIdx.x, b = blockIdx.y;
  const char* kimg = (const char*)(a.kimg + (size_t)b * nu * L::UNIT_F4);
  const char* vimg = (const char*)(a.vimg + (size_t)b * nu * L::UNIT_F4);

  auto stage = [&](const char* src, int ldsoff) {    // 48 KB by LDS-DMA: six 1 KB pieces per wave
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int piece = wave + 8 * p;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + ldsoff + piece * 1024), 16, 0, 0);
    }
  };
  stage(kimg, L::K);

  // Q^T of the wave's queries, parked in the second K slot and the V slot: free until every wave has passed the first
  // barrier of the sweep
  const float* xsrc = a.x + ((size_t)b * a.S + (size_t)qt * 128 + t0 + col) * E + 4 * slot;
  f32x4 q[NFT];
  ita_lf32_q_prologue<E>(xsrc, a.wq, a.bq, col, slot, (f32x4*)(lds + L::K + L::UNIT) + wave * NFT * 64 + lane, q);
  // taps: the output row of this lane's query (the four slot lanes of a query agree), and whether the wave has any
  int ri = -1;
  bool wave_rows = false;
  size_t rowoff = 0;      // (b * n_rows + ri) * S: where this query's logit row starts
  if constexpr (TAPS) {
    if (tp.Q) {           // the fragments the sweep multiplies with: Q[query][16 ft + 4 slot + 0..3]
      float* qr = tp.Q + ((size_t)b * a.S + (size_t)qt * 128 + t0 + col) * P + 4 * slot;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft) *(f32x4*)(qr + 16 * ft) = q[ft];
    }
    if (tp.rowidx) ri = tp.rowidx[qt * 128 + t0 + col];
    wave_rows = __builtin_amdgcn_ballot_w64(ri >= 0) != 0;
    rowoff = ((size_t)b * tp.n_rows + (size_t)max(ri, 0)) * a.S;
  }

  // the sweep: running maximum m (the same in the four lanes of a query), this lane's share l of the running sum (its 16
  // keys of every unit; the four shares carry the same factors, so they are added once, at the end), context c
  float m = -__builtin_inff(), l = 0.0f;
  f32x4 c[NFT];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) c[ft] = (f32x4){0, 0, 0, 0};
  for (int u = 0; u < nu; ++u) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // K unit u landed for every wave; every wave is done with step u - 1: the V slot and the other K slot are free
    stage(vimg + (size_t)u * L::UNIT, L::V);
    if (u + 1 < nu) stage(kimg + (size_t)(u + 1) * L::UNIT, L::K + ((u + 1) & 1) * L::UNIT);

    // S^T = K Q^T: tile kt, lane (query col, slot) holds S[query][64 u + 16 kt + 4 slot + r]
    const f32x4* kb = (const f32x4*)(lds + L::K + (u & 1) * L::UNIT);
    f32x4 s[NKT];
    ita_lf32_logits(kb, lane, q, s);
    if constexpr (TAPS) {   // s[kt] = keys 64 u + 16 kt + 4 slot + 0..3 of query col: 16 bytes per store, before s becomes e^(s - m)
      if (wave_rows && tp.logits && ri >= 0) {
        float* lr = tp.logits + rowoff + 64 * u + 4 * slot;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) *(f32x4*)(lr + 16 * kt) = s[kt];
      }
    }
    // running softmax over the unit's 64 keys of query col: 16 in the lane, the rest in lanes col + 16 slot
    {
      float down;
      const float mn = ita_lf32_running_max(s, m, down);
      float sum = 0.0f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = ita_expf(s[kt][r] - mn);
          s[kt][r] = e;
          sum += e;
        }
      l = l * down + sum;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft) c[ft] *= down;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // V unit u (and K unit u + 1, requested a whole S^T ago)
    __syncthreads();

    // ctx^T += V^T P^T: lane (query col, slot) holds ctx[query][16 ft + 4 slot + r]; k = key 64 u + 16 kt + 4 slot + r
    const f32x4* vb = (const f32x4*)(lds + L::V);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 vf[NFT];
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft) vf[ft] = vb[(ft * NKT + kt) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ft = 0; ft < NFT; ++ft) c[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[ft][r], s[kt][r], c[ft], 0, 0, 0);
    }
  }
  {
    l = ita_lf32_sum_slots(l);
    const float inv = 1.0f / l;
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) c[ft] *= inv;
    if constexpr (TAPS) {
      if (ri >= 0 && slot == 0) {
        if (tp.row_max) tp.row_max[(size_t)b * tp.n_rows + ri] = m;
        if (tp.row_sum) tp.row_sum[(size_t)b * tp.n_rows + ri] = l;
      }
      if (tp.ctx) {       // out_proj's operand: ctx[query][16 ft + 4 slot + 0..3]
        float* cr = tp.ctx + ((size_t)b * a.S + (size_t)qt * 128 + t0 + col) * P + 4 * slot;
#pragma unroll
        for (int ft = 0; ft < NFT; ++ft) *(f32x4*)(cr + 16 * ft) = c[ft];
      }
    }
  }

  // out^T = Wo ctx^T + bo: lane (query col, slot) holds out[query][16 et + 4 slot + r]
  f32x4 o[NG];
  const float* wor[NG];
#pragma unroll
  for (int et = 0; et < NG; ++et) {
    o[et] = *(const f32x4*)(a.bo + 16 * et + 4 * slot);
    wor[et] = a.wo + (16 * et + col) * P + 4 * slot;
  }
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    f32x4 wf[NG];
#pragma unroll
    for (int et = 0; et < NG; ++et) wf[et] = *(const f32x4*)(wor[et] + 16 * ft);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int et = 0; et < NG; ++et) o[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[et][r], c[ft][r], o[et], 0, 0, 0);
  }
  // the wave's own rows, over the K ring (ItaLongF32Lds): x + out, or out alone
  float* xl = (float*)(lds + L::K);
  {
    float* xr = xl + (t0 + col) * XS + 4 * slot;
#pragma unroll
    for (int et = 0; et < NG; ++et) {
      f32x4 v = o[et];
      if (a.fuse_ln) v = *(const f32x4*)(xsrc + 16 * et) + v;
      *(f32x4*)(xr + 16 * et) = v;
    }
  }
  __syncthreads();

  // finish: 4 lanes per token (token t0 + lane / 4, channels E / 4 (lane & 3) ..): LayerNorm1, y
  {
    const int tok = lane >> 2, qtr = lane & 3;
    float r[EC];
#pragma unroll
    for (int i = 0; i < EC; i += 4) {
      const f32x4 v = *(const f32x4*)(xl + (t0 + tok) * XS + qtr * EC + i);
      r[i] = v.x; r[i + 1] = v.y; r[i + 2] = v.z; r[i + 3] = v.w;
    }
    if (a.fuse_ln) layernorm_lanes<E>(r, a.ln_w, a.ln_b, qtr * EC);
    float* yrow = a.y + ((size_t)b * a.S + (size_t)qt * 128 + t0 + tok) * E + qtr * EC;
#pragma unroll
    for (int i = 0; i < EC; i += 4) *(f32x4*)(yrow + i) = (f32x4){r[i], r[i + 1], r[i + 2], r[i + 3]};
  }
}
template <int E>
__global__ __launch_bounds__(512) void ita_lf32_attn_kernel(const ItaLongF32Args a) {
  ita_lf32_attn_body<E, false>(a, ItaLongF32TapArgs{});
}
template <int E>
__global__ __launch_bounds__(512) void ita_lf32_attn_taps_kernel(const ItaLongF32Args a, const ItaLongF32TapArgs tp) {
  ita_lf32_attn_body<E, true>(a, tp);
}

// probs[b, i, k] = ita_expf(logits[b, i, k] - row_max[b, i]) * (1.0f / row_sum[b, i]): one subtraction, ita_expf, one
// division and one multiplication, each rounded on its own (the build keeps -ffp-contract=off).  One workgroup per
// (frame, chosen row), 16 bytes per lane and step.  lg may be probs itself (the caller asked for no logits): a lane reads
// the four values it then overwrites, and no other lane touches them.
__global__ __launch_bounds__(256) void ita_lf32_probs_kernel(const float* lg, float* probs, const float* row_max,
                                                             const float* row_sum, int S) {
  const size_t row = blockIdx.x;
  const float m = row_max[row], inv = 1.0f / row_sum[row];
  const f32x4* src = (const f32x4*)(lg + row * S);
  f32x4* dst = (f32x4*)(probs + row * S);
  for (int i = threadIdx.x; i < S / 4; i += 256) {
    const f32x4 v = src[i];
    f32x4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = ita_expf(v[r] - m) * inv;
    dst[i] = p;
  }
}
