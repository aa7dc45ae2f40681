// ita_attn_f32_kernel.h -- the float32 attention block of the float ViT+LSTM graph on gfx950 f32 MFMA, E = 64 and 128.
//
//   ita_attn_f32_kernel<E> : ITASelfAttention.forward (models/ITA/layers.py:47-88: q/k/v Linear E -> P, softmax(Q K^T)
//                            with no 1/sqrt(d), context V, out Linear P -> E; one head) + optional residual + LayerNorm1
//                            (E = 64: models/ITA_single_layer_upsample_shuffle/model.py:96-101, E = 128:
//                            models/ITA_upsample_shuffle/model.py:97-103), all float32:
//                            y = LayerNorm1(x + out_proj(softmax(Q K^T) V)),   Q / K / V = x W^T + b
//
// Numerics: f32 MFMA (v_mfma_f32_16x16x4_f32, an exact fmaf chain per output), every accumulator seeded with its bias.
// Summation order is free here (the reference is torch's f32 GEMMs), so each reduction walks k in the order its operands
// arrive: a lane loads 4 consecutive k as one f32x4, and k-step (g, r) of a fragment read feeds k = 16 g + 4 slot + r.
// Softmax per query row: subtract the row max, ita_expf (the oracle's exp), multiply by the reciprocal of the row sum.
//
// Shape: one frame per workgroup (grid stride), 8 waves; wave w owns tokens 16w..16w+15 as keys / values and as queries.
// Every GEMM is written so that its output accumulator IS the next GEMM's operand fragment (the A and B fragments of
// 16x16x4 share one lane map: lane & 15 = row / column, lane >> 4 = k slot):
//   Q^T = Wq x^T      D lane (token, slot) holds Q[token][16 ft + 4 slot + r]   -> B operand of S^T, in registers
//   K^T = Wk x^T      same layout                                                -> A operand of S^T, via LDS (kv)
//   S^T = K Q^T       D lane (query, slot) holds S[query][16 kt + 4 slot + r]   -> softmax over (kt, r) and slot
//   V   = x Wv^T      D lane (feature, slot) holds V[16 w + 4 slot + r][feat]   -> A operand of ctx^T, via LDS (kv)
//   ctx^T = V^T P^T   D lane (query, slot) holds ctx[query][16 ft + 4 slot + r] -> B operand of out^T, in registers
//   out^T = Wo ctx^T  D lane (query, slot) holds out[query][16 et + 4 slot + r] -> + x in the wave's own rows of LDS
// The four weight matrices stream from L1 / L2 as f32x4 fragments.
// Per frame: x -> LDS or registers | Q, K (K -> LDS) | S, softmax | V -> LDS | ctx, out | + x -> LDS rows | LayerNorm1 -> y.
//
// LDS at E = 64: the x tile [128][68] (34 KB, resident for the residual) and one fragment image of K, later of V,
// [12][8][64] f32x4 (96 KB): 130 KB, one workgroup per CU.
// LDS at E = 128: that tile is [128][132] (66 KB) and the two no longer fit in 160 KB of LDS.  But a wave only ever reads x
// of its own 16 tokens (its Q, K and V rows, its residual), so there the x fragments come straight from memory into
// registers (8 x f32x4 per lane).  LDS holds only the fragment image (96 KB): K^T, then V, and, once every wave is past
// the context GEMM, the wave's x + out rows [128][132] for the LayerNorm hand-over.
// In place (y == x) is safe at both: a wave reads its own x rows before it writes the same y rows, and no other wave reads
// them (E = 64: the whole frame is in LDS before the first y row is written).
//
// Roofline, E = 64: (3 x 128 x 64 x 192 + 2 x 128 x 128 x 192 + 128 x 192 x 64) MAC = 12.58 M MAC = 25.17 MFLOP per frame;
// f32 MFMA peak 157.3 TF -> >= 164 us per 1024 frames.  HBM: 2 x 32 KB per frame -> 13 us per 1024 frames: compute bound.
// E = 128: (3 x 128 x 128 x 192 + 2 x 128 x 128 x 192 + 128 x 192 x 128) MAC = 18.87 M MAC = 37.75 MFLOP per frame;
// >= 246 us per 1024 frames.  HBM: 2 x 64 KB per frame -> 27 us per 1024 frames: compute bound.
#pragma once
#include "ita_device.h"

struct ItaAttnF32Args {
  const float* x;                 // (rows, E) f32 block input
  float* y;                       // (rows, E) f32: fuse_ln ? LayerNorm1(x + attn(x)) : attn(x); may alias x
  const float *wq, *wk, *wv;      // [P][E] (nn.Linear [out][in])
  const float *bq, *bk, *bv;      // [P]
  const float *wo, *bo;           // [E][P], [E]
  const float *ln_w, *ln_b;       // LayerNorm1 affine
  int B;                          // frames (128 token rows each)
  int fuse_ln;
};

template <int E>
struct ItaAttnF32Lds {
  static constexpr int S = 128, P = 192, XS = E + 4, NFT = P / 16, NKT = S / 16;
  static constexpr bool X_RESIDENT = E == 64;              // else the x + out rows overlay the image (after ctx)
  static constexpr int X = 0;                              // f32 [S][XS]  x tile (resident), or x + out rows (overlay)
  static constexpr int KV = X_RESIDENT ? S * XS * 4 : 0;   // f32x4 [NFT][NKT][64]  K^T, then V, fragments
  static constexpr int TOTAL = KV + NFT * NKT * 64 * 16;   // 133120 bytes (E = 64), 98304 bytes (E = 128)
  static_assert(X_RESIDENT || S * XS * 4 <= TOTAL, "the x + out rows overlay the fragment image");
};

// a per-lane offset the compiler cannot treat as loop invariant: without it, every weight tile's 64-bit address is hoisted
// out of the frame loop and spilled
__device__ __forceinline__ int ita_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int E>
__global__ __launch_bounds__(512) void ita_attn_f32_kernel(const ItaAttnF32Args a) {
  using L = ItaAttnF32Lds<E>;
  constexpr int S = L::S, P = L::P, XS = L::XS, NFT = L::NFT, NKT = L::NKT, NG = E / 16, EC = E / 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* xl = (float*)(lds + L::X);
  f32x4* kv = (f32x4*)(lds + L::KV);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;
  const int t0 = 16 * wave;   // this wave's tokens

  // x tile staging (resident x): thread tid moves floats [16 (tid & 3), +16) of row tid / 4 (no prefetch: its 16
  // registers cost more than the load latency it would hide, once per ~10^5 MFMA cycles of a frame)
  const int sr = tid >> 2, sc = (tid & 3) * 16;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    if constexpr (L::X_RESIDENT) {
      const float* src = a.x + ((size_t)b * S + sr) * E + sc;
      f32x4 xv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[i] = *(const f32x4*)(src + 4 * i);
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(xl + sr * XS + sc + 4 * i) = xv[i];
      __syncthreads();
    }

    // x fragments of the wave's tokens: lane (token col, slot), group g holds x[t0 + col][16 g + 4 slot + 0..3]; from the
    // LDS tile, or (E = 128: no room for the tile) from memory, and then read again (from L1 / L2) for V and the
    // residual rather than held across the softmax: 32 VGPRs fewer at the peak.  xsrc is null where the tile is resident:
    // left as dead address arithmetic it reorders the live address arithmetic of the E = 64 kernel
    const float* xsrc = L::X_RESIDENT ? nullptr : a.x + ((size_t)b * S + t0 + col) * E + 4 * slot;
    f32x4 xf[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if constexpr (L::X_RESIDENT) xf[g] = *(const f32x4*)(xl + (t0 + col) * XS + 16 * g + 4 * slot);
      else xf[g] = *(const f32x4*)(xsrc + 16 * g);
    }

    // Q^T (registers) and K^T (-> LDS): rows = features 16 ft + 4 slot + r, column = token col
    f32x4 q[NFT];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
      f32x4 qa = *(const f32x4*)(a.bq + 16 * ft + 4 * slot);
      f32x4 ka = *(const f32x4*)(a.bk + 16 * ft + 4 * slot);
      const int wr = ita_opaque((16 * ft + col) * E + 4 * slot);
      const float *wqr = a.wq + wr, *wkr = a.wk + wr;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 wqf = *(const f32x4*)(wqr + 16 * g), wkf = *(const f32x4*)(wkr + 16 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          qa = __builtin_amdgcn_mfma_f32_16x16x4f32(wqf[r], xf[g][r], qa, 0, 0, 0);
          ka = __builtin_amdgcn_mfma_f32_16x16x4f32(wkf[r], xf[g][r], ka, 0, 0, 0);
        }
      }
      q[ft] = qa;
      kv[(ft * NKT + wave) * 64 + lane] = ka;
    }
    __syncthreads();

    // S^T = K Q^T: tile kt, lane (query col, slot) holds S[t0 + col][16 kt + 4 slot + r]
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) s[kt] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
      f32x4 kf[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) kf[kt] = kv[(ft * NKT + kt) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt][r], q[ft][r], s[kt], 0, 0, 0);
    }
    // softmax over the 128 keys of query col: 32 in the lane, the rest in lanes col + 16 slot
    {
      float m = s[0][0];
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, s[kt][r]);
      m = fmaxf(m, __int_as_float(xor16_i(__float_as_int(m))));
      m = fmaxf(m, __int_as_float(xor32_i(__float_as_int(m))));
      float sum = 0.0f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = ita_expf(s[kt][r] - m);
          s[kt][r] = e;
          sum += e;
        }
      sum = sum + __int_as_float(xor16_i(__float_as_int(sum)));   // the same sum in all four lanes of the row
      sum = sum + __int_as_float(xor32_i(__float_as_int(sum)));
      const float inv = 1.0f / sum;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] *= inv;
    }
    __syncthreads();   // every wave is done with K

    // V = x Wv^T (-> LDS over K): lane (feature 16 ft + col, slot) holds V[t0 + 4 slot + r][feature]
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
        f32x4 xg;
        if constexpr (L::X_RESIDENT) xg = xf[g];
        else xg = *(const f32x4*)(xsrc + 16 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          va[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xg[r], w0[r], va[0], 0, 0, 0);
          va[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(xg[r], w1[r], va[1], 0, 0, 0);
        }
      }
      kv[(ft * NKT + wave) * 64 + lane] = va[0];
      kv[((ft + 1) * NKT + wave) * 64 + lane] = va[1];
    }
    __syncthreads();

    // ctx^T = V^T P^T: lane (query col, slot) holds ctx[t0 + col][16 ft + 4 slot + r]; k = key 16 kt + 4 slot + r
    f32x4 c[NFT];
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) c[ft] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 vf[NFT];
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft) vf[ft] = kv[(ft * NKT + kt) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ft = 0; ft < NFT; ++ft) c[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[ft][r], s[kt][r], c[ft], 0, 0, 0);
    }
    if constexpr (!L::X_RESIDENT) __syncthreads();   // every wave is done with V: the x + out rows overlay the image

    // out^T = Wo ctx^T + bo: lane (query col, slot) holds out[t0 + col][16 et + 4 slot + r], the layout of xf[et].
    // The Wo row offsets are opaque per (et, ft) at E = 64; at E = 128 one opaque row offset per et, the ft steps as
    // immediates: 96 opaque offsets spill
    f32x4 o[NG];
    const float* wor[NG];
#pragma unroll
    for (int et = 0; et < NG; ++et) {
      o[et] = *(const f32x4*)(a.bo + 16 * et + 4 * slot);
      if constexpr (E != 64) wor[et] = a.wo + ita_opaque((16 * et + col) * P + 4 * slot);
    }
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
      f32x4 wf[NG];
#pragma unroll
      for (int et = 0; et < NG; ++et) {
        if constexpr (E == 64) wf[et] = *(const f32x4*)(a.wo + ita_opaque((16 * et + col) * P + 16 * ft + 4 * slot));
        else wf[et] = *(const f32x4*)(wor[et] + 16 * ft);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int et = 0; et < NG; ++et) o[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[et][r], c[ft][r], o[et], 0, 0, 0);
    }
    // the wave's own rows (no other wave reads them any more): x + out, or out alone; x from the tile, else from memory
    {
      float* xr = xl + (t0 + col) * XS + 4 * slot;
#pragma unroll
      for (int et = 0; et < NG; ++et) {
        f32x4 v = o[et];
        if (a.fuse_ln) {
          if constexpr (L::X_RESIDENT) v = *(const f32x4*)(xr + 16 * et) + v;
          else v = *(const f32x4*)(xsrc + 16 * et) + v;
        }
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
      float* yrow = a.y + ((size_t)b * S + t0 + tok) * E + qtr * EC;
#pragma unroll
      for (int i = 0; i < EC; i += 4) *(f32x4*)(yrow + i) = (f32x4){r[i], r[i + 1], r[i + 2], r[i + 3]};
    }
    __syncthreads();   // the next frame overwrites the x tile and the K image (E = 128: the rows with its K image)
  }
}
