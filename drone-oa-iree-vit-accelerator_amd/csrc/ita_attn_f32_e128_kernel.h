// ita_attn_f32_e128_kernel.h -- the float32 attention block of the E = 128 float graph on gfx950 f32 MFMA.
//
//   ita_attn_f32_e128_kernel : ITASelfAttention.forward (models/ITA/layers.py:47-88) at E = 128, + optional residual +
//                              LayerNorm1 (models/ITA_upsample_shuffle/model.py:97-103), all float32; the same block
//                              as ita_attn_f32_kernel (ita_attn_f32_kernel.h), whose numerics and GEMM chain it keeps.
//
// The E = 64 kernel keeps an x tile [128][68] resident beside the K / V fragment image (96 KB).  At E = 128 that tile is
// [128][132] (66 KB) and the two no longer fit in 160 KB of LDS.  But a wave only ever reads x of its own 16 tokens (its
// Q, K and V rows, its residual), so here the x fragments come straight from memory into registers (8 x f32x4 per lane)
// and stay there until the residual.  LDS holds only the fragment image [12][8][64] f32x4 (96 KB): K^T, then V, and,
// once every wave is past the context GEMM, the wave's x + out rows [128][132] for the LayerNorm hand-over.
// In place (y == x) is safe: a wave reads its own x rows before it writes the same y rows, and no other wave reads them.
//
// Roofline: (3 x 128 x 128 x 192 + 2 x 128 x 128 x 192 + 128 x 192 x 128) MAC = 18.87 M MAC = 37.75 MFLOP per frame;
// f32 MFMA peak 157.3 TF -> >= 246 us per 1024 frames.  HBM: 2 x 64 KB per frame -> 27 us per 1024 frames: compute bound.
#pragma once
#include "ita_attn_f32_kernel.h"

struct ItaAttnF32E128Lds {
  static constexpr int S = 128, E = 128, P = 192, XS = E + 4, NFT = P / 16, NKT = S / 16;
  static constexpr int KV = 0;                             // f32x4 [NFT][NKT][64]  K^T, then V, fragments
  static constexpr int X = 0;                              // f32 [S][XS]  x + out rows, over the image (after ctx)
  static constexpr int TOTAL = KV + NFT * NKT * 64 * 16;   // 98304 bytes
  static_assert(S * XS * 4 <= TOTAL, "the x + out rows overlay the fragment image");
};

__global__ __launch_bounds__(512) void ita_attn_f32_e128_kernel(const ItaAttnF32Args a) {
  using L = ItaAttnF32E128Lds;
  constexpr int S = L::S, E = L::E, P = L::P, XS = L::XS, NFT = L::NFT, NKT = L::NKT, NG = E / 16, EC = E / 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* xl = (float*)(lds + L::X);
  f32x4* kv = (f32x4*)(lds + L::KV);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;
  const int t0 = 16 * wave;   // this wave's tokens

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    // x fragments of the wave's tokens: lane (token col, slot), group g holds x[t0 + col][16 g + 4 slot + 0..3]; read
    // again (from L1 / L2) for V and the residual rather than held across the softmax: 32 VGPRs fewer at the peak
    const float* xsrc = a.x + ((size_t)b * S + t0 + col) * E + 4 * slot;
    f32x4 xf[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) xf[g] = *(const f32x4*)(xsrc + 16 * g);

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
        const f32x4 xg = *(const f32x4*)(xsrc + 16 * g);
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
    __syncthreads();   // every wave is done with V: the x + out rows overlay the image

    // out^T = Wo ctx^T + bo: lane (query col, slot) holds out[t0 + col][16 et + 4 slot + r], the layout of xf[et]
    f32x4 o[E / 16];
    const float* wor[E / 16];   // one opaque row offset per et, the ft steps as immediates: 96 opaque offsets spill
#pragma unroll
    for (int et = 0; et < E / 16; ++et) {
      o[et] = *(const f32x4*)(a.bo + 16 * et + 4 * slot);
      wor[et] = a.wo + ita_opaque((16 * et + col) * P + 4 * slot);
    }
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
      f32x4 wf[E / 16];
#pragma unroll
      for (int et = 0; et < E / 16; ++et) wf[et] = *(const f32x4*)(wor[et] + 16 * ft);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int et = 0; et < E / 16; ++et) o[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[et][r], c[ft][r], o[et], 0, 0, 0);
    }
    // the wave's own rows: x + out, or out alone
    {
      float* xr = xl + (t0 + col) * XS + 4 * slot;
#pragma unroll
      for (int et = 0; et < E / 16; ++et) {
        f32x4 v = o[et];
        if (a.fuse_ln) v = *(const f32x4*)(xsrc + 16 * et) + v;
        *(f32x4*)(xr + 16 * et) = v;
      }
    }
    __syncthreads();

    // finish: 4 lanes per token (token t0 + lane / 4, channels 32 (lane & 3) ..): LayerNorm1, y
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
    __syncthreads();   // the next frame overwrites the rows with its K image
  }
}
