// ita_ffn_f32_e128_kernel.h -- the float32 FFN of the E = 128 float graph on gfx950 f32 MFMA.
//
//   ita_ffn_f32_e128_kernel : ITAFeedForward.forward (models/ITA/layers.py:29-45: fc1 128 -> 256, ReLU, fc2 256 -> 128)
//                             + optional residual + LayerNorm2 (models/ITA_upsample_shuffle/model.py:97-103), float32:
//                             y = LayerNorm2(x1 + fc2(relu(fc1(x1) + b1)) + b2)
//
// Numerics: those of ita_ffn_f32_kernel (ita_ffn_f32_kernel.h:7-11), bit-identical to the oracle composition
// add_ln(x1, linear_f32(max(linear_f32(x1, W1, b1), 0), W2, b2)): every accumulator starts as the bias, k-step s feeds
// k = 4 s + slot in ascending s, and the hidden layer goes through LDS in natural [token][feature] order.
//
// At E = 64 the weights stay in registers for the whole launch (128 VGPRs).  At E = 128 they are 256 KB, 256 VGPRs
// per lane over 4 waves, so they stream from L1 / L2 as MFMA B fragments instead, from a fragment image made at load
// (ita_ffn_f32_frag_image): one f32x4 per lane carries the lane's operand for four consecutive k-steps, and each f32x4
// feeds 8 MFMAs (4 k-steps x the tile's two 16-token halves).
//
// One 256-thread workgroup (4 waves) walks 32-token tiles (a quarter frame) with a grid stride; 66 KB of LDS, so two
// workgroups per CU.  Per tile:
//   x1 tile -> LDS [32][132] (the next tile is prefetched into registers meanwhile)
//   fc1 + ReLU: wave w, features 64w..64w+63 x both 16-token halves, 8 accumulators of 32 steps -> h LDS [32][260]
//   fc2: wave w, outputs 32w..32w+31 x both halves, 4 accumulators of 64 steps -> LDS [32][132]
//   finish: 4 threads per token: + x1, layernorm_lanes<128> (bit-exact with the oracle), y / f16 planes
// Row strides of 132 and 260 floats put the 16 rows x 4 k-slots of a fragment read, and the 4 rows x 16 columns of an
// accumulator store, on 64 distinct banks.
//
// Roofline: 2 x 128 x 128 x 256 MAC = 16.8 MFLOP per frame; f32 MFMA peak 157.3 TF -> >= 109 us per 1024 frames.
// HBM: 2 x 64 KB per frame (x1 in, y out) -> 27 us per 1024 frames at 5 TB/s: compute bound.
#pragma once
#include "ita_ffn_f32_kernel.h"

struct ItaFfnF32E128Lds {
  static constexpr int TT = 32, E = 128, F = 256, XS = E + 4, HS = F + 4;
  static constexpr int X = 0;                     // f32 [TT][XS]  x1 tile
  static constexpr int H = X + TT * XS * 4;       // f32 [TT][HS]  relu(fc1)
  static constexpr int O = H + TT * HS * 4;       // f32 [TT][XS]  fc2 output
  static constexpr int TOTAL = O + TT * XS * 4;   // 67072 bytes
};

// B-fragment image of a row-major [R][K] matrix W (R, K multiples of 16), as ita_ffn_f32_e128_kernel reads it:
// f32x4 [R/16][K/16][64], lane (col, slot) of (row tile rt, k group g) holds W[16 rt + col][16 g + 4 r + slot], r = 0..3
// (its B operand for k-steps 4 g .. 4 g + 3)
inline void ita_ffn_f32_frag_image(const float* w, int R, int K, float* img) {
  for (int rt = 0; rt < R / 16; ++rt)
    for (int g = 0; g < K / 16; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r)
          img[(((size_t)rt * (K / 16) + g) * 64 + lane) * 4 + r] = w[(size_t)(16 * rt + (lane & 15)) * K + 16 * g + 4 * r + (lane >> 4)];
}

// a.w1 / a.w2 are the fragment images of W1 [256][128] and W2 [128][256] (ita_ffn_f32_frag_image), not the matrices
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ita_ffn_f32_e128_kernel(const ItaFfnF32Args a) {
  using L = ItaFfnF32E128Lds;
  constexpr int TT = L::TT, E = L::E, F = L::F, XS = L::XS, HS = L::HS, S = 128, EC = E / 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* xl = (float*)(lds + L::X);
  float* hl = (float*)(lds + L::H);
  float* ol = (float*)(lds + L::O);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;   // B fragment: row (feature) col, k = 4 * step + slot
  const int ntile = a.B * (S / TT);
  const f32x4* w1p = (const f32x4*)a.w1 + (size_t)4 * wave * (E / 16) * 64 + lane;   // row tiles 4w .. 4w + 3
  const f32x4* w2p = (const f32x4*)a.w2 + (size_t)2 * wave * (F / 16) * 64 + lane;   // row tiles 2w, 2w + 1

  float b1v[4], b2v[2];
#pragma unroll
  for (int ft = 0; ft < 4; ++ft) b1v[ft] = a.b1[64 * wave + 16 * ft + col];
#pragma unroll
  for (int et = 0; et < 2; ++et) b2v[et] = a.b2[32 * wave + 16 * et + col];

  // x1 tile staging: thread tid moves floats [16 tid, 16 tid + 16) of the 32 x 128 tile (row tid / 8)
  const int sr = tid >> 3, sc = (tid & 7) * 16;
  f32x4 xv[4] = {};
  if (blockIdx.x < ntile) {
    const float* src = a.x + ((size_t)blockIdx.x * TT + sr) * E + sc;
#pragma unroll
    for (int i = 0; i < 4; ++i) xv[i] = *(const f32x4*)(src + 4 * i);
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *(f32x4*)(xl + sr * XS + sc + 4 * i) = xv[i];
    const int b = tile / (S / TT), t0 = (tile % (S / TT)) * TT;   // frame, first token of the tile
    if (a.h0_dst && t0 == 0 && tid < 32) {
      const size_t row = a.slots ? (size_t)a.slots[b] : (size_t)b;
      *(f32x4*)(a.h0_dst + (size_t)b * 128 + 4 * tid) = *(const f32x4*)(a.h0_src + row * 128 + 4 * tid);
    }
    __syncthreads();
    const int nxt = tile + gridDim.x;
    if (nxt < ntile) {   // prefetch: consumed at the top of the next iteration
      const float* src = a.x + ((size_t)nxt * TT + sr) * E + sc;
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[i] = *(const f32x4*)(src + 4 * i);
    }

    // fc1 + ReLU
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) acc[m][ft] = (f32x4){b1v[ft], b1v[ft], b1v[ft], b1v[ft]};
      // the weight fragments of group g + 1 load while group g computes (a rolled loop: unrolled, the compiler hoists
      // every group's loads and spills)
      f32x4 wb[4];
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) wb[ft] = w1p[(size_t)ft * (E / 16) * 64];
#pragma unroll 1
      for (int g = 0; g < E / 16; ++g) {
        const int gn = g + 1 < E / 16 ? g + 1 : g;
        f32x4 wn[4];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) wn[ft] = w1p[((size_t)ft * (E / 16) + gn) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = 4 * g + r;
          const float a0 = xl[col * XS + 4 * s + slot], a1 = xl[(16 + col) * XS + 4 * s + slot];
#pragma unroll
          for (int ft = 0; ft < 4; ++ft) {
            acc[0][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wb[ft][r], acc[0][ft], 0, 0, 0);
            acc[1][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wb[ft][r], acc[1][ft], 0, 0, 0);
          }
        }
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) wb[ft] = wn[ft];
      }
      // D: lane holds rows (tokens) 4 * slot + r, column (feature) col; ReLU as max(h, 0) keeps -0 and NaN like numpy
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = acc[m][ft][r];
            hl[(16 * m + 4 * slot + r) * HS + 64 * wave + 16 * ft + col] = v < 0.0f ? 0.0f : v;
          }
    }
    __syncthreads();

    // fc2
    {
      f32x4 acc[2][2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int et = 0; et < 2; ++et) acc[m][et] = (f32x4){b2v[et], b2v[et], b2v[et], b2v[et]};
      f32x4 wb[2];
#pragma unroll
      for (int et = 0; et < 2; ++et) wb[et] = w2p[(size_t)et * (F / 16) * 64];
#pragma unroll 1
      for (int g = 0; g < F / 16; ++g) {
        const int gn = g + 1 < F / 16 ? g + 1 : g;
        f32x4 wn[2];
#pragma unroll
        for (int et = 0; et < 2; ++et) wn[et] = w2p[((size_t)et * (F / 16) + gn) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = 4 * g + r;
          const float a0 = hl[col * HS + 4 * s + slot], a1 = hl[(16 + col) * HS + 4 * s + slot];
#pragma unroll
          for (int et = 0; et < 2; ++et) {
            acc[0][et] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wb[et][r], acc[0][et], 0, 0, 0);
            acc[1][et] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wb[et][r], acc[1][et], 0, 0, 0);
          }
        }
#pragma unroll
        for (int et = 0; et < 2; ++et) wb[et] = wn[et];
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int et = 0; et < 2; ++et)
#pragma unroll
          for (int r = 0; r < 4; ++r) ol[(16 * m + 4 * slot + r) * XS + 32 * wave + 16 * et + col] = acc[m][et][r];
    }
    __syncthreads();

    // finish: token tid / 4, channels 32 * (tid & 3) ..
    if (tid < 4 * TT) {
      const int tok = tid >> 2, qtr = tid & 3;
      float r[EC];
#pragma unroll
      for (int i = 0; i < EC; i += 4) {
        const f32x4 v = *(const f32x4*)(ol + tok * XS + qtr * EC + i);
        r[i] = v.x; r[i + 1] = v.y; r[i + 2] = v.z; r[i + 3] = v.w;
      }
      if (a.fuse_ln) {
#pragma unroll
        for (int i = 0; i < EC; i += 4) {
          const f32x4 v = *(const f32x4*)(xl + tok * XS + qtr * EC + i);
          r[i] = v.x + r[i]; r[i + 1] = v.y + r[i + 1]; r[i + 2] = v.z + r[i + 2]; r[i + 3] = v.w + r[i + 3];
        }
        layernorm_lanes<E>(r, a.ln_w, a.ln_b, qtr * EC);
      }
      if (a.y) {
        float* yrow = a.y + ((size_t)tile * TT + tok) * E + qtr * EC;
#pragma unroll
        for (int i = 0; i < EC; i += 4) *(f32x4*)(yrow + i) = (f32x4){r[i], r[i + 1], r[i + 2], r[i + 3]};
      }
      if (a.y_hi) {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        const size_t po = (size_t)b * a.ld_planes + (size_t)(t0 + tok) * E + qtr * EC;
#pragma unroll
        for (int i = 0; i < EC; i += 8) {
          h8 vh, vl;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const _Float16 hh = (_Float16)r[i + j];
            vh[j] = hh;
            vl[j] = (_Float16)(r[i + j] - (float)hh);
          }
          *(h8*)(a.y_hi + po + i) = vh;
          *(h8*)(a.y_lo + po + i) = vl;
        }
      }
    }
    __syncthreads();   // the next tile overwrites the x1 and output tiles
  }
}
