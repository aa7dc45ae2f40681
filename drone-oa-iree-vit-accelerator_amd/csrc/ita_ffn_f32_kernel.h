// ita_ffn_f32_kernel.h -- the float32 FFN of the attention-only QAT graph on gfx950 f32 MFMA.
//
//   ita_ffn_f32_kernel : ITAFeedForward.forward (models/ITA/layers.py:29-45: fc1 E -> 256, ReLU, fc2 256 -> E)
//                        + optional residual + LayerNorm2 (QAT_only_attn/model.py:76-88), all float32:
//                        y = LayerNorm2(x1 + fc2(relu(fc1(x1) + b1)) + b2)
//
// Numerics: bit-identical to the oracle composition add_ln(x1, linear_f32(max(linear_f32(x1, W1, b1), 0), W2, b2)).
// ita_oracle_linear_f32 is one fmaf chain per output, started from the bias, in ascending k; v_mfma_f32_16x16x4_f32
// computes exactly that chain in k-slot order, so C starts as the bias and the K steps are issued in ascending order
// with k = 4 * step + slot.  The hidden layer goes through an LDS tile in natural [token][feature] order, so fc2's A
// fragments come in ascending k as well (the int8 FFN's register hand-over permutes k, which an f32 chain would notice).
//
// One 256-thread workgroup (4 waves, one per SIMD; 242 VGPRs, so two workgroups per CU) walks 32-token tiles (a quarter
// frame) with a grid stride.
// Weights stay in registers as MFMA B fragments for the whole launch: wave w holds W1 rows 64w..64w+63 (64 VGPRs)
// and W2 rows 16w..16w+15 (64 VGPRs).  Per tile:
//   x1 tile -> LDS [32][68] (the next tile is prefetched into registers meanwhile)
//   fc1 + ReLU: wave w, features 64w..64w+63 x both 16-token halves, 8 accumulators of 16 steps -> h LDS [32][260]
//   fc2: wave w, outputs 16w..16w+15 x both halves, 2 accumulators of 64 steps -> LDS [32][68]
//   finish: 4 threads per token: + x1, layernorm_lanes (the int8 kernels' bit-exact LayerNorm), y / f16 planes
// Row strides of 68 and 260 floats put the 16 rows x 4 k-slots of a fragment read, and the 4 rows x 16 columns of an
// accumulator store, on 64 distinct banks.
//
// Roofline: 2 x 128 x 64 x 256 MAC = 8.39 MFLOP per frame; f32 MFMA peak 157.3 TF -> >= 53 us per 1024 frames.
// HBM: 2 x 32 KB per frame (x1 in, y out) -> 13 us per 1024 frames at 5 TB/s: compute bound.
#pragma once
#include "ita_device.h"

struct ItaFfnF32Args {
  const float* x;            // (rows, E) f32 block input (x1)
  float* y;                  // (rows, E) f32: fuse_ln ? LayerNorm2(x + ffn(x)) : ffn(x); may alias x; may be null
  const float *w1, *b1;      // [F][E], [F]   (nn.Linear [out][in])
  const float *w2, *b2;      // [E][F], [E]
  const float *ln_w, *ln_b;  // LayerNorm2 affine
  int B;                     // frames (128 token rows each)
  int fuse_ln;
  // optional f16 hi/lo planes of y [B][ld_planes] for the folded decoder GEMM (tail mode 1)
  _Float16 *y_hi, *y_lo;
  int ld_planes;
  // optional side copy for the LSTM: h0_src[slots ? slots[b] : b] -> h0_dst[b] (128 floats per frame)
  const float* h0_src;
  float* h0_dst;
  const int* slots;
};

struct ItaFfnF32Lds {
  static constexpr int TT = 32, E = 64, F = 256, XS = E + 4, HS = F + 4;
  static constexpr int X = 0;                     // f32 [TT][XS]  x1 tile
  static constexpr int H = X + TT * XS * 4;       // f32 [TT][HS]  relu(fc1)
  static constexpr int O = H + TT * HS * 4;       // f32 [TT][XS]  fc2 output
  static constexpr int TOTAL = O + TT * XS * 4;   // 50688 bytes
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ita_ffn_f32_kernel(const ItaFfnF32Args a) {
  using L = ItaFfnF32Lds;
  constexpr int TT = L::TT, E = L::E, F = L::F, XS = L::XS, HS = L::HS, S = 128, EC = E / 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* xl = (float*)(lds + L::X);
  float* hl = (float*)(lds + L::H);
  float* ol = (float*)(lds + L::O);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;   // B fragment: row (feature) col, k = 4 * step + slot
  const int ntile = a.B * (S / TT);

  // weights as B fragments, resident for the whole launch
  float w1f[4][E / 4], w2f[F / 4];
#pragma unroll
  for (int ft = 0; ft < 4; ++ft)
#pragma unroll
    for (int s = 0; s < E / 4; ++s) w1f[ft][s] = a.w1[(size_t)(64 * wave + 16 * ft + col) * E + 4 * s + slot];
#pragma unroll
  for (int s = 0; s < F / 4; ++s) w2f[s] = a.w2[(size_t)(16 * wave + col) * F + 4 * s + slot];
  float b1v[4];
#pragma unroll
  for (int ft = 0; ft < 4; ++ft) b1v[ft] = a.b1[64 * wave + 16 * ft + col];
  const float b2v = a.b2[16 * wave + col];

  // x1 tile staging: thread tid moves floats [8 tid, 8 tid + 8) of the 32 x 64 tile (row tid / 8)
  const int sr = tid >> 3, sc = (tid & 7) * 8;
  f32x4 xv0 = {0, 0, 0, 0}, xv1 = {0, 0, 0, 0};
  if (blockIdx.x < ntile) {
    const float* src = a.x + ((size_t)blockIdx.x * TT + sr) * E + sc;
    xv0 = *(const f32x4*)src; xv1 = *(const f32x4*)(src + 4);
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    *(f32x4*)(xl + sr * XS + sc) = xv0;
    *(f32x4*)(xl + sr * XS + sc + 4) = xv1;
    const int b = tile / (S / TT), t0 = (tile % (S / TT)) * TT;   // frame, first token of the tile
    if (a.h0_dst && t0 == 0 && tid < 32) {
      const size_t row = a.slots ? (size_t)a.slots[b] : (size_t)b;
      *(f32x4*)(a.h0_dst + (size_t)b * 128 + 4 * tid) = *(const f32x4*)(a.h0_src + row * 128 + 4 * tid);
    }
    __syncthreads();
    const int nxt = tile + gridDim.x;
    if (nxt < ntile) {   // prefetch: consumed at the top of the next iteration
      const float* src = a.x + ((size_t)nxt * TT + sr) * E + sc;
      xv0 = *(const f32x4*)src; xv1 = *(const f32x4*)(src + 4);
    }

    // fc1 + ReLU
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) acc[m][ft] = (f32x4){b1v[ft], b1v[ft], b1v[ft], b1v[ft]};
#pragma unroll
      for (int s = 0; s < E / 4; ++s) {
        const float a0 = xl[col * XS + 4 * s + slot], a1 = xl[(16 + col) * XS + 4 * s + slot];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          acc[0][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w1f[ft][s], acc[0][ft], 0, 0, 0);
          acc[1][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w1f[ft][s], acc[1][ft], 0, 0, 0);
        }
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
      f32x4 acc0 = {b2v, b2v, b2v, b2v}, acc1 = acc0;
#pragma unroll
      for (int s = 0; s < F / 4; ++s) {
        const float a0 = hl[col * HS + 4 * s + slot], a1 = hl[(16 + col) * HS + 4 * s + slot];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w2f[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w2f[s], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ol[(4 * slot + r) * XS + 16 * wave + col] = acc0[r];
        ol[(16 + 4 * slot + r) * XS + 16 * wave + col] = acc1[r];
      }
    }
    __syncthreads();

    // finish: token tid / 4, channels 16 * (tid & 3) ..
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
