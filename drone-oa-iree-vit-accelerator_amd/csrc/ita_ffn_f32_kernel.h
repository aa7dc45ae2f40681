// ita_ffn_f32_kernel.h -- the float32 FFN of the attention-only QAT graph and of the float graph on gfx950 f32 MFMA,
// E = 64 and 128.
//
//   ita_ffn_f32_kernel<E> : ITAFeedForward.forward (models/ITA/layers.py:29-45: fc1 E -> 256, ReLU, fc2 256 -> E)
//                           + optional residual + LayerNorm2 (QAT_only_attn/model.py:76-88; E = 128:
//                           models/ITA_upsample_shuffle/model.py:97-103), all float32:
//                           y = LayerNorm2(x1 + fc2(relu(fc1(x1) + b1)) + b2)
//
// Numerics: bit-identical to the oracle composition add_ln(x1, linear_f32(max(linear_f32(x1, W1, b1), 0), W2, b2)).
// ita_oracle_linear_f32 is one fmaf chain per output, started from the bias, in ascending k; v_mfma_f32_16x16x4_f32
// computes exactly that chain in k-slot order, so C starts as the bias and the K steps are issued in ascending order
// with k = 4 * step + slot.  The hidden layer goes through an LDS tile in natural [token][feature] order, so fc2's A
// fragments come in ascending k as well (the int8 FFN's register hand-over permutes k, which an f32 chain would notice).
//
// One 256-thread workgroup (4 waves, one per SIMD) walks 32-token tiles (a quarter frame) with a grid stride; two
// workgroups per CU (E = 64: 242 VGPRs; E = 128: 66 KB of LDS).
// At E = 64 the weights stay in registers as MFMA B fragments for the whole launch: wave w holds W1 rows 64w..64w+63
// (64 VGPRs) and W2 rows 16w..16w+15 (64 VGPRs).  At E = 128 they are 256 KB, 256 VGPRs per lane over 4 waves, so they
// stream from L1 / L2 as MFMA B fragments instead, from a fragment image made at load (ita_ffn_f32_frag_image): one f32x4
// per lane carries the lane's operand for four consecutive k-steps, and each f32x4 feeds 8 MFMAs (4 k-steps x the
// tile's two 16-token halves).  Per tile (XS = E + 4):
//   x1 tile -> LDS [32][XS] (the next tile is prefetched into registers meanwhile)
//   fc1 + ReLU: wave w, features 64w..64w+63 x both 16-token halves, 8 accumulators of E / 4 steps -> h LDS [32][260]
//   fc2: wave w, outputs (E/4)w..(E/4)w+E/4-1 x both halves, 2 x E / 64 accumulators of 64 steps -> LDS [32][XS]
//   finish: 4 threads per token: + x1, layernorm_lanes (the int8 kernels' bit-exact LayerNorm), y / f16 planes
// Row strides of 68 / 132 and 260 floats put the 16 rows x 4 k-slots of a fragment read, and the 4 rows x 16 columns of
// an accumulator store, on 64 distinct banks.
//
// Roofline, E = 64: 2 x 128 x 64 x 256 MAC = 8.39 MFLOP per frame; f32 MFMA peak 157.3 TF -> >= 53 us per 1024 frames.
// HBM: 2 x 32 KB per frame (x1 in, y out) -> 13 us per 1024 frames at 5 TB/s: compute bound.
// E = 128: 2 x 128 x 128 x 256 MAC = 16.8 MFLOP per frame -> >= 109 us per 1024 frames; HBM 2 x 64 KB per frame -> 27 us.
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

template <int E>
struct ItaFfnF32Lds {
  static constexpr int TT = 32, F = 256, XS = E + 4, HS = F + 4;
  static constexpr int X = 0;                     // f32 [TT][XS]  x1 tile
  static constexpr int H = X + TT * XS * 4;       // f32 [TT][HS]  relu(fc1)
  static constexpr int O = H + TT * HS * 4;       // f32 [TT][XS]  fc2 output
  static constexpr int TOTAL = O + TT * XS * 4;   // 50688 bytes (E = 64), 67072 bytes (E = 128)
};

// B-fragment image of a row-major [R][K] matrix W (R, K multiples of 16), as ita_ffn_f32_kernel<128> reads it:
// f32x4 [R/16][K/16][64], lane (col, slot) of (row tile rt, k group g) holds W[16 rt + col][16 g + 4 r + slot], r = 0..3
// (its B operand for k-steps 4 g .. 4 g + 3)
inline void ita_ffn_f32_frag_image(const float* w, int R, int K, float* img) {
  for (int rt = 0; rt < R / 16; ++rt)
    for (int g = 0; g < K / 16; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r)
          img[(((size_t)rt * (K / 16) + g) * 64 + lane) * 4 + r] = w[(size_t)(16 * rt + (lane & 15)) * K + 16 * g + 4 * r + (lane >> 4)];
}

// E = 64: a.w1 / a.w2 are the matrices W1 [256][64] and W2 [64][256]; E = 128: their fragment images
// (ita_ffn_f32_frag_image of W1 [256][128] and W2 [128][256]), not the matrices
template <int E>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ita_ffn_f32_kernel(const ItaFfnF32Args a) {
  using L = ItaFfnF32Lds<E>;
  constexpr int TT = L::TT, F = L::F, XS = L::XS, HS = L::HS, S = 128, EC = E / 4;
  constexpr bool W_RESIDENT = E == 64;   // weights in registers for the whole launch, else streamed fragment images
  constexpr int NO = E / 64;             // 16-output tiles of fc2 per wave
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* xl = (float*)(lds + L::X);
  float* hl = (float*)(lds + L::H);
  float* ol = (float*)(lds + L::O);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;   // B fragment: row (feature) col, k = 4 * step + slot
  const int ntile = a.B * (S / TT);

  // weights as B fragments: resident for the whole launch, or the wave's row tiles of the fragment images
  float w1f[4][E / 4], w2f[F / 4];
  const f32x4* w1p = (const f32x4*)a.w1 + (size_t)4 * wave * (E / 16) * 64 + lane;    // row tiles 4w .. 4w + 3
  const f32x4* w2p = (const f32x4*)a.w2 + (size_t)NO * wave * (F / 16) * 64 + lane;   // row tiles NO w .. NO w + NO - 1
  if constexpr (W_RESIDENT) {
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int s = 0; s < E / 4; ++s) w1f[ft][s] = a.w1[(size_t)(64 * wave + 16 * ft + col) * E + 4 * s + slot];
#pragma unroll
    for (int s = 0; s < F / 4; ++s) w2f[s] = a.w2[(size_t)(16 * wave + col) * F + 4 * s + slot];
  }
  float b1v[4], b2v[NO];
#pragma unroll
  for (int ft = 0; ft < 4; ++ft) b1v[ft] = a.b1[64 * wave + 16 * ft + col];
  if constexpr (NO == 1) {   // not as a one-trip loop: that reorders the address arithmetic of the E = 64 prologue
    b2v[0] = a.b2[EC * wave + col];
  } else {
#pragma unroll
    for (int et = 0; et < NO; ++et) b2v[et] = a.b2[EC * wave + 16 * et + col];
  }

  // x1 tile staging: thread tid moves floats [E / 8 tid, +E / 8) of the 32 x E tile (row tid / 8)
  constexpr int NX = E / 32;
  const int sr = tid >> 3, sc = (tid & 7) * (E / 8);
  struct { f32x4 v[NX]; } xv = {};   // in a struct: a bare f32x4[2] is merged into one 8-float value before the loops
                                     // unroll, and the E = 64 kernel's register allocation changes
  if (blockIdx.x < ntile) {
    const float* src = a.x + ((size_t)blockIdx.x * TT + sr) * E + sc;
#pragma unroll
    for (int i = 0; i < NX; ++i) xv.v[i] = *(const f32x4*)(src + 4 * i);
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < NX; ++i) *(f32x4*)(xl + sr * XS + sc + 4 * i) = xv.v[i];
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
      for (int i = 0; i < NX; ++i) xv.v[i] = *(const f32x4*)(src + 4 * i);
    }

    // fc1 + ReLU
    {
      f32x4 acc[2][4];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) acc[m][ft] = (f32x4){b1v[ft], b1v[ft], b1v[ft], b1v[ft]};
      if constexpr (W_RESIDENT) {
#pragma unroll
        for (int s = 0; s < E / 4; ++s) {
          const float a0 = xl[col * XS + 4 * s + slot], a1 = xl[(16 + col) * XS + 4 * s + slot];
#pragma unroll
          for (int ft = 0; ft < 4; ++ft) {
            acc[0][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w1f[ft][s], acc[0][ft], 0, 0, 0);
            acc[1][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, w1f[ft][s], acc[1][ft], 0, 0, 0);
          }
        }
      } else {
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

    // fc2 (each form with its own accumulators and output store: one store nest over [2][NO] accumulators moves one of
    // the two kernels off its register allocation, E = 64 from 242 to 236 VGPRs in the streamed form's loop order,
    // E = 128 from 160 to 166 in the resident form's)
    if constexpr (W_RESIDENT) {
      f32x4 acc0 = {b2v[0], b2v[0], b2v[0], b2v[0]}, acc1 = acc0;
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
    } else {
      f32x4 acc[2][NO];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int et = 0; et < NO; ++et) acc[m][et] = (f32x4){b2v[et], b2v[et], b2v[et], b2v[et]};
      f32x4 wb[NO];
#pragma unroll
      for (int et = 0; et < NO; ++et) wb[et] = w2p[(size_t)et * (F / 16) * 64];
#pragma unroll 1
      for (int g = 0; g < F / 16; ++g) {
        const int gn = g + 1 < F / 16 ? g + 1 : g;
        f32x4 wn[NO];
#pragma unroll
        for (int et = 0; et < NO; ++et) wn[et] = w2p[((size_t)et * (F / 16) + gn) * 64];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = 4 * g + r;
          const float a0 = hl[col * HS + 4 * s + slot], a1 = hl[(16 + col) * HS + 4 * s + slot];
#pragma unroll
          for (int et = 0; et < NO; ++et) {
            acc[0][et] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, wb[et][r], acc[0][et], 0, 0, 0);
            acc[1][et] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, wb[et][r], acc[1][et], 0, 0, 0);
          }
        }
#pragma unroll
        for (int et = 0; et < NO; ++et) wb[et] = wn[et];
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int et = 0; et < NO; ++et)
#pragma unroll
          for (int r = 0; r < 4; ++r) ol[(16 * m + 4 * slot + r) * XS + EC * wave + 16 * et + col] = acc[m][et][r];
    }
    __syncthreads();

    // finish: token tid / 4, channels E / 4 * (tid & 3) ..
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
      const size_t po = (size_t)b * a.ld_planes + (size_t)(t0 + tok) * E + qtr * EC;
      store_row_planes(r, a.y ? a.y + ((size_t)tile * TT + tok) * E + qtr * EC : nullptr, a.y_hi ? a.y_hi + po : nullptr,
                       a.y_hi ? a.y_lo + po : nullptr);
    }
    __syncthreads();   // the next tile overwrites the x1 and output tiles
  }
}
