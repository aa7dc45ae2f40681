// ita_tokenizer_long_kernel.h -- the tokenizer of the long-sequence path: OverlapPatchMerging (reference
// models/ITA/QAT/layers.py:39-45) for any frame size and any token grid, conv7x7/s2/p3 + bilinear (CH x CW -> tok_h x tok_w,
// align_corners = False) + LayerNorm, from strided camera frames (u8 / u16 / f32, height x width) to (B, tok_h * tok_w, E)
// f32 token rows.  Definition: tokenizer_long_ref.py; the kernel equals it bit for bit.
//
// It is the f32 branch of ita_tok_stream_kernel (ita_tokenizer_kernel.h) with the geometry as arguments: the conv and the
// resize are both linear, so the four bilinear neighbours are blended on the 7 x 7 INPUT patches first (the conv map, 44 MB
// per 480 x 720 frame at E = 128, never exists) and one 49-step chain per token and channel follows.  Same LDS image of
// the weights (ItaTokStreamLds<E, false>: LayerNorm parameters, conv weights as v_mfma_f32_16x16x4_f32 A fragments, bias),
// same MFMA chain (on gfx950 an exact ascending-k fmaf chain), same layernorm_q16 and st_tok_quarter: at 60 x 90 -> 8 x 16 on
// f32 frames the tokens are those of ita_tok_stream_kernel<E, false>.
//
// One wave owns 16 consecutive tokens of one token row (tok_w % 16 == 0); lane (qi, kq) blends taps 4 s + kq (s = 0..12) of
// token qi -- the B operand (column = token, k = kq) of the conv's MFMA.  Work item = (frame, 16-token tile), eight
// consecutive items per persistent workgroup and round.
//
// Where the pixels come from, two forms of the one kernel, chosen per launch by the host from the geometry:
//   WIN     every 16-token tile of the grid needs at most 128 pixel columns (horizontal ratio up to about 3.8: config 5 has
//           2.8).  The wave copies the tile's 9 rows x 128 columns into a private LDS window -- 18 coalesced single-pixel
//           loads a lane, already valued and zero-padded -- and reads its 52 pixels from there.
//   direct  anything wider (at ratios above about 4.5 the patches of neighbouring tokens do not even overlap; a tile of a
//           4096-wide frame spans 3.9 k columns): four single-pixel loads per tap and lane, 52 a lane, served by L1 / L2.
//           So the window bounds no frame width.
// Measured at config 5 the direct form takes the same time at E = 64 and E = 128 -- the scattered loads set it, not the MFMAs
// or the token stores -- which is why the window exists ("Long tokenizer").
// Every load is clamped into the frame and a select puts the zero padding in: nothing outside [base, base + (height-1) *
// row_stride + width) of a frame is touched, at any alignment of base, and no lane branches around a load.
#pragma once
#include "ita_ingest_kernel.h"
#include "ita_tokenizer_kernel.h"

constexpr int ITA_TOK_LONG_WIN_W = 128;                 // columns of a wave's pixel window
constexpr int ITA_TOK_LONG_WIN_FLOATS = 9 * ITA_TOK_LONG_WIN_W;
template <int E, bool WIN>
struct ItaTokLongLds {
  static constexpr int IMAGE = ItaTokStreamLds<E, false>::IMAGE;   // copied as it stands (its tap table is not used here)
  static constexpr int LUT = (IMAGE + 15) & ~15;                   // f32 [256]: code / 255.0f (ita_ingest_u8_lut)
  static constexpr int WINS = LUT + ITA_INGEST_LUT_BYTES;          // WIN: f32 [8 waves][9][128] pixel values, zero outside the frame
  static constexpr int TOTAL = WINS + (WIN ? 8 * ITA_TOK_LONG_WIN_FLOATS * 4 : 0);
};
struct ItaTokLongArgs {
  const char* image;            // device copy of the LDS image (ItaTokStreamLds<E, false>::IMAGE bytes)
  const void* src;              // frames, strides in pixels
  float* tokens;                // (B, tok_h * tok_w, E)
  long long row_stride, frame_stride;
  float scale_y, scale_x;       // f32(CH) / f32(tok_h), f32(CW) / f32(tok_w): host IEEE divisions
  float depth_scale;
  int H, W, CH, CW;             // frame size; conv grid (H - 1) / 2 + 1, (W - 1) / 2 + 1
  int tok_h, tok_w, B;
};

// the oracle's expression (ita_oracle_blend_patch), every operation rounded on its own
__device__ __forceinline__ float ita_tok_long_blend(float h0, float h1, float w0, float w1, float a, float b, float c, float d) {
#pragma clang fp contract(off)
  return h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d);
}

template <int E, typename T, bool WIN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void ita_tok_long_kernel(const ItaTokLongArgs a) {
  using L = ItaTokLongLds<E, WIN>;
  using LS = ItaTokStreamLds<E, false>;
  constexpr int EC = E / 4, NCT = E / 16;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int p = tid; p < L::IMAGE / 16; p += 512) *(i32x4*)(lds + p * 16) = *(const i32x4*)(a.image + (size_t)p * 16);
  if (tid < 256) ((float*)(lds + L::LUT))[tid] = ita_ingest_u8_lut.v[tid];
  __syncthreads();
  const float* lnp = (const float*)(lds + LS::LNP);
  const float* cw = (const float*)(lds + LS::CW);
  const float* lut = (const float*)(lds + L::LUT);
  const int kq = lane >> 4, qi = lane & 15;
  const int tiles_x = a.tok_w >> 4, tiles = a.tok_h * tiles_x;      // 16-token tiles of a token row, of a frame
  const long long items = (long long)a.B * tiles;                     // a multiple of 8: tok_h * tok_w % 128 == 0
  const T* src = (const T*)a.src;
  for (long long it = (long long)blockIdx.x * 8 + wave; it < items; it += (long long)gridDim.x * 8) {
    // Nothing in this loop writes LDS, so without this the compiler hoists the loop-invariant weight fragments (13 E / 16
    // registers) and LayerNorm parameters out of it and spills them: they are re-read from LDS for every tile instead.
    asm volatile("" ::: "memory");
    const long long frame = it / tiles;
    const int tile = (int)(it - frame * tiles), oy = tile / tiles_x, ox = (tile - oy * tiles_x) * 16 + qi;
    int y0, yp, x0, xp;
    float h1, w1;
    bilinear_src_dev(oy, a.scale_y, a.CH, y0, yp, h1);
    bilinear_src_dev(ox, a.scale_x, a.CW, x0, xp, w1);
    const float h0 = 1.0f - h1, w0 = 1.0f - w1;
    const T* f = src + frame * a.frame_stride;
    // pixel (iy, ix) of the frame as the definition values it, 0 outside the frame.  Branch-free, so that a lane's 52 loads
    // are in flight together: the load goes to the nearest pixel INSIDE the frame and a select drops what it brought.
    auto px = [&](int iy, int ix) -> float {
      const bool inside = (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
      const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
      const float v = ita_ingest_px(f[cy * a.row_stride + cx], lut, a.depth_scale);
      return inside ? v : 0.0f;
    };
    float pb[13];
    if constexpr (WIN) {
      // The tile's pixels -- rows 2 y0 - 3 .. + 8, columns from 2 x0 - 3 of its first token on, at most 128 of them (the host
      // chose this form because every tile of the grid fits) -- go to the wave's window with coalesced loads, 18 a lane
      // instead of 52 scattered ones; the taps are then read from LDS.
      float* win = (float*)(lds + L::WINS) + wave * ITA_TOK_LONG_WIN_FLOATS;
      int xf, xpf;
      float wf;
      bilinear_src_dev(ox - qi, a.scale_x, a.CW, xf, xpf, wf);
      const int ys = 2 * y0 - 3, xs = 2 * xf - 3;
      float v[18];
#pragma unroll
      for (int j = 0; j < 18; ++j) v[j] = px(ys + (j >> 1), xs + lane + 64 * (j & 1));
#pragma unroll
      for (int j = 0; j < 18; ++j) win[(j >> 1) * ITA_TOK_LONG_WIN_W + lane + 64 * (j & 1)] = v[j];
      __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the window is private to this wave
      __builtin_amdgcn_wave_barrier();
      const float* w00 = win + 2 * (x0 - xf);
#pragma unroll
      for (int s = 0; s < 13; ++s) {
        const int t = min(4 * s + kq, 48);
        const int ky = t / 7, kx = t - 7 * ky;
        const float* p = w00 + ky * ITA_TOK_LONG_WIN_W + kx;
        pb[s] = ita_tok_long_blend(h0, h1, w0, w1, p[0], p[2 * xp], p[2 * yp * ITA_TOK_LONG_WIN_W], p[2 * yp * ITA_TOK_LONG_WIN_W + 2 * xp]);
      }
      __builtin_amdgcn_wave_barrier();      // the window is rewritten for the next tile only after these reads were issued
    } else {
#pragma unroll
      for (int s = 0; s < 13; ++s) {
        const int t = min(4 * s + kq, 48);   // slots 49..51 of the K = 52 chain (s = 12, kq > 0) read tap 48's pixels ...
        const int ky = t / 7, kx = t - 7 * ky;
        const int iy = 2 * y0 - 3 + ky, ix = 2 * x0 - 3 + kx;
        pb[s] = ita_tok_long_blend(h0, h1, w0, w1, px(iy, ix), px(iy, ix + 2 * xp), px(iy + 2 * yp, ix), px(iy + 2 * yp, ix + 2 * xp));
      }
    }
    if (kq > 0) pb[12] = 0.0f;             // ... and are exactly zero whatever those pixels hold (an inf, a NaN)
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = *(const f32x4*)(lds + LS::CB + (EC * kq + 4 * ct) * 4);
#pragma unroll
    for (int s = 0; s < 13; ++s)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cw[(s * NCT + ct) * 64 + lane], pb[s], acc[ct], 0, 0, 0);
    float xr[EC];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) xr[4 * ct + i] = acc[ct][i];
    layernorm_q16<E>(xr, lnp, lnp + E, EC * kq);
    // token frame * tok_h * tok_w + oy * tok_w + ox = it * 16 + qi
    st_tok_quarter<E>(a.tokens + ((size_t)it * 16 + qi) * E, kq, xr);
  }
}
