// ita_tokenizer_kernel.h -- the tokenizer: OverlapPatchMerging (reference models/ITA/QAT/layers.py:39-45), conv7x7/s2 +
// bilinear 30x45 -> 8x16 resize + LayerNorm, from (B,60,90) frames to (B,128,E) tokens.
//
// The conv and the resize are both linear, so the 7x7 patch is blended first and convolved once per token.  Wave w =
// token row w of the 8 x 16 grid; it needs image rows 2*y0-3 .. 2*y0+5 only (y0 = source row of the resize): a private
// 9 x 96 window in LDS with a zero border.  Lane (qi, kq) blends taps 4s+kq (s = 0..12) of token qi -- exactly the B
// operand (column = token, k = kq) of the conv's MFMA, whose A operand is a weight fragment image built at load time
// (ita_weights_load.h).  C = lane (token qi, channels (E/4)kq + 4ct + i): the layout the encoder keeps x in
// (ita_device.h: layernorm_q16).  No patch, no pre-LayerNorm token ever reaches LDS.
//
// Two users.  ita_stream_kernel<64, true, 1, ...> (ita_stream_kernel.h) runs the u8 form between the phases of the encoder
// layer, from the functions below; ita_tok_stream_kernel<E, U8> at the end of this file is the tokenizer on its own.  Both
// call the same window and conv functions on the same tables, so their tokens are the same bits.
#pragma once
#include "ita_device.h"

// ---- the conv7x7 of the u8 tokenizer as int8 MFMA (oracle/ita_oracle.c: ita_oracle_tokenizer_u8).  The blended tap is the
// exact integer B256 = 256 a1 + a0 <= 65280, the conv weight of a channel 23-bit fixed point Wq = 65536 w2 + 256 w1 + w0 with
// balanced digits, and the 49-tap sum splits into byte products that int8 MFMAs accumulate exactly:
//     S0 = sum a0 w0,  S1 = sum (a0 w1 + a1 w0),  S2 = sum (a0 w2 + a1 w1),  S3 = sum a1 w2,   L = S0 + 256 S1,  H = S2 + 256 S3
//     pre = fma((float)H, 65536 s, fma((float)L, s, bias))
// The unsigned bytes a0, a1 ride the signed MFMA as a ^ 0x80 = a - 128; the 128 * sum(w) terms sit in the accumulators'
// initial values (I0 for S0 -- it also carries 256 x the term of S1 --, I2 for S2 / S3).  K = 64 slots of the 16x16x64 MFMA:
// lane (token qi, k-group kq) holds its own 13 taps 4 j + kq in bytes j = 0..12 of its B fragment (the weight image has
// the same slot -> tap mapping, zero weights in the three pad slots).  Six MFMAs per 16-channel tile instead of thirteen
// v_mfma_f32_16x16x4_f32, which run at the f32 vector rate and hold the SIMD's VALU meanwhile (-5 us per 1024-frame launch).
template <int E>
struct ItaTokTab {
  static constexpr int NCT = E / 16;
  static constexpr int TW = 0;                          // int8 [NCT][3 byte planes][64 lanes][16]: A fragments, row rho <-> channel (E/4)(rho>>2) + 4 ct + (rho&3)
  static constexpr int TI = TW + NCT * 3 * 1024;        // int32 [2][E]: I0 | I2
  static constexpr int TS = TI + 2 * E * 4;             // f32 [3][E]: s | 65536 s | conv bias
  static constexpr int BYTES = TS + 3 * E * 4;
};
// thirteen blended taps (exact integers) -> the two B fragments (low bytes, high bytes; both ^ 0x80)
__device__ __forceinline__ void tok_u8_fragments(const unsigned (&pb)[13], i32x4& a0, i32x4& a1) {
  unsigned p16[8];
#pragma unroll
  for (int k = 0; k < 6; ++k) p16[k] = __builtin_amdgcn_perm(pb[2 * k + 1], pb[2 * k], 0x05040100u) ^ 0x80808080u;
  p16[6] = (pb[12] & 0xffffu) ^ 0x80808080u;
  p16[7] = 0;                                           // pad slots: their weights are zero
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    a0[d] = (int)__builtin_amdgcn_perm(p16[2 * d + 1], p16[2 * d], 0x06040200u);
    a1[d] = (int)__builtin_amdgcn_perm(p16[2 * d + 1], p16[2 * d], 0x07050301u);
  }
}
// one 16-channel tile: out[i] = pre-LayerNorm conv output of channel (E/4) kq + 4 ct + i of this lane's token
template <int E>
__device__ __forceinline__ void tok_u8_tile(const char* tab, int ct, int lane, int kq, const i32x4& a0, const i32x4& a1, float (&out)[4]) {
  using T = ItaTokTab<E>;
  const int c0 = (E / 4) * kq + 4 * ct;
  // (one weight fragment live at a time, the sums combined in place: the tile runs where the encoder kernel has no register to spare)
  const i32x4 z = {0, 0, 0, 0};
  i32x4 s0 = *(const i32x4*)(tab + T::TI + c0 * 4), s1, s2 = *(const i32x4*)(tab + T::TI + (E + c0) * 4), s3;
  {
    const i32x4 w0 = *(const i32x4*)(tab + T::TW + ((ct * 3 + 0) * 64 + lane) * 16);
    s0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, a0, s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, a1, z, 0, 0, 0);
  }
  {
    const i32x4 w1 = *(const i32x4*)(tab + T::TW + ((ct * 3 + 1) * 64 + lane) * 16);
    s2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, a1, s2, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, a0, s1, 0, 0, 0);
  }
  {
    const i32x4 w2 = *(const i32x4*)(tab + T::TW + ((ct * 3 + 2) * 64 + lane) * 16);
    s3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w2, a1, z, 0, 0, 0);
    s2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(w2, a0, s2, 0, 0, 0);
  }
  float lf[4], hf[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { lf[i] = (float)(s0[i] + (s1[i] << 8)); hf[i] = (float)(s2[i] + (s3[i] << 8)); }
  {
    const f32x4 sc = *(const f32x4*)(tab + T::TS + c0 * 4), cb = *(const f32x4*)(tab + T::TS + (2 * E + c0) * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) lf[i] = fmaf(lf[i], sc[i], cb[i]);
  }
  {
    const f32x4 sc16 = *(const f32x4*)(tab + T::TS + (E + c0) * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = fmaf(hf[i], sc16[i], lf[i]);
  }
}

// ---- the u8 pixel window of wave `wave` (same arithmetic and operation order as the oracle's ita_oracle_tokenizer_u8):
//   fetch : five dwords per lane of a frame (issued a phase early by the callers, consumed by fill)
//   fill  : funnel-shift to the window's 16-byte pieces, mask the border, one ds_write_b128 per lane
//   blend : this lane's 13 taps of its token as exact integers, packed into the two B fragments of the int8 conv
// `ol` is the lane id.  Every per-lane value is derived from it inside each call and nothing is kept between calls: the
// encoder kernel passes an OPAQUE copy taken once per frame, otherwise the compiler hoists ~60 registers of loop-invariant
// geometry and LDS addresses out of its frame loop and the kernel (which lives at the 256-register limit of two waves per
// SIMD) spills.  The stand-alone kernel passes the plain lane id and gets the hoisting.
constexpr int ITA_TOK_U8_WIN = 9 * 96;   // bytes of one wave's u8 window
struct ItaTokGeo { int y0, x0, rr, pc, row, o; float h1, w1; };
__device__ __forceinline__ ItaTokGeo tok_u8_geo(int wave, int ol) {
  ItaTokGeo g;
  int yp, xp;
  bilinear_src_dev(wave, 30.0f / 8.0f, 30, g.y0, yp, g.h1);        // y0 <= 27 < 29 and x0 <= 43 < 44: the second
  bilinear_src_dev(ol & 15, 45.0f / 16.0f, 45, g.x0, xp, g.w1);    // neighbour is always one row / column on
  g.rr = ol / 6; g.pc = ol - 6 * g.rr;                             // window piece of this lane (lane < 54)
  g.row = 2 * g.y0 - 3 + g.rr;                                     // image row (-1 for the top row of wave 0)
  g.o = g.row * 90 + 16 * g.pc - 3;                                // frame byte of the piece's first window byte
  return g;
}
__device__ __forceinline__ void tok_u8_fetch(const void* img, int fb, int wave, int ol, unsigned (&d)[5]) {
  const ItaTokGeo g = tok_u8_geo(wave, ol);
  const uint8_t* src = (const uint8_t*)img + (size_t)fb * 5400;
  const int a0 = g.o & ~3;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int aj = a0 + 4 * j;
    d[j] = 0;
    if (ol < 54 && g.row >= 0 && aj >= 0 && aj < 5400) d[j] = *(const unsigned*)(src + aj);
  }
}
// wins: the eight waves' windows in LDS.  (fill and blend form this wave's window address themselves, next to its use: formed
// by the caller it is hoisted above the lane-mask branch and the encoder kernel's schedule changes throughout)
__device__ __forceinline__ void tok_u8_fill(char* wins, int wave, int ol, const unsigned (&d)[5]) {
  const ItaTokGeo g = tok_u8_geo(wave, ol);
  const int sh = g.o & 3;
  unsigned o4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o4[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh);
  if (g.pc == 0) o4[0] &= 0xff000000u;        // window columns 0..2  = image columns -3..-1
  if (g.pc == 5) o4[3] &= 0x000000ffu;        // window columns 93..95 = image columns 90..92
  if (ol < 54)
    *(i32x4*)(wins + wave * ITA_TOK_U8_WIN + g.rr * 96 + 16 * g.pc) = (i32x4){(int)o4[0], (int)o4[1], (int)o4[2], (int)o4[3]};
}
// tap: int32 [52], window offset ky * 96 + kx of tap t (0 for the pad taps 49..51: their weights are 0).  Waits for the
// wave's own window stores first.
__device__ __forceinline__ void tok_u8_blend(const char* wins, const int* tap, int wave, int ol, i32x4& a0, i32x4& a1) {
  const ItaTokGeo g = tok_u8_geo(wave, ol);
  const int kq = ol >> 4;
  const uint8_t* win = (const uint8_t*)(wins + wave * ITA_TOK_U8_WIN) + 2 * g.x0;
  // The weights of this fixed resize are dyadic, h = H / 8 and w = W / 32 with 0 < H1 < 8, 0 < W1 < 32 for every
  // token, so the blend of a tap is the exact integer  256 * 255 * value = H0 W0 a + H0 W1 b + H1 W0 c + H1 W1 d
  // on the pixel CODES (each product weight <= 7 * 31 fits a byte); 1 / 65280 is folded into the conv scales
  // (oracle/ita_oracle.c ita_oracle_tokenizer_u8).  No k / 255 table, no float blend.
  const unsigned H1 = (unsigned)(8.0f * g.h1) & 7u, W1 = (unsigned)(32.0f * g.w1) & 31u, H0 = 8u - H1, W0 = 32u - W1;
  const unsigned w00 = (H0 * W0) & 255u, w01 = (H0 * W1) & 255u, w10 = (H1 * W0) & 255u, w11 = (H1 * W1) & 255u;
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the window is private to this wave
  __builtin_amdgcn_wave_barrier();
  unsigned pb[13];
#pragma unroll
  for (int s = 0; s < 13; ++s) {
    if constexpr (ITA_ABLATE & 512) { pb[s] = w00 * s; continue; }
    const int off = tap[4 * s + kq];
    pb[s] = (unsigned)win[off] * w00 + (unsigned)win[off + 2] * w01 + (unsigned)win[off + 192] * w10 +
            (unsigned)win[off + 194] * w11;
  }
  tok_u8_fragments(pb, a0, a1);
}

// ------------------------------------------------------------------ the tokenizer on its own
// For the cases the fused form does not cover: E = 128 (its encoder kernel has no LDS left for the 27 KB of conv
// fragments), f32 frames (module.main_graph's own input type: four times the window bytes) and callers of ita_tokenizer.
// One persistent 512-thread workgroup per CU, the next frame's pixels requested a frame ahead.
//   U8  : the window and conv functions above;
//   !U8 : the oracle's float blend  h0 (w0 a + w1 b) + h1 (w0 c + w1 d)  of pixels already scaled by the caller
//         (ita_oracle_tokenizer), conv weights as they are, v_mfma_f32_16x16x4_f32 (on gfx950 an exact ascending-k fmaf
//         chain); same results as ita_oracle_tokenizer bit for bit (same operation order).
template <int E, bool U8>
struct ItaTokStreamLds {
  static constexpr int NCT = E / 16;                           // 16-channel output tiles
  static constexpr int LNP = 0;                                // f32: ln_w | ln_b
  static constexpr int CW = LNP + 2 * E * 4;                   // !U8: f32 [13][NCT][64] conv weights as A fragments; U8: ItaTokTab<E>
  static constexpr int CB = CW + (U8 ? ItaTokTab<E>::BYTES : 13 * NCT * 64 * 4);   // !U8: f32 [E] conv bias (U8: inside the table)
  static constexpr int TAP = CB + (U8 ? 0 : E * 4);            // int32 [52]
  static constexpr int IMAGE = TAP + 52 * 4;
  static constexpr int IMG = (IMAGE + 15) & ~15;               // [8 waves][9][96] pixels (u8 or f32), 3 zero columns each side
  static constexpr int IMG_WAVE = ITA_TOK_U8_WIN * (U8 ? 1 : 4);
  static constexpr int TOTAL = IMG + 8 * IMG_WAVE;
};
struct ItaTokStreamArgs {
  const char* image;     // device copy of the LDS image (ItaTokStreamLds<E, U8>::IMAGE bytes)
  const void* img;       // (B,60,90) u8 or f32
  float* tokens;         // (B,128,E)
  int B;
};
template <int E, bool U8>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void ita_tok_stream_kernel(const ItaTokStreamArgs a) {
  using L = ItaTokStreamLds<E, U8>;
  constexpr int S = 128, EC = E / 4, NCT = L::NCT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* lnp = (const float*)(lds + L::LNP);
  const int kq = lane >> 4, qi = lane & 15;   // this lane's token (row = wave, column = qi) and channel quarter
  // f32 frames: the resize's source row / column and weights of the token; window element e = lane + 64 j (j < 14) =
  // (window row e / 96, window column e % 96)
  int y0, yp, x0, xp;
  float h1, w1;
  bilinear_src_dev(wave, 30.0f / 8.0f, 30, y0, yp, h1);
  bilinear_src_dev(lane & 15, 45.0f / 16.0f, 45, x0, xp, w1);
  constexpr int NF = U8 ? 1 : 14;
  unsigned tk_d[5] = {0, 0, 0, 0, 0};
  float tk_f[NF];
  auto fetch = [&](int fb) {
    if constexpr (U8) {
      tok_u8_fetch(a.img, fb, wave, lane, tk_d);
    } else {
      const float* src = (const float*)a.img + (size_t)fb * 5400;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int e = lane + 64 * j, wr = e / 96, wc = e - 96 * wr;
        const int iy = 2 * y0 - 3 + wr, ix = wc - 3;
        tk_f[j] = 0.0f;
        if (e < 9 * 96 && iy >= 0 && iy < 60 && ix >= 0 && ix < 90) tk_f[j] = src[iy * 90 + ix];
      }
    }
  };
  if ((int)blockIdx.x < a.B) fetch(blockIdx.x);
  for (int p = tid; p < L::IMAGE / 16; p += 512) *(i32x4*)(lds + p * 16) = *(const i32x4*)(a.image + (size_t)p * 16);
  __syncthreads();
  const float fh0 = 1.0f - h1, fw0 = 1.0f - w1;
  char* wbase = lds + L::IMG + wave * L::IMG_WAVE;
  const int* tap = (const int*)(lds + L::TAP);
  const float* cw = (const float*)(lds + L::CW);
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    if constexpr (U8) {
      tok_u8_fill(lds + L::IMG, wave, lane, tk_d);
    } else {
#pragma unroll
      for (int j = 0; j < NF; ++j)
        if (lane + 64 * j < 9 * 96) ((float*)wbase)[lane + 64 * j] = tk_f[j];
    }
    if (b + (int)gridDim.x < a.B) fetch(b + gridDim.x);
    float xr[EC];
    if constexpr (U8) {
      i32x4 a0, a1;
      tok_u8_blend(lds + L::IMG, tap, wave, lane, a0, a1);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        float o4[4];
        tok_u8_tile<E>(lds + L::CW, ct, lane, kq, a0, a1, o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[4 * ct + i] = o4[i];
      }
    } else {
      __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the window is private to this wave
      __builtin_amdgcn_wave_barrier();
      float tk_pt[13];
#pragma unroll
      for (int s = 0; s < 13; ++s) {
        const int off = tap[4 * s + kq];
        const float* win = (const float*)wbase + 2 * x0;
        const float va = win[off], vb = win[off + 2], vc = win[off + 192], vd = win[off + 194];
        tk_pt[s] = fh0 * (fw0 * va + w1 * vb) + h1 * (fw0 * vc + w1 * vd);   // ita_oracle_blend_patch's expression
      }
      f32x4 acc[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ct] = *(const f32x4*)(lds + L::CB + (EC * kq + 4 * ct) * 4);
#pragma unroll
      for (int s = 0; s < 13; ++s)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
          acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cw[(s * NCT + ct) * 64 + lane], tk_pt[s], acc[ct], 0, 0, 0);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[4 * ct + i] = acc[ct][i];
    }
    layernorm_q16<E>(xr, lnp, lnp + E, EC * kq);
    // 64 contiguous bytes per token and store; the encoder launch behind this one reads them: write-through
    st_tok_quarter_next<E>(ita_rsrc(a.tokens + (size_t)b * S * E), wave * 16 + qi, kq, xr);
    __builtin_amdgcn_wave_barrier();      // the window is rewritten for the next frame only after these reads were issued
  }
}
