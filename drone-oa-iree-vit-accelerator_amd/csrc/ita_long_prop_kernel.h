// ita_long_prop_kernel.h -- weighted column sums of the S x S probability matrix of the long int8 attention
// (ita_mha_long_int8_propagate):
//     out[b, r, j] = sum_i w[b, r, i] * p[b, i, j]        w int8 (B, R, S), 1 <= R <= 64; p uint8; out int32 (B, R, S)
// with p[b, i, j] the probability ita_long_attn_body gives query i for key j (ita_mha_long_int8_taps' probs).  The matrix
// is never held.  col_mass of the statistics entry is w = all ones, a probability row is w = one-hot.
//
// The entry runs four launches over the long workspace:
//   ita_long_proj_kernel<FAST, E, true>   unchanged: Q fragments and K images
//   ita_long_stats_kernel<FAST>           unchanged, row_max and row_sum only, into the workspace (sweeps 1 and 2 of every query)
//   ita_long_prop_prep_kernel             per query tile a 1 KB row-parameter image and the permuted weight images; 128 * row
//                                         sums of w (one workgroup per weight row: no atomics)
//   ita_long_prop_kernel<FAST>            the TRANSPOSED sweep 3
//
// ita_long_prop_kernel: grid (S / 128 key tiles, B), 512 threads.  Wave v owns keys 16 v .. 16 v + 15 of its key tile, their
// three K fragments are loaded once from the K image (the A and the B operand of mfma_i32_16x16x64_i8 take the same 16 bytes
// per lane: chunk 4 ks + kq of token qi).  The workgroup sweeps the query tiles.  A tile's 24 KB of Q fragments arrive by
// LDS-DMA into a two-slot ring in the K-image layout [12][128][16] -- the per-lane source address of the DMA does the gather,
// the LDS side stays lane-linear -- so ita_long_logits<FAST> (ita_long_attn_kernel.h) runs as it is, with keys and queries
// swapped: integer dot products commute, the accumulators and their requantisation are those of the attention kernel.  Lane
// (qi, kq) then holds for key qi the biased 16-bit logits of queries 16 j16 + 4 kq + 0..3, j16 = 0..7, applies each query's
// own m, cap and inv_hi (u16 vectors read from the row-parameter image in LDS; in the attention kernel they are wave constants)
// and packs p - 128 as sweep 3 of ita_long_attn_body does.  Those eight words are the B operand of a second int8 MFMA whose A
// operand is the weight tile: 16 rows per group, queries permuted inside each 64-block as the V^T image permutes keys (word
// t, byte i of lane (r, kq) = query 64 kb + 16 t + 4 kq + i).  Accumulators start from 128 * sum_i w; at the end acc[g][i]
// belongs to weight row 16 g + 4 kq + i and key qi.  One barrier per query tile, no atomics, no floating point behind the
// logits: the result is bit-reproducible by construction.  Vector stores only.
//
// Range.  Every partial sum is 128 * sum_i w + sum_{i < n} w (p - 128) with |sum w (p - 128)| and |128 sum w| each at most
// 128 * 128 * S: both fit int32 for any int8 weight at S <= 32768 (2^29 each), and at S = 65536 for weights in [-127, 127]
// (127 * 128 * 65536 < 2^30 each).  The weights are not scanned.
#pragma once
#include "ita_long_attn_kernel.h"

struct ItaLongPropPrepArgs {
  const int8_t* row_max;  // (B, S): ita_long_stats_kernel's, in the workspace
  const int* row_sum;     // (B, S)
  const int8_t* w;        // (B, n_w, S) weights, 4-byte aligned
  char* rowp;             // workspace (B, S/128, 1024): per four queries u16 m[4] | cap[4] | inv_hi[4] | 0[4]
  char* wimg;             // workspace (B, S/128, ng, 2, 64 lanes, 16 B): A fragments of the second MFMA, ng = ceil(n_w / 16)
  int* wsum;              // workspace (B, 64): 128 * sum_i w[b, r, i], 0 for r >= n_w
  int B, S, n_w;
};

struct ItaLongPropArgs {
  const char* qfrag;      // ita_long_proj_kernel's workspace: Q fragments (B, S/16, 3, 64 lanes, 16 B)
  const char* kimg;       //                                   K images (B, S/128, 24576)
  const char* rowp;       // ita_long_prop_prep_kernel's images
  const char* wimg;
  const int* wsum;
  float ml;
  int B, S, n_w;
  int* out;               // (B, n_w, S)
};

// 66 KB of LDS: two slots of Q image, weight fragments (8 KB at 64 rows) and row parameters: two workgroups per CU
struct ItaLongPropLds {
  static constexpr int KB = ItaLongLds::KB;
  static constexpr int Q = 0, W = KB, RP = KB + 8192;  // inside a slot
  static constexpr int SLOT = RP + 1024;
  static constexpr int TOTAL = 2 * SLOT;
  static_assert(2 * TOTAL <= 160 * 1024, "two workgroups per CU");
};

// Grid (S / 128 + 16 ng, B), 512 threads.  Workgroup x < S / 128: query tile x of frame b -- the row parameters of its 128
// queries from row_max and row_sum with ita_long_attn_body's expressions, and its weight fragments.  Workgroup S / 128 + r:
// 128 * the sum of weight row r.
__global__ __launch_bounds__(512) void ita_long_prop_prep_kernel(const ItaLongPropPrepArgs a) {
  __shared__ int red[8];
  const int tid = threadIdx.x, b = blockIdx.y, x = blockIdx.x;
  const int nqt = a.S / 128, ng = (a.n_w + 15) >> 4;
  if (x < nqt) {
    const size_t tile = (size_t)b * nqt + x;
    if (tid < 128) {
      const size_t row = (size_t)b * a.S + (size_t)x * 128 + tid;
      const int rm = a.row_max[row], sum = max(a.row_sum[row], 1);
      const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;
      unsigned short* p = (unsigned short*)(a.rowp + tile * 1024 + (tid >> 2) * 32) + (tid & 3);
      p[0] = (unsigned short)(rm + 32768);
      p[4] = (unsigned short)min(rm + 128, 15);
      p[8] = (unsigned short)inv_hi;
      p[12] = 0;
    }
    for (int u = tid; u < ng * 128; u += 512) {          // u = (2 g + kb) * 64 + lane
      const int g = u >> 7, kb = (u >> 6) & 1, lane = u & 63;
      const int r = 16 * g + (lane & 15), kq = lane >> 4;
      i32x4 v = {0, 0, 0, 0};
      if (r < a.n_w) {
        const int8_t* src = a.w + ((size_t)b * a.n_w + r) * a.S + (size_t)x * 128 + 64 * kb + 4 * kq;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = *(const int*)(src + 16 * t);
      }
      *(i32x4*)(a.wimg + (tile * ng * 128 + u) * 16) = v;
    }
  } else {
    const int r = x - nqt;
    int s = 0;
    if (r < a.n_w) {
      const int* src = (const int*)(a.w + ((size_t)b * a.n_w + r) * a.S);
      for (int i = tid; i < a.S / 4; i += 512) s = __builtin_amdgcn_sdot4(src[i], 0x01010101, s, false);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
#pragma unroll
      for (int v = 0; v < 8; ++v) tot += red[v];
      a.wsum[b * 64 + r] = tot * 128;
    }
  }
}

template <bool FAST>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void ita_long_prop_kernel(const ItaLongPropArgs a) {
  using L = ItaLongPropLds;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nqt = a.S / 128, kt = blockIdx.x, b = blockIdx.y;
  const int ng = (a.n_w + 15) >> 4;
  const size_t tile0 = (size_t)b * nqt;              // first tile index of this frame

  // one query tile into a ring slot by LDS-DMA.  Q: piece = 64 consecutive 16-byte units of the image [12][128][16], unit
  // c * 128 + token with c = 4 ks + kq the chunk; its source is lane 16 kq + (token & 15) of fragment (token >> 4, ks)
  auto stage = [&](int qt, int slot) {
    const char* qsrc = a.qfrag + (tile0 + qt) * L::KB;
    char* dst = lds + slot * L::SLOT;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int piece = wave + 8 * q;
      const int c = piece >> 1, token = (piece & 1) * 64 + lane;
      const int unit = ((token >> 4) * 3 + (c >> 2)) * 64 + (c & 3) * 16 + (token & 15);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qsrc + unit * 16),
                                       (__attribute__((address_space(3))) void*)(dst + L::Q + piece * 1024), 16, 0, 0);
    }
    if (wave < 2 * ng)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.wimg + ((tile0 + qt) * ng * 2 + wave) * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + L::W + wave * 1024), 16, 0, 0);
    if (wave == 7)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.rowp + (tile0 + qt) * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + L::RP), 16, 0, 0);
  };
  stage(0, 0);
  i32x4 kf[3];       // this wave's 16 keys as B fragments
#pragma unroll
  for (int ks = 0; ks < 3; ++ks)
    kf[ks] = *(const i32x4*)(a.kimg + (tile0 + kt) * L::KB + (((4 * ks + kq) * 128 + wave * 16 + qi) << 4));
  i32x4 acc[4];      // acc[g][i]: weight row 16 g + 4 kq + i, key qi; from 128 * sum w (the probabilities ride as p - 128)
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = g < ng ? *(const i32x4*)(a.wsum + b * 64 + 16 * g + 4 * kq) : (i32x4){0, 0, 0, 0};

  for (int qt = 0; qt < nqt; ++qt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // query tile qt landed for every wave; every wave is done with the other slot
    if (qt + 1 < nqt) stage(qt + 1, (qt + 1) & 1);
    const char* sb = lds + (qt & 1) * L::SLOT;
    u16x2 w[16];         // w[2 j16 + j] = queries 16 j16 + 4 kq + 2 j, + 1 of this tile against key qi
    ita_long_logits<FAST>(sb + L::Q, kf, kq, qi, a.ml, w);
    i32x4 pf[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k4 = 4 * kb + t;
        const char* rp = sb + L::RP + (4 * k4 + kq) * 32;      // queries 16 k4 + 4 kq + 0..3
        // m m | m m | cap cap | cap cap | inv_hi inv_hi | inv_hi inv_hi as u16 pairs (plain array elements: a bit_cast of a
        // vector element reads element 0 whatever the index)
        const u16x2* prm = (const u16x2*)rp;
        const u16x2 mm0 = prm[0], mm1 = prm[1], cap0 = prm[2], cap1 = prm[3], iv0 = prm[4], iv1 = prm[5];
        const u16x2 s0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm0, w[2 * k4]), cap0);
        const u16x2 s1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm1, w[2 * k4 + 1]), cap1);
        const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv0 >> s0));
        const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv1 >> s1));
        const unsigned p4 = __builtin_amdgcn_perm(p23, p01, 0x06040200u);   // u8 probabilities of queries 64 kb + 16 t + 4 kq + 0..3
        pf[kb][t] = (int)(p4 ^ 0x80808080u);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (g < ng) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          const i32x4 wf = *(const i32x4*)(sb + L::W + (((2 * g + kb) * 64 + lane) << 4));
          acc[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, pf[kb], acc[g], 0, 0, 0);
        }
      }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 16 * g + 4 * kq + i;
      if (r < a.n_w) a.out[((size_t)b * a.n_w + r) * a.S + (size_t)kt * 128 + wave * 16 + qi] = acc[g][i];
    }
}
