// ita_long_f32_prop_kernel.h -- weighted column sums of the S x S probability matrix of the long float attention
// (ita_mha_long_f32_propagate), the float sibling of ita_long_prop_kernel.h:
//     out[b, r, j] = sum_i w[b, r, i] * p[b, i, j]        w f32 (B, R, S), 1 <= R <= 64; out f32 (B, R, S)
// with p[b, i, j] = ita_expf(s - m) * (1.0f / l) the probability of ita_mha_long_f32_taps, each operation rounded on its
// own; s, m and l are the production sweep's bits.  The matrix is never held.  col_mass of the statistics entry is w = all
// ones up to the order of the additions, a probability row is w = one-hot.
//
// The entry runs three launches over the long workspace:
//   ita_lf32_projkq_kernel<E>   ita_lf32_proj_body's K loop run twice, with (wk, bk) and with (wq, bq): the K image and a Q
//                               image in the same layout (64-token units [12 ft][4 kt][64 lanes] f32x4), no V.  Q and K
//                               share the projection chain (bias seed, block sums of 16, groups ascending), so the Q image
//                               holds the bits of ita_lf32_q_prologue and the K image those of ita_lf32_proj_kernel
//   ita_lf32_stats_kernel<E>    unchanged, row_max and row_sum only (sweep 1), into the workspace: m and l of every query
//   ita_lf32_prop_kernel        the TRANSPOSED sweep
//
// ita_lf32_prop_kernel: grid (S / 128 key tiles, B), 512 threads.  Wave v owns keys 16 v .. 16 v + 15 of its key tile; their
// twelve K fragments are read once from the K image (lane (key col, slot) holds K[key][16 ft + 4 slot + r]: the image's
// A fragment is also the B fragment of v_mfma_f32_16x16x4_f32).  The workgroup sweeps the queries in 64-query units.  A
// unit's 48 KB of Q image arrive by LDS-DMA into a two-slot ring and ita_lf32_logits runs as it is with keys and queries
// swapped: f32 products commute and the chain order is the same, so lane (key col, slot) holds s[kt][r], the production
// logit of query 64 u + 16 kt + 4 slot + r for its key.  The query's m and 1.0f / l come from a table in LDS (one f32x4
// each per kt; wave 0 fills the table of unit u + 1 during step u) and p is formed as sweep 2 of the statistics kernel
// forms it.  Those registers are the B operand of a second f32 MFMA with k = query; its A operand is
// w[16 g + col][64 u + 16 kt + 4 slot + 0..3], 16 contiguous bytes of the natural layout, brought into the ring by LDS-DMA
// whose per-lane source address does the gather ([4 g][4 kt][64 lanes] f32x4 per unit; rows >= R read row R - 1 and are
// never stored: an MFMA's output row depends on its own A row only).  One barrier per unit, no atomics, no
// cross-workgroup reduction: a workgroup sees every query.  Vector stores only; rows >= R are never stored.
//
// THE ORDER OF EVERY FLOAT ADDITION (tests/long_f32_propagate_common.py is this in numpy).  For out[r][key]:
//   inside unit u the block t starts at +0.0f and takes, for kt = 0..3 ascending, inside a tile r4 = 0..3 ascending (one
//   MFMA each), inside an MFMA slot = 0..3 ascending (the MFMA's exact fmaf chain over k):
//       t = fmaf(w[r][q], p[q][key], t),   q = 64 u + 16 kt + 4 slot + r4
//   and then acc = acc + t for u ascending, acc from +0.0f.  (Blocked as row_gap of the statistics kernel is: one chain of
//   all S addends loses accuracy at S = 65536.)  A one-hot weight row gives p's bits: fmaf(0, p, t) = t, fmaf(1, p, +0) =
//   p, +0 + t = t.  A row's bits do not depend on R or on its place among the rows, nor on the batch around its frame.
//
// LDS: two slots of 48 KB Q image + 16 KB weight fragments, and 1 KB of row tables: 129 KB, one workgroup per CU, two
// waves per SIMD, as the statistics kernel.
#pragma once
#include "ita_long_f32_kernel.h"

struct ItaLongF32PropProjArgs {
  const float* x;                 // (B, S, E) f32 tokens
  const float *wk, *bk, *wq, *bq; // [P][E], [P]
  f32x4 *kimg, *qimg;             // workspace (B, S/64) units [12][4][64] f32x4 each
  int B, S;
};

struct ItaLongF32PropArgs {
  const f32x4 *kimg, *qimg;       // ita_lf32_projkq_kernel's images
  const float *row_max, *row_sum; // (B, S): ita_lf32_stats_kernel's, in the workspace
  const float* w;                 // (B, n_w, S), 16-byte aligned
  float* out;                     // (B, n_w, S)
  int B, S, n_w;
};

struct ItaLongF32PropLds {
  using L = ItaLongF32Lds;
  static constexpr int WBYTES = 4 * L::NKT * 64 * 16;      // 16384: [4 g][4 kt][64 lanes] f32x4
  static constexpr int Q = 0, W = L::UNIT;                 // inside a slot
  static constexpr int SLOT = L::UNIT + WBYTES;
  static constexpr int TAB = 2 * SLOT;                     // f32 [2][m 64 | 1 / l 64]
  static constexpr int TOTAL = TAB + 2 * 128 * 4;
  static_assert(TOTAL <= 160 * 1024, "one workgroup per CU");
};

// Persistent over the 128-token tiles like ita_lf32_proj_kernel; wave w projects its 16 tokens with ita_lf32_proj_body's K
// loop, once per weight set, and stores the accumulators as they are
template <int E>
__global__ __launch_bounds__(512) void ita_lf32_projkq_kernel(const ItaLongF32PropProjArgs a) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel k groups");
  using L = ItaLongF32Lds;
  constexpr int NFT = L::NFT, NG = E / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, slot = lane >> 4;
  const int ntile = a.B * (a.S / 128);
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const float* xsrc = a.x + ((size_t)tile * 128 + 16 * wave + col) * E + 4 * slot;
    f32x4 xf[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) xf[g] = *(const f32x4*)(xsrc + 16 * g);
    const size_t dst = ((size_t)(2 * tile + (wave >> 2)) * NFT * L::NKT + (wave & 3)) * 64 + lane;
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
      const float* wm = which ? a.wq : a.wk;
      const float* bm = which ? a.bq : a.bk;
      f32x4* d = (which ? a.qimg : a.kimg) + dst;
#pragma unroll
      for (int ft = 0; ft < NFT; ft += 2) {
        f32x4 ka[2];
        const float* wr[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          ka[u] = *(const f32x4*)(bm + 16 * (ft + u) + 4 * slot);
          wr[u] = wm + ita_opaque((16 * (ft + u) + col) * E + 4 * slot);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const f32x4 w0 = *(const f32x4*)(wr[0] + 16 * g), w1 = *(const f32x4*)(wr[1] + 16 * g);
          f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};   // block sum: 16 products from zero, then onto the total
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[r], xf[g][r], t0, 0, 0, 0);
            t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[r], xf[g][r], t1, 0, 0, 0);
          }
          ka[0] += t0;
          ka[1] += t1;
        }
        d[ft * L::NKT * 64] = ka[0];
        d[(ft + 1) * L::NKT * 64] = ka[1];
      }
    }
  }
}

__global__ __launch_bounds__(512) void ita_lf32_prop_kernel(const ItaLongF32PropArgs a) {
  using L = ItaLongF32Lds;
  using T = ItaLongF32PropLds;
  constexpr int NFT = L::NFT, NKT = L::NKT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, slot = lane >> 4;
  const int nu = a.S / 64, tile = blockIdx.x, b = blockIdx.y;
  const int ng = (a.n_w + 15) >> 4;
  const char* qimg = (const char*)(a.qimg + (size_t)b * nu * L::UNIT_F4);
  const float* rmax = a.row_max + (size_t)b * a.S;
  const float* rsum = a.row_sum + (size_t)b * a.S;
  float* tab = (float*)(lds + T::TAB);

  // unit u into a ring slot by LDS-DMA: the Q image as it lies (six 1 KB pieces per wave) and the weight fragments, piece
  // (g, kt) = lane (row col, slot) reading w[16 g + col][64 u + 16 kt + 4 slot + 0..3] (two pieces per wave)
  auto stage = [&](int u, int ring) {
    const char* src = qimg + (size_t)u * L::UNIT;
    char* dst = lds + ring * T::SLOT;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int piece = wave + 8 * p;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + T::Q + piece * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int piece = wave + 8 * p, g = piece >> 2, kt = piece & 3;
      if (g < ng) {
        const int r = min(16 * g + col, a.n_w - 1);
        const float* ws = a.w + ((size_t)b * a.n_w + r) * a.S + 64 * u + 16 * kt + 4 * slot;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)ws,
                                         (__attribute__((address_space(3))) void*)(dst + T::W + piece * 1024), 16, 0, 0);
      }
    }
  };
  stage(0, 0);
  if (wave == 0) {      // the row table of unit 0
    tab[lane] = rmax[lane];
    tab[64 + lane] = 1.0f / rsum[lane];
  }
  f32x4 kf[NFT];        // this wave's 16 keys: unit 2 tile + wave / 4 of the K image, key tile wave & 3
  {
    const f32x4* ks = a.kimg + (((size_t)b * nu + 2 * tile + (wave >> 2)) * NFT * NKT + (wave & 3)) * 64 + lane;
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) kf[ft] = ks[ft * NKT * 64];
  }
  f32x4 acc[4];         // acc[g][r]: weight row 16 g + 4 slot + r, key col
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0, 0, 0, 0};

  for (int u = 0; u < nu; ++u) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // unit u and its row table landed for every wave; every wave is done with the other slot
    float tm = 0.0f, tl = 1.0f;
    if (u + 1 < nu) {
      stage(u + 1, (u + 1) & 1);
      if (wave == 0) {
        tm = rmax[64 * (u + 1) + lane];
        tl = rsum[64 * (u + 1) + lane];
      }
    }
    const char* sb = lds + (u & 1) * T::SLOT;
    f32x4 s[NKT];
    ita_lf32_logits((const f32x4*)(sb + T::Q), lane, kf, s);
    const float* tu = tab + (u & 1) * 128 + 4 * slot;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const f32x4 m4 = *(const f32x4*)(tu + 16 * kt), i4 = *(const f32x4*)(tu + 64 + 16 * kt);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] = ita_expf(s[kt][r] - m4[r]) * i4[r];
    }
    const f32x4* wb = (const f32x4*)(sb + T::W) + lane;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (g < ng) {
        f32x4 t = {0, 0, 0, 0};
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          const f32x4 wf = wb[(g * NKT + kt) * 64];
#pragma unroll
          for (int r = 0; r < 4; ++r) t = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[r], s[kt][r], t, 0, 0, 0);
        }
        acc[g] += t;
      }
    if (wave == 0 && u + 1 < nu) {   // that table's readers of step u - 1 are behind this step's barrier; step u + 1 reads it
      float* tn = tab + ((u + 1) & 1) * 128;
      tn[lane] = tm;
      tn[64 + lane] = 1.0f / tl;
    }
  }
  float* orow = a.out + (size_t)b * a.n_w * a.S + (size_t)tile * 128 + 16 * wave + col;
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * g + 4 * slot + r;
      if (row < a.n_w) orow[(size_t)row * a.S] = acc[g][r];
    }
}
