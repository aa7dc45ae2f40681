// ita_long_f32_stats_kernel.h -- row and column statistics of the whole S x S probability matrix of the long float
// attention (ita_mha_long_f32_stats), the float sibling of ita_long_stats_kernel.h.  The matrix is never held.  Behind the
// unchanged production projection launch (ita_lf32_proj_kernel<E>; only its K image is read):
//
//   ita_lf32_stats_kernel<E> : grid (S / 128, B), 512 threads, wave w owns queries 16 w .. 16 w + 15 of its query tile,
//                              K units by LDS-DMA into the two-slot ring of ItaLongF32Lds, one barrier per step (there
//                              is no V).  Steps 0 .. nu - 1 are sweep 1, steps nu .. 2 nu - 1 sweep 2 (nu = S / 64 is
//                              even, so unit u sits in ring slot u & 1 in both; the last step of sweep 1 prefetches unit 0).
//     prologue  Q^T of the wave's queries: ita_lf32_attn_body's
//     sweep 1   ita_lf32_attn_body's loop without V and c[]: the same block-summed S^T, the same mn / down /
//               l = l * down + sum, the same closing xor16 / xor32 add: m and l are the production bits
//     sweep 2   the same MFMA chains again, so s is bit-equal to sweep 1's; per element, each operation rounded on its own,
//                   d = m - s;   p = ita_expf(s - m) * (1.0f / l)          (the probability of ita_mha_long_f32_taps)
//               and p is reduced along the row and along the column
//   ita_lf32_colsum_kernel   : one thread per (frame, key): the query tiles' partials added in ascending tile order
//
// The Q prologue, the logits chain, the running maximum and the closing add are ita_long_f32_kernel.h's functions
// (ita_lf32_q_prologue, _logits, _running_max, _sum_slots), which ita_lf32_attn_body runs too: m and l cannot drift from
// the production bits.  stage stays a lambda in both kernels: as a shared function it made this kernel 0.4 to 0.9 % slower
// ("Long attention, shared").
//
// THE ORDER OF EVERY FLOAT ADDITION (no floating-point atomics anywhere; tests/long_f32_stats_common.py is this in numpy):
//   row_gap   lane (query col, slot) holds keys 64 u + 16 kt + 4 slot + r of its query.  Inside a unit the lane's 16
//             products are added from 0.0f, gu = gu + p * d for kt ascending, inside a tile r ascending; the lane's share
//             starts at 0.0f and takes gap = gap + gu for u ascending.  (One chain of all S / 4 products lost 4.1e-5 of a
//             row_gap near 2 at S = 65536 on flat rows: 16384 small addends onto a running sum.)  The four slot lanes
//             are then added as l is: g = g + xor16(g), g = g + xor32(g), that is (g0 + g1) + (g2 + g3).
//   col_mass  (a) inside a wave, per key: the 16 query lanes of a DPP row by rotate-and-add, row_ror 8, 4, 2, 1.  Every
//                 step adds a lane's value and its partner's, so all lanes hold the same bits: with v[q] the value of
//                 query 16 w + q,  a[q] = v[q] + v[q + 8] (q < 8),  b[q] = a[q] + a[q + 4] (q < 4),
//                 c[q] = b[q] + b[q + 2] (q < 2),  wave sum = c[0] + c[1]
//             (b) the eight waves of the workgroup through an LDS table [wave][key]: ((((w0 + w1) + w2) + ...) + w7),
//                 one lane per key, stored as the partial of (frame, query tile, key) -- written exactly once
//             (c) ita_lf32_colsum_kernel: the partial of tile 0, then + tile 1, + tile 2, ... + tile S / 128 - 1
//   row_nnz, col_nnz are integer counts of p >= p_min and take the same three routes with integer additions.
// A frame's values depend on nothing but its own rows of x: blockIdx.y picks the frame, and no sum crosses frames.
//
// LDS: the K ring (2 x 48 KB) and, in the V slot of ItaLongF32Lds, the column tables: two slots by unit parity of
// f32 [8 waves][64 keys] and s32 [8 waves][64 keys], 8 KB in all.  Unit u's table is complete behind the barrier of step
// u + 1; waves 0 (masses) and 1 (counts) add it up and store the partial there, and the slot is written again two barriers
// later.  The launch asks for ItaLongF32Lds::TOTAL, as the production kernel does.
// Null row pointers skip the store; null partial pointers skip the whole column reduction; without row_gap, row_nnz and
// the partials there is no sweep 2.  Every store is at (b, token < S) or (b, query tile, key < S) of the call.
#pragma once
#include "ita_long_f32_kernel.h"

struct ItaLongF32StatsArgs {
  const float* x;                 // (B, S, E) f32 tokens: the workgroup's own 128 rows, for Q
  const float *wq, *bq;           // [P][E], [P]
  const f32x4* kimg;              // ita_lf32_proj_kernel's workspace: (B, S/64) units [12][4][64] f32x4
  int B, S;
  float p_min;
  float *row_max, *row_sum, *row_gap;   // (B, S) each; any may be null
  int* row_nnz;
  float* part_mass;               // (B, S/128, S): the workgroup's column sums of its 128 queries; may be null
  int* part_nnz;                  // (B, S/128, S); may be null
};

struct ItaLongF32StatsLds {
  using L = ItaLongF32Lds;
  static constexpr int CM = L::V;                    // f32 [2][8][64]
  static constexpr int CN = CM + 2 * 8 * 64 * 4;     // s32 [2][8][64]
  static_assert(CN + 2 * 8 * 64 * 4 <= L::TOTAL, "the column tables sit in the V slot");
};

template <int E>
__global__ __launch_bounds__(512) void ita_lf32_stats_kernel(const ItaLongF32StatsArgs a) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel groups");
  using L = ItaLongF32Lds;
  using T = ItaLongF32StatsLds;
  constexpr int NFT = L::NFT, NKT = L::NKT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, slot = lane >> 4;
  const int t0 = 16 * wave;   // this wave's queries inside the tile
  const int nu = a.S / 64, nqt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const char* kimg = (const char*)(a.kimg + (size_t)b * nu * L::UNIT_F4);
  const bool cols = a.part_mass || a.part_nnz;
  const bool sweep2 = cols || a.row_gap || a.row_nnz;
  const int nstep = sweep2 ? 2 * nu : nu;

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
  // barrier of sweep 1
  const float* xsrc = a.x + ((size_t)b * a.S + (size_t)qt * 128 + t0 + col) * E + 4 * slot;
  f32x4 q[NFT];
  ita_lf32_q_prologue<E>(xsrc, a.wq, a.bq, col, slot, (f32x4*)(lds + L::K + L::UNIT) + wave * NFT * 64 + lane, q);

  // the top of a step: its K unit (ring slot step & 1) has landed for every wave and every wave is done with the step
  // before, so the other slot is free for the next step's unit (unit 0 again behind the last step of sweep 1)
  auto step_top = [&](int step) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nx = step + 1;
    if (nx < nstep) stage(kimg + (size_t)(nx < nu ? nx : nx - nu) * L::UNIT, L::K + (nx & 1) * L::UNIT);
  };

  // ---------------- sweep 1: the running maximum m and this lane's share l of the running sum, as the production sweep
  float m = -__builtin_inff(), l = 0.0f;
  for (int u = 0; u < nu; ++u) {
    step_top(u);
    f32x4 s[NKT];
    ita_lf32_logits((const f32x4*)(lds + L::K + (u & 1) * L::UNIT), lane, q, s);
    float down;
    const float mn = ita_lf32_running_max(s, m, down);   // first unit: down is the clamp's e^-87, times l = 0
    float sum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += ita_expf(s[kt][r] - mn);
    l = l * down + sum;
  }
  l = ita_lf32_sum_slots(l);   // the same sum in all four lanes of the query
  const size_t row = (size_t)b * a.S + (size_t)qt * 128 + t0 + col;
  if (slot == 0) {
    if (a.row_max) a.row_max[row] = m;
    if (a.row_sum) a.row_sum[row] = l;
  }
  if (!sweep2) return;

  // ---------------- sweep 2: the probabilities, reduced along the rows (registers) and the columns (DPP, LDS table)
  const float inv = 1.0f / l;
  float* cm = (float*)(lds + T::CM);
  int* cn = (int*)(lds + T::CN);
  // unit u's column tables are complete behind the barrier of the step after it: wave 0 adds the eight waves' masses in
  // wave order, wave 1 their counts, one lane per key, and stores the workgroup's partial for the unit's 64 keys
  auto flush = [&](int u) {
    if (wave < 2) {
      const size_t at = ((size_t)b * nqt + qt) * a.S + 64 * u + lane;
      if (wave == 0) {
        if (a.part_mass) {
          const float* p = cm + (u & 1) * 512 + lane;
          float acc = p[0];
#pragma unroll
          for (int w = 1; w < 8; ++w) acc = acc + p[64 * w];
          a.part_mass[at] = acc;
        }
      } else if (a.part_nnz) {
        const int* p = cn + (u & 1) * 512 + lane;
        int acc = p[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) acc += p[64 * w];
        a.part_nnz[at] = acc;
      }
    }
  };
  float gap = 0.0f;
  int nnz = 0;
  for (int u = 0; u < nu; ++u) {
    step_top(nu + u);
    if (cols && u > 0) flush(u - 1);
    f32x4 s[NKT];
    ita_lf32_logits((const f32x4*)(lds + L::K + (u & 1) * L::UNIT), lane, q, s);
    unsigned f4[NKT];   // byte r of word kt: is p of key 16 kt + 4 slot + r at least p_min
    float gu = 0.0f;    // the unit's share of row_gap
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f4[kt] = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = m - s[kt][r];
        const float p = ita_expf(s[kt][r] - m) * inv;
        s[kt][r] = p;
        gu = gu + p * d;
        const unsigned f = p >= a.p_min ? 1u : 0u;
        nnz += (int)f;
        f4[kt] |= f << (8 * r);
      }
    }
    gap = gap + gu;
    if (cols) {
      float* cmw = cm + (u & 1) * 512 + wave * 64 + 4 * slot;
      int* cnw = cn + (u & 1) * 512 + wave * 64 + 4 * slot;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        f32x4 cs;
#pragma unroll
        for (int r = 0; r < 4; ++r) cs[r] = ita_row16_sumf(s[kt][r]);
        const unsigned c4 = ita_row16_sum(f4[kt]);   // <= 16 per byte
        if (col == 0) {
          *(f32x4*)(cmw + 16 * kt) = cs;
          *(i32x4*)(cnw + 16 * kt) = (i32x4){(int)(c4 & 0xffu), (int)((c4 >> 8) & 0xffu), (int)((c4 >> 16) & 0xffu), (int)(c4 >> 24)};
        }
      }
    }
  }
  if (cols) {
    __syncthreads();       // the last unit's column tables are complete
    flush(nu - 1);
  }
  gap = ita_lf32_sum_slots(gap);
  nnz = sum1632_i(nnz);
  if (slot == 0) {
    if (a.row_gap) a.row_gap[row] = gap;
    if (a.row_nnz) a.row_nnz[row] = nnz;
  }
}

// col_mass[b, j] = the partials of query tiles 0 .. nqt - 1 added in ascending tile order, col_nnz likewise: one thread
// per (frame, key), 256 consecutive keys per workgroup and load.  Either pair of pointers may be null.
__global__ __launch_bounds__(256) void ita_lf32_colsum_kernel(const float* part_mass, const int* part_nnz, float* col_mass,
                                                              int* col_nnz, int nqt, int S, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t bf = i / (size_t)S, j = i - bf * S;
    const size_t base = bf * nqt * S + j;
    if (col_mass) {
      float acc = part_mass[base];
      for (int t = 1; t < nqt; ++t) acc = acc + part_mass[base + (size_t)t * S];
      col_mass[i] = acc;
    }
    if (col_nnz) {
      int acc = part_nnz[base];
      for (int t = 1; t < nqt; ++t) acc += part_nnz[base + (size_t)t * S];
      col_nnz[i] = acc;
    }
  }
}
