// ita_long_f32_hist_kernel.h -- histograms of the logits, of their gaps to the row maximum and of the probabilities of the
// whole S x S matrix of the long float attention, and the range of its logits (ita_mha_long_f32_hist): the float sibling
// of ita_long_hist_kernel.h.  The matrix is never held.  Behind the unchanged production projection launch
// (ita_lf32_proj_kernel<E>; only its K image is read):
//
//   ita_lf32_hist_kernel<E> : grid (S / 128, B), 512 threads, wave w owns queries 16 w .. 16 w + 15 of its query tile, K
//                             units by LDS-DMA into the two-slot ring of ItaLongF32Lds, one barrier per step (there is no
//                             V).  Steps 0 .. nu - 1 are sweep 1, steps nu .. 2 nu - 1 sweep 2, as ita_lf32_stats_kernel.
//     prologue  Q^T of the wave's queries: ita_lf32_q_prologue
//     sweep 1   the production sweep for m and l (ita_lf32_logits, _running_max, _sum_slots: the production bits) and,
//               for `range`, each lane's running minimum and maximum of s.  A call that asks for range only ends here.
//     sweep 2   the same MFMA chains again, so s is bit-equal to sweep 1's; per element, each operation rounded on its own,
//                   r = rintf(s * scale)                 logit bin  clamp(r, -128, 127) + 128;  r < -128, r > 127 counted
//                   d = m - s                            gap bin    min(rintf(d * scale), 255)
//                   p = ita_expf(s - m) * (1.0f / l)     prob bin   bits(p) >> 23, the biased binary exponent
//   ita_lf32_hist_zero_kernel : the outputs to 0, range to (+inf, -inf): a kernel, so a captured call is kernel nodes only
//
// Counting.  Per-wave 32-bit sub-histograms in LDS, three tables of [8 waves][256] words (24 KB) in the V slot of
// ItaLongF32Lds, which this kernel never stages.  Hot bins are the norm here: flat rows put every probability of a
// workgroup into one exponent bin, and with |logit| in the hundreds nearly every gap sits in bin 255 and nearly every
// probability in bin 0 -- 64 lanes of one LDS atomic on one word.  So an add is aggregated inside the wave first
// (ita_lf32_hist_add): the lanes that share lane 0's bin are counted with a ballot and lane 0 adds their number once; only
// the other lanes add 1 each.  A workgroup sees 128 S <= 2^23 elements, so no 32-bit word overflows.  At the end the eight
// sub-histograms are summed per bin and added to the frame's s64 bins with 64-bit integer global atomics.
// Range.  fminf / fmaxf over the lane's logits, over the four slot lanes and the 16 query lanes of the wave in a fixed
// order; lane 0 of every wave then updates the frame's pair with INTEGER atomics on the float's bits
// (ita_lf32_atomic_minf / _maxf): signed order among non-negative floats, reversed unsigned order among negative ones, and
// either kind displaces the other in one direction only, so the result does not depend on the order of the updates.
// There are no floating-point atomics: the same input gives the same bytes on every call, in any batch position.
// A null pointer skips that output's adds and stores; without logits, shifts, probs and logits_out there is no sweep 2.
// Every index into a table is clamped to 0 .. 255 whatever the input (non-finite x: unspecified counts, no stray access).
//
// The kernels carry target("no-packed-fp32-ops") (ITA_NO_PK_F32) and live in namespace ita_f32_hist: the code-object census
// of tests/test_long_f32_propagate_abi.py counts the global ita_lf32_ kernels, and these are not of that family's ten.
// ITA_LF32_HIST_ABLATE is for timing builds only (tools/bench_long_f32_hist.py): 1 forms every bin and makes no LDS add (its counts
// are wrong): what the counting costs; 2 adds 1 per lane without the aggregation: what the aggregation saves.
#pragma once
#include "ita_long_f32_kernel.h"
#include "ita_long_heads_kernel.h"   // ITA_NO_PK_F32

#ifndef ITA_LF32_HIST_ABLATE
#define ITA_LF32_HIST_ABLATE 0
#endif

struct ItaLongF32HistArgs {
  const float* x;                 // (B, S, E) f32 tokens: the workgroup's own 128 rows, for Q
  const float *wq, *bq;           // [P][E], [P]
  const f32x4* kimg;              // ita_lf32_proj_kernel's workspace: (B, S/64) units [12][4][64] f32x4
  int B, S;
  float scale;                    // finite, > 0: 1 / the quantiser step
  unsigned long long *logits, *shifts, *probs;   // (B, 256) each, zero before the launch; any may be null
  unsigned long long* logits_out;                // (B, 2): below, above; zero before the launch
  float* range;                                  // (B, 2): +inf, -inf before the launch
};

struct ItaLongF32HistLds {
  using L = ItaLongF32Lds;
  static constexpr int TABLE = 8 * 256 * 4;          // u32 [8 waves][256]
  static constexpr int HL = L::V, HS = HL + TABLE, HP = HS + TABLE;
  static constexpr int WORDS = 3 * TABLE / 4;
  static_assert(HP + TABLE <= L::TOTAL, "the three sub-histogram tables sit in the V slot");
};

namespace ita_f32_hist {

__global__ __launch_bounds__(256) void ita_lf32_hist_zero_kernel(const ItaLongF32HistArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // (grid = B)
  if (a.logits) a.logits[i] = 0;
  if (a.shifts) a.shifts[i] = 0;
  if (a.probs) a.probs[i] = 0;
  if (threadIdx.x < 2) {
    const size_t j = (size_t)blockIdx.x * 2 + threadIdx.x;
    if (a.logits_out) a.logits_out[j] = 0;
    if (a.range) a.range[j] = threadIdx.x ? -__builtin_inff() : __builtin_inff();
  }
}

// One count into a wave's sub-histogram.  Every lane of the wave is here: the lanes whose bin is lane 0's are counted by a
// ballot and added once by lane 0, the others add 1 each.
__device__ __forceinline__ void ita_lf32_hist_add(unsigned* tbl, int bin, int lane) {
#if ITA_LF32_HIST_ABLATE == 1
  asm volatile("" ::"v"(bin));   // the bin is formed and dropped
#elif ITA_LF32_HIST_ABLATE == 2
  atomicAdd(tbl + bin, 1u);
#elif ITA_LF32_HIST_ABLATE == 0
  const int lead = __builtin_amdgcn_readfirstlane(bin);
  const unsigned long long same = __builtin_amdgcn_ballot_w64(bin == lead);
  if (lane == 0 || bin != lead) atomicAdd(tbl + bin, lane == 0 ? (unsigned)__builtin_popcountll(same) : 1u);   // (lane 0's bin is lead)
#endif
}

// minimum / maximum of a float in global memory by integer atomics on its bits (header): the stored value starts at
// +inf / -inf and every update is a finite float or an infinity
__device__ __forceinline__ void ita_lf32_atomic_minf(float* at, float v) {
  const int b = __float_as_int(v);
  if (b >= 0) atomicMin((int*)at, b);                 // among non-negative floats the signed order; a negative one stays
  else atomicMax((unsigned*)at, (unsigned)b);         // among negative floats the larger bits; displaces a non-negative one
}
__device__ __forceinline__ void ita_lf32_atomic_maxf(float* at, float v) {
  const int b = __float_as_int(v);
  if (b >= 0) atomicMax((int*)at, b);                 // displaces a negative float (a negative int)
  else atomicMin((unsigned*)at, (unsigned)b);         // a non-negative float (smaller unsigned bits) stays
}
// minimum / maximum over the 64 lanes of a wave: the four slot lanes, then the 16 lanes of a DPP row by rotation
__device__ __forceinline__ float ita_lf32_wave_minf(float v) {
  v = fminf(v, __int_as_float(xor16_i(__float_as_int(v))));
  v = fminf(v, __int_as_float(xor32_i(__float_as_int(v))));
  v = fminf(v, __uint_as_float(ita_row_ror<0x128>(__float_as_uint(v))));
  v = fminf(v, __uint_as_float(ita_row_ror<0x124>(__float_as_uint(v))));
  v = fminf(v, __uint_as_float(ita_row_ror<0x122>(__float_as_uint(v))));
  return fminf(v, __uint_as_float(ita_row_ror<0x121>(__float_as_uint(v))));
}
__device__ __forceinline__ float ita_lf32_wave_maxf(float v) {
  v = fmaxf(v, __int_as_float(xor16_i(__float_as_int(v))));
  v = fmaxf(v, __int_as_float(xor32_i(__float_as_int(v))));
  v = fmaxf(v, __uint_as_float(ita_row_ror<0x128>(__float_as_uint(v))));
  v = fmaxf(v, __uint_as_float(ita_row_ror<0x124>(__float_as_uint(v))));
  v = fmaxf(v, __uint_as_float(ita_row_ror<0x122>(__float_as_uint(v))));
  return fmaxf(v, __uint_as_float(ita_row_ror<0x121>(__float_as_uint(v))));
}

// the kernel's body: a function without the kernel's target attribute, so that its lambdas are inlined into it and it
// into the kernel (as the bodies of ita_long_heads_kernel.h)
template <int E>
__device__ __forceinline__ void ita_lf32_hist_body(const ItaLongF32HistArgs& a) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel groups");
  using L = ItaLongF32Lds;
  using T = ItaLongF32HistLds;
  constexpr int NFT = L::NFT, NKT = L::NKT;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, slot = lane >> 4;
  const int t0 = 16 * wave;   // this wave's queries inside the tile
  const int nu = a.S / 64, qt = blockIdx.x, b = blockIdx.y;
  const char* kimg = (const char*)(a.kimg + (size_t)b * nu * L::UNIT_F4);
  const bool sweep2 = a.logits || a.shifts || a.probs || a.logits_out;
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
  // barrier of sweep 1 (the tables in the V slot are zeroed behind sweep 1)
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

  // ---------------- sweep 1: the production sweep's m and l; the lane's extremes of s
  float m = -__builtin_inff(), l = 0.0f;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int u = 0; u < nu; ++u) {
    step_top(u);
    f32x4 s[NKT];
    ita_lf32_logits((const f32x4*)(lds + L::K + (u & 1) * L::UNIT), lane, q, s);
    if (a.range) {
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lo = fminf(lo, s[kt][r]);
          hi = fmaxf(hi, s[kt][r]);
        }
    }
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
  if (a.range) {
    lo = ita_lf32_wave_minf(lo);
    hi = ita_lf32_wave_maxf(hi);
    if (lane == 0) {
      ita_lf32_atomic_minf(a.range + (size_t)b * 2, lo);
      ita_lf32_atomic_maxf(a.range + (size_t)b * 2 + 1, hi);
    }
  }
  if (!sweep2) return;

  // ---------------- sweep 2: the bins.  Every wave is behind the first barrier, so every parked Q has been read back
  // and the V slot is free: the tables are zeroed here and first added to behind the next barrier
  for (int i = tid; i < T::WORDS; i += 512) ((unsigned*)(lds + T::HL))[i] = 0;
  [[maybe_unused]] unsigned* hl = (unsigned*)(lds + T::HL) + wave * 256;   // (unused in the ablation build)
  [[maybe_unused]] unsigned* hs = (unsigned*)(lds + T::HS) + wave * 256;
  [[maybe_unused]] unsigned* hp = (unsigned*)(lds + T::HP) + wave * 256;
  [[maybe_unused]] const bool want_l = a.logits != nullptr, want_s = a.shifts != nullptr, want_p = a.probs != nullptr;   // (uniform)
  const float inv = 1.0f / l, scale = a.scale;
  int below = 0, above = 0;
#pragma unroll 1
  for (int u = 0; u < nu; ++u) {
    step_top(nu + u);
    f32x4 s[NKT];
    ita_lf32_logits((const f32x4*)(lds + L::K + (u & 1) * L::UNIT), lane, q, s);
    // the logits are whole HERE: without this the block sums' additions sink into the branches of the adds below, one
    // chain per element, and all 12 x 16 block values stay live until then (spills)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) asm volatile("" : "+v"(s[kt]));
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      __builtin_amdgcn_sched_barrier(0);   // tile by tile: sixteen elements' exp chains at once are registers for nothing
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sv = s[kt][r];
        const float rq = rintf(sv * scale);
        below += rq < -128.0f ? 1 : 0;
        above += rq > 127.0f ? 1 : 0;
        if (want_l) ita_lf32_hist_add(hl, (int)fminf(fmaxf(rq, -128.0f), 127.0f) + 128, lane);
        if (want_s) {
          const float d = m - sv;
          ita_lf32_hist_add(hs, (int)fminf(fmaxf(rintf(d * scale), 0.0f), 255.0f), lane);
        }
        if (want_p) {
          const float p = ita_expf(sv - m) * inv;
          ita_lf32_hist_add(hp, (int)((__float_as_uint(p) >> 23) & 255u), lane);   // (p >= 0: & 255 only keeps the index in the table)
        }
      }
    }
  }
  __syncthreads();       // every wave's adds are in the tables
  // ---------------- the workgroup's counts into the frame's: one thread per (table, bin), the eight waves' words added
  for (int i = tid; i < 3 * 256; i += 512) {
    const int tb = i >> 8, bin = i & 255;
    unsigned long long* dst = tb == 0 ? a.logits : tb == 1 ? a.shifts : a.probs;
    if (!dst) continue;
    const unsigned* t8 = (const unsigned*)(lds + T::HL + tb * T::TABLE) + bin;
    unsigned v = 0;
#pragma unroll
    for (int wv = 0; wv < 8; ++wv) v += t8[wv * 256];
    if (v) atomicAdd(dst + (size_t)b * 256 + bin, (unsigned long long)v);
  }
  if (a.logits_out) {
    below = (int)ita_row16_sum((unsigned)sum1632_i(below));     // the wave's total in every lane: <= 16 S <= 2^20
    above = (int)ita_row16_sum((unsigned)sum1632_i(above));
    if (lane == 0) {
      if (below) atomicAdd(a.logits_out + (size_t)b * 2, (unsigned long long)below);
      if (above) atomicAdd(a.logits_out + (size_t)b * 2 + 1, (unsigned long long)above);
    }
  }
}
template <int E>
__global__ __launch_bounds__(512) ITA_NO_PK_F32 void ita_lf32_hist_kernel(const ItaLongF32HistArgs a) {
  ita_lf32_hist_body<E>(a);
}

}  // namespace ita_f32_hist
