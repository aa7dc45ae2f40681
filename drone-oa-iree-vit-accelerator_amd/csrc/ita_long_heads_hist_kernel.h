// ita_long_heads_hist_kernel.h -- per head the histograms of the logits, the softmax shifts and the u8 probabilities of the
// H whole S x S matrices of the long int8 attention with H = 2, 3, 4 or 6 heads, and the range of each head's raw
// accumulators (ita_mha_long_heads_int8_hist): ita_long_hist_kernel's five results for head hd's own matrix
// requant(Q_hd . K_hd^T, ml).  No matrix is held: the kernel runs behind the unchanged production projection launch on the
// layer's own image (Layer::limg_mha) and reads only that launch's workspace -- the Q fragments and the K images.
//
// Work split: grid (S / 128, B), 512 threads, wave w owns queries 16 w .. 16 w + 15 of its query tile, K tiles by LDS-DMA
// into the two-slot ring, one barrier per key-tile step; the ring slot of a step is step & 1 through all passes.
//   fragments  ita_long_heads_qk's: the head Q fragments (H NS of them) and the dword-gathered K fragments
//   sweep 1    ONE pass over the key tiles with all H heads inside the key-tile step (ita_long_heads_qk<H, H>): per head the
//              running minimum and maximum of the raw accumulators, 2 H registers; the maximum requantised once per head and
//              row (lh_lg16), both ends into the workgroup's range per head
//   sweep 2    HEAD GROUPS OF ONE: the key tiles are streamed once per head (ita_long_heads_qk<H, 1>), H passes of nkt steps.
//              A pass is the one-head kernel's sweep 2 on the head's logits (lh_lg16x2: every bit is what
//              ita_long_heads_attn_kernel computes with): logit bin, shift bin, below / above counts, row sum, shift classes
//              0 .. 7 per query row.  Behind a pass the probabilities come from the classes and inv_hi (no third sweep), the
//              head's tables go to the frame's int64 bins of (b, hd) with 64-bit integer global atomics and are cleared by the
//              threads that read them; the next pass's first barrier stands between the clearing and the next adds.
//
// Why head groups and not the heads inside the step.  A head needs the one-head kernel's tables: two of 8 waves x 256 words,
// 4 KB of row classes, 1 KB of probabilities = 21 KB.  Beside the 48 KB ring two workgroups per CU leave 32 KB, so with the
// heads inside the step the sub-histogram copies would have to shrink to 4, 2, 1 and less than 1 per head at H = 2, 3, 4, 6,
// and every halving doubles the lanes that meet in a hot bin -- the adds into those tables are what the sweep's time is
// made of (ita_long_hist_kernel.h, the ablation build).  With one head per pass the tables are one head's at every H: 69 KB,
// per-wave copies, a hot bin serialises inside a wave only, exactly as at H = 1, and the per-head state next to the H NS
// Q fragments is three registers (row sum, below, above) and not 6 H.  The price is staging: (1 + H) nkt tiles of 24 KB per
// workgroup instead of 2 nkt, by LDS-DMA out of L2 one step ahead of the 32 x 3 LDS adds per lane the step spends on them,
// and H flushes of 768 bins per workgroup instead of one.
//
// Bounds.  A workgroup adds 128 S <= 2^23 entries per head to its 32-bit tables (sub-histograms, probabilities), a row class
// holds <= S <= 2^16, a lane's below / above counts <= S / 4 and the wave's <= 16 S = 2^20: nothing 32-bit can overflow at
// S = 65 536.  Integer addition, minimum and maximum have no order: the same bytes on every call.  The entry sets the
// outputs to 0 (acc_range to INT_MAX, INT_MIN) with ita_long_hist_zero_kernel on B H blocks before the launch.
// A null pointer skips that output's adds and stores.
#pragma once
#include "ita_long_heads_kernel.h"
#include "ita_long_hist_kernel.h"

// ItaLongHistLds with a range per head: the two-slot K ring, ONE head's per-wave logit and shift sub-histograms, row
// classes and probability histogram (reused pass by pass), the accumulator range of every head.  Two workgroups per CU.
struct ItaLongHeadsHistLds {
  static constexpr int KB = ItaLongLds::KB;
  static constexpr int K = 0;
  static constexpr int HL = 2 * KB;                    // u32 [8 waves][256]: clamped logit + 128
  static constexpr int HS = HL + 8 * 256 * 4;          // u32 [8 waves][256]: row maximum - clamped logit
  static constexpr int RC = HS + 8 * 256 * 4;          // u32 [128 rows][8]: keys of the row at shift 0 .. 7
  static constexpr int HP = RC + 128 * 8 * 4;          // u32 [256]: probabilities
  static constexpr int RG = HP + 256 * 4;              // i32 [6 heads][2]: minimum, maximum of the biased accumulators
  static constexpr int TOTAL = RG + 64;
  static constexpr int TABLE_WORDS = (RG - HL) / 4;    // the four counting tables
  static_assert(128 * 65536 <= (1 << 23), "a workgroup's entries per head fit every 32-bit counter 512 times over");
  static_assert(2 * TOTAL <= 160 * 1024, "two workgroups per CU");
};

template <bool FAST, int H>
__device__ __forceinline__ void ita_long_heads_hist_body(const ItaLongHistArgs& a) {
  static_assert(H == 2 || H == 3 || H == 4 || H == 6, "the head counts check_blob admits besides 1");
  constexpr int NC = 12 / H, NS = (NC + 3) / 4;
  using L = ItaLongHeadsHistLds;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nkt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const size_t tile0 = (size_t)b * nkt;              // first tile index of this frame
  const char* kimg = a.kimg + tile0 * L::KB;
  unsigned* hl = (unsigned*)(lds + L::HL) + wave * 256;
  unsigned* hs = (unsigned*)(lds + L::HS) + wave * 256;
  unsigned* rc = (unsigned*)(lds + L::RC) + (wave * 16 + qi) * 8;
  unsigned* hp = (unsigned*)(lds + L::HP);
  int* rg = (int*)(lds + L::RG);

  auto stage = [&](const char* src, int ldsoff) {    // 24 KB by LDS-DMA: three 1 KB pieces per wave
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int piece = wave + 8 * q;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + ldsoff + piece * 1024), 16, 0, 0);
    }
  };
  stage(kimg, L::K);
  for (int i = tid; i < L::TABLE_WORDS; i += 512) ((unsigned*)(lds + L::HL))[i] = 0;   // (first used behind sweep 1's barriers)
  if (tid < 2 * H) rg[tid] = (tid & 1) ? (int)0x80000000 : 0x7fffffff;
  // head-relative Q fragments: ita_long_heads_attn_body's re-sort of the three H = 1 fragments, zero past a head's last tile
  i32x4 qf[H * NS];
  const int klane = (kq * 128 + qi) << 4;            // this lane's place inside a group of four K chunks
  {
    i32x4 q1[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) q1[g] = *(const i32x4*)(a.qfrag + ((((tile0 + qt) * 8 + wave) * 3 + g) * 64 + lane) * 16);
#pragma unroll
    for (int hd = 0; hd < H; ++hd)
#pragma unroll
      for (int ks = 0; ks < NS; ++ks)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int c = hd * NC + 4 * ks + d;
          qf[hd * NS + ks][d] = 4 * ks + d < NC ? q1[c >> 2][c & 3] : 0;
        }
  }
  // one step of a pass (step = pass * nkt + kt): the K tile of a step sits in ring slot step & 1 with its DMA waited for
  // here; the next step's tile goes out after the barrier (the last step of a pass prefetches tile 0 for the next pass)
  auto next_tile = [&](int step, int kt, bool more) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nx = kt + 1 < nkt ? kt + 1 : 0;
    if (more) stage(kimg + (size_t)nx * L::KB, L::K + ((step + 1) & 1) * L::KB);
  };

  // ---------------- sweep 1: per head the minimum and maximum of the raw accumulators, all heads inside the key-tile step
  int mx[H], mn[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) { mx[hd] = (int)0x80000000; mn[hd] = 0x7fffffff; }
  for (int kt = 0; kt < nkt; ++kt) {
    next_tile(kt, kt, true);
    ita_long_heads_qk<H, H>(lds + L::K + (kt & 1) * L::KB, qf, klane, 0, [&](int hd, int, const i32x4& acc) {
      mx[hd] = max(max(mx[hd], acc[0]), acc[1]);           // (v_max3_i32, v_min3_i32)
      mx[hd] = max(max(mx[hd], acc[2]), acc[3]);
      mn[hd] = min(min(mn[hd], acc[0]), acc[1]);
      mn[hd] = min(min(mn[hd], acc[2]), acc[3]);
    });
  }
  // per head and row: both ends into the workgroup's range (rg was set in front of sweep 1's barriers), the maximum
  // requantised and clamped as the attention kernel does it -- one register of state per head from here on
  unsigned mrow[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int mxr = max1632_i(mx[hd]), mnr = ~max1632_i(~mn[hd]);   // (~ reverses the order of int32)
    if (kq == 0) {
      atomicMin(rg + 2 * hd, mnr);
      atomicMax(rg + 2 * hd + 1, mxr);
    }
    const int m = (int)(lh_lg16<FAST>(mxr, a.ml) & 0xffffu);
    mrow[hd] = (unsigned)min(max(m, 32768 - 128), 32768 + 127);
  }
  const u16x2 one = {256, 256}, one1 = {1, 1};
  const u16x2 lo = {32768 - 128, 32768 - 128}, hi = {32768 + 127, 32768 + 127};
  const bool want_l = a.logits != nullptr, want_s = a.shifts != nullptr, want_p = a.probs != nullptr;   // (uniform)
  // ---------------- sweep 2: one pass over the key tiles per head
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const unsigned short m = (unsigned short)mrow[hd], capv = (unsigned short)min((int)m - (32768 - 128), 15);
    const u16x2 mm = {m, m}, cap = {capv, capv};
    int sumlo = 0, below = 0, above = 0;
    for (int kt = 0; kt < nkt; ++kt) {
      const int step = (1 + hd) * nkt + kt;
      next_tile(step, kt, hd + 1 < H || kt + 1 < nkt);
      u16x2 s2 = {0, 0}, b2 = {0, 0}, a2 = {0, 0};
      ita_long_heads_qk<H, 1>(lds + L::K + (step & 1) * L::KB, qf, klane, hd, [&](int, int j, const i32x4& acc) {
        if (j == 0) s2 = b2 = a2 = (u16x2){0, 0};
        const u16x2 w[2] = {lh_lg16x2<FAST>(acc[0], acc[1], a.ml), lh_lg16x2<FAST>(acc[2], acc[3], a.ml)};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[t]), cap);
          b2 += __builtin_elementwise_min(__builtin_elementwise_sub_sat(lo, w[t]), one1);    // 1 where w < 32768 - 128
          a2 += __builtin_elementwise_min(__builtin_elementwise_sub_sat(w[t], hi), one1);    // 1 where w > 32768 + 127
          const u16x2 c = __builtin_elementwise_min(__builtin_elementwise_max(w[t], lo), hi);
          const u16x2 cb = c - lo, sh = mm - c;               // both 0 .. 255: m is the clamped maximum of the row
          if (want_l) {
            atomicAdd(hl + cb.x, 1u);
            atomicAdd(hl + cb.y, 1u);
          }
          if (want_s) {
            atomicAdd(hs + sh.x, 1u);
            atomicAdd(hs + sh.y, 1u);
          }
          if (want_p) {
            if (sh.x < 8) atomicAdd(rc + sh.x, 1u);
            if (sh.y < 8) atomicAdd(rc + sh.y, 1u);
          }
        }
        if (j == 7) {
          sumlo += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile and lane
          below += (int)b2.x + (int)b2.y;       // <= 32 per tile and lane
          above += (int)a2.x + (int)a2.y;
        }
      });
    }
    const int sum = max(sum1632_i(sumlo), 1);
    const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;      // <= 255: the row maximum alone adds 256
    __syncthreads();       // every wave's adds of this head are in the tables
    // probabilities: lane (qi, kq) takes the classes 2 kq, 2 kq + 1 of its query and clears them; lane kq = 0 the keys beyond class 7
    if (want_p) {
      const unsigned c0 = rc[2 * kq], c1 = rc[2 * kq + 1];
      rc[2 * kq] = 0;
      rc[2 * kq + 1] = 0;
      if (c0) atomicAdd(hp + ((inv_hi & 255) >> (2 * kq)), c0);      // (& 255 changes nothing: it keeps the index inside the table)
      if (c1) atomicAdd(hp + ((inv_hi & 255) >> (2 * kq + 1)), c1);
      const int seen = sum1632_i((int)(c0 + c1));
      if (kq == 0 && seen < a.S) atomicAdd(hp, (unsigned)(a.S - seen));
    }
    below = (int)ita_row16_sum((unsigned)sum1632_i(below));     // the wave's total in every lane: <= 16 S <= 2^20
    above = (int)ita_row16_sum((unsigned)sum1632_i(above));
    __syncthreads();       // the probability histogram is whole
    // the workgroup's counts into the frame's bins of head hd: threads 0 .. 255 logits and probabilities, 256 .. 511 shifts;
    // every word is cleared by the one thread that read it, in front of the next pass's first barrier
    {
      const size_t at = ((size_t)b * H + hd) * 256;
      const int bin = tid & 255;
      unsigned* t8 = (unsigned*)(lds + (tid < 256 ? L::HL : L::HS)) + bin;
      unsigned v = 0;
#pragma unroll
      for (int wv = 0; wv < 8; ++wv) {
        v += t8[wv * 256];
        t8[wv * 256] = 0;
      }
      unsigned long long* dst = tid < 256 ? a.logits : a.shifts;
      if (dst && v) atomicAdd(dst + at + bin, (unsigned long long)v);
      if (tid < 256 && want_p) {
        const unsigned pv = hp[bin];
        hp[bin] = 0;
        if (pv) atomicAdd(a.probs + at + bin, (unsigned long long)pv);
      }
    }
    if (lane == 0 && a.logits_out) {
      if (below) atomicAdd(a.logits_out + ((size_t)b * H + hd) * 2, (unsigned long long)below);
      if (above) atomicAdd(a.logits_out + ((size_t)b * H + hd) * 2 + 1, (unsigned long long)above);
    }
  }
  // (many barriers behind the range's LDS atomics)
  if (tid < H && a.acc_range) {
    atomicMin(a.acc_range + ((size_t)b * H + tid) * 2, rg[2 * tid] - ITA_ACC_BIAS);
    atomicMax(a.acc_range + ((size_t)b * H + tid) * 2 + 1, rg[2 * tid + 1] - ITA_ACC_BIAS);
  }
}

template <bool FAST, int H>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) ITA_NO_PK_F32 void ita_long_heads_hist_kernel(
    const ItaLongHistArgs a) {
  ita_long_heads_hist_body<FAST, H>(a);
}
