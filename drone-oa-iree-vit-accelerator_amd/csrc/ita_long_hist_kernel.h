// ita_long_hist_kernel.h -- histograms of the logits, the softmax shifts and the u8 probabilities of the whole S x S matrix
// of the long int8 attention, and the range of its raw accumulators (ita_mha_long_int8_hist).  The matrix is never held: the
// kernel runs behind the unchanged production projection launch (ita_long_proj_kernel<FAST, E, true>), reads only that
// launch's workspace -- the Q fragments and the K images, so E does not appear here -- and makes TWO sweeps over the key tiles:
//     sweep 1: row maximum AND minimum of the raw accumulators (ita_long_logits_minmax: a third epilogue on ita_long_qk_tile);
//              the maximum is requantised once per row as in ita_long_attn_body, both feed acc_range without ITA_ACC_BIAS
//     sweep 2: the biased, unclamped 16-bit logits w (ita_long_logits).  From the same word come the clamped logit bin
//              c = clamp(w) - (32768 - 128), the counts of w below / above the int8 range (what the clamp changed), the shift
//              bin s = m - clamp(w) (0 .. 255: the definition's max - logit, NOT the softmax's capped shift), the row sum of
//              256 >> min(shift, cap) exactly as ita_long_attn_body forms it, and per query row the counts of the shift
//              classes s = 0 .. 7
// There is no third sweep: a probability is inv_hi >> min(s, 15) with inv_hi <= 255 (the row maximum itself adds 256 to the
// row sum), so it is 0 from s = 8 on and a row's probabilities are inv_hi >> s, s = 0 .. 7, each as often as its shift class
// occurs, and 0 for every other key.  Once the row sum is whole, eight adds per row put the classes into the probability
// histogram and one adds the row's remaining keys to bin 0.
// Same grid as ita_long_stats_kernel: (S / 128, B), 512 threads, wave w owns queries 16 w .. 16 w + 15 of its query tile,
// K tiles by LDS-DMA into the two-slot ring; stage and next_tile stay lambdas (ita_long_stats_kernel.h says why).
//
// Counting.  One LDS atomic add per logit and histogram, into 32-bit sub-histograms per wave (two tables of 8 x 256
// words): a lane's 32 logits of a tile belong to one query and four lanes share a query, so the 64 adds of one instruction
// are 16 queries against four keys and a hot bin (the clamp ends, the large shifts) serialises inside a wave only.  The
// class counts go to a table of 128 rows x 8 classes whose rows only the owning wave touches (at most the four lanes of a
// query meet in one word).  A workgroup sees 128 S <= 2^23 entries, so nothing 32-bit overflows; at the end the eight
// sub-histograms are summed per bin and added to the frame's int64 bins with 64-bit integer global atomics, the range with
// integer atomic min / max.  Integer addition, minimum and maximum are order-independent: the same bytes on every call.
// The entry sets the outputs to 0 (acc_range to INT_MAX, INT_MIN) with a small kernel before the launch.
// A null pointer skips that output's adds and stores.  ITA_LONG_HIST_ABLATE = 1 is a timing-only build without the LDS
// histogram adds of sweep 2 (its counts are wrong): the share of the time the counting costs (tools/bench_long_hist.py).
#pragma once
#include "ita_long_attn_kernel.h"

#ifndef ITA_LONG_HIST_ABLATE
#define ITA_LONG_HIST_ABLATE 0
#endif

struct ItaLongHistArgs {
  const char* qfrag;      // ita_long_proj_kernel's workspace: Q fragments (B, S/16, 3, 64 lanes, 16 B)
  const char* kimg;       //                                   K images (B, S/128, 24576)
  float ml;
  int B, S;
  unsigned long long *logits, *shifts, *probs;   // (B, 256) each, zero before the launch; any may be null
  unsigned long long* logits_out;                // (B, 2): below, above; zero before the launch
  int* acc_range;                                // (B, 2): INT_MAX, INT_MIN before the launch
};

// 69 KB of LDS: the two-slot K ring, the per-wave logit and shift sub-histograms, the rows' shift classes, the workgroup's
// probability histogram and its accumulator range.  Two workgroups per CU, as the statistics kernel.
struct ItaLongHistLds {
  static constexpr int KB = ItaLongLds::KB;
  static constexpr int K = 0;
  static constexpr int HL = 2 * KB;                    // u32 [8 waves][256]: clamped logit + 128
  static constexpr int HS = HL + 8 * 256 * 4;          // u32 [8 waves][256]: row maximum - clamped logit
  static constexpr int RC = HS + 8 * 256 * 4;          // u32 [128 rows][8]: keys of the row at shift 0 .. 7
  static constexpr int HP = RC + 128 * 8 * 4;          // u32 [256]: probabilities
  static constexpr int RG = HP + 256 * 4;              // i32 [2]: minimum, maximum of the biased accumulators (+ 2 words unused)
  static constexpr int TOTAL = RG + 16;
  static constexpr int WORDS = (TOTAL - HL) / 4;       // everything behind the ring
  static_assert(2 * TOTAL <= 160 * 1024, "two workgroups per CU");
};

// The outputs start from zero and the range from (INT_MAX, INT_MIN): one thread per bin of a frame.  A kernel and not a
// memset, as ita_long_stats_zero_kernel: a captured call is kernel nodes only.
__global__ __launch_bounds__(256) void ita_long_hist_zero_kernel(const ItaLongHistArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;   // (grid = B)
  if (a.logits) a.logits[i] = 0;
  if (a.shifts) a.shifts[i] = 0;
  if (a.probs) a.probs[i] = 0;
  if (threadIdx.x < 2) {
    const size_t j = (size_t)blockIdx.x * 2 + threadIdx.x;
    if (a.logits_out) a.logits_out[j] = 0;
    if (a.acc_range) a.acc_range[j] = threadIdx.x ? (int)0x80000000 : 0x7fffffff;
  }
}

// ita_long_logits_max that also keeps the running minimum of this lane's accumulators
__device__ __forceinline__ void ita_long_logits_minmax(const char* kb, const i32x4 (&qf)[3], int kq, int qi, int& mn, int& mx) {
  ita_long_qk_tile(kb, qf, kq, qi, [&](int, const i32x4 (&acc)[2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      mx = max(max(mx, acc[t][0]), acc[t][1]);           // (v_max3_i32, v_min3_i32)
      mx = max(max(mx, acc[t][2]), acc[t][3]);
      mn = min(min(mn, acc[t][0]), acc[t][1]);
      mn = min(min(mn, acc[t][2]), acc[t][3]);
    }
  });
}

template <bool FAST>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void ita_long_hist_kernel(const ItaLongHistArgs a) {
  using L = ItaLongHistLds;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nkt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const size_t tile0 = (size_t)b * nkt;              // first tile index of this frame
  const char* kimg = a.kimg + tile0 * L::KB;
  [[maybe_unused]] unsigned* hl = (unsigned*)(lds + L::HL) + wave * 256;   // (unused in the ablation build)
  [[maybe_unused]] unsigned* hs = (unsigned*)(lds + L::HS) + wave * 256;
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
  for (int i = tid; i < L::WORDS; i += 512) ((unsigned*)(lds + L::HL))[i] = 0;   // (first used behind sweep 1's barriers)
  i32x4 qf[3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) qf[ks] = *(const i32x4*)(a.qfrag + ((((tile0 + qt) * 8 + wave) * 3 + ks) * 64 + lane) * 16);

  auto logits = [&](const char* kb, u16x2 (&w)[16]) { ita_long_logits<FAST>(kb, qf, kq, qi, a.ml, w); };
  // one step of a sweep (step = sweep * nkt + kt): the K tile of a step sits in ring slot step & 1 with its DMA waited for
  // here; the next step's tile goes out after the barrier (the last step of sweep 1 prefetches tile 0 for sweep 2)
  auto next_tile = [&](int step, int kt, bool more) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nx = kt + 1 < nkt ? kt + 1 : 0;
    if (more) stage(kimg + (size_t)nx * L::KB, L::K + ((step + 1) & 1) * L::KB);
  };

  // ---------------- sweep 1: row maximum and minimum of the raw accumulators, one value per row requantised
  int mx = (int)0x80000000, mn = 0x7fffffff;
  for (int kt = 0; kt < nkt; ++kt) {
    next_tile(kt, kt, true);
    ita_long_logits_minmax(lds + L::K + (kt & 1) * L::KB, qf, kq, qi, mn, mx);
  }
  if (tid == 0) { rg[0] = 0x7fffffff; rg[1] = (int)0x80000000; }   // (zeroed above, in front of sweep 1's barriers)
  mx = max1632_i(mx);
  mn = ~max1632_i(~mn);                                // (~ reverses the order of int32)
  int m;
  {
    const i32x4 am[2] = {(i32x4){mx, mx, mx, mx}, (i32x4){mx, mx, mx, mx}};
    unsigned w4[4];
    if constexpr (FAST) lg8_v3<ITA_RQ_FAST>(am, a.ml, w4);
    else lg8_v3<ITA_RQ_EXACT>(am, a.ml, w4);
    m = (int)(w4[0] & 0xffffu);
  }
  m = min(max(m, 32768 - 128), 32768 + 127);
  const u16x2 mm = {(unsigned short)m, (unsigned short)m};
  const unsigned short capv = (unsigned short)min(m - (32768 - 128), 15);
  const u16x2 cap = {capv, capv}, one = {256, 256};
  const u16x2 lo = {32768 - 128, 32768 - 128}, hi = {32768 + 127, 32768 + 127}, one1 = {1, 1};
  [[maybe_unused]] const bool want_l = a.logits != nullptr, want_s = a.shifts != nullptr;   // (uniform)
  const bool want_p = a.probs != nullptr;
  // ---------------- sweep 2: logits -> bins, row sum (the ring slot of tile kt is (nkt + kt) & 1)
  int sumlo = 0, below = 0, above = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = nkt + kt;
    next_tile(step, kt, kt + 1 < nkt);
    if (kt == 0 && kq == 0) {          // behind a barrier that follows tid 0's two stores: the workgroup's range, one lane per row
      atomicMin(rg, mn);
      atomicMax(rg + 1, mx);
    }
    u16x2 w[16];
    logits(lds + L::K + (step & 1) * L::KB, w);
    u16x2 s2 = {0, 0}, b2 = {0, 0}, a2 = {0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[j]), cap);
      b2 += __builtin_elementwise_min(__builtin_elementwise_sub_sat(lo, w[j]), one1);    // 1 where w < 32768 - 128
      a2 += __builtin_elementwise_min(__builtin_elementwise_sub_sat(w[j], hi), one1);    // 1 where w > 32768 + 127
    }
    sumlo += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile and lane
    below += (int)b2.x + (int)b2.y;
    above += (int)a2.x + (int)a2.y;
#if !ITA_LONG_HIST_ABLATE
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const u16x2 c = __builtin_elementwise_min(__builtin_elementwise_max(w[j], lo), hi);
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
#endif
  }
  int sum = sum1632_i(sumlo);
  sum = max(sum, 1);
  const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;      // <= 255: sum >= 256
  __syncthreads();       // every wave's adds are in the tables
  // ---------------- probabilities: lane (qi, kq) takes the classes 2 kq, 2 kq + 1 of its query; lane kq = 0 the keys beyond class 7
  if (want_p) {
    const unsigned c0 = rc[2 * kq], c1 = rc[2 * kq + 1];
    if (c0) atomicAdd(hp + ((inv_hi & 255) >> (2 * kq)), c0);      // (& 255 changes nothing: it keeps the index inside the table)
    if (c1) atomicAdd(hp + ((inv_hi & 255) >> (2 * kq + 1)), c1);
    const int seen = sum1632_i((int)(c0 + c1));
    if (kq == 0 && seen < a.S) atomicAdd(hp, (unsigned)(a.S - seen));
  }
  below = (int)ita_row16_sum((unsigned)sum1632_i(below));     // the wave's total in every lane: <= 16 S <= 2^20
  above = (int)ita_row16_sum((unsigned)sum1632_i(above));
  __syncthreads();       // the probability histogram is whole
  // ---------------- the workgroup's counts into the frame's: threads 0 .. 255 logits and probabilities, 256 .. 511 shifts
  {
    const int bin = tid & 255;
    const unsigned* t8 = (const unsigned*)(lds + (tid < 256 ? L::HL : L::HS)) + bin;
    unsigned v = 0;
#pragma unroll
    for (int wv = 0; wv < 8; ++wv) v += t8[wv * 256];
    unsigned long long* dst = tid < 256 ? a.logits : a.shifts;
    if (dst && v) atomicAdd(dst + (size_t)b * 256 + bin, (unsigned long long)v);
    if (tid < 256 && a.probs && hp[bin]) atomicAdd(a.probs + (size_t)b * 256 + bin, (unsigned long long)hp[bin]);
  }
  if (lane == 0 && a.logits_out) {
    if (below) atomicAdd(a.logits_out + (size_t)b * 2, (unsigned long long)below);
    if (above) atomicAdd(a.logits_out + (size_t)b * 2 + 1, (unsigned long long)above);
  }
  if (tid == 0 && a.acc_range) {
    atomicMin(a.acc_range + (size_t)b * 2, rg[0] - ITA_ACC_BIAS);
    atomicMax(a.acc_range + (size_t)b * 2 + 1, rg[1] - ITA_ACC_BIAS);
  }
}
