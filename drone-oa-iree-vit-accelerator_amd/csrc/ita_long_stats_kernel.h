// ita_long_stats_kernel.h -- row and column statistics of the whole S x S probability matrix of the long int8 attention
// (ita_mha_long_int8_stats).  The matrix is never held: the kernel runs behind the unchanged production projection launch
// (ita_long_proj_kernel<FAST, E, true>), reads only that launch's workspace -- the Q fragments and the K images, so E does
// not appear here (P = 192 at either E) -- and repeats the three sweeps of ita_long_attn_body over the key tiles:
//     sweep 1: row maximum of the raw accumulators, one requantised value per row          (as ita_long_attn_body)
//     sweep 2: row sum of 256 >> (max - x) in 16-bit pairs, inv_hi                          (as ita_long_attn_body)
//     sweep 3: the same p4 words of four u8 probabilities -- and instead of feeding the A.V MFMA they are reduced
// There is no V staging, no second barrier per step and no out_proj.  Same grid as ita_long_attn_kernel: (S / 128, B), 512
// threads, wave w owns queries 16 w .. 16 w + 15 of its query tile, K tiles by LDS-DMA into the two-slot ring.
//
// The K Q^T tile pipeline and its two epilogues are ita_long_attn_kernel.h's (ita_long_logits, ita_long_logits_max): the
// logits of both kernels come from one routine.  stage and next_tile stay lambdas in both files: shared as a function,
// in either form, they change the production kernels' instruction streams ("Long attention, shared").
//
// Lane (qi = lane & 15, kq = lane >> 4) of wave w holds, per key tile, eight words p4[k4], k4 = 4 kb + t: byte i is the
// probability of key 64 kb + 16 t + 4 kq + i = 4 (4 k4 + kq) + i of the tile for query 16 w + qi.
//   rows:    mass += udot4(p4, 1 1 1 1), nnz += udot4(byte-is-non-zero mask, 1 1 1 1) per lane over all key tiles; summed
//            over the four kq lanes of a query at the end (sum1632_i); lane kq = 0 stores the query's four values
//   columns: per key tile the bytes are summed over the 16 queries of the wave by four rotate-and-add steps inside the
//            16-lane rows (masses as two 16-bit pairs per word, <= 16 * 255 < 2^12; non-zero flags stay bytes, <= 16); lane
//            qi = 0 of each row adds the 24 words into the workgroup's LDS table with LDS atomics -- still packed: eight
//            waves give <= 32 640 per 16-bit half and <= 128 per byte -- and after the NEXT step's barrier waves 0..3 unpack
//            the table (two slots, by tile parity), clear it and add 128 masses and 128 counts to col_mass / col_nnz with
//            vector global atomics, 64 consecutive int32 per instruction.  Integer addition is order-independent: the result
//            is the same bit for bit on every run.  The entry zeroes the two column arrays before the launch.
// A null pointer skips that statistic's stores (not its arithmetic).  Every store is at (b, token < S) of the call.
#pragma once
#include "ita_long_attn_kernel.h"

struct ItaLongStatsArgs {
  const char* qfrag;      // ita_long_proj_kernel's workspace: Q fragments (B, S/16, 3, 64 lanes, 16 B)
  const char* kimg;       //                                   K images (B, S/128, 24576)
  float ml;
  int B, S;
  int8_t* row_max;        // (B, S) each; any may be null
  int *row_sum, *row_mass, *row_nnz;
  int *col_mass, *col_nnz;   // zero before the launch
};

// 49 KB of LDS: the two-slot K ring and the packed column table (two slots of 64 mass words and 32 count words).  Two
// workgroups per CU at 105 registers: a third (amdgpu_waves_per_eu(6, 6), 80 registers) spills 28 and measured 12 % slower.
struct ItaLongStatsLds {
  static constexpr int KB = ItaLongLds::KB;
  static constexpr int K = 0;
  static constexpr int CM = 2 * KB;                    // u32 [2][64]: word 2 g + h of a slot = keys 4 g + h, 4 g + h + 2 (low, high half)
  static constexpr int CN = CM + 2 * 64 * 4;           // u32 [2][32]: byte i of word g = key 4 g + i
  static constexpr int TOTAL = CN + 2 * 32 * 4;
  static_assert(2 * TOTAL <= 160 * 1024, "two workgroups per CU");
};

// The column arrays start from zero: n int32 of each (either may be null), one int32 per lane and grid-stride step -- the
// arrays are only 4-byte aligned.  A kernel and not a memset, so that a captured call is kernel nodes only: a memset node in
// front of the launches did not survive the second replay of a captured call ("Long-sequence statistics").
__global__ __launch_bounds__(256) void ita_long_stats_zero_kernel(int* c0, int* c1, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if (c0) c0[i] = 0;
    if (c1) c1[i] = 0;
  }
}

template <bool FAST>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void ita_long_stats_kernel(const ItaLongStatsArgs a) {
  using L = ItaLongStatsLds;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nkt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const size_t tile0 = (size_t)b * nkt;              // first tile index of this frame
  const char* kimg = a.kimg + tile0 * L::KB;
  unsigned* cm = (unsigned*)(lds + L::CM);
  unsigned* cn = (unsigned*)(lds + L::CN);

  auto stage = [&](const char* src, int ldsoff) {    // 24 KB by LDS-DMA: three 1 KB pieces per wave
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int piece = wave + 8 * q;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + ldsoff + piece * 1024), 16, 0, 0);
    }
  };
  stage(kimg, L::K);
  if (tid < 2 * 64 + 2 * 32) cm[tid] = 0;            // (CM and CN are adjacent; first used behind many barriers)
  i32x4 qf[3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) qf[ks] = *(const i32x4*)(a.qfrag + ((((tile0 + qt) * 8 + wave) * 3 + ks) * 64 + lane) * 16);

  auto logits = [&](const char* kb, u16x2 (&w)[16]) { ita_long_logits<FAST>(kb, qf, kq, qi, a.ml, w); };
  auto logits_max = [&](const char* kb, int& mx) { ita_long_logits_max(kb, qf, kq, qi, mx); };
  // one step of sweeps 1 and 2 (step = sweep * nkt + kt): the K tile of a step sits in ring slot step & 1 with its DMA waited
  // for here; the next step's tile goes out after the barrier (the last step of a sweep prefetches tile 0 for the next sweep)
  auto next_tile = [&](int step, int kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nx = kt + 1 < nkt ? kt + 1 : 0;
    stage(kimg + (size_t)nx * L::KB, L::K + ((step + 1) & 1) * L::KB);
  };

  // ---------------- sweep 1: row maximum of the raw accumulators, one value per row requantised
  int mx = (int)0x80000000;
  for (int kt = 0; kt < nkt; ++kt) {
    next_tile(kt, kt);
    logits_max(lds + L::K + (kt & 1) * L::KB, mx);
  }
  mx = max1632_i(mx);
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
  // ---------------- sweep 2: row sum (the ring slot of tile kt is (sweep * nkt + kt) & 1)
  int sumlo = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = nkt + kt;
    next_tile(step, kt);
    u16x2 w[16];
    logits(lds + L::K + (step & 1) * L::KB, w);
    u16x2 s2 = {0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[j]), cap);
    sumlo += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile and lane
  }
  int sum = sum1632_i(sumlo);
  sum = max(sum, 1);
  const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;
  const u16x2 iv = {(unsigned short)inv_hi, (unsigned short)inv_hi};
  // ---------------- sweep 3: probabilities, reduced along the rows (registers) and along the columns (LDS table, global atomics)
  // tile kt's column table is complete behind the barrier of the step after it: waves 0, 1 take its 128 masses, waves 2, 3 its
  // 128 counts, clear the words (every reader of a word sits in the clearing wave) and add them to the frame's arrays
  auto flush = [&](int kt) {
    if (wave < 4) {
      const int k = tid & 127, slot = kt & 1;
      const size_t at = (size_t)b * a.S + (size_t)kt * 128 + k;
      if (wave < 2) {
        unsigned* p = cm + slot * 64 + (k >> 2) * 2 + (k & 1);
        const unsigned v = *p;
        *p = 0;
        if (a.col_mass) atomicAdd(a.col_mass + at, (int)((k & 2) ? v >> 16 : v & 0xffffu));
      } else {
        unsigned* p = cn + slot * 32 + (k >> 2);
        const unsigned v = *p;
        *p = 0;
        if (a.col_nnz) atomicAdd(a.col_nnz + at, (int)((v >> (8 * (k & 3))) & 0xffu));
      }
    }
  };
  unsigned mass = 0, nnz = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = 2 * nkt + kt;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // K tile kt landed; every wave is done with the previous step: its column table is complete, the other K slot free
    if (kt + 1 < nkt) stage(kimg + (size_t)(kt + 1) * L::KB, L::K + ((step + 1) & 1) * L::KB);
    if (kt > 0) flush(kt - 1);
    u16x2 w[16];
    logits(lds + L::K + (step & 1) * L::KB, w);
    unsigned lo[8], hi[8], nz[8];
#pragma unroll
    for (int k4 = 0; k4 < 8; ++k4) {
      const u16x2 s0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[2 * k4]), cap);
      const u16x2 s1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[2 * k4 + 1]), cap);
      const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s0));
      const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s1));
      const unsigned p4 = __builtin_amdgcn_perm(p23, p01, 0x06040200u);   // u8 probabilities of keys 4 (4 k4 + kq) + 0..3
      const unsigned f4 = (((p4 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | p4) >> 7 & 0x01010101u;   // 1 where the byte is non-zero
      mass = __builtin_amdgcn_udot4(p4, 0x01010101u, mass, false);
      nnz = __builtin_amdgcn_udot4(f4, 0x01010101u, nnz, false);
      lo[k4] = ita_row16_sum(p4 & 0x00ff00ffu);          // keys + 0, + 2 over the wave's 16 queries
      hi[k4] = ita_row16_sum((p4 >> 8) & 0x00ff00ffu);   // keys + 1, + 3
      nz[k4] = ita_row16_sum(f4);
    }
    if (qi == 0) {
      const int slot = kt & 1;
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4) {
        atomicAdd(cm + slot * 64 + (4 * k4 + kq) * 2, lo[k4]);
        atomicAdd(cm + slot * 64 + (4 * k4 + kq) * 2 + 1, hi[k4]);
        atomicAdd(cn + slot * 32 + 4 * k4 + kq, nz[k4]);
      }
    }
  }
  __syncthreads();       // the last tile's column table is complete
  flush(nkt - 1);
  mass = (unsigned)sum1632_i((int)mass);
  nnz = (unsigned)sum1632_i((int)nnz);
  if (kq == 0) {
    const size_t row = (size_t)b * a.S + (size_t)qt * 128 + wave * 16 + qi;
    if (a.row_max) a.row_max[row] = (int8_t)(m - 32768);
    if (a.row_sum) a.row_sum[row] = sum;
    if (a.row_mass) a.row_mass[row] = (int)mass;
    if (a.row_nnz) a.row_nnz[row] = (int)nnz;
  }
}
