// ita_long_heads_stats_kernel.h -- row and column statistics of the H whole S x S probability matrices of the long int8
// attention with H = 2, 3, 4 or 6 heads (ita_mha_long_heads_int8_stats): ita_long_stats_kernel's reductions on
// ita_long_heads_attn_kernel's probabilities.  No matrix is held: the kernel runs behind the unchanged production
// projection launch on the layer's own image (Layer::limg_mha), reads only that launch's workspace -- the Q fragments and
// the K images, so E does not appear here -- and repeats the three sweeps of ita_long_heads_attn_body over the key tiles.
//
// Work split: grid (S / 128, B), 512 threads, wave w owns queries 16 w .. 16 w + 15 of its query tile, K tiles by LDS-DMA
// into the two-slot ring, ONE barrier per key-tile step (no V staging, no out_proj).  The heads run INSIDE the key-tile
// step, as in the attention kernel: a staged 24 KB K tile serves all H heads before the ring moves on.
//   fragments  ita_long_heads_qk's: the head Q fragments (H NS of them, zero dwords past a head's last tile) and the
//              dword-gathered K fragments of the unchanged tile image
//   sweep 1, 2 the attention kernel's: H running maxima of the raw accumulators, H row sums in 16-bit pairs, one pipeline
//              over the 8 H key blocks of a tile; per head ONE register of softmax state (biased maximum | inv_hi << 16)
//   sweep 3    head by head: the p4 words of four u8 probabilities as the attention kernel forms them for A.V (lh_lg16x2
//              under ITA_NO_PK_F32: the statistics are those of the probabilities production multiplies with V), reduced
//              as ita_long_stats_kernel reduces them.  Lane (qi, kq), key block j: byte i of p4 <-> key 16 j + 4 kq + i.
//     rows     mass[hd] += udot4(p4, 1 1 1 1), nnz[hd] += udot4(non-zero mask, 1 1 1 1) per lane: 2 H accumulators, summed
//              over the four kq lanes at the end; lane kq = 0 stores the query's values at (b, hd, token)
//     columns  per key tile and head the rotate-and-add over the wave's 16 queries (masses as two 16-bit halves per word,
//              <= 16 * 255; counts as bytes, <= 16); lane qi = 0 of each row adds the head's 24 words into the workgroup's
//              packed LDS table -- two slots by tile parity, H x (64 + 32) words per slot; every head has its own words, so
//              the bounds are the one-head kernel's: 8 waves x 16 x 255 = 32 640 < 2^16 per half, <= 128 per byte.  Behind
//              the NEXT step's barrier all eight waves unpack the slot, clear it and add 256 H values to col_mass /
//              col_nnz (B, H, S) with vector global integer atomics (col_mass <= 255 * 65 536 < 2^24).  Integer addition
//              has no order: the same bytes on every call.  The entry zeroes the two column arrays before the launch.
// A null pointer skips that statistic's stores (not its arithmetic).  Every store is at (b, hd < H, token < S) of the call.
#pragma once
#include "ita_long_heads_kernel.h"
#include "ita_long_stats_kernel.h"

struct ItaLongHeadsStatsArgs {
  const char* qfrag;      // ita_long_proj_kernel's workspace: Q fragments (B, S/16, 3, 64 lanes, 16 B)
  const char* kimg;       //                                   K images (B, S/128, 24576)
  float ml;
  int B, S;
  int8_t* row_max;        // (B, H, S) each; any may be null
  int *row_sum, *row_mass, *row_nnz;
  int *col_mass, *col_nnz;   // zero before the launch
};

// The two-slot K ring and the packed column table: [2 slots][H heads][64 mass words | 32 count words].  Mass word 2 g + h
// of a head = keys 4 g + h (low half) and 4 g + h + 2 (high half); byte i of count word g = key 4 g + i.  4.6 KB at H = 6
// on top of the 48 KB ring: two workgroups per CU.
template <int H>
struct ItaLongHeadsStatsLds {
  static constexpr int KB = ItaLongLds::KB;
  static constexpr int K = 0;
  static constexpr int CT = 2 * KB;
  static constexpr int HEAD_WORDS = 64 + 32, SLOT_WORDS = H * HEAD_WORDS;
  static constexpr int TOTAL = CT + 2 * SLOT_WORDS * 4;
  static_assert(2 * TOTAL <= 160 * 1024, "two workgroups per CU");
};

// (a body of its own, inlined into the kernel as a whole: a lambda called from the kernel itself would not inline across
// the kernel's no-packed-fp32 target attribute, as in ita_long_heads_kernel.h)
template <bool FAST, int H>
__device__ __forceinline__ void ita_long_heads_stats_body(const ItaLongHeadsStatsArgs& a) {
  static_assert(H == 2 || H == 3 || H == 4 || H == 6, "the head counts check_blob admits besides 1");
  constexpr int NC = 12 / H, NS = (NC + 3) / 4;
  using L = ItaLongHeadsStatsLds<H>;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nkt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const size_t tile0 = (size_t)b * nkt;              // first tile index of this frame
  const char* kimg = a.kimg + tile0 * L::KB;
  unsigned* ct = (unsigned*)(lds + L::CT);

  auto stage = [&](const char* src, int ldsoff) {    // 24 KB by LDS-DMA: three 1 KB pieces per wave
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int piece = wave + 8 * q;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + ldsoff + piece * 1024), 16, 0, 0);
    }
  };
  stage(kimg, L::K);
  for (int i = tid; i < 2 * L::SLOT_WORDS; i += 512) ct[i] = 0;   // (first used behind many barriers)
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
  auto next_tile = [&](int step, int kt) {           // (the ring slot of a step is step & 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nx = kt + 1 < nkt ? kt + 1 : 0;
    stage(kimg + (size_t)nx * L::KB, L::K + ((step + 1) & 1) * L::KB);
  };

  // ---------------- sweep 1: H row maxima of the raw accumulators (requantisation is monotonic)
  int mx[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) mx[hd] = (int)0x80000000;
  for (int kt = 0; kt < nkt; ++kt) {
    next_tile(kt, kt);
    ita_long_heads_qk<H, H>(lds + L::K + (kt & 1) * L::KB, qf, klane, 0, [&](int hd, int, const i32x4& acc) {
      mx[hd] = max(max(mx[hd], acc[0]), acc[1]);
      mx[hd] = max(max(mx[hd], acc[2]), acc[3]);
    });
  }
  // per head: the clamped maximum as a biased u16 in the low half of mi[hd] (inv_hi joins it after sweep 2)
  unsigned mi[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int m = (int)(lh_lg16<FAST>(max1632_i(mx[hd]), a.ml) & 0xffffu);
    mi[hd] = (unsigned)min(max(m, 32768 - 128), 32768 + 127);
  }
  const u16x2 one = {256, 256};
  auto cap_of = [&](unsigned short m) { return (unsigned short)min((int)m - (32768 - 128), 15); };
  // ---------------- sweep 2: H row sums
  int sumlo[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) sumlo[hd] = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = nkt + kt;
    next_tile(step, kt);
    u16x2 s2 = {0, 0};
    ita_long_heads_qk<H, H>(lds + L::K + (step & 1) * L::KB, qf, klane, 0, [&](int hd, int j, const i32x4& acc) {
      const unsigned short m = (unsigned short)(mi[hd] & 0xffffu), cv = cap_of(m);
      const u16x2 mm = {m, m}, cap = {cv, cv};
      if (j == 0) s2 = (u16x2){0, 0};
      const u16x2 w0 = lh_lg16x2<FAST>(acc[0], acc[1], a.ml), w1 = lh_lg16x2<FAST>(acc[2], acc[3], a.ml);
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w0), cap);
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w1), cap);
      if (j == 7) sumlo[hd] += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile, head and lane
    });
  }
  const size_t row0 = (size_t)b * H * a.S + (size_t)qt * 128 + wave * 16 + qi;   // (b, 0, token); head hd is hd S further
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int sum = max(sum1632_i(sumlo[hd]), 1);
    const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;    // <= 255: the row maximum alone adds 256
    if (kq == 0) {
      if (a.row_max) a.row_max[row0 + (size_t)hd * a.S] = (int8_t)((int)(mi[hd] & 0xffffu) - 32768);
      if (a.row_sum) a.row_sum[row0 + (size_t)hd * a.S] = sum;
    }
    mi[hd] |= (unsigned)inv_hi << 16;
  }
  // ---------------- sweep 3: probabilities head by head, reduced along the rows (registers) and along the columns (LDS
  // table, global atomics).  Tile kt's table slot is complete behind the barrier of the step after it: thread t takes value
  // t & 255 (key t & 127; a mass in waves 0, 1, 4, 5, a count in the others) of the heads t >> 8, (t >> 8) + 2, ..., clears
  // the word (every reader of a word sits in the clearing wave) and adds the value to the frame's arrays
  auto flush = [&](int kt) {
    int k = tid & 127;
    asm volatile("" : "+v"(k));   // the addresses are formed here, per call: hoisted out of the key loop they cost registers the sweep needs
    unsigned* slot = ct + (kt & 1) * L::SLOT_WORDS;
    for (int hd = wave >> 2; hd < H; hd += 2) {      // (wave-uniform: scalar bases, one uniform branch)
      const size_t at = ((size_t)b * H + hd) * a.S + (size_t)kt * 128;
      if (!(wave & 2)) {
        unsigned* p = slot + hd * L::HEAD_WORDS + (k >> 2) * 2 + (k & 1);
        const unsigned v = *p;
        *p = 0;
        if (a.col_mass) atomicAdd(a.col_mass + at + k, (int)((k & 2) ? v >> 16 : v & 0xffffu));
      } else {
        unsigned* p = slot + hd * L::HEAD_WORDS + 64 + (k >> 2);
        const unsigned v = *p;
        *p = 0;
        if (a.col_nnz) atomicAdd(a.col_nnz + at + k, (int)((v >> (8 * (k & 3))) & 0xffu));
      }
    }
  };
  unsigned mass[H], nnz[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) mass[hd] = nnz[hd] = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = 2 * nkt + kt;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // K tile kt landed; every wave is done with the previous step: its table slot is complete, the other K slot free
    if (kt + 1 < nkt) stage(kimg + (size_t)(kt + 1) * L::KB, L::K + ((step + 1) & 1) * L::KB);
    if (kt > 0) flush(kt - 1);
#pragma unroll
    for (int hd = 0; hd < H; ++hd) {
      unsigned mih = mi[hd];
      asm volatile("" : "+v"(mih));   // unpacked here, per tile, as in the attention kernel: hoisted, the pairs cost 3 H registers
      const unsigned short m = (unsigned short)(mih & 0xffffu), cv = cap_of(m), ih = (unsigned short)(mih >> 16);
      const u16x2 mm = {m, m}, cap = {cv, cv}, iv = {ih, ih};
      unsigned lo[8], hi[8], nz[8];
      ita_long_heads_qk<H, 1>(lds + L::K + (step & 1) * L::KB, qf, klane, hd, [&](int, int j, const i32x4& acc) {
        const u16x2 s0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, lh_lg16x2<FAST>(acc[0], acc[1], a.ml)), cap);
        const u16x2 s1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, lh_lg16x2<FAST>(acc[2], acc[3], a.ml)), cap);
        const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s0));
        const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s1));
        const unsigned p4 = __builtin_amdgcn_perm(p23, p01, 0x06040200u);   // u8 probabilities of keys 16 j + 4 kq + 0..3
        const unsigned f4 = (((p4 & 0x7f7f7f7fu) + 0x7f7f7f7fu) | p4) >> 7 & 0x01010101u;   // 1 where the byte is non-zero
        mass[hd] = __builtin_amdgcn_udot4(p4, 0x01010101u, mass[hd], false);
        nnz[hd] = __builtin_amdgcn_udot4(f4, 0x01010101u, nnz[hd], false);
        lo[j] = ita_row16_sum(p4 & 0x00ff00ffu);          // keys + 0, + 2 over the wave's 16 queries
        hi[j] = ita_row16_sum((p4 >> 8) & 0x00ff00ffu);   // keys + 1, + 3
        nz[j] = ita_row16_sum(f4);
      });
      // (the row accumulators are complete HERE: left free, the sixteen udot4 of every head sink behind the branch below to the
      // end of the step, and their p4 / mask words stay live across all H heads)
      asm volatile("" : "+v"(mass[hd]), "+v"(nnz[hd]));
      if (qi == 0) {
        unsigned* t = ct + (kt & 1) * L::SLOT_WORDS + hd * L::HEAD_WORDS;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          atomicAdd(t + (4 * j + kq) * 2, lo[j]);
          atomicAdd(t + (4 * j + kq) * 2 + 1, hi[j]);
          atomicAdd(t + 64 + 4 * j + kq, nz[j]);
        }
      }
    }
  }
  __syncthreads();       // the last tile's table slot is complete
  flush(nkt - 1);
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int ms = sum1632_i((int)mass[hd]), nn = sum1632_i((int)nnz[hd]);
    if (kq == 0) {
      if (a.row_mass) a.row_mass[row0 + (size_t)hd * a.S] = ms;
      if (a.row_nnz) a.row_nnz[row0 + (size_t)hd * a.S] = nn;
    }
  }
}

template <bool FAST, int H>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) ITA_NO_PK_F32 void ita_long_heads_stats_kernel(
    const ItaLongHeadsStatsArgs a) {
  ita_long_heads_stats_body<FAST, H>(a);
}
