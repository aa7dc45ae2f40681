// ita_long_heads_prop_kernel.h -- weighted column sums of the H whole S x S probability matrices of the long int8 attention
// with H = 2, 3, 4 or 6 heads (ita_mha_long_heads_int8_propagate):
//     out[b, hd, r, j] = sum_i w[b, r, i] * p_hd[b, i, j]     w int8 (B, R, S), 1 <= R <= 64, shared by the heads;
//                                                             p_hd uint8; out int32 (B, H, R, S)
// with p_hd[b, i, j] the probability ita_long_heads_attn_body gives query i for key j in head hd
// (ita_mha_long_heads_int8_taps' probs).  No matrix is held.  col_mass of the heads statistics entry is w = all ones, a
// probability row of a head is w = one-hot.  ita_long_prop_kernel's transposed sweep on ita_long_heads_attn_kernel's
// probabilities; E does not appear behind the projection launch.
//
// The entry runs four launches over the long workspace:
//   ita_long_proj_kernel<FAST, E, true>        unchanged, on Layer::limg_mha: Q fragments and K images
//   ita_long_heads_rows_kernel<FAST, H>        sweeps 1 and 2 of every query and head, written straight into the
//                                              row-parameter images: 1 KB per frame, query tile and head
//   ita_long_heads_prop_wprep_kernel           the permuted weight images and 128 * row sums of w, once per call: the
//                                              weights do not depend on the head
//   ita_long_heads_prop_kernel<FAST, H, NG>    the TRANSPOSED sweep 3
//
// ita_long_heads_rows_kernel: ita_long_heads_stats_body's launch shape, K ring, fragments and first two sweeps -- the same
// ita_long_heads_qk<H, H> pipeline, the same maxima, sums and inv_hi expression -- and no sweep 3.  Lane kq = 0 of a query
// stores u16 m | cap | inv_hi | 0 of every head in ita_long_prop_prep_kernel's layout (per four queries m[4] | cap[4] |
// inv_hi[4] | 0[4]); the image of tile t and head hd lies at (t H + hd) 1024, so a tile's H KB are one piece.
//
// ita_long_heads_prop_kernel: grid (S / 128 key tiles, B, ceil(ng / NG)), 512 threads, ng = ceil(R / 16) weight groups.
// Wave v owns keys 16 v .. 16 v + 15 of its key tile; their H NS head-relative K fragments are loaded once from the K image
// -- the re-sort ita_long_heads_attn_body applies to Q, zero dwords past a head's last tile, with the roles swapped.  The
// workgroup sweeps the query tiles.  A tile's 24 KB of Q fragments arrive by LDS-DMA into a two-slot ring in the K-image
// layout [12][128][16], exactly as ita_long_prop_kernel stages them, with this workgroup's 2 NG KB of weight fragments and
// the tile's H KB of row parameters.  One barrier per query tile.  The heads run INSIDE the query-tile step: a staged Q tile
// serves all H heads before the ring moves on.  Per head ita_long_heads_qk<H, 1> runs with keys and queries swapped
// (integer dot products commute): lane (qi, kq) gets for key qi the biased accumulators of queries 16 j + 4 kq + 0..3,
// requantises them with lh_lg16x2<FAST> under ITA_NO_PK_F32 (the roundings production uses), applies each query's own m,
// cap and inv_hi (u16 vectors from the head's row-parameter image in LDS) and packs p - 128 into the two B fragments of
// mfma_i32_16x16x64_i8, whose A operand is the weight tile (word t, byte i of lane (r, kq) = query 64 kb + 16 t + 4 kq +
// i).  acc[hd][g] starts from 128 * sum_i w; at the end acc[hd][g][i] belongs to head hd, weight row 16 (NG z + g) + 4 kq +
// i and key qi.  No atomics, no floating point behind the logits: bit-reproducible by construction.  Vector stores only,
// every one at (b, hd < H, r < n_w, key < S).
//
// NG, the weight groups a workgroup accumulates, is what the registers allow beside the K fragments, the qk pipeline and
// the eight p-words ("Long-sequence heads: weighted column sums": the resource table): 4 for H = 2, 3, 4
// and 2 for H = 6, all at four waves per SIMD; grid.z covers the other groups and recomputes the probabilities.
//
// Range.  Per head, every partial sum is 128 * sum_i w + sum_{i < n} w (p - 128) with |sum w (p - 128)| and |128 sum w|
// each at most 128 * 128 * S: both fit int32 for any int8 weight at S <= 32768 (2^29 each), and at S = 65536 for weights
// in [-127, 127] (127 * 128 * 65536 < 2^30 each).  The weights are not scanned.
#pragma once
#include "ita_long_heads_kernel.h"
#include "ita_long_prop_kernel.h"

struct ItaLongHeadsRowsArgs {
  const char* qfrag;      // ita_long_proj_kernel's workspace: Q fragments (B, S/16, 3, 64 lanes, 16 B)
  const char* kimg;       //                                   K images (B, S/128, 24576)
  float ml;
  int B, S;
  char* rowp;             // workspace (B, S/128, H, 1024): per four queries u16 m[4] | cap[4] | inv_hi[4] | 0[4]
};

struct ItaLongHeadsPropWArgs {
  const int8_t* w;        // (B, n_w, S) weights, 4-byte aligned
  char* wimg;             // workspace (B, S/128, ng, 2, 64 lanes, 16 B): A fragments of the second MFMA, ng = ceil(n_w / 16)
  int* wsum;              // workspace (B, 64): 128 * sum_i w[b, r, i], 0 for r >= n_w
  int B, S, n_w;
};

struct ItaLongHeadsPropArgs {
  const char* qfrag;      // ita_long_proj_kernel's workspace
  const char* kimg;
  const char* rowp;       // ita_long_heads_rows_kernel's images
  const char* wimg;       // ita_long_heads_prop_wprep_kernel's
  const int* wsum;
  float ml;
  int B, S, n_w;
  int* out;               // (B, H, n_w, S)
};

// The weight groups one workgroup of ita_long_heads_prop_kernel accumulates (the resource table in DESIGN section 4)
template <int H>
constexpr int ita_long_heads_prop_ng = H == 6 ? 2 : 4;

// Two slots of Q image, weight fragments (8 KB at 64 rows) and H KB of row parameters: 76 KB at H = 6, two workgroups per CU
template <int H>
struct ItaLongHeadsPropLds {
  static constexpr int KB = ItaLongLds::KB;
  static constexpr int Q = 0, W = KB, RP = KB + 8192;  // inside a slot
  static constexpr int SLOT = RP + H * 1024;
  static constexpr int TOTAL = 2 * SLOT;
  static_assert(2 * TOTAL <= 160 * 1024, "two workgroups per CU");
};

// ---------------------------------------------------------------------------------------------------------------- rows
template <bool FAST, int H>
__device__ __forceinline__ void ita_long_heads_rows_body(const ItaLongHeadsRowsArgs& a) {
  static_assert(H == 2 || H == 3 || H == 4 || H == 6, "the head counts check_blob admits besides 1");
  constexpr int NC = 12 / H, NS = (NC + 3) / 4, KB = ItaLongLds::KB;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];     // the two-slot K ring
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nkt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const size_t tile0 = (size_t)b * nkt;              // first tile index of this frame
  const char* kimg = a.kimg + tile0 * KB;

  auto stage = [&](const char* src, int ldsoff) {    // 24 KB by LDS-DMA: three 1 KB pieces per wave
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int piece = wave + 8 * q;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + ldsoff + piece * 1024), 16, 0, 0);
    }
  };
  stage(kimg, 0);
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
  auto next_tile = [&](int step, int kt, bool more) {   // (the ring slot of a step is step & 1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nx = kt + 1 < nkt ? kt + 1 : 0;
    if (more) stage(kimg + (size_t)nx * KB, ((step + 1) & 1) * KB);
  };

  // ---------------- sweep 1: H row maxima of the raw accumulators (requantisation is monotonic)
  int mx[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) mx[hd] = (int)0x80000000;
  for (int kt = 0; kt < nkt; ++kt) {
    next_tile(kt, kt, true);
    ita_long_heads_qk<H, H>(lds + (kt & 1) * KB, qf, klane, 0, [&](int hd, int, const i32x4& acc) {
      mx[hd] = max(max(mx[hd], acc[0]), acc[1]);
      mx[hd] = max(max(mx[hd], acc[2]), acc[3]);
    });
  }
  unsigned mi[H];     // the clamped maximum as a biased u16
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int m = (int)(lh_lg16<FAST>(max1632_i(mx[hd]), a.ml) & 0xffffu);
    mi[hd] = (unsigned)min(max(m, 32768 - 128), 32768 + 127);
  }
  const u16x2 one = {256, 256};
  auto cap_of = [&](unsigned short m) { return (unsigned short)min((int)m - (32768 - 128), 15); };
  // ---------------- sweep 2: H row sums (the last step stages nothing: no sweep follows)
  int sumlo[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) sumlo[hd] = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = nkt + kt;
    next_tile(step, kt, kt + 1 < nkt);
    u16x2 s2 = {0, 0};
    ita_long_heads_qk<H, H>(lds + (step & 1) * KB, qf, klane, 0, [&](int hd, int j, const i32x4& acc) {
      const unsigned short m = (unsigned short)(mi[hd] & 0xffffu), cv = cap_of(m);
      const u16x2 mm = {m, m}, cap = {cv, cv};
      if (j == 0) s2 = (u16x2){0, 0};
      const u16x2 w0 = lh_lg16x2<FAST>(acc[0], acc[1], a.ml), w1 = lh_lg16x2<FAST>(acc[2], acc[3], a.ml);
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w0), cap);
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w1), cap);
      if (j == 7) sumlo[hd] += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile, head and lane
    });
  }
  // the row-parameter images: query q = 16 wave + qi of the tile, u16 slot (q >> 2) 16 + (q & 3) of head hd's KB
  const int q = wave * 16 + qi;
  unsigned short* rp = (unsigned short*)(a.rowp + (tile0 + qt) * H * 1024 + (q >> 2) * 32) + (q & 3);
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int sum = max(sum1632_i(sumlo[hd]), 1);
    const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;    // <= 255: the row maximum alone adds 256
    if (kq == 0) {
      unsigned short* p = rp + hd * 512;
      p[0] = (unsigned short)mi[hd];
      p[4] = cap_of((unsigned short)mi[hd]);
      p[8] = (unsigned short)inv_hi;
      p[12] = 0;
    }
  }
}

template <bool FAST, int H>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) ITA_NO_PK_F32 void ita_long_heads_rows_kernel(
    const ItaLongHeadsRowsArgs a) {
  ita_long_heads_rows_body<FAST, H>(a);
}

// ------------------------------------------------------------------------------------------------------------- weights
// Grid (S / 128 + 16 ng, B), 512 threads: the weight half of ita_long_prop_prep_kernel, same layouts.  Workgroup x < S / 128:
// the weight fragments of query tile x of frame b.  Workgroup S / 128 + r: 128 * the sum of weight row r (no atomics).
__global__ __launch_bounds__(512) void ita_long_heads_prop_wprep_kernel(const ItaLongHeadsPropWArgs a) {
  __shared__ int red[8];
  const int tid = threadIdx.x, b = blockIdx.y, x = blockIdx.x;
  const int nqt = a.S / 128, ng = (a.n_w + 15) >> 4;
  if (x < nqt) {
    const size_t tile = (size_t)b * nqt + x;
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

// --------------------------------------------------------------------------------------------------------------- sweep
template <bool FAST, int H, int NG>
__device__ __forceinline__ void ita_long_heads_prop_body(const ItaLongHeadsPropArgs& a) {
  static_assert(H == 2 || H == 3 || H == 4 || H == 6, "the head counts check_blob admits besides 1");
  static_assert(NG == 1 || NG == 2 || NG == 4, "16-row weight groups per workgroup");
  constexpr int NC = 12 / H, NS = (NC + 3) / 4;
  using L = ItaLongHeadsPropLds<H>;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nqt = a.S / 128, kt = blockIdx.x, b = blockIdx.y;
  const int ng = (a.n_w + 15) >> 4, g0 = blockIdx.z * NG;      // this workgroup's groups: g0 .. min(g0 + NG, ng) - 1
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
    if (wave < 2 * NG && 2 * g0 + wave < 2 * ng)     // fragment (g0 + wave / 2, kb = wave & 1) of the tile
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.wimg + ((tile0 + qt) * ng * 2 + 2 * g0 + wave) * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + L::W + wave * 1024), 16, 0, 0);
    if (wave >= 8 - H)                               // head 7 - wave's row parameters (the waves the weights leave idle first)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.rowp + ((tile0 + qt) * H + (7 - wave)) * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(dst + L::RP + (7 - wave) * 1024), 16, 0, 0);
  };
  stage(0, 0);
  // this wave's 16 keys as head-relative B fragments: the re-sort of the three H = 1 fragments, zero past a head's last tile
  i32x4 kf[H * NS];
  const int klane = (kq * 128 + qi) << 4;            // this lane's place inside a group of four Q chunks
  {
    i32x4 k1[3];
#pragma unroll
    for (int ks = 0; ks < 3; ++ks)
      k1[ks] = *(const i32x4*)(a.kimg + (tile0 + kt) * L::KB + (((4 * ks + kq) * 128 + wave * 16 + qi) << 4));
#pragma unroll
    for (int hd = 0; hd < H; ++hd)
#pragma unroll
      for (int ks = 0; ks < NS; ++ks)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int c = hd * NC + 4 * ks + d;
          kf[hd * NS + ks][d] = 4 * ks + d < NC ? k1[c >> 2][c & 3] : 0;
        }
  }
  // acc[hd][g][i]: head hd, weight row 16 (g0 + g) + 4 kq + i, key qi; from 128 * sum w (the probabilities ride as p - 128)
  i32x4 acc[H][NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const i32x4 w0 = g0 + g < ng ? *(const i32x4*)(a.wsum + b * 64 + 16 * (g0 + g) + 4 * kq) : (i32x4){0, 0, 0, 0};
#pragma unroll
    for (int hd = 0; hd < H; ++hd) acc[hd][g] = w0;
  }

  for (int qt = 0; qt < nqt; ++qt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // query tile qt landed for every wave; every wave is done with the other slot
    if (qt + 1 < nqt) stage(qt + 1, (qt + 1) & 1);
    const char* sb = lds + (qt & 1) * L::SLOT;
#pragma unroll
    for (int hd = 0; hd < H; ++hd) {
      i32x4 pf[2];
      ita_long_heads_qk<H, 1>(sb + L::Q, kf, klane, hd, [&](int, int j, const i32x4& lg) {
        // queries 16 j + 4 kq + 0..3 of the tile against key qi: m m | m m | cap cap | cap cap | inv_hi inv_hi | inv_hi inv_hi
        // as u16 pairs (plain array elements, as in ita_long_prop_kernel)
        const u16x2* prm = (const u16x2*)(sb + L::RP + hd * 1024 + (4 * j + kq) * 32);
        const u16x2 mm0 = prm[0], mm1 = prm[1], cap0 = prm[2], cap1 = prm[3], iv0 = prm[4], iv1 = prm[5];
        const u16x2 s0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm0, lh_lg16x2<FAST>(lg[0], lg[1], a.ml)), cap0);
        const u16x2 s1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm1, lh_lg16x2<FAST>(lg[2], lg[3], a.ml)), cap1);
        const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv0 >> s0));
        const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv1 >> s1));
        const unsigned p4 = __builtin_amdgcn_perm(p23, p01, 0x06040200u);   // u8 probabilities of queries 16 j + 4 kq + 0..3
        pf[j >> 2][j & 3] = (int)(p4 ^ 0x80808080u);
      });
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if (g0 + g < ng) {                           // (workgroup-uniform)
#pragma unroll
          for (int kb = 0; kb < 2; ++kb) {
            const i32x4 wf = *(const i32x4*)(sb + L::W + (((2 * g + kb) * 64 + lane) << 4));
            acc[hd][g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, pf[kb], acc[hd][g], 0, 0, 0);
          }
        }
    }
  }
#pragma unroll
  for (int hd = 0; hd < H; ++hd)
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * (g0 + g) + 4 * kq + i;
        if (r < a.n_w) a.out[(((size_t)b * H + hd) * a.n_w + r) * a.S + (size_t)kt * 128 + wave * 16 + qi] = acc[hd][g][i];
      }
}

template <bool FAST, int H, int NG>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) ITA_NO_PK_F32 void ita_long_heads_prop_kernel(
    const ItaLongHeadsPropArgs a) {
  ita_long_heads_prop_body<FAST, H, NG>(a);
}
