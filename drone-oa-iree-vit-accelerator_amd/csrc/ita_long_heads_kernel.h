// ita_long_heads_kernel.h -- ITASelfAttention_QAT with H = 2, 3, 4 or 6 heads on LONG token sequences (S a multiple of 128,
// E = 64 or 128, P = 192): the attention launch behind ita_mha_long_heads_q8 / _int8 / _int8_taps and
// ita_encoder_layer_long_heads.  The projection launch is ita_long_proj_kernel as it is (ita_long_attn_kernel.h): Q
// fragments, K images [12][128][16], V^T images and column sums do not depend on H.
//
// The arithmetic is ita_long_attn_kernel's per head of P / H features (mha_heads_ref.mha at any S): matmul1, the integer
// softmax over all S keys and matmul2 per head, the contexts concatenated, one ml and one mc for all heads.
//
// Work split: the launch shape, the LDS plan, the K ring and the V^T slot are the H = 1 kernel's -- grid (S / 128, B), 512
// threads, wave w owns 16 queries, ItaLongLds, one barrier per key tile (two in sweep 3).  The heads run INSIDE the
// key-tile step: every staged 24 KB K tile serves all H heads before the ring moves on, so staging bytes and barriers per
// step do not grow with H.
//   Q / K fragments  the projection launch sorts features so that a 16-feature tile c is dword c % 4 of every lane at k-step
//                    c / 4 (Q fragments and K chunks alike).  Head hd owns the NC = 12 / H tiles [hd NC, (hd + 1) NC); step ks
//                    of head hd takes the tiles hd NC + 4 ks + 0..3 as its four dwords: the Q fragment is a compile-time
//                    re-sort of the three H = 1 fragments, the K fragment the same dwords of the unchanged tile image.  Past
//                    the head's last tile the Q dword is zero and the K dword rereads the head's first tile (every LDS
//                    address stays inside the tile).  NS = ceil(NC / 4) steps of v_mfma_i32_16x16x64_i8 per head: 2, 1, 1, 1
//                    for H = 2, 3, 4, 6, so H NS = 4, 3, 4, 6 Q fragments stay in registers.
//   sweep 1          H running maxima of the raw accumulators per lane, one software pipeline over the 8 H key blocks of
//                    a tile; reduced over the four kq lanes and requantised once per head
//   sweep 2          H row sums, the same pipeline
//   sweep 3          head by head: the probabilities of the 128 keys go from the accumulators straight into the two B fragments
//                    of A.V (no logits array in between), then A.V for the head's own NC feature tiles -- a 16-feature tile lies
//                    inside one head for every H, so the 12 accumulator tiles and the 24 MFMAs per key tile are H = 1's
//   tail             context requantisation, out_proj, dequantise, residual + LayerNorm1 and the stores on all 192 features
// Per head and lane the softmax keeps ONE register: the clamped row maximum (biased u16) with inv_hi (<= 255) above it.
//
// Requantisation sites are written in plain C++, one value per instruction, and the kernels are compiled without the packed
// f32 VALU operations: the same roundings as lg8_v3 / dq16_b (x = acc_bits - 1.5 * 2^23 exactly, then one fma or a multiply
// and an add), value by value.
//
// Taps (ita_mha_long_heads_int8_taps): ItaLongTapArgs with logits / probs (B, H, n_rows, S) and row_max / row_sum
// (B, H, n_rows); stores only, of the registers the sweeps compute with.
#pragma once
#include "ita_long_attn_kernel.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define ITA_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ITA_NO_PK_F32   /* (the host pass does not know the device feature) */
#endif

// bits whose low 16 are rne(acc * ml) + 32768 for a biased accumulator: lg8_v3's value, one at a time
template <bool FAST>
__device__ __forceinline__ unsigned lh_lg16(int acc, float ml) {
  const float x = __int_as_float(acc) - ITA_MAGIC_F;
  if constexpr (FAST) return __float_as_uint(fmaf(x, ml, ITA_MAGIC32K_F));
  return __float_as_uint(__fadd_rn(__fmul_rn(x, ml), ITA_MAGIC32K_F));
}
template <bool FAST>
__device__ __forceinline__ ita_u16x2 lh_lg16x2(int a0, int a1, float ml) {
  return __builtin_bit_cast(ita_u16x2, __builtin_amdgcn_perm(lh_lg16<FAST>(a1, ml), lh_lg16<FAST>(a0, ml), 0x05040100u));
}
// sixteen biased out_proj accumulators -> clamped, unrounded codes f[4t + i] = med3((acc[t][i] - bias) * m, -128, 127)
__device__ __forceinline__ void lh_scale16(const i32x4 (&acc)[4], float m, float (&f)[16]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      f[4 * t + i] = __builtin_amdgcn_fmed3f(__fmul_rn(__int_as_float(acc[t][i]) - ITA_MAGIC_F, m), -128.0f, 127.0f);
}

// K Q^T of a wave's 16 queries against the 128-key tile at kb for the heads [hd0, hd0 + NHD): one pipeline over their
// 8 NHD blocks of 16 keys -- the fragments of block i + 1 load while block i multiplies, epil(hd, j, acc) takes the biased
// accumulators of key block j one step later (acc[i] <-> key 16 j + 4 kq + i of the tile, query qi).  One block per stage,
// not ita_long_qk_tile's two: the stage then holds NS fragments and one accumulator tile per buffer, which is what lets
// H NS Q fragments and the twelve A.V tiles stay in 128 registers.  A K fragment is gathered dword by dword from the
// unchanged tile image with the Q fragment's tile indices (adjacent dwords of one chunk merge into wider LDS reads); past
// the head's last tile it rereads the head's first, so every address stays inside the tile.  klane: (kq 128 + qi) 16.
template <int H, int NHD, class Epil>
__device__ __forceinline__ void ita_long_heads_qk(const char* kb, const i32x4 (&qf)[H * ((12 / H + 3) / 4)], int klane, int hd0, Epil epil) {
  constexpr int NC = 12 / H, NS = (NC + 3) / 4, NI = 8 * NHD;
  struct KFr { i32x4 w[NS]; } kfr[2];
  i32x4 la[2];
  auto ldk = [&](int i, KFr& f) {
    const int hd = hd0 + (i >> 3), j = i & 7;
#pragma unroll
    for (int ks = 0; ks < NS; ++ks)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int c = hd * NC + (4 * ks + d < NC ? 4 * ks + d : 0);   // tile c: dword c % 4 of chunk group c / 4
        f.w[ks][d] = *(const int*)(kb + (c >> 2) * 4 * 2048 + j * 256 + klane + 4 * (c & 3));
      }
  };
  auto mmk = [&](int i, const KFr& f, i32x4& acc) {
    const int hd = hd0 + (i >> 3);
    acc = (i32x4){ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS, ITA_ACC_BIAS};
#pragma unroll
    for (int ks = 0; ks < NS; ++ks) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(f.w[ks], qf[hd * NS + ks], acc, 0, 0, 0);
  };
  ldk(0, kfr[0]);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (i + 1 < NI) ldk(i + 1, kfr[(i + 1) & 1]);
    mmk(i, kfr[i & 1], la[i & 1]);
    if (i > 0) epil(hd0 + ((i - 1) >> 3), (i - 1) & 7, la[(i - 1) & 1]);
    ITA_SCHED_BARRIER();
  }
  epil(hd0 + NHD - 1, 7, la[(NI - 1) & 1]);
}

template <bool FAST, int E, int H, bool F32IO, bool TAPS>
__device__ __forceinline__ void ita_long_heads_attn_body(const ItaLongArgs& a, const ItaLongTapArgs& tp) {
  static_assert(!TAPS || F32IO, "the taps entry has the f32 form only");
  static_assert(E == 64 || E == 128, "one or two 64-channel output groups");
  static_assert(H == 2 || H == 3 || H == 4 || H == 6, "the head counts check_blob admits besides 1");
  constexpr int P = 192, EC = E / 4, NC = 12 / H, NS = (NC + 3) / 4;
  using LI = ItaStreamLds<E, false, false>;   // offsets inside the layer's image
  using L = ItaLongLds;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int nkt = a.S / 128, qt = blockIdx.x, b = blockIdx.y;
  const size_t tile0 = (size_t)b * nkt;              // first tile index of this frame
  const char* kimg = a.kimg + tile0 * L::KB;
  const char* vimg = a.vimg + tile0 * L::KB;

  auto stage = [&](const char* src, int ldsoff) {    // 24 KB by LDS-DMA: three 1 KB pieces per wave
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int piece = wave + 8 * q;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + ldsoff + piece * 1024), 16, 0, 0);
    }
  };
  stage(kimg, L::K);
  // out_proj bias from the layer's image; column sums of V over all key tiles of the frame
  if (tid < E / 4) *(i32x4*)(lds + L::BO + tid * 16) = *(const i32x4*)(a.image + LI::BIAS + (3 * P) * 4 + (size_t)tid * 16);
  if (tid < P) {
    int s = 0;
    for (int t = 0; t < nkt; ++t) s += a.csum[(tile0 + t) * P + tid];
    ((int*)(lds + L::CS))[tid] = s;
  }
  // head-relative fragments.  The projection launch's fragments and K chunks hold, in dword t of lane group kq at k-step g,
  // the features 16 (4 g + t) + 4 kq + 0..3: a 16-feature tile c = 4 g + t is ONE DWORD of every lane, and a head is the
  // NC tiles [hd NC, (hd + 1) NC).  Step ks of head hd takes the tiles hd NC + 4 ks + 0..3 as its four dwords, wherever
  // their k-steps lie -- all indices compile-time, the head's fragments are re-sorted copies of the three H = 1 fragments
  // (once per workgroup); past the head's last tile the dword is zero
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
  auto next_tile = [&](int step, int kt) {           // (ita_long_attn_body's: the ring slot of a step is step & 1)
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
      mx[hd] = max(max(mx[hd], acc[0]), acc[1]);           // (v_max3_i32)
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
  auto row_max = [&](int hd) { return (unsigned short)(mi[hd] & 0xffffu); };
  auto cap_of = [&](unsigned short m) { return (unsigned short)min((int)m - (32768 - 128), 15); };
  // taps: the output row of this lane's query (the four kq lanes of a query agree), and whether the wave has any
  int ri = -1;
  bool wave_rows = false;
  if constexpr (TAPS) {
    if (tp.rowidx) ri = tp.rowidx[qt * 128 + wave * 16 + qi];
    wave_rows = __builtin_amdgcn_ballot_w64(ri >= 0) != 0;
  }
  auto row_slot = [&](int hd) { return ((size_t)b * H + hd) * tp.n_rows + (size_t)max(ri, 0); };   // (B, H, n_rows)
  // ---------------- sweep 2: H row sums
  int sumlo[H];
#pragma unroll
  for (int hd = 0; hd < H; ++hd) sumlo[hd] = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = nkt + kt;
    next_tile(step, kt);
    u16x2 s2 = {0, 0};
    ita_long_heads_qk<H, H>(lds + L::K + (step & 1) * L::KB, qf, klane, 0, [&](int hd, int j, const i32x4& acc) {
      const unsigned short m = row_max(hd), cv = cap_of(m);
      const u16x2 mm = {m, m}, cap = {cv, cv};
      if (j == 0) s2 = (u16x2){0, 0};
      const u16x2 w0 = lh_lg16x2<FAST>(acc[0], acc[1], a.ml), w1 = lh_lg16x2<FAST>(acc[2], acc[3], a.ml);
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w0), cap);
      s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w1), cap);
      if constexpr (TAPS) {   // biased and unclamped: four int8 codes per store
        if (wave_rows && tp.logits && ri >= 0) {
          const int c0 = min(max((int)w0.x - 32768, -128), 127), c1 = min(max((int)w0.y - 32768, -128), 127);
          const int c2 = min(max((int)w1.x - 32768, -128), 127), c3 = min(max((int)w1.y - 32768, -128), 127);
          *(unsigned*)(tp.logits + row_slot(hd) * a.S + (size_t)kt * 128 + 16 * j + 4 * kq) = pack4(c0, c1, c2, c3);
        }
      }
      if (j == 7) sumlo[hd] += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile, head and lane
    });
  }
#pragma unroll
  for (int hd = 0; hd < H; ++hd) {
    const int sum = max(sum1632_i(sumlo[hd]), 1);
    const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;    // <= 255: the row maximum alone adds 256
    if constexpr (TAPS) {
      if (ri >= 0 && kq == 0) {
        if (tp.row_max) tp.row_max[row_slot(hd)] = (int8_t)((int)row_max(hd) - 32768);
        if (tp.row_sum) tp.row_sum[row_slot(hd)] = sum;
      }
    }
    mi[hd] |= (unsigned)inv_hi << 16;
  }
  // ---------------- sweep 3: per head probabilities and A.V for the head's own feature tiles; the accumulators start from
  // 128 * column sums (u8 probabilities ride the signed MFMA as p - 128)
  ITA_SCHED_BARRIER();   // (the H divisions above finish before the 48 accumulator registers go live)
  i32x4 va[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) va[c] = *(const i32x4*)(lds + L::CS + (c * 16 + 4 * kq) * 4);
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = 2 * nkt + kt;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // K tile kt landed; every wave is done with the previous step: the V^T slot and the other K slot are free
    stage(vimg + (size_t)kt * L::KB, L::V);
    if (kt + 1 < nkt) stage(kimg + (size_t)(kt + 1) * L::KB, L::K + ((step + 1) & 1) * L::KB);
#pragma unroll
    for (int hd = 0; hd < H; ++hd) {
      unsigned mih = mi[hd];
      asm volatile("" : "+v"(mih));   // unpacked HERE, per tile: hoisted out of the key loop the three pairs of every head cost 3 H registers
      const unsigned short m = (unsigned short)(mih & 0xffffu), cv = cap_of(m), ih = (unsigned short)(mih >> 16);
      const u16x2 mm = {m, m}, cap = {cv, cv}, iv = {ih, ih};
      i32x4 pf[2];
      ita_long_heads_qk<H, 1>(lds + L::K + (step & 1) * L::KB, qf, klane, hd, [&](int, int j, const i32x4& acc) {
        const u16x2 s0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, lh_lg16x2<FAST>(acc[0], acc[1], a.ml)), cap);
        const u16x2 s1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, lh_lg16x2<FAST>(acc[2], acc[3], a.ml)), cap);
        const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s0));
        const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s1));
        const unsigned p4 = __builtin_amdgcn_perm(p23, p01, 0x06040200u);   // u8 probabilities of keys 16 j + 4 kq + 0..3
        pf[j >> 2][j & 3] = (int)(p4 ^ 0x80808080u);
        if constexpr (TAPS) {
          if (wave_rows && tp.probs && ri >= 0) *(unsigned*)(tp.probs + row_slot(hd) * a.S + (size_t)kt * 128 + 16 * j + 4 * kq) = p4;
        }
      });
      if (hd == 0) {   // V^T tile kt (requested first: the three K pieces of the next step may still be on their way)
        if (!TAPS && kt + 1 < nkt) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (taps: their stores count too)
        __syncthreads();
      }
      const char* vb = lds + L::V;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int c = hd * NC; c < (hd + 1) * NC; ++c) {
          const i32x4 vf = *(const i32x4*)(vb + ((((kb * 4 + kq) * P) + c * 16 + qi) << 4));
          va[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pf[kb], va[c], 0, 0, 0);
        }
    }
  }
  // ---------------- context requantisation, out_proj, codes (or f32 rows) out: the H = 1 tail on all 192 features
  i32x4 cf[3];
#pragma unroll
  for (int dg = 0; dg < 3; ++dg) {
    float f[16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) f[4 * t + i] = __builtin_amdgcn_fmed3f(__fmul_rn((float)va[4 * dg + t][i], a.mc), -128.0f, 127.0f);
    unsigned pk[4];
    round_pack16(f, pk);
    cf[dg] = (i32x4){(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
  }
  __syncthreads();      // keeps the waves together for the stores
  const int token = wave * 16 + qi;
  const size_t row = (size_t)b * a.S + (size_t)qt * 128 + token;
  if constexpr (TAPS) {   // byte 4t + i of cf[dg] <-> feature 16 (4 dg + t) + 4 kq + i
    if (tp.ctx) {
#pragma unroll
      for (int dg = 0; dg < 3; ++dg)
#pragma unroll
        for (int t = 0; t < 4; ++t) *(int*)(tp.ctx + row * P + (4 * dg + t) * 16 + 4 * kq) = cf[dg][t];
    }
  }
  float x1[F32IO ? EC : 1];   // f32 form: this lane's quarter of the output row
#pragma unroll
  for (int eg = 0; eg < E / 64; ++eg) {
    i32x4 oa[4];
    ld_obias<E>(oa, (const int*)(lds + L::BO), 4 * eg, kq);
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
      ItaF4 ob;
      ld_frg_ks<E>(ob, a.image + LI::WO, 4 * eg, ks, qi, kq);      // (global: 48 KB per workgroup from L2, once)
      mm_ks(ob, cf[ks], oa);
    }
    float c[16];          // c[4t + i] <-> channel EC kq + 16 eg + 4t + i
    lh_scale16(oa, a.mo, c);
    if constexpr (F32IO) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        c[j] = __builtin_rintf(c[j]);
        x1[16 * eg + j] = __fmul_rn(c[j], a.so);
      }
      if constexpr (TAPS) {
        if (tp.outq) {
          i32x4 o4;
#pragma unroll
          for (int t = 0; t < 4; ++t) o4[t] = (int)pack4((int)c[4 * t], (int)c[4 * t + 1], (int)c[4 * t + 2], (int)c[4 * t + 3]);
          *(i32x4*)(tp.outq + row * E + EC * kq + 16 * eg) = o4;
        }
      }
    } else {
      unsigned pk[4];
      round_pack16(c, pk);
      *(i32x4*)(a.yq + row * E + EC * kq + 16 * eg) = (i32x4){(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
    }
  }
  if constexpr (F32IO) {
    if (a.fuse_ln) {   // (uniform) residual rows of this workgroup's own query tile, then LayerNorm1 as the stream kernel has it
      float xr[EC];
      ld_tok_items<E>(a.x + row * E, kq, xr);
      tok_items_transpose<E>(xr);
#pragma unroll
      for (int i = 0; i < EC; ++i) x1[i] = xr[i] + x1[i];
      const float* lnp = (const float*)(a.image + LI::LNP);   // n1w | n1b
      layernorm_q16<E>(x1, lnp, lnp + E, EC * kq);
    }
    st_tok_quarter<E>(a.y + row * E, kq, x1);
  }
}

template <bool FAST, int E, int H, bool F32IO>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) ITA_NO_PK_F32 void ita_long_heads_attn_kernel(const ItaLongArgs a) {
  ita_long_heads_attn_body<FAST, E, H, F32IO, false>(a, ItaLongTapArgs{});
}
// The one production form that does not fit 128 registers without scratch (FAST, E = 64, H = 6: two dwords short in either
// I/O form) runs this twin at two waves per SIMD instead ("Long-sequence heads": the resource table)
template <bool FAST, int E, int H>
constexpr bool ita_long_heads_two_waves = FAST && E == 64 && H == 6;
template <bool FAST, int E, int H, bool F32IO>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) ITA_NO_PK_F32 void ita_long_heads_attn_w2_kernel(const ItaLongArgs a) {
  ita_long_heads_attn_body<FAST, E, H, F32IO, false>(a, ItaLongTapArgs{});
}
template <bool FAST, int E, int H>
// (the taps' row addresses do not fit 128 registers beside the sweeps' state: two waves per SIMD, one workgroup per CU)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) ITA_NO_PK_F32 void ita_long_heads_attn_taps_kernel(
    const ItaLongArgs a, const ItaLongTapArgs tp) {
  ita_long_heads_attn_body<FAST, E, H, true, true>(a, tp);
}
