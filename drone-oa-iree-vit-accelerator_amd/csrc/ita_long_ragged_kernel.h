// ita_long_ragged_kernel.h -- the long int8 attention (ita_long_attn_kernel.h, H = 1, f32 form) on RAGGED batches: frame b
// has len_b = min(max(lens[b], 0), S) tokens, S (a multiple of 128) is only the stride of x and y.  lens lies in device
// memory and is read by the kernel alone, so a captured graph follows new lengths on replay.
//
// Padding x on the host is no substitute: the integer softmax takes the row's GLOBAL maximum and GLOBAL sum over all keys
// (ita_long_attn_kernel.h), so every padded key that is not masked moves the shift and the divisor of the valid rows.  The
// mask therefore sits inside the three sweeps.  What the kernel leans on:
//   * the projection launch (ita_long_proj_kernel<FAST, E, true>, unchanged) projects all B * S / 128 tiles, padded rows
//     included.  Whatever x holds there (NaN, Inf), the workspace holds int8 CODES for those rows: integers.
//   * key tiles past ceil(len_b / 128) are never fetched, and their column sums never added.
//   * in the LAST key tile, if len_b is no multiple of 128, keys >= len_b are taken out of the maximum (sweep 1), add 0 to
//     the row sum (sweep 2) and get probability 0 (sweep 3).  A probability rides the signed MFMA as p - 128 and the
//     accumulators start from 128 * (column sums of V over the fetched tiles): for a padded key (0 - 128) v + 128 v = 0
//     exactly in int32, for any code v.  So rows [0, len_b) are the definition on the unpadded frame, bit for bit.
//   * query rows >= len_b compute on padded codes (finite integers) and are stored as 0.0f; a workgroup whose whole query
//     tile lies past len_b zero-fills its 128 rows with 16-byte stores and leaves before any LDS-DMA is issued.
//
// Where the padded keys sit.  The logits MFMA (v_mfma_i32_16x16x64_i8, A = K fragment, B = Q fragment) of 16-key block j16
// of a tile leaves in lane (kq = lane >> 4, qi = lane & 15) the accumulator dwords i = 0..3 of
//         query qi  x  key 16 j16 + 4 kq + i          (row 4 kq + i, column qi of the 16 x 16 result)
// so with r = len_b - 128 * (tiles before the last) valid keys in the last tile and the per-lane value rl = r - 4 kq,
//         dword i of block j16 is a padded key  <=>  16 j16 + i >= rl
// with 16 j16 + i a compile-time constant of the unrolled code: one v_cmp against rl and one v_cndmask per dword, no branch
// inside the wave.  The later forms of the same keys follow from it:
//   sweep 2: the requantised logits travel as u16 pairs, w[2 j16 + j] = keys 16 j16 + 4 kq + 2 j (low half), + 1 (high half);
//            the numerators 256 >> shift are ANDed with a pair mask of 0xffff halves where 16 j16 + 2 j (+ 1) < rl
//   sweep 3: the u8 probabilities are packed four to a dword of the A.V MFMA's B fragment, byte i of pf[kb][t] = key
//            64 kb + 16 t + 4 kq + i; the dword is ANDed with the low min(max(rl - (64 kb + 16 t), 0), 4) bytes set, before
//            the ^ 0x80808080 that makes p - 128 of it
// Only the last tile takes these forms, behind `if (r)` (sweep 1, the masked tile peeled behind the loop) and
// `if (kt >= nfull)` (sweeps 2 and 3, behind the tile's logits: with the whole step written twice the compiler kept the LDS
// addresses of both copies live across the loop and spilled them).  len_b comes from one scalar load, so the branches are
// wave-uniform (in fact workgroup-uniform) and full tiles run the instruction stream of ita_long_attn_kernel.
//
// Ring and barriers: as in ita_long_attn_kernel with nkt = ceil(len_b / 128) in the place of S / 128.  Steps are counted
// through the sweeps, the K tile of a step sits in slot step & 1, every step has one barrier (two in sweep 3) that all eight
// waves reach: nkt is the same for the whole workgroup.  nkt = 1: every step prefetches tile 0 into the other slot;
// nkt = 2 and nkt >= 3: the last step of a sweep prefetches tile 0 of the next; the last step of sweep 3 prefetches nothing.
//
// Aliasing: y may be x, as in ita_long_attn_kernel.h -- workgroup (qt, b) reads the residual rows of its own query tile and
// nothing else of x; a zero-filling workgroup reads nothing of x at all.
#pragma once
#include "ita_long_attn_kernel.h"

template <bool FAST, int E>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void ita_long_ragged_attn_kernel(const ItaLongArgs a,
                                                                                                             const int* lens) {
  static_assert(E == 64 || E == 128, "one or two 64-channel output groups");
  constexpr int P = 192, EC = E / 4;
  using LI = ItaStreamLds<E, false, false>;   // offsets inside the layer's image
  using L = ItaLongLds;
  typedef ita_u16x2 u16x2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, kq = lane >> 4;
  const int qt = blockIdx.x, b = blockIdx.y;
  const int len = __builtin_amdgcn_readfirstlane(min(max(lens[b], 0), a.S));
  const size_t row0 = (size_t)b * a.S + (size_t)qt * 128;    // first row of this workgroup's query tile
  float* ytile = a.y + row0 * E;
  if (qt * 128 >= len) {   // (workgroup-uniform) a query tile of padding: zeros, and no DMA is in flight when the waves leave
    for (int p = tid; p < 128 * E / 4; p += 512) *(f32x4*)(ytile + (size_t)p * 4) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  const int nkt = (len + 127) >> 7, nfull = len >> 7, r = len & 127;   // key tiles, full ones, valid keys of the masked one
  // rl = r - 4 kq: block j16, dword i of this lane is a padded key <=> 16 j16 + i >= rl.  Made where a masked tile needs it
  // (the empty asm keeps it, and the masks that follow from it, out of the loops' live registers)
  auto tail_rl = [&]() {
    int rl = r - 4 * kq;
    asm volatile("" : "+v"(rl));
    return rl;
  };
  const size_t tile0 = (size_t)b * (a.S / 128);     // first tile index of this frame
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
  // out_proj bias from the layer's image; column sums of V over the key tiles this frame fetches (the masked tile's sum
  // holds its padded keys too: they cancel against probability 0, see above)
  if (tid < E / 4) *(i32x4*)(lds + L::BO + tid * 16) = *(const i32x4*)(a.image + LI::BIAS + (3 * P) * 4 + (size_t)tid * 16);
  if (tid < P) {
    int s = 0;
    for (int t = 0; t < nkt; ++t) s += a.csum[(tile0 + t) * P + tid];
    ((int*)(lds + L::CS))[tid] = s;
  }
  i32x4 qf[3];
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) qf[ks] = *(const i32x4*)(a.qfrag + ((((tile0 + qt) * 8 + wave) * 3 + ks) * 64 + lane) * 16);

  auto logits = [&](const char* kb, u16x2 (&w)[16]) { ita_long_logits<FAST>(kb, qf, kq, qi, a.ml, w); };
  // one step of sweeps 1 and 2, as in ita_long_attn_body: wait for this step's tile, barrier, send the next step's
  auto next_tile = [&](int step, int kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // this step's tile landed for every wave; every wave is done with the previous step's slot
    const int nx = kt + 1 < nkt ? kt + 1 : 0;
    stage(kimg + (size_t)nx * L::KB, L::K + ((step + 1) & 1) * L::KB);
  };

  // ---------------- sweep 1: row maximum of the raw (biased) accumulators over the valid keys
  int mx = (int)0x80000000;
  for (int kt = 0; kt < nfull; ++kt) {
    next_tile(kt, kt);
    ita_long_logits_max(lds + L::K + (kt & 1) * L::KB, qf, kq, qi, mx);
  }
  if (r) {
    const int rl = tail_rl();
    next_tile(nfull, nfull);
    ita_long_qk_tile(lds + L::K + (nfull & 1) * L::KB, qf, kq, qi, [&](int p, const i32x4 (&acc)[2]) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = max(mx, 16 * (2 * p + t) + i < rl ? acc[t][i] : (int)0x80000000);
    });
  }
  mx = max1632_i(mx);   // (a lane none of whose keys is valid brings INT_MIN; key 0 is valid: len >= 1 here)
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

  // ---------------- sweep 2: row sum of 256 >> shift over the valid keys.  One loop for full and masked tiles: the branch
  // sits behind the tile's logits, so the K Q^T stream is there once
  int sumlo = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = nkt + kt;
    next_tile(step, kt);
    u16x2 w[16];
    logits(lds + L::K + (step & 1) * L::KB, w);
    u16x2 s2 = {0, 0};
    if (kt < nfull) {
#pragma unroll
      for (int j = 0; j < 16; ++j) s2 += one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[j]), cap);
    } else {   // w[j] = keys 16 (j >> 1) + 4 kq + 2 (j & 1), + 1
      const int rl = tail_rl();
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k0 = 16 * (j >> 1) + 2 * (j & 1);
        const u16x2 n = one >> __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[j]), cap);
        s2 += n & __builtin_bit_cast(u16x2, (k0 < rl ? 0xffffu : 0u) | (k0 + 1 < rl ? 0xffff0000u : 0u));
      }
    }
    sumlo += (int)s2.x + (int)s2.y;       // <= 32 * 256 per tile and lane
  }
  int sum = sum1632_i(sumlo);
  sum = max(sum, 1);
  const int inv_hi = ((int)floorf((1.0f / (float)sum) * 16711680.0f)) >> 8;
  const u16x2 iv = {(unsigned short)inv_hi, (unsigned short)inv_hi};

  // ---------------- sweep 3: probabilities (0 for padded keys) and A.V from 128 * column sums
  i32x4 va[3][4];
#pragma unroll
  for (int dg = 0; dg < 3; ++dg)
#pragma unroll
    for (int t = 0; t < 4; ++t) va[dg][t] = *(const i32x4*)(lds + L::CS + ((4 * dg + t) * 16 + 4 * kq) * 4);
  for (int kt = 0; kt < nkt; ++kt) {
    const int step = 2 * nkt + kt;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // K tile kt landed; every wave is done with the previous step: the V^T slot and the other K slot are free
    stage(vimg + (size_t)kt * L::KB, L::V);
    if (kt + 1 < nkt) stage(kimg + (size_t)(kt + 1) * L::KB, L::K + ((step + 1) & 1) * L::KB);
    u16x2 w[16];
    logits(lds + L::K + (step & 1) * L::KB, w);
    i32x4 pf[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k4 = 4 * kb + t;
        const u16x2 s0 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[2 * k4]), cap);
        const u16x2 s1 = __builtin_elementwise_min(__builtin_elementwise_sub_sat(mm, w[2 * k4 + 1]), cap);
        const unsigned p01 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s0));
        const unsigned p23 = __builtin_bit_cast(unsigned, (u16x2)(iv >> s1));
        pf[kb][t] = (int)__builtin_amdgcn_perm(p23, p01, 0x06040200u);   // u8 probabilities of keys 64 kb + 16 t + 4 kq + 0..3
      }
    if (kt >= nfull) {   // the masked tile: of the four keys of a dword the first min(max(rl - 16 k4, 0), 4) are valid
      const int rl = tail_rl();
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4) {
        const int nv = min(max(rl - 16 * k4, 0), 4);
        pf[k4 >> 2][k4 & 3] &= (int)(nv >= 4 ? 0xffffffffu : (1u << (8 * nv)) - 1u);
      }
    }
#pragma unroll
    for (int k4 = 0; k4 < 8; ++k4) pf[k4 >> 2][k4 & 3] ^= (int)0x80808080u;   // p - 128
    // V^T tile kt (requested first: the three K pieces of the next step may still be on their way)
    if (kt + 1 < nkt) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const char* vb = lds + L::V;
#pragma unroll
    for (int st = 0; st < 6; ++st) {
      const int dg = st >> 1, kb = st & 1;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const i32x4 vf = *(const i32x4*)(vb + ((((kb * 4 + kq) * P) + (4 * dg + t) * 16 + qi) << 4));
        va[dg][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(vf, pf[kb], va[dg][t], 0, 0, 0);
      }
    }
  }

  // ---------------- context requantisation, out_proj, dequantise, (residual + LayerNorm1), rows out: ita_long_attn_body's f32 form
  i32x4 cf[3];
#pragma unroll
  for (int dg = 0; dg < 3; ++dg) {
    float f[16];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) f[4 * t + i] = __builtin_amdgcn_fmed3f((float)va[dg][t][i] * a.mc, -128.0f, 127.0f);
    unsigned pk[4];
    round_pack16(f, pk);
    cf[dg] = (i32x4){(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
  }
  __syncthreads();      // (BO was written in the prologue: visible since the first barrier; keeps the waves together for the stores)
  const int token = wave * 16 + qi;
  float x1[EC];         // this lane's quarter of the output row (the sweep accumulators are dead here)
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
    float d[16];
    dq_group(oa, a.mo, a.so, d);
#pragma unroll
    for (int j = 0; j < 16; ++j) x1[16 * eg + j] = d[j];
  }
  if (a.fuse_ln) {   // (uniform) residual rows of this workgroup's own query tile, then LayerNorm1 as the stream kernel has it
    float xr[EC];
    ld_tok_items<E>(a.x + (row0 + token) * E, kq, xr);
    tok_items_transpose<E>(xr);
#pragma unroll
    for (int i = 0; i < EC; ++i) x1[i] = xr[i] + x1[i];
    const float* lnp = (const float*)(a.image + LI::LNP);   // n1w | n1b
    layernorm_q16<E>(x1, lnp, lnp + E, EC * kq);
  }
  // rows past len_b: zeros (the four kq lanes of a token agree, and the exchanges of the store stay inside a token, so a NaN
  // that the residual of a padded row brought never reaches a valid row)
  const bool valid = qt * 128 + token < len;
#pragma unroll
  for (int i = 0; i < EC; ++i) x1[i] = valid ? x1[i] : 0.0f;
  st_tok_quarter<E>(ytile + (size_t)token * E, kq, x1);
}
