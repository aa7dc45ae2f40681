// ita_long_f32_ragged_kernel.h -- the long float attention (ita_long_f32_kernel.h) on RAGGED batches: frame b has
// len_b = min(max(lens[b], 0), S) tokens, S (a multiple of 128) is only the stride of x and y.  lens lies in device memory and
// is read by the kernels alone, so a captured graph follows new lengths on replay.
//
// Padding x on the host is no substitute: every padded key joins the softmax of every valid row, the float graph has no
// 1 / sqrt(d), and one padded row of moderate norm takes most of a valid row's probability mass.  And, other than in the
// int8 path (ita_long_ragged_kernel.h), nothing launders the padding: a NaN row of x is a NaN row of K and V, and 0 x NaN in
// the P.V MFMA would poison every valid row.  So the PROJECTION makes padding harmless, and the sweep masks what is left:
//
//   ita_lf32_ragged_proj_kernel<E> : ita_lf32_proj_kernel's tile loop and MFMA chains.  A wave's 16 tokens are key tile
//       wave & 3 of 64-key unit 2 tile + wave / 4.  A unit that starts at or past len_b is not stored (a wave-uniform
//       `continue`: the kernel has no barrier) and never fetched below.  In the unit that straddles len_b the x fragments of
//       tokens >= len_b are SELECTED to zero at the load (no multiplication): every MFMA output column (K^T) or row (V)
//       is one token's, so those tokens' K and V rows are the biases, finite whatever x held, and the valid tokens' rows
//       are the chains of ita_lf32_proj_kernel on the same operands: the same bits.
//   ita_lf32_ragged_attn_kernel<E> : one workgroup per (query tile, frame), 8 waves, the two-slot K ring and the V slot of
//       ita_lf32_attn_kernel (144 KB, two waves per SIMD).  len_b is one scalar load, every branch on it workgroup-uniform:
//       * 128 qt >= len_b: the workgroup zero-fills its 128 rows with 16-byte stores and leaves before any LDS-DMA is issued;
//         it reads nothing of x.
//       * else nu = ceil(len_b / 64) units are swept with the parent's ring and barrier schedule, nu in the place of S / 64.
//         nu is the same for all eight waves, so every wave reaches every barrier.  nu = 1: the step requests V unit 0 and no
//         further K unit; nu = 2, >= 3, odd: K unit u sits in slot u & 1 and unit u + 1 is requested into the other slot
//         behind the barrier that ends every wave's reads of it (step u - 1's logits).
//       * the last unit is masked when rem = len_b & 63 is not 0.  Lane (col, slot) holds the logits of keys
//         64 u + 16 kt + 4 slot + r in s[kt][r]:   a padded key  <=>  16 kt + r >= rem - 4 slot = rl,
//         16 kt + r a compile-time constant of the unrolled code: one v_cmp against rl and one v_cndmask per dword, no
//         divergence.  Padded logits enter the running maximum as -inf (key 64 u of a fetched unit is valid, so the maximum
//         is a finite logit), and their probabilities are 0.0f by SELECT -- ita_expf clamps at e^-87, which is not zero.
//         0 x (finite V) = 0 in the P.V chain and + 0 leaves l alone: rows [0, len_b) are the attention of the unpadded
//         frame.  The branch sits behind the unit's logits (`if (tail)`, twice: before the maximum and around the exp loop),
//         rl is formed inside it behind an empty asm so that it is no loop-invariant live register (the int8 kernel's lesson:
//         with the whole step written twice the compiler kept both copies' LDS addresses live and spilled).  Full units run
//         the parent's instruction stream, so with every length a multiple of 64 the valid rows carry the parent's bits.
//       * query rows >= len_b of a straddling tile compute on Q of the padded x, which may be NaN, and are stored as 0.0f.
//         Such a NaN never reaches a valid row: a query is one COLUMN (the B operand's) of every MFMA of the chain -- Q^T =
//         Wq x^T, S^T = K Q^T, ctx^T = V^T P^T, out^T = Wo ctx^T -- whose A operands (weights, K, V) are finite, and an MFMA
//         column depends on that column of B alone; the xor16 / xor32 exchanges of the maximum and the sum swap between the
//         four slot lanes of ONE query (lane & 15 is kept); the LDS row and the four finish lanes (layernorm_lanes: xor 1,
//         xor 2) are that query's own.
// fuse_ln, the residual read of the workgroup's own rows and y aliasing x: as in ita_lf32_attn_kernel.
//
// Namespace ita_f32_ragged: the code-object census of tests/test_long_f32_propagate_abi.py counts the global ita_lf32_
// kernels, and these are not of that family.
#pragma once
#include "ita_long_f32_kernel.h"

namespace ita_f32_ragged {

__device__ __forceinline__ int frame_len(const int* lens, int b, int S) {
  return __builtin_amdgcn_readfirstlane(min(max(lens[b], 0), S));
}

template <int E>
__global__ __launch_bounds__(512) void ita_lf32_ragged_proj_kernel(const ItaLongF32Args a, const int* lens) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel k groups");
  using L = ItaLongF32Lds;
  constexpr int S = 128, NFT = L::NFT, NG = E / 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, slot = lane >> 4;
  const int tpf = a.S / 128, ntile = a.B * tpf;      // tiles per frame, tiles
  for (int t = blockIdx.x; t < ntile; t += gridDim.x) {
    // step t is tile tf = t / B of frame b = t % B (the frame runs fastest): the tiles that frames of equal length store
    // are a dense prefix of the steps, spread over the blocks as ita_lf32_proj_kernel's are at a shorter S.  (Frame-major
    // steps gave every block the same tf for all its steps: half of the blocks idle, the other half with all the work.)
    const int tf = t / a.B, b = t - tf * a.B, tile = b * tpf + tf;
    const int len = frame_len(lens, b, a.S);
    // the wave's 16 tokens are key tile wave & 3 of unit 2 tile + wave / 4, which starts at token ustart of the frame
    const int ustart = 128 * tf + 64 * (wave >> 2);
    if (ustart >= len) continue;                     // (wave-uniform) the attention launch never fetches this unit
    const int tok = 128 * tf + 16 * wave;            // the wave's first token inside the frame
    // x fragments: lane (token col, slot), group g holds x[tok + col][16 g + 4 slot + 0..3], or zeros for a padded token
    const float* xsrc = a.x + ((size_t)tile * S + 16 * wave + col) * E + 4 * slot;
    f32x4 xf[NG];
    const bool kval = tok + col < len;               // K^T and Q^T layout: the lane's token is column col
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const f32x4 v = *(const f32x4*)(xsrc + 16 * g);
      xf[g] = kval ? v : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const size_t dst = ((size_t)(2 * tile + (wave >> 2)) * NFT * L::NKT + (wave & 3)) * 64 + lane;
    f32x4 *kd = a.kimg + dst, *vd = a.vimg + dst;

    // K^T: rows = features 16 ft + 4 slot + r, column = token col
#pragma unroll
    for (int ft = 0; ft < NFT; ft += 2) {
      f32x4 ka[2];
      const float* wkr[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        ka[u] = *(const f32x4*)(a.bk + 16 * (ft + u) + 4 * slot);
        wkr[u] = a.wk + ita_opaque((16 * (ft + u) + col) * E + 4 * slot);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 w0 = *(const f32x4*)(wkr[0] + 16 * g), w1 = *(const f32x4*)(wkr[1] + 16 * g);
        f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};   // block sum (ita_long_f32_kernel.h): 16 products from zero, then onto the total
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[r], xf[g][r], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[r], xf[g][r], t1, 0, 0, 0);
        }
        ka[0] += t0;
        ka[1] += t1;
      }
      kd[ft * L::NKT * 64] = ka[0];
      kd[(ft + 1) * L::NKT * 64] = ka[1];
    }
    // V: lane (feature 16 ft + col, slot) holds V[16 wave + 4 slot + r][feature]; x is the A operand, row = token col
#pragma unroll
    for (int ft = 0; ft < NFT; ft += 2) {
      f32x4 va[2];
      const float* wvr[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float bv = a.bv[16 * (ft + u) + col];
        va[u] = (f32x4){bv, bv, bv, bv};
        wvr[u] = a.wv + ita_opaque((16 * (ft + u) + col) * E + 4 * slot);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f32x4 w0 = *(const f32x4*)(wvr[0] + 16 * g), w1 = *(const f32x4*)(wvr[1] + 16 * g);
        f32x4 t0 = {0, 0, 0, 0}, t1 = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          t0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xf[g][r], w0[r], t0, 0, 0, 0);
          t1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xf[g][r], w1[r], t1, 0, 0, 0);
        }
        va[0] += t0;
        va[1] += t1;
      }
      vd[ft * L::NKT * 64] = va[0];
      vd[(ft + 1) * L::NKT * 64] = va[1];
    }
  }
}

template <int E>
__global__ __launch_bounds__(512) void ita_lf32_ragged_attn_kernel(const ItaLongF32Args a, const int* lens) {
  static_assert(E == 64 || E == 128, "four or eight 16-channel groups");
  using L = ItaLongF32Lds;
  constexpr int P = 192, XS = E + 4, NFT = L::NFT, NKT = L::NKT, NG = E / 16, EC = E / 4;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, slot = lane >> 4;
  const int t0 = 16 * wave;   // this wave's queries inside the tile
  // query tile (blockIdx.x + b) mod S / 128.  Unrotated, 32 frames of 4097 tokens at stride 8192 took 6.9 ms against 4.6 ms
  // for ita_lf32_attn_kernel at 4224; rotated, the whole call is below the parent's.  The times fit workgroups going to the
  // shader engines round robin in dispatch order, every frame's zero-filling workgroups on the same engines (DESIGN)
  const int b = blockIdx.y, qt = (int)((blockIdx.x + blockIdx.y) % gridDim.x);
  const int len = frame_len(lens, b, a.S);
  float* ytile = a.y + ((size_t)b * a.S + (size_t)qt * 128) * E;
  if (qt * 128 >= len) {   // (workgroup-uniform) a query tile of padding: zeros, and no DMA is in flight when the waves leave
    for (int p = tid; p < 128 * E / 4; p += 512) *(f32x4*)(ytile + (size_t)p * 4) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  const int nu = (len + 63) >> 6, rem = len & 63;   // units this frame fetches, valid keys of a masked last unit
  // rl = rem - 4 slot: dword r of key tile kt is a padded key <=> 16 kt + r >= rl.  Made where the masked unit needs it
  // (the empty asm keeps it out of the sweep's live registers)
  auto tail_rl = [&]() {
    int rl = rem - 4 * slot;
    asm volatile("" : "+v"(rl));
    return rl;
  };
  const char* kimg = (const char*)(a.kimg + (size_t)b * (a.S / 64) * L::UNIT_F4);
  const char* vimg = (const char*)(a.vimg + (size_t)b * (a.S / 64) * L::UNIT_F4);

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
  // barrier of the sweep
  const float* xsrc = a.x + ((size_t)b * a.S + (size_t)qt * 128 + t0 + col) * E + 4 * slot;
  f32x4 q[NFT];
  ita_lf32_q_prologue<E>(xsrc, a.wq, a.bq, col, slot, (f32x4*)(lds + L::K + L::UNIT) + wave * NFT * 64 + lane, q);

  float m = -__builtin_inff(), l = 0.0f;
  f32x4 c[NFT];
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) c[ft] = (f32x4){0, 0, 0, 0};
  for (int u = 0; u < nu; ++u) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // K unit u landed for every wave; every wave is done with step u - 1: the V slot and the other K slot are free
    stage(vimg + (size_t)u * L::UNIT, L::V);
    if (u + 1 < nu) stage(kimg + (size_t)(u + 1) * L::UNIT, L::K + ((u + 1) & 1) * L::UNIT);

    // S^T = K Q^T: tile kt, lane (query col, slot) holds S[query][64 u + 16 kt + 4 slot + r]
    const f32x4* kb = (const f32x4*)(lds + L::K + (u & 1) * L::UNIT);
    f32x4 s[NKT];
    ita_lf32_logits(kb, lane, q, s);
    const bool tail = rem != 0 && u == nu - 1;      // (workgroup-uniform) the unit that straddles len_b
    if (tail) {          // padded keys leave the maximum
      const int rl = tail_rl();
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = 16 * kt + r < rl ? s[kt][r] : -__builtin_inff();
    }
    {
      float down;
      const float mn = ita_lf32_running_max(s, m, down);
      float sum = 0.0f;
      if (!tail) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = ita_expf(s[kt][r] - mn);
            s[kt][r] = e;
            sum += e;
          }
      } else {           // padded keys: probability 0.0f by select (ita_expf(-inf - mn) is the clamp's e^-87)
        const int rl = tail_rl();
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = 16 * kt + r < rl ? ita_expf(s[kt][r] - mn) : 0.0f;
            s[kt][r] = e;
            sum += e;
          }
      }
      l = l * down + sum;
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft) c[ft] *= down;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // V unit u (and K unit u + 1, requested a whole S^T ago)
    __syncthreads();

    // ctx^T += V^T P^T: lane (query col, slot) holds ctx[query][16 ft + 4 slot + r]; k = key 64 u + 16 kt + 4 slot + r
    const f32x4* vb = (const f32x4*)(lds + L::V);
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      f32x4 vf[NFT];
#pragma unroll
      for (int ft = 0; ft < NFT; ++ft) vf[ft] = vb[(ft * NKT + kt) * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ft = 0; ft < NFT; ++ft) c[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[ft][r], s[kt][r], c[ft], 0, 0, 0);
    }
  }
  {
    l = ita_lf32_sum_slots(l);
    const float inv = 1.0f / l;
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) c[ft] *= inv;
  }

  // out^T = Wo ctx^T + bo: lane (query col, slot) holds out[query][16 et + 4 slot + r]
  f32x4 o[NG];
  const float* wor[NG];
#pragma unroll
  for (int et = 0; et < NG; ++et) {
    o[et] = *(const f32x4*)(a.bo + 16 * et + 4 * slot);
    wor[et] = a.wo + (16 * et + col) * P + 4 * slot;
  }
#pragma unroll
  for (int ft = 0; ft < NFT; ++ft) {
    f32x4 wf[NG];
#pragma unroll
    for (int et = 0; et < NG; ++et) wf[et] = *(const f32x4*)(wor[et] + 16 * ft);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int et = 0; et < NG; ++et) o[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[et][r], c[ft][r], o[et], 0, 0, 0);
  }
  // the wave's own rows, over the K ring (ItaLongF32Lds): x + out, or out alone
  float* xl = (float*)(lds + L::K);
  {
    float* xr = xl + (t0 + col) * XS + 4 * slot;
#pragma unroll
    for (int et = 0; et < NG; ++et) {
      f32x4 v = o[et];
      if (a.fuse_ln) v = *(const f32x4*)(xsrc + 16 * et) + v;
      *(f32x4*)(xr + 16 * et) = v;
    }
  }
  __syncthreads();

  // finish: 4 lanes per token (token t0 + lane / 4, channels E / 4 (lane & 3) ..): LayerNorm1, y; rows past len_b: zeros
  {
    const int tok = lane >> 2, qtr = lane & 3;
    float r[EC];
#pragma unroll
    for (int i = 0; i < EC; i += 4) {
      const f32x4 v = *(const f32x4*)(xl + (t0 + tok) * XS + qtr * EC + i);
      r[i] = v.x; r[i + 1] = v.y; r[i + 2] = v.z; r[i + 3] = v.w;
    }
    if (a.fuse_ln) layernorm_lanes<E>(r, a.ln_w, a.ln_b, qtr * EC);
    const bool valid = qt * 128 + t0 + tok < len;
    float* yrow = ytile + (size_t)(t0 + tok) * E + qtr * EC;
#pragma unroll
    for (int i = 0; i < EC; i += 4)
      *(f32x4*)(yrow + i) = valid ? (f32x4){r[i], r[i + 1], r[i + 2], r[i + 3]} : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
  }
}

}  // namespace ita_f32_ragged
