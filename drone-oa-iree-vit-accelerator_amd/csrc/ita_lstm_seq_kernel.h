// ita_lstm_seq_kernel.h -- the LSTM head with a time loop: T steps of layers 0, 1, 2 and the fc in one launch.
//
// ita_lstm_head_kernel (ita_lstm_head_kernel.h) advances the recurrence by one step per launch.  When the frames of a stream
// are known in advance, the image-only part of T steps x B streams (tokenizer, encoder, folded GEMM) runs as ONE batch of
// T * B frames, time-major, and only the recurrence is serial: this kernel walks it inside one launch.
//
// The decomposition (workgroup = one unit tile ut x one tile ft of 32 STREAMS, id = 16 ft + ut), the meeting protocol and
// the arithmetic are the head kernel's: both kernels are built from the device functions of ita_lstm_head_kernel.h, which
// is why T steps here equal T launches of the head kernel bit for bit.  What stays in the workgroup across the steps
// instead of being reloaded: the weight fragments of all three layers (layer 0's 9 k-steps x hi / lo in LDS, 18 KB;
// layers 1, 2: 4 + 4 k-steps x hi / lo per wave in registers), the biases, the fc weights (LDS), and h and c of the
// (stream, unit) pairs the workgroup owns -- c never leaves its owner until the last step.  Per step a workgroup reads
// only the step's split-K partials row  part[z][t * B + b][...], desvel[t][b], quat[t][b]  (all three prefetched one step
// ahead, behind the arrival at the step's first meeting) and the h hand-offs.
//
// Hand-offs.  The step path reads h(t-1) of all 128 units from memory as input state: layer 0 for its K = 144 remainder,
// layers 1, 2 for the recurrent half (k = 128 .. 255) of their operand.  Here these are hand-offs of the previous step.
// Per stream tile and step PARITY there are three buffers (ITA_SEQ_*):
//   P1  h0 as f16 hi / lo in fragment order (k < 128 of the head's layer-1 operand plane): read by layer 1 of the same
//       step (k-ranges 0, 1) and by layer 0 of the next step -- k-step s of layer 0's operand IS fragment (s / 4, s % 4);
//   P2  h1 likewise: read by layer 2 of the same step and by the recurrent half (waves 2, 3) of layer 1 of the next step;
//   H2  h2 as f32 rows [32][128]: read by the fc of the same step and, split with the same split_f16 expression, by the
//       recurrent half of layer 2 of the next step.
// Every consumer of the step path turns its f32 h into hi / lo with split_f16 before the MFMA, so consuming the published
// pairs is the same arithmetic.  The initial state takes the same road: before the first step every owner publishes its
// units of h_in into the parity-1 buffers ("step -1") and the tile meets once, so every step of the loop is alike.
//
// Meetings.  One counter per stream tile counts up through the launch.  With nt steps a workgroup arrives 2 nt + 2 times:
//   M0        after publishing the initial h                              (polled for 16)
//   M1(t)     after layer 0 of step t has published h0(t)                 (polled for 16 (2t + 2))
//   M2(t)     after layer 1 of step t has published h1(t)                 (polled for 16 (2t + 3))
//   the end   after layer 2 of the last step; not polled: the last arriver (its add returns 16 (2 nt + 2) - 1) resets the
//             counter to 0 for the next launch -- of this kernel or of the head kernel -- and computes the last step's fc.
// Order, for one workgroup:  M0 | L0(t) arrive M1(t) poll M1(t) [fc(t-1)] L1(t) arrive M2(t) poll M2(t) L2(t) | ... | end.
//   * L0(t) needs h0(t-1) of the tile: published before the arrivals at M1(t-1) (M0 for t = 0), which this workgroup has
//     polled.  L1(t) needs h0(t): M1(t); and h1(t-1): M2(t-1), polled earlier.  L2(t) needs h1(t): M2(t); and h2(t-1): every
//     workgroup stored it in L2(t-1) and drained the stores before arriving at M1(t), which precedes M2(t).
//   * fc(t) runs on workgroup ut = t % 16 behind M1(t+1): every workgroup's h2(t) stores were drained before that arrival.
// On a timeout the polling workgroup returns from the kernel at once, so a stuck tile costs one timeout, not one per step.
//
// Why two copies by step parity are enough (and one is not).  A buffer written in step t+1 is the one that held step t-1.
//   P1: the writer, L0(t+1), follows the writer's poll of M2(t) and so of M1(t); every workgroup arrived at M1(t) after its
//       L0(t) -- the last reader of P1(t-1), L1(t-1) being earlier still -- with its loads drained.
//   P2: the writer, L1(t+1), follows its poll of M1(t+1); every workgroup arrived there after L1(t) and L2(t-1), the readers
//       of P2(t-1).
//   H2: the writer, L2(t+1), follows its poll of M2(t+1); every workgroup arrived there after L2(t), the reader of H2(t-1),
//       and fc(t-1) ran before its workgroup's arrival at M2(t).
//   With a single copy L0(t+1) of a fast workgroup would overwrite h0(t) while a slow one still reads it for ITS L0(t+1).
//
// State aliasing: the state is updated in place.  A workgroup reads only the state of its own (stream, unit) pairs, before
// its first arrival, and writes the same elements once, after the last step.
//
// Progress: the head kernel's argument, with one difference.  The compiler gives this kernel 256 VGPRs + 60 AGPRs (no
// scratch; with a budget of 256 it spills 48), so a CU holds one workgroup and an XCD 32: at more than 512 streams the
// tiles run in rounds.
//
// Lengths (optional): stream b takes part in the steps t < lengths[b] of the whole sequence (this launch starts at step
// t0).  Behind its length a stream's h and c keep their values (the owner re-publishes the old h) and its velocity row is
// not written.  A tile runs  min(nsteps, max over its streams of lengths - t0)  steps: the bound is tile-uniform, so its
// sixteen workgroups agree on the number of meetings.
#pragma once
#include "ita_lstm_head_kernel.h"

constexpr int ITA_SEQ_PLANE = 2 * 4 * 64 * 16;                    // one f16 plane, k < 128, of one stream tile: 8 KB
constexpr int ITA_SEQ_P1 = 0, ITA_SEQ_P2 = 2 * ITA_SEQ_PLANE;     // [hi | lo] each
constexpr int ITA_SEQ_H2 = 4 * ITA_SEQ_PLANE;                     // f32 [32][128]
constexpr int ITA_SEQ_PARITY = ITA_SEQ_H2 + 32 * 128 * 4;         // bytes per parity copy
constexpr int ITA_SEQ_TILE = 2 * ITA_SEQ_PARITY;                  // bytes of hand-off buffers per stream tile

struct ItaLstmSeqArgs {
  ItaLstmModelArgs m;                                 // part: [NSPLIT][nsteps * B][512], row t * B + b
  const float *desvel, *quat;                         // (nsteps, B), (nsteps, B, 4): this launch's steps
  float *state_h, *state_c;                           // (3, B, 128): in the state before the first step, out after the last
  const int* lengths; int t0;                         // optional (B), in steps of the whole sequence; this launch starts at t0
  char* ho;                                           // hand-off buffers, ITA_SEQ_TILE bytes per stream tile
  const float *fc_w, *fc_b; float* vel;               // fc 128 -> 3, vel (nsteps, B, 3)
  unsigned *cnt, *err;                                // the head kernel's arrival counters (0 between launches) and error word
  int B, nsteps;
};
static_assert(offsetof(ItaLstmSeqArgs, desvel) == 104, "kernel-argument layout");

// byte offset within a plane of the 8-element group holding k (k % 8 == 0 or 4: + 2 (k & 7)) of stream r of the tile
__device__ __forceinline__ int ita_seq_plane_off(int r, int k) {
  return ((((k >> 6) * 4 + ((k >> 4) & 3)) * 64 + ((k >> 3) & 1) * 32 + r) * 8 + (k & 7)) * 2;
}

template <int NS>
__global__ __launch_bounds__(256, 1) void ita_lstm_seq_kernel(const ItaLstmSeqArgs a) {
  __shared__ __attribute__((aligned(16))) float big[32 * 132];       // layers 1, 2: the four waves' accumulators; fc: h2 rows
  __shared__ __attribute__((aligned(16))) float pt[32][36];          // layer 0: the summed partials
  __shared__ __attribute__((aligned(16))) float fw[3][128];          // fc weights
  __shared__ __attribute__((aligned(16))) _Float16 pub[2][32][8];    // layer-1 h [hi, lo][stream][unit], gathered for 16-byte stores
  __shared__ __attribute__((aligned(16))) f16x8 w0s[2][9][64];      // layer 0's weight fragments [hi, lo][k-step][lane] (wave 0 reads them)
  __shared__ unsigned flag;
  float (*hs)[132] = (float (*)[132])big;
  float (*acc4)[16][64] = (float (*)[16][64])big;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ft = blockIdx.x >> 4, ut = blockIdx.x & 15, f0 = ft * 32;
  const int r = lane & 31, h = lane >> 5;
  const int B = a.B;
  unsigned* const cnt = a.cnt + ft * ITA_HEAD_CNT_STRIDE;
  const __amdgpu_buffer_rsrc_t ho = ita_rsrc(a.ho + (size_t)ft * ITA_SEQ_TILE);

  // the tile's number of steps (uniform over its sixteen workgroups)
  int nt = a.nsteps;
  if (a.lengths) {
    int m = 0;
    for (int i = 0; i < 32; ++i) m = max(m, a.lengths[min(f0 + i, B - 1)]);
    nt = min(nt, max(m - a.t0, 0));
  }
  if (nt <= 0) return;

  // ---- operands that stay for the whole launch
  // layer 0 (wave 0 runs its MFMA chain): lane (r, h) owns units u0 .. u0+3 of stream b0
  const int b0 = f0 + r, u0 = ut * 8 + 4 * h, bc0 = min(b0, B - 1);
  f32x4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, h0 = {0.0f, 0.0f, 0.0f, 0.0f}, bz[4];
  int len0 = 0;
  if (wave == 0) {
    const _Float16* wfr_hi = a.m.w0_hi + ((size_t)ut * 9 * 64 + lane) * 8;
    const _Float16* wfr_lo = a.m.w0_lo + ((size_t)ut * 9 * 64 + lane) * 8;
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      w0s[0][s][lane] = *(const f16x8*)(wfr_hi + s * 512);
      w0s[1][s][lane] = *(const f16x8*)(wfr_lo + s * 512);
    }
    c0 = *(const f32x4*)(a.state_c + (size_t)bc0 * 128 + u0);
    h0 = *(const f32x4*)(a.state_h + (size_t)bc0 * 128 + u0);
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) bz[gt] = *(const f32x4*)(a.m.bias0 + gt * 128 + u0);
    len0 = b0 < B ? (a.lengths ? a.lengths[b0] - a.t0 : a.nsteps) : 0;
  }
  // layers 1, 2: this wave's k-range of the weights; thread t finishes (stream t / 8, unit t % 8)
  const size_t wo = ((size_t)((ut * 4 + wave) * 4) * 64 + lane) * 8;
  f16x8 w1h[4], w1l[4], w2h[4], w2l[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    w1h[s] = *(const f16x8*)(a.m.w1_hi + wo + 512 * s);
    w1l[s] = *(const f16x8*)(a.m.w1_lo + wo + 512 * s);
    w2h[s] = *(const f16x8*)(a.m.w2_hi + wo + 512 * s);
    w2l[s] = *(const f16x8*)(a.m.w2_lo + wo + 512 * s);
  }
  const int ef = tid >> 3, eu = tid & 7, eb = f0 + ef, un = ut * 8 + eu, ebc = min(eb, B - 1);
  const size_t lstride = (size_t)B * 128;
  const size_t so1 = lstride + (size_t)ebc * 128 + un, so2 = so1 + lstride;
  float c1 = a.state_c[so1], c2 = a.state_c[so2], h1 = a.state_h[so1], h2 = a.state_h[so2];
  const int lenE = eb < B ? (a.lengths ? a.lengths[eb] - a.t0 : a.nsteps) : 0;
  float bs1[4], bs2[4];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt) {
    bs1[gt] = a.m.bsum1[gt * 128 + un];
    bs2[gt] = a.m.bsum2[gt * 128 + un];
  }
  if (tid < 96) *(f32x4*)&fw[tid >> 5][4 * (tid & 31)] = *(const f32x4*)(a.fc_w + 4 * tid);
  // step 0's partials (wave w covers streams 8w .. 8w+7, lane (stream 8w + lane / 8, columns 4 (lane % 8) ..)), desvel, quat
  const size_t zstride = (size_t)a.nsteps * B * 512;
  const size_t prow = (size_t)min(f0 + 8 * wave + (lane >> 3), B - 1) * 512 + ut * 32 + 4 * (lane & 7);
  f32x4 ps;   // summed in the fixed z order (elementwise, so the layout does not matter)
  {
    f32x4 pz[NS];
#pragma unroll
    for (int z = 0; z < NS; ++z) pz[z] = *(const f32x4*)(a.m.part + z * zstride + prow);
    ps = sum_partials(pz);
  }
  f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
  float dv = 0.0f;
  if (wave == 0) {
    q = *(const f32x4*)(a.quat + (size_t)bc0 * 4);
    dv = a.desvel[bc0];
  }

  // publishing the h this workgroup owns into the buffers of parity `par`
  auto publish_h0 = [&](int par) {   // wave 0: 8-byte sc1 stores
    f16x4 x_hi, x_lo;
    split_f16x4(h0, x_hi, x_lo);
    const int o = par * ITA_SEQ_PARITY + ITA_SEQ_P1 + ita_seq_plane_off(r, u0);
    ita_store_sc1_f16x4(x_hi, ho, o);
    ita_store_sc1_f16x4(x_lo, ho, o + ITA_SEQ_PLANE);
  };
  auto publish_h1 = [&](int par) {   // every thread; gathered in LDS into one 16-byte sc1 store per stream and plane
    ita_gather_h8(h1, pub, ef, eu);
    if (wave == 0 && h == 0) {
      const int o = par * ITA_SEQ_PARITY + ITA_SEQ_P2 + ita_seq_plane_off(r, ut * 8);
      ita_publish_h8(pub, r, ho, o, ho, o + ITA_SEQ_PLANE);
    }
  };
  auto publish_h2 = [&](int par) {   // every thread: 4-byte sc1 stores
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, h2), ho, par * ITA_SEQ_PARITY + ITA_SEQ_H2 + (ef * 128 + un) * 4,
                                          0, ITA_SC1);
  };
  // the fc of one step from the H2 buffer of parity `par`: vel rows of step t (all threads of the workgroup)
  auto fc_step = [&](int par, int t) {
    f32x4 hr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      hr[i] = ita_load_sc1_f32x4(ho, par * ITA_SEQ_PARITY + ITA_SEQ_H2 + (((i * 256 + tid) >> 5) * 128 + 4 * (tid & 31)) * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) *(f32x4*)&hs[(i * 256 + tid) >> 5][4 * (tid & 31)] = hr[i];
    __syncthreads();
    lstm_fc_rows(hs, fw, a.fc_b, a.vel, (size_t)t * B, f0, B, tid, [&](int b) { return !a.lengths || a.t0 + t < a.lengths[b]; });
    __syncthreads();   // hs is the accumulators' storage of the next layer
  };

  // ---- "step -1": the initial h goes the way of every later one
  if (wave == 0) publish_h0(1);
  publish_h1(1);
  publish_h2(1);
  (void)ita_head_arrive(a.cnt, ft, tid);
  if (tid == 0) flag = ita_head_poll(cnt, 16u, a.err) ? 1u : 0u;
  __syncthreads();
  if (!flag) return;

  for (int t = 0; t < nt; ++t) {
    const int par = t & 1, prv = par ^ 1;
    // ---- layer 0: the summed partials to LDS; wave 0: [h0(t-1) | dv | quat] . [W_hh0 | w_dv | w_quat]^T
    *(f32x4*)&pt[8 * wave + (lane >> 3)][4 * (lane & 7)] = ps;
    f16x8 xh[8], xl[8];
    if (wave == 0) {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        xh[s] = ita_load_sc1_f16x8(ho, prv * ITA_SEQ_PARITY + ITA_SEQ_P1 + (s * 64 + lane) * 16);
        xl[s] = ita_load_sc1_f16x8(ho, prv * ITA_SEQ_PARITY + ITA_SEQ_P1 + ITA_SEQ_PLANE + (s * 64 + lane) * 16);
      }
    }
    __syncthreads();
    if (wave == 0) {
      f32x16 acc = {};
#pragma unroll
      for (int s = 0; s < 8; ++s) acc = mfma_f16x3(acc, w0s[0][s][lane], w0s[1][s][lane], xh[s], xl[s]);
      {   // k = 128 .. 132: [desvel / 10 | quat]
        float x1;
        const f32x4 x0 = lstm_l0_extra(dv, q, h, x1);
        f16x8 yh, yl;   // eight f32 -> hi, lo (not shared)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float x = j < 4 ? x0[j & 3] : (j == 4 ? x1 : 0.0f);
          const _Float16 hi = (_Float16)x;
          yh[j] = hi;
          yl[j] = (_Float16)(x - (float)hi);
        }
        acc = mfma_f16x3(acc, w0s[0][8][lane], w0s[1][8][lane], yh, yl);
      }
      const bool on = t < len0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float g[4];   // the pre-activation is not shared
#pragma unroll
        for (int gt = 0; gt < 4; ++gt)
          g[gt] = (pt[r][gt * 8 + 4 * h + i] * a.m.inv_fold_scale + acc[4 * gt + i] * a.m.inv_wscale0) + bz[gt][i];
        float c, hn;
        lstm_cell_fast(g[0], g[1], g[2], g[3], c0[i], c, hn);
        if (on) {
          c0[i] = c;
          h0[i] = hn;
        }
      }
      publish_h0(par);
    }
    (void)ita_head_arrive(a.cnt, ft, tid);   // M1(t)
    // the next step's partials, desvel and quat: in flight while the meeting waits
    f32x4 pz[NS];
    const bool more = t + 1 < nt;
    if (more) {
      const size_t step = (size_t)(t + 1) * B;
#pragma unroll
      for (int z = 0; z < NS; ++z) pz[z] = *(const f32x4*)(a.m.part + z * zstride + step * 512 + prow);
      if (wave == 0) {
        q = *(const f32x4*)(a.quat + (step + bc0) * 4);
        dv = a.desvel[step + bc0];
      }
    }

    // ---- layers 1 and 2: [x | h] . [W_ih | W_hh]^T, K = 256 split over the four waves, fused with the cell update
#pragma unroll
    for (int l = 1; l <= 2; ++l) {
      if (tid == 0) flag = ita_head_poll(cnt, 16u * (2u * t + 1u + l), a.err) ? 1u : 0u;
      __syncthreads();
      if (!flag) return;
      if (l == 1 && more) {   // the prefetched partials have arrived while the meeting waited (not sum_partials: not shared)
        ps = pz[0];
#pragma unroll
        for (int z = 1; z < NS; ++z) ps += pz[z];
      }
      if (l == 1 && t > 0 && ut == ((t - 1) & 15)) fc_step(prv, t - 1);
      f16x8 fah[4], fal[4];
      if (wave < 2 || l == 1) {
        // waves 0, 1: the previous layer's h of this step; waves 2, 3 of layer 1: h1 of the previous step
        const int base = (wave < 2 ? par : prv) * ITA_SEQ_PARITY + ((wave < 2) == (l == 1) ? ITA_SEQ_P1 : ITA_SEQ_P2) +
                         (((wave & 1) * 4) * 64 + lane) * 16;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          fah[s] = ita_load_sc1_f16x8(ho, base + 1024 * s);
          fal[s] = ita_load_sc1_f16x8(ho, base + ITA_SEQ_PLANE + 1024 * s);
        }
      } else {
        // waves 2, 3 of layer 2: h2 of the previous step, f32 rows split here (lane (r, h): k = 64 (wave - 2) + 16 s + 8 h ..)
        f32x4 hx[4][2];
        const int base = prv * ITA_SEQ_PARITY + ITA_SEQ_H2 + (r * 128 + 64 * (wave - 2) + 8 * h) * 4;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          hx[s][0] = ita_load_sc1_f32x4(ho, base + 64 * s);
          hx[s][1] = ita_load_sc1_f32x4(ho, base + 64 * s + 16);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)   // eight f32 -> hi, lo (not shared)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            _Float16 hi, lo;
            split_f16(hx[s][j >> 2][j & 3], hi, lo);
            fah[s][j] = hi;
            fal[s][j] = lo;
          }
      }
      f32x16 acc = {};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma_f16x3(acc, l == 1 ? w1h[s] : w2h[s], l == 1 ? w1l[s] : w2l[s], fah[s], fal[s]);
      // the four waves' accumulators through LDS to thread (stream ef, unit eu)'s four gates (not shared beyond lstm_sum4)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc4[wave][e][lane] = acc[e];
      __syncthreads();
      float gsum[4];
      const int pl = ef + 32 * (eu >> 2);
#pragma unroll
      for (int gte = 0; gte < 4; ++gte) gsum[gte] = lstm_sum4(acc4, 4 * gte + (eu & 3), pl);
      const float iws = l == 1 ? a.m.inv_wscale1 : a.m.inv_wscale2;
      const float* bs = l == 1 ? bs1 : bs2;
      const float gi = gsum[0] * iws + bs[0], gf = gsum[1] * iws + bs[1], gg = gsum[2] * iws + bs[2], go = gsum[3] * iws + bs[3];
      float c, hn;
      lstm_cell_fast(gi, gf, gg, go, l == 1 ? c1 : c2, c, hn);
      if (t < lenE) {
        if (l == 1) { c1 = c; h1 = hn; }
        else        { c2 = c; h2 = hn; }
      }
      if (l == 1) {
        publish_h1(par);
        (void)ita_head_arrive(a.cnt, ft, tid);   // M2(t)
      } else {
        publish_h2(par);   // drained by the next arrival: M1(t+1) or the end
      }
    }
  }

  // ---- the end: the state back to memory, one more arrival; the tile's last arriver re-arms the counter and computes the
  // last step's fc (every other workgroup has published its h2 and left, or is about to)
  if (wave == 0 && b0 < B) {
    *(f32x4*)(a.state_c + (size_t)b0 * 128 + u0) = c0;
    *(f32x4*)(a.state_h + (size_t)b0 * 128 + u0) = h0;
  }
  if (eb < B) {
    a.state_c[so1] = c1; a.state_h[so1] = h1;
    a.state_c[so2] = c2; a.state_h[so2] = h2;
  }
  const unsigned prev = ita_head_arrive(a.cnt, ft, tid);
  if (tid == 0) flag = prev == 16u * (2u * nt + 2u) - 1u ? 1u : 0u;
  __syncthreads();
  if (!flag) return;
  if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  fc_step((nt - 1) & 1, nt - 1);
}
