// ita_lstm_head_kernel.h -- the LSTM head of tail mode 1: layers 0, 1, 2 and the fc in one launch, and the device
// functions it shares with its time-looped form (ita_lstm_seq_kernel.h).  T steps of the sequence kernel equal T launches
// of the head kernel bit for bit because both run these functions, in this operation order.  A few blocks are still
// spelled out in both kernels (marked "not shared" there): moved into a function they compile to different, though
// arithmetically equal, code, and the kernels' machine code is what this file promises not to disturb.
#pragma once
#include <cstddef>
#include "ita_f16x3_kernels.h"

// ------------------------------------------------------------------ LSTM layer 0
// The decoder Linear feeds nothing but LSTM layer 0 (QAT/model.py:124-128), so its weights are folded
// one step further at load time:  G0 = W_ih0[:, :512] . Wfold  (512 x 8192).  The big GEMM then
// yields layer 0's gate pre-activations directly (as split-K partials, columns in the permuted
// gate order below) and the head kernel only adds the small remainder
//     [h_in0 | desvel/10 | quat] . [W_hh0 | W_ih0[:, 512:517]]^T        (K = 133, padded to 144)
// sums the partials in a fixed order, and performs the cell update.
// The [x | h] operand planes of LSTM layers 1, 2 (K = 256, f16 hi and lo) live in FRAGMENT order: the 32x32x16 B fragment
// of frame tile fg, k-range kw (64 k, one per wave of the head kernel's layers 1, 2) and k-step s is 64 lanes x 16 bytes
// contiguous, lane (r = frame & 31, h) holding k = 64 kw + 16 s + 8 h .. + 7.  Row-major planes made every fragment
// load touch 32 cache lines for 32 bytes each (and every epilogue store 32 lines for 2 bytes each); the load pipeline's
// per-line cost, not bandwidth, is what these small kernels wait for.  Rows are padded to whole 32-frame tiles.
__device__ __forceinline__ size_t ita_lstm_plane_index(int b, int k) {
  return ((size_t)(((b >> 5) * 4 + (k >> 6)) * 4 + ((k >> 4) & 3)) * 64 + ((k >> 3) & 1) * 32 + (b & 31)) * 8 + (k & 7);
}
// Gate non-linearities of the f16x3 path: v_exp_f32 / v_rcp_f32 forms (1 ulp each, ~6 instructions instead of ~28 for
// the oracle's fixed-arithmetic expf + IEEE division).  This path's tolerance against the f32 oracle is 2e-5 (measured
// max |vel - oracle| stays <= 4e-6); the exact-f32 path (tail mode 0) keeps ita_sigmoid / ita_tanh.
__device__ __forceinline__ float lstm_sigmoid_fast(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
__device__ __forceinline__ float lstm_tanh_fast(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(x * 2.88539008177792681f) + 1.0f);
}

// ------------------------------------------------------------------ the arithmetic both kernels share
// acc += wl . xh + wh . xl + wh . xh, in this order (A operand = weights, rows = permuted gates; B operand = frames)
__device__ __forceinline__ f32x16 mfma_f16x3(f32x16 acc, f16x8 wh, f16x8 wl, f16x8 xh, f16x8 xl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc, 0, 0, 0);
}
// one cell from its four gate pre-activations (i, f, g, o) and the previous c
__device__ __forceinline__ void lstm_cell_fast(float gi, float gf, float gg, float go, float c_prev, float& c, float& h) {
  const float ig = lstm_sigmoid_fast(gi), fg = lstm_sigmoid_fast(gf), cg = lstm_tanh_fast(gg), og = lstm_sigmoid_fast(go);
  c = fmaf(fg, c_prev, ig * cg);
  h = og * lstm_tanh_fast(c);
}
// four f32 -> an f16 vector of their hi parts and one of their lo parts
__device__ __forceinline__ void split_f16x4(f32x4 x, f16x4& hi, f16x4& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    _Float16 a, b;
    split_f16(x[j], a, b);
    hi[j] = a;
    lo[j] = b;
  }
}
// layer 0's operand of k = 128 .. 143, as f32: [desvel/10, q.x, q.y, q.z, q.w, 0, 0, 0] in the lanes h == 0, zero in the
// others; returns its first four, x4 = the fifth
__device__ __forceinline__ f32x4 lstm_l0_extra(float dv, f32x4 q, int h, float& x4) {
  f32x4 x0 = {0.0f, 0.0f, 0.0f, 0.0f};
  x4 = 0.0f;
  if (h == 0) {
    x0 = (f32x4){dv / 10.0f, q.x, q.y, q.z};
    x4 = q.w;
  }
  return x0;
}
// the split-K partials summed in z order (elementwise, so the layout does not matter)
template <int NS>
__device__ __forceinline__ f32x4 sum_partials(const f32x4 (&pz)[NS]) {
  f32x4 ps = pz[0];
#pragma unroll
  for (int z = 1; z < NS; ++z) ps += pz[z];
  return ps;
}
// layers 1, 2 split K over the four waves, whose accumulators meet in LDS part[wave][e][lane]: element (e, pl) combined
// ((p0 + p1) + p2) + p3.  C layout of a tile: accumulator e of lane (r, h) = gate e / 4 of unit (e % 4) + 4 h, frame r.
__device__ __forceinline__ float lstm_sum4(const float (*part)[16][64], int e, int pl) {
  return ((part[0][e][pl] + part[1][e][pl]) + part[2][e][pl]) + part[3][e][pl];
}
// the fc 128 -> 3 of a tile's 32 rows hs (f32, LDS) on threads 0 .. 95: ita_fc_kernel's fmaf chain from the bias.
// vel row of frame b is row0 + b; live(b) says whether it is written.
template <class Live>
__device__ __forceinline__ void lstm_fc_rows(const float (*hs)[132], const float (*fw)[128], const float* fc_b, float* vel,
                                             size_t row0, int f0, int B, int tid, Live live) {
  if (tid < 96) {
    const int fr = tid / 3, o = tid - 3 * fr, b = f0 + fr;
    if (b < B && live(b)) {
      float acc = fc_b[o];
      for (int k = 0; k < 128; ++k) acc = fmaf(hs[fr][k], fw[o][k], acc);
      vel[(row0 + b) * 3 + o] = acc;
    }
  }
}

// ------------------------------------------------------------------ meetings: how workgroups hand h to each other
// The sixteen workgroups of a frame tile meet on one arrival counter.  A meeting is a hand-off of h (f16 hi / lo planes
// in fragment order, or f32 rows), published write-through:
//   producer: every payload store carries sc1 (4-, 8- or 16-byte buffer stores) -> every wave  s_waitcnt vmcnt(0)  (asm,
//             not a builtin) -> workgroup barrier -> one lane: relaxed agent-scope atomic add on the counter;
//   consumer: one lane polls the counter with relaxed agent-scope (sc1) loads and s_sleep -> workgroup barrier -> every
//             load of handed-off bytes is an sc1 buffer load to registers.
// No release or acquire fence is needed (the stores bypass, the loads skip the per-CU L1), and nothing here is written with
// a scalar-memory instruction.  Spins are bounded: on a timeout a workgroup sets the device error word (*err) and returns;
// ita_head_status reports it and re-arms the counters.  A tile's last arriver of a launch resets the counter to 0, so the
// counters are valid for the next launch of either kernel (eager calls, graph replays and the pipelined loop alike); the
// workspace zeroes them when it is allocated.
// One 256-byte block per counter: packed into one cache line, the 32 counters of a 1024-frame batch took every poll and
// arrival of the 512 workgroups to one memory channel, and a meeting waited 15-25 us for its last arrival to show.
constexpr int ITA_HEAD_CNT_STRIDE = 64;
constexpr unsigned ITA_HEAD_ERR_TIMEOUT = 1;           // *err bit (ITA_HEAD_TIMEOUT of ita_head_status): a meeting waited longer than ITA_HEAD_SPIN_TICKS
constexpr unsigned long long ITA_HEAD_SPIN_TICKS = 200000000ull;   // 2 s of the 100 MHz constant clock
// h of a lane's 4 units goes to the hi and the lo plane as one 8-byte sc1 store each (split_f16x4, then two of these)
__device__ __forceinline__ void ita_store_sc1_f16x4(f16x4 v, __amdgpu_buffer_rsrc_t rsrc, int byte_off) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), rsrc, byte_off, 0, ITA_SC1);
}
// h of (frame ef, unit eu), one per thread, gathered in LDS (pub[hi, lo][frame][unit]; every thread, holds a workgroup
// barrier); then one lane per frame r writes its 8 units as one 16-byte sc1 store per plane
__device__ __forceinline__ void ita_gather_h8(float hn, _Float16 (*pub)[32][8], int ef, int eu) {
  _Float16 x, y;
  split_f16(hn, x, y);
  pub[0][ef][eu] = x;
  pub[1][ef][eu] = y;
  __syncthreads();
}
__device__ __forceinline__ void ita_publish_h8(const _Float16 (*pub)[32][8], int r, __amdgpu_buffer_rsrc_t hi, int off_hi,
                                               __amdgpu_buffer_rsrc_t lo, int off_lo) {
  const f16x8 vh = *(const f16x8*)&pub[0][r][0], vl = *(const f16x8*)&pub[1][r][0];
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, vh), hi, off_hi, 0, ITA_SC1);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, vl), lo, off_lo, 0, ITA_SC1);
}
// loads of handed-off bytes
__device__ __forceinline__ f16x8 ita_load_sc1_f16x8(__amdgpu_buffer_rsrc_t rsrc, int byte_off) {
  return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, 0, ITA_SC1));
}
__device__ __forceinline__ f32x4 ita_load_sc1_f32x4(__amdgpu_buffer_rsrc_t rsrc, int byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, byte_off, 0, ITA_SC1));
}
// arrival (whole workgroup) at tile ft's counter: every wave's payload stores and every earlier load have completed, then
// thread 0 counts the workgroup in.  Returns the counter's old value in thread 0, 0 in the others.
__device__ __forceinline__ unsigned ita_head_arrive(unsigned* cnt, int ft, int tid) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned prev = 0;
  if (tid == 0) prev = __hip_atomic_fetch_add(cnt + ft * ITA_HEAD_CNT_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return prev;
}
// one lane: wait until cnt >= target; false (and the error word set) on a timeout
__device__ __forceinline__ bool ita_head_poll(unsigned* cnt, unsigned target, unsigned* err) {
  const unsigned long long t0 = wall_clock64();
  while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    if (wall_clock64() - t0 > ITA_HEAD_SPIN_TICKS) {
      __hip_atomic_fetch_or(err, ITA_HEAD_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  return true;
}

// ------------------------------------------------------------------ the LSTM head: layers 0, 1, 2 and the fc in one launch
// gates = [x | h] . [W_ih | W_hh]^T on split-precision f16 MFMA, fused with the cell update (nn.LSTM, seq_len 1, gate order
// i,f,g,o; reference QAT/model.py:84,128-129), then fc 128 -> 3.  The 512 weight rows of every layer are permuted at load
// time to  r' = ut*32 + gate*8 + u  (ut = unit tile of 8 hidden units): one 32x32 MFMA tile then holds i,f,g,o of 8 units
// x 32 frames, and its C layout (row = (e&3) + 8*(e>>2) + 4*h) puts all four gates of a (frame, unit) pair in ONE lane.
//
// Workgroup = 4 waves = one unit tile ut x one 32-frame tile ft, for all three layers; 1-D grid of 16 * ceil(B/32),
// id = 16 ft + ut.  Each layer needs the previous layer's h of all 128 units of its frames, so the 16 workgroups of a frame
// tile meet twice (the protocol: above), on one arrival counter per frame tile (cnt[ft]: 16 arrivals per meeting), and the
// last of them to finish layer 2 computes the tile's fc.  A meeting is a hand-off of 32 frames x 8 units of h (f16 hi / lo,
// 1 KB) per workgroup.  The last arriver of layer 2 (its add returns 47) resets cnt[ft] to 0.
//
// Progress, for any grid size: ids are dealt round-robin over the eight XCDs (two of every frame tile's sixteen on each)
// and every XCD dispatches its share in id order, so the members of the lowest unfinished frame tile are dispatched before
// any workgroup of a later tile on the same XCD.  A frame tile waits for nothing outside itself, so as long as an XCD can
// hold two of these workgroups, the lowest unfinished tile always completes and frees its slots.  At <= 256 VGPRs and
// ~55 KB of LDS two workgroups fit on every CU: at 1024 frames (512 workgroups, 256 CUs) the whole grid is resident.
//
// State aliasing (h_out may alias h_in, c_out c_in; slot-indexed rows): every h_in / c_in read completes (the vmcnt drain)
// before the workgroup's first arrival, and no h_out element is written before the first meeting has completed, so no
// read sees a new value.  c is read and written by the one workgroup that owns its units.
//
// Arithmetic: layer 0 sums the split-K partials in z order and adds the K = 144 remainder on one wave's MFMA chain; layers
// 1, 2 split K over the four waves and combine ((p0 + p1) + p2) + p3; fast sigmoid / tanh; the fc is an fmaf chain from the bias.

// what both kernels read of the model: the first member of ItaLstmHeadArgs and of ItaLstmSeqArgs
struct ItaLstmModelArgs {
  const float* part; float inv_fold_scale;            // [NSPLIT][rows][512] raw split-K accumulators of x2 . (G0 * scale)^T
  const _Float16 *w0_hi, *w0_lo; float inv_wscale0;   // [ut 16][k-step 9][lane 64][8] A fragments of the permuted, pre-scaled [W_hh0 | w_dv | w_quat | 0]
  const float* bias0;                                 // [512] gate-major: W_ih0[:, :512].bias' + b_ih0 + b_hh0
  const _Float16 *w1_hi, *w1_lo, *w2_hi, *w2_lo;       // layers 1, 2: [ut 16][k-range 4][k-step 4][lane 64][8] A fragments
  float inv_wscale1, inv_wscale2;
  const float *bsum1, *bsum2;                         // [512] b_ih + b_hh, gate-major
};
struct ItaLstmHeadArgs {
  ItaLstmModelArgs m;                                 // part: [NSPLIT][B][512]
  const float *desvel, *quat;                         // (B), (B,4)
  const float *h_in, *c_in;                           // (3, rows, 128) state, layer l at + l * lstride
  float *h_out, *c_out;                               // the same shape; may alias h_in / c_in
  size_t lstride;
  _Float16 *p1_hi, *p1_lo, *p2_hi, *p2_lo;            // operand planes [h_out | h_in] of layers 1, 2 in fragment order; k < 128 handed off here
  const float *fc_w, *fc_b; float* vel;               // fc 128 -> 3, vel (B,3)
  unsigned *cnt, *err;                                // arrival counters, tile ft's at cnt[ft * ITA_HEAD_CNT_STRIDE] (0 between launches); error word
  int B;
  const int* slots;                                   // optional: state row of frame b, else b
};
// the kernels' argument loads stay where they were when the 14 leading fields were spelled out in both structs
static_assert(sizeof(ItaLstmModelArgs) == 104 && offsetof(ItaLstmHeadArgs, desvel) == 104, "kernel-argument layout");

template <int NS>
__global__ __launch_bounds__(256, 2) void ita_lstm_head_kernel(const ItaLstmHeadArgs a) {
  // phase 0: h_in0 rows [32][132] and the summed partials [32][36]; layers 1, 2: the four waves' accumulators; fc: h_out2 rows
  __shared__ __attribute__((aligned(16))) float big[32 * 132 + 32 * 36];
  __shared__ __attribute__((aligned(16))) f16x8 hin[2][2][4][2][64];   // [layer 1, 2][k-range 2, 3][k-step][hi, lo][lane]: the h_in halves
  __shared__ __attribute__((aligned(16))) _Float16 pub[2][32][8];      // layer-1 h_out [hi, lo][frame][unit], gathered for 16-byte stores
  __shared__ unsigned flag;
  float (*hs)[132] = (float (*)[132])big;
  float (*pt)[36] = (float (*)[36])(big + 32 * 132);
  float (*part)[16][64] = (float (*)[16][64])big;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ft = blockIdx.x >> 4, ut = blockIdx.x & 15, f0 = ft * 32;
  const int r = lane & 31, h = lane >> 5;
  const int B = a.B;
  // state rows of the frames this lane touches before the first meeting, looked up first (one wait, not one per load)
  const int ef = tid >> 3, eu = tid & 7;   // layers 1, 2: the cell update of (frame f0 + ef, unit ut * 8 + eu)
  int rh[4], rb0 = min(f0 + r, B - 1), reb = min(f0 + ef, B - 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) rh[i] = min(f0 + 2 * (4 * wave + i) + h, B - 1);
  if (a.slots) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rh[i] = a.slots[rh[i]];
    rb0 = a.slots[rb0];
    reb = a.slots[reb];
  }

  // ---- every load that needs no hand-off is issued up front
  // split-K partials, spread over the waves: wave w covers frames 8w .. 8w+7, lane (frame 8w + lane/8, columns 4 (lane % 8) ..)
  f32x4 pz[NS];
#pragma unroll
  for (int z = 0; z < NS; ++z)
    pz[z] = *(const f32x4*)(a.m.part + ((size_t)z * B + min(f0 + 8 * wave + (lane >> 3), B - 1)) * 512 + ut * 32 + 4 * (lane & 7));
  // layer-0 h rows: load i of wave w covers frames 2 (4w + i), 2 (4w + i) + 1
  f32x4 hv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) hv[i] = *(const f32x4*)(a.h_in + (size_t)rh[i] * 128 + 4 * r);
  const int b0 = f0 + r, u0 = ut * 8 + 4 * h;
  const size_t sb0 = (size_t)rb0;
  // the h_in halves (k = 128..255) of the layer-1 and layer-2 operands are input state, not hand-offs: waves 2, 3 (whose
  // k-ranges they are) read them now, split them and keep them in LDS in fragment order.  (Ahead of wave 0's loads in
  // program order, so that their registers and wave 0's are never live at once.)
  if (wave >= 2) {
    f32x4 hx[2][4][2];
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float* src = a.h_in + (l + 1) * a.lstride + sb0 * 128 + 64 * (wave - 2) + 16 * s + 8 * h;
        hx[l][s][0] = *(const f32x4*)src;
        hx[l][s][1] = *(const f32x4*)(src + 4);
      }
    __builtin_amdgcn_sched_barrier(0);   // all sixteen loads in flight before the first wait
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        f16x8 xh, xl;   // eight f32 -> hi, lo (not shared)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          _Float16 hi, lo;
          split_f16(hx[l][s][j >> 2][j & 3], hi, lo);
          xh[j] = hi;
          xl[j] = lo;
        }
        hin[l][wave - 2][s][0][lane] = xh;
        hin[l][wave - 2][s][1][lane] = xl;
      }
  }
  // layer 0's own operands (wave 0 runs its MFMA chain): remainder weights, desvel and quat, c_in, bias
  f16x8 wh[9], wl[9];
  f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f}, ci0 = {0.0f, 0.0f, 0.0f, 0.0f}, bz[4];
  float dv = 0.0f;
  if (wave == 0) {
    const _Float16* wfr_hi = a.m.w0_hi + ((size_t)ut * 9 * 64 + lane) * 8;   // fragment order: 1 KB per wave-load
    const _Float16* wfr_lo = a.m.w0_lo + ((size_t)ut * 9 * 64 + lane) * 8;
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      wh[s] = *(const f16x8*)(wfr_hi + s * 512);
      wl[s] = *(const f16x8*)(wfr_lo + s * 512);
    }
    const int bc = min(b0, B - 1);
    q = *(const f32x4*)(a.quat + (size_t)bc * 4);
    dv = a.desvel[bc];
    ci0 = *(const f32x4*)(a.c_in + sb0 * 128 + u0);
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) bz[gt] = *(const f32x4*)(a.m.bias0 + gt * 128 + u0);
  }
  // layer 1's weight fragments of this wave's k-range (layer 2's are fetched while the first meeting waits)
  const size_t wo = ((size_t)((ut * 4 + wave) * 4) * 64 + lane) * 8;
  f16x8 w1h[4], w1l[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    w1h[s] = *(const f16x8*)(a.m.w1_hi + wo + 512 * s);
    w1l[s] = *(const f16x8*)(a.m.w1_lo + wo + 512 * s);
  }
  // the cell updates of layers 1, 2 are dealt out by MEMORY layout: thread t finishes (frame t / 8, unit t % 8), so a wave
  // reads and writes 8 frames x 8 consecutive units = 8 row segments of 32 bytes of the state per instruction
  const int eb = f0 + ef, un = ut * 8 + eu;
  const size_t esb = (size_t)reb;
  const float c1_prev = a.c_in[a.lstride + esb * 128 + un], c2_prev = a.c_in[2 * a.lstride + esb * 128 + un];
  float bs1[4], bs2[4];
#pragma unroll
  for (int gt = 0; gt < 4; ++gt) {
    bs1[gt] = a.m.bsum1[gt * 128 + un];
    bs2[gt] = a.m.bsum2[gt * 128 + un];
  }
  __builtin_amdgcn_sched_barrier(0);   // every load above is issued before the first wait
  // partials summed in their fixed order (elementwise, so the layout does not matter), then to LDS with the h rows
  *(f32x4*)&pt[8 * wave + (lane >> 3)][4 * (lane & 7)] = sum_partials(pz);
#pragma unroll
  for (int i = 0; i < 4; ++i) *(f32x4*)&hs[2 * (4 * wave + i) + h][4 * r] = hv[i];
  __syncthreads();

  // ---- layer 0 on wave 0: A operand = weights (rows = permuted gates), B operand = this frame's [h | dv | quat]
  f32x4 hn0 = {0.0f, 0.0f, 0.0f, 0.0f};
  if (wave == 0) {
    f32x16 acc = {};
    float xlast1;   // [desvel/10 | quat] in k = 128 .. 132
    const f32x4 xlast0 = lstm_l0_extra(dv, q, h, xlast1);
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      f32x4 x0 = xlast0, x1 = {xlast1, 0.0f, 0.0f, 0.0f};
      if (s < 8) {
        x0 = *(const f32x4*)&hs[r][16 * s + 8 * h];
        x1 = *(const f32x4*)&hs[r][16 * s + 8 * h + 4];
      }
      f16x8 xh, xl;   // eight f32 -> hi, lo (not shared)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = j < 4 ? x0[j & 3] : x1[j & 3];
        const _Float16 hi = (_Float16)x;
        xh[j] = hi;
        xl[j] = (_Float16)(x - (float)hi);
      }
      acc = mfma_f16x3(acc, wh[s], wl[s], xh, xl);
    }
    // acc[4*gate + q] <-> gate (i,f,g,o), unit u0 + q, frame b0; the pre-activation is not shared
    f32x4 cn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float g[4];
#pragma unroll
      for (int gt = 0; gt < 4; ++gt)
        g[gt] = (pt[r][gt * 8 + 4 * h + q] * a.m.inv_fold_scale + acc[4 * gt + q] * a.m.inv_wscale0) + bz[gt][q];
      float c, hn;
      lstm_cell_fast(g[0], g[1], g[2], g[3], ci0[q], c, hn);
      cn[q] = c;
      hn0[q] = hn;
    }
    if (b0 < B) *(f32x4*)(a.c_out + sb0 * 128 + u0) = cn;
    // hand-off: layer 1's operand planes, k = u0 .. u0+3 of frame b0 (rows are padded to whole frame tiles): 8-byte sc1 stores
    f16x4 x_hi, x_lo;
    split_f16x4(hn0, x_hi, x_lo);
    const int o0 = (int)ita_lstm_plane_index(b0, u0) * 2;   // bytes
    ita_store_sc1_f16x4(x_hi, ita_rsrc(a.p1_hi), o0);
    ita_store_sc1_f16x4(x_lo, ita_rsrc(a.p1_lo), o0);
  }
  (void)ita_head_arrive(a.cnt, ft, tid);   // arrival 1: every read of h_in / c_in has completed, too
  f16x8 w2h[4], w2l[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    w2h[s] = *(const f16x8*)(a.m.w2_hi + wo + 512 * s);
    w2l[s] = *(const f16x8*)(a.m.w2_lo + wo + 512 * s);
  }

  // ---- layers 1 and 2: [x | h] . [W_ih | W_hh]^T, K = 256 split over the four waves, fused with the cell update
#pragma unroll
  for (int l = 1; l <= 2; ++l) {
    if (tid == 0) flag = ita_head_poll(a.cnt + ft * ITA_HEAD_CNT_STRIDE, 16u * l, a.err) ? 1u : 0u;
    __syncthreads();
    if (!flag) return;
    if (l == 1 && wave == 0 && b0 < B) *(f32x4*)(a.h_out + sb0 * 128 + u0) = hn0;   // every h_in read of the tile is done
    f16x8 fah[4], fal[4];
    if (wave < 2) {   // handed-off h of the previous layer: sc1 loads
      const int ao = (((ft * 4 + wave) * 4) * 64 + lane) * 16;   // bytes
      const _Float16* ph = l == 1 ? a.p1_hi : a.p2_hi;
      const _Float16* pl = l == 1 ? a.p1_lo : a.p2_lo;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        fah[s] = ita_load_sc1_f16x8(ita_rsrc(ph), ao + 1024 * s);
        fal[s] = ita_load_sc1_f16x8(ita_rsrc(pl), ao + 1024 * s);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        fah[s] = hin[l - 1][wave - 2][s][0][lane];
        fal[s] = hin[l - 1][wave - 2][s][1][lane];
      }
    }
    f32x16 acc = {};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma_f16x3(acc, l == 1 ? w1h[s] : w2h[s], l == 1 ? w1l[s] : w2l[s], fah[s], fal[s]);
    // the four waves' accumulators through LDS to thread (frame ef, unit eu)'s four gates (not shared beyond lstm_sum4)
#pragma unroll
    for (int e = 0; e < 16; ++e) part[wave][e][lane] = acc[e];
    __syncthreads();
    float gsum[4];
    const int pl = ef + 32 * (eu >> 2);
#pragma unroll
    for (int gte = 0; gte < 4; ++gte) gsum[gte] = lstm_sum4(part, 4 * gte + (eu & 3), pl);
    const float iws = l == 1 ? a.m.inv_wscale1 : a.m.inv_wscale2;
    const float* bs = l == 1 ? bs1 : bs2;
    const float gi = gsum[0] * iws + bs[0], gf = gsum[1] * iws + bs[1], gg = gsum[2] * iws + bs[2], go = gsum[3] * iws + bs[3];
    float c, hn;
    lstm_cell_fast(gi, gf, gg, go, l == 1 ? c1_prev : c2_prev, c, hn);
    const size_t so = l * a.lstride + esb * 128 + un;
    if (eb < B) {
      a.c_out[so] = c;
      if (l == 1) a.h_out[so] = hn;
      else        // the fc reads these: handed-off bytes, 4-byte sc1 stores
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, hn), ita_rsrc(a.h_out), (int)(so * 4), 0, ITA_SC1);
    }
    if (l == 1) {   // hand-off: layer 2's operand planes, gathered in LDS into one 16-byte sc1 store per frame and plane
      ita_gather_h8(hn, pub, ef, eu);
      if (wave == 0 && h == 0) {
        const int o = (int)ita_lstm_plane_index(f0 + r, ut * 8) * 2;   // units ut*8 .. +7 of frame f0 + r: one 16-byte slot
        ita_publish_h8(pub, r, ita_rsrc(a.p2_hi), o, ita_rsrc(a.p2_lo), o);
      }
    }
    const unsigned prev = ita_head_arrive(a.cnt, ft, tid);
    if (tid == 0 && l == 2) flag = prev == 47u ? 1u : 0u;   // 3 x 16 arrivals: this workgroup is the tile's last
  }

  // ---- fc on the tile's last arriver: no wait; every other workgroup of the tile has published its h_out2
  __syncthreads();
  if (!flag) return;
  if (tid == 0) __hip_atomic_store(a.cnt + ft * ITA_HEAD_CNT_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
  float (*fw)[128] = (float (*)[128])(big + 32 * 132);   // fc weights [3][128]
  int fro[4];   // 32 rows x 128 of h_out2 (sc1 loads: handed-off bytes) and the fc weights, one round trip
#pragma unroll
  for (int i = 0; i < 4; ++i) fro[i] = min(f0 + ((i * 256 + tid) >> 5), B - 1);
  if (a.slots) {
#pragma unroll
    for (int i = 0; i < 4; ++i) fro[i] = a.slots[fro[i]];
  }
  f32x4 hr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    hr[i] = ita_load_sc1_f32x4(ita_rsrc(a.h_out), (int)((2 * a.lstride + (size_t)fro[i] * 128 + 4 * (tid & 31)) * 4));
  const f32x4 wv = *(const f32x4*)(a.fc_w + 4 * min(tid, 95));
#pragma unroll
  for (int i = 0; i < 4; ++i) *(f32x4*)&hs[(i * 256 + tid) >> 5][4 * (tid & 31)] = hr[i];
  if (tid < 96) *(f32x4*)&fw[tid >> 5][4 * (tid & 31)] = wv;
  __syncthreads();
  lstm_fc_rows(hs, fw, a.fc_b, a.vel, 0, f0, B, tid, [](int) { return true; });
}
