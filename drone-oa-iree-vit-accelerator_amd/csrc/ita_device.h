// ita_device.h -- device-side helpers shared by the gfx950 kernels.
//
// Conventions used by every int8 kernel in this directory
// -------------------------------------------------------
// * All int8 GEMMs are "NT": C[m][n] = sum_k A[m][k] * Bt[n][k], both operands k-contiguous,
//   so one MFMA fragment is 16 contiguous bytes of one row.  The integer sum does not care
//   which k a fragment byte really is, only that A and Bt use the same slot -> k mapping,
//   which lets the attention kernel feed softmax outputs straight from registers (see
//   ita_int8_kernels.h).
// * int8 operand matrices that live in LDS are stored "chunk-major": [k/16][row][16 bytes].
//   A wave's ds_read_b128 of one fragment column then touches 16 consecutive 16-byte slots per
//   lane group -> conflict-free for both the 32x32x32 and the 16x16x64 MFMA access patterns,
//   with no padding.
// * v_mfma_i32_32x32x32_i8 : A lane l -> row l&31, k-slot group l>>5 (16 bytes);
//                            C lane l -> col l&31, row (i&3) + 8*(i>>2) + 4*(l>>5), i = 0..15
//   v_mfma_i32_16x16x64_i8 : A lane l -> row l&15, k-slot group l>>4 (16 bytes);
//                            C lane l -> col l&15, row 4*(l>>4) + i, i = 0..3
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Buffer resource over everything from p on (raw, no bounds in use: the callers keep their offsets below 2 GB).  p must be
// wave-uniform, the per-lane part of an address goes into the byte offset of the load / store.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ita_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, 0x7FFFFFFF, 0x00020000);
}
constexpr int ITA_SC1 = 16;   // buffer load / store cache policy: write-through store, L1-bypassing load

// Write-through hand-overs: what one launch of a step writes for the NEXT launch to read leaves the
// XCD's L2 while the producer still computes when it is stored sc1, instead of as dirty lines at the kernel boundary.
// 16 bytes to base + byte_off; without WRITE_THROUGH the same buffer store with no cache policy.
template <bool WRITE_THROUGH>
__device__ __forceinline__ void ita_store16(__amdgpu_buffer_rsrc_t base, int byte_off, u32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, base, byte_off, 0, WRITE_THROUGH ? ITA_SC1 : 0);
}

#define ITA_MAGIC_F 12582912.0f   /* 1.5 * 2^23: adding it rounds to nearest-even integer */
#define ITA_MAGIC_I 0x4B400000

// byte offset of (row, k-byte) in a chunk-major int8 matrix with ROWS rows
__device__ __forceinline__ int cm_off(int row, int kb, int rows) {
  return ((((kb >> 4) * rows) + row) << 4) | (kb & 15);
}

// nnq requantisation: clamp(rne(float(acc) * mult), lo, 127).  The clamp is applied before the
// rounding (same result, the bounds are integers); the rounding is the fp32 add of 1.5*2^23,
// whose mantissa then holds the two's-complement integer: returns those bits.
__device__ __forceinline__ unsigned rq_bits(int acc, float mult, float lo = -128.0f) {
  float f = (float)acc * mult;
  f = __builtin_amdgcn_fmed3f(f, lo, 127.0f);
  f = f + ITA_MAGIC_F;
  return __float_as_uint(f);
}
__device__ __forceinline__ unsigned q_bits(float x, float inv_scale) {   // torch.quantize_per_tensor
  float f = x * inv_scale;
  f = __builtin_amdgcn_fmed3f(f, -128.0f, 127.0f);
  f = f + ITA_MAGIC_F;
  return __float_as_uint(f);
}
__device__ __forceinline__ int bits_to_int(unsigned b) { return (int)b - ITA_MAGIC_I; }

// Round sixteen already-clamped floats to nearest-even integers and pack their low bytes into
// four dwords: pk[g] byte b = rne(f[4g + b]).  The rounding is the fp32 add of 1.5*2^23 (the
// mantissa then holds the two's-complement integer); SDWA writes the low byte of each sum straight
// into byte b of the destination, so the add IS the pack: 16 VALU instructions for 16 bytes instead
// of 16 adds + 20 and/shift/or.  gfx950 hazard (measured, tools/... sdwa micro test): a VALU that
// reads a VGPR written by the immediately preceding dst_sel instruction sees stale bytes, and
// inline asm is not padded by hipcc -- so the four destinations are interleaved (3 independent
// instructions between two writes of one register) and the statement ends with one wait state.
__device__ __forceinline__ void round_pack16(const float (&f)[16], unsigned (&pk)[4]) {
  const float mg = ITA_MAGIC_F;
  asm(
      "v_add_f32_sdwa %0, %4, %20 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %1, %8, %20 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %2, %12, %20 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %3, %16, %20 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %0, %5, %20 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %1, %9, %20 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %2, %13, %20 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %3, %17, %20 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %0, %6, %20 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %1, %10, %20 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %2, %14, %20 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %3, %18, %20 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %0, %7, %20 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %1, %11, %20 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %2, %15, %20 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "v_add_f32_sdwa %3, %19, %20 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\t"
      "s_nop 0"
      : "=&v"(pk[0]), "=&v"(pk[1]), "=&v"(pk[2]), "=&v"(pk[3])
      : "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7]), "v"(f[8]), "v"(f[9]),
        "v"(f[10]), "v"(f[11]), "v"(f[12]), "v"(f[13]), "v"(f[14]), "v"(f[15]), "v"(mg));
}
__device__ __forceinline__ float rq_clamped(int acc, float mult, float lo) {
  return __builtin_amdgcn_fmed3f((float)acc * mult, lo, 127.0f);
}
// requantise + pack a 16-accumulator fragment: pk[g] = bytes of acc[4g .. 4g+3]
typedef float f32x2 __attribute__((ext_vector_type(2)));
// f[i] = clamp(float(acc[i]) * mult, lo, 127) for N accumulators.  Non-packed VALU issues one
// wave-instruction per 4 cycles per SIMD on gfx950; v_pk_mul_f32 does two multiplies in that slot, so the
// scale step is written on float2 values.
template <int N, typename ACC>
__device__ __forceinline__ void scale_clamp(const ACC& acc, float mult, float lo, float (&f)[N]) {
  const f32x2 m2 = {mult, mult};
#pragma unroll
  for (int i = 0; i < N; i += 2) {
    f32x2 v = {(float)acc[i], (float)acc[i + 1]};
    v = v * m2;
    f[i] = __builtin_amdgcn_fmed3f(v.x, lo, 127.0f);
    f[i + 1] = __builtin_amdgcn_fmed3f(v.y, lo, 127.0f);
  }
}
// The same for accumulators that were started at ITA_ACC_BIAS (+ bias) instead of (bias): while |sum| < 2^22 the
// int32 bit pattern 0x4B400000 + sum IS the float 1.5 * 2^23 + sum, so the int -> float conversion becomes an exact
// float subtraction.  On gfx950 v_sub_f32 / v_mul_f32 issue at twice the rate of v_cvt_f32_i32 / v_pk_mul_f32 when two
// waves share a SIMD (tools/microbench/valu_ops.hip).
#define ITA_ACC_BIAS 0x4B400000
template <int N, typename ACC>
__device__ __forceinline__ void scale_clamp_b(const ACC& acc, float mult, float lo, float (&f)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float x = __int_as_float(acc[i]) - ITA_MAGIC_F;
    f[i] = __builtin_amdgcn_fmed3f(x * mult, lo, 127.0f);
  }
}
// ---- fixed-schedule requantisation of biased accumulators (ITA_ACC_BIAS).  What limits the encoder kernel is the
// NUMBER of VALU instructions a SIMD issues (measured: 4.0 cycles of SQ_ACTIVE_INST_VALU per instruction whatever its
// class, two waves per SIMD), so the steps that exist in packed form run packed -- v_pk_add_f32 / v_pk_mul_f32 handle two
// values per instruction -- and every block is one asm statement in an order where consecutive instructions never depend
// on each other (left to itself hipcc funnels all values through one temporary, and a dependent VALU instruction
// issues ~1.7x slower).  mult / lo / scale must be wave-uniform.
// Hazard: hipcc pads MFMA -> VALU read wait states for its own instructions, not for inline asm; an accumulator may come
// from a 4-pass MFMA issued immediately before (7-8 wait states on gfx950), so the first block opens with ten.
// eight register pairs: x = (x - 1.5 * 2^23) * mult
__device__ __forceinline__ void pk_unbias_scale(f32x2 (&x)[8], float mult) {
  const f32x2 c2 = {-ITA_MAGIC_F, -ITA_MAGIC_F}, m2 = {mult, mult};
  asm("s_nop 7\n\ts_nop 1\n\t"
      "v_pk_add_f32 %0, %0, %8\n\t"
      "v_pk_add_f32 %1, %1, %8\n\t"
      "v_pk_add_f32 %2, %2, %8\n\t"
      "v_pk_add_f32 %3, %3, %8\n\t"
      "v_pk_add_f32 %4, %4, %8\n\t"
      "v_pk_add_f32 %5, %5, %8\n\t"
      "v_pk_add_f32 %6, %6, %8\n\t"
      "v_pk_add_f32 %7, %7, %8\n\t"
      "v_pk_mul_f32 %0, %0, %9\n\t"
      "v_pk_mul_f32 %1, %1, %9\n\t"
      "v_pk_mul_f32 %2, %2, %9\n\t"
      "v_pk_mul_f32 %3, %3, %9\n\t"
      "v_pk_mul_f32 %4, %4, %9\n\t"
      "v_pk_mul_f32 %5, %5, %9\n\t"
      "v_pk_mul_f32 %6, %6, %9\n\t"
      "v_pk_mul_f32 %7, %7, %9"
      : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
      : "s"(c2), "s"(m2));
}
// sixteen biased accumulators -> their int8 codes as floats, f[4t+i] = clamp(rne(acc[t][i] * mult)): 8 + 8 + 16 + 16
__device__ __forceinline__ void rq16_b_f(const i32x4 (&acc)[4], float mult, float (&f)[16]) {
  f32x2 x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (f32x2){__int_as_float(acc[k >> 1][2 * (k & 1)]), __int_as_float(acc[k >> 1][2 * (k & 1) + 1])};
  pk_unbias_scale(x, mult);
#pragma unroll
  for (int k = 0; k < 8; ++k) { f[2 * k] = x[k].x; f[2 * k + 1] = x[k].y; }
  const float lo = -128.0f, hi = 127.0f;
  asm(
      "v_med3_f32 %0, %0, %16, %17\n\t"
      "v_med3_f32 %1, %1, %16, %17\n\t"
      "v_med3_f32 %2, %2, %16, %17\n\t"
      "v_med3_f32 %3, %3, %16, %17\n\t"
      "v_med3_f32 %4, %4, %16, %17\n\t"
      "v_med3_f32 %5, %5, %16, %17\n\t"
      "v_med3_f32 %6, %6, %16, %17\n\t"
      "v_med3_f32 %7, %7, %16, %17\n\t"
      "v_med3_f32 %8, %8, %16, %17\n\t"
      "v_med3_f32 %9, %9, %16, %17\n\t"
      "v_med3_f32 %10, %10, %16, %17\n\t"
      "v_med3_f32 %11, %11, %16, %17\n\t"
      "v_med3_f32 %12, %12, %16, %17\n\t"
      "v_med3_f32 %13, %13, %16, %17\n\t"
      "v_med3_f32 %14, %14, %16, %17\n\t"
      "v_med3_f32 %15, %15, %16, %17\n\t"
      "v_rndne_f32 %0, %0\n\t"
      "v_rndne_f32 %1, %1\n\t"
      "v_rndne_f32 %2, %2\n\t"
      "v_rndne_f32 %3, %3\n\t"
      "v_rndne_f32 %4, %4\n\t"
      "v_rndne_f32 %5, %5\n\t"
      "v_rndne_f32 %6, %6\n\t"
      "v_rndne_f32 %7, %7\n\t"
      "v_rndne_f32 %8, %8\n\t"
      "v_rndne_f32 %9, %9\n\t"
      "v_rndne_f32 %10, %10\n\t"
      "v_rndne_f32 %11, %11\n\t"
      "v_rndne_f32 %12, %12\n\t"
      "v_rndne_f32 %13, %13\n\t"
      "v_rndne_f32 %14, %14\n\t"
      "v_rndne_f32 %15, %15"
      : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]), "+v"(f[8]), "+v"(f[9]),
        "+v"(f[10]), "+v"(f[11]), "+v"(f[12]), "+v"(f[13]), "+v"(f[14]), "+v"(f[15])
      : "s"(lo), "v"(hi));
}
// block output: d[4t+i] = float(int8 code) * scale for sixteen biased accumulators: rq16_b_f + 8; c (taps): the codes
__device__ __forceinline__ void dq16_b(const i32x4 (&acc)[4], float mult, float scale, float (&d)[16], float (&c)[16]) {
  rq16_b_f(acc, mult, c);
  const f32x2 s2 = {scale, scale};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const f32x2 v = (f32x2){c[2 * k], c[2 * k + 1]} * s2;
    d[2 * k] = v.x; d[2 * k + 1] = v.y;
  }
}
__device__ __forceinline__ void dq16_b(const i32x4 (&acc)[4], float mult, float scale, float (&d)[16]) {
  float c[16];
  dq16_b(acc, mult, scale, d, c);
}
// v_pk_fma_f32 x, x, s[p:p+1], s[p:p+1] with the SGPR pair {m, K}: x * m + K in both halves (the operand modifiers hipcc
// itself emits for a splat of each dword)
#define ITA_PK_MK "op_sel:[0,0,1] op_sel_hi:[1,0,1]"
// The fused dequantise form of the same block output (out_proj, fc2; ita_weights_load.h: fused_site with dq): the accumulators
// started at the site's own integer base C, t = fma(acc_bits, m, K) with K = 1.5 * 2^23 - round(C m) in ONE v_pk_fma_f32 per
// pair -- an integer of [2^23, 2^24), rounded once --, r = t - 1.5 * 2^23 (v_pk_add_f32, exact), the float clamp, the scale:
// 8 + 8 + 16 + 8 = 2.5 instructions per value instead of 3.5.  Permitted per site by the load-time enumeration of the whole
// clamp range against the reference's two roundings; beyond that range both forms clamp (the fma is monotone).
// (m and K travel as one SGPR pair, see pk_requant_round.)
// Sign of zero: the two-rounding form yields -0.0 for a small negative accumulator (v_rndne_f32 keeps the sign), t - 1.5 * 2^23
// yields +0.0.  The proof compares codes, where the two are one; d differs in the sign bit only, and the residual x + d only
// when x is -0.0 as well, which compares equal and which the LayerNorm that follows maps to the same bits.
__device__ __forceinline__ void dq16_fused(const i32x4 (&acc)[4], float mult, float kf, float scale, float (&d)[16]) {
  f32x2 x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (f32x2){__int_as_float(acc[k >> 1][2 * (k & 1)]), __int_as_float(acc[k >> 1][2 * (k & 1) + 1])};
  const f32x2 c2 = {-ITA_MAGIC_F, -ITA_MAGIC_F}, mk = {mult, kf};
  asm("s_nop 7\n\ts_nop 1\n\t"
      "v_pk_fma_f32 %0, %0, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %1, %1, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %2, %2, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %3, %3, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %4, %4, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %5, %5, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %6, %6, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_fma_f32 %7, %7, %8, %8 " ITA_PK_MK "\n\t"
      "v_pk_add_f32 %0, %0, %9\n\t"
      "v_pk_add_f32 %1, %1, %9\n\t"
      "v_pk_add_f32 %2, %2, %9\n\t"
      "v_pk_add_f32 %3, %3, %9\n\t"
      "v_pk_add_f32 %4, %4, %9\n\t"
      "v_pk_add_f32 %5, %5, %9\n\t"
      "v_pk_add_f32 %6, %6, %9\n\t"
      "v_pk_add_f32 %7, %7, %9"
      : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
      : "s"(mk), "s"(c2));
  float f[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) { f[2 * k] = x[k].x; f[2 * k + 1] = x[k].y; }
  const float lo = -128.0f, hi = 127.0f;
  asm("v_med3_f32 %0, %0, %16, %17\n\t"
      "v_med3_f32 %1, %1, %16, %17\n\t"
      "v_med3_f32 %2, %2, %16, %17\n\t"
      "v_med3_f32 %3, %3, %16, %17\n\t"
      "v_med3_f32 %4, %4, %16, %17\n\t"
      "v_med3_f32 %5, %5, %16, %17\n\t"
      "v_med3_f32 %6, %6, %16, %17\n\t"
      "v_med3_f32 %7, %7, %16, %17\n\t"
      "v_med3_f32 %8, %8, %16, %17\n\t"
      "v_med3_f32 %9, %9, %16, %17\n\t"
      "v_med3_f32 %10, %10, %16, %17\n\t"
      "v_med3_f32 %11, %11, %16, %17\n\t"
      "v_med3_f32 %12, %12, %16, %17\n\t"
      "v_med3_f32 %13, %13, %16, %17\n\t"
      "v_med3_f32 %14, %14, %16, %17\n\t"
      "v_med3_f32 %15, %15, %16, %17"
      : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]), "+v"(f[8]), "+v"(f[9]),
        "+v"(f[10]), "+v"(f[11]), "+v"(f[12]), "+v"(f[13]), "+v"(f[14]), "+v"(f[15])
      : "s"(lo), "v"(hi));
  const f32x2 s2 = {scale, scale};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const f32x2 v = (f32x2){f[2 * k], f[2 * k + 1]} * s2;
    d[2 * k] = v.x; d[2 * k + 1] = v.y;
  }
}
// ---- round-3 requantisation of biased accumulators: the clamp moves behind the rounding, into the integer domain, where
// ONE instruction saturates two values (v_sat_pk_u8_i16) -- 2.75 VALU instructions per value instead of 3.0, and 2.25 where a
// load-time proof allows the single-rounding form:
//   exact : x = acc_bits - 1.5*2^23 (v_pk_add_f32, exact) ; y = fl(x * m) (v_pk_mul_f32: the reference's first rounding) ;
//           t = y + (1.5*2^23 + 128) (v_pk_add_f32: rounds to nearest-even INTEGER, the reference's second rounding; the low
//           16 bits of t's pattern are then r + 128 in two's complement, r = rne(y), provided |r + 128| < 2^15 -- checked per
//           weight row at load time, stream_range_ok) ; pairs of low halves -> one dword (v_perm_b32) ; u8 saturation of
//           both halves = clamp(r, -128, 127) + 128 (v_sat_pk_u8_i16, SDWA places the two bytes) ; ^ 0x80808080 per dword.
//   fast  : t = fma(x, m, 1.5*2^23 + 128) in ONE v_pk_fma_f32 -- a single rounding of the exact product.  It differs from
//           the reference's two roundings only for accumulator values whose exact product lies within half an ulp of a
//           rounding tie without being one; ita_load_weights enumerates every accumulator value of the clamp range for the
//           site's multiplier (fast_site_ok) and enables this form only when none differs.
//   fused : the accumulator was started at an integer C chosen per site at load time instead of at 1.5*2^23 (its pattern is
//           still the float C + sum), and t = fma(acc_bits, m, K), K = magic - round(C m), in ONE v_pk_fma_f32 and nothing
//           else: 1.75 instructions per value.  C is picked so that C m lies within ~1e-6 of an integer; the same
//           enumeration as for the fast form then shows that no accumulator value of the clamp range lands that close to a
//           tie (ita_weights_load.h: fused_site), else the site, and with it the layer, keeps the fast or exact form.
//   fused relu : the fused form against K = 1.5*2^23 - round(C m), no + 128: the low 16 bits are r itself, signed; one
//           v_pk_min_i16 with 127 per pair, then the u8 saturation clamps at 0: the codes are 0 .. 127 and need no sign
//           flip -- 2.0 instructions per value.  Proven per multiplier like the fused form, on codes clamped to [0, 127].
//   relu  : the exact form with the lower clamp moved into the multiply: y/256 = fl(x * (m/256)) with the VOP3P clamp
//           modifier ([0, 1] <-> y in [0, 256]), t = y/256 + (1.5*2^23 + 128)/256 (ulp 2^-8: same integer rounding, same low
//           bits), the u8 saturation then gives min(r, 127) + 128.
#define ITA_MAGIC128_F 12583040.0f        /* 1.5 * 2^23 + 128 */
#define ITA_MAGIC32K_F 12615680.0f        /* 1.5 * 2^23 + 32768: low 16 bits = r + 32768 = r ^ 0x8000 (order-preserving u16) */
enum { ITA_RQ_EXACT = 0, ITA_RQ_FAST = 1, ITA_RQ_RELU = 2, ITA_RQ_FUSED = 3, ITA_RQ_FUSED_RELU = 4 };

template <int NP, int MODE>   // NP register pairs: acc bit patterns -> float patterns whose low 16 bits hold rne(acc * mult) + bias
__device__ __forceinline__ void pk_requant_round(f32x2 (&x)[NP], float mult, float magic) {
  static_assert(NP == 8 || NP == 4, "");
  const f32x2 c2 = {-ITA_MAGIC_F, -ITA_MAGIC_F};
  if constexpr (MODE == ITA_RQ_FUSED || MODE == ITA_RQ_FUSED_RELU) {
    // `magic` is the site's K = magic - round(C m); the accumulators were started at the site's C.  The multiplier and K
    // travel as ONE SGPR pair {m, K} (ItaStreamArgs::mk*): the op_sel bits pick dword 0 for both halves of src1 and dword 1 for
    // both halves of src2, and one pair read twice is one scalar operand -- no copy of K into VGPRs (ITA_PK_MK)
    const f32x2 mk = {mult, magic};
    if constexpr (NP == 8) {
      f32x2 y[8];
      asm("s_nop 7\n\ts_nop 1\n\t"
        "v_pk_fma_f32 %0, %9, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %1, %10, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %2, %11, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %3, %12, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %4, %13, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %5, %14, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %6, %15, %8, %8 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %7, %16, %8, %8 " ITA_PK_MK
          : "=&v"(y[0]), "=&v"(y[1]), "=&v"(y[2]), "=&v"(y[3]), "=&v"(y[4]), "=&v"(y[5]), "=&v"(y[6]), "=&v"(y[7])
          : "s"(mk), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]));
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] = y[k];
    } else {
      f32x2 y[4];
      asm("s_nop 7\n\ts_nop 1\n\t"
        "v_pk_fma_f32 %0, %5, %4, %4 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %1, %6, %4, %4 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %2, %7, %4, %4 " ITA_PK_MK "\n\t"
        "v_pk_fma_f32 %3, %8, %4, %4 " ITA_PK_MK
          : "=&v"(y[0]), "=&v"(y[1]), "=&v"(y[2]), "=&v"(y[3])
          : "s"(mk), "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]));
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = y[k];
    }
  } else if constexpr (MODE == ITA_RQ_FAST) {
    // (an instruction reads at most one SGPR operand: the magic constant is copied into a VGPR pair inside the block -- as a
    //  loop-invariant VGPR pair the compiler would hoist it out of the frame loop and, at 256 registers, spill it)
    const f32x2 m2 = {mult, mult}, g2s = {magic, magic};
    f32x2 g2;
    if constexpr (NP == 8) {
      asm("s_nop 7\n\ts_nop 1\n\t"
        "v_pk_mov_b32 %8, %11, %11\n\t"
        "v_pk_add_f32 %0, %0, %9\n\t"
        "v_pk_add_f32 %1, %1, %9\n\t"
        "v_pk_add_f32 %2, %2, %9\n\t"
        "v_pk_add_f32 %3, %3, %9\n\t"
        "v_pk_add_f32 %4, %4, %9\n\t"
        "v_pk_add_f32 %5, %5, %9\n\t"
        "v_pk_add_f32 %6, %6, %9\n\t"
        "v_pk_add_f32 %7, %7, %9\n\t"
        "v_pk_fma_f32 %0, %0, %10, %8\n\t"
        "v_pk_fma_f32 %1, %1, %10, %8\n\t"
        "v_pk_fma_f32 %2, %2, %10, %8\n\t"
        "v_pk_fma_f32 %3, %3, %10, %8\n\t"
        "v_pk_fma_f32 %4, %4, %10, %8\n\t"
        "v_pk_fma_f32 %5, %5, %10, %8\n\t"
        "v_pk_fma_f32 %6, %6, %10, %8\n\t"
        "v_pk_fma_f32 %7, %7, %10, %8"
          : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]), "=&v"(g2)
          : "s"(c2), "s"(m2), "s"(g2s));
    } else {
      asm("s_nop 7\n\ts_nop 1\n\t"
        "v_pk_mov_b32 %4, %7, %7\n\t"
        "v_pk_add_f32 %0, %0, %5\n\t"
        "v_pk_add_f32 %1, %1, %5\n\t"
        "v_pk_add_f32 %2, %2, %5\n\t"
        "v_pk_add_f32 %3, %3, %5\n\t"
        "v_pk_fma_f32 %0, %0, %6, %4\n\t"
        "v_pk_fma_f32 %1, %1, %6, %4\n\t"
        "v_pk_fma_f32 %2, %2, %6, %4\n\t"
        "v_pk_fma_f32 %3, %3, %6, %4"
          : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "=&v"(g2)
          : "s"(c2), "s"(m2), "s"(g2s));
    }
  } else {
    // (RELU: the caller passes mult / 256 and magic / 256 -- both exact power-of-two scalings)
    const f32x2 m2 = {mult, mult}, g2 = {magic, magic};
    if constexpr (NP == 8) {
      if constexpr (MODE == ITA_RQ_RELU) {
        asm("s_nop 7\n\ts_nop 1\n\t"
          "v_pk_add_f32 %0, %0, %8\n\t"
          "v_pk_add_f32 %1, %1, %8\n\t"
          "v_pk_add_f32 %2, %2, %8\n\t"
          "v_pk_add_f32 %3, %3, %8\n\t"
          "v_pk_add_f32 %4, %4, %8\n\t"
          "v_pk_add_f32 %5, %5, %8\n\t"
          "v_pk_add_f32 %6, %6, %8\n\t"
          "v_pk_add_f32 %7, %7, %8\n\t"
          "v_pk_mul_f32 %0, %0, %9 clamp\n\t"
          "v_pk_mul_f32 %1, %1, %9 clamp\n\t"
          "v_pk_mul_f32 %2, %2, %9 clamp\n\t"
          "v_pk_mul_f32 %3, %3, %9 clamp\n\t"
          "v_pk_mul_f32 %4, %4, %9 clamp\n\t"
          "v_pk_mul_f32 %5, %5, %9 clamp\n\t"
          "v_pk_mul_f32 %6, %6, %9 clamp\n\t"
          "v_pk_mul_f32 %7, %7, %9 clamp\n\t"
          "v_pk_add_f32 %0, %0, %10\n\t"
          "v_pk_add_f32 %1, %1, %10\n\t"
          "v_pk_add_f32 %2, %2, %10\n\t"
          "v_pk_add_f32 %3, %3, %10\n\t"
          "v_pk_add_f32 %4, %4, %10\n\t"
          "v_pk_add_f32 %5, %5, %10\n\t"
          "v_pk_add_f32 %6, %6, %10\n\t"
          "v_pk_add_f32 %7, %7, %10"
            : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
            : "s"(c2), "s"(m2), "s"(g2));
      } else {
        asm("s_nop 7\n\ts_nop 1\n\t"
          "v_pk_add_f32 %0, %0, %8\n\t"
          "v_pk_add_f32 %1, %1, %8\n\t"
          "v_pk_add_f32 %2, %2, %8\n\t"
          "v_pk_add_f32 %3, %3, %8\n\t"
          "v_pk_add_f32 %4, %4, %8\n\t"
          "v_pk_add_f32 %5, %5, %8\n\t"
          "v_pk_add_f32 %6, %6, %8\n\t"
          "v_pk_add_f32 %7, %7, %8\n\t"
          "v_pk_mul_f32 %0, %0, %9\n\t"
          "v_pk_mul_f32 %1, %1, %9\n\t"
          "v_pk_mul_f32 %2, %2, %9\n\t"
          "v_pk_mul_f32 %3, %3, %9\n\t"
          "v_pk_mul_f32 %4, %4, %9\n\t"
          "v_pk_mul_f32 %5, %5, %9\n\t"
          "v_pk_mul_f32 %6, %6, %9\n\t"
          "v_pk_mul_f32 %7, %7, %9\n\t"
          "v_pk_add_f32 %0, %0, %10\n\t"
          "v_pk_add_f32 %1, %1, %10\n\t"
          "v_pk_add_f32 %2, %2, %10\n\t"
          "v_pk_add_f32 %3, %3, %10\n\t"
          "v_pk_add_f32 %4, %4, %10\n\t"
          "v_pk_add_f32 %5, %5, %10\n\t"
          "v_pk_add_f32 %6, %6, %10\n\t"
          "v_pk_add_f32 %7, %7, %10"
            : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])
            : "s"(c2), "s"(m2), "s"(g2));
      }
    } else {
      static_assert(MODE != ITA_RQ_RELU, "the ReLU site has 8 pairs");
      asm("s_nop 7\n\ts_nop 1\n\t"
        "v_pk_add_f32 %0, %0, %4\n\t"
        "v_pk_add_f32 %1, %1, %4\n\t"
        "v_pk_add_f32 %2, %2, %4\n\t"
        "v_pk_add_f32 %3, %3, %4\n\t"
        "v_pk_mul_f32 %0, %0, %5\n\t"
        "v_pk_mul_f32 %1, %1, %5\n\t"
        "v_pk_mul_f32 %2, %2, %5\n\t"
        "v_pk_mul_f32 %3, %3, %5\n\t"
        "v_pk_add_f32 %0, %0, %6\n\t"
        "v_pk_add_f32 %1, %1, %6\n\t"
        "v_pk_add_f32 %2, %2, %6\n\t"
        "v_pk_add_f32 %3, %3, %6"
          : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3])
          : "s"(c2), "s"(m2), "s"(g2));
    }
  }
}
// eight dwords of two 16-bit (r + 128) values each -> four dwords of four int8 codes: u8 saturation of both halves
// (= clamp(r, -128, 127) + 128), SDWA places the byte pair in the low / high word, ^ 0x80 per byte.  Same SDWA hazard rule
// as round_pack16: four destinations interleaved, one wait state at the end.
__device__ __forceinline__ i32x4 sat_pack16(const unsigned (&w)[8]) {
  unsigned p0, p1, p2, p3;
  const unsigned flip = 0x80808080u;
  asm(
      "v_sat_pk_u8_i16_sdwa %0, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %1, %6 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %2, %8 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %3, %10 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %0, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %1, %7 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %2, %9 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %3, %11 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_xor_b32 %0, %12, %0\n\t"
      "v_xor_b32 %1, %12, %1\n\t"
      "v_xor_b32 %2, %12, %2\n\t"
      "v_xor_b32 %3, %12, %3\n\t"
      "s_nop 0"
      : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
      : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]), "s"(flip));
  return (i32x4){(int)p0, (int)p1, (int)p2, (int)p3};
}
// the same for the fused ReLU form: the halves hold r (no + 128); min(r, 127) per half, then the u8 saturation = clamp(r, 0, 127)
__device__ __forceinline__ i32x4 sat_pack16_relu(unsigned (&w)[8]) {
  unsigned p0, p1, p2, p3;
  const unsigned c127 = 0x007F007Fu;
  asm(
      "v_pk_min_i16 %4, %4, %12\n\t"
      "v_pk_min_i16 %5, %5, %12\n\t"
      "v_pk_min_i16 %6, %6, %12\n\t"
      "v_pk_min_i16 %7, %7, %12\n\t"
      "v_pk_min_i16 %8, %8, %12\n\t"
      "v_pk_min_i16 %9, %9, %12\n\t"
      "v_pk_min_i16 %10, %10, %12\n\t"
      "v_pk_min_i16 %11, %11, %12\n\t"
      "v_sat_pk_u8_i16_sdwa %0, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %1, %6 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %2, %8 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %3, %10 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %0, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %1, %7 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %2, %9 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "v_sat_pk_u8_i16_sdwa %3, %11 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n\t"
      "s_nop 0"
      : "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3), "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]),
        "+v"(w[6]), "+v"(w[7])
      : "s"(c127));
  return (i32x4){(int)p0, (int)p1, (int)p2, (int)p3};
}
// requantise + pack sixteen biased accumulators (four 16x16 tiles): byte 4t + i of the result <-> acc[t][i]
// (kf: the site's K of the fused form, unused by the others)
template <int MODE>
__device__ __forceinline__ i32x4 rq_pack16_v3(const i32x4 (&acc)[4], float mult, float kf = 0.0f) {
  f32x2 x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = (f32x2){__int_as_float(acc[k >> 1][2 * (k & 1)]), __int_as_float(acc[k >> 1][2 * (k & 1) + 1])};
  if constexpr (MODE == ITA_RQ_RELU) pk_requant_round<8, MODE>(x, mult * 0.00390625f, ITA_MAGIC128_F * 0.00390625f);
  else pk_requant_round<8, MODE>(x, mult, (MODE == ITA_RQ_FUSED || MODE == ITA_RQ_FUSED_RELU) ? kf : ITA_MAGIC128_F);
  unsigned w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)   // {lo16(x.x), lo16(x.y)}
    w[k] = __builtin_amdgcn_perm(__float_as_uint(x[k].y), __float_as_uint(x[k].x), 0x05040100u);
  if constexpr (MODE == ITA_RQ_FUSED_RELU) return sat_pack16_relu(w);
  return sat_pack16(w);
}
// logits: eight biased accumulators (two key tiles) -> four dwords of two ORDER-PRESERVING u16 each: rne(acc * mult) + 32768,
// unclamped (the integer softmax clamps: ita_softmax_packed16).  Pair k <-> acc[k >> 1][2 (k & 1)], [.. + 1].
template <int MODE>
__device__ __forceinline__ void lg8_v3(const i32x4 (&acc)[2], float mult, unsigned (&w)[4], float kf = 0.0f) {
  f32x2 x[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = (f32x2){__int_as_float(acc[k >> 1][2 * (k & 1)]), __int_as_float(acc[k >> 1][2 * (k & 1) + 1])};
  pk_requant_round<4, MODE>(x, mult, MODE == ITA_RQ_FUSED ? kf : ITA_MAGIC32K_F);
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = __builtin_amdgcn_perm(__float_as_uint(x[k].y), __float_as_uint(x[k].x), 0x05040100u);
}
template <typename ACC>
__device__ __forceinline__ void rq_pack16(const ACC& acc, float mult, float lo, unsigned (&pk)[4]) {
  float f[16];
  scale_clamp<16>(acc, mult, lo, f);
  round_pack16(f, pk);
}
// sum of the four signed bytes of each of four packed dwords (v_dot4_i32_i8 against 0x01010101)
__device__ __forceinline__ int sum_bytes16(const unsigned (&pk)[4]) {
  int s = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) s = __builtin_amdgcn_sdot4((int)pk[g], 0x01010101, s, false);
  return s;
}
// torch.quantize_per_tensor on sixteen floats
__device__ __forceinline__ void q_pack16(const float* x, float inv_scale, unsigned (&pk)[4]) {
  float f[16];
  const f32x2 m2 = {inv_scale, inv_scale};
#pragma unroll
  for (int i = 0; i < 16; i += 2) {
    f32x2 v = {x[i], x[i + 1]};
    v = v * m2;
    f[i] = __builtin_amdgcn_fmed3f(v.x, -128.0f, 127.0f);
    f[i + 1] = __builtin_amdgcn_fmed3f(v.y, -128.0f, 127.0f);
  }
  round_pack16(f, pk);
}

__device__ __forceinline__ unsigned pack4(unsigned b0, unsigned b1, unsigned b2, unsigned b3) {
  return (b0 & 0xffu) | ((b1 & 0xffu) << 8) | ((b2 & 0xffu) << 16) | (b3 << 24);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt, i.e. it
// waits for every outstanding global store and prefetch load at each phase boundary.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// cross-lane exchanges on the VALU (no LDS round trip)
__device__ __forceinline__ int xor1_i(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); }   // quad_perm [1,0,3,2]
__device__ __forceinline__ int xor2_i(int v) { return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true); }   // quad_perm [2,3,0,1]
__device__ __forceinline__ float xor1_f(float v) { return __int_as_float(xor1_i(__float_as_int(v))); }
__device__ __forceinline__ float xor2_f(float v) { return __int_as_float(xor2_i(__float_as_int(v))); }
// value of lane ^ 16 / lane ^ 32
__device__ __forceinline__ int xor16_i(int v) {
  const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  return (int)(((threadIdx.x >> 4) & 1) ? r[0] : r[1]);
}
__device__ __forceinline__ int xor32_i(int v) {
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  return (int)(((threadIdx.x >> 5) & 1) ? r[0] : r[1]);
}

// exp with a fixed arithmetic, identical to oracle/ita_oracle.c:ita_oracle_expf
__device__ __forceinline__ float ita_expf(float x) {
  x = fminf(fmaxf(x, -87.0f), 88.0f);
  float n = rintf(x * 1.44269504088896341f);
  float r = fmaf(n, -0.693359375f, x);
  r = fmaf(n, 2.12194440e-4f, r);
  float p = 1.9875691500E-4f;
  p = fmaf(p, r, 1.3981999507E-3f);
  p = fmaf(p, r, 8.3334519073E-3f);
  p = fmaf(p, r, 4.1665795894E-2f);
  p = fmaf(p, r, 1.6666665459E-1f);
  p = fmaf(p, r, 5.0000001201E-1f);
  float r2 = r * r;
  p = fmaf(p, r2, r) + 1.0f;
  float s = __uint_as_float((unsigned)((int)n + 127) << 23);
  return p * s;
}
__device__ __forceinline__ float ita_sigmoid(float x) { return 1.0f / (1.0f + ita_expf(-x)); }
__device__ __forceinline__ float ita_tanh(float x) { return 1.0f - 2.0f / (ita_expf(2.0f * x) + 1.0f); }

// source row / column and weight of F.interpolate(mode='bilinear', align_corners=False)
__host__ __device__ __forceinline__ void bilinear_src_dev(int dst, float scale, int in, int& i0, int& ip, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.0f) src = 0.0f;
  int i = (int)src;
  if (i > in - 1) i = in - 1;
  i0 = i;
  ip = (i < in - 1) ? 1 : 0;
  l1 = src - (float)i;
}

// LayerNorm over E channels spread over 4 adjacent lanes, each holding EC = E/4 consecutive channels,
// in the oracle's summation order: 4 blocks of E/4 consecutive channels summed sequentially, combined
// (p0+p1)+(p2+p3).   r[] is overwritten with the result.
template <int E, typename WP, typename BP>
__device__ __forceinline__ void layernorm_lanes(float (&r)[E / 4], const WP& w, const BP& b, int c0) {
  constexpr int EC = E / 4;
  const float inv_e = 1.0f / (float)E;
  float p = 0.0f;
#pragma unroll
  for (int i = 0; i < EC; ++i) p = p + r[i];
  float s1 = p + xor1_f(p);
  float tot = s1 + xor2_f(s1);
  const float mean = tot * inv_e;
  p = 0.0f;
#pragma unroll
  for (int i = 0; i < EC; ++i) { float d = r[i] - mean; p = fmaf(d, d, p); }
  s1 = p + xor1_f(p);
  tot = s1 + xor2_f(s1);
  const float var = tot * inv_e;
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
  for (int i = 0; i < EC; ++i) r[i] = fmaf((r[i] - mean) * rstd, w[c0 + i], b[c0 + i]);
}

// Row epilogue of a finished block: r[EC] consecutive channels as f32 to yrow (if non-null) and, if planes are asked for,
// as f16 hi/lo planes for the folded decoder GEMM: hi = (f16)v, lo = (f16)(v - (float)hi), 8 channels per store.
template <int EC>
__device__ __forceinline__ void store_row_planes(const float (&r)[EC], float* __restrict__ yrow,
                                                 _Float16* __restrict__ hi_row, _Float16* __restrict__ lo_row) {
  if (yrow) {
#pragma unroll
    for (int i = 0; i < EC; i += 4) *(f32x4*)(yrow + i) = (f32x4){r[i], r[i + 1], r[i + 2], r[i + 3]};
  }
  if (hi_row) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
#pragma unroll
    for (int i = 0; i < EC; i += 8) {
      h8 vh, vl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const _Float16 hh = (_Float16)r[i + j];
        vh[j] = hh;
        vl[j] = (_Float16)(r[i + j] - (float)hh);
      }
      *(h8*)(hi_row + i) = vh;
      *(h8*)(lo_row + i) = vl;
    }
  }
}

// ---- one token per four lanes 16 and 32 apart: lane (qi = lane & 15, kq = lane >> 4) holds channels (E/4) kq .. + E/4 - 1 of
// token qi -- the C layout of the 16x16 MFMAs, shared by the encoder stream kernel (ita_stream_kernel.h) and the tokenizer
// (ita_tokenizer_kernel.h).
// ITA_ABLATE: diagnostic builds of those kernels (results are wrong; the bits are listed in ita_stream_kernel.h)
#ifndef ITA_ABLATE
#define ITA_ABLATE 0
#endif
// sums / maxima over the four lanes (kq = 0..3) that share a token: lane ^ 16, lane ^ 32.  With both
// operands the same register the swap leaves {row pairs duplicated} in the two results, so the
// commutative combine needs no select.
__device__ __forceinline__ float sum16_f(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float sum32_f(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ int sum1632_i(int v) {
  auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  v = (int)r[0] + (int)r[1];
  r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  return (int)r[0] + (int)r[1];
}
__device__ __forceinline__ int max1632_i(int v) {
  auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
  v = max((int)r[0], (int)r[1]);
  r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  return max((int)r[0], (int)r[1]);
}
// sum over the 16 lanes of a DPP row, the same bits in every lane of the row: rotate right by 8, 4, 2, 1 and add.  Every
// step adds a lane's value and its partner's: with v[q] the value of lane q, a[q] = v[q] + v[q + 8], b[q] = a[q] + a[q + 4],
// c[q] = b[q] + b[q + 2], sum = c[0] + c[1]
template <int CTRL>
__device__ __forceinline__ unsigned ita_row_ror(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned ita_row16_sum(unsigned v) {
  v += ita_row_ror<0x128>(v);   // row_ror:8
  v += ita_row_ror<0x124>(v);
  v += ita_row_ror<0x122>(v);
  return v + ita_row_ror<0x121>(v);
}
__device__ __forceinline__ float ita_row16_sumf(float v) {
  v = v + __uint_as_float(ita_row_ror<0x128>(__float_as_uint(v)));
  v = v + __uint_as_float(ita_row_ror<0x124>(__float_as_uint(v)));
  v = v + __uint_as_float(ita_row_ror<0x122>(__float_as_uint(v)));
  return v + __uint_as_float(ita_row_ror<0x121>(__float_as_uint(v)));
}

// LayerNorm over E channels held E/4 per lane by the four lanes qi, qi+16, qi+32, qi+48, in the oracle's
// summation order: the quarter sums p_kq sequentially over consecutive channels, combined (p0+p1)+(p2+p3)
// -- layernorm_lanes<E> (above) with the lane exchange 16 / 32 apart instead of 1 / 2.
template <int E>
__device__ __forceinline__ void layernorm_q16(float (&r)[E / 4], const float* w, const float* b, int c0) {
  constexpr int EC = E / 4;
  if constexpr (ITA_ABLATE & 16) return;
  const float inv_e = 1.0f / (float)E;
  float p = 0.0f;
#pragma unroll
  for (int i = 0; i < EC; ++i) p = p + r[i];
  float tot = sum32_f(sum16_f(p));
  const float mean = tot * inv_e;
  p = 0.0f;
#pragma unroll
  for (int i = 0; i < EC; ++i) { float d = r[i] - mean; p = fmaf(d, d, p); }
  tot = sum32_f(sum16_f(p));
  const float var = tot * inv_e;
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
  for (int i = 0; i < EC; i += 4) {
    const f32x4 w4 = *(const f32x4*)(w + c0 + i), b4 = *(const f32x4*)(b + c0 + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) r[i + j] = fmaf((r[i + j] - mean) * rstd, w4[j], b4[j]);
  }
}

// ---- f32 token rows in and out.  Lane (qi, kq) owns the quarter [E/4 kq, E/4 (kq+1)) of token qi's row.  Loaded or stored
// quarter by quarter, a wave-instruction touches 64 different cache lines for 16 bytes each -- the shape one CU moves at a
// fifth of its contiguous rate (tools/microbench/cu_fill_rows.hip).  Instead the four lanes of a token move 64 CONTIGUOUS
// bytes per instruction (16 rows x 64 B per wave-instruction) and a 4 x 4 transpose of 16-byte items across those lanes
// (lanes 16 and 32 apart: two rounds of v_permlane32_swap / v_permlane16_swap, 16 instructions) sorts the quarters out.
// raw[16 jj + 4 i + c]: item i of transpose jj = floats 4 p .. 4 p + 3 of the row, p = (E/16) i + 4 jj + kq.
template <int E>
__device__ __forceinline__ void ld_tok_items(const float* row, int kq, float (&raw)[E / 4]) {
  constexpr int PQ = E / 16, NJ = E / 64;
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v = *(const f32x4*)(row + 4 * (PQ * i + 4 * jj + kq));
      raw[16 * jj + 4 * i] = v.x; raw[16 * jj + 4 * i + 1] = v.y; raw[16 * jj + 4 * i + 2] = v.z; raw[16 * jj + 4 * i + 3] = v.w;
    }
}
// in place: items (as loaded / as they will be stored) <-> this lane's quarter in channel order; its own inverse
template <int E>
__device__ __forceinline__ void tok_items_transpose(float (&x)[E / 4]) {
  constexpr int NJ = E / 64;
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned i0 = __float_as_uint(x[16 * jj + c]), i1 = __float_as_uint(x[16 * jj + 4 + c]);
      unsigned i2 = __float_as_uint(x[16 * jj + 8 + c]), i3 = __float_as_uint(x[16 * jj + 12 + c]);
      const auto a02 = __builtin_amdgcn_permlane32_swap(i0, i2, false, false);
      const auto a13 = __builtin_amdgcn_permlane32_swap(i1, i3, false, false);
      const auto b01 = __builtin_amdgcn_permlane16_swap(a02[0], a13[0], false, false);
      const auto b23 = __builtin_amdgcn_permlane16_swap(a02[1], a13[1], false, false);
      x[16 * jj + c] = __uint_as_float(b01[0]); x[16 * jj + 4 + c] = __uint_as_float(b01[1]);
      x[16 * jj + 8 + c] = __uint_as_float(b23[0]); x[16 * jj + 12 + c] = __uint_as_float(b23[1]);
    }
}
template <int E>
__device__ __forceinline__ void st_tok_quarter(float* row, int kq, const float (&y)[E / 4]) {
  constexpr int PQ = E / 16, NJ = E / 64;
  float t[E / 4];
#pragma unroll
  for (int i = 0; i < E / 4; ++i) t[i] = y[i];
  tok_items_transpose<E>(t);
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *(f32x4*)(row + 4 * (PQ * i + 4 * jj + kq)) = (f32x4){t[16 * jj + 4 * i], t[16 * jj + 4 * i + 1], t[16 * jj + 4 * i + 2], t[16 * jj + 4 * i + 3]};
}
// the same for rows that the next launch reads: write-through stores of token `token` of the frame whose rows start at
// `frame` (wave-uniform, so the byte offsets stay below 64 KB at any batch size)
template <int E>
__device__ __forceinline__ void st_tok_quarter_next(__amdgpu_buffer_rsrc_t frame, int token, int kq, const float (&y)[E / 4]) {
  constexpr int PQ = E / 16, NJ = E / 64;
  float t[E / 4];
#pragma unroll
  for (int i = 0; i < E / 4; ++i) t[i] = y[i];
  tok_items_transpose<E>(t);
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      ita_store16<true>(frame, (token * E + 4 * (PQ * i + 4 * jj + kq)) * 4,
                        __builtin_bit_cast(u32x4, (f32x4){t[16 * jj + 4 * i], t[16 * jj + 4 * i + 1], t[16 * jj + 4 * i + 2], t[16 * jj + 4 * i + 3]}));
}
