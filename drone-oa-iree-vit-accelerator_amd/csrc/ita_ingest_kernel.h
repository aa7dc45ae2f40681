// ita_ingest_kernel.h -- refine_inputs' resize as a stage of its own: camera-resolution depth frames (u8 / u16 / f32,
// height x width, strided) -> (batch, 60, 90) f32, bilinear, align_corners = False.  Equal, bit for bit, to
// ingest_ref.py: ingest_reference, which restates ATen's area_pixel_compute_source_index with separately rounded float32
// operations.  The coordinate and blend functions below are compiled under `#pragma clang fp contract(off)`, so no
// multiply is fused with an add whatever the build's -ffp-contract says (the __f*_rn spellings mark the separately rounded
// operations for the reader; in this toolchain's headers they are plain *, +, - and would not prevent a contraction by
// themselves).  The only division of the definition that is not done on the host (scale = n / m, a kernel argument) is
// the u8 pixel's f32(code) / 255.0f, which is read from a 256-entry table the compiler's IEEE constant evaluator builds.
//
// Two kernels:
//   ita_ingest_rows_kernel    width >= 180 and a row of at most 4096 bytes.  One 256-thread workgroup per (frame, four
//                             output rows), one wave per output row: the wave stages the TWO source rows its output row
//                             blends into LDS with 16-byte-per-lane loads (narrow loads at a misaligned head and tail),
//                             then blends 90 outputs from LDS.  With scale_y >= 2 no other source row is ever fetched:
//                             a 480 x 640 frame costs 120 of its 480 rows.
//   ita_ingest_gather_kernel  everything else (small or upsampled sources, very wide rows): one thread per output, four
//                             clamped single-pixel loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ITA_INGEST_H = 60, ITA_INGEST_W = 90;
constexpr int ITA_INGEST_MAX_DIM = 4096;
constexpr int ITA_INGEST_ROW_BYTES = 4096;    // widest row ita_ingest_rows_kernel stages: 256 16-byte pieces, 4 per lane
constexpr int ITA_INGEST_LUT_BYTES = 1024;

struct ItaIngestU8Lut { float v[256]; };
constexpr ItaIngestU8Lut ita_ingest_make_u8_lut() {
  ItaIngestU8Lut t{};
  for (int i = 0; i < 256; ++i) t.v[i] = (float)i / 255.0f;   // constant-evaluated: IEEE round-to-nearest-even
  return t;
}
__device__ const ItaIngestU8Lut ita_ingest_u8_lut = ita_ingest_make_u8_lut();

// bytes of LDS one staged row takes: the row is stored at the offset of its misalignment (0..15), so that 16-byte pieces
// of global memory land on 16-byte LDS addresses
__host__ __device__ constexpr int ita_ingest_row_lds(int row_bytes) { return (row_bytes + 16 + 15) & ~15; }
__host__ __device__ constexpr int ita_ingest_rows_lds_total(int row_bytes) {
  return ITA_INGEST_LUT_BYTES + 4 * 2 * ita_ingest_row_lds(row_bytes);
}

struct ItaIngestCoord { int i0, i1; float l0, l1; };
__device__ __forceinline__ ItaIngestCoord ita_ingest_coord(float scale, int d, int n) {
#pragma clang fp contract(off)
  const float real = fmaxf(__fsub_rn(__fmul_rn(scale, __fadd_rn((float)d, 0.5f)), 0.5f), 0.0f);
  ItaIngestCoord c;
  c.i0 = min((int)real, n - 1);          // 0 <= real < 4096: the truncation is floor
  c.i1 = min(c.i0 + 1, n - 1);
  c.l1 = __fsub_rn(real, (float)c.i0);
  c.l0 = __fsub_rn(1.0f, c.l1);
  return c;
}

__device__ __forceinline__ float ita_ingest_px(uint8_t c, const float* lut, float) { return lut[c]; }
__device__ __forceinline__ float ita_ingest_px(uint16_t c, const float*, float depth_scale) {
#pragma clang fp contract(off)
  return fminf(__fmul_rn((float)c, depth_scale), 1.0f);
}
__device__ __forceinline__ float ita_ingest_px(float c, const float*, float) { return c; }

__device__ __forceinline__ float ita_ingest_blend(const ItaIngestCoord& cy, const ItaIngestCoord& cx, float a, float b,
                                                  float c, float d) {
#pragma clang fp contract(off)
  const float top = __fadd_rn(__fmul_rn(cx.l0, a), __fmul_rn(cx.l1, b));
  const float bot = __fadd_rn(__fmul_rn(cx.l0, c), __fmul_rn(cx.l1, d));
  return __fadd_rn(__fmul_rn(cy.l0, top), __fmul_rn(cy.l1, bot));
}

// One source row on its way from global memory to LDS, held in registers between the two so that the loads of both rows
// of an output row are in flight together.
template <typename T>
struct ItaIngestStage {
  uint4 body[4];
  T head, tail;
  int mis, nh, nbody, nt;   // misalignment of the row in bytes; head pixels, 16-byte pieces, tail pixels
};

// (the two staging functions are __host__ too: tools/ingest_stage_check.cpp runs them lane by lane on the CPU under
// AddressSanitizer, over every alignment and width class, against rows that end at the end of their allocation and have
// poisoned memory in front)
template <typename T>
__host__ __device__ __forceinline__ void ita_ingest_stage_load(ItaIngestStage<T>& s, const T* row, int W, int lane) {
  constexpr int PS = (int)sizeof(T);
  const int nb = W * PS;                                     // <= ITA_INGEST_ROW_BYTES
  s.mis = (int)((unsigned long long)row & 15);               // a multiple of PS: pixels are naturally aligned
  const int to_boundary = (16 - s.mis) & 15;
  const int headb = to_boundary < nb ? to_boundary : nb;
  s.nh = headb / PS;
  s.nbody = (nb - headb) >> 4;
  s.nt = (nb - headb - (s.nbody << 4)) / PS;
  // Every load stays inside the row's W pixels [row, row + W), by construction and for any base alignment:
  //   head   pixels [0, nh), nh * PS = headb <= nb: the bytes in front of the first 16-byte boundary (or the whole row);
  //   body   piece k covers bytes [headb + 16 k, headb + 16 k + 16) with k < nbody = (nb - headb) / 16 rounded DOWN, so
  //          it ends at or before byte nb; row + headb is 16-byte aligned whenever nbody > 0 (then headb was not cut
  //          short by nb), so the 16-byte load is an aligned one;
  //   tail   pixels [nh + 16 nbody / PS, same + nt) with nt * PS = nb - headb - 16 nbody: what is left, up to byte nb.
  // A row whose end is not on a 16-byte boundary is finished with single-pixel loads, never with a wide load that
  // reaches past it.
  s.head = T(0);
  s.tail = T(0);
  if (lane < s.nh) s.head = row[lane];
  const uint4* body = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(row) + headb);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    s.body[i] = make_uint4(0, 0, 0, 0);
    if (k < s.nbody) s.body[i] = body[k];
  }
  if (lane < s.nt) s.tail = row[s.nh + (s.nbody << 4) / PS + lane];
}

// st: the row's LDS region (16-byte aligned, ita_ingest_row_lds(nb) bytes); pixel p goes to byte mis + p * PS
template <typename T>
__host__ __device__ __forceinline__ void ita_ingest_stage_store(const ItaIngestStage<T>& s, unsigned char* st, int lane) {
  constexpr int PS = (int)sizeof(T);
  T* px = reinterpret_cast<T*>(st + s.mis);
  if (lane < s.nh) px[lane] = s.head;
  uint4* body = reinterpret_cast<uint4*>(st + s.mis + s.nh * PS);    // nbody > 0: mis + headb is 0 or 16
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane + 64 * i;
    if (k < s.nbody) body[k] = s.body[i];
  }
  if (lane < s.nt) px[s.nh + (s.nbody << 4) / PS + lane] = s.tail;
}

// grid: any number of workgroups <= batch * 15 (each strides over the (frame, row group) items); 256 threads; dynamic
// LDS ita_ingest_rows_lds_total(W * sizeof(T)).  Strides in pixels.
template <typename T>
__global__ __launch_bounds__(256) void ita_ingest_rows_kernel(const T* __restrict__ src, int H, int W, long long row_stride,
                                                              long long frame_stride, float scale_y, float scale_x,
                                                              float depth_scale, float* __restrict__ out, int batch) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* lut = reinterpret_cast<float*>(lds);
  lut[threadIdx.x] = ita_ingest_u8_lut.v[threadIdx.x];     // read behind the first barrier of the loop below
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row_lds = ita_ingest_row_lds(W * (int)sizeof(T));
  unsigned char* st0 = reinterpret_cast<unsigned char*>(lds) + ITA_INGEST_LUT_BYTES + wave * 2 * row_lds;
  unsigned char* st1 = st0 + row_lds;
  const long long items = (long long)batch * (ITA_INGEST_H / 4);
  // every wave of the workgroup runs the same number of iterations: the barriers are workgroup-uniform
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long frame = it / (ITA_INGEST_H / 4);
    const int oy = (int)(it % (ITA_INGEST_H / 4)) * 4 + wave;
    const ItaIngestCoord cy = ita_ingest_coord(scale_y, oy, H);
    const T* f = src + frame * frame_stride;
    ItaIngestStage<T> s0, s1;
    ita_ingest_stage_load(s0, f + cy.i0 * row_stride, W, lane);
    ita_ingest_stage_load(s1, f + cy.i1 * row_stride, W, lane);
    ita_ingest_stage_store(s0, st0, lane);
    ita_ingest_stage_store(s1, st1, lane);
    __syncthreads();
    const T* p0 = reinterpret_cast<const T*>(st0 + s0.mis);
    const T* p1 = reinterpret_cast<const T*>(st1 + s1.mis);
    float* o = out + (frame * ITA_INGEST_H + oy) * ITA_INGEST_W;
    for (int x = lane; x < ITA_INGEST_W; x += 64) {
      const ItaIngestCoord cx = ita_ingest_coord(scale_x, x, W);
      o[x] = ita_ingest_blend(cy, cx, ita_ingest_px(p0[cx.i0], lut, depth_scale), ita_ingest_px(p0[cx.i1], lut, depth_scale),
                              ita_ingest_px(p1[cx.i0], lut, depth_scale), ita_ingest_px(p1[cx.i1], lut, depth_scale));
    }
    __syncthreads();     // the staged rows are overwritten by the next item
  }
}

// grid: any number of 256-thread workgroups (they stride over the batch * 5400 outputs).  Indices are clamped to
// [0, H - 1] x [0, W - 1] by ita_ingest_coord, so every load is one pixel of the frame.
template <typename T>
__global__ __launch_bounds__(256) void ita_ingest_gather_kernel(const T* __restrict__ src, int H, int W, long long row_stride,
                                                                long long frame_stride, float scale_y, float scale_x,
                                                                float depth_scale, float* __restrict__ out, int batch) {
  __shared__ float lut[256];
  lut[threadIdx.x] = ita_ingest_u8_lut.v[threadIdx.x];
  __syncthreads();
  constexpr int PER_FRAME = ITA_INGEST_H * ITA_INGEST_W;
  const long long total = (long long)batch * PER_FRAME;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long frame = i / PER_FRAME;
    const int r = (int)(i % PER_FRAME), oy = r / ITA_INGEST_W, ox = r % ITA_INGEST_W;
    const ItaIngestCoord cy = ita_ingest_coord(scale_y, oy, H), cx = ita_ingest_coord(scale_x, ox, W);
    const T* r0 = src + frame * frame_stride + cy.i0 * row_stride;
    const T* r1 = src + frame * frame_stride + cy.i1 * row_stride;
    out[i] = ita_ingest_blend(cy, cx, ita_ingest_px(r0[cx.i0], lut, depth_scale), ita_ingest_px(r0[cx.i1], lut, depth_scale),
                              ita_ingest_px(r1[cx.i0], lut, depth_scale), ita_ingest_px(r1[cx.i1], lut, depth_scale));
  }
}
