// ita_ingest_wire_kernel.h -- the reference HOST's resize as a stage in front of the graph: camera-resolution u8 frames
// (height x width, strided) -> (batch, 60, 90) u8 wire frames, the input of the fused-tokenizer encoder path.
//
// The reference's replay host loads a PNG as 8 bits and calls stbir_resize_uint8_linear(..., 90, 60, ..., 1 channel)
// (samples/inference_trainingset_custom_dispatch/main.cpp:117-128).  In stb_image_resize2 that is: pixel = f32(code) *
// 3.9215689e-03f, Mitchell (B = C = 1/3) on an axis that shrinks, Catmull-Rom on one that grows or keeps its size, edge
// clamp, weights normalised per output pixel, code = trunc(clamp(y * 255 + 0.5)).  ingest_wire_ref.py restates it from
// those formulas; this file equals ingest_wire_ref.py bit for bit -- the table builder on the host, the kernel on the
// device -- and ingest_wire_ref.py is held to stb's own output (tests/golden/resize_stb_*.npz): every code within 1, a
// differing code only where y * 255 + 0.5 is within 1e-3 of an integer (stb sums its taps in SIMD order).
//
// Two parts:
//   ita_resize_axis / ita_resize_table   host only, plain C++ (no HIP): one axis' tables n0[n_out], count[n_out],
//                                        coeff[n_out][width]: output o = sum_j coeff[o][j] * source[n0[o] + j].
//   ita_ingest_wire_kernel               one table-driven kernel for every size: one 256-thread workgroup per (frame,
//                                        band of output rows), one wave per output row at a time.  The wave runs the
//                                        vertical pass of its row -- lanes own source columns, taps ascending, weights
//                                        wave-uniform -- into a W-float row of LDS, then the horizontal pass from LDS,
//                                        90 outputs.  With a row stride that is a multiple of 4 the columns are read as
//                                        aligned dwords (single pixels in front of the first and behind the last
//                                        aligned dword: no load leaves [row, row + W)); otherwise pixel by pixel.
//                                        Where a band's source rows fit into LDS (480 x 640: bands of 8 output rows, 88
//                                        source rows) they are staged there first with 16-byte loads, so that a source
//                                        byte is fetched once per band and not once per output row it feeds (four times
//                                        at 480 rows); larger sources (720 x 1280, 4096-pixel axes) read global memory
//                                        in the vertical pass itself.
// Every multiply and add of the definition is a float32 operation of its own: the arithmetic is compiled under
// `#pragma clang fp contract(off)`.
//
// Measured on one MI355X (tools/bench_ingest_wire.py, profiles/ingest_wire.json; 480 x 640 sources from a pool beyond
// the Infinity Cache, us per call): 19.9 at 1 frame (the host's call rate), 48.0 at 128, 342.6 at 1024 -- 7.8 x faster
// than torch's antialiased bilinear route (2 686 us) and 15.6 % of a 6.0 TB/s streaming rate over its bytes (floor
// 53 us): not bandwidth-bound.  DESIGN.md section 4 "Wire ingest" has the table and what was and was not analysed.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

constexpr int ITA_WIRE_H = 60, ITA_WIRE_W = 90;
constexpr int ITA_WIRE_MAX_DIM = 4096;

// ---- host: the tables ------------------------------------------------------------------------------------------------
struct ItaResizeAxis {
  std::vector<int> n0, count;
  std::vector<float> coeff;   // [n_out][width], zero padded
  int width = 0;
};

inline float ita_resize_mitchell(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  x = fabsf(x);
  if (x < 1.0f) return (16.0f + x * x * (21.0f * x - 36.0f)) / 18.0f;
  if (x < 2.0f) return (32.0f + x * (-60.0f + x * (36.0f - 7.0f * x))) / 18.0f;
  return 0.0f;
}

inline float ita_resize_catmull_rom(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  x = fabsf(x);
  if (x < 1.0f) return 1.0f - x * x * (2.5f - 1.5f * x);
  if (x < 2.0f) return 2.0f - x * (4.0f + x * (0.5f * x - 2.5f));
  return 0.0f;
}

// One axis, as ingest_wire_ref.py: resize_tables builds it (the comments there say why each step is what it is).
// false: n_in outside [1, 4096], n_out < 1, or a table that would leave the source (never seen; checked, not assumed).
inline bool ita_resize_axis(int n_in, int n_out, ItaResizeAxis& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (n_in < 1 || n_in > ITA_WIRE_MAX_DIM || n_out < 1 || n_out > ITA_WIRE_MAX_DIM) return false;
  const float small = ldexpf(1.0f, -120);
  const float scale = (float)n_out / (float)n_in, inv = (float)n_in / (float)n_out;
  std::vector<int> first(n_out, 0);
  std::vector<std::vector<float>> taps(n_out);
  if (scale < 1.0f) {
    const float radius = 2.0f * inv;
    const int margin = (int)ceilf(4.0f / scale) / 2;
    for (int i = -margin; i < n_in + margin; ++i) {
      const float centre = (float)i + 0.5f, oc = centre * scale;
      int lo = (int)floorf((centre - radius) * scale + 0.5f), hi = (int)floorf((centre + radius) * scale - 0.5f);
      if (lo < 0) lo = 0;
      if (hi > n_out - 1) hi = n_out - 1;
      for (int o = lo; o <= hi; ++o) {
        float c = ita_resize_mitchell(((float)o + 0.5f) - oc) * scale;
        if (c < small && c > -small) c = 0.0f;
        std::vector<float>& w = taps[o];
        if (w.empty() || (w.size() == 1 && w[0] == 0.0f)) {
          first[o] = i;
          w.assign(1, c);
        } else {
          w.resize((size_t)(i - first[o]), 0.0f);
          w.push_back(c);
        }
      }
    }
  } else {
    const float radius = 2.0f * scale;
    for (int o = 0; o < n_out; ++o) {
      const float c = (float)o + 0.5f, centre = c * inv;
      const int lo = (int)floorf((c - radius) * inv + 0.5f);
      int hi = (int)floorf((c + radius) * inv - 0.5f);
      if (hi < lo) hi = lo;
      if (hi > lo + 3) hi = lo + 3;
      first[o] = lo;
      std::vector<float>& w = taps[o];
      for (int p = lo; p <= hi; ++p) {
        float v = ita_resize_catmull_rom(centre - ((float)p + 0.5f));
        if (v < small && v > -small) {
          if (w.empty()) {
            first[o] = p + 1;
            continue;
          }
          v = 0.0f;
        }
        w.push_back(v);
      }
      while (!w.empty() && w.back() == 0.0f) w.pop_back();
    }
  }
  // n_out / n_in = num / den in lowest terms: the first num outputs are normalised, the others are copies den pixels on
  int g = n_in, b = n_out;
  while (b) { const int r = g % b; g = b; b = r; }
  const int num = n_out / g, den = n_in / g;
  for (int o = 0; o < num; ++o) {
    std::vector<float>& w = taps[o];
    if (w.empty()) return false;
    double total = 0.0;
    for (float c : w) total += (double)c;
    if (total < (double)small && total > -(double)small) {
      w.assign(1, 0.0f);
    } else if (total != 1.0) {
      const double k = 1.0 / total;
      for (float& c : w) c = (float)((double)c * k);
    }
  }
  for (int o = num; o < n_out; ++o) {
    first[o] = first[o - num] + den;
    taps[o] = taps[o - num];
  }
  t.n0.assign(n_out, 0);
  t.count.assign(n_out, 0);
  t.width = 0;
  for (int o = 0; o < n_out; ++o) {
    std::vector<float>& w = taps[o];
    int n0 = first[o];
    const int n1 = n0 + (int)w.size() - 1;
    if (n1 < 0 || n0 > n_in - 1) return false;
    if (n1 > n_in - 1) {                       // behind the end first, ascending, onto the last pixel
      for (int i = n_in; i <= n1; ++i) w[n_in - 1 - n0] = w[n_in - 1 - n0] + w[i - n0];
      w.resize((size_t)(n_in - n0));
    }
    if (n0 < 0) {                              // then in front, from -1 downwards, onto pixel 0
      for (int i = -1; i > n0; --i) w[-n0] = w[-n0] + w[i - n0];
      const float head = w[0];
      w.erase(w.begin(), w.begin() + (-n0));
      w[0] = w[0] + head;
      n0 = 0;
    }
    while (w.size() > 1 && w.back() == 0.0f) w.pop_back();
    if (n0 < 0 || n0 + (int)w.size() > n_in || w.empty()) return false;
    t.n0[o] = n0;
    t.count[o] = (int)w.size();
    if ((int)w.size() > t.width) t.width = (int)w.size();
  }
  t.coeff.assign((size_t)n_out * t.width, 0.0f);
  for (int o = 0; o < n_out; ++o)
    for (size_t j = 0; j < taps[o].size(); ++j) t.coeff[(size_t)o * t.width + j] = taps[o][j];
  return true;
}

// ---- device ----------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

// Device tables of one source size.  Every index they hold lies inside the source: n0 >= 0, n0 + count <= n_in
// (ita_resize_axis checks it), so the kernel's loads need no clamp of their own.
struct ItaWireTables {
  const int *n0y, *cnty, *n0x, *cntx;
  const float *wy, *wx;      // wy [60][ldy]: a row's weights are wave-uniform scalar loads; wx TRANSPOSED [ldx][90]: tap j
                             // of the 64 outputs a wave computes at once is one coalesced load
  int ldy, ldx;
};

// LDS of the kernel: one W-float row per wave for the vertical pass' result, and with STAGED in front of them the source
// rows of the band, `span` rows of ita_wire_pitch(W) bytes each.  A staged row lies at the offset of its misalignment
// (0..15), so that 16-byte pieces of global memory land on 16-byte LDS addresses.
__host__ __device__ constexpr int ita_wire_pitch(int W) { return (W + 15 + 15) & ~15; }
__host__ __device__ constexpr int ita_wire_lds_bytes(int W, int span) {
  return span * ita_wire_pitch(W) + 4 * W * (int)sizeof(float);
}
constexpr int ITA_WIRE_STAGED_LDS_MAX = 80 * 1024;   // two workgroups per CU

__device__ __forceinline__ float ita_wire_px(unsigned code) {
#pragma clang fp contract(off)
  return (float)code * 3.9215689e-03f;
}

// The band's source rows [first, first + span) of one frame -> LDS, each byte fetched once and nothing outside a row's W
// pixels touched: 16-byte pieces that lie wholly inside the row as aligned 16-byte loads, four in flight per thread; the
// at most two pieces per row that stick out (in front of the first boundary, behind the last) pixel by pixel.
__device__ __forceinline__ void ita_wire_stage(const uint8_t* __restrict__ rows, long long row_stride, int W, int span,
                                               unsigned char* stage, int pitch) {
  const int npr = pitch >> 4, total = span * npr;
  for (int base = 0; base < total; base += 4 * 256) {
    uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0, v2 = v0, v3 = v0;
    int d0 = -1, d1 = -1, d2 = -1, d3 = -1;       // LDS offset of the piece, -1: not a whole piece of a row
#define ITA_WIRE_PIECE_LOAD(u, v, d)                                                  \
    {                                                                                 \
      const int idx = base + (u) * 256 + (int)threadIdx.x;                            \
      if (idx < total) {                                                              \
        const int r = idx / npr, k = idx - r * npr;                                   \
        const uint8_t* row = rows + r * row_stride;                                   \
        const int lo = k * 16 - (int)((unsigned long long)row & 15);                  \
        if (lo >= 0 && lo + 16 <= W) {                                                \
          v = *reinterpret_cast<const uint4*>(row + lo);                              \
          d = r * pitch + k * 16;                                                     \
        }                                                                             \
      }                                                                               \
    }
    ITA_WIRE_PIECE_LOAD(0, v0, d0)
    ITA_WIRE_PIECE_LOAD(1, v1, d1)
    ITA_WIRE_PIECE_LOAD(2, v2, d2)
    ITA_WIRE_PIECE_LOAD(3, v3, d3)
#undef ITA_WIRE_PIECE_LOAD
    if (d0 >= 0) *reinterpret_cast<uint4*>(stage + d0) = v0;
    if (d1 >= 0) *reinterpret_cast<uint4*>(stage + d1) = v1;
    if (d2 >= 0) *reinterpret_cast<uint4*>(stage + d2) = v2;
    if (d3 >= 0) *reinterpret_cast<uint4*>(stage + d3) = v3;
  }
  for (int idx = threadIdx.x; idx < 2 * span; idx += 256) {
    const int r = idx >> 1;
    const uint8_t* row = rows + r * row_stride;
    const int mis = (int)((unsigned long long)row & 15);
    const int klast = (mis + W - 1) >> 4;
    if ((idx & 1) && klast == 0) continue;          // one piece holds the whole row: done as its first
    const int k = (idx & 1) ? klast : 0;
    const int lo = k * 16 - mis;
    if (lo >= 0 && lo + 16 <= W) continue;          // a whole piece: done above
    unsigned char* d = stage + r * pitch + mis;     // pixel b of the row
    const int b1 = lo + 16 < W ? lo + 16 : W;
    for (int b = lo > 0 ? lo : 0; b < b1; ++b) d[b] = row[b];
  }
}

// grid: any number of workgroups <= batch * ceil(60 / ROWS) (each strides over the (frame, band of ROWS output rows)
// items); 256 threads, wave w takes the band's rows w, w + 4, ...; ROWS a multiple of 4; dynamic LDS
// ita_wire_lds_bytes(W, STAGED ? span : 0).  Strides in pixels = bytes.
//   DWORDS  row_stride % 4 == 0 (every row of a frame then has the misalignment of its first one modulo 4): columns are
//           read as aligned dwords.  Without it, pixel by pixel.
//   STAGED  the band's source rows are first copied to LDS (ita_wire_stage) and the vertical pass reads them there: a
//           source byte comes from memory once per band, not once per output row it feeds.  span = the largest number of
//           source rows any band needs (the host takes it from the table).  Needs DWORDS.
template <bool DWORDS, bool STAGED>
__global__ __launch_bounds__(256) void ita_ingest_wire_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                              long long row_stride, long long frame_stride,
                                                              ItaWireTables t, uint8_t* __restrict__ out, int batch,
                                                              int ROWS, int span) {
#pragma clang fp contract(off)
  static_assert(DWORDS || !STAGED, "the staged rows are read as dwords");
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int pitch = ita_wire_pitch(W);
  unsigned char* stage = reinterpret_cast<unsigned char*>(lds);
  float* trow = reinterpret_cast<float*>(lds + (STAGED ? span * pitch : 0)) + wave * W;
  const int bands = (ITA_WIRE_H + ROWS - 1) / ROWS;
  const long long items = (long long)batch * bands;
  // every wave of the workgroup runs the same number of iterations of both loops (ROWS and 60 are multiples of 4): the
  // barriers are workgroup-uniform
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long frame = it / bands;
    const int oy0 = (int)(it % bands) * ROWS;
    const int nrows = ITA_WIRE_H - oy0 < ROWS ? ITA_WIRE_H - oy0 : ROWS;
    const uint8_t* f = src + frame * frame_stride;
    int first = 0;
    if (STAGED) {
      int end = 0;
      first = H;
      for (int r = 0; r < nrows; ++r) {
        const int a = t.n0y[oy0 + r], b = a + t.cnty[oy0 + r];
        first = a < first ? a : first;
        end = b > end ? b : end;
      }
      ita_wire_stage(f + (long long)first * row_stride, row_stride, W, end - first, stage, pitch);   // end - first <= span
      __syncthreads();
    }
    for (int r = wave; r < nrows; r += 4) {
      const int oy = oy0 + r;
      const int cnt = t.cnty[oy];
      const float* __restrict__ wy = t.wy + oy * t.ldy;
      const uint8_t* g0 = f + (long long)t.n0y[oy] * row_stride;   // rows g0 .. g0 + cnt - 1 < H
      // STAGED: row n0y + i lies in LDS at stage + (n0y - first + i) * pitch + (its global address & 15)
      const uint8_t* r0 = g0;
      const long long rs = row_stride;
      const int srow = STAGED ? t.n0y[oy] - first : 0;
      // ---- vertical: trow[x] = sum_i wy[i] * px(row n0y + i, x), i ascending from 0.0f
      int xs = 0, xstep = 64, xend = W;          // the columns done pixel by pixel: all of them without DWORDS
      if (DWORDS) {
        const int to_boundary = (4 - (int)((unsigned long long)g0 & 3)) & 3;
        const int head = to_boundary < W ? to_boundary : W;
        const int nbody = (W - head) >> 2;       // aligned dwords [head + 4 k, head + 4 k + 4), k < nbody: inside [0, W)
        for (int k = lane; k < nbody; k += 64) {
          float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 4
          for (int i = 0; i < cnt; ++i) {
            unsigned v;
            if (STAGED) {
              const int mis = (int)((unsigned long long)(g0 + i * row_stride) & 15);
              v = *reinterpret_cast<const unsigned*>(stage + (srow + i) * pitch + mis + head + 4 * k);
            } else {
              v = *reinterpret_cast<const unsigned*>(r0 + i * rs + head + 4 * k);
            }
            const float w = wy[i];
            a0 = a0 + w * ita_wire_px(v & 255u);
            a1 = a1 + w * ita_wire_px((v >> 8) & 255u);
            a2 = a2 + w * ita_wire_px((v >> 16) & 255u);
            a3 = a3 + w * ita_wire_px(v >> 24);
          }
          float* d = trow + head + 4 * k;
          d[0] = a0; d[1] = a1; d[2] = a2; d[3] = a3;
        }
        // what is left: `head` pixels in front and W - head - 4 nbody < 4 behind, one lane each
        const int tail0 = head + 4 * nbody, left = head + (W - tail0);
        xs = lane < head ? lane : tail0 + (lane - head);
        xstep = W;                               // one pass
        xend = lane < left ? W : 0;
      } else {
        xs = lane;
      }
      for (int x = xs; x < xend; x += xstep) {
        float a = 0.0f;
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
          unsigned c;
          if (STAGED) {
            const int mis = (int)((unsigned long long)(g0 + i * row_stride) & 15);
            c = stage[(srow + i) * pitch + mis + x];
          } else {
            c = r0[i * rs + x];
          }
          a = a + wy[i] * ita_wire_px(c);
        }
        trow[x] = a;
      }
      __syncthreads();
      // ---- horizontal from LDS, then the code
      // Every lane runs all ldx taps of the zero-padded table, behind its own count with weight 0.0f on a clamped index:
      // y + 0.0f * s is y, so the sum is the definition's, and the loop, now of one length for all lanes, unrolls with
      // its loads in flight together.  (With a per-lane count it ran load by load, each a cache latency: 5 x the time.)
      for (int ox = lane; ox < ITA_WIRE_W; ox += 64) {
        const float* __restrict__ wx = t.wx + ox;
        const int x0 = t.n0x[ox];
        float y = 0.0f;
#pragma unroll 8
        for (int j = 0; j < t.ldx; ++j) {
          const int x = x0 + j < W - 1 ? x0 + j : W - 1;
          y = y + wx[j * ITA_WIRE_W] * trow[x];
        }
        float v = y * 255.0f + 0.5f;
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        out[(frame * ITA_WIRE_H + oy) * ITA_WIRE_W + ox] = (uint8_t)(int)v;
      }
      __syncthreads();     // trow is overwritten by the wave's next row, the staged rows by the next item
    }
  }
}
#endif  // __HIPCC__
