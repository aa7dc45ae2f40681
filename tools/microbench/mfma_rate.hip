// What a CU's f16 MFMA pipe delivers in wall-clock time (not cycles): bursts of the length of the folded GEMM and long runs.
// Part 1 (mfma_loop): one workgroup per CU, WAVES waves of 64 lanes, each wave a loop of `iters` x 8 v_mfma_f32_32x32x16_f16 on
// two accumulators, operands in registers.
// Part 2 (tile_loop): the folded GEMM's own MFMA phase in both MFMA shapes -- eight waves per workgroup (two per SIMD), each wave a
// 64 x 32 output tile, three split-precision products per k-step, random hi / lo operands -- as v_mfma_f32_32x32x16_f16
// (activations as A) and as v_mfma_f32_16x16x32_f16 (weights as A), with the fragments held in registers and with every fragment
// re-read from the GEMM's swizzled LDS image by ds_read_b128 (one barrier per 64-deep k-tile, as in the GEMM).  Arms alternate;
// wall time per arm from events, wave cycles and the in-kernel clock (delta s_memtime / delta s_memrealtime x 100 MHz) from the
// STAMP instantiations, whose stamps go to a buffer of their own.
// hipcc --offload-arch=gfx950 -O3 -o mfma_rate mfma_rate.hip && ./mfma_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(512) void mfma_loop(float* out, int iters, long long* clk) {
  f16x8 a, b;
  for (int j = 0; j < 8; ++j) { a[j] = (_Float16)(0.001f * (threadIdx.x + j)); b[j] = (_Float16)(0.002f * (threadIdx.x - j)); }
  f32x16 c0, c1;
  for (int e = 0; e < 16; ++e) { c0[e] = 0.0f; c1[e] = 0.0f; }
  const long long t0 = clock64();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(b, a, c1, 0, 0, 0);
    }
  }
  const long long t1 = clock64();
  float s = 0.0f;
  for (int e = 0; e < 16; ++e) s += c0[e] + c1[e];
  if (s == 123.456f) out[0] = s;
  if (blockIdx.x == 0 && threadIdx.x == 0) clk[0] = t1 - t0;
}

// ---- part 2.  Operand planes as the GEMM stages them: x hi | x lo | w hi | w lo, each 128 rows x 64 k (128-byte rows, the eight
// 16-byte chunks of a row XOR-swizzled with (row >> 1) & 7).  `rnd` holds the four planes, 64 KB.
constexpr int PLANE = 128 * 128;
__device__ __forceinline__ f16x8 frag(const char* plane, int r, int chunk) {
  return *(const f16x8*)(plane + r * 128 + ((chunk ^ ((r >> 1) & 7)) << 4));
}

template <int SHAPE, bool FROM_LDS, bool STAMP>
__global__ __launch_bounds__(512) void tile_loop(const char* __restrict__ rnd, float* out, int ktiles, unsigned long long* stamps) {
  __shared__ __attribute__((aligned(16))) char lds[4 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 2, wn = wave & 3;
  const char* src = rnd;
  if (FROM_LDS) {
    for (int p = tid; p < 4 * PLANE / 16; p += 512) *(f16x8*)(lds + p * 16) = *(const f16x8*)(rnd + p * 16);
    __syncthreads();
    src = lds;
  }
  const char *xh = src, *xl = src + PLANE, *wh = src + 2 * PLANE, *wl = src + 3 * PLANE;
  float s = 0.0f;
  unsigned long long t0 = 0, r0 = 0, t1 = 0, r1 = 0;
  if (SHAPE == 32) {
    // wave tile = 2 x 1 MFMA tiles of 32 x 32; a k-tile = 4 k-steps of 16 = 24 MFMAs
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[2];
    for (int i = 0; i < 2; ++i)
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
    f16x8 fah[4][2], fal[4][2], fwh[4], fwl[4];
    auto load = [&](int ks) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fah[ks][i] = frag(xh, wm * 64 + i * 32 + r, 2 * ks + h);
        fal[ks][i] = frag(xl, wm * 64 + i * 32 + r, 2 * ks + h);
      }
      fwh[ks] = frag(wh, wn * 32 + r, 2 * ks + h);
      fwl[ks] = frag(wl, wn * 32 + r, 2 * ks + h);
    };
    if (!FROM_LDS)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) load(ks);
    if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    for (int t = 0; t < ktiles; ++t) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (FROM_LDS) load(ks);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fal[ks][i], fwh[ks], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[ks][i], fwl[ks], acc[i], 0, 0, 0);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah[ks][i], fwh[ks], acc[i], 0, 0, 0);
        }
      }
      if (FROM_LDS) __syncthreads();
    }
    if (STAMP) { t1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime(); }
    for (int i = 0; i < 2; ++i)
      for (int e = 0; e < 16; ++e) s += acc[i][e];
  } else {
    // wave tile = 2 (n) x 4 (m) MFMA tiles of 16 x 16, weights as A; a k-tile = 2 k-steps of 32 = 48 MFMAs
    const int r = lane & 15, q = lane >> 4;
    f32x4 acc[4][2];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    f16x8 fxh[2][4], fxl[2][4], fwh[2][2], fwl[2][2];
    auto load = [&](int ks) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        fwh[ks][j] = frag(wh, wn * 32 + j * 16 + r, 4 * ks + q);
        fwl[ks][j] = frag(wl, wn * 32 + j * 16 + r, 4 * ks + q);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fxh[ks][i] = frag(xh, wm * 64 + i * 16 + r, 4 * ks + q);
        fxl[ks][i] = frag(xl, wm * 64 + i * 16 + r, 4 * ks + q);
      }
    };
    if (!FROM_LDS)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) load(ks);
    if (STAMP) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
    for (int t = 0; t < ktiles; ++t) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (FROM_LDS) load(ks);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[ks][j], fxl[ks][i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwl[ks][j], fxh[ks][i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fwh[ks][j], fxh[ks][i], acc[i][j], 0, 0, 0);
          }
      }
      if (FROM_LDS) __syncthreads();
    }
    if (STAMP) { t1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime(); }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 2; ++j)
        for (int e = 0; e < 4; ++e) s += acc[i][j][e];
  }
  if (s == 123.456f) out[0] = s;
  if (STAMP && lane == 0) {
    unsigned long long* st = stamps + ((size_t)blockIdx.x * 8 + wave) * 2;
    st[0] = t1 - t0; st[1] = r1 - r0;
  }
}

struct Arm { const char* name; void (*plain)(const char*, float*, int, unsigned long long*); void (*stamp)(const char*, float*, int, unsigned long long*); };

int main() {
  hipDeviceProp_t p;
  hipGetDeviceProperties(&p, 0);
  const int cus = p.multiProcessorCount;
  float* out; long long* clk;
  hipMalloc(&out, 4); hipMalloc(&clk, 8);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int waves : {4, 8}) {
    for (int iters : {48, 480, 48000}) {   // 48 x 8 = 384 MFMAs per wave = the folded GEMM's count per wave (16 k-tiles x 24)
      for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(mfma_loop, dim3(cus), dim3(64 * waves), 0, 0, out, iters, clk);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        long long c; hipMemcpy(&c, clk, 8, hipMemcpyDeviceToHost);
        const double flop = 2.0 * 32 * 32 * 16 * 8.0 * iters * waves * cus;
        printf("waves/CU %d  iters %6d  %9.3f us  %7.1f TFLOP/s   clock64 delta %lld (%.1f per MFMA per wave)\n", waves, iters,
               ms * 1e3, flop / (ms * 1e-3) / 1e12, c, (double)c / (8.0 * iters));
      }
    }
  }

  // ---- part 2: random split-precision operands, x = hi + lo
  std::vector<_Float16> h(4 * PLANE / 2);
  srand(1);
  for (int pl = 0; pl < 2; ++pl)
    for (int i = 0; i < PLANE / 2; ++i) {
      const float x = 2.0f * (float)rand() / (float)RAND_MAX - 1.0f;
      const _Float16 hi = (_Float16)x, lo = (_Float16)(x - (float)hi);
      h[(2 * pl) * (PLANE / 2) + i] = hi;
      h[(2 * pl + 1) * (PLANE / 2) + i] = lo;
    }
  char* rnd; unsigned long long* stamps;
  hipMalloc(&rnd, 4 * PLANE);
  hipMalloc(&stamps, (size_t)cus * 8 * 2 * 8);
  hipMemcpy(rnd, h.data(), 4 * PLANE, hipMemcpyHostToDevice);
  const Arm arms[4] = {
      {"32x32x16 registers", tile_loop<32, false, false>, tile_loop<32, false, true>},
      {"16x16x32 registers", tile_loop<16, false, false>, tile_loop<16, false, true>},
      {"32x32x16 LDS b128 ", tile_loop<32, true, false>, tile_loop<32, true, true>},
      {"16x16x32 LDS b128 ", tile_loop<16, true, false>, tile_loop<16, true, true>},
  };
  // >= 2 s of back-to-back launches on random data before anything is timed
  for (int i = 0; i < 40; ++i)
    for (const Arm& a : arms) hipLaunchKernelGGL(a.plain, dim3(cus), dim3(512), 0, 0, rnd, out, 16000, stamps);
  hipDeviceSynchronize();
  constexpr int REPS = 7;
  std::vector<unsigned long long> st((size_t)cus * 8 * 2);
  for (int ktiles : {16, 16000}) {         // 16 k-tiles = one K slice of the folded GEMM; 16000 = a long run
    const int batch = ktiles == 16 ? 200 : 1;   // short form: launches back to back, time per launch
    double wall[4][REPS], cyc[4][REPS], ghz[4][REPS];
    for (int rep = 0; rep < REPS; ++rep)
      for (int a = 0; a < 4; ++a) {
        hipEventRecord(e0);
        for (int b = 0; b < batch; ++b) hipLaunchKernelGGL(arms[a].plain, dim3(cus), dim3(512), 0, 0, rnd, out, ktiles, stamps);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        wall[a][rep] = ms * 1e3 / batch;
        for (int b = 0; b < batch; ++b) hipLaunchKernelGGL(arms[a].stamp, dim3(cus), dim3(512), 0, 0, rnd, out, ktiles, stamps);
        hipMemcpy(st.data(), stamps, st.size() * 8, hipMemcpyDeviceToHost);
        std::vector<double> c, g;
        for (size_t w = 0; w < st.size() / 2; ++w) {
          c.push_back((double)st[2 * w]);
          g.push_back(st[2 * w + 1] ? (double)st[2 * w] / (double)st[2 * w + 1] * 0.1 : 0.0);
        }
        std::sort(c.begin(), c.end()); std::sort(g.begin(), g.end());
        cyc[a][rep] = c[c.size() / 2]; ghz[a][rep] = g[g.size() / 2];
      }
    printf("\nk-tiles %d per wave (%d launches per timing), %d alternating repetitions, %d CUs x 8 waves, wave tile 64 x 32, 3 products\n",
           ktiles, batch, REPS, cus);
    printf("%-20s %30s %34s %24s\n", "arm", "wall us/launch min med max", "wave cycles (median wave) min med max", "in-kernel GHz min med max");
    double med[4];
    for (int a = 0; a < 4; ++a) {
      std::sort(wall[a], wall[a] + REPS); std::sort(cyc[a], cyc[a] + REPS); std::sort(ghz[a], ghz[a] + REPS);
      med[a] = wall[a][REPS / 2];
      printf("%-20s %9.2f %9.2f %9.2f   %11.0f %11.0f %11.0f   %7.3f %7.3f %7.3f\n", arms[a].name, wall[a][0], wall[a][REPS / 2],
             wall[a][REPS - 1], cyc[a][0], cyc[a][REPS / 2], cyc[a][REPS - 1], ghz[a][0], ghz[a][REPS / 2], ghz[a][REPS - 1]);
    }
    printf("wall ratio 32x32x16 / 16x16x32 (medians): registers %.3f   LDS %.3f\n", med[0] / med[1], med[2] / med[3]);
  }
  return 0;
}
