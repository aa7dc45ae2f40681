// Cost of the LSTM head's in-launch meetings (ita_lstm_head_kernel, csrc/ita_lstm_head_kernel.h) against the same phases as separate launches, on the
// head's geometry: 256-thread workgroups in groups of 16 consecutive ids, 4 and 32 groups (128 and 1024 frames).  Per
// workgroup and edge a 1 KB payload stored write-through (sc1), then every member reads its group's 16 KB with sc1 loads.
// Meeting = every wave s_waitcnt vmcnt(0) (asm) -> barrier -> one lane's relaxed agent-scope atomic add -> one lane polls
// relaxed (sc1) loads with s_sleep -> barrier.  No release / acquire fence.  Counters one per 256 bytes, reset in-kernel by
// the group's last arriver.  Launch forms:
//   one launch, M meetings (M = 0, 1, 2; with M = 2 the last arriver of the final publish reads the group's 16 KB: fan-in)
//   four launches: publish | read + publish | read + publish | fan-in read (one workgroup per group)
// hipcc --offload-arch=gfx950 -O3 -o /tmp/head_meet tools/microbench/head_meet.hip && /tmp/head_meet
#include <hip/hip_runtime.h>
#include <cstdio>
#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int STRIDE = 64;   // counter words per 256-byte block

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, 0x7FFFFFFF, 0x00020000);
}
// 1 KB per workgroup: wave 0, 16 bytes per lane
__device__ __forceinline__ void publish(unsigned* buf, int G, int edge, int grp, int m, unsigned v) {
  if (threadIdx.x < 64) {
    const u32x4 x = {v, v + 1, v + 2, v + 3};
    const int off = (((edge * G + grp) * 16 + m) * 256 + threadIdx.x * 4) * 4;
    __builtin_amdgcn_raw_buffer_store_b128(x, rsrc(buf), off, 0, 16);
  }
}
// the group's 16 KB: 256 threads x 4 x 16 bytes, sc1 loads
__device__ __forceinline__ unsigned read_group(const unsigned* buf, int G, int edge, int grp) {
  unsigned acc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int off = ((edge * G + grp) * 16 * 256 + (i * 256 + threadIdx.x) * 4) * 4;
    const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rsrc(buf), off, 0, 16);
    acc += x.x ^ x.y ^ x.z ^ x.w;
  }
  return acc;
}
__device__ __forceinline__ bool poll(unsigned* cnt, unsigned target, unsigned* err) {
  const unsigned long long t0 = wall_clock64();
  while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    if (wall_clock64() - t0 > 100000000ull) { __hip_atomic_fetch_add(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return false; }
    __builtin_amdgcn_s_sleep(2);
  }
  return true;
}

__global__ __launch_bounds__(256, 2) void one_launch(unsigned* buf, unsigned* cnt, unsigned* err, unsigned* sink, int meetings) {
  __shared__ unsigned flag;
  const int G = gridDim.x / 16, grp = blockIdx.x >> 4, m = blockIdx.x & 15, tid = threadIdx.x;
  unsigned* c = cnt + grp * STRIDE;
  unsigned acc = 0;
  for (int e = 0; e <= meetings; ++e) {
    publish(buf, G, e, grp, m, acc + e);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const unsigned prev = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      flag = prev == 16u * (meetings + 1) - 1;   // last arriver of the final edge
    }
    if (e == meetings) break;
    if (tid == 0) flag = poll(c, 16u * (e + 1), err) ? 1u : 0u;
    __syncthreads();
    if (!flag) return;
    acc += read_group(buf, G, e, grp);
  }
  __syncthreads();
  if (!flag) return;
  if (tid == 0) __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (meetings == 2) acc += read_group(buf, G, meetings, grp);
  if (acc == 0x12345u) sink[0] = acc;
}
__global__ __launch_bounds__(256) void phase_launch(unsigned* buf, unsigned* sink, int edge) {
  const int G = gridDim.x / 16, grp = blockIdx.x >> 4, m = blockIdx.x & 15;
  unsigned acc = edge > 0 ? read_group(buf, G, edge - 1, grp) : 0u;
  publish(buf, G, edge, grp, m, acc + edge);
  if (acc == 0x12345u) sink[0] = acc;
}
__global__ __launch_bounds__(256) void fanin_launch(unsigned* buf, unsigned* sink, int edge) {
  const unsigned acc = read_group(buf, gridDim.x, edge, blockIdx.x);   // one workgroup per group: gridDim.x = groups
  if (acc == 0x12345u) sink[0] = acc;
}

int main() {
  const int IT = 500;
  unsigned *buf, *cnt, *err, *sink;
  CHK(hipMalloc(&buf, sizeof(unsigned) * 3 * 32 * 16 * 256));
  CHK(hipMalloc(&cnt, sizeof(unsigned) * 32 * STRIDE)); CHK(hipMalloc(&err, 4)); CHK(hipMalloc(&sink, 4));
  CHK(hipMemset(cnt, 0, sizeof(unsigned) * 32 * STRIDE)); CHK(hipMemset(err, 0, 4));
  hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  hipStream_t s; CHK(hipStreamCreate(&s));
  for (int G : {4, 32}) {
    for (int meetings : {0, 1, 2}) {
      for (int rep = 0; rep < 2; ++rep) {   // the first pass warms up
        CHK(hipEventRecord(e0, s));
        for (int it = 0; it < IT; ++it) hipLaunchKernelGGL(one_launch, dim3(16 * G), dim3(256), 0, s, buf, cnt, err, sink, meetings);
        CHK(hipEventRecord(e1, s)); CHK(hipEventSynchronize(e1));
      }
      float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
      unsigned herr; CHK(hipMemcpy(&herr, err, 4, hipMemcpyDeviceToHost));
      printf("%2d groups (%4d frames) one launch, %d meeting(s)%s: %6.2f us   (timeouts %u)\n", G, 32 * G, meetings,
             meetings == 2 ? " + fan-in" : "          ", ms * 1000 / IT, herr);
      if (herr) return 1;
    }
    for (int rep = 0; rep < 2; ++rep) {
      CHK(hipEventRecord(e0, s));
      for (int it = 0; it < IT; ++it) {
        for (int e = 0; e < 3; ++e) hipLaunchKernelGGL(phase_launch, dim3(16 * G), dim3(256), 0, s, buf, sink, e);
        hipLaunchKernelGGL(fanin_launch, dim3(G), dim3(256), 0, s, buf, sink, 2);
      }
      CHK(hipEventRecord(e1, s)); CHK(hipEventSynchronize(e1));
    }
    float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
    printf("%2d groups (%4d frames) four launches (3 phases + fan-in)   : %6.2f us\n", G, 32 * G, ms * 1000 / IT);
  }
  return 0;
}
