// What a kernel's output stores leave for the next kernel's boundary: a hipGraph chain of
// (producer -> trivial dependent consumer) pairs, 256 workgroups x 8 waves each.  The producer
// writes B bytes with the conv epilogue's address pattern (NHWC, 32 16-bit channels = 64 bytes per
// pixel, lane = (pixel = lane & 15, channel group = lane >> 4), one 16-pixel fragment per wave and
// step) in one of four store flavours:
//   plain 8 B per lane          two stores per fragment (channels 16 fc + 4 g .. + 3), today's epilogue
//   plain 16 B per lane         one store per fragment (channels 8 g .. 8 g + 7)
//   write-through 8 B per lane  the same addresses, relaxed agent-scope atomic stores (sc1)
//   write-through 16 B per lane raw buffer stores with the sc1 cache bit
// Every block stamps s_memrealtime (100 MHz) at entry and exit.  Reported per flavour and size:
// producer span (first entry -> last exit), boundary gap (last producer exit -> first consumer
// entry), consumer -> next producer gap, and the wall time of a pair under graph replay.
//   hipcc -O3 --offload-arch=gfx950 tools/mb_boundary.hip -o tools/_mb_boundary && ./tools/_mb_boundary
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned long long gu64;

constexpr int G = 256, NT = 512, NWV = NT / 64;

__device__ unsigned long long* g_st;   // [launch][block][2], not a kernel argument

__device__ __forceinline__ unsigned long long rt() { return __builtin_amdgcn_s_memrealtime(); }

// FL: 0 plain 8 B, 1 plain 16 B, 2 write-through 8 B, 3 write-through 16 B
template <int FL>
__global__ __launch_bounds__(NT) void producer(char* __restrict__ out, int frags_per_block, unsigned seed, int launch) {
  const unsigned long long t0 = rt();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = lane & 15, g = lane >> 4;
  const unsigned blk0 = (unsigned)blockIdx.x * frags_per_block;            // fragments of 1024 bytes
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((unsigned)G * frags_per_block * 1024u), 0x00020000);
  for (int f = wave; f < frags_per_block; f += NWV) {
    const unsigned base = (blk0 + f) * 1024u + px * 64u;
    const unsigned v = seed + base + g;                                    // any lane-dependent payload
    if constexpr (FL == 0) {
      *(u32x2*)(out + base + g * 8) = u32x2{v, v + 1};
      *(u32x2*)(out + base + 32 + g * 8) = u32x2{v + 2, v + 3};
    } else if constexpr (FL == 1) {
      *(u32x4*)(out + base + g * 16) = u32x4{v, v + 1, v + 2, v + 3};
    } else if constexpr (FL == 2) {
      __hip_atomic_store((gu64*)(out + base + g * 8), ((unsigned long long)(v + 1) << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store((gu64*)(out + base + 32 + g * 8), ((unsigned long long)(v + 3) << 32) | (v + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      __builtin_amdgcn_raw_buffer_store_b128(u32x4{v, v + 1, v + 2, v + 3}, rs, (int)(base + g * 16), 0, 16);
    }
  }
  if (threadIdx.x == 0) {
    unsigned long long* s = g_st + ((size_t)launch * G + blockIdx.x) * 2;
    s[0] = t0; s[1] = rt();
  }
}

// reads one word of the producer's output per thread (spread over the whole buffer), writes it on
__global__ __launch_bounds__(NT) void consumer(const unsigned* __restrict__ in, unsigned* __restrict__ sink, unsigned words, int launch) {
  const unsigned long long t0 = rt();
  const unsigned i = blockIdx.x * NT + threadIdx.x;
  sink[i] = in[(unsigned)(((unsigned long long)i * words) / (G * NT))] + 1u;
  if (threadIdx.x == 0) {
    unsigned long long* s = g_st + ((size_t)launch * G + blockIdx.x) * 2;
    s[0] = t0; s[1] = rt();
  }
}

template <int FL>
static void launch_producer(hipStream_t s, char* out, int fpb, unsigned seed, int launch) {
  hipLaunchKernelGGL(producer<FL>, dim3(G), dim3(NT), 0, s, out, fpb, seed, launch);
}

int main() {
  const int PAIRS = 12, L = 2 * PAIRS, REPS = 30;
  const size_t MAXB = 34u << 20;
  char* buf;
  unsigned* sink;
  CK(hipMalloc(&buf, MAXB)); CK(hipMalloc(&sink, G * NT * 4));
  CK(hipMemset(buf, 0, MAXB)); CK(hipMemset(sink, 0, G * NT * 4));
  unsigned long long* st;
  CK(hipMalloc(&st, sizeof(unsigned long long) * L * G * 2));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_st), &st, sizeof(st)));
  hipStream_t s;
  CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  const char* names[4] = {"plain 8 B", "plain 16 B", "write-through 8 B", "write-through 16 B"};
  const int mbs[4] = {2, 8, 17, 34};
  printf("%-20s %6s | %14s %14s %14s %14s | %10s\n", "flavour", "MB", "producer span", "boundary gap", "cons->prod gap",
         "span + gap", "pair wall");
  for (int mi = 0; mi < 4; ++mi) {
    const int fpb = (int)(((size_t)mbs[mi] << 20) / 1024 / G);             // whole fragments per block
    const unsigned words = (unsigned)((size_t)G * fpb * 1024 / 4);
    for (int fl = 0; fl < 4; ++fl) {
      hipGraph_t g;
      hipGraphExec_t ge;
      CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      for (int p = 0; p < PAIRS; ++p) {
        const unsigned seed = 17u * p + fl;
        switch (fl) {
          case 0: launch_producer<0>(s, buf, fpb, seed, 2 * p); break;
          case 1: launch_producer<1>(s, buf, fpb, seed, 2 * p); break;
          case 2: launch_producer<2>(s, buf, fpb, seed, 2 * p); break;
          default: launch_producer<3>(s, buf, fpb, seed, 2 * p); break;
        }
        hipLaunchKernelGGL(consumer, dim3(G), dim3(NT), 0, s, (const unsigned*)buf, sink, words, 2 * p + 1);
      }
      CK(hipStreamEndCapture(s, &g));
      CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
      for (int r = 0; r < 5; ++r) CK(hipGraphLaunch(ge, s));
      CK(hipStreamSynchronize(s));
      std::vector<unsigned long long> h((size_t)L * G * 2);
      CK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
      auto first = [&](int l) { unsigned long long m = ~0ull; for (int b = 0; b < G; ++b) m = std::min(m, h[((size_t)l * G + b) * 2]); return m; };
      auto last = [&](int l) { unsigned long long m = 0; for (int b = 0; b < G; ++b) m = std::max(m, h[((size_t)l * G + b) * 2 + 1]); return m; };
      double span = 0, gap = 0, gap2 = 0;
      int n = 0, n2 = 0;
      for (int p = 1; p < PAIRS; ++p) {                                    // pair 0 starts cold
        span += (double)(last(2 * p) - first(2 * p));
        gap += (double)first(2 * p + 1) - (double)last(2 * p);
        ++n;
        if (p + 1 < PAIRS) { gap2 += (double)first(2 * p + 2) - (double)last(2 * p + 1); ++n2; }
      }
      hipEvent_t e0, e1;
      CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
      CK(hipEventRecord(e0, s));
      for (int r = 0; r < REPS; ++r) CK(hipGraphLaunch(ge, s));
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      // check: the last producer's payload landed (first and last word of the buffer)
      unsigned w0 = 0, w1 = 0;
      CK(hipMemcpy(&w0, buf, 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(&w1, buf + (size_t)words * 4 - 4, 4, hipMemcpyDeviceToHost));
      const unsigned seedl = 17u * (PAIRS - 1) + fl, basel = (unsigned)((size_t)words * 4 - 64);
      const bool ok = w0 == seedl && w1 == seedl + basel + 3 + 3;
      printf("%-20s %6d | %11.2f us %11.2f us %11.2f us %11.2f us | %7.2f us%s\n", names[fl], mbs[mi], span / n * 1e-2,
             gap / n * 1e-2, gap2 / n2 * 1e-2, (span + gap) / n * 1e-2, ms * 1e3 / (REPS * PAIRS), ok ? "" : "  PAYLOAD MISMATCH");
      CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
      CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
    }
  }
  printf("MB_OK\n");
  return 0;
}
