// Stand-alone timing of four ways to count 16-bit values into 65536 64-bit bins (the design choice behind drs_hist_u16,
// csrc/radiometry.hip), on three distributions: uniform over 0 .. 65535, scene-like (a gamma law: a few
// hundred values carry the band) and one constant value.
//   global        every pixel one 64-bit global atomic
//   global+wave   the same, but a wave whose lanes agree adds their number once
//   lds16         65536 16-bit bins in 128 KB of LDS, every pixel one LDS atomic, non-zero bins flushed every 65280 pixels
//   lds16+wave    lds16 with the wave-uniform add (the shipped form)
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/micro/hist_u16_variants.hip -o hist_u16_variants ; run: ./hist_u16_variants [Mpixels]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));                         \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

constexpr int kWords = 32768;
constexpr long long kChunk = 65280;

template <bool WAVE>
__device__ __forceinline__ void add_global(unsigned long long* counts, unsigned v) {
  if (WAVE) {
    const unsigned long long act = __ballot(1);
    const unsigned first = __builtin_amdgcn_readfirstlane(v);
    if (__ballot(v == first) == act) {
      if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(counts + first, (unsigned long long)__popcll(act));
      return;
    }
  }
  atomicAdd(counts + v, 1ull);
}

template <bool WAVE>
__device__ __forceinline__ void add_lds(unsigned* bins, unsigned v) {
  if (WAVE) {
    const unsigned long long act = __ballot(1);
    const unsigned first = __builtin_amdgcn_readfirstlane(v);
    if (__ballot(v == first) == act) {
      if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(&bins[first >> 1], (unsigned)__popcll(act) << (16 * (first & 1)));
      return;
    }
  }
  atomicAdd(&bins[v >> 1], 1u << (16 * (v & 1)));
}

template <bool WAVE>
__global__ __launch_bounds__(256) void hist_global(const unsigned short* __restrict__ v, long long n, unsigned long long* counts) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n / 8; g += (long long)gridDim.x * 256) {
    const uint4 q = *reinterpret_cast<const uint4*>(v + 8 * g);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) add_global<WAVE>(counts, (w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
  }
}

template <bool WAVE>
__global__ __launch_bounds__(1024) void hist_lds(const unsigned short* __restrict__ v, long long n, unsigned long long* counts) {
  extern __shared__ unsigned bins[];
  for (int w = threadIdx.x; w < kWords; w += 1024) bins[w] = 0u;
  __syncthreads();
  const long long chunks = (n + kChunk - 1) / kChunk;
  for (long long item = blockIdx.x; item < chunks; item += gridDim.x) {
    const long long p0 = item * kChunk, p1 = p0 + kChunk < n ? p0 + kChunk : n;
    for (long long g = threadIdx.x; g < (p1 - p0) / 8; g += 1024) {
      const uint4 q = *reinterpret_cast<const uint4*>(v + p0 + 8 * g);
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 8; ++k) add_lds<WAVE>(bins, (w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < kWords; w += 1024) {
      const unsigned two = bins[w];
      if (two) {
        bins[w] = 0u;
        if (two & 0xffffu) atomicAdd(counts + 2 * w, (unsigned long long)(two & 0xffffu));
        if (two >> 16) atomicAdd(counts + 2 * w + 1, (unsigned long long)(two >> 16));
      }
    }
    __syncthreads();
  }
}

int main(int argc, char** argv) {
  const long long n = (argc > 1 ? std::atoll(argv[1]) : 54) * 1000000ll / kChunk * kChunk;  // whole chunks, a multiple of 8
  int cus = 0;
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(hist_lds<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kWords * 4));
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(hist_lds<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kWords * 4));
  unsigned short* d = nullptr;
  unsigned long long* counts = nullptr;
  CHECK(hipMalloc(&d, n * 2));
  CHECK(hipMalloc(&counts, 65536 * 8));
  std::vector<unsigned short> h(n);
  std::vector<unsigned long long> want(65536), got(65536);
  std::mt19937_64 rng(1);
  const char* names[3] = {"uniform", "scene", "constant"};
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  for (int dist = 0; dist < 3; ++dist) {
    std::gamma_distribution<double> gamma(2.0, 150.0);
    for (long long i = 0; i < n; ++i)
      h[i] = dist == 0 ? (unsigned short)(rng() & 0xffff) : dist == 1 ? (unsigned short)std::fmin(gamma(rng), 65535.0) : (unsigned short)4242;
    std::fill(want.begin(), want.end(), 0ull);
    for (long long i = 0; i < n; ++i) ++want[h[i]];
    CHECK(hipMemcpy(d, h.data(), n * 2, hipMemcpyHostToDevice));
    for (int variant = 0; variant < 4; ++variant) {
      const int iters = 10;
      float best = 1e30f;
      for (int it = 0; it < iters + 1; ++it) {
        CHECK(hipMemsetAsync(counts, 0, 65536 * 8, 0));
        CHECK(hipEventRecord(a, 0));
        if (variant == 0) hipLaunchKernelGGL(hist_global<false>, dim3(cus * 8), dim3(256), 0, 0, d, n, counts);
        if (variant == 1) hipLaunchKernelGGL(hist_global<true>, dim3(cus * 8), dim3(256), 0, 0, d, n, counts);
        if (variant == 2) hipLaunchKernelGGL(hist_lds<false>, dim3(cus), dim3(1024), kWords * 4, 0, d, n, counts);
        if (variant == 3) hipLaunchKernelGGL(hist_lds<true>, dim3(cus), dim3(1024), kWords * 4, 0, d, n, counts);
        CHECK(hipEventRecord(b, 0));
        CHECK(hipEventSynchronize(b));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (it > 0 && ms < best) best = ms;
      }
      CHECK(hipMemcpy(got.data(), counts, 65536 * 8, hipMemcpyDeviceToHost));
      const char* vn[4] = {"global", "global+wave", "lds16", "lds16+wave"};
      std::printf("{\"pixels\": %lld, \"data\": \"%s\", \"variant\": \"%s\", \"best_ms\": %.4f, \"GBps\": %.1f, \"exact\": %s}\n", n, names[dist],
                  vn[variant], best, n * 2 / best / 1e6, got == want ? "true" : "false");
      std::fflush(stdout);
    }
  }
  return 0;
}
