// Batch gathers of the SAR -> NDVI and class-folder data feeds (feeds.py): the dataset lives decoded in a cache on the device,
// and one launch writes a whole batch in the form the reference's dataset item has it:
//   pairs: out[i, :] = (cache[idx[i], :] + 1) * 0.5   for both tensors of a (SAR, NDVI) pair (utils.py:88-89: `(img + 1) / 2`;
//          halving and dividing by two are the same IEEE operation)
//   u8:    img[i, :] = float(cache[idx[i], :]) / 255  (ToTensor's `.div(255)`: a true division), labels_out[i] = labels[idx[i]]
// Pure streaming: each output row is cut into `slots` of one 16-byte vector of the source (4 floats / 16 bytes), one thread per
// slot.  Source row idx[i] and output row i start at unrelated offsets, so a row goes one of two ways:
//   * co-aligned (after a head of h elements both pointers are 16-byte aligned): slot 0 = the scalar head, slots 1 .. nb = one
//     vector load and one (u8: four) vector store(s), slot nb + 1 = the scalar tail;
//   * otherwise (rows of a length that is no multiple of 4 / 16, from the second row on): element q + k * slots for k < 4 / 16,
//     so that the lanes of a wave still touch consecutive addresses.
// blockIdx.y walks the batch rows (and, for pairs, blockIdx.z the two tensors), blockIdx.x the slots of a row: no division.
// An index outside [0, L) reads nothing: its row is written as zeros, its label as -1.
#include "drs_common.h"

namespace {

constexpr int kThreads = 256;

struct PairSide {
  const float* cache;
  float* out;
  int row;
};

__device__ __forceinline__ float unit_from_pm1(float v) {
#pragma clang fp contract(off)
  return (v + 1.0f) * 0.5f;
}

__device__ __forceinline__ float unit_from_u8(unsigned b) { return __fdiv_rn((float)b, 255.f); }

__global__ __launch_bounds__(kThreads) void gather_pairs_kernel(PairSide sar, PairSide ndvi, const long long* __restrict__ idx,
                                                                int n, long long L) {
  const PairSide side = blockIdx.z == 0 ? sar : ndvi;
  const int row = side.row;
  const int slots = row / 4 + 2;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const long long src_row = idx[i];
    const bool valid = src_row >= 0 && src_row < L;
    const float* __restrict__ s = side.cache + (valid ? src_row : 0) * row;
    float* __restrict__ d = side.out + (long long)i * row;
    int h = (int)(((16 - ((uintptr_t)d & 15)) & 15) >> 2);  // floats in front of the first 16-byte aligned one of the output row
    if (h > row) h = row;
    const bool vec = valid && (((uintptr_t)(s + h)) & 15) == 0;
    const int nb = (row - h) / 4;
    for (int q = blockIdx.x * kThreads + threadIdx.x; q < slots; q += gridDim.x * kThreads) {
      if (!vec) {
        for (int k = 0; k < 4; ++k) {
          const long long e = q + (long long)k * slots;
          if (e < row) d[e] = valid ? unit_from_pm1(s[e]) : 0.f;
        }
      } else if (q == 0) {
        for (int e = 0; e < h; ++e) d[e] = unit_from_pm1(s[e]);
      } else if (q <= nb) {
        const int e = h + 4 * (q - 1);
        const float4 v = *reinterpret_cast<const float4*>(s + e);
        *reinterpret_cast<float4*>(d + e) =
            make_float4(unit_from_pm1(v.x), unit_from_pm1(v.y), unit_from_pm1(v.z), unit_from_pm1(v.w));
      } else if (q == nb + 1) {
        for (int e = h + 4 * nb; e < row; ++e) d[e] = unit_from_pm1(s[e]);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void gather_u8_kernel(const unsigned char* __restrict__ cache,
                                                             const long long* __restrict__ labels,
                                                             const long long* __restrict__ idx, int n, long long L, int row,
                                                             float* __restrict__ img_out, long long* __restrict__ labels_out) {
  const int slots = row / 16 + 2;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const long long src_row = idx[i];
    const bool valid = src_row >= 0 && src_row < L;
    if (blockIdx.x == 0 && threadIdx.x == 0) labels_out[i] = valid ? labels[src_row] : -1;
    const unsigned char* __restrict__ s = cache + (valid ? src_row : 0) * row;
    float* __restrict__ d = img_out + (long long)i * row;
    int h = (int)((16 - ((uintptr_t)s & 15)) & 15);  // bytes in front of the first 16-byte aligned one of the cache row
    if (h > row) h = row;
    const bool vec = valid && (((uintptr_t)(d + h)) & 15) == 0;
    const int nb = (row - h) / 16;
    for (int q = blockIdx.x * kThreads + threadIdx.x; q < slots; q += gridDim.x * kThreads) {
      if (!vec) {
        for (int k = 0; k < 16; ++k) {
          const long long e = q + (long long)k * slots;
          if (e < row) d[e] = valid ? unit_from_u8(s[e]) : 0.f;
        }
      } else if (q == 0) {
        for (int e = 0; e < h; ++e) d[e] = unit_from_u8(s[e]);
      } else if (q <= nb) {
        const int e = h + 16 * (q - 1);
        const uint4 v = *reinterpret_cast<const uint4*>(s + e);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<float4*>(d + e + 4 * j) =
              make_float4(unit_from_u8(w[j] & 0xffu), unit_from_u8((w[j] >> 8) & 0xffu), unit_from_u8((w[j] >> 16) & 0xffu),
                          unit_from_u8(w[j] >> 24));
      } else if (q == nb + 1) {
        for (int e = h + 16 * nb; e < row; ++e) d[e] = unit_from_u8(s[e]);
      }
    }
  }
}

// blocks along a row of `slots` slots (at most 1024, the rest by the kernel's stride), batch rows along y (at most 65535)
inline dim3 feed_grid(int slots, int n, int sides) {
  const int bx = (slots + kThreads - 1) / kThreads;
  return dim3((unsigned)(bx > 1024 ? 1024 : bx), (unsigned)(n > 65535 ? 65535 : n), (unsigned)sides);
}
}  // namespace

extern "C" int drs_gather_pairs_f32(const float* sar_cache, const float* ndvi_cache, const int64_t* idx, int n, int64_t L,
                                    int sar_row, int ndvi_row, float* sar_out, float* ndvi_out, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(sar_cache && ndvi_cache && idx && sar_out && ndvi_out, DRS_ERR_ARG, "gather_pairs: null pointer");
  DRS_REQUIRE(n >= 1 && L >= 1 && sar_row >= 1 && ndvi_row >= 1, DRS_ERR_SHAPE,
              "gather_pairs: n=%d L=%lld sar_row=%d ndvi_row=%d", n, (long long)L, sar_row, ndvi_row);
  const int slots = (sar_row > ndvi_row ? sar_row : ndvi_row) / 4 + 2;
  DRS_LAUNCH(gather_pairs_kernel, feed_grid(slots, n, 2), dim3(kThreads), 0, s, PairSide{sar_cache, sar_out, sar_row},
             PairSide{ndvi_cache, ndvi_out, ndvi_row}, (const long long*)idx, n, (long long)L);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_gather_u8_f32(const uint8_t* cache_u8, const int64_t* labels, const int64_t* idx, int n, int64_t L, int row,
                                 float* img_out, int64_t* labels_out, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(cache_u8 && labels && idx && img_out && labels_out, DRS_ERR_ARG, "gather_u8: null pointer");
  DRS_REQUIRE(n >= 1 && L >= 1 && row >= 1, DRS_ERR_SHAPE, "gather_u8: n=%d L=%lld row=%d", n, (long long)L, row);
  DRS_LAUNCH(gather_u8_kernel, feed_grid(row / 16 + 2, n, 1), dim3(kThreads), 0, s, cache_u8, (const long long*)labels,
             (const long long*)idx, n, (long long)L, row, img_out, (long long*)labels_out);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
