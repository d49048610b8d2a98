// The no-data pixel rule, written once: a pixel of a clean / truth image (C, H, W) is no-data when any
// of its bands is NaN or, with a finite `nodata_value`, when all of its bands equal it (fp32 compare).  The mask is per pixel,
// shared by the bands, and taken from the image as stored, before any clamp.  A kernel feeds the bands of its V pixels one by
// one (nodata.hip: the noising kernel; metrics.hip: the pointwise kernel and hr_mask_kernel).
#pragma once
#include <hip/hip_runtime.h>

template <int V>
struct NodataRule {
  bool nan[V], same[V];
  __device__ __forceinline__ NodataRule() {
#pragma unroll
    for (int k = 0; k < V; ++k) nan[k] = false, same[k] = true;
  }
  __device__ __forceinline__ void band(const float (&v)[V], float nodata_value) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      nan[k] = nan[k] || v[k] != v[k];
      same[k] = same[k] && v[k] == nodata_value;
    }
  }
  // `by_value` = __builtin_isfinite(nodata_value), formed once per kernel
  __device__ __forceinline__ bool nodata(int k, bool by_value) const { return nan[k] || (by_value && same[k]); }
};
