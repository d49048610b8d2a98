// The two helpers the partial-row reductions of the training kernels share (bn_train.hip, colsum.hip and the backward files).
#pragma once

template <typename T>
__device__ __forceinline__ T sum16(T (*red)[64], int cl) {  // the 16 row-group partials of channel column cl
  T v = 0;
#pragma unroll
  for (int g = 0; g < 16; ++g) v += red[g][cl];
  return v;
}

static inline unsigned grid1d(long long total, int per_block, int cap) {
  long long b = (total + per_block - 1) / per_block;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}
