// The row layout of the streaming kernels whose tensors hold one row of `chw` floats per image (prediction.hip,
// x0_threshold.hip): 16-byte accesses over rows that need not be multiples of 4 floats or 16-byte aligned, and the capped grid.
#pragma once
#include <initializer_list>

#include "drs_common.h"

// One image's elements as [head | groups of 4 | tail]: the tensors of a call have one row of `chw` floats per image, and chw
// need not be a multiple of 4, so the rows after the first may start anywhere in a 16-byte line.  `phase` is the position
// (0 .. 3, in floats) of the tensors' first element in its line - the same for every tensor of the call, or the call runs
// element by element (`vec` false: groups = 0, everything is tail).
struct RowSpan {
  int64_t head, groups;
  __device__ RowSpan(bool vec, int phase, int64_t row_start, int64_t chw) {
    const int64_t h = (4 - ((phase + row_start) & 3)) & 3;
    head = !vec ? 0 : (h < chw ? h : chw);
    groups = vec ? (chw - head) / 4 : 0;
  }
  __device__ int64_t tail() const { return head + 4 * groups; }
};

inline int phase_of(const void* p) { return (int)(((uintptr_t)p & 15u) >> 2); }
// 16-byte accesses need every tensor's first element at the same place of its 16-byte line (then every row's is, too)
inline bool same_phase(std::initializer_list<const void*> ptrs) {
  const uintptr_t want = (uintptr_t)*ptrs.begin() & 15u;
  for (const void* p : ptrs)
    if (p && ((uintptr_t)p & 15u) != want) return false;
  return true;
}
// (blocks per image, images per sweep): about 2048 blocks of 256 threads in all, one thread per group (or element)
inline dim3 stream_grid(int n, int64_t chw, bool vec) {
  const int gy = n < 65535 ? n : 65535;
  const int64_t items = vec ? (chw + 3) / 4 + 1 : chw;
  int64_t gx = (items + 255) / 256, cap = 2048 / gy;
  if (cap < 1) cap = 1;
  if (gx > cap) gx = cap;
  return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)gy);
}
