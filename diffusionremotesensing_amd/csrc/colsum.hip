// Column sums of channels-last slices (the bias and time-embedding gradients of loss.backward(), reference
// train_diffusion_superres.py:388-393) and the finish kernel that adds per-block partial rows of floats in a fixed order.
#include "drs_common.h"
#include "train_reduce.h"

// ---------------------------------------------------------------------------------------------------------------
// Column sums of a channels-last slice: out[c] += sum_p t[p][c]   (bias gradients), or per image:
// out[n*out_stride + c] += sum over the image's pixels (time-embedding gradients).  fp32 partials + float atomics.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ t, int cs, int co, int C, long long npix,
                                                     long long pix_per_image, int per_image, int out_stride,
                                                     float* __restrict__ out, int rows_per_block) {
  __shared__ float red[256];
  const int lanes_c = C < 256 ? C : 256;            // threads along channels
  const int rows = 256 / lanes_c;                    // pixel rows handled concurrently
  const int c = threadIdx.x % lanes_c, row = threadIdx.x / lanes_c;
  const long long p_begin = (long long)blockIdx.x * rows_per_block;
  const long long p_end = min(npix, p_begin + rows_per_block);
  for (int cb = 0; cb < C; cb += lanes_c) {
    float s = 0.f;
    if (row < rows && cb + c < C)
      for (long long p = p_begin + row; p < p_end; p += rows) s += t[p * cs + co + cb + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (row == 0 && cb + c < C) {
      for (int r = 1; r < rows; ++r) s += red[r * lanes_c + c];
      const long long n = per_image ? p_begin / pix_per_image : 0;
      atomicAdd(&out[n * out_stride + cb + c], s);
    }
    __syncthreads();
  }
}
// float4 variant (C, cs, co multiples of 4; C <= 1024): thread = (pixel row, channel quad), 4 independent loads in flight
__global__ __launch_bounds__(256) void colsum4_kernel(const float* __restrict__ t, int cs, int co, int C, long long npix,
                                                      long long pix_per_image, int per_image, int out_stride,
                                                      float* __restrict__ out, int rows_per_block) {
  __shared__ float red[256][4];
  const int qn = C >> 2;
  const int rows = 256 / qn;
  const int q = threadIdx.x % qn, row = threadIdx.x / qn;
  const long long p_begin = (long long)blockIdx.x * rows_per_block;
  const long long p_end = min(npix, p_begin + rows_per_block);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    const float* base = t + co + q * 4;
    long long p = p_begin + row;
    for (; p + 3LL * rows < p_end; p += 4LL * rows) {
      const float4 a = *reinterpret_cast<const float4*>(base + p * cs);
      const float4 b = *reinterpret_cast<const float4*>(base + (p + rows) * cs);
      const float4 c2 = *reinterpret_cast<const float4*>(base + (p + 2LL * rows) * cs);
      const float4 d = *reinterpret_cast<const float4*>(base + (p + 3LL * rows) * cs);
      s[0] += (a.x + b.x) + (c2.x + d.x); s[1] += (a.y + b.y) + (c2.y + d.y);
      s[2] += (a.z + b.z) + (c2.z + d.z); s[3] += (a.w + b.w) + (c2.w + d.w);
    }
    for (; p < p_end; p += rows) {
      const float4 a = *reinterpret_cast<const float4*>(base + p * cs);
      s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[threadIdx.x][j] = s[j];
  __syncthreads();
  if (threadIdx.x < qn) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = 0.f;
      for (int r = 0; r < rows; ++r) v += red[r * qn + threadIdx.x][j];
      const long long n = per_image ? p_begin / pix_per_image : 0;
      atomicAdd(&out[n * out_stride + threadIdx.x * 4 + j], v);
    }
  }
}
// whole-tensor column sums without atomics: block b sums its rows into partials[b][C] (grid-stride over row groups), the
// finish kernel adds the rows into out
__global__ __launch_bounds__(256) void colsum4_partial_kernel(const float* __restrict__ t, int cs, int co, int C, long long npix,
                                                              float* __restrict__ partials) {
  __shared__ float red[256][4];
  const int qn = C >> 2;
  const int rows = 256 / qn;
  const int q = threadIdx.x % qn, row = threadIdx.x / qn;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    const float* base = t + co + q * 4;
    const long long stride = (long long)gridDim.x * rows;
    long long p = (long long)blockIdx.x * rows + row;
    for (; p + 3 * stride < npix; p += 4 * stride) {
      const float4 a = *reinterpret_cast<const float4*>(base + p * cs);
      const float4 b = *reinterpret_cast<const float4*>(base + (p + stride) * cs);
      const float4 c2 = *reinterpret_cast<const float4*>(base + (p + 2 * stride) * cs);
      const float4 d = *reinterpret_cast<const float4*>(base + (p + 3 * stride) * cs);
      s[0] += (a.x + b.x) + (c2.x + d.x); s[1] += (a.y + b.y) + (c2.y + d.y);
      s[2] += (a.z + b.z) + (c2.z + d.z); s[3] += (a.w + b.w) + (c2.w + d.w);
    }
    for (; p < npix; p += stride) {
      const float4 a = *reinterpret_cast<const float4*>(base + p * cs);
      s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[threadIdx.x][j] = s[j];
  __syncthreads();
  if (threadIdx.x < qn) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = 0.f;
      for (int r = 0; r < rows; ++r) v += red[r * qn + threadIdx.x][j];
      partials[(size_t)blockIdx.x * C + threadIdx.x * 4 + j] = v;
    }
  }
}
// The one float finish kernel of the per-block partial rows (column sums, psi, stem and few-channel weight gradients):
// dW[c] += sum of the partial rows for c < nW, db[c - nW] += ... for the rest; block = 64 columns x 16 row groups
__global__ __launch_bounds__(1024) void rows_finish_kernel(const float* __restrict__ partials, int nrows, int ncol, int nW,
                                                          float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float red[16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float v = 0.f;
  if (c < ncol)
#pragma unroll 8
    for (int r = rg; r < nrows; r += 16) v += partials[(size_t)r * ncol + c];
  red[rg][cl] = v;
  __syncthreads();
  if (rg != 0 || c >= ncol) return;
  const float s = sum16(red, cl);
  if (c < nW) { if (dW) dW[c] += s; }
  else if (db) db[c - nW] += s;
}
int drs_launch_rows_finish(const float* partials, int nrows, int ncol, int nW, float* dst_a, float* dst_b, hipStream_t s) {
  DRS_LAUNCH(rows_finish_kernel, dim3((ncol + 63) / 64), dim3(1024), 0, s, partials, nrows, ncol, nW, dst_a, dst_b);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
int drs_launch_colsum(const float* t, int cs, int co, int C, long long npix, long long pix_per_image, int per_image,
                      int out_stride, float* out, hipStream_t s, float* partials) {
  if (npix == 0) return DRS_OK;
  const bool vec4 = C % 4 == 0 && cs % 4 == 0 && co % 4 == 0 && C <= 1024 && 256 % (C >> 2) == 0;
  if (partials && !per_image && vec4) {
    // whole-tensor sums (bias gradients): every block would end in C float atomics onto the same C addresses - 2048 blocks x
    // ~90 ns per serialised atomic set the launch time (95 - 210 us), not the 134 MB it reads
    // (1024 blocks: with 512, 8 waves per CU x 4 loads in flight moved 1 TB/s - 154 us for the 268 MB slice of grad.cat2;
    //  the partials buffer holds DRS_RED_BLOCKS x 2 x 1024 doubles, i.e. 4096 rows of <= 1024 floats)
    const int rows = 256 / (C >> 2);
    const unsigned blocks = grid1d(npix, rows, 2 * DRS_RED_BLOCKS);
    DRS_LAUNCH(colsum4_partial_kernel, dim3(blocks), dim3(256), 0, s, t, cs, co, C, npix, partials);
    return drs_launch_rows_finish(partials, (int)blocks, C, C, out, nullptr, s);
  }
  long long rpb = per_image ? 512 : 2048;  // per-image sums: pix_per_image / rpb atomics per address (128 at 256 x 256)
  if (per_image) {
    // at least ~2048 blocks (the 17 - 67 MB tensors of the deep levels ran one block per CU at 1 TB/s), a block's rows a
    // multiple of 4 loads x the pixel rows it covers per pass; blocks must not straddle images
    const long long pass = vec4 ? 4LL * (256 / (C >> 2)) : 1;
    while (rpb > pass && npix / rpb < 2048) rpb >>= 1;
    while (pix_per_image % rpb) rpb >>= 1;
  }
  const long long blocks = (npix + rpb - 1) / rpb;
  if (vec4) {
    DRS_LAUNCH(colsum4_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, cs, co, C, npix, pix_per_image, per_image,
                       out_stride, out, (int)rpb);
    DRS_CHECK_HIP(hipGetLastError());
    return DRS_OK;
  }
  DRS_LAUNCH(colsum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, cs, co, C, npix, pix_per_image, per_image,
                     out_stride, out, (int)rpb);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
