// Image-quality sums of a super-resolved batch against its ground truth (metrics.py: PSNR, SSIM, SAM, ERGAS), per image.
// drs_metrics_pointwise reads both tensors once and leaves the per-band squared error, the per-band sum of the truth and
// the sum of the per-pixel spectral angles; drs_ssim is the 11 x 11 Gaussian-window SSIM of Wang et al. 2004 over the
// "valid" positions.  Both reduce the same way: fp32 per thread, wave and block, one fp64 partial per block in the
// caller's workspace, and a second kernel that adds the partials of an image in a fixed order - no atomics, so two calls
// on the same inputs return the same bits.
//
// drs_metrics_pointwise_nodata and drs_ssim_nodata are the MASKED instances of the same two kernels:
// no-data pixels of the truth (nodata_rule.h) are SELECTED out - never multiplied by zero - so that a NaN or an infinity under
// the mask reaches no output, and a batch without a no-data pixel gives the unmasked entries' bits.
#include "drs_common.h"
#include "nodata_rule.h"
#include <cmath>

// No contraction of a * b + c in this file (every fused multiply-add below is an explicit fmaf): identical inputs must give
// exactly 0 degrees and exactly SSIM 1, and a product contracted into a subtraction - u ru - v rv as one FMA - returns the
// rounding residue of the other product instead (HIP's __fmul_rn is a plain multiplication and does not prevent it).
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

// torch.clamp(v, 0, 1): a NaN stays a NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp01(float v) {
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, 0.f), 1.f);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0 holds the sum, always formed in the same order
}

// ---- pointwise sums ----------------------------------------------------------------------------------------------
// blockIdx.y = image, the x-grid strides over the groups of V consecutive pixels of that image; a thread holds the C values
// of its V pixels of both tensors in registers (CB = the register rows: 4 or kMaxBands), so that the two passes the angle
// needs (norms, then the difference of the NORMALISED vectors) cost no second read.  V = 4 needs hw % 4 == 0 and 16-byte
// aligned tensors: every plane of every image then starts on a 16-byte boundary.
// Angle of a pixel: 2 atan2(|u/|u| - v/|v||, |u/|u| + v/|v||).  Near-parallel vectors leave a small difference of nearly
// equal numbers, formed exactly, where acos(u.v / |u||v|) has lost half its digits (identical vectors: exactly 0).  A pixel
// whose vector is exactly zero in either image has no angle and is left out of sum and count.
// MASKED (drs_metrics_pointwise_nodata): the mask is that of hr's pixel (nodata_rule.h), taken from hr as stored, before the
// clamp; a no-data pixel leaves every chain as it was, so a batch without one gives the unmasked bits.
// partials: [image][block][K] = sse[C] | sum_hr[C] | angle sum (radians) | pixels in the angle sum, K = 2 C + 2;
// MASKED: | valid pixels, K = 2 C + 3
template <int V, int CB, bool MASKED>
__global__ __launch_bounds__(kThreads) void metrics_pointwise_kernel(const float* __restrict__ sr,
                                                                     const float* __restrict__ hr, float nodata_value,
                                                                     double* __restrict__ partials, int C, int64_t hw,
                                                                     int clamp) {
  constexpr int kCounts = MASKED ? 2 : 1;
  __shared__ float red[2 * CB + 1][kWaves];
  __shared__ int red_n[kCounts][kWaves];
  const float* sp = sr + (int64_t)blockIdx.y * C * hw;
  const float* hp = hr + (int64_t)blockIdx.y * C * hw;
  const int64_t groups = hw / V;
  const bool by_value = __builtin_isfinite(nodata_value);  // MASKED only, as ok, rule and nvalid
  float sse[CB], shr[CB], ang = 0.f;
  int cnt = 0, nvalid = 0;
#pragma unroll
  for (int c = 0; c < CB; ++c) sse[c] = shr[c] = 0.f;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
    float u[CB][V], v[CB][V], uu[V], vv[V];
    bool ok[V];
    NodataRule<V> rule;
#pragma unroll
    for (int p = 0; p < V; ++p) uu[p] = vv[p] = 0.f;
    // MASKED: a pixel's mask needs all its bands, so the sums wait for a second walk over the bands held in registers
    constexpr int kSumPass = MASKED ? 1 : 0;
#pragma unroll
    for (int pass = 0; pass <= kSumPass; ++pass) {
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        if (c >= C) continue;
        if (pass == 0) {
          if constexpr (V == 4) {
            const float4 a = *reinterpret_cast<const float4*>(sp + c * hw + g * 4);
            const float4 b = *reinterpret_cast<const float4*>(hp + c * hw + g * 4);
            u[c][0] = a.x; u[c][1] = a.y; u[c][2] = a.z; u[c][3] = a.w;
            v[c][0] = b.x; v[c][1] = b.y; v[c][2] = b.z; v[c][3] = b.w;
          } else {
            u[c][0] = sp[c * hw + g];
            v[c][0] = hp[c * hw + g];
          }
          if constexpr (MASKED) rule.band(v[c], nodata_value);
        }
        if (pass != kSumPass) continue;
#pragma unroll
        for (int p = 0; p < V; ++p) {
          if (clamp) {
            u[c][p] = clamp01(u[c][p]);
            v[c][p] = clamp01(v[c][p]);
          }
          if constexpr (MASKED)
            if (!ok[p]) continue;
          const float d = u[c][p] - v[c][p];
          sse[c] = fmaf(d, d, sse[c]);
          shr[c] += v[c][p];
          uu[p] = fmaf(u[c][p], u[c][p], uu[p]);
          vv[p] = fmaf(v[c][p], v[c][p], vv[p]);
        }
      }
      if constexpr (MASKED) {
        if (pass == 0) {
#pragma unroll
          for (int p = 0; p < V; ++p) {
            ok[p] = !rule.nodata(p, by_value);
            nvalid += ok[p];
          }
        }
      }
    }
#pragma unroll
    for (int p = 0; p < V; ++p) {
      if (uu[p] == 0.f || vv[p] == 0.f) continue;  // (a NaN norm is not zero: it enters, and the image's angle is NaN)
      if constexpr (MASKED)
        if (!ok[p]) continue;
      const float ru = 1.f / sqrtf(uu[p]), rv = 1.f / sqrtf(vv[p]);
      float d2 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        if (c >= C) continue;
        const float a = u[c][p] * ru, b = v[c][p] * rv;
        d2 = fmaf(a - b, a - b, d2);
        s2 = fmaf(a + b, a + b, s2);
      }
      ang += 2.f * atan2f(sqrtf(d2), sqrtf(s2));
      cnt += 1;
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    if (c >= C) continue;
    const float a = wave_sum(sse[c]), b = wave_sum(shr[c]);
    if (lane == 0) {
      red[c][wave] = a;
      red[CB + c][wave] = b;
    }
  }
  ang = wave_sum(ang);
  cnt = wave_sum(cnt);
  if constexpr (MASKED) nvalid = wave_sum(nvalid);
  if (lane == 0) {
    red[2 * CB][wave] = ang;
    red_n[0][wave] = cnt;
    if constexpr (MASKED) red_n[1][wave] = nvalid;
  }
  __syncthreads();
  const int K = 2 * C + 1 + kCounts, k = threadIdx.x;
  if (k < K) {
    double* out = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * K;
    if (k >= K - kCounts) {
      int n = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) n += red_n[k - (K - kCounts)][w];
      out[k] = (double)n;
    } else {
      const int row = k < C ? k : (k < 2 * C ? CB + k - C : 2 * CB);
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) s += red[row][w];
      out[k] = (double)s;
    }
  }
}

// The block sum behind every reduce: threads stride over the n partials of a column (K doubles apart), then the LDS tree.
// All threads return the sum; `red` is free again after a barrier.
__device__ __forceinline__ double column_sum(const double* p, int64_t n, int K, double* red) {
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kThreads) s += p[j * K];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// out[image][k] = (sum over j < n, in a fixed order, of partials[image][j][k]) / divisor.  blockIdx.x = k, blockIdx.y = image.
// (divisor 1: the sum's own bits)
__global__ __launch_bounds__(kThreads) void metrics_reduce_kernel(const double* __restrict__ partials,
                                                                  double* __restrict__ out, int64_t n, int K,
                                                                  double divisor) {
  __shared__ double red[kThreads];
  const double s = column_sum(partials + (int64_t)blockIdx.y * n * K + blockIdx.x, n, K, red);
  if (threadIdx.x == 0) out[(int64_t)blockIdx.y * K + blockIdx.x] = s / divisor;
}

// out[image] = (sum of the C * tiles SSIM partials / (C * positions), positions) with positions = the sum of the image's
// `tiles` counts; NaN without a position.  blockIdx.x = image.
__global__ __launch_bounds__(kThreads) void ssim_nodata_reduce_kernel(const double* __restrict__ sums,
                                                                      const double* __restrict__ counts,
                                                                      double* __restrict__ out, int C, int64_t tiles) {
  __shared__ double red[kThreads];
  const double s = column_sum(sums + (int64_t)blockIdx.x * C * tiles, (int64_t)C * tiles, 1, red);
  __syncthreads();
  const double n = column_sum(counts + (int64_t)blockIdx.x * tiles, tiles, 1, red);
  if (threadIdx.x == 0) {
    out[2 * (int64_t)blockIdx.x] = n > 0.0 ? s / ((double)C * n) : __longlong_as_double(0x7ff8000000000000LL);
    out[2 * (int64_t)blockIdx.x + 1] = n;
  }
}

// mask[image][pixel] = 1 where hr's pixel is data, from one pass over hr: blockIdx.y = image, a thread takes V consecutive pixels
// of all bands (V = 4: hw % 4 == 0 and a 16-byte aligned hr; the mask rows are then 4-byte aligned in the workspace).
template <int V>
__global__ __launch_bounds__(kThreads) void hr_mask_kernel(const float* __restrict__ hr, float nodata_value,
                                                           unsigned char* __restrict__ mask, int C, int64_t hw) {
  const float* hp = hr + (int64_t)blockIdx.y * C * hw;
  unsigned char* mp = mask + (int64_t)blockIdx.y * hw;
  const bool by_value = __builtin_isfinite(nodata_value);
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < hw / V; g += (int64_t)gridDim.x * kThreads) {
    NodataRule<V> rule;
    for (int c = 0; c < C; ++c) {
      float v[V];
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(hp + c * hw + g * 4);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
        v[0] = hp[c * hw + g];
      }
      rule.band(v, nodata_value);
    }
    unsigned char ok[V];
#pragma unroll
    for (int p = 0; p < V; ++p) ok[p] = !rule.nodata(p, by_value);
    if constexpr (V == 4) {
      *reinterpret_cast<uchar4*>(mp + g * 4) = make_uchar4(ok[0], ok[1], ok[2], ok[3]);
    } else {
      mp[g] = ok[0];
    }
  }
}

// ---- SSIM --------------------------------------------------------------------------------------------------------
constexpr int kWin = 11;                        // window side; sigma 1.5 (ssim_window)
constexpr int kTile = 32;                       // output positions of a block: kTile x kTile
constexpr int kIn = kTile + kWin - 1;           // 42: side of the staged input tile (5-pixel halo on every side)
constexpr int kInStride = kIn + 1, kRowStride = kTile + 1;
constexpr int kRun = 4;                         // consecutive outputs one thread forms in the horizontal pass
struct SsimWindow { float g[kWin]; };

// One block per (output tile, band, image).  Both input tiles are staged in LDS with a per-tile pivot (the pixel in the
// middle of the tile) subtracted: variances and covariance do not change under a shift, the pivot goes back into the means
// only, and E[x^2] - mu^2 no longer cancels on flat bright terrain (0.95 +- 0.002: the moments are formed on +-0.002).
// Horizontal 11-tap pass of the five moments (x, y, x^2, y^2, xy) into LDS, vertical pass in registers (a thread owns 4
// rows of one column), SSIM per position, block sum.  Tiles may overhang the image: positions outside the (H - 10) x
// (W - 10) valid region contribute nothing, pixels outside the image are staged as zeros and reach no valid position.
// The formula is evaluated with explicitly rounded operations so that sr == hr gives num == den bit for bit: exactly 1.
// MASKED (drs_ssim_nodata): over the window positions whose 11 x 11 pixels are all valid.  The block first stages the mask of
// its 42 x 42 input tile (hr_mask_kernel's bytes: one per pixel, shared by the bands' blocks), then takes the pivot from the
// tile's middle pixel, or - when that pixel is no-data - from the first valid pixel of the tile in row order; no-data pixels
// are staged as zeros in both images and reach counted positions never: a position is counted when the box sum of the mask
// over its window is 121.  counts[image][tile] = the positions counted (the mask is the bands' own: band 0's blocks write it).
template <bool MASKED>
struct SsimMaskLds {};  // (the unmasked kernel holds no byte of it)
template <>
struct SsimMaskLds<true> {
  // (each array on a 16-byte boundary, as separate __shared__ arrays are: 1.6 % of the kernel's time on an MI355X)
  alignas(16) unsigned char sm[kIn * kInStride];      // the tile's mask: 1 = inside the image and valid
  alignas(16) unsigned char hk[kIn][kRowStride + 3];  // its horizontal 11-sums
  alignas(16) int red_i[kWaves];
};

template <bool MASKED>
__global__ __launch_bounds__(kThreads) void ssim_kernel(const float* __restrict__ sr, const float* __restrict__ hr,
                                                        const unsigned char* __restrict__ mask, double* __restrict__ partials,
                                                        double* __restrict__ counts, SsimWindow win, int C, int H, int W,
                                                        int tiles_x, int clamp) {
  __shared__ float sx[kIn * kInStride], sy[kIn * kInStride];
  __shared__ float hm[5][kIn][kRowStride];
  __shared__ float red[kWaves];
  __shared__ SsimMaskLds<MASKED> ml;
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
  const float* xp = sr + ((int64_t)b * C + c) * H * W;
  const float* yp = hr + ((int64_t)b * C + c) * H * W;
  int py = min(ty0 + kIn / 2, H - 1), px = min(tx0 + kIn / 2, W - 1);  // the pivot: image coordinates
  if constexpr (MASKED) {
    const unsigned char* mp = mask + (int64_t)b * H * W;
    for (int i = tid; i < kIn * kIn; i += kThreads) {
      const int ly = i / kIn, lx = i % kIn, gy = ty0 + ly, gx = tx0 + lx;
      ml.sm[ly * kInStride + lx] = gy < H && gx < W && mp[(int64_t)gy * W + gx] != 0;
    }
    __syncthreads();
    if (!ml.sm[(py - ty0) * kInStride + px - tx0]) {  // (the same for every thread of the block)
      int best = kIn * kIn;
      for (int i = tid; i < kIn * kIn; i += kThreads)
        if (ml.sm[(i / kIn) * kInStride + i % kIn]) best = min(best, i);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_down(best, o, 64));
      if (tid % 64 == 0) ml.red_i[tid / 64] = best;
      __syncthreads();
      best = min(min(ml.red_i[0], ml.red_i[1]), min(ml.red_i[2], ml.red_i[3]));
      // (no valid pixel: no position is counted, the pivot is not used)
      if (best < kIn * kIn) py = ty0 + best / kIn, px = tx0 + best % kIn;
    }
  }
  const int64_t pivot = (int64_t)py * W + px;
  const float pvx = clamp ? clamp01(xp[pivot]) : xp[pivot], pvy = clamp ? clamp01(yp[pivot]) : yp[pivot];
  for (int i = tid; i < kIn * kIn; i += kThreads) {
    const int ly = i / kIn, lx = i % kIn, gy = ty0 + ly, gx = tx0 + lx;
    float a = 0.f, v = 0.f;
    bool staged = gy < H && gx < W;
    if constexpr (MASKED) staged = ml.sm[ly * kInStride + lx];  // (inside the image, and valid)
    if (staged) {
      a = xp[(int64_t)gy * W + gx];
      v = yp[(int64_t)gy * W + gx];
      if (clamp) {
        a = clamp01(a);
        v = clamp01(v);
      }
      a -= pvx;
      v -= pvy;
    }
    sx[ly * kInStride + lx] = a;
    sy[ly * kInStride + lx] = v;
  }
  __syncthreads();
  for (int i = tid; i < kIn * (kTile / kRun); i += kThreads) {
    const int r = i / (kTile / kRun), q = (i % (kTile / kRun)) * kRun;
    float xs[kRun + kWin - 1], ys[kRun + kWin - 1];
    int ms[kRun + kWin - 1];  // MASKED only
#pragma unroll
    for (int k = 0; k < kRun + kWin - 1; ++k) {
      xs[k] = sx[r * kInStride + q + k];
      ys[k] = sy[r * kInStride + q + k];
      if constexpr (MASKED) ms[k] = ml.sm[r * kInStride + q + k];
    }
#pragma unroll
    for (int o = 0; o < kRun; ++o) {
      float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
      int valid = 0;
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const float w = win.g[k], a = xs[o + k], v = ys[o + k];
        const float aa = __fmul_rn(a, a), vv = __fmul_rn(v, v), av = __fmul_rn(a, v);
        m[0] = fmaf(w, a, m[0]);
        m[1] = fmaf(w, v, m[1]);
        m[2] = fmaf(w, aa, m[2]);
        m[3] = fmaf(w, vv, m[3]);
        m[4] = fmaf(w, av, m[4]);
        if constexpr (MASKED) valid += ms[o + k];
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) hm[j][r][q + o] = m[j];
      if constexpr (MASKED) ml.hk[r][q + o] = (unsigned char)valid;
    }
  }
  __syncthreads();
  constexpr int kRows = kTile * kTile / kThreads;  // 4 rows of one column per thread
  const int col = tid % kTile, row0 = (tid / kTile) * kRows;
  float mo[5][kRows];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    float vals[kRows + kWin - 1];
#pragma unroll
    for (int k = 0; k < kRows + kWin - 1; ++k) vals[k] = hm[j][row0 + k][col];
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; ++k) s = fmaf(win.g[k], vals[o + k], s);
      mo[j][o] = s;
    }
  }
  int box[kRows];  // MASKED only: the valid pixels under each position's window
  if constexpr (MASKED) {
    int vals[kRows + kWin - 1];
#pragma unroll
    for (int k = 0; k < kRows + kWin - 1; ++k) vals[k] = ml.hk[row0 + k][col];
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < kWin; ++k) s += vals[o + k];
      box[o] = s;
    }
  }
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;  // (K1 L)^2, (K2 L)^2 with data range L = 1
  float acc = 0.f;
  int positions = 0;
#pragma unroll
  for (int o = 0; o < kRows; ++o) {
    if (ty0 + row0 + o > H - kWin || tx0 + col > W - kWin) continue;
    if constexpr (MASKED)
      if (box[o] != kWin * kWin) continue;
    const float mx = mo[0][o], my = mo[1][o];
    const float vx = fmaf(-mx, mx, mo[2][o]), vy = fmaf(-my, my, mo[3][o]), cxy = fmaf(-mx, my, mo[4][o]);
    const float mux = __fadd_rn(mx, pvx), muy = __fadd_rn(my, pvy);
    const float mxy = __fmul_rn(mux, muy);
    const float num = __fmul_rn(__fadd_rn(__fadd_rn(mxy, mxy), C1), __fadd_rn(__fadd_rn(cxy, cxy), C2));
    const float den = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(mux, mux), __fmul_rn(muy, muy)), C1),
                                __fadd_rn(__fadd_rn(vx, vy), C2));
    acc += __fdiv_rn(num, den);
    positions += 1;
  }
  acc = wave_sum(acc);
  if constexpr (MASKED) {
    positions = wave_sum(positions);
    __syncthreads();  // (red_i: the pivot search)
    if (tid % 64 == 0) ml.red_i[tid / 64] = positions;
  }
  if (tid % 64 == 0) red[tid / 64] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[w];
    partials[((int64_t)b * C + c) * gridDim.x + blockIdx.x] = (double)s;
    if constexpr (MASKED) {
      int n = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) n += ml.red_i[w];
      if (c == 0) counts[(int64_t)b * gridDim.x + blockIdx.x] = (double)n;
    }
  }
}

SsimWindow ssim_window() {
  double g[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) sum += g[k] = std::exp(-(k - kWin / 2) * (k - kWin / 2) / (2.0 * 1.5 * 1.5));
  SsimWindow w;
  for (int k = 0; k < kWin; ++k) w.g[k] = (float)(g[k] / sum);
  return w;
}

// blocks per image of the pointwise kernel: about two groups per thread, at most 256 partial rows per image
int pointwise_blocks(int64_t hw, int V) {
  const int64_t b = (hw / V + 2 * kThreads - 1) / (2 * kThreads);
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}
int64_t ssim_tiles(int H, int W) {
  return (int64_t)drs_cdiv(H - kWin + 1, kTile) * drs_cdiv(W - kWin + 1, kTile);
}
bool shape_ok(int B, int C, int H, int W, int side) {
  return B >= 1 && B <= 65535 && C >= 1 && C <= kMaxBands && H >= side && W >= side;
}

// The workspace of either pair of entries.  MASKED: one column more per pointwise row, one count per SSIM tile, then
// drs_ssim_nodata's mask bytes.
size_t metrics_workspace_bytes(int B, int C, int H, int W, bool masked) {
  if (!shape_ok(B, C, H, W, 1)) return 0;
  const int extra = masked ? 1 : 0;
  // (the scalar instance of the pointwise kernel has the most blocks)
  size_t rows = (size_t)pointwise_blocks((int64_t)H * W, 1) * (2 * C + 2 + extra);
  if (H >= kWin && W >= kWin && (size_t)(C + extra) * ssim_tiles(H, W) > rows) rows = (size_t)(C + extra) * ssim_tiles(H, W);
  return (size_t)B * rows * sizeof(double) + (masked ? (size_t)B * H * W : 0);
}

template <int V, bool MASKED>
void launch_pointwise(const float* sr, const float* hr, float nodata_value, double* ws, int B, int C, int64_t hw, int clamp,
                      int nb, hipStream_t s) {
  if (C <= 4) {
    DRS_LAUNCH((metrics_pointwise_kernel<V, 4, MASKED>), dim3(nb, B), dim3(kThreads), 0, s, sr, hr, nodata_value, ws, C, hw, clamp);
  } else {
    DRS_LAUNCH((metrics_pointwise_kernel<V, kMaxBands, MASKED>), dim3(nb, B), dim3(kThreads), 0, s, sr, hr, nodata_value, ws, C, hw,
               clamp);
  }
}

// drs_metrics_pointwise and, MASKED, drs_metrics_pointwise_nodata; `what` names the entry in the error texts
template <bool MASKED>
int metrics_pointwise(const char* what, const float* sr, const float* hr, float nodata_value, double* out, int B, int C, int H,
                      int W, int clamp, void* workspace, size_t workspace_bytes, hipStream_t s) {
  DRS_REQUIRE(sr && hr && out && workspace, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(shape_ok(B, C, H, W, 1), DRS_ERR_SHAPE, "%s: B=%d C=%d H=%d W=%d (1 <= C <= %d)", what, B, C, H, W, kMaxBands);
  const int64_t hw = (int64_t)H * W;
  const bool wide = hw % 4 == 0 && ((uintptr_t)sr | (uintptr_t)hr) % 16 == 0;
  const int nb = pointwise_blocks(hw, wide ? 4 : 1), K = 2 * C + (MASKED ? 3 : 2);
  DRS_REQUIRE(workspace_bytes >= (size_t)B * nb * K * sizeof(double), DRS_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed",
              what, workspace_bytes, (size_t)B * nb * K * sizeof(double));
  double* ws = (double*)workspace;
  if (wide) launch_pointwise<4, MASKED>(sr, hr, nodata_value, ws, B, C, hw, clamp, nb, s);
  else launch_pointwise<1, MASKED>(sr, hr, nodata_value, ws, B, C, hw, clamp, nb, s);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(metrics_reduce_kernel, dim3(K, B), dim3(kThreads), 0, s, ws, out, (int64_t)nb, K, 1.0);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// drs_ssim and, MASKED, drs_ssim_nodata.  MASKED workspace: the C * tiles sums, the tiles' counts, then the mask bytes.
template <bool MASKED>
int ssim(const char* what, const float* sr, const float* hr, float nodata_value, double* out, int B, int C, int H, int W,
         int clamp, void* workspace, size_t workspace_bytes, hipStream_t s) {
  DRS_REQUIRE(sr && hr && out && workspace, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(shape_ok(B, C, H, W, kWin), DRS_ERR_SHAPE, "%s: B=%d C=%d H=%d W=%d (1 <= C <= %d, H and W >= %d)", what, B, C, H, W,
              kMaxBands, kWin);
  const int64_t tiles = ssim_tiles(H, W), hw = (int64_t)H * W;
  DRS_REQUIRE(tiles <= INT32_MAX, DRS_ERR_SHAPE, "%s: H=%d W=%d need more tiles than one launch holds", what, H, W);
  const size_t need = (size_t)B * (C + (MASKED ? 1 : 0)) * tiles * sizeof(double) + (MASKED ? (size_t)B * hw : 0);
  DRS_REQUIRE(workspace_bytes >= need, DRS_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  double* ws = (double*)workspace;
  double* counts = MASKED ? ws + (size_t)B * C * tiles : nullptr;
  unsigned char* mask = MASKED ? (unsigned char*)(counts + (size_t)B * tiles) : nullptr;
  if (MASKED) {
    const bool wide = hw % 4 == 0 && (uintptr_t)hr % 16 == 0 && (uintptr_t)mask % 4 == 0;
    const int V = wide ? 4 : 1;
    const dim3 mgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>((hw / V + kThreads - 1) / kThreads, 1024)), B);
    if (wide) DRS_LAUNCH(hr_mask_kernel<4>, mgrid, dim3(kThreads), 0, s, hr, nodata_value, mask, C, hw);
    else DRS_LAUNCH(hr_mask_kernel<1>, mgrid, dim3(kThreads), 0, s, hr, nodata_value, mask, C, hw);
    DRS_CHECK_HIP(hipGetLastError());
  }
  DRS_LAUNCH(ssim_kernel<MASKED>, dim3((unsigned)tiles, C, B), dim3(kThreads), 0, s, sr, hr, (const unsigned char*)mask, ws, counts,
             ssim_window(), C, H, W, drs_cdiv(W - kWin + 1, kTile), clamp);
  DRS_CHECK_HIP(hipGetLastError());
  if (MASKED)
    DRS_LAUNCH(ssim_nodata_reduce_kernel, dim3(B), dim3(kThreads), 0, s, (const double*)ws, (const double*)counts, out, C, tiles);
  else
    DRS_LAUNCH(metrics_reduce_kernel, dim3(1, B), dim3(kThreads), 0, s, (const double*)ws, out, (int64_t)C * tiles, 1,
               (double)C * (H - kWin + 1) * (double)(W - kWin + 1));
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

}  // namespace

extern "C" DRS_API size_t drs_metrics_workspace_bytes(int B, int C, int H, int W) {
  return metrics_workspace_bytes(B, C, H, W, false);
}

extern "C" DRS_API size_t drs_metrics_nodata_workspace_bytes(int B, int C, int H, int W) {
  return metrics_workspace_bytes(B, C, H, W, true);
}

extern "C" DRS_API int drs_metrics_pointwise(const float* sr, const float* hr, double* out, int B, int C, int H, int W,
                                             int clamp, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return metrics_pointwise<false>("metrics_pointwise", sr, hr, 0.f, out, B, C, H, W, clamp, workspace, workspace_bytes,
                                  (hipStream_t)stream);
}

extern "C" DRS_API int drs_metrics_pointwise_nodata(const float* sr, const float* hr, float nodata_value, double* out, int B,
                                                    int C, int H, int W, int clamp, void* workspace, size_t workspace_bytes,
                                                    drs_stream_t stream) {
  return metrics_pointwise<true>("metrics_pointwise_nodata", sr, hr, nodata_value, out, B, C, H, W, clamp, workspace,
                                 workspace_bytes, (hipStream_t)stream);
}

extern "C" DRS_API int drs_ssim(const float* sr, const float* hr, double* out, int B, int C, int H, int W, int clamp,
                                void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return ssim<false>("ssim", sr, hr, 0.f, out, B, C, H, W, clamp, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" DRS_API int drs_ssim_nodata(const float* sr, const float* hr, float nodata_value, double* out, int B, int C, int H,
                                       int W, int clamp, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return ssim<true>("ssim_nodata", sr, hr, nodata_value, out, B, C, H, W, clamp, workspace, workspace_bytes, (hipStream_t)stream);
}
