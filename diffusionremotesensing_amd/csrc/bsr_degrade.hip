// The ops of the blind (BSRGAN-plus) degradation feed (bsr.py; definitions in include/drs_hip.h and DESIGN.md section 19), each one
// launch over a dense (N, C, H, W) fp32 batch:
//   blur      a k x k kernel per image (k odd, <= 25), true convolution on the reflect-101 border, image tile + halo and the
//             image's kernel in LDS; a separable form for one 1-D kernel of up to 51 taps (the USM's Gaussian)
//   sharpen   the USM of the HR image on two launches of the separable form
//   resize    bilinear / bicubic (a = -0.75) / area at half-pixel centres on a replicated border, clip fused
//   noise     additive / speckle / Poisson combination per image from given draws (no RNG in a kernel), clip fused
//   jpeg      a baseline-JPEG round trip (4:2:0, per-image quality) in integer arithmetic, one work-group per 16 x 16 MCU
#include "drs_common.h"

namespace {

constexpr int kThreads = 256;

// index i of an axis of n samples continued by reflection about the centres of the first and last sample (cv2's
// BORDER_REFLECT_101, scipy's "mirror"), as often as it takes: an image may be smaller than the halo
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}
__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---- blur: one k x k kernel per image -------------------------------------------------------------------------------------
// One block per kBW x kBH output tile of one plane.  The tile and its halo of r = ks / 2 pixels are staged in LDS with the
// border already resolved, the image's kernel is staged FLIPPED and by columns, kf[b][kPad + a] = k[2r - a][2r - b], between
// kPad zeros, so the convolution out(y, x) = sum k[i][j] in(y + r - i, x + r - j) is the correlation sum_{a,b} kf[b][a]
// tile[ly + a][lx + b].  A thread owns one column of kRun consecutive rows: per (b, t) it reads ONE tile value and ONE kernel
// value (the same address for the whole wave: a broadcast) and issues kRun FMAs, the kernel values sliding through registers;
// the zeros past the kernel's end turn the last kRun - 1 steps of a column into no-ops without a branch.
// A wave reads 64 consecutive floats of one tile row: no bank conflicts.
constexpr int kMaxK = 25, kBW = 64, kBH = 32, kRun = 4, kPad = kRun - 1;
constexpr int kTileW = kBW + kMaxK - 1, kTileH = kBH + kMaxK - 1;  // 88 x 56 floats: 19.3 KB
constexpr int kKfRow = kMaxK + 2 * kPad;

__global__ __launch_bounds__(kThreads) void bsr_blur_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                            const float* __restrict__ kernels, const int* __restrict__ ksizes,
                                                            int C, int H, int W, int K, int tiles_x, int tiles_per_plane) {
  __shared__ float tile[kTileH * kTileW];
  __shared__ float kf[kMaxK * kKfRow];
  const int64_t plane = blockIdx.x / tiles_per_plane;
  const int t = blockIdx.x % tiles_per_plane;
  const int n = (int)(plane / C);
  const int ty0 = (t / tiles_x) * kBH, tx0 = (t % tiles_x) * kBW;
  int ks = ksizes ? ksizes[n] : K;
  if (ks < 1 || ks > K || !(ks & 1)) ks = K;  // (documented: anything but an odd size in 1 .. K means K)
  const int r = ks / 2, off = (K - ks) / 2;
  const float* kp = kernels + (int64_t)n * K * K;
  for (int i = threadIdx.x; i < ks * kKfRow; i += kThreads) {
    const int b = i / kKfRow, a = i % kKfRow - kPad;
    kf[i] = a >= 0 && a < ks ? kp[(off + 2 * r - a) * K + off + 2 * r - b] : 0.f;
  }
  const float* xp = x + plane * H * W;
  const int rows = kBH + 2 * r, cols = kBW + 2 * r;
  for (int i = threadIdx.x; i < rows * cols; i += kThreads) {
    const int row = i / cols, col = i % cols;
    tile[row * kTileW + col] = xp[(int64_t)reflect101(ty0 - r + row, H) * W + reflect101(tx0 - r + col, W)];
  }
  __syncthreads();
  const int lx = threadIdx.x % kBW;
  float* op = out + plane * H * W;
  for (int ly0 = (threadIdx.x / kBW) * kRun; ly0 < kBH; ly0 += (kThreads / kBW) * kRun) {
    if (ty0 + ly0 >= H) break;
    float acc[kRun] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < ks; ++b) {
      const float* kc = kf + b * kKfRow + kPad;
      const float* tp = tile + ly0 * kTileW + lx + b;
      float w1 = 0.f, w2 = 0.f, w3 = 0.f;
      for (int tt = 0; tt < ks + kPad; ++tt) {
        const float w0 = kc[tt], v = tp[tt * kTileW];
        acc[0] = fmaf(w0, v, acc[0]);
        acc[1] = fmaf(w1, v, acc[1]);
        acc[2] = fmaf(w2, v, acc[2]);
        acc[3] = fmaf(w3, v, acc[3]);
        w3 = w2; w2 = w1; w1 = w0;
      }
    }
    if (tx0 + lx < W) {
#pragma unroll
      for (int o = 0; o < kRun; ++o)
        if (ty0 + ly0 + o < H) op[(int64_t)(ty0 + ly0 + o) * W + tx0 + lx] = acc[o];
    }
  }
}

// ---- separable blur and the USM built on it ---------------------------------------------------------------------------------
// out = g (*) g^T (*) src for one 1-D kernel g of k <= 51 taps (by value in the kernel arguments: no device table), the same for
// every plane; true convolution, reflect-101 border.  One block per kBW x kBH tile: source tile + halo in LDS buffer A, row pass
// A -> B (all rows of the halo), column pass B -> registers.
//   EPI_BLUR  src = x, out = the blur.
//   EPI_USM   second launch of the USM: `blurred` = blur(x) of the first launch; src = mask = (|x - blurred| * 255 > threshold),
//             formed while the tile is staged; soft = blur(mask); sharp = clip(x + weight (x - blurred)); out = soft sharp +
//             (1 - soft) x.
constexpr int kSepMaxK = 51, kSepA_W = kBW + kSepMaxK - 1, kSepA_H = kBH + kSepMaxK - 1;  // 114 x 82
struct SepTaps { float w[kSepMaxK]; int k; };
enum { EPI_BLUR = 0, EPI_USM = 1 };

template <int EPI>
__global__ __launch_bounds__(kThreads) void bsr_sep_blur_kernel(const float* __restrict__ x, const float* __restrict__ blurred,
                                                                float* __restrict__ out, SepTaps taps, float weight,
                                                                float threshold, int H, int W, int tiles_x, int tiles_per_plane) {
  __shared__ float A[kSepA_H * kSepA_W];  // 36.5 KB
  __shared__ float Bf[kSepA_H * kBW];     // 20.5 KB
  __shared__ float g[kSepMaxK];
  const int64_t plane = blockIdx.x / tiles_per_plane;
  const int t = blockIdx.x % tiles_per_plane;
  const int ty0 = (t / tiles_x) * kBH, tx0 = (t % tiles_x) * kBW;
  const int k = taps.k, r = k / 2;
  if (threadIdx.x < k) g[threadIdx.x] = taps.w[threadIdx.x];
  const float* xp = x + plane * H * W;
  const float* bp = EPI == EPI_USM ? blurred + plane * H * W : nullptr;
  const int rows = kBH + 2 * r, cols = kBW + 2 * r;
  for (int i = threadIdx.x; i < rows * cols; i += kThreads) {
    const int row = i / cols, col = i % cols;
    const int64_t gi = (int64_t)reflect101(ty0 - r + row, H) * W + reflect101(tx0 - r + col, W);
    float v = xp[gi];
    if constexpr (EPI == EPI_USM) v = fabsf(v - bp[gi]) * 255.f > threshold ? 1.f : 0.f;
    A[row * kSepA_W + col] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x % kBW, lq = threadIdx.x / kBW;
  for (int row = lq; row < rows; row += kThreads / kBW) {
    const float* ap = A + row * kSepA_W + lx + 2 * r;
    float acc = 0.f;
    for (int j = 0; j < k; ++j) acc = fmaf(g[j], ap[-j], acc);
    Bf[row * kBW + lx] = acc;
  }
  __syncthreads();
  if (tx0 + lx >= W) return;
  for (int ly = lq; ly < kBH && ty0 + ly < H; ly += kThreads / kBW) {
    const float* bq = Bf + (ly + 2 * r) * kBW + lx;
    float acc = 0.f;
    for (int i = 0; i < k; ++i) acc = fmaf(g[i], bq[-i * kBW], acc);
    const int64_t gi = (int64_t)(ty0 + ly) * W + tx0 + lx;
    if constexpr (EPI == EPI_USM) {
      const float v = xp[gi], sharp = clip01(fmaf(weight, v - bp[gi], v));
      acc = fmaf(acc, sharp, (1.f - acc) * v);
    }
    out[plane * H * W + gi] = acc;
  }
}

// ---- resize -------------------------------------------------------------------------------------------------------------
// Output sample o of an axis in -> out sits at source coordinate (o + 1/2) in / out - 1/2 = num / den with num = (2 o + 1) in -
// out, den = 2 out: floor and fraction are formed in integers, so a weight carries one fp32 rounding and in == out is the
// identity bit for bit.  mode 1 bilinear (2 taps), 2 bicubic (4 taps of the cubic convolution kernel with a = -0.75), 3 area:
// where the axis shrinks, the mean over [o in / out, (o + 1) in / out) with the partial overlaps of the end pixels - overlap
// lengths are integers in units of 1 / out - and bilinear where it does not.  Taps outside the image take the border pixel.
struct Axis {
  int s0, cnt, in, out, o;
  bool box;
  float w0, w1, w2, w3;
};
__device__ __forceinline__ Axis make_axis(int mode, int o, int in, int out) {
  Axis a;
  a.in = in; a.out = out; a.o = o;
  a.box = mode == 3 && in > out;
  a.w0 = a.w1 = a.w2 = a.w3 = 0.f;
  if (a.box) {
    a.s0 = (int)((int64_t)o * in / out);
    a.cnt = (int)((((int64_t)o + 1) * in + out - 1) / out) - a.s0;
    return a;
  }
  const int64_t num = (2 * (int64_t)o + 1) * in - out, den = 2 * (int64_t)out;
  const int64_t q = num >= 0 ? num / den : -((-num + den - 1) / den);
  const float f = (float)(num - q * den) / (float)den;
  if (mode == 2) {
    constexpr float a_ = -0.75f;
    const float g = 1.f - f;
    a.w0 = ((a_ * (f + 1.f) - 5.f * a_) * (f + 1.f) + 8.f * a_) * (f + 1.f) - 4.f * a_;
    a.w1 = ((a_ + 2.f) * f - (a_ + 3.f)) * f * f + 1.f;
    a.w2 = ((a_ + 2.f) * g - (a_ + 3.f)) * g * g + 1.f;
    a.w3 = 1.f - a.w0 - a.w1 - a.w2;
    a.s0 = (int)q - 1;
    a.cnt = 4;
  } else {
    a.w0 = 1.f - f;
    a.w1 = f;
    a.s0 = (int)q;
    a.cnt = 2;
  }
  return a;
}
__device__ __forceinline__ float axis_weight(const Axis& a, int j) {
  if (a.box) {
    const int64_t lo = max((int64_t)a.o * a.in, (int64_t)(a.s0 + j) * a.out);
    const int64_t hi = min(((int64_t)a.o + 1) * a.in, (int64_t)(a.s0 + j + 1) * a.out);
    return (float)(hi - lo) / (float)a.in;
  }
  return j == 0 ? a.w0 : j == 1 ? a.w1 : j == 2 ? a.w2 : a.w3;
}
__device__ __forceinline__ int axis_index(const Axis& a, int j) { return min(max(a.s0 + j, 0), a.in - 1); }

__global__ __launch_bounds__(kThreads) void bsr_resize_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              float* __restrict__ out_q, int64_t planes, int H, int W, int H2,
                                                              int W2, int mode) {
  const int64_t total = planes * H2 * W2;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int ox = (int)(i % W2), oy = (int)(i / W2 % H2);
    const float* xp = x + (i / ((int64_t)H2 * W2)) * H * W;
    const Axis ay = make_axis(mode, oy, H, H2), ax = make_axis(mode, ox, W, W2);
    float acc = 0.f;
    for (int jy = 0; jy < ay.cnt; ++jy) {
      const float* row = xp + (int64_t)axis_index(ay, jy) * W;
      float racc = 0.f;
      for (int jx = 0; jx < ax.cnt; ++jx) racc = fmaf(axis_weight(ax, jx), row[axis_index(ax, jx)], racc);
      acc = fmaf(axis_weight(ay, jy), racc, acc);
    }
    acc = clip01(acc);
    out[i] = acc;
    if (out_q) out_q[i] = rintf(acc * 255.f) / 255.f;
  }
}

// ---- noise ----------------------------------------------------------------------------------------------------------------
// One thread per pixel of one image, all its bands (the correlated branch mixes them).  mode[n] = (kind, branch), par[n] =
// (sigma, A[3][3]): see drs_bsr_noise in include/drs_hip.h.  kind 0 writes nothing: the image keeps its bits.
enum { NOISE_OFF = 0, NOISE_ADD = 1, NOISE_SPECKLE = 2, NOISE_POISSON = 3, NOISE_POISSON_GRAY = 4 };
enum { BRANCH_BAND = 0, BRANCH_GRAY = 1, BRANCH_CORR = 2 };
constexpr int kNoisePar = 10;

__global__ __launch_bounds__(kThreads) void bsr_noise_kernel(float* __restrict__ x, const float* __restrict__ z,
                                                             const float* __restrict__ aux, const int* __restrict__ mode,
                                                             const float* __restrict__ par, int N, int C, int64_t hw) {
  const int64_t total = (int64_t)N * hw;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int n = (int)(i / hw);
    const int64_t p = i % hw;
    const int kind = mode[2 * n];
    int branch = mode[2 * n + 1];
    if (kind < NOISE_ADD || kind > NOISE_POISSON_GRAY || (kind == NOISE_POISSON_GRAY && !aux)) continue;
    if (branch == BRANCH_CORR && C != 3) branch = BRANCH_BAND;
    const float* pr = par + (int64_t)n * kNoisePar;
    const float sigma = pr[0];
    float* xp = x + (int64_t)n * C * hw + p;
    const float* zp = z + (int64_t)n * C * hw + p;
    if (kind == NOISE_POISSON) {  // z = the Poisson draw at rate q(x) sigma: x = z / sigma
      for (int c = 0; c < C; ++c) xp[c * hw] = clip01(zp[c * hw] / sigma);
    } else if (kind == NOISE_POISSON_GRAY) {  // z[0] = the draw at rate aux = gray(q(x)) sigma: x = q(x) + (z[0] - aux) / sigma
      const float d = (zp[0] - aux[(int64_t)n * hw + p]) / sigma;
      for (int c = 0; c < C; ++c) xp[c * hw] = clip01(rintf(clip01(xp[c * hw]) * 255.f) / 255.f + d);
    } else {
      float z0 = 0.f, z1 = 0.f, z2 = 0.f;
      if (branch == BRANCH_CORR) { z0 = zp[0]; z1 = zp[hw]; z2 = zp[2 * hw]; }
      const float gray = sigma * zp[0];
      for (int c = 0; c < C; ++c) {
        float nv;
        if (branch == BRANCH_CORR) nv = fmaf(pr[1 + 3 * c], z0, fmaf(pr[2 + 3 * c], z1, pr[3 + 3 * c] * z2));
        else nv = branch == BRANCH_GRAY ? gray : sigma * zp[c * hw];
        const float v = xp[c * hw];
        xp[c * hw] = kind == NOISE_ADD ? clip01(v + nv) : clip01(fmaf(clip01(v), nv, clip01(v)));
      }
    }
  }
}

// ---- JPEG round trip ----------------------------------------------------------------------------------------------------------
// DESIGN.md section 19 holds the definition; the integer DCT: C[u][x] = round(2^14 (c_u / 2) cos((2 x + 1) u pi / 16)),
//   forward   t[y][v] = (sum_x C[v][x] s[y][x] + 2^8) >> 9,   F[u][v] = sum_y C[u][y] t[y][v]        (F = 2^19 x the DCT)
//   quantise  q = sign(F) ((|F| + Q 2^18) / (Q 2^19))   (integer division: the nearest integer, halves away from zero), D = q Q
//   inverse   t[y][v] = (sum_u C[u][y] D[u][v] + 2^8) >> 9,   s[y][x] = (sum_v C[v][x] t[y][v] + 2^18) >> 19
// with 64-bit sums (every one of them also fits 32 bits for 8-bit samples: |row sum of C| <= 46344), >> the arithmetic shift.
__device__ const int kDct[64] = {
    5793,  5793,  5793,  5793,  5793,  5793,  5793,  5793,
    8035,  6811,  4551,  1598, -1598, -4551, -6811, -8035,
    7568,  3135, -3135, -7568, -7568, -3135,  3135,  7568,
    6811, -1598, -8035, -4551,  4551,  8035,  1598, -6811,
    5793, -5793, -5793,  5793,  5793, -5793, -5793,  5793,
    4551, -8035,  1598,  6811, -6811, -1598,  8035, -4551,
    3135, -7568,  7568, -3135, -3135,  7568, -7568,  3135,
    1598, -4551,  6811, -8035,  8035, -6811,  4551, -1598,
};
// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row by row
__device__ const unsigned char kQuantBase[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__device__ __forceinline__ int q8(float v) { return (int)rintf(clip01(v) * 255.f); }

// grid (MCUs across, MCUs down, N), 256 threads = the 16 x 16 pixels of the MCU.  Writes the DECODED planes: yp (N, Hp, Wp),
// cbp / crp (N, Hp / 2, Wp / 2) uint8, Hp and Wp the size rounded up to 16 (the edge pixel repeated).
__global__ __launch_bounds__(kThreads) void bsr_jpeg_blocks_kernel(const float* __restrict__ x, const int* __restrict__ quality,
                                                                   unsigned char* __restrict__ yp, unsigned char* __restrict__ cbp,
                                                                   unsigned char* __restrict__ crp, int H, int W, int Hp, int Wp) {
  __shared__ int cm[64];
  __shared__ int blk[6][64];
  __shared__ int tmp[6][64];
  __shared__ int cfull[2][256];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int n = blockIdx.z, x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  if (t < 64) cm[t] = kDct[t];
  const int64_t hw = (int64_t)H * W;
  const float* p = x + (int64_t)n * 3 * hw + (int64_t)min(y0 + ty, H - 1) * W + min(x0 + tx, W - 1);
  const int R = q8(p[0]), G = q8(p[hw]), B = q8(p[2 * hw]);
  blk[(ty >> 3) * 2 + (tx >> 3)][(ty & 7) * 8 + (tx & 7)] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
  cfull[0][t] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
  cfull[1][t] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
  __syncthreads();
  if (t < 128) {
    const int c = t >> 6, i = t & 63, cy = i >> 3, cx = i & 7;
    const int* f = cfull[c] + 32 * cy + 2 * cx;
    blk[4 + c][i] = ((f[0] + f[1] + f[16] + f[17] + 1 + (cx & 1)) >> 2) - 128;
  }
  __syncthreads();
  int qv = quality[n];
  qv = min(max(qv, 1), 100);
  const int scale = qv < 50 ? 5000 / qv : 200 - 2 * qv;
  for (int i = t; i < 384; i += kThreads) {  // forward, rows
    const int b = i >> 6, y = (i >> 3) & 7, v = i & 7;
    long long acc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (long long)cm[v * 8 + j] * blk[b][y * 8 + j];
    tmp[b][y * 8 + v] = (int)((acc + 256) >> 9);
  }
  __syncthreads();
  for (int i = t; i < 384; i += kThreads) {  // forward, columns; quantise; dequantise
    const int b = i >> 6, u = (i >> 3) & 7, v = i & 7;
    long long acc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (long long)cm[u * 8 + j] * tmp[b][j * 8 + v];
    const long long Q = min(max(((int)kQuantBase[b >= 4][i & 63] * scale + 50) / 100, 1), 255);
    const long long mag = ((acc < 0 ? -acc : acc) + (Q << 18)) / (Q << 19);
    blk[b][i & 63] = (int)((acc < 0 ? -mag : mag) * Q);
  }
  __syncthreads();
  for (int i = t; i < 384; i += kThreads) {  // inverse, columns
    const int b = i >> 6, y = (i >> 3) & 7, v = i & 7;
    long long acc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (long long)cm[j * 8 + y] * blk[b][j * 8 + v];
    tmp[b][y * 8 + v] = (int)((acc + 256) >> 9);
  }
  __syncthreads();
  for (int i = t; i < 384; i += kThreads) {  // inverse, rows; level shift; clamp
    const int b = i >> 6, y = (i >> 3) & 7, xx = i & 7;
    long long acc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (long long)cm[j * 8 + xx] * tmp[b][y * 8 + j];
    const int s = min(max((int)((acc + (1 << 18)) >> 19) + 128, 0), 255);
    if (b < 4) {
      yp[((int64_t)n * Hp + y0 + (b >> 1) * 8 + y) * Wp + x0 + (b & 1) * 8 + xx] = (unsigned char)s;
    } else {
      (b == 4 ? cbp : crp)[((int64_t)n * (Hp / 2) + y0 / 2 + y) * (Wp / 2) + x0 / 2 + xx] = (unsigned char)s;
    }
  }
}

// One thread per output pixel: chroma up-sampled with the triangle filter (3/4 of the nearer, 1/4 of the further sample, first
// down, then across; neighbours past the edge of the padded chroma plane are the edge sample), then YCbCr -> RGB.
__global__ __launch_bounds__(kThreads) void bsr_jpeg_color_kernel(const unsigned char* __restrict__ yp,
                                                                  const unsigned char* __restrict__ cbp,
                                                                  const unsigned char* __restrict__ crp, float* __restrict__ out,
                                                                  int N, int H, int W, int Hp, int Wp) {
  const int64_t hw = (int64_t)H * W, total = (int64_t)N * hw;
  const int Hc = Hp / 2, Wc = Wp / 2;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int n = (int)(i / hw), y = (int)(i % hw / W), xx = (int)(i % W);
    const int cy = y >> 1, cx = xx >> 1;
    const int yn = (y & 1) ? min(cy + 1, Hc - 1) : max(cy - 1, 0), xn = (xx & 1) ? min(cx + 1, Wc - 1) : max(cx - 1, 0);
    const int bias = (xx & 1) ? 7 : 8;
    int ch[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const unsigned char* q = (c ? crp : cbp) + (int64_t)n * Hc * Wc;
      const int near_ = 3 * q[cy * Wc + cx] + q[yn * Wc + cx], far_ = 3 * q[cy * Wc + xn] + q[yn * Wc + xn];
      ch[c] = ((3 * near_ + far_ + bias) >> 4) - 128;
    }
    const int Y = yp[((int64_t)n * Hp + y) * Wp + xx];
    const int R = Y + ((91881 * ch[1] + 32768) >> 16);
    const int G = Y + ((-22554 * ch[0] - 46802 * ch[1] + 32768) >> 16);
    const int B = Y + ((116130 * ch[0] + 32768) >> 16);
    float* op = out + (int64_t)n * 3 * hw + i % hw;
    op[0] = (float)min(max(R, 0), 255) / 255.f;
    op[hw] = (float)min(max(G, 0), 255) / 255.f;
    op[2 * hw] = (float)min(max(B, 0), 255) / 255.f;
  }
}

// ---- argument checks ------------------------------------------------------------------------------------------------------------
bool overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bbytes && y < x + abytes;
}
int check_shape(const char* what, int N, int C, int H, int W) {
  DRS_REQUIRE(N >= 1 && C >= 1 && C <= kMaxBands && H >= 1 && W >= 1, DRS_ERR_SHAPE, "%s: N=%d C=%d H=%d W=%d (1 <= C <= %d)", what, N,
              C, H, W, kMaxBands);
  return DRS_OK;
}
int tile_grid(const char* what, int N, int C, int H, int W, int* tiles_x, int* tiles_per_plane, unsigned* blocks) {
  *tiles_x = drs_cdiv(W, kBW);
  const int64_t tpp = (int64_t)*tiles_x * drs_cdiv(H, kBH), b = tpp * N * C;
  DRS_REQUIRE(b <= INT32_MAX, DRS_ERR_SHAPE, "%s: N=%d C=%d H=%d W=%d need more tiles than one launch holds", what, N, C, H, W);
  *tiles_per_plane = (int)tpp;
  *blocks = (unsigned)b;
  return DRS_OK;
}
int make_taps(const char* what, const float* taps, int k, SepTaps* t) {
  DRS_REQUIRE(taps, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(k >= 1 && k <= kSepMaxK && (k & 1), DRS_ERR_SHAPE, "%s: k=%d must be odd and in 1 .. %d", what, k, kSepMaxK);
  for (int i = 0; i < kSepMaxK; ++i) t->w[i] = i < k ? taps[i] : 0.f;
  t->k = k;
  return DRS_OK;
}
size_t jpeg_pad(int v) { return ((size_t)v + 15) / 16 * 16; }

}  // namespace

extern "C" DRS_API int drs_bsr_blur(const float* x, float* out, const float* kernels, const int* ksizes, int N, int C, int H, int W,
                                    int K, drs_stream_t stream) {
  DRS_REQUIRE(x && out && kernels, DRS_ERR_ARG, "bsr_blur: null pointer");
  if (const int rc = check_shape("bsr_blur", N, C, H, W)) return rc;
  DRS_REQUIRE(K >= 1 && K <= kMaxK && (K & 1), DRS_ERR_SHAPE, "bsr_blur: K=%d must be odd and in 1 .. %d", K, kMaxK);
  const size_t bytes = (size_t)N * C * H * W * sizeof(float);
  DRS_REQUIRE(!overlap(out, bytes, x, bytes), DRS_ERR_ARG, "bsr_blur: out overlaps x (a tile reads its neighbours: in place is a race)");
  int tiles_x, tpp;
  unsigned blocks;
  if (const int rc = tile_grid("bsr_blur", N, C, H, W, &tiles_x, &tpp, &blocks)) return rc;
  DRS_LAUNCH(bsr_blur_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, x, out, kernels, ksizes, C, H, W, K, tiles_x, tpp);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API int drs_bsr_blur_sep(const float* x, float* out, const float* taps, int k, int N, int C, int H, int W,
                                        drs_stream_t stream) {
  DRS_REQUIRE(x && out, DRS_ERR_ARG, "bsr_blur_sep: null pointer");
  if (const int rc = check_shape("bsr_blur_sep", N, C, H, W)) return rc;
  SepTaps t;
  if (const int rc = make_taps("bsr_blur_sep", taps, k, &t)) return rc;
  const size_t bytes = (size_t)N * C * H * W * sizeof(float);
  DRS_REQUIRE(!overlap(out, bytes, x, bytes), DRS_ERR_ARG, "bsr_blur_sep: out overlaps x (a tile reads its neighbours)");
  int tiles_x, tpp;
  unsigned blocks;
  if (const int rc = tile_grid("bsr_blur_sep", N, C, H, W, &tiles_x, &tpp, &blocks)) return rc;
  DRS_LAUNCH(bsr_sep_blur_kernel<EPI_BLUR>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, x, (const float*)nullptr, out, t,
             0.f, 0.f, H, W, tiles_x, tpp);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API int drs_bsr_sharpen(const float* x, float* out, float* scratch, const float* taps, int k, float weight,
                                       float threshold, int N, int C, int H, int W, drs_stream_t stream) {
  DRS_REQUIRE(x && out && scratch, DRS_ERR_ARG, "bsr_sharpen: null pointer");
  if (const int rc = check_shape("bsr_sharpen", N, C, H, W)) return rc;
  SepTaps t;
  if (const int rc = make_taps("bsr_sharpen", taps, k, &t)) return rc;
  const size_t bytes = (size_t)N * C * H * W * sizeof(float);
  DRS_REQUIRE(!overlap(out, bytes, x, bytes) && !overlap(scratch, bytes, x, bytes) && !overlap(scratch, bytes, out, bytes),
              DRS_ERR_ARG, "bsr_sharpen: x, out and scratch must not overlap");
  int tiles_x, tpp;
  unsigned blocks;
  if (const int rc = tile_grid("bsr_sharpen", N, C, H, W, &tiles_x, &tpp, &blocks)) return rc;
  hipStream_t s = (hipStream_t)stream;
  DRS_LAUNCH(bsr_sep_blur_kernel<EPI_BLUR>, dim3(blocks), dim3(kThreads), 0, s, x, (const float*)nullptr, scratch, t, 0.f, 0.f, H, W,
             tiles_x, tpp);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(bsr_sep_blur_kernel<EPI_USM>, dim3(blocks), dim3(kThreads), 0, s, x, (const float*)scratch, out, t, weight, threshold, H,
             W, tiles_x, tpp);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API int drs_bsr_resize(const float* x, float* out, float* out_q, int N, int C, int H, int W, int H2, int W2, int mode,
                                      drs_stream_t stream) {
  DRS_REQUIRE(x && out, DRS_ERR_ARG, "bsr_resize: null pointer");
  if (const int rc = check_shape("bsr_resize", N, C, H, W)) return rc;
  DRS_REQUIRE(H2 >= 1 && W2 >= 1, DRS_ERR_SHAPE, "bsr_resize: output size %d x %d", H2, W2);
  DRS_REQUIRE(mode >= 1 && mode <= 3, DRS_ERR_ARG, "bsr_resize: mode=%d (1 bilinear, 2 bicubic, 3 area)", mode);
  const size_t in_bytes = (size_t)N * C * H * W * sizeof(float), out_bytes = (size_t)N * C * H2 * W2 * sizeof(float);
  DRS_REQUIRE(!overlap(out, out_bytes, x, in_bytes) && (!out_q || (!overlap(out_q, out_bytes, x, in_bytes) &&
                                                                   !overlap(out_q, out_bytes, out, out_bytes))),
              DRS_ERR_ARG, "bsr_resize: x, out and out_q must not overlap");
  DRS_LAUNCH(bsr_resize_kernel, dim3(ew_blocks((int64_t)N * C * H2 * W2)), dim3(kThreads), 0, (hipStream_t)stream, x, out, out_q,
             (int64_t)N * C, H, W, H2, W2, mode);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API int drs_bsr_noise(float* x, const float* z, const float* aux, const int* mode, const float* par, int N, int C,
                                     int H, int W, drs_stream_t stream) {
  DRS_REQUIRE(x && z && mode && par, DRS_ERR_ARG, "bsr_noise: null pointer");
  if (const int rc = check_shape("bsr_noise", N, C, H, W)) return rc;
  const size_t bytes = (size_t)N * C * H * W * sizeof(float);
  DRS_REQUIRE(!overlap(x, bytes, z, bytes), DRS_ERR_ARG, "bsr_noise: z overlaps x");
  DRS_LAUNCH(bsr_noise_kernel, dim3(ew_blocks((int64_t)N * H * W)), dim3(kThreads), 0, (hipStream_t)stream, x, z, aux, mode, par, N, C,
             (int64_t)H * W);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API size_t drs_bsr_jpeg_scratch_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return (size_t)N * jpeg_pad(H) * jpeg_pad(W) * 3 / 2;
}

extern "C" DRS_API int drs_bsr_jpeg(const float* x, float* out, const int* quality, int N, int H, int W, void* scratch,
                                    size_t scratch_bytes, drs_stream_t stream) {
  DRS_REQUIRE(x && out && quality && scratch, DRS_ERR_ARG, "bsr_jpeg: null pointer");
  DRS_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20), DRS_ERR_SHAPE, "bsr_jpeg: N=%d H=%d W=%d",
              N, H, W);
  const size_t need = drs_bsr_jpeg_scratch_bytes(N, H, W);
  DRS_REQUIRE(scratch_bytes >= need, DRS_ERR_WORKSPACE, "bsr_jpeg: scratch of %zu bytes, %zu needed", scratch_bytes, need);
  const int Hp = (int)jpeg_pad(H), Wp = (int)jpeg_pad(W);
  DRS_REQUIRE(Hp / 16 <= 65535, DRS_ERR_SHAPE, "bsr_jpeg: H=%d is more MCU rows than one launch holds", H);
  unsigned char* yp = (unsigned char*)scratch;
  unsigned char* cbp = yp + (size_t)N * Hp * Wp;
  unsigned char* crp = cbp + (size_t)N * Hp * Wp / 4;
  hipStream_t s = (hipStream_t)stream;
  DRS_LAUNCH(bsr_jpeg_blocks_kernel, dim3(Wp / 16, Hp / 16, N), dim3(kThreads), 0, s, x, quality, yp, cbp, crp, H, W, Hp, Wp);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(bsr_jpeg_color_kernel, dim3(ew_blocks((int64_t)N * H * W)), dim3(kThreads), 0, s, (const unsigned char*)yp,
             (const unsigned char*)cbp, (const unsigned char*)crp, out, N, H, W, Hp, Wp);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
