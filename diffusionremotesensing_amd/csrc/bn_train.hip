// Train-mode BatchNorm over channels-last activations (reference nn.BatchNorm2d in training: batch mean / biased
// variance over (N,H,W), running statistics updated with momentum 0.1 and the UNBIASED variance; eps 1e-5).
// In train mode the normalisation cannot be folded into the preceding convolution, so the plan runs
//   conv (raw weights) -> Z  ->  bn_stats(Z)  ->  bn_finalize  ->  bn_apply(Z) with the block's activation / adds.
// Its backward (bn_bwd_reduce -> bn_bwd_finish -> bn_bwd_apply) follows below: same partial-row layout, same row buffer.
// Plans with DRS_PLAN_FROZEN_BN normalise with the running statistics instead and never write them:
//   conv -> Z  ->  bn_frozen_stats (C threads)  ->  bn_apply(Z),   backward  bn_bwd_frozen (one pass)  ->  bn_bwd_finish.
#include "conv_epilogue.h"  // drs_sp_split4
#include "drs_common.h"
#include "train_reduce.h"

// Per-channel sum and sum of squares.  Thread = (pixel row in block, group of 4 channels): float4 loads, fp32 partials
// over a few thousand elements per thread, LDS reduction over the block, then the block's 2 x C fp64 partial sums go to
// ITS row of `partials` (gridDim.x rows); bn_finalize_kernel adds the rows up.  (Atomics onto 2 x C shared addresses
// serialise: 512 blocks x ~90 ns = 46 us per launch at ANY tensor size.)
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ z, long long npix, int C, int cs,
                                                       int co, double* __restrict__ partials) {
  __shared__ float red[2][256][4];
  const int c4n = C >> 2;             // channel groups
  const int rows = 256 / c4n;         // pixel rows handled concurrently by the block (C <= 1024)
  const int cg = threadIdx.x % c4n, row = threadIdx.x / c4n;
  float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    // four independent 16-byte loads in flight per thread (with one, 512 blocks keep 2 MB in flight: 1.0 - 1.6 TB/s measured)
    const long long stride = (long long)gridDim.x * rows;
    const float* base = z + co + cg * 4;
    long long p = (long long)blockIdx.x * rows + row;
    for (; p + 3 * stride < npix; p += 4 * stride) {
      const float4 v0 = *reinterpret_cast<const float4*>(base + p * cs);
      const float4 v1 = *reinterpret_cast<const float4*>(base + (p + stride) * cs);
      const float4 v2 = *reinterpret_cast<const float4*>(base + (p + 2 * stride) * cs);
      const float4 v3 = *reinterpret_cast<const float4*>(base + (p + 3 * stride) * cs);
      s[0] += (v0.x + v1.x) + (v2.x + v3.x); s[1] += (v0.y + v1.y) + (v2.y + v3.y);
      s[2] += (v0.z + v1.z) + (v2.z + v3.z); s[3] += (v0.w + v1.w) + (v2.w + v3.w);
      q[0] += (v0.x * v0.x + v1.x * v1.x) + (v2.x * v2.x + v3.x * v3.x);
      q[1] += (v0.y * v0.y + v1.y * v1.y) + (v2.y * v2.y + v3.y * v3.y);
      q[2] += (v0.z * v0.z + v1.z * v1.z) + (v2.z * v2.z + v3.z * v3.z);
      q[3] += (v0.w * v0.w + v1.w * v1.w) + (v2.w * v2.w + v3.w * v3.w);
    }
    for (; p < npix; p += stride) {
      const float4 v = *reinterpret_cast<const float4*>(base + p * cs);
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
      q[0] += v.x * v.x; q[1] += v.y * v.y; q[2] += v.z * v.z; q[3] += v.w * v.w;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[0][threadIdx.x][j] = s[j]; red[1][threadIdx.x][j] = q[j]; }
  __syncthreads();
  if (threadIdx.x < c4n) {
    double ds[4] = {0, 0, 0, 0}, dq[4] = {0, 0, 0, 0};
    for (int r = 0; r < rows; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ds[j] += (double)red[0][r * c4n + threadIdx.x][j];
        dq[j] += (double)red[1][r * c4n + threadIdx.x][j];
      }
    double* row = partials + (size_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      row[threadIdx.x * 4 + j] = ds[j];
      row[C + threadIdx.x * 4 + j] = dq[j];
    }
  }
}

// Adds up the `nrows` partial rows and finalises: block = 64 channels x 4 row groups.
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const double* __restrict__ partials, int nrows, long long npix, int C,
                                                          float eps, float momentum, float* __restrict__ mean,
                                                          float* __restrict__ rstd, float* __restrict__ running_mean,
                                                          float* __restrict__ running_var) {
  __shared__ double red[2][16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s = 0, q = 0;
  if (c < C)
#pragma unroll 8
    for (int r = rg; r < nrows; r += 16) {
      s += partials[(size_t)r * 2 * C + c];
      q += partials[(size_t)r * 2 * C + C + c];
    }
  red[0][rg][cl] = s;
  red[1][rg][cl] = q;
  __syncthreads();
  if (rg != 0 || c >= C) return;
  s = sum16(red[0], cl);
  q = sum16(red[1], cl);
  const double m = s / (double)npix;
  double var = q / (double)npix - m * m;  // biased
  if (var < 0) var = 0;
  mean[c] = (float)m;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = npix > 1 ? var * (double)npix / (double)(npix - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// y = relu_post( relu_pre( (z - mean) * rstd * gamma + beta ) + post_add[n][c] + res ), channels-last slices.
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, int z_cs, int z_co,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ post_add, int post_cs,
                                                       const float* __restrict__ res, int res_cs, int res_co,
                                                       float* __restrict__ out, int out_cs, int out_co, long long npix,
                                                       long long pix_per_image, int C, int relu_pre, int relu_post) {
  const int c4n = C >> 2;
  const long long total = npix * c4n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % c4n);
    const long long p = i / c4n;
    const int c = cg * 4;
    const float4 v = *reinterpret_cast<const float4*>(z + p * z_cs + z_co + c);
    const float4 m = *reinterpret_cast<const float4*>(mean + c), r = *reinterpret_cast<const float4*>(rstd + c);
    const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
    float y[4] = {(v.x - m.x) * r.x * g.x + b.x, (v.y - m.y) * r.y * g.y + b.y, (v.z - m.z) * r.z * g.z + b.z,
                  (v.w - m.w) * r.w * g.w + b.w};
    if (relu_pre)
      for (int j = 0; j < 4; ++j) y[j] = drs_maxf(y[j], 0.f);
    if (post_add) {
      const float4 a = *reinterpret_cast<const float4*>(post_add + (p / pix_per_image) * post_cs + c);
      y[0] += a.x; y[1] += a.y; y[2] += a.z; y[3] += a.w;
    }
    if (res) {
      const float4 a = *reinterpret_cast<const float4*>(res + p * res_cs + res_co + c);
      y[0] += a.x; y[1] += a.y; y[2] += a.z; y[3] += a.w;
    }
    if (relu_post)
      for (int j = 0; j < 4; ++j) y[j] = drs_maxf(y[j], 0.f);
    *reinterpret_cast<float4*>(out + p * out_cs + out_co + c) = make_float4(y[0], y[1], y[2], y[3]);
  }
}

int drs_launch_bn_train(const float* z, int z_cs, int z_co, long long npix, long long pix_per_image, int C,
                        const float* gamma, const float* beta, float* running_mean, float* running_var, float eps,
                        float momentum, double* sums_scratch, float* mean, float* rstd, const float* post_add,
                        int post_cs, const float* res, int res_cs, int res_co, float* out, int out_cs, int out_co,
                        int relu_pre, int relu_post, hipStream_t s) {
  DRS_REQUIRE(C % 4 == 0 && C <= 1024, DRS_ERR_SHAPE, "bn_train: C=%d", C);
  DRS_REQUIRE((z_cs & 3) == 0 && (z_co & 3) == 0 && (out_cs & 3) == 0 && (out_co & 3) == 0, DRS_ERR_SHAPE,
              "bn_train: unaligned channel slices");
  // (sums_scratch: DRS_RED_BLOCKS rows of 2 x C fp64 partial sums, rewritten by every call: calls must be stream-ordered)
  const int rows = 256 / (C >> 2);
  const unsigned blocks = grid1d(npix, rows, DRS_RED_BLOCKS);
  DRS_LAUNCH(bn_stats_kernel, dim3(blocks), dim3(256), 0, s, z, npix, C, z_cs, z_co, sums_scratch);
  DRS_LAUNCH(bn_finalize_kernel, dim3((C + 63) / 64), dim3(1024), 0, s, sums_scratch, (int)blocks, npix, C, eps, momentum, mean,
                     rstd, running_mean, running_var);
  DRS_LAUNCH(bn_apply_kernel, dim3(grid1d(npix * (C >> 2), 256, 8192)), dim3(256), 0, s, z, z_cs, z_co, mean, rstd, gamma, beta,
                     post_add, post_cs, res, res_cs, res_co, out, out_cs, out_co, npix, pix_per_image, C, relu_pre, relu_post);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// Frozen statistics (DRS_PLAN_FROZEN_BN: the reference modules under model.train() with every BatchNorm2d in .eval()):
// y = (z - running_mean) / sqrt(running_var + eps) * gamma + beta.  No pass over Z: one thread per channel copies the
// running statistics into the layer's mean | rstd slot (rstd rounded like bn_finalize_kernel's), which bn_apply_kernel, the
// backward and its ReLU-mask recomputation read as they read batch statistics.  The running statistics are only read.
__global__ __launch_bounds__(256) void bn_frozen_stats_kernel(const float* __restrict__ running_mean,
                                                              const float* __restrict__ running_var, float eps, int C,
                                                              float* __restrict__ mean, float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = running_mean[c];
  rstd[c] = (float)(1.0 / sqrt((double)running_var[c] + (double)eps));
}

int drs_launch_bn_frozen(const float* z, int z_cs, int z_co, long long npix, long long pix_per_image, int C,
                         const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                         float eps, float* mean, float* rstd, const float* post_add, int post_cs, const float* res,
                         int res_cs, int res_co, float* out, int out_cs, int out_co, int relu_pre, int relu_post,
                         hipStream_t s) {
  DRS_REQUIRE(C % 4 == 0 && C <= 1024, DRS_ERR_SHAPE, "bn_frozen: C=%d", C);
  DRS_REQUIRE((z_cs & 3) == 0 && (z_co & 3) == 0 && (out_cs & 3) == 0 && (out_co & 3) == 0, DRS_ERR_SHAPE,
              "bn_frozen: unaligned channel slices");
  DRS_LAUNCH(bn_frozen_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, s, running_mean, running_var, eps, C, mean, rstd);
  DRS_LAUNCH(bn_apply_kernel, dim3(grid1d(npix * (C >> 2), 256, 8192)), dim3(256), 0, s, z, z_cs, z_co, mean, rstd, gamma, beta,
                     post_add, post_cs, res, res_cs, res_co, out, out_cs, out_co, npix, pix_per_image, C, relu_pre, relu_post);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// BatchNorm backward (training statistics).  g = gradient w.r.t. the BatchNorm output (after the optional ReLU mask
// that sat directly on it: relu_pre), zhat = (z - mean) * rstd:
//   dbeta = sum g, dgamma = sum g*zhat, dz = gamma*rstd*(g - dbeta/M - zhat*dgamma/M).
// Pass 1 reduces (fp64 atomics), pass 2 writes dz IN PLACE over z.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 drs_mask4(const float4& g, const float4& y) {  // g * (y > 0)
  return make_float4(y.x > 0.f ? g.x : 0.f, y.y > 0.f ? g.y : 0.f, y.z > 0.f ? g.z : 0.f, y.w > 0.f ? g.w : 0.f);
}
// thread = (pixel row in block, group of 4 channels): 16-byte loads, two pixels in flight per thread
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ g, int g_cs, int g_co,
                                                            const float* __restrict__ z, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int relu_pre, int C,
                                                            long long npix, double* __restrict__ partials,
                                                            const float* __restrict__ mask_y, int my_cs, int my_co) {
  // mask_y: optional output of a ReLU that sat on top of g's tensor (g is taken as g * (mask_y > 0)): the residual block's
  // final ReLU, whose masking pass over gR this replaces
  __shared__ float red[2][256][4];
  const int c4n = C >> 2;
  const int rows = 256 / c4n;
  const int cg = threadIdx.x % c4n, row = threadIdx.x / c4n;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    const int c = cg * 4;
    const float4 m = *reinterpret_cast<const float4*>(mean + c), r = *reinterpret_cast<const float4*>(rstd + c);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
    const float mm[4] = {m.x, m.y, m.z, m.w}, rr[4] = {r.x, r.y, r.z, r.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w},
                bb[4] = {be.x, be.y, be.z, be.w};
    auto one = [&](const float4& zv, const float4& gv4) __attribute__((always_inline)) {
      const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
      float gv[4] = {gv4.x, gv4.y, gv4.z, gv4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float zh = (zz[j] - mm[j]) * rr[j];
        if (relu_pre && !(zh * gg[j] + bb[j] > 0.f)) gv[j] = 0.f;
        s1[j] += gv[j];
        s2[j] += gv[j] * zh;
      }
    };
    const long long stride = (long long)gridDim.x * rows;
    long long p = (long long)blockIdx.x * rows + row;
    // four pixels in flight per thread (8 - 12 sixteen-byte loads): with two, the 134 MB layers ran at 2.1 TB/s (150 - 187 us)
    for (; p + 3 * stride < npix; p += 4 * stride) {
      float4 zv[4], gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        zv[u] = *reinterpret_cast<const float4*>(z + (p + u * stride) * C + c);
        gv[u] = *reinterpret_cast<const float4*>(g + (p + u * stride) * g_cs + g_co + c);
      }
      if (mask_y) {
        float4 yv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) yv[u] = *reinterpret_cast<const float4*>(mask_y + (p + u * stride) * my_cs + my_co + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = drs_mask4(gv[u], yv[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(zv[u], gv[u]);
    }
    for (; p < npix; p += stride) {
      float4 g0 = *reinterpret_cast<const float4*>(g + p * g_cs + g_co + c);
      if (mask_y) g0 = drs_mask4(g0, *reinterpret_cast<const float4*>(mask_y + p * my_cs + my_co + c));
      one(*reinterpret_cast<const float4*>(z + p * C + c), g0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[0][threadIdx.x][j] = s1[j]; red[1][threadIdx.x][j] = s2[j]; }
  __syncthreads();
  if (threadIdx.x < c4n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double d1 = 0, d2 = 0;
      for (int r = 0; r < rows; ++r) { d1 += (double)red[0][r * c4n + threadIdx.x][j]; d2 += (double)red[1][r * c4n + threadIdx.x][j]; }
      // this block's row of the partials buffer (no atomics: see bn_stats_kernel); bn_bwd_finish_kernel adds the rows up
      partials[(size_t)blockIdx.x * 2 * C + threadIdx.x * 4 + j] = d1;
      partials[(size_t)blockIdx.x * 2 * C + C + threadIdx.x * 4 + j] = d2;
    }
  }
}
// sums[c] = sum of the partial rows (dbeta | dgamma), also written out as the parameter gradients; block = 64 channels x 4 row groups
__global__ __launch_bounds__(1024) void bn_bwd_finish_kernel(const double* __restrict__ partials, int nrows, int C,
                                                            double* __restrict__ sums, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
  __shared__ double red[2][16][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s1 = 0, s2 = 0;
  if (c < C)
#pragma unroll 8
    for (int r = rg; r < nrows; r += 16) {
      s1 += partials[(size_t)r * 2 * C + c];
      s2 += partials[(size_t)r * 2 * C + C + c];
    }
  red[0][rg][cl] = s1;
  red[1][rg][cl] = s2;
  __syncthreads();
  if (rg != 0 || c >= C) return;
  s1 = sum16(red[0], cl);
  s2 = sum16(red[1], cl);
  sums[c] = s1;
  sums[C + c] = s2;
  dbeta[c] = (float)s1;
  dgamma[c] = (float)s2;
}
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, int g_cs, int g_co,
                                                           float* __restrict__ z, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int relu_pre, int C,
                                                           long long npix, const double* __restrict__ sums,
                                                           char* __restrict__ z_sp, const float* __restrict__ mask_y,
                                                           int my_cs, int my_co) {
  // z_sp: optional second copy of dz in SP format (split bf16 hi | lo per 32-channel group, drs_common.h): the operand form
  // of the wave-specialised data-gradient convolution that reads it next (C % 32 == 0)
  const int c4n = C >> 2;
  const long long total = npix * c4n;
  const double inv = 1.0 / (double)npix;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4n) * 4;
    const long long p = i / c4n;
    const float4 m = *reinterpret_cast<const float4*>(mean + c), r = *reinterpret_cast<const float4*>(rstd + c);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
    const float4 zv = *reinterpret_cast<const float4*>(z + p * C + c);
    float4 gv4 = *reinterpret_cast<const float4*>(g + p * g_cs + g_co + c);
    if (mask_y) gv4 = drs_mask4(gv4, *reinterpret_cast<const float4*>(mask_y + p * my_cs + my_co + c));
    const float mm[4] = {m.x, m.y, m.z, m.w}, rr[4] = {r.x, r.y, r.z, r.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w},
                bb[4] = {be.x, be.y, be.z, be.w}, zz[4] = {zv.x, zv.y, zv.z, zv.w};
    float gv[4] = {gv4.x, gv4.y, gv4.z, gv4.w}, o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float zh = (zz[j] - mm[j]) * rr[j];
      if (relu_pre && !(zh * gg[j] + bb[j] > 0.f)) gv[j] = 0.f;
      o[j] = gg[j] * rr[j] * (gv[j] - (float)(sums[c + j] * inv) - zh * (float)(sums[C + c + j] * inv));
    }
    *reinterpret_cast<float4*>(z + p * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    if (z_sp) {
      unsigned hi[2], lo[2];
      drs_sp_split4(o, hi, lo);
      char* gp = z_sp + ((size_t)p * C + (c & ~31)) * 4 + (c & 31) * 2;  // the group's hi half; the lo half 64 bytes further
      *reinterpret_cast<uint2*>(gp) = make_uint2(hi[0], hi[1]);
      *reinterpret_cast<uint2*>(gp + 64) = make_uint2(lo[0], lo[1]);
    }
  }
}
int drs_launch_bn_bwd(const float* g, int g_cs, int g_co, float* z, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int relu_pre, int C, long long npix, double* partials,
                      double* sums, float* dgamma, float* dbeta, hipStream_t s, float* z_sp, const float* mask_y, int my_cs,
                      int my_co) {
  DRS_REQUIRE(!z_sp || C % 32 == 0, DRS_ERR_SHAPE, "bn_bwd: an SP copy needs C %% 32 == 0 (C=%d)", C);
  DRS_REQUIRE(!mask_y || ((my_cs & 3) == 0 && (my_co & 3) == 0), DRS_ERR_SHAPE, "bn_bwd: unaligned mask slice");
  // partials: DRS_RED_BLOCKS rows of 2 x C doubles (rewritten by every call: calls must be stream-ordered); sums: this layer's 2 x C totals
  DRS_REQUIRE(C % 4 == 0 && C <= 1024 && 256 % (C >> 2) == 0 && (g_cs & 3) == 0 && (g_co & 3) == 0, DRS_ERR_SHAPE,
              "bn_bwd: C=%d g_cs=%d g_co=%d", C, g_cs, g_co);
  const int rows = 256 / (C >> 2);
  const unsigned blocks = grid1d(npix, rows, DRS_RED_BLOCKS);
  DRS_LAUNCH(bn_bwd_reduce_kernel, dim3(blocks), dim3(256), 0, s, g, g_cs, g_co, z, mean, rstd, gamma, beta, relu_pre, C, npix,
             partials, mask_y, my_cs, my_co);
  DRS_LAUNCH(bn_bwd_finish_kernel, dim3((C + 63) / 64), dim3(1024), 0, s, partials, (int)blocks, C, sums, dgamma, dbeta);
  DRS_LAUNCH(bn_bwd_apply_kernel, dim3(grid1d(npix * (C >> 2), 256, 8192)), dim3(256), 0, s, g, g_cs, g_co, z, mean, rstd,
                     gamma, beta, relu_pre, C, npix, sums, reinterpret_cast<char*>(z_sp), mask_y, my_cs, my_co);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// BatchNorm backward with frozen statistics: mean and rstd are constants of the step, so
//   dbeta = sum g, dgamma = sum g*zhat, dz = gamma*rstd*g
// and dz no longer waits for the sums: ONE pass reads g (with its masks) and Z, accumulates the block's row of the two sums
// in bn_bwd_reduce_kernel's layout (fp32 per thread, fp64 rows, no atomics) and writes dz over Z (and the SP copy);
// bn_bwd_finish_kernel then adds the rows up as it does for the batch-statistics backward.
// In place: thread = (pixel row in block, group of 4 channels) and the pixels p = blockIdx.x * rows + row + k * stride
// of one thread are its own for reading AND for writing (the same map for both): the 16 bytes of Z at (p, channel group)
// are loaded by exactly one thread of the grid, once, and that thread stores dz there after the load (each round loads its
// four pixels before it stores any of them).  g and mask_y are other tensors and only read.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_frozen_kernel(const float* __restrict__ g, int g_cs, int g_co,
                                                            float* __restrict__ z, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int relu_pre, int C,
                                                            long long npix, double* __restrict__ partials,
                                                            char* __restrict__ z_sp, const float* __restrict__ mask_y,
                                                            int my_cs, int my_co) {
  __shared__ float red[2][256][4];
  const int c4n = C >> 2;
  const int rows = 256 / c4n;
  const int cg = threadIdx.x % c4n, row = threadIdx.x / c4n;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    const int c = cg * 4;
    const float4 m = *reinterpret_cast<const float4*>(mean + c), r = *reinterpret_cast<const float4*>(rstd + c);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
    const float mm[4] = {m.x, m.y, m.z, m.w}, rr[4] = {r.x, r.y, r.z, r.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w},
                bb[4] = {be.x, be.y, be.z, be.w};
    const float gr[4] = {gg[0] * rr[0], gg[1] * rr[1], gg[2] * rr[2], gg[3] * rr[3]};
    auto one = [&](long long p, const float4& zv, const float4& gv4) __attribute__((always_inline)) {
      const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
      float gv[4] = {gv4.x, gv4.y, gv4.z, gv4.w}, o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float zh = (zz[j] - mm[j]) * rr[j];
        if (relu_pre && !(zh * gg[j] + bb[j] > 0.f)) gv[j] = 0.f;
        s1[j] += gv[j];
        s2[j] += gv[j] * zh;
        o[j] = gr[j] * gv[j];
      }
      *reinterpret_cast<float4*>(z + p * C + c) = make_float4(o[0], o[1], o[2], o[3]);
      if (z_sp) {  // (bn_bwd_apply_kernel's SP copy)
        unsigned hi[2], lo[2];
        drs_sp_split4(o, hi, lo);
        char* gp = z_sp + ((size_t)p * C + (c & ~31)) * 4 + (c & 31) * 2;
        *reinterpret_cast<uint2*>(gp) = make_uint2(hi[0], hi[1]);
        *reinterpret_cast<uint2*>(gp + 64) = make_uint2(lo[0], lo[1]);
      }
    };
    const long long stride = (long long)gridDim.x * rows;
    long long p = (long long)blockIdx.x * rows + row;
    // four pixels in flight per thread, as in bn_bwd_reduce_kernel: all of a round's loads are issued before its stores
    for (; p + 3 * stride < npix; p += 4 * stride) {
      float4 zv[4], gv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        zv[u] = *reinterpret_cast<const float4*>(z + (p + u * stride) * C + c);
        gv[u] = *reinterpret_cast<const float4*>(g + (p + u * stride) * g_cs + g_co + c);
      }
      if (mask_y) {
        float4 yv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) yv[u] = *reinterpret_cast<const float4*>(mask_y + (p + u * stride) * my_cs + my_co + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = drs_mask4(gv[u], yv[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(p + u * stride, zv[u], gv[u]);
    }
    for (; p < npix; p += stride) {
      float4 g0 = *reinterpret_cast<const float4*>(g + p * g_cs + g_co + c);
      if (mask_y) g0 = drs_mask4(g0, *reinterpret_cast<const float4*>(mask_y + p * my_cs + my_co + c));
      one(p, *reinterpret_cast<const float4*>(z + p * C + c), g0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { red[0][threadIdx.x][j] = s1[j]; red[1][threadIdx.x][j] = s2[j]; }
  __syncthreads();
  if (threadIdx.x < c4n) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double d1 = 0, d2 = 0;
      for (int r = 0; r < rows; ++r) { d1 += (double)red[0][r * c4n + threadIdx.x][j]; d2 += (double)red[1][r * c4n + threadIdx.x][j]; }
      partials[(size_t)blockIdx.x * 2 * C + threadIdx.x * 4 + j] = d1;
      partials[(size_t)blockIdx.x * 2 * C + C + threadIdx.x * 4 + j] = d2;
    }
  }
}
int drs_launch_bn_bwd_frozen(const float* g, int g_cs, int g_co, float* z, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, int relu_pre, int C, long long npix, double* partials,
                             double* sums, float* dgamma, float* dbeta, hipStream_t s, float* z_sp, const float* mask_y,
                             int my_cs, int my_co) {
  DRS_REQUIRE(!z_sp || C % 32 == 0, DRS_ERR_SHAPE, "bn_bwd_frozen: an SP copy needs C %% 32 == 0 (C=%d)", C);
  DRS_REQUIRE(!mask_y || ((my_cs & 3) == 0 && (my_co & 3) == 0), DRS_ERR_SHAPE, "bn_bwd_frozen: unaligned mask slice");
  DRS_REQUIRE(C % 4 == 0 && C <= 1024 && 256 % (C >> 2) == 0 && (g_cs & 3) == 0 && (g_co & 3) == 0, DRS_ERR_SHAPE,
              "bn_bwd_frozen: C=%d g_cs=%d g_co=%d", C, g_cs, g_co);
  const int rows = 256 / (C >> 2);
  const unsigned blocks = grid1d(npix, rows, DRS_RED_BLOCKS);  // one partials row per block: at most DRS_RED_BLOCKS rows
  DRS_LAUNCH(bn_bwd_frozen_kernel, dim3(blocks), dim3(256), 0, s, g, g_cs, g_co, z, mean, rstd, gamma, beta, relu_pre, C, npix,
             partials, reinterpret_cast<char*>(z_sp), mask_y, my_cs, my_co);
  DRS_LAUNCH(bn_bwd_finish_kernel, dim3((C + 63) / 64), dim3(1024), 0, s, partials, (int)blocks, C, sums, dgamma, dbeta);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
