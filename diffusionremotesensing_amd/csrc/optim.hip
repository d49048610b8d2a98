// Clipped, decayed, guarded Adam (include/drs_hip.h: drs_grad_sumsq_partials, drs_adamw_clip_multi): the global gradient
// norm and the update that consumes it, two launches on one stream and no host synchronisation between them.  Both run on
// the (chunk of kChunk, tensor) grid of adam_multi_kernel (below); the update's per-element arithmetic IS that kernel's,
// on the scaled gradient and the decayed parameter.  The plain multi-tensor Adam and the parameter EMA close the file.
//
// Reduction order (the only thing here that could make two runs differ): thread t of a chunk adds the squares of elements
// t, t + 256, ... in that order; 64 lanes are combined by a shuffle tree (offsets 32, 16, .. 1); the four wave sums are added
// in wave order through LDS.  The update kernel adds the chunks' partials in index order, every block on its own: every
// block holds the same bits, and neither the dispatch order nor the grid's extent enters.  No atomics, no fences.
#include "drs_common.h"

constexpr int kChunk = 4096;            // elements per block of every kernel here
constexpr int kPerThread = kChunk / 256;
constexpr int kPartialTile = 2048;      // partials staged in LDS at a time (16 KiB)

// A product that stays a product.  The __f*_rn functions of this compiler are plain operators, open to contraction into a
// fused multiply-add with whatever consumes them: the scaled gradient and the decayed parameter must reach the update as
// ROUNDED values (torch rounds them: mul_ writes them to memory), and the update itself must see them as adam_multi_kernel
// sees its loads, or the compiler picks other products to fuse there and the two kernels stop agreeing bit for bit.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const drs_adamw_tensor* __restrict__ table,
                                                         double* __restrict__ partials) {
  const drs_adamw_tensor t = table[blockIdx.y];
  const long long lo = (long long)blockIdx.x * kChunk;
  if (lo >= t.n) return;
  const long long hi = min((long long)t.n, lo + kChunk);
  double s = 0.0;
  if (t.g) {
    float g[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const long long i = lo + threadIdx.x + 256 * k;
      g[k] = i < hi ? t.g[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) s = __dadd_rn(s, __dmul_rn((double)g[k], (double)g[k]));
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = __dadd_rn(s, __shfl_down(s, off, 64));
  __shared__ double wave_sum[4];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[t.part0 + blockIdx.x] =
        __dadd_rn(__dadd_rn(__dadd_rn(wave_sum[0], wave_sum[1]), wave_sum[2]), wave_sum[3]);
}

extern "C" int drs_grad_sumsq_partials(const drs_adamw_tensor* table, int ntensors, int64_t max_numel, double* partials,
                                       drs_stream_t stream) {
  DRS_REQUIRE(table && partials && ntensors >= 0, DRS_ERR_ARG, "grad_sumsq_partials: bad arguments");
  if (ntensors == 0 || max_numel <= 0) return DRS_OK;
  const unsigned gx = (unsigned)((max_numel + kChunk - 1) / kChunk);
  DRS_LAUNCH(grad_sumsq_kernel, dim3(gx, ntensors), dim3(256), 0, (hipStream_t)stream, table, partials);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

__global__ __launch_bounds__(256) void adamw_clip_multi_kernel(const drs_adamw_tensor* __restrict__ table, double lr,
                                                               double b1d, double b2d, float eps, double weight_decay,
                                                               double max_norm, int skip_nonfinite,
                                                               const double* __restrict__ partials, int npartials,
                                                               drs_adamw_stats* __restrict__ stats) {
  const drs_adamw_tensor t = table[blockIdx.y];
  const bool first = blockIdx.x == 0 && blockIdx.y == 0;  // writes the statistics, live or not
  const long long lo = (long long)blockIdx.x * kChunk;
  const bool live = t.g && lo < t.n;
  if (!live && !first) return;  // (block-uniform)
  const long long hi = live ? min((long long)t.n, lo + kChunk) : lo;
  // S: the partials in index order, on one chain.  All threads bring a tile of them into LDS (one round trip to L2 instead of
  // one per handful of terms), then the first wave adds the tile in order - every lane the same chain, lane 0 keeps it.
  __shared__ double tile[kPartialTile];
  __shared__ double total;
  double S = 0.0;
  for (int j0 = 0; j0 < npartials; j0 += kPartialTile) {
    const int nj = min(kPartialTile, npartials - j0);
    for (int j = threadIdx.x; j < nj; j += 256) tile[j] = partials[j0 + j];
    __syncthreads();
    if (threadIdx.x < 64) {
#pragma unroll 16
      for (int j = 0; j < nj; ++j) S = __dadd_rn(S, tile[j]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) total = S;
  __syncthreads();
  S = total;
  const bool finite = isfinite(S);
  const bool skip = skip_nonfinite && !finite;
  const double norm = sqrt(S);
  float coef = 1.0f;
  if (max_norm > 0.0) {  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1.0), a NaN stays one
    const double c = max_norm / (norm + 1e-6);
    coef = (float)(c > 1.0 ? 1.0 : c);
  }
  if (first && threadIdx.x == 0 && stats) {
    stats->norm = (float)norm;
    stats->coef = coef;
    stats->skipped = skip ? 1 : 0;
    if (skip) stats->skipped_total += 1;
  }
  if (skip || !live) return;  // a skipped step leaves p, m and v of every tensor untouched
  // torch forms 1 - beta in Python doubles and rounds the result to fp32 inside the kernels
  const float beta2 = (float)b2d, w1 = (float)(1.0 - b1d), w2 = (float)(1.0 - b2d);
  const float keep = (float)(1.0 - lr * weight_decay);  // torch.optim.AdamW: param.mul_(1 - lr * weight_decay)
  const double bc1 = 1.0 - pow(b1d, (double)t.step), bc2 = 1.0 - pow(b2d, (double)t.step);
  const float lr_over_bc1 = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const float g = mul_rounded(t.g[i], coef);
    float m = t.m[i], v = t.v[i];
    const float p = mul_rounded(t.p[i], keep);
    // from here: adam_multi_kernel's sequence
    m = w1 < 0.5f ? fmaf(w1, __fsub_rn(g, m), m) : __fsub_rn(g, __fmul_rn(__fsub_rn(g, m), __fsub_rn(1.f, w1)));  // lerp_
    v = __fadd_rn(__fmul_rn(v, beta2), __fmul_rn(__fmul_rn(w2, g), g));                                          // mul_, addcmul_
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);
    t.m[i] = m;
    t.v[i] = v;
    t.p[i] = __fadd_rn(p, __fmul_rn(-lr_over_bc1, __fdiv_rn(m, denom)));                                         // addcdiv_
  }
}

extern "C" int drs_adamw_clip_multi(const drs_adamw_tensor* table, int ntensors, int64_t max_numel, double lr, double beta1,
                                    double beta2, double eps, double weight_decay, double max_norm, int skip_nonfinite,
                                    const double* partials, int npartials, drs_adamw_stats* stats, drs_stream_t stream) {
  DRS_REQUIRE(table && ntensors >= 0 && npartials >= 0 && (partials || npartials == 0), DRS_ERR_ARG,
              "adamw_clip_multi: bad arguments");
  DRS_REQUIRE(npartials > 0 || !(max_norm > 0.0), DRS_ERR_ARG, "adamw_clip_multi: max_norm=%g needs the norm's partials",
              max_norm);
  if (ntensors == 0 || max_numel <= 0) return DRS_OK;
  const unsigned gx = (unsigned)((max_numel + kChunk - 1) / kChunk);
  DRS_LAUNCH(adamw_clip_multi_kernel, dim3(gx, ntensors), dim3(256), 0, (hipStream_t)stream, table, lr, beta1, beta2,
             (float)eps, weight_decay, max_norm, skip_nonfinite, partials, npartials, stats);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Multi-tensor Adam (torch.optim.Adam defaults), one launch for all parameters: grid = (chunks of the largest tensor,
// tensors); blocks beyond a tensor's length exit.  Same operation order as torch's single-tensor implementation.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_multi_kernel(const drs_adam_tensor* __restrict__ table, double lr, double b1d,
                                                         double b2d, float eps) {
  const drs_adam_tensor t = table[blockIdx.y];
  if (!t.g) return;  // no gradient this step: torch skips the parameter (state untouched)
  // torch forms 1 - beta in Python doubles and rounds the result to fp32 inside the kernels
  const float beta2 = (float)b2d, w1 = (float)(1.0 - b1d), w2 = (float)(1.0 - b2d);
  const long long lo = (long long)blockIdx.x * kChunk;
  if (lo >= t.n) return;
  const long long hi = min(t.n, lo + kChunk);
  // bias corrections in double like torch's Python-side scalars (step_size = lr / bc1, bias_correction2_sqrt)
  const double bc1 = 1.0 - pow(b1d, (double)t.step), bc2 = 1.0 - pow(b2d, (double)t.step);
  const float lr_over_bc1 = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  for (long long i = lo + threadIdx.x; i < hi; i += 256) {
    const float g = t.g[i];
    float m = t.m[i], v = t.v[i];
    m = w1 < 0.5f ? fmaf(w1, __fsub_rn(g, m), m) : __fsub_rn(g, __fmul_rn(__fsub_rn(g, m), __fsub_rn(1.f, w1)));  // lerp_
    v = __fadd_rn(__fmul_rn(v, beta2), __fmul_rn(__fmul_rn(w2, g), g));                                          // mul_, addcmul_
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), eps);
    t.m[i] = m;
    t.v[i] = v;
    t.p[i] = __fadd_rn(t.p[i], __fmul_rn(-lr_over_bc1, __fdiv_rn(m, denom)));                                    // addcdiv_
  }
}
extern "C" int drs_adam_multi(const drs_adam_tensor* table, int ntensors, int64_t max_numel, double lr, double beta1,
                              double beta2, double eps, drs_stream_t stream) {
  DRS_REQUIRE(table && ntensors >= 0, DRS_ERR_ARG, "adam_multi: bad arguments");
  if (ntensors == 0 || max_numel <= 0) return DRS_OK;
  const unsigned gx = (unsigned)((max_numel + kChunk - 1) / kChunk);
  DRS_LAUNCH(adam_multi_kernel, dim3(gx, ntensors), dim3(256), 0, (hipStream_t)stream, table, lr, beta1, beta2,
                     (float)eps);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Multi-tensor EMA of the parameters (include/drs_hip.h: drs_ema_multi; reference EMA, UNet_model_superres.py:12-55):
// grid = (chunks of the largest tensor, tensors).  mode 0: old * beta + (1 - beta) * new with torch's rounding (scalar
// operands rounded to fp32, two products and one sum, no fused multiply-add); mode 1: word copy (warm-up).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ema_multi_kernel(const drs_ema_tensor* __restrict__ table, float beta, float w, int mode) {
  const drs_ema_tensor t = table[blockIdx.y];
  const long long lo = (long long)blockIdx.x * kChunk;
  if (lo >= t.n) return;
  const long long hi = min((long long)t.n, lo + kChunk);
  if (mode == 1) {
    unsigned* dst = (unsigned*)t.ema;
    const unsigned* src = (const unsigned*)t.cur;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) dst[i] = src[i];
  } else {
    float* e = (float*)t.ema;
    const float* c = (const float*)t.cur;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) e[i] = __fadd_rn(__fmul_rn(e[i], beta), __fmul_rn(w, c[i]));
  }
}
extern "C" int drs_ema_multi(const drs_ema_tensor* table, int ntensors, int64_t max_numel, double beta, int mode,
                             drs_stream_t stream) {
  DRS_REQUIRE(table && ntensors >= 0 && (mode == 0 || mode == 1), DRS_ERR_ARG, "ema_multi: bad arguments");
  if (ntensors == 0 || max_numel <= 0) return DRS_OK;
  const unsigned gx = (unsigned)((max_numel + kChunk - 1) / kChunk);
  DRS_LAUNCH(ema_multi_kernel, dim3(gx, ntensors), dim3(256), 0, (hipStream_t)stream, table, (float)beta,
                     (float)(1.0 - beta), mode);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
