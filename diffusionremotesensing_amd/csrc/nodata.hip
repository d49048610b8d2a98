// Training and scoring on imagery with no-data pixels (include/drs_hip.h: drs_noise_target_nodata, drs_diffusion_loss_masked,
// drs_metrics_pointwise_nodata, drs_ssim_nodata).  A pixel of a clean image (C, H, W) is no-data when any
// of its bands is NaN or, with a finite `nodata_value`, when all of its bands equal it (fp32 compare); the mask is per pixel,
// shared by the bands, and taken from the clean / truth image before any clamp.  No-data elements are SELECTED out - never
// multiplied by zero - so that a NaN or an infinity under the mask reaches no output.
//
// The four entries restate the per-element arithmetic and the reduction order of their unmasked siblings (small_kernels.hip /
// prediction.hip: forward noising and targets; loss.hip: chunks of 4096, thread / shuffle tree / wave order, doubles;
// metrics.hip: fp32 in the block, one fp64 partial per block, fixed-order sum), so that a batch without a no-data pixel gives
// the siblings' bits.  No atomics anywhere: two calls give the same bits.
#include "drs_common.h"
#include "step_update.h"
#include <cmath>

// (as metrics.hip: identical inputs must give exactly 0 degrees and SSIM 1; every fused multiply-add below is an explicit fmaf)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

__device__ __forceinline__ bool is_nan(float v) { return v != v; }

// ---- forward noising, target and mask ------------------------------------------------------------------------------
struct NoiseNodataArgs {
  const float* x0;
  const float* eps;
  const int64_t* t;
  const float* alpha_hat;
  float* xt;
  float* target;
  unsigned char* valid;
  int n, C, noise_steps, kind;
  float nodata_value, fill;
  int64_t hw;
};

// blockIdx.y strides over the images, blockIdx.x over one image's groups of V consecutive pixels.  A thread holds the C bands
// of its pixels of x0 in registers (CB register rows, as metrics_pointwise_kernel), decides the mask, then walks the bands
// once more for eps and the two stores.  V = 4: hw % 4 == 0 and 16-byte aligned tensors, the four decisions are one 32-bit store.
template <int V, int CB>
__global__ __launch_bounds__(kThreads) void noise_target_nodata_kernel(const NoiseNodataArgs p) {
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
  const int64_t groups = p.hw / V;
  const bool by_value = __builtin_isfinite(p.nodata_value);
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    const int64_t tn = p.t[img];
    const bool bad = tn < 0 || tn >= p.noise_steps;  // never indexes the table: this image's outputs are NaN, its mask 0
    const float ah = bad ? 0.f : p.alpha_hat[tn];
    const float a = sqrtf(ah), b = sqrtf(1.f - ah);  // fp32, as noise_images_kernel
    const int64_t row = (int64_t)img * p.C * p.hw;
    for (int64_t g = tid; g < groups; g += stride) {
      const int64_t at = g * V;
      float x[CB][V];
      bool nan[V], same[V];
#pragma unroll
      for (int k = 0; k < V; ++k) nan[k] = false, same[k] = true;
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        if (c >= p.C) continue;
        const float* xp = p.x0 + row + c * p.hw + at;
        if constexpr (V == 4) {
          const float4 v = *reinterpret_cast<const float4*>(xp);
          x[c][0] = v.x, x[c][1] = v.y, x[c][2] = v.z, x[c][3] = v.w;
        } else {
          x[c][0] = *xp;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          nan[k] = nan[k] || is_nan(x[c][k]);
          same[k] = same[k] && x[c][k] == p.nodata_value;
        }
      }
      bool nd[V];
      unsigned char ok[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        nd[k] = nan[k] || (by_value && same[k]);
        ok[k] = !nd[k] && !bad;
      }
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        if (c >= p.C) continue;
        const int64_t off = row + c * p.hw + at;
        float e[V], o[V], w[V];
        if constexpr (V == 4) {
          const float4 v = *reinterpret_cast<const float4*>(p.eps + off);
          e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
        } else {
          e[0] = p.eps[off];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float xv = x[c][k];
          const float tv = p.kind == DRS_PRED_EPS ? e[k] : p.kind == DRS_PRED_V ? drs_v_target(a, b, xv, e[k]) : xv;
          o[k] = bad ? __builtin_nanf("") : drs_forward_noise(a, b, nd[k] ? p.fill : xv, e[k]);
          w[k] = bad ? __builtin_nanf("") : nd[k] ? 0.f : tv;
        }
        if constexpr (V == 4) {
          *reinterpret_cast<float4*>(p.xt + off) = make_float4(o[0], o[1], o[2], o[3]);
          *reinterpret_cast<float4*>(p.target + off) = make_float4(w[0], w[1], w[2], w[3]);
        } else {
          p.xt[off] = o[0];
          p.target[off] = w[0];
        }
      }
      unsigned char* vp = p.valid + (int64_t)img * p.hw + at;
      if constexpr (V == 4) {
        *reinterpret_cast<uchar4*>(vp) = make_uchar4(ok[0], ok[1], ok[2], ok[3]);
      } else {
        *vp = ok[0];
      }
    }
  }
}

template <int V>
void launch_noise(const NoiseNodataArgs& a, hipStream_t s) {
  const int gy = a.n < 65535 ? a.n : 65535;
  int64_t gx = (a.hw / V + kThreads - 1) / kThreads, cap = std::max(1, 4096 / gy);
  gx = std::max<int64_t>(1, std::min(gx, cap));
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (a.C <= 4) DRS_LAUNCH((noise_target_nodata_kernel<V, 4>), grid, dim3(kThreads), 0, s, a);
  else DRS_LAUNCH((noise_target_nodata_kernel<V, kMaxBands>), grid, dim3(kThreads), 0, s, a);
}

// ---- masked loss ---------------------------------------------------------------------------------------------------
constexpr int kChunk = 4096;       // as loss.hip: elements per block, 256 threads x 4 groups of 4
constexpr int kGroups = 4;
constexpr int kFinThreads = 1024;
constexpr int kMaxBins = 64, kMaxHistory = 32;

__device__ __forceinline__ int row_misalignment(const float* p) { return (int)(((uintptr_t)p >> 2) & 3u); }

// (loss.hip) w_b = table[t_b] * sample_w[b] in double; a t_b outside [0, T) with a table gives NaN, not a read
__device__ __forceinline__ double image_weight(const float* table, int T, long long tb, const float* sample_w, int b) {
  double w = 1.0;
  if (table) w = (tb >= 0 && tb < T) ? (double)table[tb] : __longlong_as_double(0x7ff8000000000000LL);
  if (sample_w) w = __dmul_rn(w, (double)sample_w[b]);
  return w;
}

// (loss.hip) one element: adds l(d) to `s` in double, returns coef * l'(d)
template <int KIND>
__device__ __forceinline__ float loss_element(float p, float q, double delta, float coef, float coef_delta, double& s) {
  const float d = __fsub_rn(p, q);
  const double dd = (double)d;
  const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : d;
  if (KIND == DRS_LOSS_MSE) {
    s = __dadd_rn(s, __dmul_rn(dd, dd));
    return __fmul_rn(coef, d);
  }
  const double ad = fabs(dd);
  if (KIND == DRS_LOSS_MAE) {
    s = __dadd_rn(s, ad);
    return __fmul_rn(coef, sg);
  }
  const bool outer = ad > delta;
  s = __dadd_rn(s, outer ? __dmul_rn(delta, __dsub_rn(ad, __dmul_rn(0.5, delta))) : __dmul_rn(0.5, __dmul_rn(ad, ad)));
  return outer ? __fmul_rn(coef_delta, sg) : __fmul_rn(coef, d);
}

// counts[b] = the valid pixels of image b: one block per image, 16 mask bytes per thread and trip where the row allows
__global__ __launch_bounds__(kThreads) void valid_count_kernel(const unsigned char* __restrict__ valid, int64_t hw,
                                                               long long* __restrict__ counts) {
  __shared__ long long red[kWaves];
  const unsigned char* row = valid + (int64_t)blockIdx.x * hw;
  const int64_t lead = (16 - ((uintptr_t)row & 15u)) & 15u, head = lead < hw ? lead : hw, lines = (hw - head) / 16;
  long long n = 0;
  for (int64_t j = threadIdx.x; j < lines; j += kThreads) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + head + 16 * j);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      n += ((w[k] & 0xffu) != 0) + ((w[k] & 0xff00u) != 0) + ((w[k] & 0xff0000u) != 0) + ((w[k] & 0xff000000u) != 0);
  }
  const int64_t rest = hw - 16 * lines;  // head and tail bytes: at most 30
  for (int64_t r = threadIdx.x; r < rest; r += kThreads) n += row[r < head ? r : 16 * lines + r] != 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// diffusion_loss_kernel (loss.hip) with the mask: grid (chunks, B), the same virtual 16-byte grid of the row's start address,
// the same 16 elements per thread in the same order.  Element i of a row belongs to pixel i % hw; the four decisions of a
// group are one 32-bit load where the group lies inside one band and its mask bytes are 4-byte aligned, four byte loads
// otherwise.  A no-data element adds nothing and its gradient is +0.0; its pred and target are loaded but never used.
// The coefficient needs Bv (images with a valid pixel) and n_b = C nv_b: every block counts Bv from `counts` itself.
template <int KIND, bool GRAD>
__global__ __launch_bounds__(kThreads) void diffusion_loss_masked_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, const unsigned char* __restrict__ valid,
    const long long* __restrict__ t, int B, int C, long long hw, const float* __restrict__ table, int T,
    const float* __restrict__ sample_w, double delta, const long long* __restrict__ counts, float* __restrict__ grad,
    double* __restrict__ partials) {
  __shared__ double wave_sum[kWaves];
  __shared__ int wave_images[kWaves];
  const int b = blockIdx.y;
  const long long n = (long long)C * hw;
  const float* p = pred + (long long)b * n;
  const float* q = target + (long long)b * n;
  const unsigned char* m = valid + (long long)b * hw;
  float* g = GRAD ? grad + (long long)b * n : nullptr;
  const int mp = row_misalignment(p);
  const bool vec = mp == row_misalignment(q) && (!GRAD || mp == row_misalignment(g));
  const int mis = vec ? mp : 0;
  float coef = 0.f, coef_delta = 0.f;
  if (GRAD) {
    int images = 0;
    for (int i = threadIdx.x; i < B; i += kThreads) images += counts[i] > 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) images += __shfl_down(images, off, 64);
    if ((threadIdx.x & 63) == 0) wave_images[threadIdx.x >> 6] = images;
    __syncthreads();
    const int Bv = wave_images[0] + wave_images[1] + wave_images[2] + wave_images[3];
    const long long nv = counts[b];
    if (nv > 0) {  // (then Bv >= 1)
      const double scale = 1.0 / ((double)Bv * (double)((long long)C * nv));
      const double w = image_weight(table, T, table ? t[b] : 0, sample_w, b);
      coef = (float)__dmul_rn(w, KIND == DRS_LOSS_MSE ? 2.0 * scale : scale);
      coef_delta = (float)__dmul_rn(w, delta * scale);
    }
  }
  float pv[kGroups][4], qv[kGroups][4];
  bool ok[kGroups][4];
  long long first[kGroups];
  const long long i0 = 4 * ((long long)blockIdx.x * (kChunk / 4) + threadIdx.x) - mis;
  long long pix = i0 % hw;  // the pixel of the thread's first element (of element -mis .. -1: counted back from the row's end)
  if (pix < 0) pix += hw;
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const long long i = i0 + 4 * kThreads * k;  // the group's first element
    first[k] = i;
    const bool whole = vec && i >= 0 && i + 4 <= n;
    if (whole) {
      const float4 a = *reinterpret_cast<const float4*>(p + i), c = *reinterpret_cast<const float4*>(q + i);
      pv[k][0] = a.x, pv[k][1] = a.y, pv[k][2] = a.z, pv[k][3] = a.w;
      qv[k][0] = c.x, qv[k][1] = c.y, qv[k][2] = c.z, qv[k][3] = c.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = i + e >= 0 && i + e < n;
        pv[k][e] = in ? p[i + e] : 0.f;
        qv[k][e] = in ? q[i + e] : 0.f;
      }
    }
    if (whole && pix + 4 <= hw && (((uintptr_t)(m + pix)) & 3u) == 0) {
      const unsigned four = *reinterpret_cast<const unsigned*>(m + pix);
      ok[k][0] = (four & 0xffu) != 0, ok[k][1] = (four & 0xff00u) != 0;
      ok[k][2] = (four & 0xff0000u) != 0, ok[k][3] = (four & 0xff000000u) != 0;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        long long at = pix + e;
        if (at >= hw) at %= hw;
        ok[k][e] = i + e >= 0 && i + e < n && m[at] != 0;  // (outside the row: nothing is read, added or stored)
      }
    }
    pix += 4 * kThreads;
    if (pix >= hw) pix = hw > 4 * kThreads ? pix - hw : pix % hw;
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const long long i = first[k];
    float gv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gv[e] = 0.f;
      if (ok[k][e]) gv[e] = loss_element<KIND>(pv[k][e], qv[k][e], delta, coef, coef_delta, s);
    }
    if (!GRAD) continue;
    if (vec && i >= 0 && i + 4 <= n) {
      *reinterpret_cast<float4*>(g + i) = make_float4(gv[0], gv[1], gv[2], gv[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i + e >= 0 && i + e < n) g[i + e] = gv[e];
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = __dadd_rn(s, __shfl_down(s, off, 64));
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(long long)b * gridDim.x + blockIdx.x] =
        __dadd_rn(__dadd_rn(__dadd_rn(wave_sum[0], wave_sum[1]), wave_sum[2]), wave_sum[3]);
}

// diffusion_loss_finish_kernel (loss.hip) over the images that have a valid pixel: per_image divides by n_b = C nv_b, the loss
// by Bv; an image without a valid pixel has per_image 0 and enters neither the loss, the bins nor the ring.
__global__ __launch_bounds__(kFinThreads) void diffusion_loss_masked_finish_kernel(
    const double* __restrict__ partials, const long long* __restrict__ counts, int chunks, int B, int C,
    const long long* __restrict__ t, const float* __restrict__ table, int T, const float* __restrict__ sample_w,
    double* __restrict__ per_image, double* __restrict__ out, double* __restrict__ bins, int nbins, int history, int update_ring,
    long long* __restrict__ bad_t) {
  __shared__ double image_loss[kFinThreads], weight[kFinThreads];
  __shared__ long long elements[kFinThreads];  // n_b; 0: no valid pixel
  __shared__ int image_bin[kFinThreads];       // >= 0: the bin, -1: no bins, -2: t outside [0, T)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool uses_t = table || bins;
  const bool bin_thread = bins && tid < nbins;
  double bin_sum = 0.0;
  long long bin_count = 0, bin_appended = 0;
  int ring_pos = 0;
  double* ring = nullptr;
  if (bin_thread) {
    bin_sum = bins[tid];
    bin_count = __double_as_longlong(bins[nbins + tid]);
    bin_appended = __double_as_longlong(bins[2 * nbins + tid]);
    ring_pos = (int)((bin_appended % history + history) % history);
    ring = bins + 3 * nbins + 1 + tid * history;
  }
  double S = 0.0;
  long long bad = 0, nonfinite = 0, Bv = 0;
  for (int b0 = 0; b0 < B; b0 += kFinThreads) {
    const int nb = min(kFinThreads, B - b0);
    __syncthreads();
    if (tid < nb) {
      const int b = b0 + tid;
      const long long tv = uses_t ? t[b] : 0;
      const bool in_range = tv >= 0 && tv < T;
      weight[tid] = image_weight(table, T, tv, sample_w, b);
      image_bin[tid] = !uses_t || in_range ? (bins ? (int)(tv * nbins / T) : -1) : -2;
      elements[tid] = (long long)C * counts[b];
    }
    __syncthreads();
    for (int i = wave; i < nb; i += kFinThreads / 64) {
      const double* row = partials + (long long)(b0 + i) * chunks;
      double s = 0.0;
      for (int j0 = 0; j0 < chunks; j0 += 256) {
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = j0 + lane + 64 * k;
          r[k] = j < chunks ? row[j] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s = __dadd_rn(s, r[k]);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s = __dadd_rn(s, __shfl_down(s, off, 64));
      if (lane == 0) {
        const double v = elements[i] > 0 ? s / (double)elements[i] : 0.0;
        per_image[b0 + i] = v;
        image_loss[i] = v;
      }
    }
    __syncthreads();
    if (bin_thread) {
      for (int i = 0; i < nb; ++i) {
        const double v = image_loss[i];
        if (image_bin[i] != tid || elements[i] == 0 || !isfinite(v)) continue;
        bin_sum = __dadd_rn(bin_sum, v);
        ++bin_count;
        if (update_ring) {
          ring[ring_pos] = v;
          ring_pos = ring_pos + 1 == history ? 0 : ring_pos + 1;
          ++bin_appended;
        }
      }
    } else if (tid == 64) {
      for (int i = 0; i < nb; ++i) {
        bad += image_bin[i] == -2;
        if (elements[i] == 0) continue;
        const double v = image_loss[i];
        S = __dadd_rn(S, __dmul_rn(weight[i], v));
        ++Bv;
        nonfinite += image_bin[i] >= 0 && !isfinite(v);
      }
    }
  }
  if (bin_thread) {
    bins[tid] = bin_sum;
    bins[nbins + tid] = __longlong_as_double(bin_count);
    bins[2 * nbins + tid] = __longlong_as_double(bin_appended);
  }
  if (tid == 64) {
    const double loss = Bv > 0 ? S / (double)Bv : 0.0;
    out[0] = loss;
    reinterpret_cast<float*>(out)[2] = (float)loss;
    if (nonfinite) bins[3 * nbins] = __longlong_as_double(__double_as_longlong(bins[3 * nbins]) + nonfinite);
    if (bad && bad_t) *bad_t += bad;
  }
}

template <int KIND>
void launch_masked_loss(dim3 grid, hipStream_t s, const float* pred, const float* target, const unsigned char* valid,
                        const int64_t* t, int B, int C, int64_t hw, const float* table, int T, const float* sample_w, double delta,
                        const long long* counts, float* grad, double* partials) {
  if (grad)
    DRS_LAUNCH((diffusion_loss_masked_kernel<KIND, true>), grid, dim3(kThreads), 0, s, pred, target, valid, (const long long*)t, B,
               C, (long long)hw, table, T, sample_w, delta, counts, grad, partials);
  else
    DRS_LAUNCH((diffusion_loss_masked_kernel<KIND, false>), grid, dim3(kThreads), 0, s, pred, target, valid, (const long long*)t, B,
               C, (long long)hw, table, T, sample_w, delta, counts, grad, partials);
}

// ---- metrics -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float v) {  // torch.clamp(v, 0, 1): a NaN stays a NaN
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, 0.f), 1.f);
}

template <typename T>
__device__ __forceinline__ T wave_sum_of(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// metrics_pointwise_kernel (metrics.hip) with the mask of hr's pixel: the same groups per thread, the same fp32 chains; a
// no-data pixel leaves every chain as it was.  partials: [image][block][2 C + 3] = sse[C] | sum_hr[C] | angle sum | pixels in
// the angle sum | valid pixels
template <int V, int CB>
__global__ __launch_bounds__(kThreads) void metrics_pointwise_nodata_kernel(const float* __restrict__ sr,
                                                                            const float* __restrict__ hr, float nodata_value,
                                                                            double* __restrict__ partials, int C, int64_t hw,
                                                                            int clamp) {
  __shared__ float red[2 * CB + 1][kWaves];
  __shared__ int red_n[2][kWaves];
  const float* sp = sr + (int64_t)blockIdx.y * C * hw;
  const float* hp = hr + (int64_t)blockIdx.y * C * hw;
  const int64_t groups = hw / V;
  const bool by_value = __builtin_isfinite(nodata_value);
  float sse[CB], shr[CB], ang = 0.f;
  int cnt = 0, nvalid = 0;
#pragma unroll
  for (int c = 0; c < CB; ++c) sse[c] = shr[c] = 0.f;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
    float u[CB][V], v[CB][V], uu[V], vv[V];
    bool nan[V], same[V], ok[V];
#pragma unroll
    for (int p = 0; p < V; ++p) uu[p] = vv[p] = 0.f, nan[p] = false, same[p] = true;
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      if (c >= C) continue;
      if constexpr (V == 4) {
        const float4 a = *reinterpret_cast<const float4*>(sp + c * hw + g * 4);
        const float4 b = *reinterpret_cast<const float4*>(hp + c * hw + g * 4);
        u[c][0] = a.x; u[c][1] = a.y; u[c][2] = a.z; u[c][3] = a.w;
        v[c][0] = b.x; v[c][1] = b.y; v[c][2] = b.z; v[c][3] = b.w;
      } else {
        u[c][0] = sp[c * hw + g];
        v[c][0] = hp[c * hw + g];
      }
#pragma unroll
      for (int p = 0; p < V; ++p) {  // the mask: hr as stored, before the clamp
        nan[p] = nan[p] || is_nan(v[c][p]);
        same[p] = same[p] && v[c][p] == nodata_value;
      }
    }
#pragma unroll
    for (int p = 0; p < V; ++p) {
      ok[p] = !(nan[p] || (by_value && same[p]));
      nvalid += ok[p];
    }
#pragma unroll
    for (int c = 0; c < CB; ++c) {
      if (c >= C) continue;
#pragma unroll
      for (int p = 0; p < V; ++p) {
        if (clamp) {
          u[c][p] = clamp01(u[c][p]);
          v[c][p] = clamp01(v[c][p]);
        }
        if (!ok[p]) continue;
        const float d = u[c][p] - v[c][p];
        sse[c] = fmaf(d, d, sse[c]);
        shr[c] += v[c][p];
        uu[p] = fmaf(u[c][p], u[c][p], uu[p]);
        vv[p] = fmaf(v[c][p], v[c][p], vv[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < V; ++p) {
      if (!ok[p] || uu[p] == 0.f || vv[p] == 0.f) continue;
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
    const float a = wave_sum_of(sse[c]), b = wave_sum_of(shr[c]);
    if (lane == 0) {
      red[c][wave] = a;
      red[CB + c][wave] = b;
    }
  }
  ang = wave_sum_of(ang);
  cnt = wave_sum_of(cnt);
  nvalid = wave_sum_of(nvalid);
  if (lane == 0) {
    red[2 * CB][wave] = ang;
    red_n[0][wave] = cnt;
    red_n[1][wave] = nvalid;
  }
  __syncthreads();
  const int K = 2 * C + 3, k = threadIdx.x;
  if (k < K) {
    double* out = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * K;
    if (k >= K - 2) {
      int n = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) n += red_n[k - (K - 2)][w];
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

// the block sum of metrics_reduce_kernel (metrics.hip): threads stride over the n partials of a column, then the LDS tree
__device__ __forceinline__ double column_sum(const double* p, int64_t n, int K, double* red) {
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < n; j += kThreads) s += p[j * K];
  __syncthreads();  // (a previous column's tree)
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// out[image][k] = the sum over the n partial rows, in metrics_reduce_kernel's order.  blockIdx.x = k, blockIdx.y = image.
__global__ __launch_bounds__(kThreads) void nodata_reduce_kernel(const double* __restrict__ partials, double* __restrict__ out,
                                                                 int64_t n, int K) {
  __shared__ double red[kThreads];
  const double s = column_sum(partials + (int64_t)blockIdx.y * n * K + blockIdx.x, n, K, red);
  if (threadIdx.x == 0) out[(int64_t)blockIdx.y * K + blockIdx.x] = s;
}

// out[image] = (sum of the C * tiles SSIM partials / (C * positions), positions) with positions = the sum of the image's
// `tiles` counts.  blockIdx.x = image.
__global__ __launch_bounds__(kThreads) void ssim_nodata_reduce_kernel(const double* __restrict__ sums,
                                                                      const double* __restrict__ counts,
                                                                      double* __restrict__ out, int C, int64_t tiles) {
  __shared__ double red[kThreads];
  const double s = column_sum(sums + (int64_t)blockIdx.x * C * tiles, (int64_t)C * tiles, 1, red);
  const double n = column_sum(counts + (int64_t)blockIdx.x * tiles, tiles, 1, red);
  if (threadIdx.x == 0) {
    out[2 * (int64_t)blockIdx.x] = n > 0.0 ? s / ((double)C * n) : __longlong_as_double(0x7ff8000000000000LL);
    out[2 * (int64_t)blockIdx.x + 1] = n;
  }
}

constexpr int kWin = 11, kTile = 32, kIn = kTile + kWin - 1, kInStride = kIn + 1, kRowStride = kTile + 1, kRun = 4;
struct SsimWindow { float g[kWin]; };

// mask[image][pixel] = 1 where hr's pixel is data, from one pass over hr: blockIdx.y = image, a thread takes V consecutive pixels
// of all bands (V = 4: hw % 4 == 0 and a 16-byte aligned hr; the mask rows are then 4-byte aligned in the workspace).
template <int V>
__global__ __launch_bounds__(kThreads) void hr_mask_kernel(const float* __restrict__ hr, float nodata_value,
                                                           unsigned char* __restrict__ mask, int C, int64_t hw) {
  const float* hp = hr + (int64_t)blockIdx.y * C * hw;
  unsigned char* mp = mask + (int64_t)blockIdx.y * hw;
  const bool by_value = __builtin_isfinite(nodata_value);
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < hw / V; g += (int64_t)gridDim.x * kThreads) {
    bool nan[V], same[V];
#pragma unroll
    for (int p = 0; p < V; ++p) nan[p] = false, same[p] = true;
    for (int c = 0; c < C; ++c) {
      float v[V];
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(hp + c * hw + g * 4);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
        v[0] = hp[c * hw + g];
      }
#pragma unroll
      for (int p = 0; p < V; ++p) {
        nan[p] = nan[p] || is_nan(v[p]);
        same[p] = same[p] && v[p] == nodata_value;
      }
    }
    unsigned char ok[V];
#pragma unroll
    for (int p = 0; p < V; ++p) ok[p] = !(nan[p] || (by_value && same[p]));
    if constexpr (V == 4) {
      *reinterpret_cast<uchar4*>(mp + g * 4) = make_uchar4(ok[0], ok[1], ok[2], ok[3]);
    } else {
      mp[g] = ok[0];
    }
  }
}

// ssim_kernel (metrics.hip) over the window positions whose 11 x 11 pixels are all valid.  The block first stages the mask of
// its 42 x 42 input tile (hr_mask_kernel's bytes: one per pixel, shared by the bands' blocks), then takes the pivot from the
// tile's middle pixel, or - when that
// pixel is no-data - from the first valid pixel of the tile in row order; no-data pixels are staged as zeros in both images
// and reach counted positions never: a position is counted when the box sum of the mask over its window is 121.
__global__ __launch_bounds__(kThreads) void ssim_nodata_kernel(const float* __restrict__ sr, const float* __restrict__ hr,
                                                               const unsigned char* __restrict__ mask,
                                                               double* __restrict__ partials,
                                                               double* __restrict__ counts, SsimWindow win, int C, int H, int W,
                                                               int tiles_x, int clamp) {
  __shared__ float sx[kIn * kInStride], sy[kIn * kInStride];
  __shared__ float hm[5][kIn][kRowStride];
  __shared__ unsigned char sm[kIn * kInStride], hk[kIn][kRowStride + 3];
  __shared__ float red[kWaves];
  __shared__ int red_i[kWaves];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
  const int64_t plane = (int64_t)H * W;
  const float* xp = sr + ((int64_t)b * C + c) * plane;
  const float* yp = hr + ((int64_t)b * C + c) * plane;
  const unsigned char* mp = mask + (int64_t)b * plane;
  for (int i = tid; i < kIn * kIn; i += kThreads) {
    const int ly = i / kIn, lx = i % kIn, gy = ty0 + ly, gx = tx0 + lx;
    sm[ly * kInStride + lx] = gy < H && gx < W && mp[(int64_t)gy * W + gx] != 0;
  }
  __syncthreads();
  int py = min(ty0 + kIn / 2, H - 1) - ty0, px = min(tx0 + kIn / 2, W - 1) - tx0;
  if (!sm[py * kInStride + px]) {  // (the same for every thread of the block)
    int best = kIn * kIn;
    for (int i = tid; i < kIn * kIn; i += kThreads)
      if (sm[(i / kIn) * kInStride + i % kIn]) best = min(best, i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_down(best, o, 64));
    if (tid % 64 == 0) red_i[tid / 64] = best;
    __syncthreads();
    best = min(min(red_i[0], red_i[1]), min(red_i[2], red_i[3]));
    if (best < kIn * kIn) py = best / kIn, px = best % kIn;  // (no valid pixel: no position is counted, the pivot is not used)
  }
  const int64_t pivot = (int64_t)(ty0 + py) * W + tx0 + px;
  const float pvx = clamp ? clamp01(xp[pivot]) : xp[pivot], pvy = clamp ? clamp01(yp[pivot]) : yp[pivot];
  for (int i = tid; i < kIn * kIn; i += kThreads) {
    const int ly = i / kIn, lx = i % kIn, gy = ty0 + ly, gx = tx0 + lx;
    float a = 0.f, v = 0.f;
    if (sm[ly * kInStride + lx]) {  // (inside the image, and valid)
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
    int ms[kRun + kWin - 1];
#pragma unroll
    for (int k = 0; k < kRun + kWin - 1; ++k) {
      xs[k] = sx[r * kInStride + q + k];
      ys[k] = sy[r * kInStride + q + k];
      ms[k] = sm[r * kInStride + q + k];
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
        valid += ms[o + k];
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) hm[j][r][q + o] = m[j];
      hk[r][q + o] = (unsigned char)valid;
    }
  }
  __syncthreads();
  constexpr int kRows = kTile * kTile / kThreads;
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
  int box[kRows];
  {
    int vals[kRows + kWin - 1];
#pragma unroll
    for (int k = 0; k < kRows + kWin - 1; ++k) vals[k] = hk[row0 + k][col];
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < kWin; ++k) s += vals[o + k];
      box[o] = s;
    }
  }
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  float acc = 0.f;
  int positions = 0;
#pragma unroll
  for (int o = 0; o < kRows; ++o) {
    if (ty0 + row0 + o > H - kWin || tx0 + col > W - kWin || box[o] != kWin * kWin) continue;
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
  acc = wave_sum_of(acc);
  positions = wave_sum_of(positions);
  __syncthreads();  // (red_i: the pivot search)
  if (tid % 64 == 0) {
    red[tid / 64] = acc;
    red_i[tid / 64] = positions;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    int n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[w], n += red_i[w];
    partials[((int64_t)b * C + c) * gridDim.x + blockIdx.x] = (double)s;
    if (c == 0) counts[(int64_t)b * gridDim.x + blockIdx.x] = (double)n;  // (the mask is the bands' own: one count per tile)
  }
}

SsimWindow ssim_window() {  // (metrics.hip)
  double g[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) sum += g[k] = std::exp(-(k - kWin / 2) * (k - kWin / 2) / (2.0 * 1.5 * 1.5));
  SsimWindow w;
  for (int k = 0; k < kWin; ++k) w.g[k] = (float)(g[k] / sum);
  return w;
}

int pointwise_blocks(int64_t hw, int V) {  // (metrics.hip: the same blocks, so the same partial sums)
  const int64_t b = (hw / V + 2 * kThreads - 1) / (2 * kThreads);
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}
int64_t ssim_tiles(int H, int W) { return (int64_t)drs_cdiv(H - kWin + 1, kTile) * drs_cdiv(W - kWin + 1, kTile); }
bool shape_ok(int B, int C, int H, int W, int side) {
  return B >= 1 && B <= 65535 && C >= 1 && C <= kMaxBands && H >= side && W >= side;
}

template <int V>
void launch_pointwise(const float* sr, const float* hr, float nodata_value, double* ws, int B, int C, int64_t hw, int clamp,
                      int nb, hipStream_t s) {
  if (C <= 4) {
    DRS_LAUNCH((metrics_pointwise_nodata_kernel<V, 4>), dim3(nb, B), dim3(kThreads), 0, s, sr, hr, nodata_value, ws, C, hw, clamp);
  } else {
    DRS_LAUNCH((metrics_pointwise_nodata_kernel<V, kMaxBands>), dim3(nb, B), dim3(kThreads), 0, s, sr, hr, nodata_value, ws, C, hw,
               clamp);
  }
}

}  // namespace

extern "C" int drs_noise_target_nodata(const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                                       int noise_steps, int kind, float nodata_value, float fill, float* x_t, float* target,
                                       uint8_t* valid, int n, int C, int64_t hw, drs_stream_t stream) {
  DRS_REQUIRE(x0 && eps && t && alpha_hat && x_t && target && valid, DRS_ERR_ARG, "noise_target_nodata: null pointer");
  DRS_REQUIRE(x_t != target, DRS_ERR_ARG, "noise_target_nodata: x_t and target are one buffer");
  DRS_REQUIRE(kind == DRS_PRED_EPS || kind == DRS_PRED_V || kind == DRS_PRED_X0, DRS_ERR_ARG,
              "noise_target_nodata: kind=%d is none of DRS_PRED_EPS, DRS_PRED_V, DRS_PRED_X0", kind);
  DRS_REQUIRE(1 <= C && C <= kMaxBands, DRS_ERR_SHAPE, "noise_target_nodata: C=%d outside 1 .. %d", C, kMaxBands);
  DRS_REQUIRE(n >= 0 && hw >= 0 && noise_steps > 0, DRS_ERR_SHAPE, "noise_target_nodata: n=%d hw=%lld noise_steps=%d", n,
              (long long)hw, noise_steps);
  if (n == 0 || hw == 0) return DRS_OK;
  NoiseNodataArgs a;
  a.x0 = x0; a.eps = eps; a.t = t; a.alpha_hat = alpha_hat; a.xt = x_t; a.target = target; a.valid = valid;
  a.n = n; a.C = C; a.noise_steps = noise_steps; a.kind = kind; a.nodata_value = nodata_value; a.fill = fill; a.hw = hw;
  // every plane of every image starts on a 16-byte boundary, every image's mask row on a 4-byte one
  const bool wide = hw % 4 == 0 && ((uintptr_t)x0 | (uintptr_t)eps | (uintptr_t)x_t | (uintptr_t)target) % 16 == 0 &&
                    (uintptr_t)valid % 4 == 0;
  if (wide) launch_noise<4>(a, (hipStream_t)stream);
  else launch_noise<1>(a, (hipStream_t)stream);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_diffusion_loss_masked(const float* pred, const float* target, const uint8_t* valid, const int64_t* t, int B,
                                         int C, int64_t hw, const float* table, int T, const float* sample_w, int kind,
                                         double delta, float* grad, double* per_image, int64_t* counts, double* partials,
                                         double* out, double* bins, int nbins, int history, int update_ring, int64_t* bad_t,
                                         drs_stream_t stream) {
  DRS_REQUIRE(pred && target && valid && per_image && counts && partials && out, DRS_ERR_ARG,
              "diffusion_loss_masked: null pointer");
  DRS_REQUIRE(kind == DRS_LOSS_MSE || kind == DRS_LOSS_MAE || kind == DRS_LOSS_HUBER, DRS_ERR_ARG,
              "diffusion_loss_masked: unknown kind %d", kind);
  DRS_REQUIRE(kind != DRS_LOSS_HUBER || delta > 0.0, DRS_ERR_ARG, "diffusion_loss_masked: Huber needs delta > 0, got %g", delta);
  DRS_REQUIRE(1 <= B && B <= 65535 && 1 <= C && C <= kMaxBands && hw >= 1, DRS_ERR_SHAPE,
              "diffusion_loss_masked: need 1 <= B <= 65535, 1 <= C <= %d and hw >= 1, got B=%d C=%d hw=%lld", kMaxBands, B, C,
              (long long)hw);
  DRS_REQUIRE(!(table || bins) || (t && T >= 1), DRS_ERR_ARG,
              "diffusion_loss_masked: a table or bins need t and T >= 1, got T=%d", T);
  if (bins) {
    DRS_REQUIRE(2 <= nbins && nbins <= kMaxBins && nbins <= T / 2, DRS_ERR_ARG,
                "diffusion_loss_masked: need 2 <= nbins <= 64 and nbins <= T / 2, got nbins=%d T=%d", nbins, T);
    DRS_REQUIRE(1 <= history && history <= kMaxHistory, DRS_ERR_ARG, "diffusion_loss_masked: history=%d outside 1 .. 32", history);
  }
  const int64_t n = (int64_t)C * hw;
  DRS_REQUIRE(n / kChunk + 1 < (1LL << 31) / 256, DRS_ERR_SHAPE, "diffusion_loss_masked: C hw=%lld is too large", (long long)n);
  const int chunks = (int)((n + 3) / kChunk + 1);
  const dim3 grid(chunks, B);
  hipStream_t s = (hipStream_t)stream;
  long long* cnt = (long long*)counts;
  DRS_LAUNCH(valid_count_kernel, dim3(B), dim3(kThreads), 0, s, valid, hw, cnt);
  DRS_CHECK_HIP(hipGetLastError());
  if (kind == DRS_LOSS_MSE)
    launch_masked_loss<DRS_LOSS_MSE>(grid, s, pred, target, valid, t, B, C, hw, table, T, sample_w, delta, cnt, grad, partials);
  if (kind == DRS_LOSS_MAE)
    launch_masked_loss<DRS_LOSS_MAE>(grid, s, pred, target, valid, t, B, C, hw, table, T, sample_w, delta, cnt, grad, partials);
  if (kind == DRS_LOSS_HUBER)
    launch_masked_loss<DRS_LOSS_HUBER>(grid, s, pred, target, valid, t, B, C, hw, table, T, sample_w, delta, cnt, grad, partials);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(diffusion_loss_masked_finish_kernel, dim3(1), dim3(kFinThreads), 0, s, partials, cnt, chunks, B, C,
             (const long long*)t, table, T, sample_w, per_image, out, bins, nbins, history, update_ring, (long long*)bad_t);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API size_t drs_metrics_nodata_workspace_bytes(int B, int C, int H, int W) {
  if (!shape_ok(B, C, H, W, 1)) return 0;
  size_t rows = (size_t)pointwise_blocks((int64_t)H * W, 1) * (2 * C + 3);
  if (H >= kWin && W >= kWin && (size_t)(C + 1) * ssim_tiles(H, W) > rows) rows = (size_t)(C + 1) * ssim_tiles(H, W);
  return (size_t)B * rows * sizeof(double) + (size_t)B * H * W;  // (the partial rows, then drs_ssim_nodata's mask bytes)
}

extern "C" DRS_API int drs_metrics_pointwise_nodata(const float* sr, const float* hr, float nodata_value, double* out, int B,
                                                    int C, int H, int W, int clamp, void* workspace, size_t workspace_bytes,
                                                    drs_stream_t stream) {
  DRS_REQUIRE(sr && hr && out && workspace, DRS_ERR_ARG, "metrics_pointwise_nodata: null pointer");
  DRS_REQUIRE(shape_ok(B, C, H, W, 1), DRS_ERR_SHAPE, "metrics_pointwise_nodata: B=%d C=%d H=%d W=%d (1 <= C <= %d)", B, C, H, W,
              kMaxBands);
  const int64_t hw = (int64_t)H * W;
  const bool wide = hw % 4 == 0 && ((uintptr_t)sr | (uintptr_t)hr) % 16 == 0;
  const int nb = pointwise_blocks(hw, wide ? 4 : 1), K = 2 * C + 3;
  DRS_REQUIRE(workspace_bytes >= (size_t)B * nb * K * sizeof(double), DRS_ERR_WORKSPACE,
              "metrics_pointwise_nodata: workspace of %zu bytes, %zu needed", workspace_bytes,
              (size_t)B * nb * K * sizeof(double));
  double* ws = (double*)workspace;
  if (wide) launch_pointwise<4>(sr, hr, nodata_value, ws, B, C, hw, clamp, nb, (hipStream_t)stream);
  else launch_pointwise<1>(sr, hr, nodata_value, ws, B, C, hw, clamp, nb, (hipStream_t)stream);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(nodata_reduce_kernel, dim3(K, B), dim3(kThreads), 0, (hipStream_t)stream, ws, out, (int64_t)nb, K);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API int drs_ssim_nodata(const float* sr, const float* hr, float nodata_value, double* out, int B, int C, int H,
                                       int W, int clamp, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  DRS_REQUIRE(sr && hr && out && workspace, DRS_ERR_ARG, "ssim_nodata: null pointer");
  DRS_REQUIRE(shape_ok(B, C, H, W, kWin), DRS_ERR_SHAPE, "ssim_nodata: B=%d C=%d H=%d W=%d (1 <= C <= %d, H and W >= %d)", B, C,
              H, W, kMaxBands, kWin);
  const int64_t tiles = ssim_tiles(H, W);
  DRS_REQUIRE(tiles <= INT32_MAX, DRS_ERR_SHAPE, "ssim_nodata: H=%d W=%d need more tiles than one launch holds", H, W);
  const int64_t hw = (int64_t)H * W;
  const size_t need = (size_t)B * (C + 1) * tiles * sizeof(double) + (size_t)B * hw;
  DRS_REQUIRE(workspace_bytes >= need, DRS_ERR_WORKSPACE, "ssim_nodata: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  double* ws = (double*)workspace;
  double* counts = ws + (size_t)B * C * tiles;
  unsigned char* mask = (unsigned char*)(counts + (size_t)B * tiles);
  const bool wide = hw % 4 == 0 && (uintptr_t)hr % 16 == 0 && (uintptr_t)mask % 4 == 0;
  const int V = wide ? 4 : 1;
  const dim3 mgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>((hw / V + kThreads - 1) / kThreads, 1024)), B);
  if (wide) DRS_LAUNCH(hr_mask_kernel<4>, mgrid, dim3(kThreads), 0, (hipStream_t)stream, hr, nodata_value, mask, C, hw);
  else DRS_LAUNCH(hr_mask_kernel<1>, mgrid, dim3(kThreads), 0, (hipStream_t)stream, hr, nodata_value, mask, C, hw);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(ssim_nodata_kernel, dim3((unsigned)tiles, C, B), dim3(kThreads), 0, (hipStream_t)stream, sr, hr, mask, ws,
             counts, ssim_window(), C, H, W, drs_cdiv(W - kWin + 1, kTile), clamp);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(ssim_nodata_reduce_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, ws, counts, out, C, tiles);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
