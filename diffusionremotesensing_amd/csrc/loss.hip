// The training objective on the device (include/drs_hip.h: drs_diffusion_loss, drs_timestep_draw): loss value, gradient and
// per-image losses from ONE pass over (pred, target) - two reads, one write, 16 bytes per lane - a small ordered finish on
// the same stream, and the loss-aware timestep draw that reads the finish's ring.  No host synchronisation anywhere.
//
// Reduction order (what makes two calls agree bit for bit), as in optim.hip: a thread adds its 16 elements in element order;
// 64 lanes are combined by a shuffle tree (offsets 32, 16, .. 1); the four wave sums are added in wave order through LDS; the
// finish combines an image's chunk partials the same way (a lane adds chunks l, l + 64, ... in that order, then the shuffle
// tree), then adds the images' weighted losses in batch order.  No atomics, no fences: the finish is a second launch.
#include "drs_common.h"

constexpr int kChunk = 4096;         // elements per block of the streaming pass: 256 threads x 4 groups of 4
constexpr int kGroups = 4;           // 16-byte groups per thread
constexpr int kFinThreads = 1024;    // the finish: one block of 16 waves, one wave per image
constexpr int kMaxBins = 64, kMaxHistory = 32;

__device__ __forceinline__ int row_misalignment(const float* p) { return (int)(((uintptr_t)p >> 2) & 3u); }

// w_b = table[t_b] * sample_w[b] in double (missing factors are 1); a t_b outside [0, T) with a table gives NaN, not a read.
__device__ __forceinline__ double image_weight(const float* table, int T, long long tb, const float* sample_w, int b) {
  double w = 1.0;
  if (table) w = (tb >= 0 && tb < T) ? (double)table[tb] : __longlong_as_double(0x7ff8000000000000LL);
  if (sample_w) w = __dmul_rn(w, (double)sample_w[b]);
  return w;
}

// One element: adds l(d) to `s` in double, returns coef * l'(d).  `coef` = (float)(w_b * c / (B n)) with c = 2 for MSE and 1
// otherwise; `coef_delta` = (float)(w_b * delta / (B n)) (Huber's outer branch: its product with the sign is exact).
template <int KIND>
__device__ __forceinline__ float loss_element(float p, float q, double delta, float coef, float coef_delta, double& s) {
  const float d = __fsub_rn(p, q);
  const double dd = (double)d;
  const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : d;  // sign(d): +-0 and NaN stay what they are (torch.sign)
  if (KIND == DRS_LOSS_MSE) {
    s = __dadd_rn(s, __dmul_rn(dd, dd));
    return __fmul_rn(coef, d);
  }
  const double ad = fabs(dd);
  if (KIND == DRS_LOSS_MAE) {
    s = __dadd_rn(s, ad);
    return __fmul_rn(coef, sg);
  }
  const bool outer = ad > delta;  // torch.huber_loss: 0.5 d^2 for |d| < delta, delta (|d| - 0.5 delta) otherwise (equal at |d| == delta)
  s = __dadd_rn(s, outer ? __dmul_rn(delta, __dsub_rn(ad, __dmul_rn(0.5, delta))) : __dmul_rn(0.5, __dmul_rn(ad, ad)));
  return outer ? __fmul_rn(coef_delta, sg) : __fmul_rn(coef, d);
}

// Grid (chunks, B).  A row's elements are addressed on the 16-byte grid of its own start address (virtual index = element
// index + the start's misalignment in floats), so every whole group is one aligned float4 whatever n is; the groups cut by the
// row's two ends, and every group when the three tensors' rows are misaligned differently, go element by element.
template <int KIND, bool GRAD>
__global__ __launch_bounds__(256) void diffusion_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const long long* __restrict__ t, long long n,
                                                             const float* __restrict__ table, int T,
                                                             const float* __restrict__ sample_w, double delta, double scale,
                                                             float* __restrict__ grad, double* __restrict__ partials) {
  const int b = blockIdx.y;
  const float* p = pred + (long long)b * n;
  const float* q = target + (long long)b * n;
  float* g = GRAD ? grad + (long long)b * n : nullptr;
  const int mp = row_misalignment(p);
  const bool vec = mp == row_misalignment(q) && (!GRAD || mp == row_misalignment(g));
  const int mis = vec ? mp : 0;
  float coef = 0.f, coef_delta = 0.f;
  if (GRAD) {
    const double w = image_weight(table, T, table ? t[b] : 0, sample_w, b);
    coef = (float)__dmul_rn(w, KIND == DRS_LOSS_MSE ? 2.0 * scale : scale);  // (2 * scale is exact)
    coef_delta = (float)__dmul_rn(w, delta * scale);
  }
  float pv[kGroups][4], qv[kGroups][4];
  long long first[kGroups];
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const long long i = 4 * ((long long)blockIdx.x * (kChunk / 4) + threadIdx.x + 256 * k) - mis;  // the group's first element
    first[k] = i;
    if (vec && i >= 0 && i + 4 <= n) {
      const float4 a = *reinterpret_cast<const float4*>(p + i), c = *reinterpret_cast<const float4*>(q + i);
      pv[k][0] = a.x, pv[k][1] = a.y, pv[k][2] = a.z, pv[k][3] = a.w;
      qv[k][0] = c.x, qv[k][1] = c.y, qv[k][2] = c.z, qv[k][3] = c.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = i + e >= 0 && i + e < n;
        pv[k][e] = in ? p[i + e] : 0.f;  // (outside the row: d = 0 adds nothing, and nothing is stored)
        qv[k][e] = in ? q[i + e] : 0.f;
      }
    }
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const long long i = first[k];
    float gv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = loss_element<KIND>(pv[k][e], qv[k][e], delta, coef, coef_delta, s);
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
  __shared__ double wave_sum[4];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(long long)b * gridDim.x + blockIdx.x] =
        __dadd_rn(__dadd_rn(__dadd_rn(wave_sum[0], wave_sum[1]), wave_sum[2]), wave_sum[3]);
}

// One block of 16 waves.  Images are taken 1024 at a time: thread i forms image i's weight and bin; wave w adds the chunk
// partials of images w, w + 16, ... - lane l those of chunks l, l + 64, ... in that order, then the shuffle tree of pass one -
// with an image's loads issued together (the sum is a few additions; what it would wait for is one L2 round trip per load).
// Then the batch is walked in order by nbins + 1 threads at once: thread k < nbins keeps bin k (sum, count and ring position in
// registers), thread 64 - another wave - the weighted sum and the two counters.
__global__ __launch_bounds__(kFinThreads) void diffusion_loss_finish_kernel(
    const double* __restrict__ partials, int chunks, int B, long long n, const long long* __restrict__ t,
    const float* __restrict__ table, int T, const float* __restrict__ sample_w, double* __restrict__ per_image,
    double* __restrict__ out, double* __restrict__ bins, int nbins, int history, int update_ring,
    long long* __restrict__ bad_t) {
  __shared__ double image_loss[kFinThreads], weight[kFinThreads];
  __shared__ int image_bin[kFinThreads];  // >= 0: the bin, -1: no bins, -2: t outside [0, T)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool uses_t = table || bins;
  const bool bin_thread = bins && tid < nbins;
  double bin_sum = 0.0;
  long long bin_count = 0, bin_appended = 0;
  int ring_pos = 0;
  double* ring = nullptr;
  if (bin_thread) {  // (the int64 words are moved as bits)
    bin_sum = bins[tid];
    bin_count = __double_as_longlong(bins[nbins + tid]);
    bin_appended = __double_as_longlong(bins[2 * nbins + tid]);
    ring_pos = (int)((bin_appended % history + history) % history);  // inside the ring whatever the word holds
    ring = bins + 3 * nbins + 1 + tid * history;
  }
  double S = 0.0;
  long long bad = 0, nonfinite = 0;
  for (int b0 = 0; b0 < B; b0 += kFinThreads) {
    const int nb = min(kFinThreads, B - b0);
    __syncthreads();  // (the previous tile's walk)
    if (tid < nb) {
      const int b = b0 + tid;
      const long long tv = uses_t ? t[b] : 0;
      const bool in_range = tv >= 0 && tv < T;
      weight[tid] = image_weight(table, T, tv, sample_w, b);
      image_bin[tid] = !uses_t || in_range ? (bins ? (int)(tv * nbins / T) : -1) : -2;
    }
    for (int i = wave; i < nb; i += kFinThreads / 64) {
      const double* row = partials + (long long)(b0 + i) * chunks;
      double s = 0.0;
      for (int j0 = 0; j0 < chunks; j0 += 256) {
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = j0 + lane + 64 * k;
          r[k] = j < chunks ? row[j] : 0.0;  // (a missing term adds nothing)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s = __dadd_rn(s, r[k]);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s = __dadd_rn(s, __shfl_down(s, off, 64));
      if (lane == 0) {
        const double v = s / (double)n;
        per_image[b0 + i] = v;
        image_loss[i] = v;
      }
    }
    __syncthreads();
    if (bin_thread) {
      for (int i = 0; i < nb; ++i) {
        const double v = image_loss[i];
        if (image_bin[i] != tid || !isfinite(v)) continue;
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
        const double v = image_loss[i];
        S = __dadd_rn(S, __dmul_rn(weight[i], v));
        bad += image_bin[i] == -2;
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
    const double loss = S / (double)B;
    out[0] = loss;
    reinterpret_cast<float*>(out)[2] = (float)loss;
    if (nonfinite) bins[3 * nbins] = __longlong_as_double(__double_as_longlong(bins[3 * nbins]) + nonfinite);
    if (bad && bad_t) *bad_t += bad;
  }
}

static int check_bins(const char* what, const void* bins, int T, int nbins, int history) {
  if (!bins) return DRS_OK;
  DRS_REQUIRE(2 <= nbins && nbins <= kMaxBins && nbins <= T / 2, DRS_ERR_ARG,
              "%s: need 2 <= nbins <= 64 and nbins <= T / 2, got nbins=%d T=%d", what, nbins, T);
  DRS_REQUIRE(1 <= history && history <= kMaxHistory, DRS_ERR_ARG, "%s: history=%d outside 1 .. 32", what, history);
  return DRS_OK;
}

template <int KIND>
static void launch_loss(dim3 grid, hipStream_t s, const float* pred, const float* target, const int64_t* t, int64_t n,
                        const float* table, int T, const float* sample_w, double delta, double scale, float* grad,
                        double* partials) {
  if (grad)
    DRS_LAUNCH((diffusion_loss_kernel<KIND, true>), grid, dim3(256), 0, s, pred, target, (const long long*)t, (long long)n,
               table, T, sample_w, delta, scale, grad, partials);
  else
    DRS_LAUNCH((diffusion_loss_kernel<KIND, false>), grid, dim3(256), 0, s, pred, target, (const long long*)t, (long long)n,
               table, T, sample_w, delta, scale, grad, partials);
}

extern "C" int drs_diffusion_loss(const float* pred, const float* target, const int64_t* t, int B, int64_t n,
                                  const float* table, int T, const float* sample_w, int kind, double delta, float* grad,
                                  double* per_image, double* partials, double* out, double* bins, int nbins, int history,
                                  int update_ring, int64_t* bad_t, drs_stream_t stream) {
  DRS_REQUIRE(pred && target && per_image && partials && out, DRS_ERR_ARG, "diffusion_loss: null pointer");
  DRS_REQUIRE(kind == DRS_LOSS_MSE || kind == DRS_LOSS_MAE || kind == DRS_LOSS_HUBER, DRS_ERR_ARG,
              "diffusion_loss: unknown kind %d", kind);
  DRS_REQUIRE(kind != DRS_LOSS_HUBER || delta > 0.0, DRS_ERR_ARG, "diffusion_loss: Huber needs delta > 0, got %g", delta);
  DRS_REQUIRE(1 <= B && B <= 65535 && n >= 1, DRS_ERR_SHAPE, "diffusion_loss: need 1 <= B <= 65535 and n >= 1, got B=%d n=%lld",
              B, (long long)n);
  DRS_REQUIRE(n / kChunk + 1 < (1LL << 31) / 256, DRS_ERR_SHAPE, "diffusion_loss: n=%lld is too large", (long long)n);
  DRS_REQUIRE(!(table || bins) || (t && T >= 1), DRS_ERR_ARG, "diffusion_loss: a table or bins need t and T >= 1, got T=%d", T);
  if (int st = check_bins("diffusion_loss", bins, T, nbins, history)) return st;
  const int chunks = (int)((n + 3) / kChunk + 1);  // covers the row on the grid of its start address (up to 3 floats in front)
  const double scale = 1.0 / ((double)B * (double)n);
  const dim3 grid(chunks, B);
  hipStream_t s = (hipStream_t)stream;
  if (kind == DRS_LOSS_MSE) launch_loss<DRS_LOSS_MSE>(grid, s, pred, target, t, n, table, T, sample_w, delta, scale, grad, partials);
  if (kind == DRS_LOSS_MAE) launch_loss<DRS_LOSS_MAE>(grid, s, pred, target, t, n, table, T, sample_w, delta, scale, grad, partials);
  if (kind == DRS_LOSS_HUBER)
    launch_loss<DRS_LOSS_HUBER>(grid, s, pred, target, t, n, table, T, sample_w, delta, scale, grad, partials);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(diffusion_loss_finish_kernel, dim3(1), dim3(kFinThreads), 0, s, partials, chunks, B, (long long)n, (const long long*)t,
             table, T, sample_w, per_image, out, bins, nbins, history, update_ring, (long long*)bad_t);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// Every block forms the proposal from the ring on its own (nbins <= 64 terms, in double, in index order: all blocks hold the
// same bits), then one thread per sample.
__global__ __launch_bounds__(256) void timestep_draw_kernel(const double* __restrict__ bins, int nbins, int history,
                                                            const float* __restrict__ u1, const float* __restrict__ u2, int B,
                                                            int T, double eps, long long* __restrict__ t_out,
                                                            float* __restrict__ w_out) {
  __shared__ double r[kMaxBins], p[kMaxBins], cum[kMaxBins];
  __shared__ int all_full;
  const int tid = threadIdx.x;
  if (tid < nbins) {
    const bool full = __double_as_longlong(bins[2 * nbins + tid]) >= history;
    double s = 0.0;
    if (full)
      for (int j = 0; j < history; ++j) {
        const double v = bins[3 * nbins + 1 + tid * history + j];
        s = __dadd_rn(s, __dmul_rn(v, v));
      }
    r[tid] = full ? sqrt(s / (double)history) : -1.0;
  }
  __syncthreads();
  if (tid == 0) {
    bool full = true;
    double sum = 0.0;
    for (int k = 0; k < nbins; ++k) {
      full = full && r[k] >= 0.0;
      sum = __dadd_rn(sum, r[k]);
    }
    all_full = full;
    double c = 0.0;
    for (int k = 0; k < nbins && full; ++k) {
      // (rings of zeros: nothing to prefer)
      p[k] = sum > 0.0 ? __dadd_rn(__dmul_rn(1.0 - eps, r[k] / sum), eps / (double)nbins) : 1.0 / (double)nbins;
      c = __dadd_rn(c, p[k]);
      cum[k] = c;
    }
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + tid;
  if (i >= B) return;
  if (!all_full) {
    t_out[i] = 1 + min((long long)(T - 2), (long long)floor((double)u1[i] * (double)(T - 1)));
    w_out[i] = 1.f;
    return;
  }
  const double a = (double)u1[i];
  int k = 0;
  while (k < nbins - 1 && !(cum[k] > a)) ++k;
  // bin k holds the timesteps ceil(k T / nbins) .. ceil((k + 1) T / nbins) - 1; t = 0 is not drawn
  const long long lo = max(1LL, ((long long)k * T + nbins - 1) / nbins), hi = ((long long)(k + 1) * T + nbins - 1) / nbins;
  const long long cnt = hi - lo;
  t_out[i] = lo + min(cnt - 1, (long long)floor((double)u2[i] * (double)cnt));
  w_out[i] = (float)((double)cnt / ((double)(T - 1) * p[k]));
}

extern "C" int drs_timestep_draw(const double* bins, int nbins, int history, const float* u1, const float* u2, int B, int T,
                                 double eps_uniform, int64_t* t, float* sample_w, drs_stream_t stream) {
  DRS_REQUIRE(bins && u1 && u2 && t && sample_w, DRS_ERR_ARG, "timestep_draw: null pointer");
  DRS_REQUIRE(B >= 1, DRS_ERR_SHAPE, "timestep_draw: B=%d", B);
  DRS_REQUIRE(eps_uniform >= 0.0 && eps_uniform <= 1.0, DRS_ERR_ARG, "timestep_draw: eps_uniform=%g outside [0, 1]", eps_uniform);
  if (int st = check_bins("timestep_draw", bins, T, nbins, history)) return st;
  DRS_LAUNCH(timestep_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, bins, nbins, history, u1, u2, B, T,
             eps_uniform, (long long*)t, sample_w);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
