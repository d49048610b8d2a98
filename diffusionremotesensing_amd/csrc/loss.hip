// The training objective on the device (include/drs_hip.h: drs_diffusion_loss, drs_timestep_draw): loss value, gradient and
// per-image losses from ONE pass over (pred, target) - two reads, one write, 16 bytes per lane - a small ordered finish on
// the same stream, and the loss-aware timestep draw that reads the finish's ring.  No host synchronisation anywhere.
//
// Reduction order (what makes two calls agree bit for bit), as in optim.hip: a thread adds its 16 elements in element order;
// 64 lanes are combined by a shuffle tree (offsets 32, 16, .. 1); the four wave sums are added in wave order through LDS; the
// finish combines an image's chunk partials the same way (a lane adds chunks l, l + 64, ... in that order, then the shuffle
// tree), then adds the images' weighted losses in batch order.  No atomics, no fences: the finish is a second launch.
//
// drs_diffusion_loss_masked is the MASKED instance of the same two kernels behind a count of every
// image's valid pixels: a no-data element is SELECTED out - it adds nothing and its gradient is +0.0 - so a mask without a
// no-data pixel gives the unmasked entry's bits.
#include "drs_common.h"

constexpr int kThreads = 256, kWaves = kThreads / 64;
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
// MASKED: element i of a row belongs to pixel i % hw.  The four decisions of a group are one 32-bit load where the group lies
// inside one band and its mask bytes are 4-byte aligned, four byte loads otherwise.  A no-data element's pred and target are
// loaded but never used.  The coefficient needs Bv (the images with a valid pixel) and n_b = C nv_b instead of `scale`: every
// block counts Bv from `counts` itself.
struct LossMask {
  const unsigned char* valid;  // [B][hw], non-zero = data
  const long long* counts;     // [B]: valid_count_kernel's
  long long hw;
  int B, C;
};

template <int KIND, bool GRAD, bool MASKED>
__global__ __launch_bounds__(256) void diffusion_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const long long* __restrict__ t, long long n,
                                                             const float* __restrict__ table, int T,
                                                             const float* __restrict__ sample_w, double delta, double scale,
                                                             float* __restrict__ grad, double* __restrict__ partials,
                                                             const LossMask mask) {
  const int b = blockIdx.y;
  const float* p = pred + (long long)b * n;
  const float* q = target + (long long)b * n;
  float* g = GRAD ? grad + (long long)b * n : nullptr;
  const int mp = row_misalignment(p);
  const bool vec = mp == row_misalignment(q) && (!GRAD || mp == row_misalignment(g));
  const int mis = vec ? mp : 0;
  float coef = 0.f, coef_delta = 0.f;
  if (GRAD) {
    double image_scale = scale;  // 1 / (B n); MASKED: 1 / (Bv n_b)
    if constexpr (MASKED) {
      __shared__ int wave_images[kWaves];
      int images = 0;
      for (int i = threadIdx.x; i < mask.B; i += kThreads) images += mask.counts[i] > 0;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) images += __shfl_down(images, off, 64);
      if ((threadIdx.x & 63) == 0) wave_images[threadIdx.x >> 6] = images;
      __syncthreads();
      const int Bv = wave_images[0] + wave_images[1] + wave_images[2] + wave_images[3];
      // An image without a valid pixel (nv_b = 0) gets 1 / 0 here and a non-finite coef: every one of its elements is selected
      // out below, so no element takes it.  (A guard around it costs nothing in time but moves the instance off the register
      // budget - and the occupancy - DESIGN.md section 27 records for it.)
      image_scale = 1.0 / ((double)Bv * (double)((long long)mask.C * mask.counts[b]));
    }
    const double w = image_weight(table, T, table ? t[b] : 0, sample_w, b);
    coef = (float)__dmul_rn(w, KIND == DRS_LOSS_MSE ? 2.0 * image_scale : image_scale);  // (2 * scale is exact)
    coef_delta = (float)__dmul_rn(w, delta * image_scale);
  }
  float pv[kGroups][4], qv[kGroups][4];
  bool ok[kGroups][4];  // MASKED only
  long long first[kGroups];
  long long pix = 0;  // MASKED only: the pixel of the group's first element
  if constexpr (MASKED) {
    pix = (4 * ((long long)blockIdx.x * (kChunk / 4) + threadIdx.x) - mis) % mask.hw;
    if (pix < 0) pix += mask.hw;  // (of element -mis .. -1: counted back from the row's end)
  }
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
    if constexpr (MASKED) {
      const unsigned char* m = mask.valid + (long long)b * mask.hw;
      if (vec && i >= 0 && i + 4 <= n && pix + 4 <= mask.hw && (((uintptr_t)(m + pix)) & 3u) == 0) {
        const unsigned four = *reinterpret_cast<const unsigned*>(m + pix);
        ok[k][0] = (four & 0xffu) != 0, ok[k][1] = (four & 0xff00u) != 0;
        ok[k][2] = (four & 0xff0000u) != 0, ok[k][3] = (four & 0xff000000u) != 0;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          long long at = pix + e;
          if (at >= mask.hw) at %= mask.hw;
          ok[k][e] = i + e >= 0 && i + e < n && m[at] != 0;  // (outside the row: nothing is read, added or stored)
        }
      }
      pix += 4 * kThreads;
      if (pix >= mask.hw) pix = mask.hw > 4 * kThreads ? pix - mask.hw : pix % mask.hw;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kGroups; ++k) {
    const long long i = first[k];
    float gv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (MASKED) {
        gv[e] = 0.f;
        if (!ok[k][e]) continue;
      }
      gv[e] = loss_element<KIND>(pv[k][e], qv[k][e], delta, coef, coef_delta, s);
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
  __shared__ double wave_sum[4];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(long long)b * gridDim.x + blockIdx.x] =
        __dadd_rn(__dadd_rn(__dadd_rn(wave_sum[0], wave_sum[1]), wave_sum[2]), wave_sum[3]);
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

// One block of 16 waves.  Images are taken 1024 at a time: thread i forms image i's weight and bin; wave w adds the chunk
// partials of images w, w + 16, ... - lane l those of chunks l, l + 64, ... in that order, then the shuffle tree of pass one -
// with an image's loads issued together (the sum is a few additions; what it would wait for is one L2 round trip per load).
// Then the batch is walked in order by nbins + 1 threads at once: thread k < nbins keeps bin k (sum, count and ring position in
// registers), thread 64 - another wave - the weighted sum and the two counters.
// MASKED: over the images that have a valid pixel.  per_image divides by n_b = C counts[b] instead of n, the loss by Bv instead
// of B; an image without a valid pixel has per_image 0 and enters neither the loss, the bins nor the ring.
template <bool MASKED>
struct FinishMaskLds {};
template <>
struct FinishMaskLds<true> {
  long long elements[kFinThreads];  // n_b; 0: no valid pixel
};

template <bool MASKED>
__global__ __launch_bounds__(kFinThreads) void diffusion_loss_finish_kernel(
    const double* __restrict__ partials, int chunks, int B, long long n, const long long* __restrict__ t,
    const float* __restrict__ table, int T, const float* __restrict__ sample_w, double* __restrict__ per_image,
    double* __restrict__ out, double* __restrict__ bins, int nbins, int history, int update_ring,
    long long* __restrict__ bad_t, const long long* __restrict__ counts, int C) {
  __shared__ double image_loss[kFinThreads], weight[kFinThreads];
  __shared__ int image_bin[kFinThreads];  // >= 0: the bin, -1: no bins, -2: t outside [0, T)
  __shared__ FinishMaskLds<MASKED> ml;
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
  long long bad = 0, nonfinite = 0, Bv = 0;
  for (int b0 = 0; b0 < B; b0 += kFinThreads) {
    const int nb = min(kFinThreads, B - b0);
    __syncthreads();  // (the previous tile's walk)
    if (tid < nb) {
      const int b = b0 + tid;
      const long long tv = uses_t ? t[b] : 0;
      const bool in_range = tv >= 0 && tv < T;
      weight[tid] = image_weight(table, T, tv, sample_w, b);
      image_bin[tid] = !uses_t || in_range ? (bins ? (int)(tv * nbins / T) : -1) : -2;
      if constexpr (MASKED) ml.elements[tid] = (long long)C * counts[b];
    }
    if constexpr (MASKED) __syncthreads();  // (elements: read by the waves below)
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
        double v;
        if constexpr (MASKED) v = ml.elements[i] > 0 ? s / (double)ml.elements[i] : 0.0;
        else v = s / (double)n;
        per_image[b0 + i] = v;
        image_loss[i] = v;
      }
    }
    __syncthreads();
    if (bin_thread) {
      for (int i = 0; i < nb; ++i) {
        const double v = image_loss[i];
        if (image_bin[i] != tid || !isfinite(v)) continue;
        if constexpr (MASKED)
          if (ml.elements[i] == 0) continue;
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
        bad += image_bin[i] == -2;
        if constexpr (MASKED) {
          if (ml.elements[i] == 0) continue;
          ++Bv;
        }
        S = __dadd_rn(S, __dmul_rn(weight[i], v));
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
    const double loss = !MASKED ? S / (double)B : Bv > 0 ? S / (double)Bv : 0.0;
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

template <int KIND, bool MASKED>
static void launch_loss(dim3 grid, hipStream_t s, const float* pred, const float* target, const long long* t, long long n,
                        const float* table, int T, const float* sample_w, double delta, double scale, float* grad,
                        double* partials, const LossMask& mask) {
  if (grad)
    DRS_LAUNCH((diffusion_loss_kernel<KIND, true, MASKED>), grid, dim3(256), 0, s, pred, target, t, n, table, T, sample_w, delta,
               scale, grad, partials, mask);
  else
    DRS_LAUNCH((diffusion_loss_kernel<KIND, false, MASKED>), grid, dim3(256), 0, s, pred, target, t, n, table, T, sample_w, delta,
               scale, grad, partials, mask);
}

// The checks of both entries, under the entry's name `what`, in the order the unmasked entry always had: pointers (the entry's
// own), check_kind, the shape (the entry's own), then the rest in diffusion_loss.
static int check_kind(const char* what, int kind, double delta) {
  DRS_REQUIRE(kind == DRS_LOSS_MSE || kind == DRS_LOSS_MAE || kind == DRS_LOSS_HUBER, DRS_ERR_ARG, "%s: unknown kind %d", what,
              kind);
  DRS_REQUIRE(kind != DRS_LOSS_HUBER || delta > 0.0, DRS_ERR_ARG, "%s: Huber needs delta > 0, got %g", what, delta);
  return DRS_OK;
}

// What the two entries share after those: the remaining checks, then the launches.  n = C hw for the masked entry, whose scale
// is formed per image on the device.
template <bool MASKED>
static int diffusion_loss(const char* what, const float* pred, const float* target, const long long* t, int B, long long n,
                          const float* table, int T, const float* sample_w, int kind, double delta, float* grad,
                          double* per_image, double* partials, double* out, double* bins, int nbins, int history,
                          int update_ring, long long* bad_t, const LossMask& mask, hipStream_t s) {
  DRS_REQUIRE(n / kChunk + 1 < (1LL << 31) / 256, DRS_ERR_SHAPE, "%s: %s=%lld is too large", what, MASKED ? "C hw" : "n", n);
  DRS_REQUIRE(!(table || bins) || (t && T >= 1), DRS_ERR_ARG, "%s: a table or bins need t and T >= 1, got T=%d", what, T);
  if (int st = check_bins(what, bins, T, nbins, history)) return st;
  const int chunks = (int)((n + 3) / kChunk + 1);  // covers the row on the grid of its start address (up to 3 floats in front)
  const double scale = MASKED ? 0.0 : 1.0 / ((double)B * (double)n);
  const dim3 grid(chunks, B);
  if (MASKED) {
    DRS_LAUNCH(valid_count_kernel, dim3(B), dim3(kThreads), 0, s, mask.valid, (int64_t)mask.hw,
               const_cast<long long*>(mask.counts));
    DRS_CHECK_HIP(hipGetLastError());
  }
  if (kind == DRS_LOSS_MSE)
    launch_loss<DRS_LOSS_MSE, MASKED>(grid, s, pred, target, t, n, table, T, sample_w, delta, scale, grad, partials, mask);
  if (kind == DRS_LOSS_MAE)
    launch_loss<DRS_LOSS_MAE, MASKED>(grid, s, pred, target, t, n, table, T, sample_w, delta, scale, grad, partials, mask);
  if (kind == DRS_LOSS_HUBER)
    launch_loss<DRS_LOSS_HUBER, MASKED>(grid, s, pred, target, t, n, table, T, sample_w, delta, scale, grad, partials, mask);
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(diffusion_loss_finish_kernel<MASKED>, dim3(1), dim3(kFinThreads), 0, s, partials, chunks, B, n, t, table, T,
             sample_w, per_image, out, bins, nbins, history, update_ring, bad_t, mask.counts, mask.C);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_diffusion_loss(const float* pred, const float* target, const int64_t* t, int B, int64_t n,
                                  const float* table, int T, const float* sample_w, int kind, double delta, float* grad,
                                  double* per_image, double* partials, double* out, double* bins, int nbins, int history,
                                  int update_ring, int64_t* bad_t, drs_stream_t stream) {
  DRS_REQUIRE(pred && target && per_image && partials && out, DRS_ERR_ARG, "diffusion_loss: null pointer");
  if (int st = check_kind("diffusion_loss", kind, delta)) return st;
  DRS_REQUIRE(1 <= B && B <= 65535 && n >= 1, DRS_ERR_SHAPE, "diffusion_loss: need 1 <= B <= 65535 and n >= 1, got B=%d n=%lld",
              B, (long long)n);
  return diffusion_loss<false>("diffusion_loss", pred, target, (const long long*)t, B, n, table, T, sample_w, kind, delta, grad,
                               per_image, partials, out, bins, nbins, history, update_ring, (long long*)bad_t, LossMask{},
                               (hipStream_t)stream);
}

extern "C" int drs_diffusion_loss_masked(const float* pred, const float* target, const uint8_t* valid, const int64_t* t, int B,
                                         int C, int64_t hw, const float* table, int T, const float* sample_w, int kind,
                                         double delta, float* grad, double* per_image, int64_t* counts, double* partials,
                                         double* out, double* bins, int nbins, int history, int update_ring, int64_t* bad_t,
                                         drs_stream_t stream) {
  DRS_REQUIRE(pred && target && valid && per_image && counts && partials && out, DRS_ERR_ARG,
              "diffusion_loss_masked: null pointer");
  if (int st = check_kind("diffusion_loss_masked", kind, delta)) return st;
  DRS_REQUIRE(1 <= B && B <= 65535 && 1 <= C && C <= kMaxBands && hw >= 1, DRS_ERR_SHAPE,
              "diffusion_loss_masked: need 1 <= B <= 65535, 1 <= C <= %d and hw >= 1, got B=%d C=%d hw=%lld", kMaxBands, B, C,
              (long long)hw);
  const LossMask mask{valid, (const long long*)counts, hw, B, C};
  return diffusion_loss<true>("diffusion_loss_masked", pred, target, (const long long*)t, B, (long long)C * hw, table, T, sample_w,
                              kind, delta, grad, per_image, partials, out, bins, nbins, history, update_ring, (long long*)bad_t,
                              mask, (hipStream_t)stream);
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
