// Per-pixel statistics and scores of an ensemble of N samples of one conditional distribution (ensemble.py): the members
// are x of shape (N, B, C, H, W), member axis first, 2 <= N <= 32.  drs_ensemble_stats leaves the maps mean, std (unbiased)
// and up to 8 linearly interpolated quantiles; drs_ensemble_scores scores the members against a truth y (B, C, H, W): an
// optional per-pixel CRPS map, per image the sums of CRPS, variance and (mean - y)^2, and the rank histogram.
// Both read every member element once: lanes take consecutive pixels (each member row is a coalesced read, 16 bytes per
// lane where the element count and the alignment allow), the N values of a pixel live in registers and are sorted by a
// fully unrolled bitonic network over NP = the next power of two, the rows past N padded with +inf.  The sort and the
// comparisons are exact fp32; every sum, the interpolation and the CRPS are fp64 over the SORTED order (a permutation of
// the members changes no bit) and are rounded to fp32 once, at the store of a map.  The per-image sums take the fp64
// per-pixel values: fp64 per thread, wave and block, one partial row per block in the caller's workspace, and a second
// kernel that adds the rows of an image in a fixed order - no floating-point atomics, two calls return the same bits.
// The rank histogram is counted in integer LDS counters (integer counts do not depend on the order).
#include "drs_common.h"
#include <cmath>

// a / N - b / N^2 and s_k + f (s_k1 - s_k) are evaluated as written (q = 0 and q = 1 return min and max exactly either
// way; the float64 oracle restates the same operations)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxMembers = 32, kMaxQ = 8;
constexpr int kSums = 3;  // crps | variance | (mean - y)^2

// position of quantile j in the sorted members: s_k + frac (s_k1 - s_k), k1 = min(k + 1, N - 1); formed on the host in fp64
struct QuantileSpec {
  int k[kMaxQ], k1[kMaxQ];
  double frac[kMaxQ];
};

// torch.clamp(v, lo, hi): a NaN stays a NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clampf(float v, float lo, float hi) {
  return __builtin_elementwise_minimum(__builtin_elementwise_maximum(v, lo), hi);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0 holds the sum, always formed in the same order
}

constexpr int log2i(int n) { return n <= 1 ? 0 : 1 + log2i(n / 2); }

// Members i < N of the V pixels at element e, clamped; rows N .. NP - 1 are +inf.  bad[p]: pixel p holds a NaN member.
template <int NP, int V>
__device__ __forceinline__ void load_members(const float* __restrict__ x, int64_t stride, int64_t e, int N, int clamp,
                                             float lo, float hi, float (&s)[NP][V], bool (&bad)[V]) {
#pragma unroll
  for (int p = 0; p < V; ++p) bad[p] = false;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i < N) {
      if constexpr (V == 4) {
        const float4 a = *reinterpret_cast<const float4*>(x + i * stride + e);
        s[i][0] = a.x; s[i][1] = a.y; s[i][2] = a.z; s[i][3] = a.w;
      } else {
        s[i][0] = x[i * stride + e];
      }
#pragma unroll
      for (int p = 0; p < V; ++p) {
        if (clamp) s[i][p] = clampf(s[i][p], lo, hi);
        bad[p] |= s[i][p] != s[i][p];
      }
    } else {
#pragma unroll
      for (int p = 0; p < V; ++p) s[i][p] = INFINITY;
    }
  }
}

// Bitonic sorting network over the NP rows, ascending, every index a compile-time constant (all loops have constant trip
// counts and are unrolled: the rows stay in registers).  A pixel with a NaN is not sorted meaningfully; its outputs are NaN.
template <int NP, int V>
__device__ __forceinline__ void sort_members(float (&s)[NP][V]) {
  constexpr int L = log2i(NP);
#pragma unroll
  for (int kk = 1; kk <= L; ++kk) {
#pragma unroll
    for (int jj = L - 1; jj >= 0; --jj) {
      if (jj >= kk) continue;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int l = i ^ (1 << jj);
        if (l < i) continue;
        const bool up = (i & (1 << kk)) == 0;
#pragma unroll
        for (int p = 0; p < V; ++p) {
          const float a = s[i][p], b = s[l][p];
          const float mn = __builtin_fminf(a, b), mx = __builtin_fmaxf(a, b);
          s[i][p] = up ? mn : mx;
          s[l][p] = up ? mx : mn;
        }
      }
    }
  }
}

// s[k][p] for a wave-uniform runtime k, as an unrolled select chain over compile-time rows.  The selection is written on the
// bit patterns, (bits & mask) | acc with a scalar all-ones / zero mask per row: the compiler turns a chain of `k == i ?
// s[i][p] : v` back into ONE load at a runtime index, which moves the whole array into scratch memory.
template <int NP, int V>
__device__ __forceinline__ float pick(const float (&s)[NP][V], int p, int k) {
  unsigned bits = 0u;
#pragma unroll
  for (int i = 0; i < NP; ++i) bits |= __float_as_uint(s[i][p]) & (k == i ? 0xffffffffu : 0u);
  return __uint_as_float(bits);
}

// mean = sum(s) / N and ssq = sum (s_i - mean)^2 of pixel p, fp64 over the sorted order
template <int NP, int V>
__device__ __forceinline__ void moments(const float (&s)[NP][V], int p, int N, double& mean, double& ssq) {
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (i < N) sum += (double)s[i][p];
  mean = sum / (double)N;
  ssq = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (i < N) {
      const double d = (double)s[i][p] - mean;
      ssq += d * d;
    }
}

template <int V>
__device__ __forceinline__ void store_map(float* __restrict__ out, int64_t e, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(out + e) = float4{v[0], v[1], v[2], v[3]};
  } else {
    out[e] = v[0];
  }
}

// ---- maps ----------------------------------------------------------------------------------------------------------
// The grid strides over the groups of V consecutive elements of the `total` = B C H W elements of a member.
// V = 4 needs total % 4 == 0 and 16-byte aligned tensors: every member row then starts on a 16-byte boundary.
template <int NP, int V>
__global__ __launch_bounds__(kThreads) void ensemble_stats_kernel(const float* __restrict__ x, float* __restrict__ mean_out,
                                                                  float* __restrict__ std_out, float* __restrict__ q_out,
                                                                  QuantileSpec qs, int Q, int N, int64_t total, int clamp,
                                                                  float lo, float hi) {
  const int64_t groups = total / V;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
    const int64_t e = g * V;
    float s[NP][V];
    bool bad[V];
    load_members<NP, V>(x, total, e, N, clamp, lo, hi, s, bad);
    sort_members<NP, V>(s);
    if (mean_out || std_out) {
      float m[V], sd[V];
#pragma unroll
      for (int p = 0; p < V; ++p) {
        double mean, ssq;
        moments<NP, V>(s, p, N, mean, ssq);
        m[p] = bad[p] ? NAN : (float)mean;
        sd[p] = bad[p] ? NAN : (float)sqrt(ssq / (double)(N - 1));
      }
      if (mean_out) store_map<V>(mean_out, e, m);
      if (std_out) store_map<V>(std_out, e, sd);
    }
#pragma unroll
    for (int j = 0; j < kMaxQ; ++j) {
      if (j >= Q) continue;
      float r[V];
#pragma unroll
      for (int p = 0; p < V; ++p) {
        const double a = (double)pick<NP, V>(s, p, qs.k[j]), b = (double)pick<NP, V>(s, p, qs.k1[j]);
        r[p] = bad[p] ? NAN : (float)(a + qs.frac[j] * (b - a));
      }
      store_map<V>(q_out + j * total, e, r);
    }
  }
}

// ---- scores --------------------------------------------------------------------------------------------------------
// blockIdx.y = image, the x-grid strides over the groups of V consecutive elements of the chw = C H W elements of that
// image.  V = 4 needs chw % 4 == 0 and 16-byte aligned tensors.
// partials: [image][block][kSums + N + 1] 8-byte words = the three fp64 sums | the N + 1 rank counts as int64
template <int NP, int V>
__global__ __launch_bounds__(kThreads) void ensemble_scores_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                   float* __restrict__ crps_out, double* __restrict__ partials,
                                                                   int N, int64_t chw, int64_t member_stride, int clamp,
                                                                   float lo, float hi) {
  __shared__ double red[kSums][kWaves];
  __shared__ unsigned hist[kMaxMembers + 1];
  if (threadIdx.x <= kMaxMembers) hist[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.y * chw, groups = chw / V;
  double acc[kSums] = {0.0, 0.0, 0.0};
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kThreads) {
    const int64_t e = base + g * V;
    float s[NP][V], t[V], c[V];
    bool bad[V];
    load_members<NP, V>(x, member_stride, e, N, clamp, lo, hi, s, bad);
    if constexpr (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(y + e);
      t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
    } else {
      t[0] = y[e];
    }
    sort_members<NP, V>(s);
#pragma unroll
    for (int p = 0; p < V; ++p) {
      if (clamp) t[p] = clampf(t[p], lo, hi);
      const double yd = (double)t[p];
      double mean, ssq, dist = 0.0, wsum = 0.0;
      moments<NP, V>(s, p, N, mean, ssq);
      int rank = 0;
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (i < N) {
          dist += fabs((double)s[i][p] - yd);
          wsum += (double)(2 * i - N + 1) * (double)s[i][p];
          rank += s[i][p] < t[p] ? 1 : 0;
        }
      double crps = dist / (double)N - wsum / ((double)N * (double)N);
      double var = ssq / (double)(N - 1), err = (mean - yd) * (mean - yd);
      if (bad[p] || t[p] != t[p]) {
        crps = var = err = (double)NAN;
      } else {
        atomicAdd(&hist[rank], 1u);
      }
      c[p] = (float)crps;
      acc[0] += crps;
      acc[1] += var;
      acc[2] += err;
    }
    if (crps_out) store_map<V>(crps_out, e, c);
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[k][wave] = v;
  }
  __syncthreads();
  const int K = kSums + N + 1, k = threadIdx.x;
  if (k < K) {
    double* out = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * K;
    if (k < kSums) {
      double v = 0.0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) v += red[k][w];
      out[k] = v;
    } else {
      reinterpret_cast<long long*>(out)[k] = (long long)hist[k - kSums];
    }
  }
}

// sums[image][k] (k < kSums) or hist[image][k - kSums] = the sum over the n partial rows of that image, in a fixed order.
// blockIdx.x = k, blockIdx.y = image.
__global__ __launch_bounds__(kThreads) void ensemble_reduce_kernel(const double* __restrict__ partials, double* __restrict__ sums,
                                                                   long long* __restrict__ hist_out, int64_t n, int K) {
  __shared__ double red[kThreads];
  __shared__ long long red_n[kThreads];
  const int k = blockIdx.x;
  const double* p = partials + (int64_t)blockIdx.y * n * K + k;
  if (k < kSums) {
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += kThreads) s += p[j * K];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[(int64_t)blockIdx.y * kSums + k] = red[0];
  } else {
    const long long* pn = reinterpret_cast<const long long*>(p);
    long long s = 0;
    for (int64_t j = threadIdx.x; j < n; j += kThreads) s += pn[j * K];
    red_n[threadIdx.x] = s;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red_n[threadIdx.x] += red_n[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) hist_out[(int64_t)blockIdx.y * (K - kSums) + k - kSums] = red_n[0];
  }
}

// blocks per image of the scores kernel: about one group per thread, at most 512 partial rows per image
int scores_blocks(int64_t chw, int V) {
  const int64_t b = (chw / V + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}
int stats_blocks(int64_t total, int V) {
  const int64_t b = (total / V + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}
bool members_ok(int N) { return N >= 2 && N <= kMaxMembers; }
bool shape_ok(int B, int C, int H, int W) { return B >= 1 && B <= 65535 && C >= 1 && H >= 1 && W >= 1; }

template <int NP>
void launch_stats(bool wide, const float* x, float* mean, float* std, float* quant, const QuantileSpec& qs, int Q, int N,
                  int64_t total, int clamp, float lo, float hi, hipStream_t s) {
  if (wide) {
    DRS_LAUNCH((ensemble_stats_kernel<NP, 4>), dim3(stats_blocks(total, 4)), dim3(kThreads), 0, s, x, mean, std, quant, qs, Q, N,
               total, clamp, lo, hi);
  } else {
    DRS_LAUNCH((ensemble_stats_kernel<NP, 1>), dim3(stats_blocks(total, 1)), dim3(kThreads), 0, s, x, mean, std, quant, qs, Q, N,
               total, clamp, lo, hi);
  }
}

template <int NP>
void launch_scores(bool wide, const float* x, const float* y, float* crps, double* ws, int N, int B, int64_t chw, int nb, int clamp,
                   float lo, float hi, hipStream_t s) {
  if (wide) {
    DRS_LAUNCH((ensemble_scores_kernel<NP, 4>), dim3(nb, B), dim3(kThreads), 0, s, x, y, crps, ws, N, chw, (int64_t)B * chw, clamp,
               lo, hi);
  } else {
    DRS_LAUNCH((ensemble_scores_kernel<NP, 1>), dim3(nb, B), dim3(kThreads), 0, s, x, y, crps, ws, N, chw, (int64_t)B * chw, clamp,
               lo, hi);
  }
}

// the size bucket of N members: the next power of two
#define DRS_ENSEMBLE_DISPATCH(N, call)  \
  do {                                  \
    if ((N) <= 2) call(2);              \
    else if ((N) <= 4) call(4);         \
    else if ((N) <= 8) call(8);         \
    else if ((N) <= 16) call(16);       \
    else call(32);                      \
  } while (0)

}  // namespace

extern "C" DRS_API size_t drs_ensemble_workspace_bytes(int N, int B, int C, int H, int W) {
  if (!members_ok(N) || !shape_ok(B, C, H, W)) return 0;
  // (the scalar instance of the scores kernel has the most blocks)
  return (size_t)B * scores_blocks((int64_t)C * H * W, 1) * (kSums + N + 1) * sizeof(double);
}

extern "C" DRS_API int drs_ensemble_stats(const float* members, float* mean, float* std, float* quantiles, const double* q, int Q,
                                          int N, int B, int C, int H, int W, int clamp, float lo, float hi, drs_stream_t stream) {
  DRS_REQUIRE(members, DRS_ERR_ARG, "ensemble_stats: null pointer (members)");
  DRS_REQUIRE(Q >= 0 && Q <= kMaxQ, DRS_ERR_SHAPE, "ensemble_stats: Q=%d quantiles (0 <= Q <= %d)", Q, kMaxQ);
  DRS_REQUIRE(Q == 0 || (quantiles && q), DRS_ERR_ARG, "ensemble_stats: null pointer (quantiles / q with Q=%d)", Q);
  DRS_REQUIRE(members_ok(N), DRS_ERR_SHAPE, "ensemble_stats: N=%d members (2 <= N <= %d)", N, kMaxMembers);
  DRS_REQUIRE(shape_ok(B, C, H, W), DRS_ERR_SHAPE, "ensemble_stats: B=%d C=%d H=%d W=%d", B, C, H, W);
  DRS_REQUIRE(!clamp || lo <= hi, DRS_ERR_ARG, "ensemble_stats: clamp range [%g, %g]", (double)lo, (double)hi);
  QuantileSpec qs = {};
  for (int j = 0; j < Q; ++j) {
    DRS_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0, DRS_ERR_SHAPE, "ensemble_stats: q[%d]=%g outside [0, 1]", j, q[j]);
    const double pos = q[j] * (double)(N - 1);
    const int k = (int)std::floor(pos);
    qs.k[j] = k;
    qs.k1[j] = k + 1 < N ? k + 1 : N - 1;
    qs.frac[j] = pos - (double)k;
  }
  if (!mean && !std && Q == 0) return DRS_OK;
  const int64_t total = (int64_t)B * C * H * W;
  const bool wide = total % 4 == 0 &&
                    ((uintptr_t)members | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)quantiles) % 16 == 0;
#define DRS_CALL(NP) launch_stats<NP>(wide, members, mean, std, quantiles, qs, Q, N, total, clamp, lo, hi, (hipStream_t)stream)
  DRS_ENSEMBLE_DISPATCH(N, DRS_CALL);
#undef DRS_CALL
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API int drs_ensemble_scores(const float* members, const float* truth, float* crps_map, double* sums,
                                           int64_t* rank_histogram, int N, int B, int C, int H, int W, int clamp, float lo,
                                           float hi, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  DRS_REQUIRE(members && truth && sums && rank_histogram && workspace, DRS_ERR_ARG, "ensemble_scores: null pointer");
  DRS_REQUIRE(members_ok(N), DRS_ERR_SHAPE, "ensemble_scores: N=%d members (2 <= N <= %d)", N, kMaxMembers);
  DRS_REQUIRE(shape_ok(B, C, H, W), DRS_ERR_SHAPE, "ensemble_scores: B=%d C=%d H=%d W=%d (B <= 65535)", B, C, H, W);
  DRS_REQUIRE(!clamp || lo <= hi, DRS_ERR_ARG, "ensemble_scores: clamp range [%g, %g]", (double)lo, (double)hi);
  const int64_t chw = (int64_t)C * H * W;
  const bool wide = chw % 4 == 0 && ((uintptr_t)members | (uintptr_t)truth | (uintptr_t)crps_map) % 16 == 0;
  const int nb = scores_blocks(chw, wide ? 4 : 1), K = kSums + N + 1;
  const size_t need = (size_t)B * nb * K * sizeof(double);
  DRS_REQUIRE(workspace_bytes >= need, DRS_ERR_WORKSPACE, "ensemble_scores: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  double* ws = (double*)workspace;
#define DRS_CALL(NP) launch_scores<NP>(wide, members, truth, crps_map, ws, N, B, chw, nb, clamp, lo, hi, (hipStream_t)stream)
  DRS_ENSEMBLE_DISPATCH(N, DRS_CALL);
#undef DRS_CALL
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(ensemble_reduce_kernel, dim3(K, B), dim3(kThreads), 0, (hipStream_t)stream, ws, sums, (long long*)rank_histogram,
             (int64_t)nb, K);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
