// Colour correction of a super-resolved batch `sr` against a guide of the same size, the up-sampled LR observation
// (colorfix.py), per (image, band) plane: the sample keeps its fine detail and takes the large-scale content of the guide.
//   wavelet: out = sr + low_L(guide - sr), low_L = L dilated 3 x 3 binomial blurs on replicate padding (one launch, all
//            levels in LDS);
//   adain:   out = a sr + b with the plane's mean and standard deviation moved onto the guide's (a statistics pass with a
//            fixed-order fp64 reduction - no atomics, two calls write the same bits - then an apply pass).
#include "drs_common.h"
#include <cmath>

namespace {

// ---- wavelet ------------------------------------------------------------------------------------------------------------
// One block per kTile x kTile output tile of one plane.  With halo = 2^L - 1 the tile's result depends on the
// (kTile + 2 halo)^2 pixels around it and on nothing else: D = guide - sr of that region, clipped to the image, is staged in
// LDS buffer A, and level l = 1 .. L (dilation d = 2^(l-1)) runs there as a row pass A -> B and a column pass B -> A.
// The map is linear, so blurring the difference and adding sr back is the published (sr - low(sr)) + low(guide); it needs one
// staged tensor instead of two, and guide == sr gives D = 0 and out == sr bit for bit.
// Level l is only formed where the later levels read it: on the tile grown by m_l = 2^L - 2^l pixels (126, 124, 120, 112,
// 96, 64 pixels a side for the input and the five levels of L = 5), its row pass on d more rows above and below.  Taps are
// clamped in IMAGE coordinates (replicate padding of the whole plane, not of the tile); the clamped taps of a position of
// level l lie inside the clipped region of level l - 1, because m_(l-1) = m_l + d, so nothing outside the image and nothing
// outside the staged region is read.  The weights are powers of two: a pass costs two roundings per element.
// Threads are 64 columns x 16 rows; every LDS access of a wave is 64 consecutive floats of one row (no bank conflicts in
// either pass).  In the column pass a thread forms kRun outputs d rows apart from kRun + 2 reads (they share taps).
constexpr int kTile = 64, kMaxLevels = 5;
constexpr int kWThreads = 1024, kWRows = kWThreads / 64;
constexpr int kRun = 4;
constexpr int wavelet_side(int levels) { return kTile + 2 * ((1 << levels) - 1); }                  // 126 at L = 5
constexpr size_t wavelet_lds(int levels) { return 2 * sizeof(float) * wavelet_side(levels) * wavelet_side(levels); }
static_assert(wavelet_lds(kMaxLevels) <= 160 * 1024, "LDS budget");

template <bool VEC>
__global__ __launch_bounds__(kWThreads) void colorfix_wavelet_kernel(const float* __restrict__ sr,
                                                                     const float* __restrict__ guide,
                                                                     float* __restrict__ out, int H, int W, int levels,
                                                                     int tiles_x, int tiles_per_plane) {
  extern __shared__ __align__(16) float lds[];
  const int halo = (1 << levels) - 1, R = kTile + 2 * halo;
  float* A = lds;
  float* Bf = lds + R * R;
  const int tx = threadIdx.x % 64, ty = threadIdx.x / 64;
  const int64_t plane = blockIdx.x / tiles_per_plane;
  const int t = blockIdx.x % tiles_per_plane;
  const int ty0 = (t / tiles_x) * kTile, tx0 = (t % tiles_x) * kTile;
  const int ty1 = min(ty0 + kTile, H), tx1 = min(tx0 + kTile, W);
  const int oy = max(ty0 - halo, 0), ox = max(tx0 - halo, 0);  // image position of A[0] / Bf[0]
  const int ey = min(ty1 + halo, H), ex = min(tx1 + halo, W);
  const float* sp = sr + plane * H * W;
  const float* gp = guide + plane * H * W;
  {  // every load of the thread is issued before the first use: the region costs one memory latency, not one per row
    constexpr int kI = (wavelet_side(kMaxLevels) + kWRows - 1) / kWRows, kJ = (wavelet_side(kMaxLevels) + 63) / 64;
    float dv[kI][kJ];
#pragma unroll
    for (int i = 0; i < kI; ++i)
#pragma unroll
      for (int j = 0; j < kJ; ++j) {
        const int y = oy + ty + i * kWRows, x = ox + tx + j * 64;
        const int64_t g = (int64_t)y * W + x;
        dv[i][j] = y < ey && x < ex ? gp[g] - sp[g] : 0.f;
      }
#pragma unroll
    for (int i = 0; i < kI; ++i)
#pragma unroll
      for (int j = 0; j < kJ; ++j) {
        const int y = oy + ty + i * kWRows, x = ox + tx + j * 64;
        if (y < ey && x < ex) A[(y - oy) * R + (x - ox)] = dv[i][j];
      }
  }
  __syncthreads();
  for (int l = 1; l <= levels; ++l) {
    const int d = 1 << (l - 1), m = (1 << levels) - (1 << l);
    const int y0 = max(ty0 - m, 0), y1 = min(ty1 + m, H), x0 = max(tx0 - m, 0), x1 = min(tx1 + m, W);
    const int ys = max(y0 - d, 0), ye = min(y1 + d, H);
    for (int x = x0 + tx; x < x1; x += 64) {
      const int cm = max(x - d, 0) - ox, cc = x - ox, cp = min(x + d, W - 1) - ox;  // the three columns, once per level
#pragma unroll 4
      for (int row = (ys + ty - oy) * R; row < (ye - oy) * R; row += kWRows * R)
        Bf[row + cc] = 0.25f * A[row + cm] + 0.5f * A[row + cc] + 0.25f * A[row + cp];
    }
    __syncthreads();
    // chain q: rows yb, yb + d, ... of a block of kRun d rows; rows of Bf outside [ys, ye) feed no kept output
    const int nq = (y1 - y0 + kRun * d - 1) / (kRun * d) * d;
    for (int q = ty; q < nq; q += kWRows) {
      const int yb = y0 + (q >> (l - 1)) * (kRun * d) + (q & (d - 1));
      for (int x = x0 + tx; x < x1; x += 64) {
        float v[kRun + 2];
#pragma unroll
        for (int k = 0; k < kRun + 2; ++k) v[k] = Bf[(min(max(yb + (k - 1) * d, ys), ye - 1) - oy) * R + (x - ox)];
#pragma unroll
        for (int k = 0; k < kRun; ++k)
          if (yb + k * d < y1) A[(yb + k * d - oy) * R + (x - ox)] = 0.25f * v[k] + 0.5f * v[k + 1] + 0.25f * v[k + 2];
      }
    }
    __syncthreads();
  }
  float* op = out + plane * H * W;
  if constexpr (VEC) {  // W % 4 == 0, 16-byte aligned tensors: 16 threads a row, one 16-byte store each
    const int x = tx0 + (threadIdx.x % 16) * 4;
    for (int y = ty0 + threadIdx.x / 16; y < ty1; y += kWThreads / 16) {
      if (x >= tx1) continue;
      const float* a = A + (y - oy) * R + (x - ox);
      float4 s = *reinterpret_cast<const float4*>(sp + (int64_t)y * W + x);
      s.x += a[0]; s.y += a[1]; s.z += a[2]; s.w += a[3];
      *reinterpret_cast<float4*>(op + (int64_t)y * W + x) = s;
    }
  } else {
    for (int y = ty0 + ty; y < ty1; y += kWRows)
      for (int x = tx0 + tx; x < tx1; x += 64) op[(int64_t)y * W + x] = sp[(int64_t)y * W + x] + A[(y - oy) * R + (x - ox)];
  }
}

// ---- AdaIN --------------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxStatBlocks = 256;  // partial rows of a plane

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;  // lane 0 holds the sum, always formed in the same order
}

// blocks per plane of the statistics and the apply kernel: about two groups of V pixels per thread
int plane_blocks(int64_t hw, int V, int most) {
  const int64_t b = (hw / V + 2 * kThreads - 1) / (2 * kThreads);
  return (int)(b < 1 ? 1 : (b > most ? most : b));
}

// blockIdx.x = plane * nb + j; block j strides over the groups of V consecutive pixels of its plane and leaves
// partials[plane][j][4] = sum sr | sum sr^2 | sum guide | sum guide^2, every sum carried in fp64 from the first element on
// (a plane of mean 0.95 and deviation 0.002 keeps its variance to 1e-11 of itself).  V = 4 needs hw % 4 == 0 and 16-byte
// aligned tensors; the hw % V pixels past the last group (V = 1: none) do not exist then.
template <int V>
__global__ __launch_bounds__(kThreads) void adain_stats_kernel(const float* __restrict__ sr, const float* __restrict__ guide,
                                                               double* __restrict__ partials, int64_t hw, int nb) {
  __shared__ double red[4][kWaves];
  const int64_t plane = blockIdx.x / nb;
  const int j = blockIdx.x % nb;
  const float* sp = sr + plane * hw;
  const float* gp = guide + plane * hw;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const int64_t groups = hw / V;
  for (int64_t g = (int64_t)j * kThreads + threadIdx.x; g < groups; g += (int64_t)nb * kThreads) {
    float u[V], v[V];
    if constexpr (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(sp + g * 4);
      const float4 b = *reinterpret_cast<const float4*>(gp + g * 4);
      u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
      v[0] = b.x; v[1] = b.y; v[2] = b.z; v[3] = b.w;
    } else {
      u[0] = sp[g];
      v[0] = gp[g];
    }
#pragma unroll
    for (int p = 0; p < V; ++p) {
      const double a = (double)u[p], b = (double)v[p];
      s[0] += a;
      s[1] = fma(a, a, s[1]);
      s[2] += b;
      s[3] = fma(b, b, s[3]);
    }
  }
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = wave_sum(s[k]);
    if (lane == 0) red[k][wave] = w;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double w = 0.0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) w += red[threadIdx.x][i];
    partials[((int64_t)plane * nb + j) * 4 + threadIdx.x] = w;
  }
}

// One block per plane: wave k adds the nb partials of sum k in a fixed order, thread 0 forms, all in fp64,
//   var = (sum x^2 - (sum x)^2 / n) / (n - 1),  std = sqrt(var + 1e-5),  a = std_g / std_sr,  b = mean_g - a mean_sr
// and rounds a and b to fp32 once: coef[plane] = (a, b).
__global__ __launch_bounds__(kThreads) void adain_coef_kernel(const double* __restrict__ partials, float2* __restrict__ coef,
                                                              int64_t hw, int nb) {
  __shared__ double sum[4];
  const int k = threadIdx.x / 64, lane = threadIdx.x % 64;
  const double* p = partials + (int64_t)blockIdx.x * nb * 4 + k;
  double s = 0.0;
  for (int j = lane; j < nb; j += 64) s += p[(int64_t)j * 4];
  s = wave_sum(s);
  if (lane == 0) sum[k] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = (double)hw;
    const double mean_s = sum[0] / n, mean_g = sum[2] / n;
    const double var_s = (sum[1] - sum[0] * sum[0] / n) / (n - 1.0), var_g = (sum[3] - sum[2] * sum[2] / n) / (n - 1.0);
    const double a = sqrt(var_g + 1e-5) / sqrt(var_s + 1e-5);
    coef[blockIdx.x] = make_float2((float)a, (float)(mean_g - a * mean_s));
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void adain_apply_kernel(const float* __restrict__ sr, const float2* __restrict__ coef,
                                                               float* __restrict__ out, int64_t hw, int nb) {
  const int64_t plane = blockIdx.x / nb;
  const int j = blockIdx.x % nb;
  const float2 c = coef[plane];
  const float* sp = sr + plane * hw;
  float* op = out + plane * hw;
  const int64_t groups = hw / V;
  for (int64_t g = (int64_t)j * kThreads + threadIdx.x; g < groups; g += (int64_t)nb * kThreads) {
    if constexpr (V == 4) {
      float4 a = *reinterpret_cast<const float4*>(sp + g * 4);
      a.x = fmaf(c.x, a.x, c.y); a.y = fmaf(c.x, a.y, c.y); a.z = fmaf(c.x, a.z, c.y); a.w = fmaf(c.x, a.w, c.y);
      *reinterpret_cast<float4*>(op + g * 4) = a;
    } else {
      op[g] = fmaf(c.x, sp[g], c.y);
    }
  }
}

constexpr int kMaxApplyBlocks = 2048;

// ---- argument checks of both entry points ---------------------------------------------------------------------------------
bool overlap(const float* a, const float* b, size_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = n * sizeof(float);
  return x < y + bytes && y < x + bytes;
}
int check_args(const char* what, const float* sr, const float* guide, const float* out, int B, int C, int H, int W) {
  DRS_REQUIRE(sr && guide && out, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(B >= 1 && C >= 1 && C <= kMaxBands && H >= 1 && W >= 1, DRS_ERR_SHAPE, "%s: B=%d C=%d H=%d W=%d (1 <= C <= %d)", what,
              B, C, H, W, kMaxBands);
  const size_t n = (size_t)B * C * H * W;
  DRS_REQUIRE(!overlap(out, sr, n) && !overlap(out, guide, n), DRS_ERR_ARG,
              "%s: out overlaps sr or guide (a tile reads its neighbours' sr: in place is a race)", what);
  return DRS_OK;
}
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" DRS_API int drs_colorfix_wavelet(const float* sr, const float* guide, float* out, int B, int C, int H, int W,
                                            int levels, drs_stream_t stream) {
  if (const int rc = check_args("colorfix_wavelet", sr, guide, out, B, C, H, W)) return rc;
  DRS_REQUIRE(levels >= 1 && levels <= kMaxLevels, DRS_ERR_SHAPE, "colorfix_wavelet: levels=%d outside 1 .. %d", levels,
              kMaxLevels);
  const int tiles_x = drs_cdiv(W, kTile);
  const int64_t tiles_per_plane = (int64_t)tiles_x * drs_cdiv(H, kTile), blocks = tiles_per_plane * B * C;
  DRS_REQUIRE(blocks <= INT32_MAX, DRS_ERR_SHAPE, "colorfix_wavelet: B=%d C=%d H=%d W=%d need more tiles than one launch holds",
              B, C, H, W);
  const bool wide = W % 4 == 0 && aligned16(sr) && aligned16(out);
  const void* kern = wide ? reinterpret_cast<const void*>(colorfix_wavelet_kernel<true>)
                          : reinterpret_cast<const void*>(colorfix_wavelet_kernel<false>);
  int num_cu = 0;
  if (const int rc = drs_kernel_prepare(kern, (int)wavelet_lds(kMaxLevels), &num_cu)) return rc;
  const size_t lds = wavelet_lds(levels);
  if (wide) {
    DRS_LAUNCH(colorfix_wavelet_kernel<true>, dim3((unsigned)blocks), dim3(kWThreads), lds, (hipStream_t)stream, sr, guide, out,
               H, W, levels, tiles_x, (int)tiles_per_plane);
  } else {
    DRS_LAUNCH(colorfix_wavelet_kernel<false>, dim3((unsigned)blocks), dim3(kWThreads), lds, (hipStream_t)stream, sr, guide, out,
               H, W, levels, tiles_x, (int)tiles_per_plane);
  }
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" DRS_API size_t drs_colorfix_adain_workspace_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || C > kMaxBands || H < 1 || W < 1 || (int64_t)H * W < 2) return 0;
  // (the scalar instance of the statistics kernel has the most blocks): coefficients, then the partial rows
  const size_t planes = (size_t)B * C;
  return align16(planes * sizeof(float2)) + planes * plane_blocks((int64_t)H * W, 1, kMaxStatBlocks) * 4 * sizeof(double);
}

extern "C" DRS_API int drs_colorfix_adain(const float* sr, const float* guide, float* out, int B, int C, int H, int W,
                                          void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  DRS_REQUIRE(workspace, DRS_ERR_ARG, "colorfix_adain: null pointer");
  if (const int rc = check_args("colorfix_adain", sr, guide, out, B, C, H, W)) return rc;
  const int64_t hw = (int64_t)H * W, planes = (int64_t)B * C;
  DRS_REQUIRE(hw >= 2, DRS_ERR_SHAPE, "colorfix_adain: H=%d W=%d: the unbiased variance needs H W >= 2", H, W);
  const bool wide = hw % 4 == 0 && aligned16(sr) && aligned16(guide) && aligned16(out);
  const int V = wide ? 4 : 1;
  const int nb = plane_blocks(hw, V, kMaxStatBlocks), nba = plane_blocks(hw, V, kMaxApplyBlocks);
  DRS_REQUIRE(planes * nba <= INT32_MAX, DRS_ERR_SHAPE, "colorfix_adain: B=%d C=%d H=%d W=%d need more blocks than one launch holds",
              B, C, H, W);
  const size_t coef_bytes = align16((size_t)planes * sizeof(float2));
  const size_t need = coef_bytes + (size_t)planes * nb * 4 * sizeof(double);
  DRS_REQUIRE(workspace_bytes >= need, DRS_ERR_WORKSPACE, "colorfix_adain: workspace of %zu bytes, %zu needed", workspace_bytes,
              need);
  DRS_REQUIRE(((uintptr_t)workspace & 7u) == 0, DRS_ERR_ARG, "colorfix_adain: workspace must be 8-byte aligned");
  float2* coef = (float2*)workspace;
  double* partials = (double*)((char*)workspace + coef_bytes);
  hipStream_t s = (hipStream_t)stream;
  if (wide) {
    DRS_LAUNCH(adain_stats_kernel<4>, dim3((unsigned)(planes * nb)), dim3(kThreads), 0, s, sr, guide, partials, hw, nb);
  } else {
    DRS_LAUNCH(adain_stats_kernel<1>, dim3((unsigned)(planes * nb)), dim3(kThreads), 0, s, sr, guide, partials, hw, nb);
  }
  DRS_CHECK_HIP(hipGetLastError());
  DRS_LAUNCH(adain_coef_kernel, dim3((unsigned)planes), dim3(kThreads), 0, s, partials, coef, hw, nb);
  DRS_CHECK_HIP(hipGetLastError());
  if (wide) {
    DRS_LAUNCH(adain_apply_kernel<4>, dim3((unsigned)(planes * nba)), dim3(kThreads), 0, s, sr, coef, out, hw, nba);
  } else {
    DRS_LAUNCH(adain_apply_kernel<1>, dim3((unsigned)(planes * nba)), dim3(kThreads), 0, s, sr, coef, out, hw, nba);
  }
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
