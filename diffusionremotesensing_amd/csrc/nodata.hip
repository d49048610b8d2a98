// Training on imagery with no-data pixels: forward noising, target and mask in one pass (include/drs_hip.h:
// drs_noise_target_nodata).  The pixel rule is nodata_rule.h's.  No-data elements are SELECTED out - never
// multiplied by zero - so that a NaN or an infinity under the mask reaches no output.  The kernel restates the per-element
// arithmetic of its unmasked siblings (small_kernels.hip / prediction.hip: forward noising and targets, through step_update.h),
// so that a batch without a no-data pixel gives the siblings' bits.
//
// The other three no-data entries live with their unmasked siblings, as the MASKED instances of the same kernel bodies:
// drs_diffusion_loss_masked in loss.hip, drs_metrics_pointwise_nodata and drs_ssim_nodata in metrics.hip.
#include "drs_common.h"
#include "nodata_rule.h"
#include "step_update.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

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
      NodataRule<V> rule;
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
        rule.band(x[c], p.nodata_value);
      }
      bool nd[V];
      unsigned char ok[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        nd[k] = rule.nodata(k, by_value);
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
