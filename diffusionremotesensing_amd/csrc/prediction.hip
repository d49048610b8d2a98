// What the network predicts: eps, v = sqrt(ah) eps - sqrt(1 - ah) x0 (Salimans & Ho, "Progressive
// Distillation for Fast Sampling of Diffusion Models", 2022) or x0.  Two element-wise, HBM-bound entry points (every byte
// moves once; no LDS, no atomics, plain vector loads and stores): drs_noise_v_target forward-noises a training batch and forms
// its v target in the same pass, drs_pred_to_eps turns a prediction of any kind - guided and with its implied x0 clipped to
// the data range, if asked - into the eps the reverse-step kernels take (reverse_step.hip, tile_chain.hip), against the x the
// network saw.  Per-element arithmetic: step_update.h.
#include "drs_common.h"
#include "row_span.h"
#include "step_update.h"

namespace {

struct VTargetArgs {
  const float* x0;
  const float* eps;
  const int64_t* t;
  const float* alpha_hat;
  float* xt;
  float* v;
  int n, noise_steps, phase;
  int64_t chw;
  bool vec;
};

__device__ __forceinline__ void v_target_at(float a, float b, bool bad, float x, float e, float& xt, float& v) {
  xt = bad ? __builtin_nanf("") : drs_forward_noise(a, b, x, e);
  v = bad ? __builtin_nanf("") : drs_v_target(a, b, x, e);
}

// blockIdx.y strides over the images, blockIdx.x over one image's groups (then over its head and tail elements)
__global__ __launch_bounds__(256) void noise_v_target_kernel(const VTargetArgs p) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    const int64_t tn = p.t[img];
    const bool bad = tn < 0 || tn >= p.noise_steps;  // never indexes the table: this image's outputs are NaN
    const float ah = bad ? 0.f : p.alpha_hat[tn];
    const float a = sqrtf(ah), b = sqrtf(1.f - ah);  // fp32, as noise_images_kernel (small_kernels.hip)
    const int64_t row = (int64_t)img * p.chw;
    const float* xp = p.x0 + row;
    const float* ep = p.eps + row;
    float* tp = p.xt + row;
    float* vp = p.v + row;
    const RowSpan s(p.vec, p.phase, row, p.chw);
    for (int64_t g = tid; g < s.groups; g += stride) {
      const int64_t at = s.head + 4 * g;
      const float4 x4 = *reinterpret_cast<const float4*>(xp + at);
      const float4 e4 = *reinterpret_cast<const float4*>(ep + at);
      float4 o, w;
      v_target_at(a, b, bad, x4.x, e4.x, o.x, w.x);
      v_target_at(a, b, bad, x4.y, e4.y, o.y, w.y);
      v_target_at(a, b, bad, x4.z, e4.z, o.z, w.z);
      v_target_at(a, b, bad, x4.w, e4.w, o.w, w.w);
      *reinterpret_cast<float4*>(tp + at) = o;
      *reinterpret_cast<float4*>(vp + at) = w;
    }
    const int64_t rest = p.chw - 4 * s.groups;  // head and tail elements: at most 6 with `vec`
    for (int64_t r = tid; r < rest; r += stride) {
      const int64_t i = r < s.head ? r : s.tail() + (r - s.head);
      v_target_at(a, b, bad, xp[i], ep[i], tp[i], vp[i]);
    }
  }
}

struct ToEpsArgs {
  const float* pred;  // may be `out`
  const float* pu;    // the unconditional prediction, or null: no guidance
  float w;
  const float* x;
  const int64_t* t;
  const float* alpha_hat;
  float* out;
  int n, noise_steps, phase, kind, clip;
  float lo, hi;
  int64_t chw;
  bool vec;
};

template <bool GUIDED>
__global__ __launch_bounds__(256) void pred_to_eps_kernel(const ToEpsArgs p) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    const int64_t tn = p.t[img];
    const bool bad = tn < 0 || tn >= p.noise_steps;  // never indexes the table: this image's eps is NaN
    const DrsPredCoef k = drs_pred_coef(bad ? 0.f : p.alpha_hat[tn], p.kind, p.clip != 0, p.lo, p.hi, bad);
    const int64_t row = (int64_t)img * p.chw;
    const float* pp = p.pred + row;
    const float* up = GUIDED ? p.pu + row : nullptr;
    const float* xp = p.x + row;
    float* op = p.out + row;
    const RowSpan s(p.vec, p.phase, row, p.chw);
    for (int64_t g = tid; g < s.groups; g += stride) {
      const int64_t at = s.head + 4 * g;
      float4 p4 = *reinterpret_cast<const float4*>(pp + at);
      const float4 x4 = *reinterpret_cast<const float4*>(xp + at);
      if constexpr (GUIDED) {
        const float4 u4 = *reinterpret_cast<const float4*>(up + at);
        p4.x = drs_cfg_lerp(u4.x, p4.x, p.w); p4.y = drs_cfg_lerp(u4.y, p4.y, p.w);
        p4.z = drs_cfg_lerp(u4.z, p4.z, p.w); p4.w = drs_cfg_lerp(u4.w, p4.w, p.w);
      }
      float4 o;
      o.x = drs_pred_eps(k, x4.x, p4.x); o.y = drs_pred_eps(k, x4.y, p4.y);
      o.z = drs_pred_eps(k, x4.z, p4.z); o.w = drs_pred_eps(k, x4.w, p4.w);
      *reinterpret_cast<float4*>(op + at) = o;
    }
    const int64_t rest = p.chw - 4 * s.groups;
    for (int64_t r = tid; r < rest; r += stride) {
      const int64_t i = r < s.head ? r : s.tail() + (r - s.head);
      float q = pp[i];
      if constexpr (GUIDED) q = drs_cfg_lerp(up[i], q, p.w);
      op[i] = drs_pred_eps(k, xp[i], q);
    }
  }
}

}  // namespace

extern "C" int drs_noise_v_target(const float* x0, const float* eps, const int64_t* t, const float* alpha_hat, int noise_steps,
                                  float* x_t, float* v, int n, int64_t chw, drs_stream_t stream) {
  DRS_REQUIRE(x0 && eps && t && alpha_hat && x_t && v, DRS_ERR_ARG, "noise_v_target: null pointer");
  DRS_REQUIRE(n >= 0 && chw >= 0 && noise_steps > 0, DRS_ERR_SHAPE, "noise_v_target: n=%d chw=%lld noise_steps=%d", n,
              (long long)chw, noise_steps);
  DRS_REQUIRE(x_t != v, DRS_ERR_ARG, "noise_v_target: x_t and v are one buffer");
  if (n == 0 || chw == 0) return DRS_OK;
  VTargetArgs a;
  a.x0 = x0; a.eps = eps; a.t = t; a.alpha_hat = alpha_hat; a.xt = x_t; a.v = v;
  a.n = n; a.noise_steps = noise_steps; a.chw = chw;
  a.vec = same_phase({x0, eps, x_t, v});
  a.phase = phase_of(x0);
  DRS_LAUNCH(noise_v_target_kernel, stream_grid(n, chw, a.vec), dim3(256), 0, (hipStream_t)stream, a);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_pred_to_eps(const float* pred, const float* pred_uncond, float cfg_scale, const float* x, const int64_t* t,
                               const float* alpha_hat, int noise_steps, int kind, int clip, float lo, float hi, float* out, int n,
                               int64_t chw, drs_stream_t stream) {
  DRS_REQUIRE(pred && x && t && alpha_hat && out, DRS_ERR_ARG, "pred_to_eps: null pointer");
  DRS_REQUIRE(kind == DRS_PRED_EPS || kind == DRS_PRED_V || kind == DRS_PRED_X0, DRS_ERR_ARG,
              "pred_to_eps: kind=%d is none of DRS_PRED_EPS, DRS_PRED_V, DRS_PRED_X0", kind);
  DRS_REQUIRE(!clip || lo < hi, DRS_ERR_ARG, "pred_to_eps: clip needs lo < hi, got lo=%g hi=%g", (double)lo, (double)hi);
  DRS_REQUIRE(!pred_uncond || std::isfinite(cfg_scale), DRS_ERR_ARG, "pred_to_eps: cfg_scale=%g must be finite",
              (double)cfg_scale);
  DRS_REQUIRE(n >= 0 && chw >= 0 && noise_steps > 0, DRS_ERR_SHAPE, "pred_to_eps: n=%d chw=%lld noise_steps=%d", n,
              (long long)chw, noise_steps);
  if (n == 0 || chw == 0) return DRS_OK;
  ToEpsArgs a;
  a.pred = pred; a.pu = pred_uncond; a.w = cfg_scale; a.x = x; a.t = t; a.alpha_hat = alpha_hat; a.out = out;
  a.n = n; a.noise_steps = noise_steps; a.kind = kind; a.clip = clip; a.lo = lo; a.hi = hi; a.chw = chw;
  a.vec = same_phase({pred, pred_uncond, x, out});
  a.phase = phase_of(pred);
  const dim3 grid = stream_grid(n, chw, a.vec);
  if (pred_uncond) DRS_LAUNCH(pred_to_eps_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else DRS_LAUNCH(pred_to_eps_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
