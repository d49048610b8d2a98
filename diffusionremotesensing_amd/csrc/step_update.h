// The per-element arithmetic of the reverse-step updates, shared by every kernel that applies one: the ancestral and the DDIM
// update (reverse_step.hip: drs_sampler_step, drs_sampler_step_cfg, drs_ddim_step; drs_inpaint_step takes the coefficients)
// and the per-step tile blend, which forms eps itself and then takes the same step (tile_chain.hip: drs_blend_step,
// drs_blend_step_ddim).
// One definition, so that a scene state and a tile state that see the same eps move by the same bits.
#pragma once
#include <hip/hip_runtime.h>

// torch.lerp(start = uncond, end = cond, w): |w| < 0.5 ? fma(w, diff, start) : end - diff * (1 - w)
__device__ __forceinline__ float drs_cfg_lerp(float uncond, float cond, float w) {
  const float d = __fsub_rn(cond, uncond);
  return fabsf(w) < 0.5f ? fmaf(w, d, uncond) : __fsub_rn(cond, __fmul_rn(d, __fsub_rn(1.f, w)));
}

// Ancestral step (reference train_diffusion_superres.py:240-249): the same operations, in the same order and without
// fused multiply-adds, as the reference expression; the three coefficients are read from the device tables by every thread.
struct DrsAncestralCoef {
  float c_inv, c_eps, c_sig;
};
__device__ __forceinline__ DrsAncestralCoef drs_ancestral_coef(const float* __restrict__ alpha,
                                                               const float* __restrict__ alpha_hat,
                                                               const float* __restrict__ beta, int t) {
  const float a = alpha[t], ah = alpha_hat[t], b = beta[t];
  DrsAncestralCoef k;
  k.c_inv = __fdiv_rn(1.f, sqrtf(a));
  k.c_eps = __fdiv_rn(__fsub_rn(1.f, a), sqrtf(__fsub_rn(1.f, ah)));
  k.c_sig = sqrtf(b);
  return k;
}
__device__ __forceinline__ float drs_ancestral_update(const DrsAncestralCoef& k, float x, float eps) {
  return __fmul_rn(k.c_inv, __fsub_rn(x, __fmul_rn(k.c_eps, eps)));
}
__device__ __forceinline__ float drs_ancestral_noise(const DrsAncestralCoef& k, float v, float z) {
  return __fadd_rn(v, __fmul_rn(k.c_sig, z));
}

// DDIM step t -> t_prev.  Every thread forms the same three coefficients: ah_t / ah_p are read from the device table (no
// read-back to the host) and combined in fp64, then rounded to fp32 once.  Near t = T - 1 of the cosine schedule ah_t is
// ~1e-6: on a long jump A = sqrt(ah_p / ah_t) and the two terms of B are each ~900, and B is their difference, which fp32
// terms rounded one by one would leave with ~4 digits.
struct DrsDdimCoef {
  float a, b, s;
  bool has_sigma;  // sigma > 0: the step adds s * noise
};
__device__ __forceinline__ DrsDdimCoef drs_ddim_coef(const float* __restrict__ alpha_hat, int t, int t_prev, float eta) {
  const double at = (double)alpha_hat[t], ap = (double)alpha_hat[t_prev];
  double sig = 0.0;
  if (t_prev > 0 && eta > 0.f) sig = (double)eta * sqrt((1.0 - ap) / (1.0 - at)) * sqrt(1.0 - at / ap);
  const double A = sqrt(ap / at);
  const double B = sqrt(fmax(1.0 - ap - sig * sig, 0.0)) - sqrt(ap) * sqrt(1.0 - at) / sqrt(at);
  DrsDdimCoef k;
  k.a = (float)A;
  k.b = (float)B;
  k.s = (float)sig;
  k.has_sigma = sig > 0.0;
  return k;
}
__device__ __forceinline__ float drs_ddim_update(const DrsDdimCoef& k, float x, float eps) {
  return __fadd_rn(__fmul_rn(k.a, x), __fmul_rn(k.b, eps));
}
__device__ __forceinline__ float drs_ddim_noise(const DrsDdimCoef& k, float v, float z) {
  return __fadd_rn(v, __fmul_rn(k.s, z));
}
