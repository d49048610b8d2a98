// The per-element arithmetic of the reverse-step updates, shared by every kernel that applies one: the ancestral and the DDIM
// update (reverse_step.hip: drs_sampler_step, drs_sampler_step_cfg, drs_ddim_step; drs_inpaint_step takes the coefficients)
// and the per-step tile blend, which forms eps itself and then takes the same step (tile_chain.hip: drs_blend_step,
// drs_blend_step_ddim), the DPM-Solver++(2M) move of both (drs_dpm_step, drs_blend_step_dpm), and the forward-noised known
// element of the moves with known pixels (drs_inpaint_step, drs_blend_step_known).
// One definition, so that a scene state and a tile state that see the same eps move by the same bits.
// At the end: the forward process with its v target, and the conversion of a v / x0 prediction into that eps (prediction.hip).
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

// DPM-Solver++(2M) move t -> t_p (Lu et al., "DPM-Solver++", Algorithm 2, data prediction), with the level t_q > t of the
// previous move, or t_q = -1 for a first-order move (no valid history, or the move to level 0):
//   a = sqrt(ah), s = sqrt(1 - ah), E = (s_p / a_p) (a_t / s_t) = exp(-h), phi = a_p (1 - E), lam = ln(a / s),
//   r = (lam_t - lam_q) / (lam_p - lam_t)
//   x0 = cx x + ce eps,  cx = 1 / a_t,  ce = -s_t / a_t
//   x' = A x + B eps + C x0_prev,  k0 = phi (1 + 1 / (2 r)) | phi,  A = s_p / s_t + k0 / a_t,  B = -k0 s_t / a_t,
//                                  C = -phi / (2 r) | 0
// E is formed without logarithms, so the move to level 0 (ah_0 = 1: E = 0, x' = x0) takes none; r needs them only when
// t_q >= 0, and then t_p > 0 (checked on the host).  Every thread forms the coefficients in fp64 from the fp32 table and
// rounds them once, for the reason given at drs_ddim_coef.  Products and sums are rounded one by one (no contraction), so
// that the scene state of the tile blend and a sampler state that see the same eps move by the same bits.
struct DrsDpmCoef {
  float cx, ce, a, b, c;
  bool second;  // the move reads x0_prev
};
__device__ __forceinline__ DrsDpmCoef drs_dpm_coef(const float* __restrict__ alpha_hat, int t_q, int t, int t_p) {
  const double aht = (double)alpha_hat[t], ahp = (double)alpha_hat[t_p];
  const double a_t = sqrt(aht), s_t = sqrt(1.0 - aht), a_p = sqrt(ahp), s_p = sqrt(fmax(1.0 - ahp, 0.0));
  const double E = (s_p / a_p) * (a_t / s_t);
  const double phi = a_p * (1.0 - E);
  double k0 = phi, C = 0.0;
  DrsDpmCoef k;
  k.second = t_q >= 0;
  if (k.second) {
    const double ahq = (double)alpha_hat[t_q];
    const double lam_t = 0.5 * log(aht / (1.0 - aht)), lam_q = 0.5 * log(ahq / (1.0 - ahq));
    const double lam_p = 0.5 * log(ahp / (1.0 - ahp));
    const double inv_2r = 0.5 * (lam_p - lam_t) / (lam_t - lam_q);
    k0 = phi * (1.0 + inv_2r);
    C = -phi * inv_2r;
  }
  k.cx = (float)(1.0 / a_t);
  k.ce = (float)(-s_t / a_t);
  k.a = (float)(s_p / s_t + k0 / a_t);
  k.b = (float)(-k0 * s_t / a_t);
  k.c = (float)C;
  return k;
}
__device__ __forceinline__ float drs_dpm_x0(const DrsDpmCoef& k, float x, float eps) {
#pragma clang fp contract(off)
  const float p = k.cx * x, q = k.ce * eps;
  return p + q;
}
// `x0_prev` is used by a second-order move only (a first-order one may be handed anything)
__device__ __forceinline__ float drs_dpm_update(const DrsDpmCoef& k, float x, float eps, float x0_prev) {
#pragma clang fp contract(off)
  const float p = k.a * x, q = k.b * eps;
  float v = p + q;
  if (k.second) {
    const float h = k.c * x0_prev;
    v = v + h;
  }
  return v;
}

// q(x_t | x_0) of one known element at level t_prev (drs_inpaint_step, drs_blend_step_known): fl(a * known) + fl(b * z), a =
// sqrt(ah), b = sqrt(1 - ah) formed in fp64 from the fp32 table entry and rounded once (as drs_ddim_coef does), no contraction
// into a fused multiply-add.
struct DrsKnownCoef {
  float a, b;
  __device__ DrsKnownCoef(const float* __restrict__ alpha_hat, int t_prev) {
    const double ah = (double)alpha_hat[t_prev];
    a = (float)sqrt(ah);
    b = (float)sqrt(1.0 - ah);
  }
  __device__ float at(float known, float z) const {
#pragma clang fp contract(off)
    const float p = a * known, q = b * z;
    return p + q;
  }
};

// The forward process of one training element and its v target (prediction.hip: drs_noise_v_target), a = sqrtf(ah) and
// b = sqrtf(1 - ah) in fp32 as drs_noise_images forms them: fl(a x0) + fl(b eps) and fl(a eps) - fl(b x0), no contraction.
// Plain operators under contract(off), as above: HIP's __fmul_rn / __fadd_rn are inline functions of a header compiled with
// contraction on, and once inlined into an unrolled group the compiler fuses them (v_pk_fma_f32) whatever this file says.
__device__ __forceinline__ float drs_forward_noise(float a, float b, float x0, float eps) {
#pragma clang fp contract(off)
  const float p = a * x0, q = b * eps;
  return p + q;
}
__device__ __forceinline__ float drs_v_target(float a, float b, float x0, float eps) {
#pragma clang fp contract(off)
  const float p = a * eps, q = b * x0;
  return p - q;
}

// A prediction p of the network - eps, v = a eps - s x0 or x0 (`kind`: DRS_PRED_EPS / _V / _X0 = 0 / 1 / 2 of include/drs_hip.h)
// - as the eps every update above takes, against the x the network saw at the level of table entry `ah`; with `clip` the
// implied x0 is first clamped to [lo, hi] (prediction.hip: drs_pred_to_eps).  a = sqrt(ah), s = sqrt(1 - ah) in fp64 from the
// fp32 entry, each coefficient rounded once (as drs_ddim_coef), products and sums rounded one by one:
//   no clip   eps: p          v: s x + a p            x0: (1/s) x + (-a/s) p
//   clip      x0 = eps: (1/a) x + (-s/a) p   v: a x + (-s) p   x0: p;   eps = (1/s) x + (-a/s) clamp(x0)
// Where s == 0 (ah == 1, level 0 of the cosine table) the forms that divide by s give 0; where a == 0 an eps prediction is
// passed through unclipped; `bad` (a level outside the table) gives NaN.  No chain predicts at those levels.
struct DrsPredCoef {
  enum Form { PASS, LINEAR, CLIP_LINEAR, CLIP_PRED, ZERO, BAD };
  Form form;
  float xa, xb;  // CLIP_LINEAR: x0 = xa x + xb p
  float ea, eb;  // eps = ea x + eb q, q = p (LINEAR) or the clamped x0
  float lo, hi;
};
__device__ __forceinline__ DrsPredCoef drs_pred_coef(float ah, int kind, bool clip, float lo, float hi, bool bad) {
  const double a = sqrt((double)ah), s = sqrt(fmax(1.0 - (double)ah, 0.0));
  DrsPredCoef k;
  k.xa = k.xb = k.ea = k.eb = 0.f;
  k.lo = lo;
  k.hi = hi;
  const bool is_eps = kind == 0, is_v = kind == 1;
  if (bad) {
    k.form = DrsPredCoef::BAD;
  } else if (is_eps && (!clip || a == 0.0)) {
    k.form = DrsPredCoef::PASS;
  } else if (is_v && !clip) {
    k.form = DrsPredCoef::LINEAR;
    k.ea = (float)s;
    k.eb = (float)a;
  } else if (s == 0.0) {
    k.form = DrsPredCoef::ZERO;
  } else {
    k.ea = (float)(1.0 / s);
    k.eb = (float)(-a / s);
    if (!clip) {
      k.form = DrsPredCoef::LINEAR;
    } else if (is_eps) {
      k.form = DrsPredCoef::CLIP_LINEAR;
      k.xa = (float)(1.0 / a);
      k.xb = (float)(-s / a);
    } else if (is_v) {
      k.form = DrsPredCoef::CLIP_LINEAR;
      k.xa = (float)a;
      k.xb = (float)(-s);
    } else {
      k.form = DrsPredCoef::CLIP_PRED;
    }
  }
  return k;
}
__device__ __forceinline__ float drs_pred_eps(const DrsPredCoef& k, float x, float p) {
#pragma clang fp contract(off)
  if (k.form == DrsPredCoef::PASS) return p;
  if (k.form == DrsPredCoef::ZERO) return 0.f;
  if (k.form == DrsPredCoef::BAD) return __builtin_nanf("");
  float q = p;
  if (k.form == DrsPredCoef::CLIP_LINEAR) {
    const float u = k.xa * x, w = k.xb * p;
    q = u + w;
  }
  if (k.form != DrsPredCoef::LINEAR && fabsf(q) < __builtin_huge_valf())  // a NaN or an infinity stays what it is (no fminf / fmaxf)
    q = q < k.lo ? k.lo : (q > k.hi ? k.hi : q);
  const float u = k.ea * x, w = k.eb * q;
  return u + w;
}

// Dynamic thresholding of the implied x0 (Saharia et al., "Imagen", 2022, section 2.3; x0_threshold.hip: drs_pred_to_eps_dyn,
// DESIGN.md section 24), element by element.  The x0 is the clip path's `q` before its clamp (forms CLIP_LINEAR / CLIP_PRED of
// drs_pred_coef); c = (lo + hi) / 2 and r = (hi - lo) / 2 are formed in fp64 and rounded once.  An image is ranked by
// key = bits(|fl(x0 - c)|) as an unsigned integer, a NaN or an infinity as +inf; its scale s is the key of one rank.
__device__ __forceinline__ float drs_pred_x0(const DrsPredCoef& k, float x, float p) {
#pragma clang fp contract(off)
  if (k.form != DrsPredCoef::CLIP_LINEAR) return p;
  const float u = k.xa * x, w = k.xb * p;
  return u + w;
}
__device__ __forceinline__ unsigned drs_dyn_key(float x0, float c) {
  const unsigned key = __float_as_uint(fabsf(x0 - c));
  return key < 0x7f800000u ? key : 0x7f800000u;
}
// s <= r or s not finite: the static clamp of drs_pred_eps; otherwise clamp(c + clamp(x0 - c, -s, s) rho, lo, hi) with
// rho = (float)((double)r / s), products and sums rounded one by one.  A NaN or an infinity stays what it is.
struct DrsDynScale {
  float c, s, rho;
  bool dynamic;
  __device__ DrsDynScale(float lo, float hi, float scale) {
    c = (float)(((double)lo + (double)hi) / 2.0);
    const float r = (float)(((double)hi - (double)lo) / 2.0);
    s = scale;
    dynamic = scale > r && scale < __builtin_huge_valf();
    rho = dynamic ? (float)((double)r / (double)scale) : 1.f;
  }
};
__device__ __forceinline__ float drs_dyn_q(const DrsPredCoef& k, const DrsDynScale& y, float x0) {
#pragma clang fp contract(off)
  if (!(fabsf(x0) < __builtin_huge_valf())) return x0;
  float q = x0;
  if (y.dynamic) {
    const float d = x0 - y.c;
    const float e = d < -y.s ? -y.s : (d > y.s ? y.s : d);
    const float m = e * y.rho;
    q = y.c + m;
  }
  return q < k.lo ? k.lo : (q > k.hi ? k.hi : q);
}
// eps = fl(ea x) + fl(eb q) of the clip forms, q the clamped or thresholded x0
__device__ __forceinline__ float drs_eps_of_x0(const DrsPredCoef& k, float x, float q) {
#pragma clang fp contract(off)
  const float u = k.ea * x, w = k.eb * q;
  return u + w;
}
