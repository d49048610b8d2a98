// DDIM update (Song et al., "Denoising Diffusion Implicit Models"): the strided-timestep sampler of Diffusion.sample
// (sampling_steps=S).  Element-wise and HBM-bound like the ancestral update in small_kernels.hip, which it leaves alone.
#include "drs_common.h"
#include <cmath>

namespace {

// Every thread forms the same three coefficients: ah_t / ah_p are read from the device table (no read-back to the host)
// and combined in fp64, then rounded to fp32 once.  Near t = T - 1 of the cosine schedule ah_t is ~1e-6: on a long jump
// A = sqrt(ah_p / ah_t) and the two terms of B are each ~900, and B is their difference, which fp32 terms rounded one by
// one would leave with ~4 digits.
__global__ __launch_bounds__(256) void ddim_step_kernel(float* __restrict__ x, const float* __restrict__ ec,
                                                        const float* __restrict__ eu, float w,
                                                        const float* __restrict__ noise, int t, int t_prev, float eta,
                                                        const float* __restrict__ alpha_hat, int64_t numel) {
  const double at = (double)alpha_hat[t], ap = (double)alpha_hat[t_prev];
  double sig = 0.0;
  if (t_prev > 0 && eta > 0.f) sig = (double)eta * sqrt((1.0 - ap) / (1.0 - at)) * sqrt(1.0 - at / ap);
  const double A = sqrt(ap / at);
  const double B = sqrt(fmax(1.0 - ap - sig * sig, 0.0)) - sqrt(ap) * sqrt(1.0 - at) / sqrt(at);
  const float a = (float)A, b = (float)B, s = (float)sig;
  const bool add_noise = noise != nullptr && sig > 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x) {
    float e = ec[i];
    if (eu) {
      // torch.lerp(start = uncond, end = cond, w): |w| < 0.5 ? fma(w, diff, start) : end - diff * (1 - w)
      const float u = eu[i], d = __fsub_rn(e, u);
      e = fabsf(w) < 0.5f ? fmaf(w, d, u) : __fsub_rn(e, __fmul_rn(d, __fsub_rn(1.f, w)));
    }
    float v = __fadd_rn(__fmul_rn(a, x[i]), __fmul_rn(b, e));
    if (add_noise) v = __fadd_rn(v, __fmul_rn(s, noise[i]));
    x[i] = v;
  }
}

int ew_blocks(int64_t total) {
  int64_t b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int drs_ddim_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                             const float* noise, int t, int t_prev, float eta, const float* alpha_hat, int noise_steps,
                             int64_t numel, drs_stream_t stream) {
  DRS_REQUIRE(x && eps_cond && alpha_hat, DRS_ERR_ARG, "ddim_step: null pointer");
  DRS_REQUIRE(0 <= t_prev && t_prev < t && t < noise_steps, DRS_ERR_ARG,
              "ddim_step: need 0 <= t_prev < t < noise_steps, got t_prev=%d t=%d noise_steps=%d", t_prev, t, noise_steps);
  DRS_REQUIRE(std::isfinite(eta) && eta >= 0.f, DRS_ERR_ARG, "ddim_step: eta=%g must be finite and >= 0", (double)eta);
  // sigma > 0 exactly when eta > 0 and t_prev > 0 (alpha_hat decreases strictly along the schedule)
  DRS_REQUIRE(noise || !(eta > 0.f && t_prev > 0), DRS_ERR_ARG,
              "ddim_step: eta=%g > 0 and t_prev=%d > 0 need a noise tensor", (double)eta, t_prev);
  DRS_REQUIRE(numel >= 0, DRS_ERR_SHAPE, "ddim_step: numel=%lld", (long long)numel);
  if (numel == 0) return DRS_OK;
  DRS_LAUNCH(ddim_step_kernel, dim3(ew_blocks(numel)), dim3(256), 0, (hipStream_t)stream, x, eps_cond, eps_uncond,
             cfg_scale, noise, t, t_prev, eta, alpha_hat, numel);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
