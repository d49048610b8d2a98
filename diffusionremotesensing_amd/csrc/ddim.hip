// DDIM update (Song et al., "Denoising Diffusion Implicit Models"): the strided-timestep sampler of Diffusion.sample
// (sampling_steps=S).  Element-wise and HBM-bound like the ancestral update in small_kernels.hip, which it leaves alone.
#include "drs_common.h"
#include "step_update.h"
#include <cmath>

namespace {

// The coefficients (fp64, rounded once) and the per-element update live in step_update.h, shared with the tile blend.
__global__ __launch_bounds__(256) void ddim_step_kernel(float* __restrict__ x, const float* __restrict__ ec,
                                                        const float* __restrict__ eu, float w,
                                                        const float* __restrict__ noise, int t, int t_prev, float eta,
                                                        const float* __restrict__ alpha_hat, int64_t numel) {
  const DrsDdimCoef k = drs_ddim_coef(alpha_hat, t, t_prev, eta);
  const bool add_noise = noise != nullptr && k.has_sigma;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x) {
    float e = ec[i];
    if (eu) e = drs_cfg_lerp(eu[i], e, w);
    float v = drs_ddim_update(k, x[i], e);
    if (add_noise) v = drs_ddim_noise(k, v, noise[i]);
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
