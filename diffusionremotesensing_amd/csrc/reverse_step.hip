// The reverse-step entry points, element-wise and HBM-bound (every byte moves once; no atomics, no clamp): the reference's
// ancestral update (drs_sampler_step, with guidance drs_sampler_step_cfg), the DDIM update of Diffusion.sample(sampling_steps=S)
// (drs_ddim_step; Song et al., "Denoising Diffusion Implicit Models") and either with known pixels (drs_inpaint_step; RePaint,
// Lugmayr et al., CVPR 2022, Algorithm 1: the unknown pixels take the sampler's step, lines 6-7, the known ones become the known
// image forward-noised to t_prev, lines 4-5, merged by a per-element select, line 8); drs_renoise is the closed form of the
// forward steps of its resampling (line 10); drs_dpm_step is the DPM-Solver++(2M) move (Lu et al., 2022), which also keeps
// the x0 prediction of the move before.  Coefficients and per-element update: step_update.h, shared with tile_chain.hip.
#include "drs_common.h"
#include "step_update.h"

// The three schedule coefficients of one step are read back once per plan of T steps by the host
// wrapper (they are T-long tables living on the device); here they arrive as device tables and a scalar t,
// and a 1-thread prologue would cost a launch, so the kernel below reads them itself.
__global__ __launch_bounds__(256) void sampler_step_tab_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                                               const float* __restrict__ noise, int t,
                                                               const float* __restrict__ alpha,
                                                               const float* __restrict__ alpha_hat,
                                                               const float* __restrict__ beta, int64_t numel) {
  const DrsAncestralCoef k = drs_ancestral_coef(alpha, alpha_hat, beta, t);  // (step_update.h)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x) {
    float v = drs_ancestral_update(k, x[i], eps[i]);
    if (noise) v = drs_ancestral_noise(k, v, noise[i]);
    x[i] = v;
  }
}

extern "C" int drs_sampler_step(float* x, const float* eps_pred, const float* noise, int t, const float* alpha,
                                const float* alpha_hat, const float* beta, int noise_steps, int64_t numel,
                                drs_stream_t stream) {
  DRS_REQUIRE(x && eps_pred && alpha && alpha_hat && beta, DRS_ERR_ARG, "sampler_step: null pointer");
  if (int st = drs_check_move("sampler_step", false, 0, t, 0, 0.f, noise_steps, noise, DRS_NOISE_OPTIONAL)) return st;
  if (numel <= 0) return DRS_OK;
  DRS_LAUNCH(sampler_step_tab_kernel, dim3(ew_blocks(numel)), dim3(256), 0, (hipStream_t)stream, x, eps_pred,
                     noise, t, alpha, alpha_hat, beta, numel);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

__global__ void sampler_step_cfg_kernel(float* __restrict__ x, const float* __restrict__ ec,
                                        const float* __restrict__ eu, float w, const float* __restrict__ noise, int t,
                                        const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
                                        const float* __restrict__ beta, int64_t numel) {
  // same operations, in the same order and without fused multiply-adds, as the reference expressions
  // (train_diffusion_generation.py:239 torch.lerp, :249 the update): step_update.h
  const DrsAncestralCoef k = drs_ancestral_coef(alpha, alpha_hat, beta, t);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (int64_t)gridDim.x * blockDim.x) {
    float v = drs_ancestral_update(k, x[i], drs_cfg_lerp(eu[i], ec[i], w));
    if (noise) v = drs_ancestral_noise(k, v, noise[i]);
    x[i] = v;
  }
}
extern "C" int drs_sampler_step_cfg(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                                    const float* noise, int t, const float* alpha, const float* alpha_hat,
                                    const float* beta, int noise_steps, int64_t numel, drs_stream_t stream) {
  DRS_REQUIRE(x && eps_cond && eps_uncond && alpha && alpha_hat && beta, DRS_ERR_ARG, "sampler_step_cfg: null pointer");
  if (int st = drs_check_move("sampler_step_cfg", false, 0, t, 0, 0.f, noise_steps, noise, DRS_NOISE_OPTIONAL)) return st;
  if (numel <= 0) return DRS_OK;
  DRS_LAUNCH(sampler_step_cfg_kernel, dim3(ew_blocks(numel)), dim3(256), 0, (hipStream_t)stream, x, eps_cond,
                     eps_uncond, cfg_scale, noise, t, alpha, alpha_hat, beta, numel);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

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

// The unknown branch: the update of sampler_step_tab_kernel / sampler_step_cfg_kernel or of ddim_step_kernel
// above, bit for bit.  The coefficients come from the functions of step_update.h.  The per-element
// expressions of that header are plain products and sums (HIP's __fmul_rn / __fadd_rn are), which the compiler contracts
// into fused multiply-adds as the surrounding code suggests to it - differently in this kernel's unrolled groups than in
// the siblings' loops.  So the forms the siblings are compiled to are written out here, under contract(off):
//   ancestral   c_inv * fma(-c_eps, eps, x),  then fma(c_sig, z, v)
//   DDIM        fl(a * x) + fl(b * eps),      then fma(s, z, v)
//   guidance    |w| < 0.5 ? fma(w, d, uncond) : fma(-(1 - w), d, cond),  d = cond - uncond
// (tests/test_gpu_inpaint.py holds the two sides to torch.equal on every form.)
__device__ __forceinline__ float cfg_lerp(float uncond, float cond, float w) {
#pragma clang fp contract(off)
  const float d = cond - uncond;
  return fabsf(w) < 0.5f ? fmaf(w, d, uncond) : fmaf(-(1.f - w), d, cond);
}

template <bool DDIM>
struct MoveCoef;
template <>
struct MoveCoef<false> {
  DrsAncestralCoef k;
  __device__ MoveCoef(const float* alpha, const float* alpha_hat, const float* beta, int t, int, float)
      : k(drs_ancestral_coef(alpha, alpha_hat, beta, t)) {}
  __device__ bool draws() const { return true; }
  __device__ float step(float x, float eps) const {
#pragma clang fp contract(off)
    return k.c_inv * fmaf(-k.c_eps, eps, x);
  }
  __device__ float add(float v, float z) const { return fmaf(k.c_sig, z, v); }
};
template <>
struct MoveCoef<true> {
  DrsDdimCoef k;
  __device__ MoveCoef(const float*, const float* alpha_hat, const float*, int t, int t_prev, float eta)
      : k(drs_ddim_coef(alpha_hat, t, t_prev, eta)) {}
  __device__ bool draws() const { return k.has_sigma; }
  __device__ float step(float x, float eps) const {
#pragma clang fp contract(off)
    const float p = k.a * x, q = k.b * eps;
    return p + q;
  }
  __device__ float add(float v, float z) const { return fmaf(k.s, z, v); }
};

struct InpaintArgs {
  float* x;
  const float* ec;
  const float* eu;  // or null: no guidance
  float w;
  const float* noise;  // or null (t_prev == 0 only: checked on the host)
  const float* known;
  const unsigned char* mask;
  int planes, C, Cm;  // planes = n * C
  int64_t hw;
  int t, t_prev;
  float eta;
  const float *alpha, *alpha_hat, *beta;
};

// blockIdx.y strides over the n * C planes, blockIdx.x over the H * W / V groups of V consecutive pixels of one plane: the
// mask entry of a group is found from (image, pixel) - plane / C once per plane, no division per element - and a
// single-band mask (Cm == 1) is read by all C bands of its image.  V = 4 needs H * W % 4 == 0 and 16-byte aligned
// pointers: one float4 per tensor and the group's four mask bytes as one 32-bit word.
template <int V, bool DDIM>
__global__ __launch_bounds__(256) void inpaint_step_kernel(const InpaintArgs a) {
  const MoveCoef<DDIM> coef(a.alpha, a.alpha_hat, a.beta, a.t, a.t_prev, a.eta);
  const DrsKnownCoef kc(a.alpha_hat, a.t_prev);  // (step_update.h, shared with the tile blend)
  const bool add_noise = a.noise != nullptr && coef.draws();
  const bool to_zero = a.t_prev == 0;  // the known pixels arrive at the known image itself; z is not read for them
  const int64_t groups = a.hw / V;
  for (int plane = blockIdx.y; plane < a.planes; plane += gridDim.y) {
    const int64_t base = (int64_t)plane * a.hw;
    const unsigned char* mp = a.mask + (a.Cm == 1 ? (int64_t)(plane / a.C) * a.hw : base);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
      const int64_t at = base + g * V;
      float xs[V], es[V], ks[V], zs[V];
      unsigned m;
      if constexpr (V == 4) {
        const float4 x4 = *reinterpret_cast<const float4*>(a.x + at);
        const float4 e4 = *reinterpret_cast<const float4*>(a.ec + at);
        const float4 k4 = *reinterpret_cast<const float4*>(a.known + at);
        xs[0] = x4.x; xs[1] = x4.y; xs[2] = x4.z; xs[3] = x4.w;
        es[0] = e4.x; es[1] = e4.y; es[2] = e4.z; es[3] = e4.w;
        ks[0] = k4.x; ks[1] = k4.y; ks[2] = k4.z; ks[3] = k4.w;
        if (a.eu) {
          const float4 u4 = *reinterpret_cast<const float4*>(a.eu + at);
          es[0] = cfg_lerp(u4.x, es[0], a.w); es[1] = cfg_lerp(u4.y, es[1], a.w);
          es[2] = cfg_lerp(u4.z, es[2], a.w); es[3] = cfg_lerp(u4.w, es[3], a.w);
        }
        if (a.noise) {
          const float4 z4 = *reinterpret_cast<const float4*>(a.noise + at);
          zs[0] = z4.x; zs[1] = z4.y; zs[2] = z4.z; zs[3] = z4.w;
        }
        m = *reinterpret_cast<const unsigned*>(mp + g * 4);
      } else {
        xs[0] = a.x[at];
        es[0] = a.ec[at];
        ks[0] = a.known[at];
        if (a.eu) es[0] = cfg_lerp(a.eu[at], es[0], a.w);
        if (a.noise) zs[0] = a.noise[at];
        m = mp[g];
      }
#pragma unroll
      for (int p = 0; p < V; ++p) {
        float v = coef.step(xs[p], es[p]);
        if (add_noise) v = coef.add(v, zs[p]);
        if ((m >> (8 * p)) & 0xffu) v = to_zero ? ks[p] : kc.at(ks[p], zs[p]);
        xs[p] = v;
      }
      if constexpr (V == 4) *reinterpret_cast<float4*>(a.x + at) = make_float4(xs[0], xs[1], xs[2], xs[3]);
      else a.x[at] = xs[0];
    }
  }
}

// fl(A x) + fl(B z): both products rounded before the sum
__device__ __forceinline__ float jump_to(float A, float x, float B, float z) {
#pragma clang fp contract(off)
  const float p = A * x, q = B * z;
  return p + q;
}

// x = fl(A x) + fl(B z) over the flat tensor: float4 groups (`vec`: both pointers 16-byte aligned), then the numel % 4 tail.
__global__ __launch_bounds__(256) void renoise_kernel(float* __restrict__ x, const float* __restrict__ z, int s, int t,
                                                      const float* __restrict__ alpha_hat, int64_t numel, bool vec) {
  // the ratio in fp64: near T - 1 the cosine alpha_hat is ~1e-6 and an fp32 quotient would leave B with few digits
  const double r = (double)alpha_hat[t] / (double)alpha_hat[s];
  const float A = (float)sqrt(r), B = (float)sqrt(fmax(1.0 - r, 0.0));
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t groups = vec ? numel / 4 : 0;
  for (int64_t g = tid; g < groups; g += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[g];
    const float4 n = reinterpret_cast<const float4*>(z)[g];
    v.x = jump_to(A, v.x, B, n.x);
    v.y = jump_to(A, v.y, B, n.y);
    v.z = jump_to(A, v.z, B, n.z);
    v.w = jump_to(A, v.w, B, n.w);
    reinterpret_cast<float4*>(x)[g] = v;
  }
  for (int64_t i = groups * 4 + tid; i < numel; i += stride) x[i] = jump_to(A, x[i], B, z[i]);
}

// x0 = cx x + ce eps -> hist, x = A x + B eps + C hist (read before it is written, by a second-order move only): float4
// groups (`vec`: every pointer 16-byte aligned), then the numel % 4 tail.  Three reads and two writes per element.
__global__ __launch_bounds__(256) void dpm_step_kernel(float* __restrict__ x, const float* __restrict__ ec,
                                                       const float* __restrict__ eu, float w, float* __restrict__ hist,
                                                       int t_q, int t, int t_p, const float* __restrict__ alpha_hat,
                                                       int64_t numel, bool vec) {
  const DrsDpmCoef k = drs_dpm_coef(alpha_hat, t_q, t, t_p);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t groups = vec ? numel / 4 : 0;
  for (int64_t g = tid; g < groups; g += stride) {
    const float4 x4 = reinterpret_cast<const float4*>(x)[g];
    const float4 e4 = reinterpret_cast<const float4*>(ec)[g];
    float xs[4] = {x4.x, x4.y, x4.z, x4.w}, es[4] = {e4.x, e4.y, e4.z, e4.w}, hs[4] = {0.f, 0.f, 0.f, 0.f};
    if (eu) {
      const float4 u4 = reinterpret_cast<const float4*>(eu)[g];
      es[0] = drs_cfg_lerp(u4.x, es[0], w); es[1] = drs_cfg_lerp(u4.y, es[1], w);
      es[2] = drs_cfg_lerp(u4.z, es[2], w); es[3] = drs_cfg_lerp(u4.w, es[3], w);
    }
    if (k.second) {
      const float4 h4 = reinterpret_cast<const float4*>(hist)[g];
      hs[0] = h4.x; hs[1] = h4.y; hs[2] = h4.z; hs[3] = h4.w;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float x0 = drs_dpm_x0(k, xs[p], es[p]);
      xs[p] = drs_dpm_update(k, xs[p], es[p], hs[p]);
      hs[p] = x0;
    }
    reinterpret_cast<float4*>(hist)[g] = make_float4(hs[0], hs[1], hs[2], hs[3]);
    reinterpret_cast<float4*>(x)[g] = make_float4(xs[0], xs[1], xs[2], xs[3]);
  }
  for (int64_t i = groups * 4 + tid; i < numel; i += stride) {
    float e = ec[i];
    if (eu) e = drs_cfg_lerp(eu[i], e, w);
    const float xv = x[i], h = k.second ? hist[i] : 0.f;
    hist[i] = drs_dpm_x0(k, xv, e);
    x[i] = drs_dpm_update(k, xv, e, h);
  }
}

template <bool DDIM>
int launch_inpaint(const InpaintArgs& a, hipStream_t s) {
  const bool wide = a.hw % 4 == 0 && aligned16(a.x) && aligned16(a.ec) && aligned16(a.known) && ((uintptr_t)a.mask & 3u) == 0 &&
                    (!a.eu || aligned16(a.eu)) && (!a.noise || aligned16(a.noise));
  const int gx = ew_blocks(wide ? a.hw / 4 : a.hw);
  int gy = 8192 / gx;
  if (gy > a.planes) gy = a.planes;
  if (gy < 1) gy = 1;
  if (wide) DRS_LAUNCH((inpaint_step_kernel<4, DDIM>), dim3(gx, gy), dim3(256), 0, s, a);
  else DRS_LAUNCH((inpaint_step_kernel<1, DDIM>), dim3(gx, gy), dim3(256), 0, s, a);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

}  // namespace

extern "C" int drs_ddim_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale,
                             const float* noise, int t, int t_prev, float eta, const float* alpha_hat, int noise_steps,
                             int64_t numel, drs_stream_t stream) {
  DRS_REQUIRE(x && eps_cond && alpha_hat, DRS_ERR_ARG, "ddim_step: null pointer");
  if (int st = drs_check_move("ddim_step", true, 0, t, t_prev, eta, noise_steps, noise, DRS_NOISE_IF_SIGMA)) return st;
  DRS_REQUIRE(numel >= 0, DRS_ERR_SHAPE, "ddim_step: numel=%lld", (long long)numel);
  if (numel == 0) return DRS_OK;
  DRS_LAUNCH(ddim_step_kernel, dim3(ew_blocks(numel)), dim3(256), 0, (hipStream_t)stream, x, eps_cond, eps_uncond,
             cfg_scale, noise, t, t_prev, eta, alpha_hat, numel);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_dpm_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale, float* x0_hist, int t_q,
                            int t, int t_p, const float* alpha_hat, int noise_steps, int64_t numel, drs_stream_t stream) {
  DRS_REQUIRE(x && eps_cond && x0_hist && alpha_hat, DRS_ERR_ARG, "dpm_step: null pointer");
  if (int st = drs_check_dpm_move("dpm_step", t_q, t, t_p, noise_steps)) return st;
  DRS_REQUIRE(numel >= 0, DRS_ERR_ARG, "dpm_step: numel=%lld", (long long)numel);
  if (numel == 0) return DRS_OK;
  const bool vec = aligned16(x) && aligned16(eps_cond) && aligned16(x0_hist) && (!eps_uncond || aligned16(eps_uncond));
  DRS_LAUNCH(dpm_step_kernel, dim3(ew_blocks(vec ? (numel + 3) / 4 : numel)), dim3(256), 0, (hipStream_t)stream, x, eps_cond,
             eps_uncond, cfg_scale, x0_hist, t_q, t, t_p, alpha_hat, numel, vec);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" int drs_inpaint_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale, const float* noise,
                                const float* known, const uint8_t* mask, int n, int C, int H, int W, int mask_channels,
                                int ddim, int t, int t_prev, float eta, const float* alpha, const float* alpha_hat,
                                const float* beta, int noise_steps, drs_stream_t stream) {
  DRS_REQUIRE(x && eps_cond && known && mask && alpha_hat, DRS_ERR_ARG, "inpaint_step: null pointer");
  DRS_REQUIRE(n >= 0 && C >= 1 && H >= 0 && W >= 0, DRS_ERR_SHAPE, "inpaint_step: n=%d C=%d H=%d W=%d", n, C, H, W);
  DRS_REQUIRE(mask_channels == 1 || mask_channels == C, DRS_ERR_SHAPE,
              "inpaint_step: a mask of %d bands for an image of %d (1 or %d)", mask_channels, C, C);
  DRS_REQUIRE((int64_t)n * C <= INT32_MAX, DRS_ERR_SHAPE, "inpaint_step: n=%d x C=%d planes", n, C);
  if (!ddim) DRS_REQUIRE(alpha && beta, DRS_ERR_ARG, "inpaint_step: the ancestral form needs the alpha and beta tables");
  // above level 0 every element reads z: the unknown ones as the sampler's noise, the known ones as their forward noise
  if (int st = drs_check_move("inpaint_step", ddim, 1, t, t_prev, eta, noise_steps, noise, DRS_NOISE_ABOVE_0)) return st;
  if (!ddim) t_prev = t - 1;
  if (n == 0 || H == 0 || W == 0) return DRS_OK;
  InpaintArgs a;
  a.x = x; a.ec = eps_cond; a.eu = eps_uncond; a.w = cfg_scale; a.noise = noise; a.known = known; a.mask = mask;
  a.planes = n * C; a.C = C; a.Cm = mask_channels; a.hw = (int64_t)H * W;
  a.t = t; a.t_prev = t_prev; a.eta = eta; a.alpha = alpha; a.alpha_hat = alpha_hat; a.beta = beta;
  return ddim ? launch_inpaint<true>(a, (hipStream_t)stream) : launch_inpaint<false>(a, (hipStream_t)stream);
}

extern "C" int drs_renoise(float* x, const float* noise, int s, int t, const float* alpha_hat, int noise_steps, int64_t numel,
                           drs_stream_t stream) {
  DRS_REQUIRE(x && noise && alpha_hat, DRS_ERR_ARG, "renoise: null pointer");
  DRS_REQUIRE(1 <= s && s < t && t < noise_steps, DRS_ERR_ARG, "renoise: need 1 <= s < t < noise_steps, got s=%d t=%d noise_steps=%d",
              s, t, noise_steps);
  DRS_REQUIRE(numel >= 0, DRS_ERR_SHAPE, "renoise: numel=%lld", (long long)numel);
  if (numel == 0) return DRS_OK;
  const bool vec = aligned16(x) && aligned16(noise);
  DRS_LAUNCH(renoise_kernel, dim3(ew_blocks(vec ? (numel + 3) / 4 : numel)), dim3(256), 0, (hipStream_t)stream, x, noise, s, t,
             alpha_hat, numel, vec);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
