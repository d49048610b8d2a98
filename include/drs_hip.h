/*
 * drs_hip.h — C-ABI of the MI355X (gfx950) DDPM denoising hot path.
 *
 * This is the drop-in boundary: every entry point takes raw DEVICE pointers, explicit
 * shapes and a HIP stream, and returns an int status (0 = ok).  No torch types, no
 * exceptions, no ownership transfer: the caller (PyTorch's allocator in the shipped
 * host code) owns every buffer including the workspaces passed in.  The only opaque
 * state is `drs_plan`, created and destroyed explicitly.
 *
 * Each declaration cites the reference code it replaces.  Paths are relative to the
 * reference checkout of AdrianoEttari/DiffusionRemoteSensing (2024-10-22).
 *
 * Conventions: all floating tensors are fp32, row-major contiguous; images at the
 * boundary are NCHW exactly like the reference; timesteps are int64.  Internally the
 * plan keeps activations channels-last (NHWC) in the caller's workspace.
 */
#ifndef DRS_HIP_H
#define DRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: these entry points are its whole dynamic symbol table
 * (tests/test_abi_symbols.py checks exported == declared). */
#define DRS_API __attribute__((visibility("default")))

typedef void* drs_stream_t; /* hipStream_t; NULL = default stream */
typedef struct drs_plan drs_plan;

enum {
  DRS_OK = 0,
  DRS_ERR_ARG = 1,       /* null pointer / bad enum */
  DRS_ERR_SHAPE = 2,     /* shape the kernels do not support (e.g. H,W not divisible by 8) */
  DRS_ERR_HIP = 3,       /* a HIP runtime call failed; see drs_last_error() */
  DRS_ERR_WORKSPACE = 4, /* workspace / packed buffer too small */
  DRS_ERR_STATE = 5,     /* plan used before its weights were packed */
  DRS_ERR_RANGE = 6      /* drs_unet_check_faults: an activation left the range of the fp16 main operand of the FL arithmetic
                          * (csrc/conv_mfma_fl.hip) during a forward since the last check: that forward's result is invalid; the
                          * plan has switched itself to the split-bf16 kernels - run the forward / the chain again */
};

/* Convolution implementations (same arithmetic, different kernels). */
enum {
  DRS_IMPL_DIRECT = 0, /* fp32 VALU direct convolution: the on-device reference path */
  DRS_IMPL_MFMA_F32 = 1, /* LDS-tiled implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32) */
  DRS_IMPL_MFMA_BF16X3 = 2, /* implicit GEMM, operands split hi+lo bf16, 3 MFMAs per product */
  DRS_IMPL_MFMA_F16 = 3  /* implicit GEMM, fp16 operands, fp32 accumulate */
};

/* Threading: a drs_plan (and the buffers bound to it) is used by ONE host thread at a time - its launches, events and side
 * streams are not locked.  Every entry orders all of its work, side streams included, after the work already enqueued on the
 * `stream` it is given and before anything enqueued on that stream later.
 * Different plans may be driven from different threads and on different devices; the plan-less
 * entry points (noise_images, sampler steps, adam / ema, downblur, the feed gathers, aggregate) are re-entrant.  The library's only
 * process-wide state is a mutex-guarded per-device cache of kernel attributes, plus kernel-family switches read ONCE per
 * process from the environment (A/B experiments and the variant tests; unset = the shipped defaults): DRS_SP,
 * DRS_FL, DRS_WS, DRS_D3K, DRS_S2K, DRS_FUSE_GATE, DRS_UPFUSE, DRS_XT_ONLY, DRS_RB0, DRS_DOWNK, DRS_SP8,
 * DRS_FOLD_PROJ, DRS_GATE_PSI, DRS_CONCURRENT, DRS_TRAIN_BWD_IMPL, DRS_TRAIN_WGRAD_IMPL, DRS_WGRAD_STREAM.
 * Human-readable message for the last non-zero status returned on this thread. */
DRS_API const char* drs_last_error(void);
/* ABI version of this header; bumped on any signature change. */
DRS_API int drs_abi_version(void);  /* 8 */

/* ------------------------------------------------------------------------------------------
 * Diffusion arithmetic
 * ------------------------------------------------------------------------------------------ */

/* Forward process q(x_t | x_0): x_t[i] = sqrt(alpha_hat[t[i]]) * x0[i] + sqrt(1 - alpha_hat[t[i]]) * eps[i]
 * for n images of `chw` elements each.  `eps` is supplied by the caller (torch.randn_like).
 * Replaces Diffusion.noise_images, train_diffusion_superres.py:171-190. */
DRS_API int drs_noise_images(const float* x0, const float* eps, const int64_t* t, const float* alpha_hat,
                     int noise_steps, float* x_t, int n, int64_t chw, drs_stream_t stream);

/* One ancestral sampling update, in place on x:
 *   x = 1/sqrt(alpha[t]) * (x - (1 - alpha[t]) / sqrt(1 - alpha_hat[t]) * eps_pred) + sqrt(beta[t]) * noise
 * `noise` may be NULL (last step: reference uses zeros).  `t` is one scalar timestep shared by the
 * batch (the reference builds ones(n)*i).  Replaces the loop body at train_diffusion_superres.py:240-249. */
DRS_API int drs_sampler_step(float* x, const float* eps_pred, const float* noise, int t, const float* alpha,
                     const float* alpha_hat, const float* beta, int noise_steps, int64_t numel,
                     drs_stream_t stream);

/* Same update with classifier-free guidance folded in: eps = lerp(eps_uncond, eps_cond, cfg_scale) with torch.lerp's
 * formula (weight >= 0.5: end - (end - start) * (1 - weight)), then the ancestral update above.
 * Replaces generate_new_imgs/train_diffusion_generation.py:236-249. */
DRS_API int drs_sampler_step_cfg(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale, const float* noise,
                         int t, const float* alpha, const float* alpha_hat, const float* beta, int noise_steps,
                         int64_t numel, drs_stream_t stream);

/* One DDIM update (Song et al., "Denoising Diffusion Implicit Models"), in place on x, from timestep t to t_prev:
 *   eps   = eps_uncond ? lerp(eps_uncond, eps_cond, cfg_scale) : eps_cond   (torch.lerp, as drs_sampler_step_cfg)
 *   sigma = t_prev == 0 ? 0 : eta * sqrt((1 - ah_p) / (1 - ah_t)) * sqrt(1 - ah_t / ah_p)
 *   x     = sqrt(ah_p / ah_t) * x + (sqrt(max(1 - ah_p - sigma^2, 0)) - sqrt(ah_p) * sqrt(1 - ah_t) / sqrt(ah_t)) * eps
 *           + sigma * noise
 * with ah_t = alpha_hat[t], ah_p = alpha_hat[t_prev] read on the device.  The three coefficients are formed in fp64 and
 * rounded to fp32 once (near t = T - 1 of the cosine schedule ah_t is ~1e-6 and they reach ~+-900 on a long jump); the
 * per-element update is fp32.  The step to t_prev = 0 is deterministic whatever eta is (the reference adds zeros at its
 * last step).  `eps_uncond` and `noise` may be NULL; `noise` must be given when eta > 0 and t_prev > 0.
 * Requires 0 <= t_prev < t < noise_steps and a finite eta >= 0 (DRS_ERR_ARG otherwise). */
DRS_API int drs_ddim_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale, const float* noise,
                          int t, int t_prev, float eta, const float* alpha_hat, int noise_steps, int64_t numel,
                          drs_stream_t stream);

/* One DPM-Solver++(2M) move (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models",
 * 2022, Algorithm 2), in place on x, from level t to t_p, with the level t_q > t the previous move left (-1: none).  With
 * a = sqrt(ah), s = sqrt(1 - ah), lam = ln(a / s), E = (s_p / a_p)(a_t / s_t), phi = a_p (1 - E) and
 * r = (lam_t - lam_q) / (lam_p - lam_t):
 *   eps  = eps_uncond ? lerp(eps_uncond, eps_cond, cfg_scale) : eps_cond            (as drs_ddim_step)
 *   x0   = (x - s_t eps) / a_t
 *   x    = (s_p / s_t) x + phi ((1 + 1 / (2 r)) x0 - 1 / (2 r) x0_hist)             t_q >= 0 (second order)
 *   x    = (s_p / s_t) x + phi x0                                                    t_q == -1 (first order: the DDIM
 *                                                                                    eta = 0 move)
 * and x0 is then stored to x0_hist (numel fp32; written by every move, read by a second-order one only, so it may be
 * uninitialised at the first move of a chain).  The move is applied as x0 = cx x + ce eps, x = A x + B eps + C x0_hist with
 * five coefficients formed in fp64 from the device table and rounded to fp32 once; products and sums are fp32, rounded one
 * by one.  E is formed without logarithms: the move to level 0 must be first order (alpha_hat[0] may be 1).  16-byte
 * accesses when every pointer is 16-byte aligned, element by element otherwise.  DRS_ERR_ARG: null pointer (eps_uncond may
 * be NULL), not 0 <= t_p < t < noise_steps, t_q neither -1 nor in (t, noise_steps), t_q >= 0 with t_p == 0, numel < 0. */
DRS_API int drs_dpm_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale, float* x0_hist, int t_q,
                         int t, int t_p, const float* alpha_hat, int noise_steps, int64_t numel, drs_stream_t stream);

/* One reverse move t -> t_prev with known pixels (RePaint, Lugmayr et al., CVPR 2022, Algorithm 1, lines 4-8), in place on
 * x and in one pass (csrc/reverse_step.hip).  x, eps_cond, eps_uncond, noise, known: (n,C,H,W) fp32; mask: (n,mask_channels,H,W)
 * uint8 with mask_channels 1 (one entry per pixel, shared by the C bands) or C; a nonzero entry marks a known pixel.
 *   mask == 0:  the update of drs_sampler_step / drs_sampler_step_cfg (ddim == 0: t_prev = t - 1 is implied, `t_prev` and
 *               `eta` are ignored, alpha / alpha_hat / beta are read) or of drs_ddim_step (ddim != 0: alpha and beta may be
 *               NULL), guidance folded in when eps_uncond is given - the same bits as those entries.
 *   mask != 0:  x = known                                                          for t_prev == 0,
 *               x = sqrt(alpha_hat[t_prev]) * known + sqrt(1 - alpha_hat[t_prev]) * noise      otherwise
 *               (q(x_t_prev | known); both factors formed in fp64 and rounded once, products and sum rounded one by one).
 * One noise tensor serves both branches: an element uses noise[i] either as the sampler's noise or as the forward noise of
 * its known pixel.  `noise` may be NULL only for t_prev == 0 (DRS_ERR_ARG otherwise, whatever eta is); `known` is used as
 * given (no clamp).  16-byte accesses need H * W % 4 == 0 and 16-byte aligned pointers; any other shape runs element by
 * element.  No atomics: two calls give the same bits.  DRS_ERR_ARG: null pointer, ddim == 0 and not 1 <= t < noise_steps,
 * ddim != 0 and not 0 <= t_prev < t < noise_steps or eta negative or not finite; DRS_ERR_SHAPE: mask_channels not 1 or C. */
DRS_API int drs_inpaint_step(float* x, const float* eps_cond, const float* eps_uncond, float cfg_scale, const float* noise,
                             const float* known, const uint8_t* mask, int n, int C, int H, int W, int mask_channels, int ddim,
                             int t, int t_prev, float eta, const float* alpha, const float* alpha_hat, const float* beta,
                             int noise_steps, drs_stream_t stream);

/* One forward jump from level s to level t > s >= 1, in place: x = sqrt(r) * x + sqrt(1 - r) * noise with
 * r = alpha_hat[t] / alpha_hat[s] - the closed form of the t - s single forward steps of RePaint's resampling (Algorithm 1,
 * line 10).  r and both factors are formed in fp64 from the device table and rounded once (near t = T - 1 of the cosine
 * schedule alpha_hat is ~1e-6).  DRS_ERR_ARG: null pointer, not 1 <= s < t < noise_steps. */
DRS_API int drs_renoise(float* x, const float* noise, int s, int t, const float* alpha_hat, int noise_steps, int64_t numel,
                        drs_stream_t stream);

/* What the network predicts (csrc/prediction.hip; not in the reference, whose networks all predict the noise). */
enum {
  DRS_PRED_EPS = 0, /* the noise eps */
  DRS_PRED_V = 1,   /* v = sqrt(alpha_hat) eps - sqrt(1 - alpha_hat) x0 */
  DRS_PRED_X0 = 2   /* the clean image x0 */
};

/* The forward process and the v target of a training batch in one pass: per image i of `chw` elements, with
 * a = sqrtf(alpha_hat[t[i]]) and b = sqrtf(1 - alpha_hat[t[i]]) in fp32,
 *   x_t = fl(a x0) + fl(b eps)          v = fl(a eps) - fl(b x0)
 * every product and sum rounded on its own (no fused multiply-add): x_t is the documented value of the entry above.
 * A t[i] outside [0, noise_steps) does not index the table: x_t and v of that image are NaN, the other images are untouched
 * by it.  x_t and v must be two buffers.  16-byte accesses when x0, eps, x_t and v start at the same place of a 16-byte line
 * (chw need not be a multiple of 4: each image then has a scalar head and tail), element by element otherwise.
 * DRS_ERR_ARG: null pointer, x_t == v; DRS_ERR_SHAPE: n < 0, chw < 0, noise_steps <= 0. */
DRS_API int drs_noise_v_target(const float* x0, const float* eps, const int64_t* t, const float* alpha_hat, int noise_steps,
                               float* x_t, float* v, int n, int64_t chw, drs_stream_t stream);

/* A prediction of `kind` (DRS_PRED_*) as the eps the reverse-step entries take, against the x the network saw; n images of
 * `chw` elements, t: n int64 levels on the device.  Per image a = sqrt(ah), s = sqrt(1 - ah) are formed in fp64 from the fp32
 * table entry ah = alpha_hat[t[i]]; every coefficient below is rounded to fp32 once, products and sums are fp32 and rounded one
 * by one.  First p = pred_uncond ? lerp(pred_uncond, pred, cfg_scale) : pred   (torch.lerp, as the guided step entries).
 *   clip == 0:   EPS: eps = p      V: eps = s x + a p      X0: eps = (1/s) x + (-a/s) p
 *   clip != 0:   x0 = EPS: (1/a) x + (-s/a) p    V: a x + (-s) p    X0: p
 *                x0c = min(max(x0, lo), hi) for a finite x0, x0 itself otherwise (a NaN or an infinity of the network is
 *                never clamped into range);     eps = (1/s) x + (-a/s) x0c
 * Where s == 0 (ah == 1: level 0 of the cosine table) the forms that divide by s give eps = 0; where a == 0 an EPS prediction
 * is passed through unclipped.  A t[i] outside [0, noise_steps) does not index the table: that image's eps is NaN.
 * `out` may be `pred` (in place); `pred_uncond` may be NULL.  Accesses as drs_noise_v_target (pred, pred_uncond, x, out).
 * DRS_ERR_ARG: null pointer, unknown kind, clip with lo >= hi, pred_uncond with a cfg_scale that is not finite;
 * DRS_ERR_SHAPE: n < 0, chw < 0, noise_steps <= 0. */
DRS_API int drs_pred_to_eps(const float* pred, const float* pred_uncond, float cfg_scale, const float* x, const int64_t* t,
                            const float* alpha_hat, int noise_steps, int kind, int clip, float lo, float hi, float* out, int n,
                            int64_t chw, drs_stream_t stream);

/* Dynamic thresholding of the implied x0 (Saharia et al., "Imagen", 2022, section 2.3), per image, in place of the static clip of
 * drs_pred_to_eps (arguments as there; the clip range [lo, hi] is mandatory).  With c = (float)((lo + hi) / 2) and
 * r = (float)((hi - lo) / 2), formed in double, and x0 the clip path's value before its clamp:
 *   d = fl(x0 - c),  key = bits(|d|) as an unsigned integer, a NaN or an infinity ranked as +inf (0x7f800000)
 *   s = the value whose key is the k-th smallest (0-based) of the image's chw keys, all bands together: an exact order
 *       statistic, torch.quantile(|d|, p, interpolation="lower") for k = floor(p (chw - 1)); no interpolation
 *   s <= r, or s not finite:  q = clamp(x0, lo, hi), the bits drs_pred_to_eps gives that image with clip != 0
 *   otherwise:                q = clamp(c + clamp(d, -s, s) * rho, lo, hi),  rho = (float)((double)r / s)
 *   eps = fl(ea x) + fl(eb q) with the clip path's coefficients; a non-finite x0 element is never clamped.
 * Products and sums are fp32 and rounded one by one.  Images at a level where drs_pred_to_eps does not form an x0 (s == 0,
 * an EPS prediction where a == 0, a t[i] outside the table) get exactly its result and the scale 0: nothing is thresholded.
 * The selection is a radix select over the 31 key bits (digits of 11, 10 and 10 bits, one streaming pass each, integer
 * counts only): s and every output are bitwise reproducible.  No allocation, no device-to-host copy, no synchronisation:
 * `workspace` (device, 4-byte aligned, >= drs_x0_threshold_workspace_bytes(n) bytes) is zeroed on `stream` by the call.
 *
 * drs_x0_quantile: the selection alone.  out = the implied x0 (the eps of drs_pred_to_eps for the images named last above),
 * scale[i] = s of image i as found, before the s <= r rule.
 * drs_pred_to_eps_dyn: the whole operation; out = eps, scale_out (optional, may be NULL) as `scale` above.
 * `out` may be `pred`; `x` must not be `out` (x is read again after out has been written).
 * DRS_ERR_ARG: null pointer (pred, x, t, alpha_hat, out, workspace, scale of drs_x0_quantile), unknown kind, lo >= hi,
 * pred_uncond with a cfg_scale that is not finite, x == out, k outside [0, chw), workspace_bytes too small;
 * DRS_ERR_SHAPE: n < 0, chw < 0 or chw >= 2^32, noise_steps <= 0.  n == 0 or chw == 0: DRS_OK, nothing is done. */
DRS_API size_t drs_x0_threshold_workspace_bytes(int n);
DRS_API int drs_x0_quantile(const float* pred, const float* pred_uncond, float cfg_scale, const float* x, const int64_t* t,
                            const float* alpha_hat, int noise_steps, int kind, float lo, float hi, int64_t k, float* out,
                            float* scale, int n, int64_t chw, void* workspace, size_t workspace_bytes, drs_stream_t stream);
DRS_API int drs_pred_to_eps_dyn(const float* pred, const float* pred_uncond, float cfg_scale, const float* x, const int64_t* t,
                                const float* alpha_hat, int noise_steps, int kind, float lo, float hi, int64_t k, float* out,
                                float* scale_out, int n, int64_t chw, void* workspace, size_t workspace_bytes,
                                drs_stream_t stream);

/* The reverse move away from the terminal level of a zero-terminal-SNR schedule (alpha_hat[t] == 0; Lin et al., "Common
 * Diffusion Noise Schedules and Sample Steps Are Flawed", 2024; csrc/terminal_step.hip), in place on x (n,C,H,W), one scalar t
 * and t_prev for all images as in drs_ddim_step.  At that level x is the noise itself and the network names x0 directly, so the
 * move divides by nothing.  Per element, with ah_p = alpha_hat[t_prev] read on the device (for t_prev == 0 too, as drs_ddim_step):
 *   p     = pred_uncond ? lerp(pred_uncond, pred, cfg_scale) : pred              (torch.lerp, as the guided step entries)
 *   x0    = kind == DRS_PRED_V ? -p : p
 *   x0    = clip, scale == NULL: min(max(x0, lo), hi) for a finite x0, x0 itself otherwise     (as drs_pred_to_eps)
 *           scale != NULL (needs clip): the rule of drs_pred_to_eps_dyn with s = scale[image] and its fp32 c and r: the static
 *           clamp (its bits) where s <= r or s is not finite; otherwise clamp(c + (clamp(x0 - c, -s, s) / s) r, lo, hi), which
 *           is evaluated in fp64 from the fp32 inputs (the guidance lerp included) and rounded to fp32 once - that entry's
 *           fp32 steps round around c and s, many ulps of a result next to the lower edge of a (0, 1) range; an element
 *           clamped to c +- s lands on lo / hi exactly
 *   x0_hist = x0                                                                  (if given: the history of drs_dpm_step)
 *   sigma = t_prev == 0 ? 0 : eta sqrt(1 - ah_p),   c0 = sqrt(ah_p),   c1 = sqrt(max(0, (1 - ah_p)(1 - eta^2)))
 *   x     = fl(fl(c0 x0) + fl(c1 x)) + fl(sigma noise)                            (the last term only where sigma != 0)
 * The coefficients are formed in fp64 from the fp32 table entry and rounded to fp32 once; products and sums are fp32, rounded one
 * by one.  eta = 1 is the true posterior at beta_t = 1: mean sqrt(ah_p) x0, variance 1 - ah_p.  Where mask != 0 (known, mask as in
 * drs_inpaint_step; both NULL: no known pixels) the element is exactly drs_inpaint_step's known-pixel value for that t_prev and
 * noise.  `noise` is required iff t_prev > 0 and (eta > 0 or there are known pixels).
 * If alpha_hat[t] != 0 on the device, or not 0 <= t_prev < t < noise_steps, every output of the call (x, x0_hist) is NaN and the
 * table is not indexed outside its bounds: the convention of drs_pred_to_eps.  16-byte accesses when x, pred, pred_uncond, noise,
 * known and x0_hist start at the same place of a 16-byte line (rows as drs_noise_v_target), element by element otherwise.
 * DRS_ERR_ARG (x untouched): null x / pred / alpha_hat, kind not DRS_PRED_V or DRS_PRED_X0, known without mask or the reverse,
 * clip with lo >= hi, scale without clip, a cfg_scale that is not finite, eta outside [0, 1], a missing noise, x0_hist == x;
 * DRS_ERR_SHAPE: n < 0, C < 1, H < 0, W < 0, noise_steps <= 0, mask_channels neither 1 nor C. */
DRS_API int drs_terminal_step(float* x, const float* pred, const float* pred_uncond, float cfg_scale, const float* noise,
                              const float* known, const uint8_t* mask, int mask_channels, int kind, int clip, float lo, float hi,
                              const float* scale, float* x0_hist, int n, int C, int H, int W, int t, int t_prev, float eta,
                              const float* alpha_hat, int noise_steps, drs_stream_t stream);

/* Guidance rescale (the same paper, section 3.4), per image of `chw` elements:
 *   g   = lerp(uncond, cond, cfg_scale)                      (torch.lerp, fp32, as the guided step entries)
 *   f   = 1 + phi (std(cond) / std(g) - 1)                   fp64, rounded to fp32 once; both stds over the image's chw elements
 *   out = fl(g f)
 * std(g) == 0 or a ratio that is not finite gives f = 1.  Two launches on `stream`, no atomics and no host synchronisation:
 * the first writes, per chunk of 4096 elements, fp64 sums and sums of squares of cond - cond[0] and g - g[0] (added in a fixed
 * order: per thread in element order, a shuffle tree over the wave, the four waves in order); the second adds an image's
 * partials in index order in every block and scales.  Two calls give the same bits.  `out` may be `cond`.  `workspace`: device,
 * 8-byte aligned, >= drs_cfg_rescale_workspace_bytes(n, chw) bytes.
 * DRS_ERR_ARG: null pointer, cfg_scale not finite, phi outside [0, 1], workspace too small; DRS_ERR_SHAPE: n < 0, chw < 0,
 * n > 65535. */
DRS_API size_t drs_cfg_rescale_workspace_bytes(int n, int64_t chw);
DRS_API int drs_cfg_rescale(const float* cond, const float* uncond, float cfg_scale, float phi, float* out, int n, int64_t chw,
                            void* workspace, size_t workspace_bytes, drs_stream_t stream);

/* One Adam step over many tensors in ONE launch (torch.optim.Adam defaults: no weight decay, no amsgrad):
 *   m = lerp(m, g, 1-beta1); v = v*beta2 + (1-beta2)*g*g; p -= lr/(1-beta1^step) * m / (sqrt(v)/sqrt(1-beta2^step) + eps)
 * `table` (device): ntensors x drs_adam_tensor {p, g, m, v, n, step}; entries with g == NULL are skipped (parameters
 * that got no gradient, like torch).  `step` is that tensor's 1-based step count after the increment (torch keeps one
 * per parameter: a parameter that skipped steps has its own bias correction).
 * Replaces `optimizer.step()` of torch.optim.Adam in the training loop body, train_diffusion_superres.py:337,393. */
typedef struct drs_adam_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int64_t step;
} drs_adam_tensor;
DRS_API int drs_adam_multi(const drs_adam_tensor* table, int ntensors, int64_t max_numel, double lr, double beta1, double beta2,
                   double eps, drs_stream_t stream);

/* AdamW with global-norm gradient clipping and a non-finite guard, as TWO launches on one stream and no host
 * synchronisation (torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, which the reference leaves commented out next to
 * Adam, train_diffusion_superres.py:337-338).  Both use the grid of drs_adam_multi: (chunks of 4096 elements, tensors).
 *
 * `table` (device): ntensors x drs_adamw_tensor = drs_adam_tensor's fields + `part0`, the index of the tensor's first chunk
 * in `partials` (chunk c of the tensor owns partials[part0 + c]; the caller lays the tensors out back to back, so
 * npartials = sum over tensors of ceil(n / 4096)).
 *
 * drs_grad_sumsq_partials: every chunk writes ONE double, the sum of (double)g * (double)g over the chunk, added in a fixed
 * order (per thread in element order, a shuffle tree over the wave, the four waves in order): two calls give the same bits.
 * Chunks of tensors with g == NULL write 0.
 *
 * drs_adamw_clip_multi: every block first adds partials[0 .. npartials) in index order (so all blocks hold the same S; no
 * atomics, no fence, no ticket), then with norm = sqrt(S) in double:
 *   skip:  if skip_nonfinite != 0 and S is not finite, p, m and v of EVERY tensor are left untouched;
 *   coef = max_norm > 0 ? (float)min(1.0, max_norm / (norm + 1e-6)) : 1.0f        (clip_grad_norm_; a NaN stays NaN)
 *   g'   = g * coef                                                               (rounded once; exact at coef == 1)
 *   p    = p * (float)(1.0 - lr * weight_decay)                                   (AdamW's param.mul_, before the update)
 *   then drs_adam_multi's update of m, v and p with g' in place of g, operation for operation.
 * With max_norm <= 0, weight_decay == 0 and finite gradients the result is bit-identical to drs_adam_multi's.
 * npartials == 0 (partials may be NULL) means S = 0: no clipping and no guard, one launch (max_norm > 0 is DRS_ERR_ARG then).
 * `stats` (device, may be NULL) is written by block (0,0): the pre-clip norm, coef, whether this step was skipped, and a
 * count of skipped steps that the kernel increments (zero it once).  The caller's per-tensor `step` counts attempted steps: after
 * a skip the bias correction is one step ahead (documented deviation; it costs no synchronisation). */
typedef struct drs_adamw_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int64_t step;
  int64_t part0;
} drs_adamw_tensor;
typedef struct drs_adamw_stats {
  float norm;
  float coef;
  int32_t skipped;
  int32_t reserved;
  int64_t skipped_total;
} drs_adamw_stats;
DRS_API int drs_grad_sumsq_partials(const drs_adamw_tensor* table, int ntensors, int64_t max_numel, double* partials,
                                    drs_stream_t stream);
DRS_API int drs_adamw_clip_multi(const drs_adamw_tensor* table, int ntensors, int64_t max_numel, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, double max_norm, int skip_nonfinite,
                                 const double* partials, int npartials, drs_adamw_stats* stats, drs_stream_t stream);

/* The training objective: loss value, gradient and per-image losses from ONE pass over the data, plus a small ordered finish
 * launched behind it on the same stream (no atomics, no host synchronisation; two calls on the same inputs give the same bits
 * in every output).  pred, target: (B, n) fp32 contiguous; with d = pred - target formed in fp32 and l = torch's mse_loss /
 * l1_loss / huber_loss(delta) element function,
 *   per_image[b] = (1/n) sum_i l(d[b,i])                     double, summed in double in a fixed order
 *   w_b          = table[t[b]] * sample_w[b]                 double; a NULL table or sample_w is a factor 1
 *   loss         = (1/B) sum_b w_b * per_image[b]            out[0] as double, and as fp32 in the 4 bytes at out + 1
 *   grad[b,i]    = (float)(w_b c / (B n)) * l'(d[b,i])       c = 2, l' = d for MSE; c = 1, l' = sign(d) (0 at 0) for MAE; Huber:
 *                                                            l' = d for |d| <= delta, else (float)(w_b delta / (B n)) * sign(d)
 * `grad` may be NULL (validation: nothing is written).  `table` holds T floats and is indexed by t (B int64, device); `t` may be
 * NULL when neither a table nor bins are given.  `partials`: workspace of B * ((n + 3) / 4096 + 1) doubles.
 *
 * `bins` (may be NULL): 3 nbins + 1 + nbins history 8-byte words on the device, zeroed once by the caller -
 *   double sum[nbins]; int64 count[nbins]; int64 appended[nbins]; int64 nonfinite; double ring[nbins][history]
 * - with bin(t) = t nbins / T (integer division).  In batch order every finite per_image[b] is added to sum / count of its bin and,
 * when update_ring != 0, written to ring[bin][appended % history] (appended counts them: the ring holds the last `history`
 * losses of the bin); a non-finite one only raises `nonfinite`.  `loss` carries it all the same.
 * A t[b] outside [0, T), with a table or bins: nothing is read or binned for that image, its weight is NaN (so `loss` and its
 * gradient row are) and *bad_t (device int64, may be NULL, never reset here) grows by one: the caller reads it where it
 * synchronises anyway.
 * DRS_ERR_ARG: null pointer, unknown kind, Huber with delta <= 0, a table or bins without t or T, nbins outside 2 .. min(64, T / 2),
 * history outside 1 .. 32; DRS_ERR_SHAPE: B outside 1 .. 65535, n < 1.  All are reported before anything is launched. */
enum { DRS_LOSS_MSE = 0, DRS_LOSS_MAE = 1, DRS_LOSS_HUBER = 2 };
DRS_API int drs_diffusion_loss(const float* pred, const float* target, const int64_t* t, int B, int64_t n, const float* table,
                               int T, const float* sample_w, int kind, double delta, float* grad, double* per_image,
                               double* partials, double* out, double* bins, int nbins, int history, int update_ring,
                               int64_t* bad_t, drs_stream_t stream);

/* Loss-aware timesteps (the loss-second-moment resampler of Nichol & Dhariwal 2021, per bin) from the ring of `bins` (layout
 * above) and two uniforms per sample, u1, u2 in [0, 1) (B floats each): t (B int64, in 1 .. T - 1) and sample_w (B floats).
 * With cnt_k the number of timesteps 1 .. T - 1 in bin k: while any bin has appended < history,
 *   t = 1 + min(T - 2, floor(u1 (T - 1))), sample_w = 1;
 * afterwards r_k = sqrt(mean of ring[k]^2), p_k = (1 - eps) r_k / sum r + eps / nbins (p_k = 1 / nbins when sum r == 0), k = the
 * first bin whose cumulative p exceeds u1 (the last bin if none does), t = the floor(u2 cnt_k)-th of bin k's timesteps and
 * sample_w = cnt_k / ((T - 1) p_k), the ratio uniform / proposal.  p and its cumulative sums are formed in double, in index
 * order.  DRS_ERR_ARG: null pointer, eps outside [0, 1], nbins / history as above; DRS_ERR_SHAPE: B < 1. */
DRS_API int drs_timestep_draw(const double* bins, int nbins, int history, const float* u1, const float* u2, int B, int T,
                              double eps_uniform, int64_t* t, float* sample_w, drs_stream_t stream);

/* Multi-tensor exponential moving average of the parameters, ONE launch for all tensors:
 *   mode 0:  ema[i] = ema[i] * beta + (1 - beta) * cur[i]   (fp32; `1 - beta` is formed in double and rounded to fp32, the
 *            two products and the sum are rounded separately - reference EMA.update_average, UNet_model_superres.py:25-30,
 *            applied per parameter by EMA.update_model_average :18-23);
 *   mode 1:  ema[i] = cur[i] as 32-bit words (the warm-up copy of EMA.reset_parameters :52-55, which load_state_dict()s
 *            parameters AND buffers: int64 counters are two words).
 * `table` (device): ntensors x drs_ema_tensor {ema, cur, n}; n counts 32-bit elements.  Replaces the 176 (mode 0) /
 * 299 (mode 1) small kernels of `ema.step_ema(ema_model, model)` in the training loop body, train_diffusion_superres.py:396. */
typedef struct drs_ema_tensor {
  void* ema;
  const void* cur;
  int64_t n;
} drs_ema_tensor;
DRS_API int drs_ema_multi(const drs_ema_tensor* table, int ntensors, int64_t max_numel, double beta, int mode, drs_stream_t stream);

/* Gaussian-weighted blend of n overlapping super-resolved tiles into one image, normalised and clamped to [0,1]:
 *   out[c][y][x] = clamp( sum_i w[y-y0_i][x-x0_i] * tiles[i][c][y-y0_i][x-x0_i] / sum_i w[y-y0_i][x-x0_i], 0, 1 )
 * over the tiles i (in index order, like the reference's sequential `+=`) whose window [y0_i, y0_i+S) x [x0_i, x0_i+S)
 * contains (y, x).  tiles: (n,C,S,S); origins: n x 2 int32 (y0, x0) on the device; weight: (S,S); out: (C,H,W).
 * Returns DRS_ERR_SHAPE through `uncovered` (device int, may be NULL) != 0 semantics: the count of output pixels no
 * tile covers is written there (the reference asserts pixel_count != 0).
 * Replaces the loop + normalisation of split_aggregation_sampling.aggregation_sampling, Aggregation_Sampling.py:90-116. */
DRS_API int drs_aggregate_tiles(const float* tiles, const int32_t* origins, const float* weight, float* out, int32_t* uncovered,
                        int n, int C, int S, int H, int W, drs_stream_t stream);

/* drs_aggregate_tiles with the clamp as an argument and optional known pixels (the final blend of a tiled scene whose data
 * range is not [0,1], NDVI in [-1,1] for one, or that keeps given pixels): the same sums in the same order, then
 *   out = known          where mask != 0 (known, mask: both NULL or both given),
 *   out = clamp(out, lo, hi)   when clamp != 0, known pixels included; clamp == 0 writes the quotient as it is.
 * known: (C,H,W) fp32; mask: (mask_channels,H,W) uint8 with mask_channels 1 or C, nonzero = known.  `uncovered` as in
 * drs_aggregate_tiles (a covered-by-no-tile pixel counts whether it is known or not).  With clamp = (0, 1) and no known
 * pixels the output is that of drs_aggregate_tiles, bit for bit.  DRS_ERR_ARG: null pointer, known without mask or the
 * reverse, lo > hi; DRS_ERR_SHAPE: as drs_aggregate_tiles, mask_channels not 1 or C. */
DRS_API int drs_aggregate_tiles_known(const float* tiles, const int32_t* origins, const float* weight, const float* known,
                                      const uint8_t* mask, float* out, int32_t* uncovered, int n, int C, int S, int H, int W,
                                      int mask_channels, int clamp, float lo, float hi, drs_stream_t stream);

/* Per-step tile aggregation (split_aggregation_sampling.sample_scene; csrc/tile_chain.hip): one state of scene size is
 * denoised, the tiles' noise predictions are blended at every reverse step.  Not in the reference.
 *
 * Cut `count` tiles out of a scene: tiles[k] = scene[:, y0:y0+S, x0:x0+S] with (y0, x0) = origins[min(first + k, n - 1)],
 * a pure copy (bit-exact).  scene: (C,Hs,Ws); origins: n x 2 int32 (y0, x0) on the device, the table drs_aggregate_tiles
 * takes; tiles: (count,C,S,S).  `first` / `count` select a chunk of the n tiles without staging the whole set; a chunk
 * that runs past tile n - 1 repeats the last tile (the padding of a fixed-size chunk).  An origin whose window leaves the
 * scene is not read: that tile is written as zeros.  Requires 0 <= first < n, count >= 1 (DRS_ERR_ARG) and
 * 1 <= S <= Hs, Ws (DRS_ERR_SHAPE). */
DRS_API int drs_gather_tiles(const float* scene, const int32_t* origins, float* tiles, int first, int count, int n, int C,
                             int S, int Hs, int Ws, drs_stream_t stream);

/* One ancestral reverse step of a scene state, in place and in one launch, from the noise predictions of its n tiles:
 *   eps[c][y][x] = sum_i w[y-y0_i][x-x0_i] * eps_tiles[i][c][y-y0_i][x-x0_i] / sum_i w[y-y0_i][x-x0_i]
 * over the tiles i that cover (y, x), in index order (the sums of drs_aggregate_tiles: deterministic, no atomics), without a
 * clamp, followed by exactly the update of drs_sampler_step with that eps (`noise`, of scene shape, may be NULL: last step).
 * scene, noise: (C,Hs,Ws); eps_tiles: (n,C,S,S); origins: n x 2 int32 on the device; weight: (S,S).
 * `uncovered` (device int, may be NULL) is INCREASED by the number of pixels no tile covers (their state becomes NaN); it is
 * not reset here, so that a chain reads it once.  16-byte accesses need S % 4 == 0 and Ws % 4 == 0; any other shape runs
 * element by element.  DRS_ERR_ARG: null pointer, t outside [0, noise_steps); DRS_ERR_SHAPE: n, C, S < 1, S > Hs or S > Ws. */
DRS_API int drs_blend_step(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                           const float* noise, int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t,
                           const float* alpha, const float* alpha_hat, const float* beta, int noise_steps,
                           drs_stream_t stream);

/* The same blend followed by exactly the update of drs_ddim_step (no guidance) from timestep t to t_prev: coefficients
 * formed in fp64 from the device table and rounded once, deterministic step to t_prev = 0.  `noise` may be NULL unless
 * eta > 0 and t_prev > 0.  DRS_ERR_ARG: null pointer, not 0 <= t_prev < t < noise_steps, eta negative or not finite,
 * missing noise when sigma > 0; DRS_ERR_SHAPE as drs_blend_step. */
DRS_API int drs_blend_step_ddim(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                                const float* noise, int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t,
                                int t_prev, float eta, const float* alpha_hat, int noise_steps, drs_stream_t stream);

/* The same blend followed by exactly the move of drs_dpm_step (no guidance) from level t to t_p on the scene state, with a
 * history `x0_hist` of scene shape (C,Hs,Ws) and the previous level t_q (-1: first order).  It draws no noise.  `x0_hist` is
 * accessed like `scene` and `noise` (16 bytes per access when S and Ws are multiples of 4; unlike drs_dpm_step there is no
 * element-wise path for a base pointer that is not 16-byte aligned) and must not overlap `scene`.
 * DRS_ERR_ARG: null pointer, or a move drs_dpm_step refuses; DRS_ERR_SHAPE as drs_blend_step. */
DRS_API int drs_blend_step_dpm(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                               float* x0_hist, int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t_q, int t,
                               int t_p, const float* alpha_hat, int noise_steps, drs_stream_t stream);

/* drs_blend_step / drs_blend_step_ddim (`ddim` selects the form, as in drs_inpaint_step: ddim == 0 implies t_prev = t - 1,
 * ignores `t_prev` and `eta` and reads alpha / alpha_hat / beta; ddim != 0 reads alpha_hat only) followed, in the same launch,
 * by the known-pixel select of drs_inpaint_step on the scene state (RePaint over a tiled scene).  known: (C,Hs,Ws) fp32, used
 * as given; mask: (mask_channels,Hs,Ws) uint8 with mask_channels 1 or C, nonzero = known.  Per element, after the blended eps
 * and the step:
 *   mask == 0:  the value drs_blend_step / drs_blend_step_ddim writes, bit for bit;
 *   mask != 0:  known for t_prev == 0, else sqrt(alpha_hat[t_prev]) * known + sqrt(1 - alpha_hat[t_prev]) * noise, the
 *               arithmetic (and the bits) of drs_inpaint_step.
 * One noise tensor serves both branches; `noise` may be NULL only for t_prev == 0 (DRS_ERR_ARG otherwise, whatever eta is).
 * `uncovered` and the 16-byte path (S % 4 == 0 and Ws % 4 == 0) as in drs_blend_step; there `known` is read 16 bytes and the
 * mask 4 bytes at a time when their base pointers are so aligned, element by element otherwise.  No atomics on the data path:
 * two calls give the same bits.  DRS_ERR_ARG: null pointer, a move drs_inpaint_step refuses; DRS_ERR_SHAPE as
 * drs_blend_step, mask_channels not 1 or C. */
DRS_API int drs_blend_step_known(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                                 const float* noise, const float* known, const uint8_t* mask, int32_t* uncovered, int n, int C,
                                 int S, int Hs, int Ws, int mask_channels, int ddim, int t, int t_prev, float eta,
                                 const float* alpha, const float* alpha_hat, const float* beta, int noise_steps,
                                 drs_stream_t stream);

/* Image-quality sums of an estimate `sr` against the truth `hr`, per image (csrc/metrics.hip; finalised into PSNR, SSIM, SAM
 * and ERGAS by diffusionremotesensing_amd/metrics.py).  Not in the reference, which only looks at its samples.
 *   sr, hr: (B,C,H,W) fp32, 1 <= C <= 16;  clamp != 0: both are clamped to [0, 1] as they are loaded (the reference clamps
 *   a sample before showing it, superres_and_NDVIgen.py:49; a NaN stays a NaN).
 * Both entry points reduce deterministically (fp32 in the block, one fp64 partial per block in `workspace`, a fixed-order
 * sum of the partials; no atomics): two calls on the same inputs write the same bits.  One workspace of
 * drs_metrics_workspace_bytes(B, C, H, W) bytes serves either call (0 for a shape neither takes).
 * DRS_ERR_ARG: null pointer; DRS_ERR_SHAPE: B or C < 1, C > 16, B > 65535, H or W < 1 (drs_ssim: < 11);
 * DRS_ERR_WORKSPACE: workspace too small.
 *
 * drs_metrics_pointwise, one pass over both tensors: out is B x (2 C + 2) doubles,
 *   out[b][c]         = sum over pixels of (sr - hr)^2 of band c
 *   out[b][C + c]     = sum over pixels of hr of band c
 *   out[b][2 C]       = sum over pixels of the angle (radians) between the C-vectors of sr and hr at that pixel, formed as
 *                       2 atan2(|u^ - v^|, |u^ + v^|) on the normalised vectors (exactly 0 for identical vectors)
 *   out[b][2 C + 1]   = the number of pixels in that sum: a pixel whose vector is exactly zero in either image has no angle
 * 16-byte loads need H * W % 4 == 0 and 16-byte aligned tensors; anything else runs element by element.
 *
 * drs_ssim: out[b] = mean over bands and over the (H - 10) x (W - 10) "valid" window positions of the SSIM of Wang et al.
 * 2004: 11 x 11 Gaussian window, sigma 1.5, normalised; K1 = 0.01, K2 = 0.03, data range 1.  Moments are formed on values
 * centred on a per-tile pivot. */
DRS_API size_t drs_metrics_workspace_bytes(int B, int C, int H, int W);
DRS_API int drs_metrics_pointwise(const float* sr, const float* hr, double* out, int B, int C, int H, int W, int clamp,
                                  void* workspace, size_t workspace_bytes, drs_stream_t stream);
DRS_API int drs_ssim(const float* sr, const float* hr, double* out, int B, int C, int H, int W, int clamp, void* workspace,
                     size_t workspace_bytes, drs_stream_t stream);

/* Training and scoring on imagery with no-data pixels (csrc/nodata.hip; not in the reference).  One rule everywhere: a pixel of
 * a clean / truth image (C, H, W) is NO-DATA when any of its bands is NaN, or when `nodata_value` is finite and all of its bands
 * equal it (fp32 compare); nodata_value = NaN means "the NaN rule only".  The mask is per pixel, shared by the bands, and taken
 * from the image as stored, before any clamp.  No-data elements are selected out, not multiplied by zero: a NaN or an infinity
 * there reaches no output.  No atomics, no host synchronisation: two calls give the same bits.  Every refusal below is reported
 * before anything is launched.
 *
 * drs_noise_target_nodata: x_t, the training target and the mask of a batch x0 (n, C, hw) from one pass.  valid: (n, hw) uint8,
 * 1 = data.  At a valid pixel x_t has the bits of drs_noise_images and target those of eps (DRS_PRED_EPS), of drs_noise_v_target's
 * v (DRS_PRED_V) or of x0 (DRS_PRED_X0); at a no-data pixel x_t = fl(a fill) + fl(b eps) and target = +0.0.  A t[i] outside
 * [0, noise_steps) makes x_t and target of that image NaN and its valid 0, and reads no table entry.  16-byte accesses (and one
 * 32-bit store of four mask decisions) need hw % 4 == 0, 16-byte aligned fp32 tensors and a 4-byte aligned mask; anything else
 * runs element by element.  DRS_ERR_ARG: null pointer, x_t == target, unknown kind; DRS_ERR_SHAPE: C outside 1 .. 16, n < 0,
 * hw < 0, noise_steps <= 0.  n == 0 or hw == 0: DRS_OK, nothing is done.
 *
 * drs_diffusion_loss_masked: drs_diffusion_loss over the valid elements of pred, target (B, C, hw) under valid (B, hw) uint8
 * (non-zero = data).  With nv_b the valid pixels of image b (written to counts, B int64), n_b = C nv_b and Bv the images with
 * nv_b > 0:
 *   per_image[b] = (1/n_b) sum over valid elements of l(d)          0 when nv_b = 0
 *   loss         = (1/Bv) sum over nv_b > 0 of w_b per_image[b]     0 when Bv = 0
 *   grad[b,i]    = (float)(w_b c / (Bv n_b)) * l'(d[b,i])           +0.0 at no-data elements; Huber's outer branch likewise
 * An image with nv_b = 0 enters neither bins nor ring.  Chunks, order and precision of the sums are drs_diffusion_loss's: when
 * every pixel is valid every output has its bits.  `partials`: workspace of B * ((C hw + 3) / 4096 + 1) doubles.  Three
 * launches on the stream: the count of the mask rows, the streaming pass, the finish.  Refusals as drs_diffusion_loss, and
 * DRS_ERR_ARG for a null valid or counts, DRS_ERR_SHAPE for C outside 1 .. 16 or hw < 1.
 *
 * drs_metrics_pointwise_nodata: out is B x (2 C + 3) doubles: the 2 C + 2 sums of drs_metrics_pointwise over the valid pixels
 * of hr, then out[b][2 C + 2] = nv_b.  drs_ssim_nodata: out is B x 2 doubles: out[b][0] = the mean SSIM over the bands and over
 * the window positions whose 11 x 11 pixels are all valid (NaN when there is none), out[b][1] = the number of such positions
 * (per band).  The per-tile pivot is the tile's middle pixel or, when that is no-data, the first valid pixel of the tile in row
 * order.  drs_ssim_nodata first writes hr's mask into the workspace (one pass over hr, one byte per pixel), so that the blocks
 * of a tile's C bands read a byte per pixel instead of every band.  With every pixel valid the shared outputs have the bits of
 * drs_metrics_pointwise / drs_ssim.  One workspace of drs_metrics_nodata_workspace_bytes(B, C, H, W) bytes (the partial rows,
 * then B H W mask bytes) serves either call.  Refusals as drs_metrics_pointwise / drs_ssim. */
DRS_API int drs_noise_target_nodata(const float* x0, const float* eps, const int64_t* t, const float* alpha_hat, int noise_steps,
                                    int kind, float nodata_value, float fill, float* x_t, float* target, uint8_t* valid, int n,
                                    int C, int64_t hw, drs_stream_t stream);
DRS_API int drs_diffusion_loss_masked(const float* pred, const float* target, const uint8_t* valid, const int64_t* t, int B,
                                      int C, int64_t hw, const float* table, int T, const float* sample_w, int kind, double delta,
                                      float* grad, double* per_image, int64_t* counts, double* partials, double* out,
                                      double* bins, int nbins, int history, int update_ring, int64_t* bad_t, drs_stream_t stream);
DRS_API size_t drs_metrics_nodata_workspace_bytes(int B, int C, int H, int W);
DRS_API int drs_metrics_pointwise_nodata(const float* sr, const float* hr, float nodata_value, double* out, int B, int C, int H,
                                         int W, int clamp, void* workspace, size_t workspace_bytes, drs_stream_t stream);
DRS_API int drs_ssim_nodata(const float* sr, const float* hr, float nodata_value, double* out, int B, int C, int H, int W,
                            int clamp, void* workspace, size_t workspace_bytes, drs_stream_t stream);

/* Per-pixel statistics and scores of an ensemble of N samples of one conditional distribution (csrc/ensemble.hip; public
 * API in diffusionremotesensing_amd/ensemble.py).  The reference draws its n_generations samples and plots them.
 *   members: (N,B,C,H,W) fp32, member axis first, 2 <= N <= 32;  truth: (B,C,H,W) fp32;  clamp != 0: members and truth are
 *   clamped to [lo, hi] as they are loaded (a NaN stays a NaN).  With the sorted members s_0 <= ... <= s_{N-1} of an element:
 *     mean = sum(s) / N;  std = sqrt(sum (s_i - mean)^2 / (N - 1));
 *     quantile(q): pos = q (N - 1), k = floor(pos), s_k + (pos - k) (s_{min(k+1,N-1)} - s_k)   (q = 0, 1: min and max exactly);
 *     crps = 1/N sum |s_i - y| - 1/N^2 sum_i (2 i - N + 1) s_i;  rank = #{i : s_i < y}.
 *   The sort and the comparisons are exact fp32; the sums, the interpolation and the CRPS are fp64 over the sorted order and
 *   are rounded to fp32 once, at the store of a map.  An element with a NaN member (or a NaN truth, in drs_ensemble_scores)
 *   gets NaN in its maps, is left out of the rank histogram and makes its image's three sums NaN.  Each member element is
 *   read once; 16-byte loads need an element count divisible by 4 (B C H W for the maps, C H W for the scores) and 16-byte
 *   aligned tensors, anything else runs element by element.  Two calls on the same inputs write the same bits.
 * DRS_ERR_ARG: null pointer where one is not allowed, lo > hi; DRS_ERR_SHAPE: N outside 2 .. 32, Q outside 0 .. 8, a q outside
 * [0, 1], B, C, H or W < 1, B > 65535; DRS_ERR_WORKSPACE: workspace too small.  All are reported before anything is launched.
 *
 * drs_ensemble_stats: mean, std (B,C,H,W) and quantiles (Q,B,C,H,W); each may be NULL (quantiles only with Q == 0) and is then
 *   not computed.  q: Q host doubles.
 * drs_ensemble_scores: crps_map (B,C,H,W) or NULL; sums: B x 3 doubles = per image the sum over C, H, W of crps | of the
 *   variance sum (s_i - mean)^2 / (N - 1) | of (mean - y)^2, from the fp64 per-element values; rank_histogram: B x (N + 1)
 *   counts of the elements of the image by rank.  Partials go through `workspace`, drs_ensemble_workspace_bytes(N, B, C, H,
 *   W) bytes (0 for arguments the call does not take), and are added in a fixed order: no floating-point atomics. */
DRS_API size_t drs_ensemble_workspace_bytes(int N, int B, int C, int H, int W);
DRS_API int drs_ensemble_stats(const float* members, float* mean, float* std, float* quantiles, const double* q, int Q, int N,
                               int B, int C, int H, int W, int clamp, float lo, float hi, drs_stream_t stream);
DRS_API int drs_ensemble_scores(const float* members, const float* truth, float* crps_map, double* sums,
                                int64_t* rank_histogram, int N, int B, int C, int H, int W, int clamp, float lo, float hi,
                                void* workspace, size_t workspace_bytes, drs_stream_t stream);

/* Colour correction of a super-resolved batch against a guide of its size - the up-sampled LR observation - per (image, band)
 * plane (csrc/colorfix.hip; public API in diffusionremotesensing_amd/colorfix.py).  A diffusion super-resolver drifts
 * radiometrically; this post-process keeps the sample's fine detail and takes the large-scale content of the guide (the colour
 * fix StableSR ships next to its aggregation sampling).  Not in the reference.
 *   sr, guide, out: (B,C,H,W) fp32, 1 <= C <= 16;  `out` must not overlap `sr` or `guide`.  Nothing is clamped; a NaN goes where
 *   the arithmetic takes it.  Two calls on the same inputs write the same bits.
 * DRS_ERR_ARG: null pointer, `out` overlapping an input; DRS_ERR_SHAPE: B, C, H or W < 1, C > 16, levels outside 1 .. 5, H W < 2
 * (drs_colorfix_adain); DRS_ERR_WORKSPACE: workspace too small.  All are reported before anything is launched.
 *
 * drs_colorfix_wavelet: with k = (1/4, 1/2, 1/4) and
 *     blur_d(x)[y][x] = sum_{i,j in -1..1} k_i k_j x[clamp(y + i d, 0, H-1)][clamp(x + j d, 0, W-1)]
 *   (a 3 x 3 convolution of dilation d on replicate padding) and low_L = blur_{2^(L-1)} o ... o blur_2 o blur_1, L = levels:
 *     out = sr + low_L(guide - sr)      (= (sr - low_L(sr)) + low_L(guide): the map is linear)
 *   One launch for all levels: a workgroup stages guide - sr of a 64 x 64 tile and its halo of 2^L - 1 pixels (clipped to the
 *   image) in LDS and runs the L separable blurs there, clamping in image coordinates.  guide == sr returns sr bit for bit.
 *   Any H, W >= 1; 16-byte stores need W % 4 == 0 and 16-byte aligned sr and out, anything else is written element by element.
 *
 * drs_colorfix_adain: with mean and unbiased variance (divisor H W - 1) of each plane of sr and of guide, std = sqrt(var + 1e-5):
 *     out = a sr + b,   a = std_guide / std_sr,   b = mean_guide - a mean_sr
 *   The sums of x and x^2 are carried in fp64 (per thread, per block in `workspace`, then added in a fixed order: no atomics),
 *   a and b are formed in fp64 and rounded to fp32 once, out = fma(a, sr, b).  `workspace`: 8-byte aligned,
 *   drs_colorfix_adain_workspace_bytes(B, C, H, W) bytes (0 for a shape the call does not take).  16-byte accesses need
 *   H W % 4 == 0 and 16-byte aligned tensors; anything else runs element by element. */
DRS_API int drs_colorfix_wavelet(const float* sr, const float* guide, float* out, int B, int C, int H, int W, int levels,
                                 drs_stream_t stream);
DRS_API size_t drs_colorfix_adain_workspace_bytes(int B, int C, int H, int W);
DRS_API int drs_colorfix_adain(const float* sr, const float* guide, float* out, int B, int C, int H, int W, void* workspace,
                               size_t workspace_bytes, drs_stream_t stream);

/* LR-consistent sampling (csrc/consistency.hip; not in the reference): the damped range-null-space
 * projection of an image onto the images a separable linear degradation A_y . A_x^T maps to the observation.  All tensors are
 * fp32 and row-major; x: (n,c,H,W); with the thin SVDs A = P diag(s) V^T per axis the caller holds
 *   d_y (h,H) = diag(s_y) V_y^T,  d_x (w,W);  u_y (H,h) = V_y,  u_x (W,w);  gain (h,w);  yt (n,c,h,w) = P_y^T y P_x per plane.
 * drs_sep_apply:        out (n,c,h,w) = d_y x d_x^T per plane, for any pair of matrices of those shapes (the degradation itself,
 *                       the residual basis, or - with P_y^T (h,h) and P_x^T (w,w) on an (n,c,h,w) input - yt).
 * drs_sep_project:      out = x + strength u_y (gain o (yt - d_y x d_x^T)) u_x^T per plane; out may be x.
 * drs_sep_project_eps:  the same on the x0 that the noise prediction `eps` implies for the state `x` at the levels t (n int64
 *                       on the device), x0 = (x - sqrt(1 - ah) eps) / sqrt(ah), formed as it is loaded and never stored; eps is
 *                       replaced by the prediction of the projected x0, eps - sqrt(ah / (1 - ah)) strength (the correction).  The
 *                       coefficients are formed in fp64 from the device table and rounded once (as drs_ddim_step's).  A level
 *                       outside the table never indexes it: that image's eps comes out NaN (as drs_pred_to_eps; t lives on the
 *                       device and is not read back).  No chain calls it at a level with ah == 0 or ah == 1.
 * Every product is an exact fp32 multiply-add chain (v_mfma_f32_16x16x4_f32) in a fixed order, without atomics: two calls give
 * the same bits, and so does a call whose pointers are not 16-byte aligned (4-byte loads of the same elements).  strength == 0
 * launches nothing (drs_sep_project: one copy when out != x).  No host synchronisation.  workspace: 4-byte aligned,
 * >= drs_sep_workspace_bytes(n, c, H, W, h, w) bytes (0 for a shape the calls do not take).
 * DRS_ERR_ARG: null pointer, strength not finite, noise_steps < 1, eps == x; DRS_ERR_SHAPE: c > 16, any extent < 1, a plane or
 * a matrix of 2^31 elements; DRS_ERR_WORKSPACE: workspace too small or misaligned.  All are reported before any launch. */
DRS_API size_t drs_sep_workspace_bytes(int n, int c, int H, int W, int h, int w);
DRS_API int drs_sep_apply(const float* x, const float* d_y, const float* d_x, float* out, int n, int c, int H, int W, int h,
                          int w, void* workspace, size_t workspace_bytes, drs_stream_t stream);
DRS_API int drs_sep_project(const float* x, const float* yt, const float* d_y, const float* d_x, const float* u_y,
                            const float* u_x, const float* gain, float strength, float* out, int n, int c, int H, int W,
                            int h, int w, void* workspace, size_t workspace_bytes, drs_stream_t stream);
DRS_API int drs_sep_project_eps(float* eps, const float* x, const int64_t* t, const float* alpha_hat, int noise_steps,
                                const float* yt, const float* d_y, const float* d_x, const float* u_y, const float* u_x,
                                const float* gain, float strength, int n, int c, int H, int W, int h, int w, void* workspace,
                                size_t workspace_bytes, drs_stream_t stream);

/* Per-band operators (not in the reference): the three calls above with one operator per band.  d_y, d_x,
 * u_y, u_x and gain carry a leading n_ops axis - d_y (n_ops,h,H), d_x (n_ops,w,W), u_y (n_ops,H,h), u_x (n_ops,W,w), gain
 * (n_ops,h,w) - and band b of every image uses slot band_op[b].  band_op: c int32 values in 0 .. n_ops-1 in HOST memory, copied
 * into the kernel arguments before the call returns; NULL: band b uses slot min(b, n_ops-1).  yt stays per plane.  Same tiles,
 * same MFMA order, same workspace and same contract as the calls above, which are these with n_ops = 1 and keep their bits.
 * DRS_ERR_SHAPE besides theirs: n_ops outside 1 .. c, a band_op entry outside 0 .. n_ops-1. */
DRS_API int drs_sep_apply_bands(const float* x, const float* d_y, const float* d_x, float* out, int n, int c, int H, int W, int h,
                                int w, const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                                drs_stream_t stream);
DRS_API int drs_sep_project_bands(const float* x, const float* yt, const float* d_y, const float* d_x, const float* u_y,
                                  const float* u_x, const float* gain, float strength, float* out, int n, int c, int H, int W,
                                  int h, int w, const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                                  drs_stream_t stream);
DRS_API int drs_sep_project_eps_bands(float* eps, const float* x, const int64_t* t, const float* alpha_hat, int noise_steps,
                                      const float* yt, const float* d_y, const float* d_x, const float* u_y, const float* u_x,
                                      const float* gain, float strength, int n, int c, int H, int W, int h, int w,
                                      const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                                      drs_stream_t stream);

/* Sensor-MTF degradation (csrc/mtf.hip, diffusionremotesensing_amd/mtf.py; not in the reference): a
 * separable FIR blur and decimation by m in one launch, with one pair of tap rows per operator slot:
 *   out[i][j] = sum_u ky[op][u] * sum_v kx[op][v] * x[clamp(i m + u - Ly, 0, H-1)][clamp(j m + v - Lx, 0, W-1)],  op = band_op[band]
 * x: (n,c,H,W) fp32; taps_y (n_ops,ntaps_y), taps_x (n_ops,ntaps_x) fp32 on the device; band_op as in the *_bands calls above
 * (host, c int32, may be NULL); out: (n,c,h,w) with h m <= H and w m <= W (rows and columns past h m, w m are only ever taps).
 * noise (n,c,h,w) standard normals with sigma (c fp32 on the device), both or neither: v = fmaf(sigma[band], z, v); clamp01 != 0:
 * v = min(max(v, 0), 1) last.  A workgroup stages the clamped input window of its LR tile in LDS, runs the row-direction pass
 * (kx, along W) and then the column-direction pass (ky) from there, each an fmaf chain from 0 in ascending tap order: the sum
 * depends on nothing but the output pixel, so two calls, any pointer phase (16-byte loads where pointer, W and plane stride allow
 * them, 4-byte loads of the same elements otherwise) and any tile position give the same bits.  No atomics, no workspace, no host
 * synchronisation.  DRS_ERR_ARG: null pointer, noise without sigma or the reverse, x and out overlapping; DRS_ERR_SHAPE: c > 16,
 * n_ops outside 1 .. c, a band_op entry outside 0 .. n_ops-1, m outside 1 .. 8, ntaps outside 1 .. 64, L outside 0 .. ntaps-1,
 * h m > H or w m > W, an extent < 1, a plane of 2^31 elements.  All are reported before the launch. */
DRS_API int drs_fir_decimate(const float* x, const float* taps_y, const float* taps_x, const int32_t* band_op, int n_ops,
                             int ntaps_y, int ntaps_x, int Ly, int Lx, int m, const float* noise, const float* sigma,
                             int clamp01, float* out, int n, int c, int H, int W, int h, int w, drs_stream_t stream);

/* "DownBlur" degradation of the super-resolution data feed on the device, bit-exact with the Pillow calls of the
 * reference's dataset item: x = ToTensor(GaussianBlur(radius)(resize(y, (out_w, out_h), BICUBIC))), y = ToTensor(hr).
 *   hr: (N,C,H,W) uint8;  x_lr: (N,C,out_h,out_w) float32 in [0,1];  y_hr: (N,C,H,W) float32 or NULL;
 *   blur_radius: Pillow's GaussianBlur radius (0 = no blur);  scratch: drs_downblur_scratch_bytes(...) bytes.
 * Replaces get_data_superres.__getitem__, utils.py:140-158 (Gauss_noise=False). */
DRS_API size_t drs_downblur_scratch_bytes(int N, int C, int H, int W, int out_h, int out_w);
DRS_API int drs_downblur_u8(const uint8_t* hr, int N, int C, int H, int W, int out_h, int out_w, float blur_radius, float* x_lr,
                    float* y_hr, void* scratch, size_t scratch_bytes, drs_stream_t stream);

/* The device half of the dataset item's `Gauss_noise=True` step: x (N,C,H,W) float32 += noise (N,H,W,C) float32, clipped to
 * [0, 1], in place.  The noise is drawn on the host from the generators the reference uses (Python `random`, numpy's global
 * generator), in its order, by diffusionremotesensing_amd.degradation.reference_noise.
 * Replaces the add and the clip of add_Gaussian_noise, utils.py:27-36 (called at utils.py:163-164). */
DRS_API int drs_add_noise_clip_f32(float* x, const float* noise_nhwc, int N, int C, int H, int W, drs_stream_t stream);

/* One batch of the SAR -> NDVI data feed from the decoded dataset on the device, both tensors of the pair in one launch:
 *   sar_out[i, :] = (sar_cache[idx[i], :] + 1) * 0.5,  ndvi_out[i, :] = (ndvi_cache[idx[i], :] + 1) * 0.5   for i < n
 * sar_cache: (L, sar_row) fp32, ndvi_cache: (L, ndvi_row) fp32 (a row = one C x H x W image as the file holds it, in [-1, 1]);
 * idx: n int64 on the device; sar_out: (n, sar_row), ndvi_out: (n, ndvi_row).  An index outside [0, L) reads nothing: its two
 * output rows are zeros.  16-byte loads and stores where a cache row and its output row are aligned alike, element by element
 * otherwise; no workspace.  Replaces get_data_SAR_TO_NDVI.__getitem__'s `(img + 1) / 2` and the DataLoader's collation,
 * utils.py:65-91. */
DRS_API int drs_gather_pairs_f32(const float* sar_cache, const float* ndvi_cache, const int64_t* idx, int n, int64_t L,
                                 int sar_row, int ndvi_row, float* sar_out, float* ndvi_out, drs_stream_t stream);

/* One batch of the class-folder data feed from the decoded uint8 dataset on the device:
 *   img_out[i, :] = float(cache_u8[idx[i], :]) / 255 (a true division: ToTensor's `.div(255)`),  labels_out[i] = labels[idx[i]]
 * cache_u8: (L, row) uint8; labels: L int64; idx: n int64 on the device; img_out: (n, row) fp32; labels_out: n int64.  An index
 * outside [0, L) reads nothing: its row is zeros, its label -1.  One 16-byte load feeds four 16-byte stores where the rows are
 * aligned for it; no workspace.  Replaces torchvision's ToTensor on an ImageFolder item and the DataLoader's collation,
 * generate_new_imgs/train_diffusion_generation.py:574-584. */
DRS_API int drs_gather_u8_f32(const uint8_t* cache_u8, const int64_t* labels, const int64_t* idx, int n, int64_t L, int row,
                              float* img_out, int64_t* labels_out, drs_stream_t stream);

/* Random crops and dihedral augmentation of the device feeds (csrc/augment.hip, diffusionremotesensing_amd/augment.py; DESIGN.md
 * section 20): one launch writes a batch of n windows.  items: (n, 4) int32 on the device, items[i] = (src, y0, x0, code): the
 * S x S window of cache image src with top-left corner (y0, x0) under dihedral code 0..7 -
 *   if code & 4: w = w.swapaxes(-1, -2);  if code & 1: w = w[..., ::-1];  if code & 2: w = w[..., ::-1, :]   (in this order)
 * i.e. out[i, c, y, x] = cache[src, c, y0 + y', x0 + x'] with (u, v) = (code & 2 ? S-1-y : y, code & 1 ? S-1-x : x) and
 * (y', x') = code & 4 ? (v, u) : (u, v).  All bands of an item, and both tensors of a pair, share window and code.  An item with
 * src outside [0, L), a window that does not lie inside H x W or a code outside 0..7 reads nothing: zeros, label -1.
 *   drs_crop_d4_u8:        cache (L, C, H, W) uint8 -> out (n, C, S, S) uint8, the bytes themselves
 *   drs_crop_d4_u8_f32:    the same cache -> img_out (n, C, S, S) fp32 = float(b) / 255 (a true division, as drs_gather_u8_f32),
 *                          labels_out[i] = labels[src]  (labels: L int64, labels_out: n int64)
 *   drs_crop_d4_pairs_f32: sar_cache (L, Cs, H, W), ndvi_cache (L, Cn, H, W) fp32 -> sar_out (n, Cs, S, S), ndvi_out (n, Cn, S, S)
 *                          = (v + 1) * 0.5, as drs_gather_pairs_f32
 * H != W is allowed, the window is square.  No workspace, no atomics.  DRS_ERR_ARG: null pointer; DRS_ERR_SHAPE: n, L, a band
 * count, H, W or S < 1, S > H or S > W.  Not in the reference's device path: its BSRGAN dataset cut `num_crops` random patches on
 * the host (utils.py:205-210, degradation_from_BSRGAN.py:584), its other datasets do not augment. */
DRS_API int drs_crop_d4_u8(const uint8_t* cache_u8, const int32_t* items, int n, int64_t L, int C, int H, int W, int S,
                           uint8_t* out, drs_stream_t stream);
DRS_API int drs_crop_d4_u8_f32(const uint8_t* cache_u8, const int64_t* labels, const int32_t* items, int n, int64_t L, int C,
                               int H, int W, int S, float* img_out, int64_t* labels_out, drs_stream_t stream);
DRS_API int drs_crop_d4_pairs_f32(const float* sar_cache, const float* ndvi_cache, const int32_t* items, int n, int64_t L,
                                  int Cs, int Cn, int H, int W, int S, float* sar_out, float* ndvi_out, drs_stream_t stream);

/* 16-bit radiometry (csrc/radiometry.hip, diffusionremotesensing_amd/radiometry.py): a uint16 scene cache
 * (L, C, H, W) of digital numbers beside the uint8 one.  range: (C, 2) fp32 on the device, range[c] = (lo_c, hi_c), hi_c > lo_c,
 * both in 0 .. 65535 (the caller checks); the span hi_c - lo_c is formed once in fp32.  Every step below is one correctly
 * rounded fp32 operation (no contraction):
 *   normalise:  x = min(max((float(v) - lo_c) / (hi_c - lo_c), 0), 1)
 *   quantise:   v = clamp(rint(min(max(x, 0), 1) * (hi_c - lo_c) + lo_c), 0, 65535), rint to even; a NaN x gives `fill`
 * so quantise(normalise(v)) == v for every v in [lo_c, hi_c].  nodata: -1 (none) or the stored value 0 .. 65535 that marks a
 * no-data pixel when ALL C bands of the pixel hold it (compared on the integers).  1 <= C <= 16.
 *   drs_hist_u16:        counts (C, 65536) uint64, zeroed by the entry on `stream`, then the exact number of pixels of band c
 *                        that hold each value, over the whole cache, no-data pixels left out.  Integer atomics: the result is
 *                        the same in every run.
 *   drs_crop_d4_u16_f32: the batch launch of the 16-bit feed: items (n, 4) int32 and the dihedral rule as drs_crop_d4_u8 above;
 *                        hr (n, C, S, S) fp32 = the normalised windows; hr_marked (NULL: not written) the same values with NaN
 *                        in all bands of every no-data pixel.  An invalid item reads nothing: zeros in both.
 *   drs_quantize_u16:    x (n, C, HW) fp32 -> out (n, C, HW) uint16.
 * Vector accesses only where the address is aligned for them (a uint16 row starts on any 2-byte phase), element-wise otherwise,
 * with the same bits.  No workspace, no host synchronisation.  DRS_ERR_ARG: null or misaligned pointer, nodata / fill out of range;
 * DRS_ERR_SHAPE: an extent < 1, C > 16, S > H or W, more than 2^40 elements.  Replaces: none - not in the reference, whose
 * datasets are 8-bit (`(y * 255).astype(np.uint8)`, utils.py:131-133). */
DRS_API int drs_hist_u16(const uint16_t* cache_u16, int64_t L, int C, int H, int W, int nodata, uint64_t* counts,
                         drs_stream_t stream);
DRS_API int drs_crop_d4_u16_f32(const uint16_t* cache_u16, const int32_t* items, int n, int64_t L, int C, int H, int W, int S,
                                const float* range, int nodata, float* hr, float* hr_marked, drs_stream_t stream);
DRS_API int drs_quantize_u16(const float* x, int n, int C, int64_t HW, const float* range, int fill, uint16_t* out,
                             drs_stream_t stream);

/* The ops of the blind (BSRGAN-plus) degradation feed (csrc/bsr_degrade.hip; recipe and feed in diffusionremotesensing_amd/bsr.py,
 * definitions in DESIGN.md section 19).  Every op is one launch (sharpen and jpeg: two) over a dense (N,C,H,W) fp32 batch, 1 <= C
 * <= 16; per-image parameters are device arrays, so a batch's whole recipe is one upload.  Nothing draws random numbers.
 * DRS_ERR_ARG: null pointer, overlapping tensors, unknown mode; DRS_ERR_SHAPE: sizes; DRS_ERR_WORKSPACE: scratch too small.
 *
 * drs_bsr_blur: out[n][c] = kernel_n (*) x[n][c], a TRUE convolution (scipy.ndimage.convolve: the kernel is flipped) with the
 *   border continued by reflection about the edge pixels' centres (cv2 BORDER_REFLECT_101, scipy "mirror"), repeated as often as
 *   the image's size asks.  kernels: (N,K,K) fp32 on the device, K odd, 1 <= K <= 25; ksizes: N int32 on the device or NULL -
 *   image n's kernel is the centred ksizes[n] x ksizes[n] part of its table (the rest is not read; anything but an odd size in
 *   1 .. K means K).  `out` must not overlap `x`.
 * drs_bsr_blur_sep: out = g (*) g^T (*) x for ONE 1-D kernel g of k taps (HOST pointer; k odd, 1 <= k <= 51), all planes alike;
 *   same border.  The USM's Gaussian is k = 51, sigma = 0.3 ((k - 1) / 2 - 1) + 0.8 = 8 (cv2.GaussianBlur's rule for sigma 0).
 * drs_bsr_sharpen: unsharp masking, blur = drs_bsr_blur_sep(x):
 *     mask = |x - blur| * 255 > threshold,  soft = drs_bsr_blur_sep(mask),  out = soft clip(x + weight (x - blur), 0, 1) + (1 - soft) x
 *   scratch: N C H W floats (holds blur).  x, out and scratch must not overlap.
 * drs_bsr_resize: (N,C,H,W) -> (N,C,H2,W2), clipped to [0, 1].  Output sample o of an axis sits at (o + 1/2) in / out - 1/2; taps
 *   outside the image take the border pixel.  mode 1: bilinear.  mode 2: bicubic, the 4-tap cubic convolution kernel with a =
 *   -0.75, no antialiasing.  mode 3: area - per axis, where it shrinks, the mean over [o in / out, (o + 1) in / out) with
 *   fractional end pixels, and bilinear where it does not.  These are the project's definitions of cv2.resize's interpolation
 *   flags 1 / 2 / 3; no parity with cv2 is claimed.  in == out is the identity.  out_q (or NULL): a second output,
 *   rint(out * 255) / 255.
 * drs_bsr_noise: in place, per image n with mode[n] = (kind, branch) int32 and par[n] = (sigma, A[3][3]) - 10 floats - on the
 *   device, z (N,C,H,W) the given draws:
 *     noise   branch 0: nv[c] = sigma z[c];  1: nv[c] = sigma z[0];  2 (C == 3, else taken as 0): nv = A (z[0], z[1], z[2])
 *     kind 0  the image is not written;  1  x = clip(x + nv);  2  x = clip(clip(x) + clip(x) nv)   (speckle)
 *     kind 3  x[c] = clip(z[c] / sigma)   (z: Poisson draws at rate q(x) sigma, q(x) = rint(clip(x) 255) / 255)
 *     kind 4  x[c] = clip(q(x[c]) + (z[0] - aux) / sigma)   (aux (N,H,W): the rate gray(q(x)) sigma of the draw z[0]; without
 *             aux the image is not written)
 * drs_bsr_jpeg: C = 3; out = the baseline-JPEG round trip of x at quality[n] (N int32 on the device, clamped to 1 .. 100),
 *   4:2:0, in integer arithmetic throughout: bytes rint(clip(x) 255), libjpeg's 16-bit fixed-point YCbCr,
 *   2 x 2 chroma means with the alternating bias, the edge pixel repeated up to a multiple of 16, Annex K tables under
 *   libjpeg's quality rule, a 14-bit fixed-point 8 x 8 DCT, quantisation to the nearest integer with halves away from zero,
 *   triangle chroma up-sampling, bytes / 255.  One work-group per 16 x 16 MCU writes the decoded planes to `scratch`
 *   (drs_bsr_jpeg_scratch_bytes(N, H, W) bytes); a second launch up-samples across MCU borders and converts.  out may be x. */
DRS_API int drs_bsr_blur(const float* x, float* out, const float* kernels, const int* ksizes, int N, int C, int H, int W, int K,
                         drs_stream_t stream);
DRS_API int drs_bsr_blur_sep(const float* x, float* out, const float* taps, int k, int N, int C, int H, int W, drs_stream_t stream);
DRS_API int drs_bsr_sharpen(const float* x, float* out, float* scratch, const float* taps, int k, float weight, float threshold,
                            int N, int C, int H, int W, drs_stream_t stream);
DRS_API int drs_bsr_resize(const float* x, float* out, float* out_q, int N, int C, int H, int W, int H2, int W2, int mode,
                           drs_stream_t stream);
DRS_API int drs_bsr_noise(float* x, const float* z, const float* aux, const int* mode, const float* par, int N, int C, int H, int W,
                          drs_stream_t stream);
DRS_API size_t drs_bsr_jpeg_scratch_bytes(int N, int H, int W);
DRS_API int drs_bsr_jpeg(const float* x, float* out, const int* quality, int N, int H, int W, void* scratch, size_t scratch_bytes,
                         drs_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Operator-level entry points (used by the parity tests for every convolution flavour
 * the UNet contains, at arbitrary/ragged shapes)
 * ------------------------------------------------------------------------------------------ */

/* y = conv2d(x, w, b) or conv_transpose2d(x, w, b), NCHW in/out like torch.
 *   x: (N,Cin,H,W)   w: (Cout,Cin,KH,KW) [transposed: (Cin,Cout,KH,KW)]   b: (Cout) or NULL
 *   y: (N,Cout,OH,OW) with OH = (H + 2*pad - KH)/stride + 1, transposed: (H-1)*stride - 2*pad + KH + out_pad
 * Supported flavours (all the reference uses): 3x3 s1 p1; 3x3 s2 p1; 1x1; 2x2 s2 p0;
 * transposed 3x3 s2 p1 out_pad 1.  `relu` != 0 applies max(.,0).
 * workspace: device scratch of at least drs_conv2d_workspace_bytes() bytes.
 * Replaces nn.Conv2d / nn.ConvTranspose2d calls at UNet_model_superres.py:70-85,123-141,184-185,217,298,321,325. */
DRS_API size_t drs_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride,
                                  int pad, int transposed, int out_pad);
DRS_API int drs_conv2d_nchw(const float* x, const float* w, const float* b, float* y, int N, int Cin, int H, int W,
                    int Cout, int KH, int KW, int stride, int pad, int transposed, int out_pad, int relu,
                    void* workspace, size_t workspace_bytes, int impl, drs_stream_t stream);

/* One up-sampling stage of the decoder as the eval plan runs it (split-bf16 kernels, activations in the plan's SP format):
 *   y = conv2d(cat([conv_transpose2d(h, t_w, t_b, stride 2, padding 1, output_padding 1), att], 1), v_w, v_b, padding 1)
 * computed WITHOUT the transposed convolution's output: ups.i.transform and the first Cc input channels of up_convs.i are
 * one linear map (no activation between them), composed at pack time into a stride-2 transposed convolution with 3 x 3 /
 * 3 x 2 / 2 x 3 / 2 x 2 taps per output phase (csrc/upfuse_sp.hip).
 *   h: (N,Cc,LH,LW)  att: (N,Ch,2LH,2LW)  t_w: (Cc,Cc,3,3)  t_b: (Cc)  v_w: (Ch,Cc+Ch,3,3)  v_b: (Ch)  y: (N,Ch,2LH,2LW)
 *   post2 / y2 (both or neither): y2 = y + post2[n][c] (the next UpConvBlock's x + relu(time_mlp(t)), reference :199)
 *   fuse_w (fuse_dim,Ch) / fuse_b (fuse_dim): with Ch == 32, y is (N,fuse_dim,2LH,2LW) = conv1x1(y32) (the UNet's `output`)
 * Cc, Ch multiples of 32.  Replaces UpConvBlock.transform + torch.cat + up_convs[i] (+ output),
 * UNet_model_superres.py:206-207,376-377,379. */
DRS_API size_t drs_upconv_fused_workspace_bytes(int N, int Cc, int Ch, int LH, int LW);
DRS_API int drs_upconv_fused_nchw(const float* h, const float* att, const float* t_w, const float* t_b, const float* v_w,
                          const float* v_b, const float* post2, const float* fuse_w, const float* fuse_b, int fuse_dim,
                          float* y, float* y2, int N, int Cc, int Ch, int LH, int LW, void* workspace, size_t workspace_bytes,
                          drs_stream_t stream);

/* y = F.interpolate(x, scale_factor=scale, mode='bicubic') (align_corners=False, A=-0.75, border clamp),
 * integer scale.  x: (N,C,H,W) -> y: (N,C,H*scale,W*scale).  Replaces UNet_model_superres.py:349. */
DRS_API int drs_bicubic_upsample_nchw(const float* x, float* y, int N, int C, int H, int W, int scale,
                              drs_stream_t stream);

/* out[b, :] = relu(W2 @ silu(W1 @ posenc(t[b]) + b1) + b2), posenc = [sin(t*f_j) | cos(t*f_j)], j < dim_in/2,
 * inv_freq[j] = f_j supplied by the caller (dim_in/2 floats).  W1: (dim_out, dim_in), W2: (dim_out, dim_out).
 * Replaces pos_encoding + time_mlp + ReLU, UNet_model_superres.py:328-335,143-151,161 (and :187-199). */
DRS_API int drs_time_mlp(const int64_t* t, const float* inv_freq, const float* W1, const float* b1, const float* W2,
                 const float* b2, float* out, int B, int dim_in, int dim_out, drs_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Whole-network plan: Residual_Attention_UNet_superres.forward (UNet_model_superres.py:337-379)
 * in eval mode (BatchNorm running statistics folded into the convolutions at pack time).
 * ------------------------------------------------------------------------------------------ */

typedef struct drs_unet_config {
  int batch;          /* n images in x */
  int lr_batch;       /* batch of lr_img: == batch, or 1 (broadcast, Diffusion.sample :224) */
  int image_channels; /* reference ctor arg (3); 1..16 bands */
  int out_dim;        /* reference ctor arg (3); 1..16 (above 4 the output projection is not folded into up_convs.2) */
  int height, width;  /* of x; divisible by 8 and by magnification */
  int magnification;  /* lr_img is (height/mag, width/mag) */
  int impl;           /* DRS_IMPL_* used for the wide convolutions */
  float bn_eps;       /* 1e-5 */
  int flags;          /* DRS_PLAN_* */
  int variant;        /* DRS_VARIANT_* : which of the reference's three near-identical UNets */
  int cond_channels;  /* channels of the conditioning image, 1..16 (superres: = image_channels; SAR: 2; generation: 0) */
  int num_classes;    /* generation: rows of label_emb (0 = no label embedding) */
} drs_unet_config;
/* Variants (same kernels, different wiring and state_dict key names):
 *  SUPERRES    Residual_Attention_UNet_superres   UNet_model_superres.py:266-379   cond = lr_img, bicubic x mag
 *  SAR_TO_NDVI Residual_Attention_UNet_SAR_TO_NDVI UNet_model_SAR_TO_NDVI.py:263-370 cond = SAR image at full size
 *              (magnification must be 1), image_channels = out_dim = NDVI channels
 *  GENERATION  Residual_Attention_UNet_generation generate_new_imgs/UNet_model_generation.py:226-329  no conditioning
 *              image; optional class label added to the time encoding (t += label_emb(y), :300-301) */
#define DRS_VARIANT_SUPERRES 0
#define DRS_VARIANT_SAR_TO_NDVI 1
#define DRS_VARIANT_GENERATION 2
/* Keep every intermediate activation readable through drs_unet_read_tensor (parity tests).  Without it the
 * 32-channel output of up_convs.2 is never written: the final 1x1 `output` conv is fused into its epilogue. */
#define DRS_PLAN_KEEP_ALL 1
/* Train-mode plan: BatchNorm uses batch statistics (and updates running_mean / running_var in place through the
 * parameter pointers given to drs_unet_pack_weights), nothing is folded or fused across a BatchNorm, every
 * pre-normalisation tensor is kept.  Reference: model.train() + nn.BatchNorm2d defaults (eps 1e-5, momentum 0.1). */
#define DRS_PLAN_TRAIN 2
/* Frozen BatchNorm statistics, for fine-tuning a snapshot on small batches; valid only together with DRS_PLAN_TRAIN
 * (plan creation returns DRS_ERR_ARG otherwise).  Reference: model.train() with every nn.BatchNorm2d in .eval():
 * y = (z - running_mean) / sqrt(running_var + eps) * gamma + beta.  The running statistics are read through the
 * parameter pointers on every forward and never written.  Everything else is the train plan: nothing folded, every
 * pre-normalisation tensor kept, the same workspace layout and the same backward contract (its BatchNorm step is
 * dz = gamma * rstd * g, with dgamma / dbeta as before; a conv bias in front of a BatchNorm now has a real gradient). */
#define DRS_PLAN_FROZEN_BN 4

DRS_API int drs_unet_plan_create(drs_plan** plan, const drs_unet_config* cfg);
DRS_API void drs_unet_plan_destroy(drs_plan* plan);

/* The state_dict entries the plan consumes, in the order drs_unet_pack_weights expects. */
DRS_API int drs_unet_num_params(const drs_plan* plan);
DRS_API const char* drs_unet_param_name(const drs_plan* plan, int i);
DRS_API int64_t drs_unet_param_numel(const drs_plan* plan, int i);

DRS_API size_t drs_unet_packed_bytes(const drs_plan* plan);
DRS_API size_t drs_unet_workspace_bytes(const drs_plan* plan);

/* Fold BatchNorm (eval) into conv weights/biases and re-lay every weight for the kernels.
 * params[i] = device pointer of state_dict[drs_unet_param_name(i)] (fp32).  inv_freq = 50 floats (host
 * pointer) computed like reference :329-331.  Must be re-run whenever the parameters change. */
DRS_API int drs_unet_pack_weights(drs_plan* plan, const void* const* params, const float* inv_freq_host, void* packed,
                          size_t packed_bytes, drs_stream_t stream);

/* eps_pred = model(x, t, lr_img, magnification).  x: (batch,C,H,W)  t: (batch) int64
 * lr_img: (lr_batch,C,H/mag,W/mag)  out: (batch,out_dim,H,W).
 * flags bit 0 (DRS_FWD_REUSE_COND): skip the LR-conditioning branch (RRDB -> bicubic -> conv, reference
 * :345-353) and reuse the one left in the workspace by the previous call — valid while lr_img and the weights
 * are unchanged, i.e. inside one Diffusion.sample chain (the reference recomputes it every step). */
#define DRS_FWD_REUSE_COND 1
DRS_API int drs_unet_forward(drs_plan* plan, const void* packed, const float* x, const int64_t* t, const float* lr_img,
                     float* out, void* workspace, size_t workspace_bytes, int flags, drs_stream_t stream);
/* Same, with class labels for the GENERATION variant: labels = int64[label_batch] (label_batch == batch or 1,
 * broadcast) or NULL for the unconditional forward (reference forward(x, timestep, y=None)). */
DRS_API int drs_unet_forward_labels(drs_plan* plan, const void* packed, const float* x, const int64_t* t, const float* cond,
                            const int64_t* labels, int label_batch, float* out, void* workspace,
                            size_t workspace_bytes, int flags, drs_stream_t stream);

/* Introspection for block-level parity tests: intermediate activations left in the workspace by the last
 * forward, converted to NCHW into `dst`.  Names follow the reference module tree
 * ("conv_blocks.0", "downs.1", "attention_blocks.2", ...). */
DRS_API int drs_unet_num_tensors(const drs_plan* plan);
DRS_API const char* drs_unet_tensor_name(const drs_plan* plan, int i);
DRS_API int drs_unet_tensor_shape(const drs_plan* plan, int i, int* n, int* c, int* h, int* w);
DRS_API int drs_unet_read_tensor(const drs_plan* plan, int i, const void* workspace, float* dst_nchw, drs_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Training step, backward half (reference loop body train_diffusion_superres.py:388-393: loss.backward()).
 * Given d(loss)/d(eps_pred) (`dout`, NCHW like the output) it produces d(loss)/d(parameter) for every parameter of
 * drs_unet_param_name(): grads[i] = device pointer of drs_unet_param_numel(i) floats, or NULL to skip (BatchNorm
 * running statistics, which receive no gradient, must be NULL).  Gradients are OVERWRITTEN (zeroed first).
 * Requires a DRS_PLAN_TRAIN plan with lr_batch == batch and the workspace exactly as the last drs_unet_forward
 * (train mode) on this plan left it; `packed_bwd` is scratch for the re-packed (transposed) weights.  The call consumes
 * that workspace (BatchNorm turns Z into dZ in place): one backward per forward.  Any subset of the slots may be NULL,
 * down to a single wanted gradient; a NULL slot is neither written nor zeroed and costs no other gradient anything.
 * ------------------------------------------------------------------------------------------ */
DRS_API size_t drs_unet_packed_bwd_bytes(const drs_plan* plan);
DRS_API int drs_unet_backward(drs_plan* plan, const void* packed, void* packed_bwd, size_t packed_bwd_bytes, const float* x,
                      const int64_t* t, const float* dout, float* const* grads, void* workspace, size_t workspace_bytes,
                      drs_stream_t stream);
/* Same for a forward that was given class labels (GENERATION variant): also produces d(label_emb.weight). */
DRS_API int drs_unet_backward_labels(drs_plan* plan, const void* packed, void* packed_bwd, size_t packed_bwd_bytes,
                             const float* x, const int64_t* t, const int64_t* labels, int label_batch,
                             const float* dout, float* const* grads, void* workspace, size_t workspace_bytes,
                             drs_stream_t stream);

/* Per-op timing of the forward schedule: with profiling on, drs_unet_forward brackets every op with HIP events on
 * the stream it launches on; afterwards read (name, milliseconds, algorithmic FLOPs, algorithmic bytes) per op.
 * Used by bench.py for the roofline of the dominant kernel.  Not for use inside graph capture. */
/* Synchronises `stream` and returns DRS_ERR_HIP if a wave of the wave-specialised kernels gave up waiting on an LDS
 * counter since the weights were last packed into `packed` (a protocol bug; such a wave records it and ends instead of
 * hanging or faulting the device: csrc/sp_sync.h).  Debug / test aid; a healthy run never sets it. */
DRS_API int drs_unet_check_faults(drs_plan* plan, const void* packed, drs_stream_t stream);

DRS_API int drs_unet_profile_enable(drs_plan* plan, int on);
DRS_API int drs_unet_profile_num_ops(const drs_plan* plan);
DRS_API int drs_unet_profile_read(drs_plan* plan, int i, char* name, int name_len, float* ms, double* flops, double* bytes);
/* Launch log of the last PROFILED forward (ABI 6): one entry per kernel the forward launched, in host launch order, with
 * the kernel's name as the runtime reports it (demangled) and the op of the schedule that issued it ("" for launches
 * outside any op bracket, e.g. the per-image gate-bias tables).  A rocprofv3 counter pass over the same process sees
 * exactly these dispatches, in this order, as the process's last launches: tools/collect_pmc.py joins the two and
 * refuses to attribute bytes if a kernel name differs. */
DRS_API int drs_unet_profile_num_launches(const drs_plan* plan);
DRS_API int drs_unet_profile_launch(const drs_plan* plan, int i, char* op, int op_len, char* kernel, int kernel_len);

/* ---- VGG19 perceptual loss (the MSE+Perceptual_noise training loss; csrc/vgg_loss.hip) ----------------------------------
 * Replaces VGGPerceptualLoss.forward (reference train_diffusion_superres.py:63-68, train_diffusion_SAR_TO_NDVI.py:64-69,
 * generate_new_imgs/train_diffusion_generation.py:66-71) and its autograd backward w.r.t. the prediction:
 *   loss = mean((F(P(pred)) - F(P(target)))^2),  P = bicubic resize to 224 x 224 when width != 224 (:46-50) + ImageNet
 *   normalise (:42-44),  F = torchvision vgg19().features (:28).
 * pred / target: (batch, 3, height, width) NCHW fp32.  Prediction and target run as one batched forward of 2 x batch images.
 * Every convolution runs on the MFMA kernels (impl DRS_IMPL_MFMA_F32 or DRS_IMPL_MFMA_BF16X3); a shape any layer of which
 * they do not take fails plan creation with DRS_ERR_SHAPE. */
typedef struct drs_vgg_plan drs_vgg_plan;
DRS_API int drs_vgg_plan_create(drs_vgg_plan** plan, int batch, int height, int width, int impl);
DRS_API void drs_vgg_plan_destroy(drs_vgg_plan* plan);
DRS_API size_t drs_vgg_packed_bytes(const drs_vgg_plan* plan);
DRS_API size_t drs_vgg_workspace_bytes(const drs_vgg_plan* plan);
/* params[2 l], params[2 l + 1] = device pointers of features.{k}.weight / .bias of the l-th convolution (k = 0, 2, 5, 7, 10, 12,
 * 14, 16, 19, 21, 23, 25, 28, 30, 32, 34: torchvision's key layout), fp32.  Packs forward and data-gradient images once. */
DRS_API int drs_vgg_pack_weights(drs_vgg_plan* plan, const void* const* params, void* packed, size_t packed_bytes,
                         drs_stream_t stream);
/* *loss (device scalar) = the loss.  save = 1 keeps the prediction half's activations in the workspace for drs_vgg_backward;
 * save = 0 (validation under torch.no_grad) keeps nothing.  No host synchronisation. */
DRS_API int drs_vgg_forward(drs_vgg_plan* plan, const void* packed, const float* pred, const float* target, float* loss,
                    int save, void* workspace, size_t workspace_bytes, drs_stream_t stream);
/* dpred = d(loss)/d(pred) * (*grad_loss) (device scalar: autograd's upstream gradient); needs the workspace as the last
 * drs_vgg_forward with save = 1 left it.  Deterministic: no atomics. */
DRS_API int drs_vgg_backward(drs_vgg_plan* plan, const void* packed, const float* grad_loss, float* dpred, void* workspace,
                     size_t workspace_bytes, drs_stream_t stream);
/* Per-op timing of the last forward / backward (HIP events on its stream): name, milliseconds, algorithmic FLOPs. */
DRS_API int drs_vgg_profile_enable(drs_vgg_plan* plan, int on);
DRS_API int drs_vgg_profile_num_ops(const drs_vgg_plan* plan);
DRS_API int drs_vgg_profile_read(drs_vgg_plan* plan, int i, char* name, int name_len, float* ms, double* flops);
/* Read-out of the tensors a forward leaves in the workspace (ABI 8; the per-layer parity tests), as drs_unet_*_tensor:
 *   "x0"                   (2 batch, 4, H0, W0)  the prep output, channel 3 = the zero pad channel
 *   "conv1" .. "conv16"    (batch, C, h, w)      the saved prediction-half ReLU outputs, i.e. what drs_vgg_backward reads;
 *                                                valid only after a forward with save = 1, else DRS_ERR_STATE
 *   "features"             (2 batch, 512, h5, w5)
 * drs_vgg_read_tensor copies tensor i out of `workspace` (NHWC) into dst_nchw (device, n * c * h * w floats). */
DRS_API int drs_vgg_num_tensors(const drs_vgg_plan* plan);
DRS_API const char* drs_vgg_tensor_name(const drs_vgg_plan* plan, int i);
DRS_API int drs_vgg_tensor_shape(const drs_vgg_plan* plan, int i, int* n, int* c, int* h, int* w);
DRS_API int drs_vgg_read_tensor(const drs_vgg_plan* plan, int i, const void* workspace, float* dst_nchw, drs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRS_HIP_H */
