// Zero-terminal-SNR sampling (Lin et al., "Common Diffusion Noise Schedules and Sample Steps Are Flawed",
// WACV 2024).  Two entry points, both HBM-bound streaming passes with plain vector loads and stores:
//   drs_terminal_step  the reverse move away from the one level whose alpha_hat is 0.  There x_t is the noise itself, a v network's
//                      x0 is -v and an x0 network's is its output, and the move to t_prev is a closed form in (x0, x_t, z) that
//                      divides by nothing - every other move of a chain stays with reverse_step.hip.  Row layout and grid:
//                      row_span.h (as prediction.hip); no LDS, no atomics.
//   drs_cfg_rescale    the guidance rescale of the same paper (section 3.4): the guided prediction scaled per image towards the
//                      standard deviation of the conditional one.  Two launches on one stream: fp64 partial sums per 4096-element
//                      chunk in a fixed order (the scheme of drs_grad_sumsq_partials, optim.hip), then every block adds its
//                      image's partials in index order and scales its chunk.  No atomics, no host synchronisation.
// Per-element arithmetic of the move: step_update.h (guidance, clamp, threshold, known pixels), products and sums rounded one by
// one.
#include "drs_common.h"
#include "row_span.h"
#include "step_update.h"

namespace {

struct TermArgs {
  float* x;
  const float* pred;
  const float* pu;     // the unconditional prediction, or null: no guidance
  float w;
  const float* noise;  // or null (checked on the host)
  const float* known;  // with `mask`, or both null
  const unsigned char* mask;
  const float* scale;  // n dynamic-threshold scales, or null: the static clamp (if `clip`)
  float* hist;         // or null
  const float* alpha_hat;
  int n, Cm, C, kind, clip, phase, t, t_prev, noise_steps;
  float lo, hi, eta;
  int64_t chw, hw;
  bool vec;
};

// c0 = sqrt(ah_p), c1 = sqrt(max(0, (1 - ah_p)(1 - eta^2))), sigma = eta sqrt(1 - ah_p) (0 at t_prev == 0): fp64 from the fp32
// table entry, rounded once (as drs_ddim_coef).  `bad`: a level outside the table or one whose alpha_hat is not 0.
struct TermCoef {
  float c0, c1, sigma;
  bool bad;
  __device__ TermCoef(const TermArgs& p) {
    bad = p.t < 0 || p.t >= p.noise_steps || p.t_prev < 0 || p.t_prev >= p.t;  // never indexes the table
    c0 = c1 = sigma = 0.f;
    if (bad) return;
    if (p.alpha_hat[p.t] != 0.f) {
      bad = true;
      return;
    }
    const double ap = (double)p.alpha_hat[p.t_prev], eta = (double)p.eta;
    const double q = fmax(1.0 - ap, 0.0);
    c0 = (float)sqrt(ap);
    c1 = (float)sqrt(fmax(q * (1.0 - eta * eta), 0.0));
    sigma = p.t_prev == 0 ? 0.f : (float)(eta * sqrt(q));
  }
};

// An image that is thresholded (scale > r, finite): drs_pred_to_eps_dyn's definition - c and r rounded to fp32 once, x0 clamped to
// c +- s, rescaled by r / s, clamped to [lo, hi] - evaluated in fp64 from the fp32 inputs, guidance included, and rounded to fp32
// once.  That entry's own fp32 steps round around c and s (d = fl(x0 - c), fl(d rho), fl(c + m)), which next to the lower edge of
// a (0, 1) range is many ulps of the result; here the x0 that goes into the move and the history is within one rounding of the
// definition, and an element clamped to c +- s lands on lo / hi exactly ((+-s / s) r = +-r).
__device__ __forceinline__ float term_x0_dyn(const TermArgs& p, const DrsDynScale& y, float q, float u) {
  double g = (double)q;
  if (p.pu) {  // torch.lerp's two forms, in fp64
    const double w = (double)p.w, d = g - (double)u;
    g = fabs(w) < 0.5 ? (double)u + w * d : g - d * (1.0 - w);
  }
  const double x0 = p.kind == DRS_PRED_V ? -g : g;
  if (!(fabs(x0) < (double)__builtin_huge_valf())) return (float)x0;  // a NaN or an infinity stays what it is
  const double c = (double)y.c, s = (double)y.s, r = (double)(float)(((double)p.hi - (double)p.lo) / 2.0);
  const double d = x0 - c, e = d < -s ? -s : (d > s ? s : d);
  const double v = c + (e / s) * r;
  return (float)(v < (double)p.lo ? (double)p.lo : (v > (double)p.hi ? (double)p.hi : v));
}

// the x0 of one element: guidance, sign, then the static clamp of drs_pred_eps (also where the image's scale does not exceed
// the half-range: the bits of the static clip), or the threshold above
__device__ __forceinline__ float term_x0(const TermArgs& p, const DrsPredCoef& k, const DrsDynScale& y, bool dyn, float q, float u) {
  if (dyn && y.dynamic) return term_x0_dyn(p, y, q, u);
  if (p.pu) q = drs_cfg_lerp(u, q, p.w);
  float x0 = p.kind == DRS_PRED_V ? -q : q;
  if (dyn) return drs_dyn_q(k, y, x0);
  if (p.clip && fabsf(x0) < __builtin_huge_valf()) x0 = x0 < p.lo ? p.lo : (x0 > p.hi ? p.hi : x0);
  return x0;
}
// x' = fl(fl(c0 x0) + fl(c1 x)) + fl(sigma z), the last term only when the move draws
__device__ __forceinline__ float term_move(const TermCoef& c, bool add_noise, float x0, float x, float z) {
#pragma clang fp contract(off)
  const float a = c.c0 * x0, b = c.c1 * x;
  float v = a + b;
  if (add_noise) {
    const float s = c.sigma * z;
    v = v + s;
  }
  return v;
}

// blockIdx.y strides over the images, blockIdx.x over one image's groups of four (then over its head and tail elements)
__global__ __launch_bounds__(256) void terminal_step_kernel(const TermArgs p) {
  const TermCoef c(p);
  const float nan = __builtin_nanf("");
  const bool add_noise = p.noise != nullptr && c.sigma != 0.f;
  const bool to_zero = p.t_prev == 0;  // the known pixels arrive at the known image itself; z is not read for them
  const bool dyn = p.scale != nullptr;
  DrsPredCoef k;
  k.form = DrsPredCoef::CLIP_PRED;
  k.xa = k.xb = k.ea = k.eb = 0.f;
  k.lo = p.lo;
  k.hi = p.hi;
  const DrsKnownCoef kc(p.alpha_hat, c.bad ? 0 : p.t_prev);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    const DrsDynScale y(p.lo, p.hi, dyn ? p.scale[img] : 0.f);
    const int64_t row = (int64_t)img * p.chw;
    float* xp = p.x + row;
    const float* pp = p.pred + row;
    const float* up = p.pu ? p.pu + row : nullptr;
    const float* zp = p.noise ? p.noise + row : nullptr;
    const float* kp = p.known ? p.known + row : nullptr;
    float* hp = p.hist ? p.hist + row : nullptr;
    // the mask entry of element i of this image: i itself with a mask of C bands, i % hw with a single-band one
    const unsigned char* mp = p.mask ? p.mask + (p.Cm == 1 ? (int64_t)img * p.hw : row) : nullptr;
    const bool wrap = p.Cm == 1 && p.C > 1;
    auto one = [&](int64_t mi, float x, float q, float u, float z, float kn, float& h) -> float {
      if (c.bad) {
        h = nan;
        return nan;
      }
      const float x0 = term_x0(p, k, y, dyn, q, u);
      h = x0;
      float v = term_move(c, add_noise, x0, x, z);
      if (mp && mp[mi]) v = to_zero ? kn : kc.at(kn, z);
      return v;
    };
    const RowSpan s(p.vec, p.phase, row, p.chw);
    for (int64_t g = tid; g < s.groups; g += stride) {
      const int64_t at = s.head + 4 * g;
      const float4 x4 = *reinterpret_cast<const float4*>(xp + at);
      const float4 p4 = *reinterpret_cast<const float4*>(pp + at);
      float4 u4 = {0.f, 0.f, 0.f, 0.f}, z4 = u4, k4 = u4, h4, o;
      if (up) u4 = *reinterpret_cast<const float4*>(up + at);
      if (zp) z4 = *reinterpret_cast<const float4*>(zp + at);
      if (kp) k4 = *reinterpret_cast<const float4*>(kp + at);
      int64_t m[4] = {at, at + 1, at + 2, at + 3};
      if (wrap) {  // one division per group: a group may straddle two bands
        m[0] = at % p.hw;
        for (int j = 1; j < 4; ++j) m[j] = m[j - 1] + 1 == p.hw ? 0 : m[j - 1] + 1;
      }
      o.x = one(m[0], x4.x, p4.x, u4.x, z4.x, k4.x, h4.x);
      o.y = one(m[1], x4.y, p4.y, u4.y, z4.y, k4.y, h4.y);
      o.z = one(m[2], x4.z, p4.z, u4.z, z4.z, k4.z, h4.z);
      o.w = one(m[3], x4.w, p4.w, u4.w, z4.w, k4.w, h4.w);
      *reinterpret_cast<float4*>(xp + at) = o;
      if (hp) *reinterpret_cast<float4*>(hp + at) = h4;
    }
    const int64_t rest = p.chw - 4 * s.groups;  // head and tail elements: at most 6 with `vec`
    for (int64_t r = tid; r < rest; r += stride) {
      const int64_t i = r < s.head ? r : s.tail() + (r - s.head);
      float h;
      const float o = one(wrap ? i % p.hw : i, xp[i], pp[i], up ? up[i] : 0.f, zp ? zp[i] : 0.f, kp ? kp[i] : 0.f, h);
      xp[i] = o;
      if (hp) hp[i] = h;
    }
  }
}

// ---- guidance rescale --------------------------------------------------------------------------------------------------------
constexpr int kChunk = 4096;  // elements per block of both launches
constexpr int kPerThread = kChunk / 256;
constexpr int kSums = 4;      // per chunk: sum and sum of squares of cond - cond[0] and of g - g[0]

struct RescaleArgs {
  const float* cond;
  const float* uncond;
  float w, phi;
  float* out;
  double* partials;  // n x chunks x kSums
  int n, chunks;
  int64_t chw;
};

// Sums are taken of the differences to the image's first element: a constant image then sums to exactly 0 (its standard
// deviation is 0, not rounding noise), and sum of squares minus squared sum loses nothing to a large mean.
__global__ __launch_bounds__(256) void cfg_rescale_partials_kernel(const RescaleArgs p) {
  const int img = blockIdx.y;
  const int64_t row = (int64_t)img * p.chw, lo = (int64_t)blockIdx.x * kChunk;
  const int64_t hi = lo + kChunk < p.chw ? lo + kChunk : p.chw;
  const float* cp = p.cond + row;
  const float* up = p.uncond + row;
  const double c0 = (double)cp[0], g0 = (double)drs_cfg_lerp(up[0], cp[0], p.w);
  float cs[kPerThread], gs[kPerThread];
  bool in[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = lo + threadIdx.x + 256 * k;
    in[k] = i < hi;
    cs[k] = in[k] ? cp[i] : 0.f;
    gs[k] = in[k] ? drs_cfg_lerp(up[i], cs[k], p.w) : 0.f;
  }
  double s[kSums] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const double dc = in[k] ? (double)cs[k] - c0 : 0.0, dg = in[k] ? (double)gs[k] - g0 : 0.0;
    s[0] = __dadd_rn(s[0], dc);
    s[1] = __dadd_rn(s[1], __dmul_rn(dc, dc));
    s[2] = __dadd_rn(s[2], dg);
    s[3] = __dadd_rn(s[3], __dmul_rn(dg, dg));
  }
  __shared__ double wave_sum[4][kSums];
#pragma unroll
  for (int j = 0; j < kSums; ++j) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s[j] = __dadd_rn(s[j], __shfl_down(s[j], off, 64));
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6][j] = s[j];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const int j = threadIdx.x;
    p.partials[((int64_t)img * p.chunks + blockIdx.x) * kSums + j] =
        __dadd_rn(__dadd_rn(__dadd_rn(wave_sum[0][j], wave_sum[1][j]), wave_sum[2][j]), wave_sum[3][j]);
  }
}

// Every block adds its image's partials in index order (all blocks of an image hold the same bits), forms
// f = 1 + phi (sqrt(var(cond) / var(g)) - 1) in fp64 - the 1 / chw of both variances cancels -, rounds it once and writes
// out = fl(g f) over its chunk.  var(g) == 0 or a ratio that is not finite: f = 1.
__global__ __launch_bounds__(256) void cfg_rescale_apply_kernel(const RescaleArgs p) {
  const int img = blockIdx.y;
  __shared__ double total[kSums];
  if (threadIdx.x < kSums) {
    const double* q = p.partials + (int64_t)img * p.chunks * kSums + threadIdx.x;
    double S = 0.0;
    for (int j = 0; j < p.chunks; ++j) S = __dadd_rn(S, q[(int64_t)j * kSums]);
    total[threadIdx.x] = S;
  }
  __syncthreads();
  const double N = (double)p.chw;
  const double var_c = total[1] - total[0] * total[0] / N, var_g = total[3] - total[2] * total[2] / N;
  double f = 1.0;
  if (var_g > 0.0 && var_c >= 0.0) {
    const double ratio = sqrt(var_c / var_g);
    if (isfinite(ratio)) f = 1.0 + (double)p.phi * (ratio - 1.0);
  }
  const float ff = (float)f;
  const int64_t row = (int64_t)img * p.chw, lo = (int64_t)blockIdx.x * kChunk;
  const int64_t hi = lo + kChunk < p.chw ? lo + kChunk : p.chw;
  const float* cp = p.cond + row;
  const float* up = p.uncond + row;
  float* op = p.out + row;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) op[i] = __fmul_rn(drs_cfg_lerp(up[i], cp[i], p.w), ff);
}

}  // namespace

extern "C" int drs_terminal_step(float* x, const float* pred, const float* pred_uncond, float cfg_scale, const float* noise,
                                 const float* known, const uint8_t* mask, int mask_channels, int kind, int clip, float lo,
                                 float hi, const float* scale, float* x0_hist, int n, int C, int H, int W, int t, int t_prev,
                                 float eta, const float* alpha_hat, int noise_steps, drs_stream_t stream) {
  DRS_REQUIRE(x && pred && alpha_hat, DRS_ERR_ARG, "terminal_step: null pointer");
  DRS_REQUIRE(kind == DRS_PRED_V || kind == DRS_PRED_X0, DRS_ERR_ARG,
              "terminal_step: kind=%d is neither DRS_PRED_V nor DRS_PRED_X0 (at alpha_hat == 0 an eps prediction is the state itself: "
              "it names no x0)", kind);
  DRS_REQUIRE((known == nullptr) == (mask == nullptr), DRS_ERR_ARG, "terminal_step: known and mask go together");
  DRS_REQUIRE(n >= 0 && C >= 1 && H >= 0 && W >= 0 && noise_steps > 0, DRS_ERR_SHAPE,
              "terminal_step: n=%d C=%d H=%d W=%d noise_steps=%d", n, C, H, W, noise_steps);
  DRS_REQUIRE(!mask || mask_channels == 1 || mask_channels == C, DRS_ERR_SHAPE,
              "terminal_step: a mask of %d bands for an image of %d (1 or %d)", mask_channels, C, C);
  DRS_REQUIRE(!clip || lo < hi, DRS_ERR_ARG, "terminal_step: clip needs lo < hi, got lo=%g hi=%g", (double)lo, (double)hi);
  DRS_REQUIRE(!scale || clip, DRS_ERR_ARG, "terminal_step: the threshold scales need the clip range they compress into");
  DRS_REQUIRE(!pred_uncond || std::isfinite(cfg_scale), DRS_ERR_ARG, "terminal_step: cfg_scale=%g must be finite",
              (double)cfg_scale);
  DRS_REQUIRE(std::isfinite(eta) && eta >= 0.f && eta <= 1.f, DRS_ERR_ARG, "terminal_step: eta=%g must lie in [0, 1]",
              (double)eta);
  DRS_REQUIRE(noise || !(t_prev > 0 && (eta > 0.f || known)), DRS_ERR_ARG,
              "terminal_step: t_prev=%d > 0 with eta=%g%s needs a noise tensor", t_prev, (double)eta,
              known ? " and known pixels" : "");
  DRS_REQUIRE(!x0_hist || x0_hist != x, DRS_ERR_ARG, "terminal_step: x0_hist and x are one buffer");
  if (n == 0 || H == 0 || W == 0) return DRS_OK;
  TermArgs a;
  a.x = x; a.pred = pred; a.pu = pred_uncond; a.w = cfg_scale; a.noise = noise; a.known = known; a.mask = mask;
  a.scale = scale; a.hist = x0_hist; a.alpha_hat = alpha_hat;
  a.n = n; a.Cm = mask ? mask_channels : C; a.C = C; a.kind = kind; a.clip = clip; a.t = t; a.t_prev = t_prev;
  a.noise_steps = noise_steps; a.lo = lo; a.hi = hi; a.eta = eta;
  a.hw = (int64_t)H * W;
  a.chw = a.hw * C;
  a.vec = same_phase({x, pred, pred_uncond, noise, known, x0_hist});
  a.phase = phase_of(x);
  DRS_LAUNCH(terminal_step_kernel, stream_grid(n, a.chw, a.vec), dim3(256), 0, (hipStream_t)stream, a);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

extern "C" size_t drs_cfg_rescale_workspace_bytes(int n, int64_t chw) {
  if (n <= 0 || chw <= 0) return 0;
  return (size_t)n * (size_t)((chw + kChunk - 1) / kChunk) * kSums * sizeof(double);
}

extern "C" int drs_cfg_rescale(const float* cond, const float* uncond, float cfg_scale, float phi, float* out, int n, int64_t chw,
                               void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  DRS_REQUIRE(cond && uncond && out, DRS_ERR_ARG, "cfg_rescale: null pointer");
  DRS_REQUIRE(std::isfinite(cfg_scale), DRS_ERR_ARG, "cfg_rescale: cfg_scale=%g must be finite", (double)cfg_scale);
  DRS_REQUIRE(phi >= 0.f && phi <= 1.f, DRS_ERR_ARG, "cfg_rescale: phi=%g must lie in [0, 1]", (double)phi);
  DRS_REQUIRE(n >= 0 && chw >= 0, DRS_ERR_SHAPE, "cfg_rescale: n=%d chw=%lld", n, (long long)chw);
  if (n == 0 || chw == 0) return DRS_OK;
  const int64_t chunks = (chw + kChunk - 1) / kChunk;
  DRS_REQUIRE(n <= 65535 && chunks <= INT32_MAX, DRS_ERR_SHAPE, "cfg_rescale: n=%d images of %lld chunks", n, (long long)chunks);
  const size_t need = drs_cfg_rescale_workspace_bytes(n, chw);
  DRS_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7u) == 0, DRS_ERR_ARG,
              "cfg_rescale: workspace of %zu bytes, needs %zu (8-byte aligned)", workspace_bytes, need);
  RescaleArgs a;
  a.cond = cond; a.uncond = uncond; a.w = cfg_scale; a.phi = phi; a.out = out;
  a.partials = static_cast<double*>(workspace);
  a.n = n; a.chunks = (int)chunks; a.chw = chw;
  const dim3 grid((unsigned)chunks, (unsigned)n);
  DRS_LAUNCH(cfg_rescale_partials_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  DRS_LAUNCH(cfg_rescale_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
