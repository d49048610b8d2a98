// Dynamic thresholding of the implied x0 (Saharia et al., "Imagen", 2022, section 2.3): per image, an
// exact order statistic s of |x0 - c| and, where s exceeds the half-range r, x0 clamped to c +- s and rescaled by r / s instead
// of the static clamp of drs_pred_to_eps.  The statistic is a radix select over the 31 bits of key = bits(|x0 - c|), digits of
// 11 + 10 + 10 bits from the top, one streaming pass per digit:
//   pass 1      reads pred (pred_uncond) and x, writes x0 into `out`, counts the top digit
//   pass 2, 3   read `out`, count the next digit among the elements whose higher digits are the prefix found so far
//   apply       reads `out` and x, writes eps
// Between the passes a one-block-per-image launch turns the histogram just counted into (prefix, remaining rank) of the image's
// state: the passes depend on each other through launch boundaries of the one stream only.  Counts are integers (LDS atomics
// per block, then one global atomic per non-empty bin), so s and the output do not depend on arrival order.  Per-element
// arithmetic: step_update.h; row layout and grid: row_span.h.
#include "drs_common.h"
#include "row_span.h"
#include "step_update.h"

namespace {

constexpr int kBins1 = 2048, kBins2 = 1024;         // 11 | 10 | 10 bits
constexpr int kHistWords = kBins1 + 2 * kBins2;     // per image: the three histograms
constexpr int kStateWords = 4;                      // per image: prefix, remaining rank (padded to 16 bytes)

struct ThrArgs {
  const float* pred;  // may be `out`
  const float* pu;    // the unconditional prediction, or null: no guidance
  float w;
  const float* x;
  const int64_t* t;
  const float* alpha_hat;
  float* out;
  float* scale_out;  // n scales, or null
  unsigned* hist;    // n x kHistWords
  unsigned* state;   // n x kStateWords
  int n, noise_steps, phase, kind;
  float lo, hi, c;
  int64_t chw, k;
  bool vec;
};

__device__ __forceinline__ DrsPredCoef coef_of(const ThrArgs& p, int img) {
  const int64_t tn = p.t[img];
  const bool bad = tn < 0 || tn >= p.noise_steps;  // never indexes the table
  return drs_pred_coef(bad ? 0.f : p.alpha_hat[tn], p.kind, true, p.lo, p.hi, bad);
}
// an image whose x0 is formed and ranked; the others get drs_pred_eps in pass 1 and are left alone afterwards
__device__ __forceinline__ bool ranked(const DrsPredCoef& k) {
  return k.form == DrsPredCoef::CLIP_LINEAR || k.form == DrsPredCoef::CLIP_PRED;
}

// the block's counts of one image into the image's histogram: one atomic per non-empty bin
template <int BINS>
__device__ __forceinline__ void flush_hist(const unsigned* lds, unsigned* ghist) {
  for (int b = threadIdx.x; b < BINS; b += blockDim.x)
    if (lds[b]) atomicAdd(ghist + b, lds[b]);
}

__device__ __forceinline__ float thr_x0(const ThrArgs& p, const DrsPredCoef& k, float x, float q, float u, bool guided) {
  if (guided) q = drs_cfg_lerp(u, q, p.w);
  return ranked(k) ? drs_pred_x0(k, x, q) : drs_pred_eps(k, x, q);
}

// Real x0 values sit in a few exponents, so the top digit of a block's elements lands in a few dozen bins and lanes of one wave
// hit the same LDS address.  Measured: 1, 4 and 8 histograms per block (picked by lane) cost 53 / 57 /
// 67 us on such an input at 16 x 3 x 256 x 256 - zeroing and flushing the copies costs more than the collisions they spare - so
// a block keeps one; a thread merges the equal digits of its group of 4 before it adds.
template <bool GUIDED>
__global__ __launch_bounds__(256) void x0_count_top_kernel(const ThrArgs p) {
  __shared__ unsigned lds[kBins1];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    const DrsPredCoef k = coef_of(p, img);
    const bool count = ranked(k);
    for (int b = threadIdx.x; b < kBins1; b += blockDim.x) lds[b] = 0;
    __syncthreads();
    const int64_t row = (int64_t)img * p.chw;
    const float* pp = p.pred + row;
    const float* up = GUIDED ? p.pu + row : nullptr;
    const float* xp = p.x + row;
    float* op = p.out + row;
    const RowSpan s(p.vec, p.phase, row, p.chw);
    for (int64_t g = tid; g < s.groups; g += stride) {
      const int64_t at = s.head + 4 * g;
      const float4 p4 = *reinterpret_cast<const float4*>(pp + at);
      const float4 x4 = *reinterpret_cast<const float4*>(xp + at);
      float4 u4 = {0.f, 0.f, 0.f, 0.f};
      if constexpr (GUIDED) u4 = *reinterpret_cast<const float4*>(up + at);
      float4 o;
      o.x = thr_x0(p, k, x4.x, p4.x, u4.x, GUIDED); o.y = thr_x0(p, k, x4.y, p4.y, u4.y, GUIDED);
      o.z = thr_x0(p, k, x4.z, p4.z, u4.z, GUIDED); o.w = thr_x0(p, k, x4.w, p4.w, u4.w, GUIDED);
      *reinterpret_cast<float4*>(op + at) = o;
      if (count) {
        const unsigned a = drs_dyn_key(o.x, p.c) >> 20, b = drs_dyn_key(o.y, p.c) >> 20;
        const unsigned c = drs_dyn_key(o.z, p.c) >> 20, d = drs_dyn_key(o.w, p.c) >> 20;
        atomicAdd(lds + a, 1u + (b == a) + (c == a) + (d == a));
        if (b != a) atomicAdd(lds + b, 1u + (c == b) + (d == b));
        if (c != a && c != b) atomicAdd(lds + c, 1u + (d == c));
        if (d != a && d != b && d != c) atomicAdd(lds + d, 1u);
      }
    }
    const int64_t rest = p.chw - 4 * s.groups;  // head and tail elements: at most 6 with `vec`
    for (int64_t r = tid; r < rest; r += stride) {
      const int64_t i = r < s.head ? r : s.tail() + (r - s.head);
      const float o = thr_x0(p, k, xp[i], pp[i], GUIDED ? up[i] : 0.f, GUIDED);
      op[i] = o;
      if (count) atomicAdd(lds + (drs_dyn_key(o, p.c) >> 20), 1u);
    }
    __syncthreads();
    if (count) flush_hist<kBins1>(lds, p.hist + (int64_t)img * kHistWords);
    __syncthreads();
  }
}

// SHIFT 10: the middle digit among the keys whose top 11 bits are the prefix; SHIFT 0: the low digit under the top 21 bits
template <int SHIFT>
__global__ __launch_bounds__(256) void x0_count_next_kernel(const ThrArgs p) {
  __shared__ unsigned lds[kBins2];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    if (!ranked(coef_of(p, img))) continue;  // (uniform over the block)
    const unsigned prefix = p.state[(int64_t)img * kStateWords];
    for (int b = threadIdx.x; b < kBins2; b += blockDim.x) lds[b] = 0;
    __syncthreads();
    const int64_t row = (int64_t)img * p.chw;
    const float* op = p.out + row;
    const RowSpan s(p.vec, p.phase, row, p.chw);
    for (int64_t g = tid; g < s.groups; g += stride) {
      const float4 o = *reinterpret_cast<const float4*>(op + s.head + 4 * g);
      const unsigned key[4] = {drs_dyn_key(o.x, p.c), drs_dyn_key(o.y, p.c), drs_dyn_key(o.z, p.c), drs_dyn_key(o.w, p.c)};
      for (int j = 0; j < 4; ++j)
        if ((key[j] >> (SHIFT + 10)) == prefix) atomicAdd(lds + ((key[j] >> SHIFT) & (kBins2 - 1)), 1u);
    }
    const int64_t rest = p.chw - 4 * s.groups;
    for (int64_t r = tid; r < rest; r += stride) {
      const int64_t i = r < s.head ? r : s.tail() + (r - s.head);
      const unsigned key = drs_dyn_key(op[i], p.c);
      if ((key >> (SHIFT + 10)) == prefix) atomicAdd(lds + ((key >> SHIFT) & (kBins2 - 1)), 1u);
    }
    __syncthreads();
    flush_hist<kBins2>(lds, p.hist + (int64_t)img * kHistWords + (SHIFT ? kBins1 : kBins1 + kBins2));
    __syncthreads();
  }
}

// One block per image: the digit at which the running count of `hist` (BINS bins) passes the image's remaining rank extends
// the prefix; the rank becomes the rank within that bin.  FIRST: the rank is the call's k; LAST: the prefix is the whole key,
// whose float is the scale.  An image that was not ranked has an empty histogram: prefix 0, scale 0.
template <int BINS, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void x0_digit_kernel(const ThrArgs p, int hist_at) {
  __shared__ unsigned incl[256];
  constexpr int PER = BINS / 256;
  const int img = blockIdx.x;
  const unsigned* h = p.hist + (int64_t)img * kHistWords + hist_at;
  unsigned* st = p.state + (int64_t)img * kStateWords;
  const unsigned prefix = FIRST ? 0u : st[0];
  const unsigned rank = FIRST ? (unsigned)p.k : st[1];
  unsigned cnt[PER], sum = 0;
  for (int j = 0; j < PER; ++j) sum += cnt[j] = h[threadIdx.x * PER + j];
  incl[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {  // inclusive scan of the 256 partial counts
    const unsigned add = threadIdx.x >= off ? incl[threadIdx.x - off] : 0u;
    __syncthreads();
    incl[threadIdx.x] += add;
    __syncthreads();
  }
  const unsigned total = incl[255];
  unsigned before = incl[threadIdx.x] - sum;
  if (total <= rank) {  // not ranked (or no element matched: cannot happen for a ranked image, k < chw)
    if (threadIdx.x == 0) {
      st[0] = 0; st[1] = 0;
      if (LAST && p.scale_out) p.scale_out[img] = 0.f;
    }
    return;
  }
  if (before <= rank && rank < before + sum) {  // exactly one thread
    int j = 0;
    while (before + cnt[j] <= rank) before += cnt[j++];
    const unsigned key = (prefix << (BINS == kBins1 ? 11 : 10)) | (unsigned)(threadIdx.x * PER + j);
    st[0] = key;
    st[1] = rank - before;
    if (LAST && p.scale_out) p.scale_out[img] = __uint_as_float(key);
  }
}

__global__ __launch_bounds__(256) void x0_apply_kernel(const ThrArgs p) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int img = blockIdx.y; img < p.n; img += gridDim.y) {
    const DrsPredCoef k = coef_of(p, img);
    if (!ranked(k)) continue;  // `out` holds this image's eps already
    const DrsDynScale y(p.lo, p.hi, __uint_as_float(p.state[(int64_t)img * kStateWords]));
    const int64_t row = (int64_t)img * p.chw;
    const float* xp = p.x + row;
    float* op = p.out + row;
    const RowSpan s(p.vec, p.phase, row, p.chw);
    for (int64_t g = tid; g < s.groups; g += stride) {
      const int64_t at = s.head + 4 * g;
      const float4 q4 = *reinterpret_cast<const float4*>(op + at);
      const float4 x4 = *reinterpret_cast<const float4*>(xp + at);
      float4 o;
      o.x = drs_eps_of_x0(k, x4.x, drs_dyn_q(k, y, q4.x)); o.y = drs_eps_of_x0(k, x4.y, drs_dyn_q(k, y, q4.y));
      o.z = drs_eps_of_x0(k, x4.z, drs_dyn_q(k, y, q4.z)); o.w = drs_eps_of_x0(k, x4.w, drs_dyn_q(k, y, q4.w));
      *reinterpret_cast<float4*>(op + at) = o;
    }
    const int64_t rest = p.chw - 4 * s.groups;
    for (int64_t r = tid; r < rest; r += stride) {
      const int64_t i = r < s.head ? r : s.tail() + (r - s.head);
      op[i] = drs_eps_of_x0(k, xp[i], drs_dyn_q(k, y, op[i]));
    }
  }
}

int threshold_run(const char* what, const float* pred, const float* pred_uncond, float cfg_scale, const float* x,
                  const int64_t* t, const float* alpha_hat, int noise_steps, int kind, float lo, float hi, int64_t k, float* out,
                  float* scale, bool need_scale, bool apply, int n, int64_t chw, void* workspace, size_t workspace_bytes,
                  hipStream_t stream) {
  DRS_REQUIRE(pred && x && t && alpha_hat && out && workspace && (scale || !need_scale), DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(kind == DRS_PRED_EPS || kind == DRS_PRED_V || kind == DRS_PRED_X0, DRS_ERR_ARG,
              "%s: kind=%d is none of DRS_PRED_EPS, DRS_PRED_V, DRS_PRED_X0", what, kind);
  DRS_REQUIRE(lo < hi, DRS_ERR_ARG, "%s: the clip range needs lo < hi, got lo=%g hi=%g", what, (double)lo, (double)hi);
  DRS_REQUIRE(!pred_uncond || std::isfinite(cfg_scale), DRS_ERR_ARG, "%s: cfg_scale=%g must be finite", what, (double)cfg_scale);
  DRS_REQUIRE(n >= 0 && chw >= 0 && chw < ((int64_t)1 << 32) && noise_steps > 0, DRS_ERR_SHAPE,
              "%s: n=%d chw=%lld noise_steps=%d", what, n, (long long)chw, noise_steps);
  DRS_REQUIRE(x != out, DRS_ERR_ARG, "%s: x and out are one buffer (x is read again after out is written)", what);
  if (n == 0 || chw == 0) return DRS_OK;
  DRS_REQUIRE(k >= 0 && k < chw, DRS_ERR_ARG, "%s: rank k=%lld outside [0, chw=%lld)", what, (long long)k, (long long)chw);
  const size_t need = drs_x0_threshold_workspace_bytes(n);
  DRS_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 3u) == 0, DRS_ERR_ARG,
              "%s: workspace of %zu bytes, needs %zu (4-byte aligned)", what, workspace_bytes, need);
  ThrArgs a;
  a.pred = pred; a.pu = pred_uncond; a.w = cfg_scale; a.x = x; a.t = t; a.alpha_hat = alpha_hat; a.out = out;
  a.scale_out = scale;
  a.hist = static_cast<unsigned*>(workspace);
  a.state = a.hist + (size_t)n * kHistWords;
  a.n = n; a.noise_steps = noise_steps; a.kind = kind; a.lo = lo; a.hi = hi; a.chw = chw; a.k = k;
  a.c = (float)(((double)lo + (double)hi) / 2.0);
  DRS_CHECK_HIP(hipMemsetAsync(workspace, 0, need, stream));
  const dim3 block(256), images((unsigned)n);
  // pass 1 over every tensor of the call
  a.vec = same_phase({pred, pred_uncond, x, out});
  a.phase = phase_of(pred);
  const dim3 grid = stream_grid(n, chw, a.vec);
  if (pred_uncond) DRS_LAUNCH(x0_count_top_kernel<true>, grid, block, 0, stream, a);
  else DRS_LAUNCH(x0_count_top_kernel<false>, grid, block, 0, stream, a);
  DRS_LAUNCH((x0_digit_kernel<kBins1, true, false>), images, block, 0, stream, a, 0);
  // passes 2 and 3 read `out` alone
  a.vec = true;
  a.phase = phase_of(out);
  const dim3 grid_out = stream_grid(n, chw, true);
  DRS_LAUNCH(x0_count_next_kernel<10>, grid_out, block, 0, stream, a);
  DRS_LAUNCH((x0_digit_kernel<kBins2, false, false>), images, block, 0, stream, a, kBins1);
  DRS_LAUNCH(x0_count_next_kernel<0>, grid_out, block, 0, stream, a);
  DRS_LAUNCH((x0_digit_kernel<kBins2, false, true>), images, block, 0, stream, a, kBins1 + kBins2);
  if (apply) {
    a.vec = same_phase({x, out});
    a.phase = phase_of(out);
    DRS_LAUNCH(x0_apply_kernel, stream_grid(n, chw, a.vec), block, 0, stream, a);
  }
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

}  // namespace

extern "C" size_t drs_x0_threshold_workspace_bytes(int n) {
  return n > 0 ? (size_t)n * (kHistWords + kStateWords) * sizeof(unsigned) : 0;
}

extern "C" int drs_x0_quantile(const float* pred, const float* pred_uncond, float cfg_scale, const float* x, const int64_t* t,
                               const float* alpha_hat, int noise_steps, int kind, float lo, float hi, int64_t k, float* out,
                               float* scale, int n, int64_t chw, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return threshold_run("x0_quantile", pred, pred_uncond, cfg_scale, x, t, alpha_hat, noise_steps, kind, lo, hi, k, out, scale,
                       true, false, n, chw, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int drs_pred_to_eps_dyn(const float* pred, const float* pred_uncond, float cfg_scale, const float* x, const int64_t* t,
                                   const float* alpha_hat, int noise_steps, int kind, float lo, float hi, int64_t k, float* out,
                                   float* scale_out, int n, int64_t chw, void* workspace, size_t workspace_bytes,
                                   drs_stream_t stream) {
  return threshold_run("pred_to_eps_dyn", pred, pred_uncond, cfg_scale, x, t, alpha_hat, noise_steps, kind, lo, hi, k, out,
                       scale_out, false, true, n, chw, workspace, workspace_bytes, (hipStream_t)stream);
}
