// Per-step tile aggregation (split_aggregation_sampling.sample_scene): ONE state of scene size is denoised; every reverse
// step cuts it into the tiles the UNet sees (drs_gather_tiles), and blends the tiles' noise predictions back into one
// eps per scene element before taking the step (drs_blend_step / drs_blend_step_ddim / drs_blend_step_dpm; with known pixels
// drs_blend_step_known, which also replaces them in the same launch).  The kernels move each byte once and are bound by HBM
// traffic; none has an atomic on its data path and none clamps.
#include "drs_common.h"
#include "step_update.h"

#include <type_traits>

namespace {

// tiles[k] = scene[:, y0:y0+S, x0:x0+S] for the origin of tile min(first + k, n - 1).  blockIdx.y = k * C + c, the x-grid
// strides over the S * S / V groups of V consecutive elements of one plane.  The tile side is written with V-wide stores
// (S % V == 0); the scene side is read V-wide where its address is aligned (x0 % V == 0 and Ws % V == 0, uniform over a
// block) and element by element otherwise (an odd x0 is possible at magnification 1).  An origin that would leave the
// scene reads nothing: its elements are written as zeros.
template <int V>
__global__ __launch_bounds__(256) void gather_tiles_kernel(const float* __restrict__ scene,
                                                           const int* __restrict__ origins, float* __restrict__ tiles,
                                                           int first, int n, int C, int S, int Hs, int Ws) {
  const int k = blockIdx.y / C, c = blockIdx.y % C;
  const int src = min(first + k, n - 1);
  const int y0 = origins[2 * src], x0 = origins[2 * src + 1];
  const bool inside = y0 >= 0 && x0 >= 0 && y0 <= Hs - S && x0 <= Ws - S;
  const bool wide = V == 4 && (x0 % 4 == 0) && (Ws % 4 == 0);
  const float* sp = scene + (int64_t)c * Hs * Ws;
  float* tp = tiles + ((int64_t)k * C + c) * S * S;
  const int per_row = S / V, groups = S * per_row;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
    const int ly = g / per_row, lx = (g % per_row) * V;
    const int64_t from = (int64_t)(y0 + ly) * Ws + x0 + lx;
    if constexpr (V == 4) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (inside) {
        if (wide) v = *reinterpret_cast<const float4*>(sp + from);
        else v = make_float4(sp[from], sp[from + 1], sp[from + 2], sp[from + 3]);
      }
      *reinterpret_cast<float4*>(tp + (int64_t)ly * S + lx) = v;
    } else {
      tp[(int64_t)ly * S + lx] = inside ? sp[from] : 0.f;
    }
  }
}

// The step of one scene element once its eps is known: ancestral (t) or DDIM (t -> t_prev).  Coefficients and update are
// those of sampler_step_tab_kernel / ddim_step_kernel (step_update.h), formed by every thread from the device tables.
template <bool DDIM>
struct StepCoef;
template <>
struct StepCoef<false> {
  DrsAncestralCoef k;
  __device__ StepCoef(const float* alpha, const float* alpha_hat, const float* beta, int t, int, float)
      : k(drs_ancestral_coef(alpha, alpha_hat, beta, t)) {}
  __device__ bool draws() const { return true; }
  __device__ float step(float x, float eps) const { return drs_ancestral_update(k, x, eps); }
  __device__ float add(float v, float z) const { return drs_ancestral_noise(k, v, z); }
};
template <>
struct StepCoef<true> {
  DrsDdimCoef k;
  __device__ StepCoef(const float*, const float* alpha_hat, const float*, int t, int t_prev, float eta)
      : k(drs_ddim_coef(alpha_hat, t, t_prev, eta)) {}
  __device__ bool draws() const { return k.has_sigma; }
  __device__ float step(float x, float eps) const { return drs_ddim_update(k, x, eps); }
  __device__ float add(float v, float z) const { return drs_ddim_noise(k, v, z); }
};

// The DPM-Solver++(2M) move of dpm_step_kernel (step_update.h): `step` also returns the x0 prediction the history keeps.
struct DpmStepCoef {
  DrsDpmCoef k;
  __device__ DpmStepCoef(const float* alpha_hat, int t_q, int t, int t_p) : k(drs_dpm_coef(alpha_hat, t_q, t, t_p)) {}
  __device__ float step(float x, float eps, float& h) const {
    const float x0 = drs_dpm_x0(k, x, eps);
    const float v = drs_dpm_update(k, x, eps, h);
    h = x0;
    return v;
  }
};

enum BlendMode { kAncestral, kDdim, kDpm };

// One thread per group of V consecutive scene pixels of one row (V = 4 needs Ws % 4 == 0 and S % 4 == 0), channels in
// chunks of 4.  For every pixel the covering tiles are visited in index order - the summation order of
// aggregate_tiles_kernel: cnt += w, acc += tile * w, then acc / cnt - so the blended eps does not depend on the launch
// geometry.  A tile whose window holds the whole group at a 16-byte aligned offset is read with one float4 per plane
// (weight and eps), any other one element by element under its own bounds check: eps_tiles is only ever indexed with
// 0 <= ly, lx < S, whatever the origins hold.  A pixel no tile covers gets 0 / 0 = NaN and is counted in `uncovered`.
// MODE kDpm: `hist` (scene shape) holds the x0 prediction of the move before, read by a second-order move (t_q >= 0) and
// written by every move; it draws no noise.  With V = 4 it is accessed like `scene` and `noise`: one float4 per group at the
// group's element offset, so it wants the alignment of `scene` (both are whole torch allocations in `blend_step_`).
template <int V, BlendMode MODE>
__global__ __launch_bounds__(256) void blend_step_kernel(float* __restrict__ scene, const float* __restrict__ eps_tiles,
                                                         const int* __restrict__ origins,
                                                         const float* __restrict__ weight,
                                                         const float* __restrict__ noise, int* __restrict__ uncovered,
                                                         int n, int C, int S, int Hs, int Ws, int t, int t_prev, float eta,
                                                         const float* __restrict__ alpha,
                                                         const float* __restrict__ alpha_hat,
                                                         const float* __restrict__ beta, float* __restrict__ hist, int t_q) {
  using Coef = std::conditional_t<MODE == kDpm, DpmStepCoef, StepCoef<MODE == kDdim>>;
  const Coef coef = [&] {
    if constexpr (MODE == kDpm) return Coef(alpha_hat, t_q, t, t_prev);
    else return Coef(alpha, alpha_hat, beta, t, t_prev, eta);
  }();
  bool add_noise = false;
  if constexpr (MODE != kDpm) add_noise = noise != nullptr && coef.draws();
  const int per_row = Ws / V;
  const int64_t groups = (int64_t)Hs * per_row, hw = (int64_t)Hs * Ws, ss = (int64_t)S * S;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(g / per_row), x = (int)(g % per_row) * V;
    float cnt[V];
    for (int c0 = 0; c0 < C; c0 += 4) {
      float acc[4][V];
#pragma unroll
      for (int p = 0; p < V; ++p) {
        cnt[p] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][p] = 0.f;
      }
      for (int i = 0; i < n; ++i) {
        const int ly = y - origins[2 * i], lx = x - origins[2 * i + 1];
        if (ly < 0 || ly >= S || lx <= -V || lx >= S) continue;
        const float* wp = weight + (int64_t)ly * S + lx;
        const float* ep = eps_tiles + ((int64_t)i * C + c0) * ss + (int64_t)ly * S + lx;
        if (V == 4 && lx >= 0 && lx + 4 <= S && (lx & 3) == 0) {
          const float4 w4 = *reinterpret_cast<const float4*>(wp);
          const float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int p = 0; p < V; ++p) cnt[p] = __fadd_rn(cnt[p], w[p]);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < C) {
              const float4 e4 = *reinterpret_cast<const float4*>(ep + j * ss);
              const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
              for (int p = 0; p < V; ++p) acc[j][p] = __fadd_rn(acc[j][p], __fmul_rn(e[p], w[p]));
            }
        } else {
#pragma unroll
          for (int p = 0; p < V; ++p) {
            if (lx + p < 0 || lx + p >= S) continue;
            const float w = wp[p];
            cnt[p] = __fadd_rn(cnt[p], w);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (c0 + j < C) acc[j][p] = __fadd_rn(acc[j][p], __fmul_rn(ep[j * ss + p], w));
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c0 + j >= C) continue;
        const int64_t at = (int64_t)(c0 + j) * hw + (int64_t)y * Ws + x;
        float xs[V], zs[V];
        if constexpr (V == 4) {
          const float4 x4 = *reinterpret_cast<const float4*>(scene + at);
          xs[0] = x4.x; xs[1] = x4.y; xs[2] = x4.z; xs[3] = x4.w;
          if (add_noise) {
            const float4 z4 = *reinterpret_cast<const float4*>(noise + at);
            zs[0] = z4.x; zs[1] = z4.y; zs[2] = z4.z; zs[3] = z4.w;
          }
        } else {
          xs[0] = scene[at];
          if (add_noise) zs[0] = noise[at];
        }
        if constexpr (MODE == kDpm) {
          float hs[V] = {};
          if (coef.k.second) {
            if constexpr (V == 4) {
              const float4 h4 = *reinterpret_cast<const float4*>(hist + at);
              hs[0] = h4.x; hs[1] = h4.y; hs[2] = h4.z; hs[3] = h4.w;
            } else {
              hs[0] = hist[at];
            }
          }
#pragma unroll
          for (int p = 0; p < V; ++p) xs[p] = coef.step(xs[p], __fdiv_rn(acc[j][p], cnt[p]), hs[p]);
          if constexpr (V == 4) *reinterpret_cast<float4*>(hist + at) = make_float4(hs[0], hs[1], hs[2], hs[3]);
          else hist[at] = hs[0];
        } else {
#pragma unroll
          for (int p = 0; p < V; ++p) {
            float v = coef.step(xs[p], __fdiv_rn(acc[j][p], cnt[p]));
            if (add_noise) v = coef.add(v, zs[p]);
            xs[p] = v;
          }
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(scene + at) = make_float4(xs[0], xs[1], xs[2], xs[3]);
        else scene[at] = xs[0];
      }
    }
    if (uncovered) {
      int holes = 0;
#pragma unroll
      for (int p = 0; p < V; ++p) holes += cnt[p] == 0.f;
      if (holes) atomicAdd(uncovered, holes);
    }
  }
}

// The step of blend_step_kernel<V, kAncestral | kDdim> in the form it is compiled to.  step_update.h's expressions are plain
// products and sums, and the compiler chooses their fused multiply-adds kernel by kernel: in blend_step_kernel the choice
// depends on V and, with noise, on the band's place j in its chunk of four (its unrolled band loop hoists the noise product
// of band 1 only).  A kernel that repeats those expressions next to a select is compiled to yet other forms, so the forms of
// the plain instantiations (read off their gfx950 code) are written out here under contract(off), with u = fma(-c_eps, eps, x):
//   ancestral  V = 4   fl(c_inv u);                then fma(c_sig, z, .)   | band 1: fma(c_inv, u, fl(c_sig z))
//              V = 1   fl(c_inv u);                then . + fl(c_sig z)
//   DDIM       V = 4   w = fma(a, x, fl(b eps));   then fma(s, z, w)       | band 1: fl(s z) + w
//              V = 1   w = fl(a x) + fl(b eps);    then fma(s, z, w)       | band 1: fl(s z) + w
// tests/test_gpu_tile_known.py holds the two kernels to torch.equal on every form; a compiler that contracts the plain
// kernel otherwise fails it, and this table is then read off again.
template <int V, bool DDIM>
struct PlainStep;
template <int V>
struct PlainStep<V, false> {
  DrsAncestralCoef k;
  __device__ PlainStep(const float* alpha, const float* alpha_hat, const float* beta, int t, int, float)
      : k(drs_ancestral_coef(alpha, alpha_hat, beta, t)) {}
  __device__ bool draws() const { return true; }
  __device__ float move(int j, float x, float eps, float z, bool add_noise) const {
#pragma clang fp contract(off)
    const float u = fmaf(-k.c_eps, eps, x);
    const float v = k.c_inv * u;
    if (!add_noise) return v;
    const float q = k.c_sig * z;
    if (V == 1) return v + q;
    return j == 1 ? fmaf(k.c_inv, u, q) : fmaf(k.c_sig, z, v);
  }
};
template <int V>
struct PlainStep<V, true> {
  DrsDdimCoef k;
  __device__ PlainStep(const float*, const float* alpha_hat, const float*, int t, int t_prev, float eta)
      : k(drs_ddim_coef(alpha_hat, t, t_prev, eta)) {}
  __device__ bool draws() const { return k.has_sigma; }
  __device__ float move(int j, float x, float eps, float z, bool add_noise) const {
#pragma clang fp contract(off)
    const float p = k.a * x, q = k.b * eps;
    const float w = V == 4 ? fmaf(k.a, x, q) : p + q;
    if (!add_noise) return w;
    const float r = k.s * z;
    return j == 1 ? r + w : fmaf(k.s, z, w);
  }
};

// drs_blend_step_known: the blend and the step of blend_step_kernel<V, kAncestral | kDdim>, then the known-pixel select of
// inpaint_step_kernel (reverse_step.hip) on the scene state.  The blend is that kernel's loop, repeated here and not shared
// with it, so that the plain instantiations stay exactly as they are compiled; its sums are written as the fused
// multiply-adds they are there (acc = fma(eps, w, acc)), the step is PlainStep: the elements the mask leaves unknown carry
// the bits of drs_blend_step / drs_blend_step_ddim.  `known` (C, Hs, Ws) and `mask` (Cm = 1 | C planes of Hs x Ws bytes,
// nonzero = known) are read at the group's element offset: one float4 and one 32-bit word of four mask bytes on the V = 4
// path when their base pointers allow it (`kwide`, uniform over the launch), element by element otherwise.  A known element
// becomes `known` at t_prev == 0 and DrsKnownCoef::at(known, z) above it, z being the element of the one `noise` tensor that
// the step of an unknown element adds; so `noise` is read whenever it is given, whatever eta is.
template <int V, bool DDIM>
__global__ __launch_bounds__(256) void blend_step_known_kernel(
    float* __restrict__ scene, const float* __restrict__ eps_tiles, const int* __restrict__ origins,
    const float* __restrict__ weight, const float* __restrict__ noise, const float* __restrict__ known,
    const unsigned char* __restrict__ mask, int* __restrict__ uncovered, int n, int C, int Cm, int S, int Hs, int Ws, int t,
    int t_prev, float eta, const float* __restrict__ alpha, const float* __restrict__ alpha_hat,
    const float* __restrict__ beta) {
  const PlainStep<V, DDIM> coef(alpha, alpha_hat, beta, t, t_prev, eta);
  const DrsKnownCoef kc(alpha_hat, t_prev);
  const bool add_noise = noise != nullptr && coef.draws();
  const bool to_zero = t_prev == 0;  // the known pixels arrive at the known image itself; z is not read for them
  const bool kwide = V == 4 && ((uintptr_t)known & 15u) == 0 && ((uintptr_t)mask & 3u) == 0;
  const int per_row = Ws / V;
  const int64_t groups = (int64_t)Hs * per_row, hw = (int64_t)Hs * Ws, ss = (int64_t)S * S;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(g / per_row), x = (int)(g % per_row) * V;
    float cnt[V];
    for (int c0 = 0; c0 < C; c0 += 4) {
      float acc[4][V];
#pragma unroll
      for (int p = 0; p < V; ++p) {
        cnt[p] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][p] = 0.f;
      }
      for (int i = 0; i < n; ++i) {
        const int ly = y - origins[2 * i], lx = x - origins[2 * i + 1];
        if (ly < 0 || ly >= S || lx <= -V || lx >= S) continue;
        const float* wp = weight + (int64_t)ly * S + lx;
        const float* ep = eps_tiles + ((int64_t)i * C + c0) * ss + (int64_t)ly * S + lx;
        if (V == 4 && lx >= 0 && lx + 4 <= S && (lx & 3) == 0) {
          const float4 w4 = *reinterpret_cast<const float4*>(wp);
          const float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int p = 0; p < V; ++p) cnt[p] = __fadd_rn(cnt[p], w[p]);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < C) {
              const float4 e4 = *reinterpret_cast<const float4*>(ep + j * ss);
              const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
              for (int p = 0; p < V; ++p) acc[j][p] = fmaf(e[p], w[p], acc[j][p]);
            }
        } else {
#pragma unroll
          for (int p = 0; p < V; ++p) {
            if (lx + p < 0 || lx + p >= S) continue;
            const float w = wp[p];
            cnt[p] = __fadd_rn(cnt[p], w);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (c0 + j < C) acc[j][p] = fmaf(ep[j * ss + p], w, acc[j][p]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c0 + j >= C) continue;
        const int64_t in_plane = (int64_t)y * Ws + x, at = (int64_t)(c0 + j) * hw + in_plane;
        const unsigned char* mp = mask + (Cm == 1 ? in_plane : at);
        float xs[V], zs[V], ks[V];
        unsigned m;
        if constexpr (V == 4) {
          const float4 x4 = *reinterpret_cast<const float4*>(scene + at);
          xs[0] = x4.x; xs[1] = x4.y; xs[2] = x4.z; xs[3] = x4.w;
          if (noise) {
            const float4 z4 = *reinterpret_cast<const float4*>(noise + at);
            zs[0] = z4.x; zs[1] = z4.y; zs[2] = z4.z; zs[3] = z4.w;
          }
          if (kwide) {
            const float4 k4 = *reinterpret_cast<const float4*>(known + at);
            ks[0] = k4.x; ks[1] = k4.y; ks[2] = k4.z; ks[3] = k4.w;
            m = *reinterpret_cast<const unsigned*>(mp);
          } else {
            ks[0] = known[at]; ks[1] = known[at + 1]; ks[2] = known[at + 2]; ks[3] = known[at + 3];
            m = (unsigned)mp[0] | ((unsigned)mp[1] << 8) | ((unsigned)mp[2] << 16) | ((unsigned)mp[3] << 24);
          }
        } else {
          xs[0] = scene[at];
          if (noise) zs[0] = noise[at];
          ks[0] = known[at];
          m = mp[0];
        }
#pragma unroll
        for (int p = 0; p < V; ++p) {
          float v = coef.move(j, xs[p], __fdiv_rn(acc[j][p], cnt[p]), zs[p], add_noise);
          if ((m >> (8 * p)) & 0xffu) v = to_zero ? ks[p] : kc.at(ks[p], zs[p]);
          xs[p] = v;
        }
        if constexpr (V == 4) *reinterpret_cast<float4*>(scene + at) = make_float4(xs[0], xs[1], xs[2], xs[3]);
        else scene[at] = xs[0];
      }
    }
    if (uncovered) {
      int holes = 0;
#pragma unroll
      for (int p = 0; p < V; ++p) holes += cnt[p] == 0.f;
      if (holes) atomicAdd(uncovered, holes);
    }
  }
}

}  // namespace

extern "C" int drs_gather_tiles(const float* scene, const int32_t* origins, float* tiles, int first, int count, int n, int C,
                                int S, int Hs, int Ws, drs_stream_t stream) {
  DRS_REQUIRE(scene && origins && tiles, DRS_ERR_ARG, "gather_tiles: null pointer");
  DRS_REQUIRE(n >= 1 && first >= 0 && first < n && count >= 1, DRS_ERR_ARG, "gather_tiles: first=%d count=%d n=%d", first,
              count, n);
  DRS_REQUIRE(C >= 1 && S >= 1 && Hs >= S && Ws >= S, DRS_ERR_SHAPE, "gather_tiles: C=%d S=%d Hs=%d Ws=%d", C, S, Hs, Ws);
  DRS_REQUIRE((int64_t)count * C <= 65535, DRS_ERR_SHAPE, "gather_tiles: count=%d x C=%d planes exceed one launch", count, C);
  const unsigned planes = (unsigned)(count * C);
  if (S % 4 == 0) {
    DRS_LAUNCH(gather_tiles_kernel<4>, dim3(ew_blocks((int64_t)S * S / 4), planes), dim3(256), 0, (hipStream_t)stream, scene,
               origins, tiles, first, n, C, S, Hs, Ws);
  } else {
    DRS_LAUNCH(gather_tiles_kernel<1>, dim3(ew_blocks((int64_t)S * S), planes), dim3(256), 0, (hipStream_t)stream, scene,
               origins, tiles, first, n, C, S, Hs, Ws);
  }
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

namespace {

template <BlendMode MODE>
int launch_blend(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight, const float* noise,
                 int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t, int t_prev, float eta, const float* alpha,
                 const float* alpha_hat, const float* beta, hipStream_t s, float* hist = nullptr, int t_q = -1) {
  if (S % 4 == 0 && Ws % 4 == 0) {
    DRS_LAUNCH((blend_step_kernel<4, MODE>), dim3(ew_blocks((int64_t)Hs * (Ws / 4))), dim3(256), 0, s, scene, eps_tiles,
               origins, weight, noise, uncovered, n, C, S, Hs, Ws, t, t_prev, eta, alpha, alpha_hat, beta, hist, t_q);
  } else {
    DRS_LAUNCH((blend_step_kernel<1, MODE>), dim3(ew_blocks((int64_t)Hs * Ws)), dim3(256), 0, s, scene, eps_tiles, origins,
               weight, noise, uncovered, n, C, S, Hs, Ws, t, t_prev, eta, alpha, alpha_hat, beta, hist, t_q);
  }
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

}  // namespace

#define DRS_BLEND_REQUIRE(what)                                                                                           \
  DRS_REQUIRE(scene && eps_tiles && origins && weight, DRS_ERR_ARG, what ": null pointer");                               \
  DRS_REQUIRE(n >= 1 && C >= 1 && S >= 1 && Hs >= S && Ws >= S, DRS_ERR_SHAPE, what ": n=%d C=%d S=%d Hs=%d Ws=%d", n, C, S, \
              Hs, Ws)

extern "C" int drs_blend_step(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                              const float* noise, int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t,
                              const float* alpha, const float* alpha_hat, const float* beta, int noise_steps,
                              drs_stream_t stream) {
  DRS_BLEND_REQUIRE("blend_step");
  DRS_REQUIRE(alpha && alpha_hat && beta, DRS_ERR_ARG, "blend_step: null schedule table");
  if (int st = drs_check_move("blend_step", false, 0, t, 0, 0.f, noise_steps, noise, DRS_NOISE_OPTIONAL)) return st;
  return launch_blend<kAncestral>(scene, eps_tiles, origins, weight, noise, uncovered, n, C, S, Hs, Ws, t, 0, 0.f, alpha,
                                  alpha_hat, beta, (hipStream_t)stream);
}

extern "C" int drs_blend_step_ddim(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                                   const float* noise, int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t,
                                   int t_prev, float eta, const float* alpha_hat, int noise_steps, drs_stream_t stream) {
  DRS_BLEND_REQUIRE("blend_step_ddim");
  DRS_REQUIRE(alpha_hat, DRS_ERR_ARG, "blend_step_ddim: null schedule table");
  if (int st = drs_check_move("blend_step_ddim", true, 0, t, t_prev, eta, noise_steps, noise, DRS_NOISE_IF_SIGMA)) return st;
  return launch_blend<kDdim>(scene, eps_tiles, origins, weight, noise, uncovered, n, C, S, Hs, Ws, t, t_prev, eta, nullptr,
                             alpha_hat, nullptr, (hipStream_t)stream);
}

extern "C" int drs_blend_step_dpm(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                                  float* x0_hist, int32_t* uncovered, int n, int C, int S, int Hs, int Ws, int t_q, int t,
                                  int t_p, const float* alpha_hat, int noise_steps, drs_stream_t stream) {
  DRS_BLEND_REQUIRE("blend_step_dpm");
  DRS_REQUIRE(x0_hist && alpha_hat, DRS_ERR_ARG, "blend_step_dpm: null history or schedule table");
  if (int st = drs_check_dpm_move("blend_step_dpm", t_q, t, t_p, noise_steps)) return st;
  return launch_blend<kDpm>(scene, eps_tiles, origins, weight, nullptr, uncovered, n, C, S, Hs, Ws, t, t_p, 0.f, nullptr,
                            alpha_hat, nullptr, (hipStream_t)stream, x0_hist, t_q);
}

namespace {

template <bool DDIM>
int launch_blend_known(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight, const float* noise,
                       const float* known, const uint8_t* mask, int32_t* uncovered, int n, int C, int Cm, int S, int Hs, int Ws,
                       int t, int t_prev, float eta, const float* alpha, const float* alpha_hat, const float* beta,
                       hipStream_t s) {
  if (S % 4 == 0 && Ws % 4 == 0) {
    DRS_LAUNCH((blend_step_known_kernel<4, DDIM>), dim3(ew_blocks((int64_t)Hs * (Ws / 4))), dim3(256), 0, s, scene, eps_tiles,
               origins, weight, noise, known, mask, uncovered, n, C, Cm, S, Hs, Ws, t, t_prev, eta, alpha, alpha_hat, beta);
  } else {
    DRS_LAUNCH((blend_step_known_kernel<1, DDIM>), dim3(ew_blocks((int64_t)Hs * Ws)), dim3(256), 0, s, scene, eps_tiles,
               origins, weight, noise, known, mask, uncovered, n, C, Cm, S, Hs, Ws, t, t_prev, eta, alpha, alpha_hat, beta);
  }
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

}  // namespace

extern "C" int drs_blend_step_known(float* scene, const float* eps_tiles, const int32_t* origins, const float* weight,
                                    const float* noise, const float* known, const uint8_t* mask, int32_t* uncovered, int n,
                                    int C, int S, int Hs, int Ws, int mask_channels, int ddim, int t, int t_prev, float eta,
                                    const float* alpha, const float* alpha_hat, const float* beta, int noise_steps,
                                    drs_stream_t stream) {
  DRS_BLEND_REQUIRE("blend_step_known");
  DRS_REQUIRE(known && mask && alpha_hat, DRS_ERR_ARG, "blend_step_known: null known image, mask or schedule table");
  DRS_REQUIRE(mask_channels == 1 || mask_channels == C, DRS_ERR_SHAPE,
              "blend_step_known: a mask of %d bands for a scene of %d (1 or %d)", mask_channels, C, C);
  if (!ddim) DRS_REQUIRE(alpha && beta, DRS_ERR_ARG, "blend_step_known: the ancestral form needs the alpha and beta tables");
  // above level 0 every element reads z: the unknown ones as the step's noise, the known ones as their forward noise
  if (int st = drs_check_move("blend_step_known", ddim, 1, t, t_prev, eta, noise_steps, noise, DRS_NOISE_ABOVE_0)) return st;
  if (!ddim) t_prev = t - 1;
  return ddim ? launch_blend_known<true>(scene, eps_tiles, origins, weight, noise, known, mask, uncovered, n, C, mask_channels,
                                         S, Hs, Ws, t, t_prev, eta, nullptr, alpha_hat, nullptr, (hipStream_t)stream)
              : launch_blend_known<false>(scene, eps_tiles, origins, weight, noise, known, mask, uncovered, n, C, mask_channels,
                                          S, Hs, Ws, t, t_prev, 0.f, alpha, alpha_hat, beta, (hipStream_t)stream);
}
