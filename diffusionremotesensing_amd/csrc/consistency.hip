// LR-consistent sampling: the range-null-space projection of an implied x0 onto { x : A_y x A_x^T = y } for a separable linear
// degradation (Wang et al., "DDNM", 2023), damped in the SVD basis.  With the thin SVDs A = P diag(s) V^T
// per axis the host hands over  D = diag(s) V^T (h x H, w x W),  U = V (H x h, W x w),  the gain G (h x w) and, per plane,
// Yt = P_y^T y P_x; a plane moves to
//   X' = X + strength * U_y (G o (Yt - D_y X D_x^T)) U_x^T.
// Four batched products, all of the form C = A B^T with both operands row-major along the summed index:
//   1  T1^T (w x H) = D_x  X^T          (X: the plane, or the x0 an eps prediction implies, formed as it is loaded)
//   2  R    (h x w) = G o (Yt - D_y T1)
//   3  T2^T (W x h) = U_x  R^T
//   4  out  (H x W) = X + strength U_y T2      (or eps' = eps - sqrt(ah / (1 - ah)) strength U_y T2: x0 is never stored)
// on v_mfma_f32_16x16x4_f32: exact fp32 products, one rounding per product, accumulated in a fixed order - no atomics, no split
// operands, so two calls give the same bits.  A lane's four consecutive k of an operand row are one 16-byte load when the
// pointer, the row length and the plane stride allow it and four 4-byte loads otherwise: the same elements reach the same MFMA
// in the same order, so an unaligned pointer changes no bit.  The intermediates live in the workspace (T1^T and T2^T share it).
// Per-band operators: D, U and G may be stacks of n_ops operators; a plane takes the matrix operand and
// the gain of slot op[plane % bands], a 16-byte table in the kernel arguments.  One operator is slot 0 for every band: the same
// addresses, tiles and MFMA order as before the table existed, so the one-operator entries keep their bits.
#include "drs_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { LOAD_PLAIN = 0, LOAD_X0 = 1 };
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_ADD = 2, EPI_EPS = 3 };
constexpr int kTile = 64;  // a block's tile of C: 4 waves of 32 x 32, each 2 x 2 MFMA tiles

struct SepArgs {
  const float* A;   // M x K, row-major; a_plane floats between planes (0: one matrix per operator slot, a_slot floats apart)
  const float* B;   // N x K
  const float* B2;  // LOAD_X0: eps beside the state B
  float* C;         // M x N
  const float* E1;  // EPI_RESID: Yt; EPI_ADD: X - laid out as C
  const float* E2;  // EPI_RESID: the gain, one M x N matrix per operator slot
  const int64_t* t;
  const float* alpha_hat;
  int64_t a_plane, a_slot, b_plane, c_plane;
  int M, N, K, planes, bands, noise_steps;
  float strength;
  bool a_vec, b_vec;
  signed char op[kMaxBands];  // the operator slot of each band (all 0: one operator)
};

// elements k .. k + 3 of a row of K (zero past the end and for a row outside the matrix); `vec`: k % 4 == K % 4 == 0, 16-byte aligned
__device__ __forceinline__ f32x4 load_k4(const float* row, bool row_ok, int k, int K, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!row_ok || k >= K) return v;
  if (vec) return *reinterpret_cast<const f32x4*>(row + k);
  v.x = row[k];
  if (k + 1 < K) v.y = row[k + 1];
  if (k + 2 < K) v.z = row[k + 2];
  if (k + 3 < K) v.w = row[k + 3];
  return v;
}

// x0 = fl(ca x) + fl(cb eps), ca = 1 / sqrt(ah), cb = -sqrt(1 - ah) / sqrt(ah) (drs_dpm_x0's form)
__device__ __forceinline__ f32x4 x0_of(f32x4 x, f32x4 e, float ca, float cb) {
#pragma clang fp contract(off)
  const f32x4 p = x * ca, q = e * cb;
  return p + q;
}

template <int LOAD, int EPI>
__global__ __launch_bounds__(256) void sep_gemm_kernel(const SepArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * kTile + (wave >> 1) * 32, n0 = blockIdx.x * kTile + (wave & 1) * 32;
  if (m0 >= p.M || n0 >= p.N) return;  // (the whole wave: no barrier below)
  for (int pl = blockIdx.z; pl < p.planes; pl += gridDim.z) {
    float ca = 0.f, cb = 0.f, ce = 0.f;
    if (LOAD == LOAD_X0 || EPI == EPI_EPS) {  // fp64 from the fp32 table entry, each coefficient rounded once (drs_ddim_coef)
      const int64_t tn = p.t[pl / p.bands];
      if (tn < 0 || tn >= p.noise_steps) {  // never indexes the table: the image comes out NaN
        ca = cb = ce = __builtin_nanf("");
      } else {
        const double ah = (double)p.alpha_hat[tn], a = sqrt(ah), s = sqrt(fmax(1.0 - ah, 0.0));
        ca = (float)(1.0 / a);
        cb = (float)(-s / a);
        ce = (float)(a / s * (double)p.strength);
      }
    }
    const int slot = p.op[pl % p.bands];
    const float* A = p.A + (int64_t)pl * p.a_plane + (int64_t)slot * p.a_slot;
    const float* B = p.B + (int64_t)pl * p.b_plane;
    const float* B2 = LOAD == LOAD_X0 ? p.B2 + (int64_t)pl * p.b_plane : nullptr;
    const float* arow[2];
    const float* brow[2];
    const float* erow[2];
    bool aok[2], bok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + 16 * i + r, n = n0 + 16 * i + r;
      aok[i] = m < p.M;
      bok[i] = n < p.N;
      arow[i] = A + (int64_t)(aok[i] ? m : 0) * p.K;
      brow[i] = B + (int64_t)(bok[i] ? n : 0) * p.K;
      erow[i] = LOAD == LOAD_X0 ? B2 + (int64_t)(bok[i] ? n : 0) * p.K : nullptr;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // a chunk of 16 k: lane (r, q) holds k0 + 4 q + s, s = 0 .. 3, of its rows; MFMA s sums its four q in order
#pragma unroll 2
    for (int k0 = 0; k0 < p.K; k0 += 16) {
      const int k = k0 + 4 * q;
      f32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = load_k4(arow[i], aok[i], k, p.K, p.a_vec);
        b[i] = load_k4(brow[i], bok[i], k, p.K, p.b_vec);
        if (LOAD == LOAD_X0) b[i] = x0_of(b[i], load_k4(erow[i], bok[i], k, p.K, p.b_vec), ca, cb);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
    }
    // lane (r, q) holds C[m0 + 16 i + 4 q + e][n0 + 16 j + r] in acc[i][j][e]
    float* Cp = p.C + (int64_t)pl * p.c_plane;
    const float* E1 = (EPI == EPI_RESID || EPI == EPI_ADD) ? p.E1 + (int64_t)pl * p.c_plane : nullptr;
    const float* E2 = EPI == EPI_RESID ? p.E2 + (int64_t)slot * p.c_plane : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int m = m0 + 16 * i + 4 * q + e, n = n0 + 16 * j + r;
          if (m >= p.M || n >= p.N) continue;
          const int64_t at = (int64_t)m * p.N + n;
          const float v = acc[i][j][e];
          float o;
          {
#pragma clang fp contract(off)
            if (EPI == EPI_STORE) {
              o = v;
            } else if (EPI == EPI_RESID) {
              const float d = E1[at] - v;
              o = E2[at] * d;
            } else if (EPI == EPI_ADD) {
              const float d = p.strength * v;
              o = E1[at] + d;
            } else {
              const float d = ce * v;
              o = Cp[at] - d;
            }
          }
          Cp[at] = o;
        }
  }
}

bool vec_ok(const float* ptr, int K, int64_t plane) { return aligned16(ptr) && K % 4 == 0 && plane % 4 == 0; }

template <int LOAD, int EPI>
void launch(SepArgs a, hipStream_t stream) {
  a.a_vec = vec_ok(a.A, a.K, a.a_plane) && a.a_slot % 4 == 0;
  a.b_vec = vec_ok(a.B, a.K, a.b_plane) && (LOAD != LOAD_X0 || vec_ok(a.B2, a.K, a.b_plane));
  const dim3 grid((unsigned)drs_cdiv(a.N, kTile), (unsigned)drs_cdiv(a.M, kTile), (unsigned)std::min(a.planes, 65535));
  DRS_LAUNCH((sep_gemm_kernel<LOAD, EPI>), grid, dim3(256), 0, stream, a);
}

// the operator slot of every band: band_op as the caller gave it (host memory), or band b -> min(b, n_ops - 1)
struct BandSlots {
  signed char op[kMaxBands];
};

int check_slots(const char* what, int c, const int32_t* band_op, int n_ops, BandSlots* slots) {
  DRS_REQUIRE(n_ops >= 1 && n_ops <= c, DRS_ERR_SHAPE, "%s: n_ops=%d outside 1 .. c=%d", what, n_ops, c);
  *slots = BandSlots{};
  for (int b = 0; b < c; ++b) {
    const int op = band_op ? band_op[b] : std::min(b, n_ops - 1);
    DRS_REQUIRE(op >= 0 && op < n_ops, DRS_ERR_SHAPE, "%s: band_op[%d]=%d outside 0 .. n_ops-1=%d", what, b, op, n_ops - 1);
    slots->op[b] = (signed char)op;
  }
  return DRS_OK;
}

struct SepShape {
  int n, c, H, W, h, w;
  BandSlots slots;  // (all 0 until check_slots fills it)
  int planes() const { return n * c; }
  int64_t t_floats() const { return (int64_t)planes() * std::max((int64_t)w * H, (int64_t)W * h); }
  int64_t r_floats() const { return (int64_t)planes() * h * w; }
};

int check_shape(const char* what, const SepShape& s) {
  DRS_REQUIRE(s.n >= 1 && s.c >= 1 && s.H >= 1 && s.W >= 1 && s.h >= 1 && s.w >= 1, DRS_ERR_SHAPE,
              "%s: every extent must be >= 1, got n=%d c=%d H=%d W=%d h=%d w=%d", what, s.n, s.c, s.H, s.W, s.h, s.w);
  DRS_REQUIRE(s.c <= kMaxBands, DRS_ERR_SHAPE, "%s: c=%d bands, at most %d", what, s.c, kMaxBands);
  const int64_t lim = (int64_t)1 << 31;
  DRS_REQUIRE((int64_t)s.H * s.W < lim && (int64_t)s.h * s.H < lim && (int64_t)s.w * s.W < lim && (int64_t)s.n * s.c < lim,
              DRS_ERR_SHAPE, "%s: a plane or a matrix of 2^31 elements or more (H=%d W=%d h=%d w=%d)", what, s.H, s.W, s.h, s.w);
  return DRS_OK;
}

// the 16-byte aligned start of the intermediates inside the caller's workspace
float* ws_base(void* workspace) { return reinterpret_cast<float*>(((uintptr_t)workspace + 15u) & ~(uintptr_t)15u); }

int check_workspace(const char* what, const SepShape& s, const void* workspace, size_t bytes) {
  DRS_REQUIRE(workspace, DRS_ERR_ARG, "%s: null pointer", what);
  const size_t need = drs_sep_workspace_bytes(s.n, s.c, s.H, s.W, s.h, s.w);
  DRS_REQUIRE(bytes >= need && ((uintptr_t)workspace & 3u) == 0, DRS_ERR_WORKSPACE,
              "%s: workspace of %zu bytes, needs %zu (4-byte aligned)", what, bytes, need);
  return DRS_OK;
}

// products 1 and 2: C2 (h x w per plane) = epilogue(D_y X D_x^T), X from `x` (and `eps` with LOAD_X0)
template <int LOAD, int EPI>
void run_down(const SepShape& s, const float* x, const float* eps, const int64_t* t, const float* alpha_hat, int noise_steps,
              const float* d_y, const float* d_x, const float* yt, const float* gain, float* t1, float* c2, hipStream_t stream) {
  SepArgs a = {};
  a.planes = s.planes(); a.bands = s.c; a.t = t; a.alpha_hat = alpha_hat; a.noise_steps = noise_steps; a.strength = 0.f;
  std::copy(s.slots.op, s.slots.op + kMaxBands, a.op);
  a.A = d_x; a.a_plane = 0; a.a_slot = (int64_t)s.w * s.W; a.B = x; a.B2 = eps; a.b_plane = (int64_t)s.H * s.W;
  a.C = t1; a.c_plane = (int64_t)s.w * s.H; a.M = s.w; a.N = s.H; a.K = s.W;
  launch<LOAD, EPI_STORE>(a, stream);
  a.A = d_y; a.a_slot = (int64_t)s.h * s.H; a.B = t1; a.B2 = nullptr; a.b_plane = (int64_t)s.w * s.H;
  a.C = c2; a.c_plane = (int64_t)s.h * s.w; a.M = s.h; a.N = s.w; a.K = s.H;
  a.E1 = yt; a.E2 = gain;
  launch<LOAD_PLAIN, EPI>(a, stream);
}

// products 3 and 4: C = epilogue(U_y R U_x^T) over the H x W planes
template <int EPI>
void run_up(const SepShape& s, const float* r, const float* u_y, const float* u_x, float strength, const float* x, float* out,
            const int64_t* t, const float* alpha_hat, int noise_steps, float* t2, hipStream_t stream) {
  SepArgs a = {};
  a.planes = s.planes(); a.bands = s.c; a.t = t; a.alpha_hat = alpha_hat; a.noise_steps = noise_steps; a.strength = strength;
  std::copy(s.slots.op, s.slots.op + kMaxBands, a.op);
  a.A = u_x; a.a_plane = 0; a.a_slot = (int64_t)s.W * s.w; a.B = r; a.b_plane = (int64_t)s.h * s.w;
  a.C = t2; a.c_plane = (int64_t)s.W * s.h; a.M = s.W; a.N = s.h; a.K = s.w;
  launch<LOAD_PLAIN, EPI_STORE>(a, stream);
  a.A = u_y; a.a_slot = (int64_t)s.H * s.h; a.B = t2; a.b_plane = (int64_t)s.W * s.h;
  a.C = out; a.c_plane = (int64_t)s.H * s.W; a.M = s.H; a.N = s.W; a.K = s.h;
  a.E1 = x;
  launch<LOAD_PLAIN, EPI>(a, stream);
}

}  // namespace

extern "C" size_t drs_sep_workspace_bytes(int n, int c, int H, int W, int h, int w) {
  if (n < 1 || c < 1 || H < 1 || W < 1 || h < 1 || w < 1) return 0;
  const SepShape s{n, c, H, W, h, w};
  return (size_t)(s.t_floats() + s.r_floats()) * sizeof(float) + 16;
}


namespace {

int apply_bands(const char* what, const float* x, const float* d_y, const float* d_x, float* out, SepShape s,
                const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  DRS_REQUIRE(x && d_y && d_x && out, DRS_ERR_ARG, "%s: null pointer", what);
  if (int st = check_shape(what, s)) return st;
  if (int st = check_slots(what, s.c, band_op, n_ops, &s.slots)) return st;
  if (int st = check_workspace(what, s, workspace, workspace_bytes)) return st;
  run_down<LOAD_PLAIN, EPI_STORE>(s, x, nullptr, nullptr, nullptr, 0, d_y, d_x, nullptr, nullptr, ws_base(workspace), out,
                                  (hipStream_t)stream);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

int project_bands(const char* what, const float* x, const float* yt, const float* d_y, const float* d_x, const float* u_y,
                  const float* u_x, const float* gain, float strength, float* out, SepShape s, const int32_t* band_op, int n_ops,
                  void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  DRS_REQUIRE(x && yt && d_y && d_x && u_y && u_x && gain && out, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(std::isfinite(strength), DRS_ERR_ARG, "%s: strength=%g must be finite", what, (double)strength);
  if (int st = check_shape(what, s)) return st;
  if (int st = check_slots(what, s.c, band_op, n_ops, &s.slots)) return st;
  if (int st = check_workspace(what, s, workspace, workspace_bytes)) return st;
  hipStream_t hs = (hipStream_t)stream;
  if (strength == 0.f) {  // the identity, bit for bit
    if (out != x)
      DRS_CHECK_HIP(hipMemcpyAsync(out, x, (size_t)s.planes() * s.H * s.W * sizeof(float), hipMemcpyDeviceToDevice, hs));
    return DRS_OK;
  }
  float* tbuf = ws_base(workspace);
  float* rbuf = tbuf + s.t_floats();
  run_down<LOAD_PLAIN, EPI_RESID>(s, x, nullptr, nullptr, nullptr, 0, d_y, d_x, yt, gain, tbuf, rbuf, hs);
  run_up<EPI_ADD>(s, rbuf, u_y, u_x, strength, x, out, nullptr, nullptr, 0, tbuf, hs);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

int project_eps_bands(const char* what, float* eps, const float* x, const int64_t* t, const float* alpha_hat, int noise_steps,
                      const float* yt, const float* d_y, const float* d_x, const float* u_y, const float* u_x, const float* gain,
                      float strength, SepShape s, const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                      drs_stream_t stream) {
  DRS_REQUIRE(eps && x && t && alpha_hat && yt && d_y && d_x && u_y && u_x && gain, DRS_ERR_ARG, "%s: null pointer", what);
  DRS_REQUIRE(noise_steps >= 1, DRS_ERR_ARG, "%s: noise_steps=%d", what, noise_steps);
  DRS_REQUIRE(std::isfinite(strength), DRS_ERR_ARG, "%s: strength=%g must be finite", what, (double)strength);
  DRS_REQUIRE(eps != x, DRS_ERR_ARG, "%s: eps and x are one buffer", what);
  if (int st = check_shape(what, s)) return st;
  if (int st = check_slots(what, s.c, band_op, n_ops, &s.slots)) return st;
  if (int st = check_workspace(what, s, workspace, workspace_bytes)) return st;
  if (strength == 0.f) return DRS_OK;  // eps keeps its bits
  hipStream_t hs = (hipStream_t)stream;
  float* tbuf = ws_base(workspace);
  float* rbuf = tbuf + s.t_floats();
  run_down<LOAD_X0, EPI_RESID>(s, x, eps, t, alpha_hat, noise_steps, d_y, d_x, yt, gain, tbuf, rbuf, hs);
  run_up<EPI_EPS>(s, rbuf, u_y, u_x, strength, nullptr, eps, t, alpha_hat, noise_steps, tbuf, hs);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

}  // namespace

extern "C" int drs_sep_apply_bands(const float* x, const float* d_y, const float* d_x, float* out, int n, int c, int H, int W,
                                   int h, int w, const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                                   drs_stream_t stream) {
  return apply_bands("sep_apply_bands", x, d_y, d_x, out, SepShape{n, c, H, W, h, w}, band_op, n_ops, workspace, workspace_bytes,
                     stream);
}

extern "C" int drs_sep_project_bands(const float* x, const float* yt, const float* d_y, const float* d_x, const float* u_y,
                                     const float* u_x, const float* gain, float strength, float* out, int n, int c, int H, int W,
                                     int h, int w, const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                                     drs_stream_t stream) {
  return project_bands("sep_project_bands", x, yt, d_y, d_x, u_y, u_x, gain, strength, out, SepShape{n, c, H, W, h, w}, band_op,
                       n_ops, workspace, workspace_bytes, stream);
}

extern "C" int drs_sep_project_eps_bands(float* eps, const float* x, const int64_t* t, const float* alpha_hat, int noise_steps,
                                         const float* yt, const float* d_y, const float* d_x, const float* u_y, const float* u_x,
                                         const float* gain, float strength, int n, int c, int H, int W, int h, int w,
                                         const int32_t* band_op, int n_ops, void* workspace, size_t workspace_bytes,
                                         drs_stream_t stream) {
  return project_eps_bands("sep_project_eps_bands", eps, x, t, alpha_hat, noise_steps, yt, d_y, d_x, u_y, u_x, gain, strength,
                           SepShape{n, c, H, W, h, w}, band_op, n_ops, workspace, workspace_bytes, stream);
}

// one operator for all bands: the calls above with n_ops = 1
extern "C" int drs_sep_apply(const float* x, const float* d_y, const float* d_x, float* out, int n, int c, int H, int W, int h,
                             int w, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return apply_bands("sep_apply", x, d_y, d_x, out, SepShape{n, c, H, W, h, w}, nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int drs_sep_project(const float* x, const float* yt, const float* d_y, const float* d_x, const float* u_y,
                               const float* u_x, const float* gain, float strength, float* out, int n, int c, int H, int W,
                               int h, int w, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return project_bands("sep_project", x, yt, d_y, d_x, u_y, u_x, gain, strength, out, SepShape{n, c, H, W, h, w}, nullptr, 1,
                       workspace, workspace_bytes, stream);
}

extern "C" int drs_sep_project_eps(float* eps, const float* x, const int64_t* t, const float* alpha_hat, int noise_steps,
                                   const float* yt, const float* d_y, const float* d_x, const float* u_y, const float* u_x,
                                   const float* gain, float strength, int n, int c, int H, int W, int h, int w, void* workspace,
                                   size_t workspace_bytes, drs_stream_t stream) {
  return project_eps_bands("sep_project_eps", eps, x, t, alpha_hat, noise_steps, yt, d_y, d_x, u_y, u_x, gain, strength,
                           SepShape{n, c, H, W, h, w}, nullptr, 1, workspace, workspace_bytes, stream);
}
