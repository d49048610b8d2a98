// Sensor-MTF degradation (mtf.py; not in the reference): a separable FIR blur and decimation by m, one
// launch per batch, one pair of tap rows per operator slot and a slot per band:
//   out[i][j] = sum_u ky[op][u] * sum_v kx[op][v] * x[clamp(i m + u - Ly)][clamp(j m + v - Lx)],   op = band_op[band]
// A 256-thread block owns one TH x TW tile of LR pixels of one plane (blockIdx.x = the tile, blockIdx.y strides over the planes):
//   1. the tile's input window - wr = (TH - 1) m + ntaps_y rows, wc = (TW - 1) m + ntaps_x columns from (ty0 m - Ly, tx0 m - Lx),
//      every index clamped into the image - goes to LDS in groups of four columns that start on a multiple of four columns of
//      the image: one 16-byte load where the group lies inside the row and pointer and W allow it, four 4-byte loads of the
//      same (clamped) elements otherwise.  The window so starts `off` = 0 .. 3 columns into its LDS rows;
//   2. row-direction pass: t[r][j] = sum_v kx[v] win[r][j m + v] for every window row r and tile column j, an fmaf chain from 0
//      in ascending v, stored transposed (t[j][r]);
//   3. column-direction pass: out[i][j] = sum_u ky[u] t[j][i m + u], the same kind of chain in ascending u, then the epilogue
//      v = fmaf(sigma[band], z, v) (with noise) and min(max(v, 0), 1) (with clamp01), and the store.
//   The chains depend on nothing but the output pixel: tile size, tile position, pointer phase and run change no bit.
// LDS: one word per element.  bank = word address mod 32, conflicts counted within a 32-lane half.  Pass 2 gives consecutive
// lanes consecutive r of one j: words r pitch + const with an odd pitch - 32 distinct banks - and writes consecutive words of
// t[j][.].  Pass 3 gives consecutive lanes consecutive j: words j tp + const with an odd tp.  The taps sit in LDS too: every
// lane reads the same word (a broadcast).  The tile is the largest of a fixed list whose window, t and taps fit 64 KB, so
// at least two blocks share a CU's 160 KB: 32 x 32 at m = 2 with 8 taps (29 KB), 8 x 8 at m = 8 with 46 taps (46 KB).
// No atomics; every output element is written once, by one thread.
#include "drs_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTaps = 64;
constexpr int kMaxFactor = 8;
constexpr size_t kLdsBudget = 64 * 1024;

struct FirArgs {
  const float* x;
  const float* ky;  // (n_ops, ny)
  const float* kx;  // (n_ops, nx)
  const float* noise;
  const float* sigma;
  float* out;
  int planes, bands, H, W, h, w;
  int ny, nx, Ly, Lx, m;
  int TH, TW, tiles_x;
  int wr, ng, pitch, tp;  // window rows, 4-column groups per window row, LDS pitch of the window (odd), of t (odd)
  int clamp01;
  bool vec;
  signed char op[kMaxBands];
};

__global__ __launch_bounds__(kThreads) void fir_decimate_kernel(const FirArgs p) {
  extern __shared__ float lds[];
  float* sky = lds;                       // kMaxTaps
  float* skx = lds + kMaxTaps;            // kMaxTaps
  float* win = lds + 2 * kMaxTaps;        // wr x pitch
  float* tt = win + p.wr * p.pitch;       // TW x tp
  const int tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
  const int ty0 = tile_y * p.TH, tx0 = tile_x * p.TW;
  const int th = min(p.TH, p.h - ty0), tw = min(p.TW, p.w - tx0);
  const int gy0 = ty0 * p.m - p.Ly, gx0 = tx0 * p.m - p.Lx;  // the window's first row and column (may lie outside the image)
  const int ax0 = gx0 & ~3, off = gx0 - ax0;                  // the multiple of four at or below gx0
  const long long plane = (long long)p.H * p.W, oplane = (long long)p.h * p.w;
  for (int pl = blockIdx.y; pl < p.planes; pl += gridDim.y) {
    const int band = pl % p.bands, op = p.op[band];
    if ((int)threadIdx.x < p.ny) sky[threadIdx.x] = p.ky[op * p.ny + threadIdx.x];
    if ((int)threadIdx.x >= 64 && (int)threadIdx.x - 64 < p.nx) skx[threadIdx.x - 64] = p.kx[op * p.nx + threadIdx.x - 64];
    const float* __restrict__ xp = p.x + pl * plane;
    for (int idx = threadIdx.x; idx < p.wr * p.ng; idx += kThreads) {
      const int r = idx / p.ng, g = idx - r * p.ng;
      const int sy = min(max(gy0 + r, 0), p.H - 1), c0 = ax0 + 4 * g;
      const float* __restrict__ row = xp + (long long)sy * p.W;
      float v[4];
      if (p.vec && c0 >= 0 && c0 + 3 < p.W) {
        const float4 q = *reinterpret_cast<const float4*>(row + c0);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = row[min(max(c0 + k, 0), p.W - 1)];
      }
      float* d = win + r * p.pitch + 4 * g;
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = v[k];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < p.wr * p.TW; idx += kThreads) {
      const int j = idx / p.wr, r = idx - j * p.wr;
      const float* s = win + r * p.pitch + off + j * p.m;
      float acc = 0.f;
      for (int v = 0; v < p.nx; ++v) acc = fmaf(skx[v], s[v], acc);
      tt[j * p.tp + r] = acc;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < p.TH * p.TW; idx += kThreads) {
      const int i = idx / p.TW, j = idx - i * p.TW;
      if (i >= th || j >= tw) continue;
      const float* s = tt + j * p.tp + i * p.m;
      float acc = 0.f;
      for (int u = 0; u < p.ny; ++u) acc = fmaf(sky[u], s[u], acc);
      const long long at = pl * oplane + (long long)(ty0 + i) * p.w + (tx0 + j);
      if (p.noise) acc = fmaf(p.sigma[band], p.noise[at], acc);
      if (p.clamp01) acc = fminf(fmaxf(acc, 0.f), 1.f);
      p.out[at] = acc;
    }
    __syncthreads();  // win, t and the taps are written again for the block's next plane
  }
}

// LDS bytes of a TH x TW tile, and its derived extents into `a`
size_t tile_lds(FirArgs& a, int TH, int TW) {
  a.TH = TH, a.TW = TW;
  a.wr = (TH - 1) * a.m + a.ny;
  const int wc = (TW - 1) * a.m + a.nx;
  a.ng = (wc + 3 + 3) / 4;  // the window starts up to 3 columns into its first group
  a.pitch = 4 * a.ng + 1;
  a.tp = a.wr | 1;
  return ((size_t)2 * kMaxTaps + (size_t)a.wr * a.pitch + (size_t)TW * a.tp) * sizeof(float);
}

}  // namespace

extern "C" int drs_fir_decimate(const float* x, const float* taps_y, const float* taps_x, const int32_t* band_op, int n_ops,
                                int ntaps_y, int ntaps_x, int Ly, int Lx, int m, const float* noise, const float* sigma,
                                int clamp01, float* out, int n, int c, int H, int W, int h, int w, drs_stream_t stream) {
  DRS_REQUIRE(x && taps_y && taps_x && out, DRS_ERR_ARG, "fir_decimate: null pointer");
  DRS_REQUIRE((noise != nullptr) == (sigma != nullptr), DRS_ERR_ARG, "fir_decimate: noise and sigma go together");
  DRS_REQUIRE(n >= 1 && c >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1, DRS_ERR_SHAPE,
              "fir_decimate: every extent must be >= 1, got n=%d c=%d H=%d W=%d h=%d w=%d", n, c, H, W, h, w);
  DRS_REQUIRE(c <= kMaxBands, DRS_ERR_SHAPE, "fir_decimate: c=%d bands, at most %d", c, kMaxBands);
  DRS_REQUIRE(n_ops >= 1 && n_ops <= c, DRS_ERR_SHAPE, "fir_decimate: n_ops=%d outside 1 .. c=%d", n_ops, c);
  DRS_REQUIRE(m >= 1 && m <= kMaxFactor, DRS_ERR_SHAPE, "fir_decimate: m=%d outside 1 .. %d", m, kMaxFactor);
  DRS_REQUIRE(ntaps_y >= 1 && ntaps_y <= kMaxTaps && ntaps_x >= 1 && ntaps_x <= kMaxTaps, DRS_ERR_SHAPE,
              "fir_decimate: ntaps_y=%d ntaps_x=%d outside 1 .. %d", ntaps_y, ntaps_x, kMaxTaps);
  DRS_REQUIRE(Ly >= 0 && Ly < ntaps_y && Lx >= 0 && Lx < ntaps_x, DRS_ERR_SHAPE,
              "fir_decimate: Ly=%d Lx=%d outside 0 .. ntaps-1 (%d, %d)", Ly, Lx, ntaps_y, ntaps_x);
  DRS_REQUIRE((int64_t)h * m <= H && (int64_t)w * m <= W, DRS_ERR_SHAPE, "fir_decimate: h m = %d x %d > H=%d or w m = %d x %d > W=%d",
              h, m, H, w, m, W);
  const int64_t lim = (int64_t)1 << 31;
  DRS_REQUIRE((int64_t)H * W < lim && (int64_t)n * c < lim, DRS_ERR_SHAPE,
              "fir_decimate: a plane of 2^31 elements or more (H=%d W=%d), or as many planes", H, W);
  FirArgs a = {};
  for (int b = 0; b < c; ++b) {
    const int op = band_op ? band_op[b] : std::min(b, n_ops - 1);
    DRS_REQUIRE(op >= 0 && op < n_ops, DRS_ERR_SHAPE, "fir_decimate: band_op[%d]=%d outside 0 .. n_ops-1=%d", b, op, n_ops - 1);
    a.op[b] = (signed char)op;
  }
  const int64_t planes = (int64_t)n * c;
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)planes * H * W * sizeof(float);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)planes * h * w * sizeof(float);
  DRS_REQUIRE(o1 <= x0 || x1 <= o0, DRS_ERR_ARG, "fir_decimate: x and out overlap");
  a.x = x; a.ky = taps_y; a.kx = taps_x; a.noise = noise; a.sigma = sigma; a.out = out;
  a.planes = (int)planes; a.bands = c; a.H = H; a.W = W; a.h = h; a.w = w;
  a.ny = ntaps_y; a.nx = ntaps_x; a.Ly = Ly; a.Lx = Lx; a.m = m; a.clamp01 = clamp01 != 0;
  a.vec = aligned16(x) && W % 4 == 0;
  static const int kTiles[][2] = {{32, 32}, {16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 2}, {1, 1}};
  size_t bytes = 0;
  for (const auto& t : kTiles) {  // (1, 1): 64 rows of 69 words, 18 KB - the list always ends inside the budget
    bytes = tile_lds(a, t[0], t[1]);
    if (bytes <= kLdsBudget) break;
  }
  DRS_REQUIRE(bytes <= kLdsBudget, DRS_ERR_SHAPE, "fir_decimate: no tile fits the LDS (m=%d, %d x %d taps)", m, ntaps_y, ntaps_x);
  a.tiles_x = drs_cdiv(w, a.TW);
  const int64_t tiles = (int64_t)a.tiles_x * drs_cdiv(h, a.TH);
  DRS_REQUIRE(tiles < lim, DRS_ERR_SHAPE, "fir_decimate: %lld tiles", (long long)tiles);
  DRS_LAUNCH(fir_decimate_kernel, dim3((unsigned)tiles, (unsigned)std::min<int64_t>(planes, 65535)), dim3(kThreads), bytes,
             (hipStream_t)stream, a);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
