// The few-channel image side of the backward: the bicubic adjoint, the 3x3 layers of the LR / SAR encoder and the stem
// convolutions' weight and data gradients (reference UNet_model_superres.py:237-260,:281,:287,:349).  The weight-gradient
// kernels leave per-block partial rows; rows_finish_kernel (colsum.hip) adds them up.
#include "drs_common.h"
#include "train_reduce.h"

// ---------------------------------------------------------------------------------------------------------------
// Adjoint of the bicubic up-sampling (channels-last, C channels; forward: F.interpolate(mode='bicubic'), A = -0.75,
// align_corners=False, source indices clamped at the borders, reference UNet_model_superres.py:349).  GATHER form: one
// thread per element of dx collects the output-gradient pixels whose (clamped) taps land on it - at most 5*scale per
// axis - with the forward's own weights.  No atomics, no zero-fill, deterministic; the scatter form this replaces issued
// 16 float atomics per output element onto 3-channel rows (611 us per configs[2] step).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_w(float t, float c[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
  c[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  c[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  c[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  c[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}
// weight with which output position o (of a size * scale axis) reads source index j (clamped taps summed)
__device__ __forceinline__ float bicubic_adjoint_w(int o, int j, int size, float rs) {
  const float sv = rs * ((float)o + 0.5f) - 0.5f;
  const float fv = floorf(sv);
  float cw[4];
  cubic_w(sv - fv, cw);
  float w = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) w += (min(max((int)fv - 1 + a, 0), size - 1) == j) ? cw[a] : 0.f;
  return w;
}
__global__ __launch_bounds__(256) void bicubic_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int N, int C,
                                                          int H, int W, int scale) {
  const int OH = H * scale, OW = W * scale;
  const long long total = (long long)N * H * W * C;
  const float rs = 1.f / (float)scale;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int xx = (int)((i / C) % W), yy = (int)((i / ((long long)C * W)) % H);
    const int n = (int)(i / ((long long)C * W * H));
    // an output row oy reads source rows floor(sy) - 1 .. floor(sy) + 2 (then clamped): row yy is reached from
    // oy in [(yy - 2) * scale, (yy + 3) * scale); the exact weight (zero for most of that range's ends) decides
    const int oy0 = max((yy - 2) * scale, 0), oy1 = min((yy + 3) * scale, OH);
    const int ox0 = max((xx - 2) * scale, 0), ox1 = min((xx + 3) * scale, OW);
    float acc = 0.f;
    for (int oy = oy0; oy < oy1; ++oy) {
      const float wy = bicubic_adjoint_w(oy, yy, H, rs);
      if (wy == 0.f) continue;
      const float* row = dy + (((long long)n * OH + oy) * OW) * C + c;
      float racc = 0.f;
      for (int ox = ox0; ox < ox1; ++ox) racc = fmaf(bicubic_adjoint_w(ox, xx, W, rs), row[(long long)ox * C], racc);
      acc = fmaf(wy, racc, acc);
    }
    dx[i] = acc;
  }
}
int drs_launch_bicubic_bwd(const float* dy, float* dx, int N, int C, int H, int W, int scale, hipStream_t s) {
  const long long total = (long long)N * H * W * C;
  if (total == 0) return DRS_OK;
  DRS_LAUNCH(bicubic_bwd_kernel, dim3(grid1d(total, 256, 16384)), dim3(256), 0, s, dy, dx, N, C, H, W, scale);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Whole backward of ONE few-channel 3x3 layer of the LR / SAR encoder (reference ResidualBlock / RRDB,
// UNet_model_superres.py:237-260: CC -> CC channels, stride 1, pad 1, CC <= kMaxBands; channels-last tensors, pixel stride CC):
//   dW[co][ci][ky][kx] += sum_p gout[p][co] * in[p + (ky-1, kx-1)][ci]          db[co] += sum_p gout[p][co]
//   gin[p][ci] (+)= sum_{co,ky,kx} W[co][ci][ky][kx] * gout[p - (ky-1, kx-1)][co], then * (mask_y[p][ci] > 0) if mask_y
// (zero outside the image).  The channels go in chunks of KC = min(CC, 4): block row blockIdx.y = (output chunk k, input chunk
// j) owns the KC x KC x 9 (+ KC bias) weight-gradient sums of that pair, one thread per pixel, in registers -> wave shuffles
// -> LDS -> its columns of this block's row of `partials`; rows_finish_kernel adds the rows in a fixed order into dW /
// db.  The k = 0 blocks also form input chunk j of gin, over every output channel in the order co, ky, kx.  With CC <= 4 there
// is one chunk pair and that is the arithmetic of the single-chunk kernel this generalises.  (A first version let the last
// block to arrive add the rows itself: one block summing 256 rows was a 40 us tail on a 25 us kernel.)  Replaces, per layer, a
// weight-gradient launch of the MFMA kernel on the side stream (35 us + a 50 us reduce for 81 sums) that the main stream had
// to wait for, a weight re-pack, a direct tap convolution and a mask pass: the seven layers were 0.9 ms of a 16.5 ms training
// step spent almost idle.
// ---------------------------------------------------------------------------------------------------------------
template <int CC>
__global__ __launch_bounds__(256) void small_conv_bwd_kernel(const float* __restrict__ in, const float* __restrict__ gout,
                                                             const float* __restrict__ w, float* __restrict__ gin,
                                                             int accumulate, const float* __restrict__ mask_y, int N, int H,
                                                             int W, float* __restrict__ partials, const float* dW,
                                                             const float* db) {
  constexpr int KC = CC < 4 ? CC : 4, NCH = (CC + KC - 1) / KC;  // chunk width, chunks per side
  constexpr int NW = KC * KC * 9, NACC = NW + KC, NCOL = CC * CC * 9 + CC;
  __shared__ float red[4][NACC];
  const int k = blockIdx.y / NCH, j = blockIdx.y % NCH;  // output chunk, input chunk (block-uniform)
  const int co0 = k * KC, ci0 = j * KC;
  const long long npix = (long long)N * H * W;
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) {
    const int x = (int)(p % W), y = (int)((p / W) % H);
    float go[3][3][KC], xi[3][3][KC];  // gout: output chunk kk of the gin loop below; in: input chunk j
    auto load_go = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int yy = y + ky - 1, xx = x + kx - 1;
          const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
          const long long q = (p + (long long)(ky - 1) * W + (kx - 1)) * CC + c0;
#pragma unroll
          for (int c = 0; c < KC; ++c) go[ky][kx][c] = ok && c0 + c < CC ? gout[q + c] : 0.f;
        }
    };
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const long long q = (p + (long long)(ky - 1) * W + (kx - 1)) * CC + ci0;
#pragma unroll
        for (int c = 0; c < KC; ++c) xi[ky][kx][c] = ok && ci0 + c < CC ? in[q + c] : 0.f;
      }
    load_go(co0);
#pragma unroll
    for (int co = 0; co < KC; ++co) {
      acc[NW + co] += go[1][1][co];
#pragma unroll
      for (int ci = 0; ci < KC; ++ci)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) acc[((co * KC + ci) * 3 + ky) * 3 + kx] += go[1][1][co] * xi[ky][kx][ci];
    }
    if (k != 0) continue;  // (block-uniform)
    float o[KC];
#pragma unroll
    for (int ci = 0; ci < KC; ++ci) o[ci] = accumulate && ci0 + ci < CC ? gin[p * CC + ci0 + ci] : 0.f;
#pragma unroll 1
    for (int kk = 0; kk < NCH; ++kk) {  // (a loop: the weights of one output chunk at a time, not all of W, stay in registers)
      if (kk > 0) load_go(kk * KC);
#pragma unroll
      for (int co = 0; co < KC; ++co) {
        if (kk * KC + co >= CC) break;
#pragma unroll
        for (int ci = 0; ci < KC; ++ci) {
          if (ci0 + ci >= CC) break;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
              o[ci] += w[(((kk * KC + co) * CC + ci0 + ci) * 3 + ky) * 3 + kx] * go[2 - ky][2 - kx][co];  // (launch-uniform: scalar loads)
        }
      }
    }
#pragma unroll
    for (int ci = 0; ci < KC; ++ci) {
      if (ci0 + ci >= CC) break;
      if (mask_y && !(mask_y[p * CC + ci0 + ci] > 0.f)) o[ci] = 0.f;
      gin[p * CC + ci0 + ci] = o[ci];
    }
  }
  if (!dW && !db) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    float v = acc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= NACC) return;
  int col;
  if (i < NW) {  // ((co0 + co) * CC + ci0 + ci) * 9 + t
    const int co = i / (KC * 9), ci = (i / 9) % KC, t = i % 9;
    if (co0 + co >= CC || ci0 + ci >= CC) return;
    col = ((co0 + co) * CC + ci0 + ci) * 9 + t;
  } else {  // bias sums: written by the j = 0 blocks
    if (j != 0 || co0 + i - NW >= CC) return;
    col = CC * CC * 9 + co0 + i - NW;
  }
  partials[(size_t)blockIdx.x * NCOL + col] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}
// one instantiation per band count (1 .. kMaxBands) of a few-channel template kernel
#define DRS_BANDS_SWITCH(n, X)                                                                                              \
  switch (n) {                                                                                                              \
    case 1: X(1); break; case 2: X(2); break; case 3: X(3); break; case 4: X(4); break; case 5: X(5); break;               \
    case 6: X(6); break; case 7: X(7); break; case 8: X(8); break; case 9: X(9); break; case 10: X(10); break;             \
    case 11: X(11); break; case 12: X(12); break; case 13: X(13); break; case 14: X(14); break; case 15: X(15); break;      \
    default: X(16); break;                                                                                                  \
  }
static_assert(kMaxBands == 16, "DRS_BANDS_SWITCH instantiates 1 .. 16");
int drs_launch_small_conv_bwd(const float* in, const float* gout, const float* w, float* gin, int accumulate,
                              const float* mask_y, int N, int CC, int H, int W, float* partials, size_t partial_bytes,
                              float* dW, float* db, hipStream_t s) {
  DRS_REQUIRE(CC >= 1 && CC <= kMaxBands, DRS_ERR_SHAPE, "small_conv_bwd: CC=%d (1..%d)", CC, kMaxBands);
  const long long npix = (long long)N * H * W;
  if (npix == 0) return DRS_OK;
  const unsigned blocks = grid1d(npix, 256, 1024);  // <= 1024 partial rows of 9 CC^2 + CC floats
  const int ncol = 9 * CC * CC + CC, nch = (CC + 3) / 4;
  DRS_REQUIRE(!(dW || db) || partial_bytes >= (size_t)blocks * ncol * 4, DRS_ERR_WORKSPACE,
              "small_conv_bwd: partial workspace too small");
#define DRS_SCB(K) DRS_LAUNCH(small_conv_bwd_kernel<K>, dim3(blocks, nch * nch), dim3(256), 0, s, in, gout, w, gin, accumulate, \
                              mask_y, N, H, W, partials, dW, db)
  DRS_BANDS_SWITCH(CC, DRS_SCB)
#undef DRS_SCB
  if (dW || db) return drs_launch_rows_finish(partials, (int)blocks, ncol, 9 * CC * CC, dW, db, s);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Weight + bias gradient of a stem convolution (3x3, pad 1, CI <= kMaxBands image-like channels -> 16; reference conv0 /
// conv_upsampled_lr_img, UNet_model_superres.py:281,287):
//   dW[co][ci][ky][kx] += sum_p g[p][co] * x[p + (ky-1, kx-1)][ci]      db[co] += sum_p g[p][co]
// g: channels-last, pixel stride g_cs (16 used); x: channels-last, CI channels.  Block row blockIdx.y = input chunk j of
// KC = min(CI, 4) channels; wave w of a block owns output channels 4w .. 4w+3 for 64 pixels per pass: 36 KC + 4 sums per lane
// in registers over the block's pixels, one shuffle reduction at the end, lane 0 writes the wave's columns of the block's
// partial row (column = flat dW index, then the 16 bias sums, those from the j = 0 blocks); rows_finish_kernel adds the
// rows in a fixed order.  The MFMA weight-gradient kernel spent 230 us + a 35 - 90 us slice reduction per layer on these 432
// sums (scalar staging of a 3-channel operand into 16-wide tiles).
// ---------------------------------------------------------------------------------------------------------------
template <int CI>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ g, int g_cs, const float* __restrict__ x,
                                                         int N, int H, int W, float* __restrict__ partials) {
  constexpr int KC = CI < 4 ? CI : 4;
  constexpr int NW = 4 * KC * 9, NACC = NW + 4, NCOL = 16 * CI * 9 + 16;
  const int lane = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const int ci0 = blockIdx.y * KC;
  const long long npix = (long long)N * H * W;
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  for (long long p = (long long)blockIdx.x * 64 + lane; p < npix; p += (long long)gridDim.x * 64) {
    const int xx = (int)(p % W), yy = (int)((p / W) % H);
    const float4 gv4 = *reinterpret_cast<const float4*>(g + p * g_cs + cg * 4);
    const float gv[4] = {gv4.x, gv4.y, gv4.z, gv4.w};
    float xi[9][KC];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int y2 = yy + ky - 1, x2 = xx + kx - 1;
        const bool ok = y2 >= 0 && y2 < H && x2 >= 0 && x2 < W;
        const long long q = (p + (long long)(ky - 1) * W + (kx - 1)) * CI + ci0;
#pragma unroll
        for (int c = 0; c < KC; ++c) xi[ky * 3 + kx][c] = ok && ci0 + c < CI ? x[q + c] : 0.f;
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[NW + j] += gv[j];
#pragma unroll
      for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[(j * KC + c) * 9 + t] += gv[j] * xi[t][c];
    }
  }
  float* row = partials + (size_t)blockIdx.x * NCOL;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    float v = acc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) {
      if (i < NW) {  // ((4 cg + j) * CI + ci0 + c) * 9 + t
        const int j = i / (KC * 9), c = (i / 9) % KC, t = i % 9;
        if (ci0 + c < CI) row[((4 * cg + j) * CI + ci0 + c) * 9 + t] = v;
      } else if (blockIdx.y == 0) {
        row[16 * CI * 9 + cg * 4 + (i - NW)] = v;
      }
    }
  }
}
int drs_launch_stem_wgrad(const float* g, int g_cs, const float* x, int N, int CI, int H, int W, float* partials,
                          size_t partial_bytes, float* dW, float* db, hipStream_t s) {
  DRS_REQUIRE(CI >= 1 && CI <= kMaxBands && (g_cs & 3) == 0, DRS_ERR_SHAPE, "stem_wgrad: CI=%d g_cs=%d", CI, g_cs);
  const long long npix = (long long)N * H * W;
  if (npix == 0 || (!dW && !db)) return DRS_OK;
  const int ncol = 16 * CI * 9 + 16;
  const unsigned blocks = grid1d(npix, 64, 512);
  DRS_REQUIRE(partial_bytes >= (size_t)blocks * ncol * 4, DRS_ERR_WORKSPACE, "stem_wgrad: partial workspace too small");
#define DRS_SWG(K) DRS_LAUNCH(stem_wgrad_kernel<K>, dim3(blocks, (K + 3) / 4), dim3(256), 0, s, g, g_cs, x, N, H, W, partials)
  DRS_BANDS_SWITCH(CI, DRS_SWG)
#undef DRS_SWG
  return drs_launch_rows_finish(partials, (int)blocks, ncol, 16 * CI * 9, dW, db, s);
}

// ---------------------------------------------------------------------------------------------------------------
// Data gradient of a stem convolution (3x3, pad 1, C <= kMaxBands image-like channels -> 16; reference conv_upsampled_lr_img /
// conv0, UNet_model_superres.py:281,287):  dx[n][y][x][c] = sum_{ky,kx,o} g[n][y+1-ky][x+1-kx][o] * w[o][c][ky][kx], zero
// outside the image.  Block = 16 x 16 pixels; the 18 x 18 x 16 tile of g goes through LDS once (the direct tap kernel this
// replaces re-read every pixel's 16 channels for each of the 9 taps from L1 / L2: 610 us per configs[2] step for a
// 3-channel result).  Up to kMaxBands accumulators, the 4-wide groups past C skipped; each sums in the order ky, kx, o.
// g: channels-last with pixel stride g_cs (16 used); w: the layer's own (16, C, 3, 3) parameter.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const float* __restrict__ g, int g_cs, const float* __restrict__ w,
                                                         float* __restrict__ dx, int H, int W, int C) {
  constexpr int kC = kMaxBands;
  __shared__ float sg[18 * 18][17];   // (+1: a lane's 16-float rows start in different banks)
  __shared__ float sw[16 * kC * 9];   // [o][c (padded to kC)][tap]
  const int n = blockIdx.z, y0 = blockIdx.y * 16, x0 = blockIdx.x * 16;
  const int cpad = (C + 3) & ~3;      // channels rounded up to the 4-wide chunks (the padding weights are zero)
  for (int i = threadIdx.x; i < 16 * cpad * 9; i += 256) {
    const int tap = i % 9, c = (i / 9) % cpad, o = i / (9 * cpad);
    sw[(o * kC + c) * 9 + tap] = c < C ? w[(o * C + c) * 9 + tap] : 0.f;
  }
  for (int i = threadIdx.x; i < 18 * 18 * 4; i += 256) {  // one float4 (4 of the 16 channels) per step
    const int q = i & 3, pix = i >> 2;
    const int py = pix / 18, px = pix - py * 18;
    const int y = y0 - 1 + py, x = x0 - 1 + px;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y >= 0 && y < H && x >= 0 && x < W)
      v = *reinterpret_cast<const float4*>(g + (((long long)n * H + y) * W + x) * g_cs + q * 4);
    sg[pix][q * 4] = v.x; sg[pix][q * 4 + 1] = v.y; sg[pix][q * 4 + 2] = v.z; sg[pix][q * 4 + 3] = v.w;
  }
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int y = y0 + ty, x = x0 + tx;
  if (y >= H || x >= W) return;
  float acc[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) acc[c] = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const float* gp = sg[(ty + 2 - ky) * 18 + (tx + 2 - kx)];  // g at (y + 1 - ky, x + 1 - kx)
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        const float gv = gp[o];
#pragma unroll
        for (int c0 = 0; c0 < kC; c0 += 4) {
          if (c0 >= cpad) break;  // (launch-uniform)
#pragma unroll
          for (int c = c0; c < c0 + 4; ++c) acc[c] = fmaf(gv, sw[(o * kC + c) * 9 + ky * 3 + kx], acc[c]);
        }
      }
    }
  float* out = dx + (((long long)n * H + y) * W + x) * C;
#pragma unroll
  for (int c = 0; c < kC; ++c)
    if (c < C) out[c] = acc[c];
}
int drs_launch_stem_dgrad(const float* g, int g_cs, const float* w, float* dx, int N, int H, int W, int C, hipStream_t s) {
  DRS_REQUIRE(C >= 1 && C <= kMaxBands && (g_cs & 3) == 0 && g_cs >= 16, DRS_ERR_SHAPE, "stem_dgrad: C=%d g_cs=%d", C, g_cs);
  if ((long long)N * H * W == 0) return DRS_OK;
  DRS_LAUNCH(stem_dgrad_kernel, dim3((W + 15) / 16, (H + 15) / 16, N), dim3(256), 0, s, g, g_cs, w, dx, H, W, C);
  DRS_CHECK_HIP(hipGetLastError());
  return DRS_OK;
}
