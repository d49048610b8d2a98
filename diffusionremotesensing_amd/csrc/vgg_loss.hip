// VGG19 perceptual loss of the MSE+Perceptual_noise training loss (reference train_diffusion_superres.py:25-63):
//   vgg(x, y) = mean((F(P(x)) - F(P(y)))^2),  P = bicubic resize to 224 x 224 (only when width != 224) + ImageNet normalise,
//   F = torchvision vgg19().features (16 x [3x3 conv + ReLU], 5 x MaxPool2d(2, 2)).
// Prediction and target go through ONE batched forward of 2B images (same kernels, so both sides carry the same rounding);
// the backward runs on the prediction half only and ends in d(loss)/d(pred).
//
// Per forward:   prep (bicubic + normalise, NHWC padded to 4 channels) -> 16 tap convolutions on the MFMA family (bias + ReLU
//                in the epilogue) with 5 NHWC max-pools -> two-stage loss reduction into a device scalar.
// Per backward:  gradient seed 2 (fx - fy) / numel * g  ->  per layer: pool backward with the ReLU mask fused (layers in
//                front of a pool) or a ReLU mask pass, then the data-gradient convolution (flipped, transposed packed
//                weights) -> normalisation adjoint (1/std) -> separable bicubic adjoint over host-built transpose tap tables.
// Nothing here uses atomics: every reduction has a fixed order, so two identical calls give identical bits.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "drs_common.h"

namespace {

constexpr int kConvs = 16;
constexpr int kCfg[kConvs] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512};
// the layers a MaxPool2d follows (torchvision cfg "E": 64,64,M,128,128,M,256x4,M,512x4,M,512x4,M)
constexpr bool pool_after(int l) { return l == 1 || l == 3 || l == 7 || l == 11 || l == 15; }
constexpr int level_of(int l) { return l < 2 ? 0 : l < 4 ? 1 : l < 8 ? 2 : l < 12 ? 3 : 4; }
constexpr int cin_of(int l) { return l == 0 ? 3 : kCfg[l - 1]; }
constexpr int kRedBlocks = 256;  // stage-1 blocks of the loss reduction (fixed: the summation order never changes)
__constant__ float kMean[3] = {0.485f, 0.456f, 0.406f};  // torchvision ImageNet statistics (reference :43)
__constant__ float kStd[3] = {0.229f, 0.224f, 0.225f};

inline size_t align_up(size_t v) { return (v + 255) / 256 * 256; }
inline unsigned grid_for(long long total, int per_block = 256, long long cap = 16384) {
  long long b = (total + per_block - 1) / per_block;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

// ---- ATen upsample_bicubic2d (align_corners=False, no antialias) as per-axis tap tables ------------------------------------
//   src = scale * (dst + 0.5) - 0.5 with scale = in / out and no clamping of src; taps floor(src) - 1 .. + 2 clamped to
//   [0, in - 1]; weights: cubic convolution with A = -0.75 (aten/src/ATen/native/UpSample.h).
double cubic1(double x, double A) { return ((A + 2) * x - (A + 3)) * x * x + 1; }
double cubic2(double x, double A) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; }
void bicubic_taps(int in, int out, std::vector<int>& idx, std::vector<float>& w) {
  idx.resize((size_t)out * 4);
  w.resize((size_t)out * 4);
  const double A = -0.75, scale = (double)in / out;
  for (int o = 0; o < out; ++o) {
    const double src = scale * (o + 0.5) - 0.5;
    const double f = floor(src), t = src - f;
    const double c[4] = {cubic2(t + 1, A), cubic1(t, A), cubic1(1 - t, A), cubic2(2 - t, A)};
    for (int k = 0; k < 4; ++k) {
      int i = (int)f - 1 + k;
      i = i < 0 ? 0 : (i > in - 1 ? in - 1 : i);
      idx[(size_t)o * 4 + k] = i;
      w[(size_t)o * 4 + k] = (float)c[k];
    }
  }
}
// transpose of one axis: for input index i, the (output index, weight) pairs of every forward tap that lands on i, in
// (output, tap) order - a gather with a fixed order instead of a scatter
void transpose_taps(int in, int out, const std::vector<int>& idx, const std::vector<float>& w, std::vector<int>& offs,
                    std::vector<int>& tidx, std::vector<float>& tw) {
  offs.assign((size_t)in + 1, 0);
  for (int e = 0; e < out * 4; ++e) ++offs[(size_t)idx[e] + 1];
  for (int i = 0; i < in; ++i) offs[(size_t)i + 1] += offs[i];
  std::vector<int> fill(offs.begin(), offs.end() - 1);
  tidx.resize((size_t)out * 4);
  tw.resize((size_t)out * 4);
  for (int e = 0; e < out * 4; ++e) {
    const int p = fill[idx[e]]++;
    tidx[p] = e / 4;
    tw[p] = w[e];
  }
}

// ---- kernels -------------------------------------------------------------------------------------------------------------
// prep: out[n][y][x][0..3] = (resize(img)[c][y][x] - mean[c]) / std[c], channel 3 = 0.  n < B: pred[n], else target[n - B].
// ty / tx: 4 forward taps per output row / column (resize == 0: identity, the input is already H0 x W0).
__global__ void vgg_prep_kernel(const float* __restrict__ pred, const float* __restrict__ target, int B, int H, int W,
                                int H0, int W0, int resize, const int* __restrict__ ty_i, const float* __restrict__ ty_w,
                                const int* __restrict__ tx_i, const float* __restrict__ tx_w, float4* __restrict__ out) {
  const long long total = 2LL * B * H0 * W0;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(p % W0);
    const int y = (int)((p / W0) % H0);
    const int n = (int)(p / ((long long)W0 * H0));
    const float* img = n < B ? pred + (size_t)n * 3 * H * W : target + (size_t)(n - B) * 3 * H * W;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* plane = img + (size_t)c * H * W;
      float r;
      if (resize) {
        // ATen's order: interpolate each of the 4 source rows along x, then the 4 row values along y
        float rows[4];
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
          const float* row = plane + (size_t)ty_i[y * 4 + ky] * W;
          rows[ky] = row[tx_i[x * 4 + 0]] * tx_w[x * 4 + 0] + row[tx_i[x * 4 + 1]] * tx_w[x * 4 + 1] +
                     row[tx_i[x * 4 + 2]] * tx_w[x * 4 + 2] + row[tx_i[x * 4 + 3]] * tx_w[x * 4 + 3];
        }
        r = rows[0] * ty_w[y * 4 + 0] + rows[1] * ty_w[y * 4 + 1] + rows[2] * ty_w[y * 4 + 2] + rows[3] * ty_w[y * 4 + 3];
      } else {
        r = plane[(size_t)y * W + x];
      }
      v[c] = (r - kMean[c]) / kStd[c];  // torchvision Normalize: sub_(mean).div_(std)
    }
    out[p] = make_float4(v[0], v[1], v[2], 0.f);
  }
}

// MaxPool2d(2, 2) on NHWC, floor sizes.  ATen's scan: the first maximum in window order wins, a NaN always wins.
__device__ __forceinline__ int pool_pick(float a0, float a1, float a2, float a3) {
  float m = a0; int k = 0;
  if (a1 > m || isnan(a1)) { m = a1; k = 1; }
  if (a2 > m || isnan(a2)) { m = a2; k = 2; }
  if (a3 > m || isnan(a3)) { m = a3; k = 3; }
  return k;
}
__global__ void vgg_pool_fwd_kernel(const float4* __restrict__ in, float4* __restrict__ out, int N, int H, int W, int C4) {
  const int OH = H >> 1, OW = W >> 1;
  const long long total = (long long)N * OH * OW * C4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    long long r = i / C4;
    const int ox = (int)(r % OW); r /= OW;
    const int oy = (int)(r % OH);
    const int n = (int)(r / OH);
    const float4* p = in + (((size_t)n * H + 2 * oy) * W + 2 * ox) * C4 + c;
    const float4 a = p[0], b = p[C4], d = p[(size_t)W * C4], e = p[(size_t)W * C4 + C4];
    const float av[4][4] = {{a.x, b.x, d.x, e.x}, {a.y, b.y, d.y, e.y}, {a.z, b.z, d.z, e.z}, {a.w, b.w, d.w, e.w}};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = av[j][pool_pick(av[j][0], av[j][1], av[j][2], av[j][3])];
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}
// pool backward + the ReLU in front of it: gin[n][y][x][c] = (argmax of its window is (y, x) ? gout : 0), zeroed where the
// saved ReLU output y <= 0 (torch's threshold_backward); rows / columns the floor drops get 0
__global__ void vgg_pool_bwd_kernel(const float4* __restrict__ gout, const float4* __restrict__ y, float4* __restrict__ gin,
                                    int N, int H, int W, int C4) {
  const int OH = H >> 1, OW = W >> 1;
  const long long total = (long long)N * H * W * C4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    long long r = i / C4;
    const int x = (int)(r % W); r /= W;
    const int yy = (int)(r % H);
    const int n = (int)(r / H);
    const int oy = yy >> 1, ox = x >> 1;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (oy < OH && ox < OW) {
      const float4* p = y + (((size_t)n * H + 2 * oy) * W + 2 * ox) * C4 + c;
      const float4 a = p[0], b = p[C4], d = p[(size_t)W * C4], e = p[(size_t)W * C4 + C4];
      const float4 go = gout[(((size_t)n * OH + oy) * OW + ox) * C4 + c];
      const float4 me = y[i];
      const int k = ((yy & 1) << 1) | (x & 1);
      g.x = (pool_pick(a.x, b.x, d.x, e.x) == k && !(me.x <= 0.f)) ? go.x : 0.f;
      g.y = (pool_pick(a.y, b.y, d.y, e.y) == k && !(me.y <= 0.f)) ? go.y : 0.f;
      g.z = (pool_pick(a.z, b.z, d.z, e.z) == k && !(me.z <= 0.f)) ? go.z : 0.f;
      g.w = (pool_pick(a.w, b.w, d.w, e.w) == k && !(me.w <= 0.f)) ? go.w : 0.f;
    }
    gin[i] = g;
  }
}
// ReLU backward in place: g = 0 where the saved output y <= 0
__global__ void vgg_relu_mask_kernel(float4* __restrict__ g, const float4* __restrict__ y, long long n4) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 v = g[i];
    const float4 m = y[i];
    if (m.x <= 0.f) v.x = 0.f;
    if (m.y <= 0.f) v.y = 0.f;
    if (m.z <= 0.f) v.z = 0.f;
    if (m.w <= 0.f) v.w = 0.f;
    g[i] = v;
  }
}

// loss, stage 1: block b sums (fx - fy)^2 over the fixed grid-stride set of elements it owns (fp64), fixed tree in LDS
__global__ __launch_bounds__(256) void vgg_loss_partial_kernel(const float* __restrict__ f, long long numel,
                                                               double* __restrict__ partial) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < numel; i += (long long)kRedBlocks * 256) {
    const double d = (double)f[i] - (double)f[i + numel];
    s += d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
// stage 2: one block, kRedBlocks partials in a fixed tree; loss = sum / numel
__global__ __launch_bounds__(256) void vgg_loss_final_kernel(const double* __restrict__ partial, long long numel,
                                                             float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < kRedBlocks; i += 256) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)numel);
}
// gradient seed: dF = 2 (fx - fy) / numel * g, g = the autograd upstream scalar (device pointer: no host sync)
__global__ void vgg_seed_kernel(const float* __restrict__ f, long long numel, const float* __restrict__ g,
                                float* __restrict__ df) {
  const float sc = (float)(2.0 / (double)numel) * g[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x)
    df[i] = (f[i] - f[i + numel]) * sc;
}
// normalisation adjoint: dp[n][c][y][x] = dx0[n][y][x][c] / std[c] (dx0: the first layer's data gradient, pixel stride cs)
__global__ void vgg_norm_bwd_kernel(const float* __restrict__ dx0, int cs, float* __restrict__ dp, int B, int H0, int W0) {
  const long long total = (long long)B * 3 * H0 * W0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % W0);
    long long r = i / W0;
    const int y = (int)(r % H0); r /= H0;
    const int c = (int)(r % 3);
    const int n = (int)(r / 3);
    dp[i] = dx0[(((size_t)n * H0 + y) * W0 + x) * cs + c] / kStd[c];
  }
}
// bicubic adjoint along x: t[p][ix] = sum over the transpose taps of column ix of w * dp[p][ox]   (p = one (n, c, row) line)
__global__ void vgg_bicubic_bwd_x_kernel(const float* __restrict__ dp, float* __restrict__ t, long long lines, int W0, int W,
                                         const int* __restrict__ offs, const int* __restrict__ oi, const float* __restrict__ ow) {
  const long long total = lines * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ix = (int)(i % W);
    const float* src = dp + (i / W) * W0;
    float s = 0.f;
    for (int e = offs[ix]; e < offs[ix + 1]; ++e) s += ow[e] * src[oi[e]];
    t[i] = s;
  }
}
// ... and along y: dx[nc][iy][ix] = sum over the transpose taps of row iy of w * t[nc][oy][ix]
__global__ void vgg_bicubic_bwd_y_kernel(const float* __restrict__ t, float* __restrict__ dx, int planes, int H0, int H, int W,
                                         const int* __restrict__ offs, const int* __restrict__ oi, const float* __restrict__ ow) {
  const long long total = (long long)planes * H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int ix = (int)(i % W);
    const int iy = (int)((i / W) % H);
    const float* src = t + (i / ((long long)W * H)) * H0 * W + ix;
    float s = 0.f;
    for (int e = offs[iy]; e < offs[iy + 1]; ++e) s += ow[e] * src[(size_t)oi[e] * W];
    dx[i] = s;
  }
}

}  // namespace

// ---- plan -----------------------------------------------------------------------------------------------------------------
struct drs_vgg_plan {
  int B, H, W, impl;
  int H0, W0, resize;
  int LH[5], LW[5];  // spatial size of each level (conv outputs of that level)
  // packed buffer: per layer forward image + bias, data-gradient image; bicubic tables
  size_t o_wf[kConvs], o_bf[kConvs], o_wd[kConvs], packed_bytes;
  size_t o_ty_i, o_ty_w, o_tx_i, o_tx_w;                      // forward taps (4 per output row / column)
  size_t o_rx_off, o_rx_i, o_rx_w, o_ry_off, o_ry_i, o_ry_w;  // transpose taps
  std::vector<int> ty_i, tx_i, rx_off, rx_i, ry_off, ry_i;
  std::vector<float> ty_w, tx_w, rx_w, ry_w;
  // workspace
  size_t o_x0, o_act[2], o_feat, o_part, o_save[kConvs], o_g[2], o_dp, o_t, ws_bytes;
  const void* packed_ptr = nullptr;
  bool packed_ok = false;
  int saved = 0;  // 1: the workspace holds the activations of a forward with save = 1 (what backward needs)
  // optional per-op timing
  struct OpRec { std::string name; double flops; hipEvent_t e0, e1; };
  bool prof = false;
  std::vector<OpRec> ops;
  size_t nops = 0;
};

static TapConv vgg_conv(const float* in, int N, int H, int W, int Cin, const void* w, const float* bias, float* out, int Cout) {
  TapConv d = {};
  d.in = in; d.in_cs = Cin; d.in_co = 0;
  d.N = N; d.H = H; d.W = W; d.Cin = Cin;
  d.w = (const float*)w; d.bias = bias;
  d.out = out; d.out_cs = Cout; d.out_co = 0;
  d.OH = H; d.OW = W; d.Cout = Cout; d.TH = H; d.TW = W;
  d.in_stride = 1; d.out_scale = 1;
  d.ntaps = 9; d.wtaps_total = 9;
  for (int i = 0; i < 9; ++i) { d.dy[i] = i / 3 - 1; d.dx[i] = i % 3 - 1; d.wtap[i] = i; }
  return d;
}
// channels of the tensors the convolutions read / write: the prep output is padded to 4, the first layer's data gradient to
// the 32-channel MFMA tile (zero weights)
static inline int fwd_cin(int l) { return l == 0 ? 4 : cin_of(l); }
static inline int dgrad_cout(int l) { return l == 0 ? 32 : cin_of(l); }

namespace {
struct OpScope {  // per-op events of a profiled call
  drs_vgg_plan* p; hipStream_t s; size_t i;
  OpScope(drs_vgg_plan* p_, hipStream_t s_, const char* name, double flops) : p(p_), s(s_), i(0) {
    if (!p->prof) return;
    if (p->nops == p->ops.size()) {
      drs_vgg_plan::OpRec r{name, flops, nullptr, nullptr};
      (void)hipEventCreate(&r.e0);
      (void)hipEventCreate(&r.e1);
      p->ops.push_back(r);
    }
    i = p->nops++;
    p->ops[i].name = name;
    p->ops[i].flops = flops;
    (void)hipEventRecord(p->ops[i].e0, s);
  }
  ~OpScope() {
    if (p->prof) (void)hipEventRecord(p->ops[i].e1, s);
  }
};
}  // namespace

extern "C" int drs_vgg_plan_create(drs_vgg_plan** out, int batch, int height, int width, int impl) {
  DRS_REQUIRE(out, DRS_ERR_ARG, "vgg_plan_create: null pointer");
  *out = nullptr;
  DRS_REQUIRE(impl == DRS_IMPL_MFMA_F32 || impl == DRS_IMPL_MFMA_BF16X3, DRS_ERR_ARG,
              "vgg_plan_create: impl must be DRS_IMPL_MFMA_F32 or DRS_IMPL_MFMA_BF16X3");
  DRS_REQUIRE(batch >= 1 && height >= 1 && width >= 1, DRS_ERR_SHAPE, "vgg_plan_create: empty input");
  drs_vgg_plan* p = new drs_vgg_plan();
  p->B = batch; p->H = height; p->W = width; p->impl = impl;
  p->resize = width != 224;  // the reference tests the width only (train_diffusion_superres.py:47)
  p->H0 = p->resize ? 224 : height;
  p->W0 = 224;
  for (int v = 0; v < 5; ++v) { p->LH[v] = p->H0 >> v; p->LW[v] = p->W0 >> v; }
  if ((p->H0 >> 5) < 1 || (size_t)2 * batch * p->H0 * p->W0 * 64 * 4 >= (1ull << 31)) {
    delete p;
    DrsErr::set("vgg_plan_create: %d x %d input gives an empty feature map, or batch %d too large", height, width, batch);
    return DRS_ERR_SHAPE;
  }
  // every layer (forward and data gradient) must run on the MFMA family: no silent fall-back to the direct kernels
  static const float dummy = 0.f;
  for (int l = 0; l < kConvs; ++l) {
    const int v = level_of(l);
    TapConv f = vgg_conv(&dummy, 2 * batch, p->LH[v], p->LW[v], fwd_cin(l), &dummy, &dummy, (float*)&dummy, kCfg[l]);
    f.relu_pre = 1;
    TapConv g = vgg_conv(&dummy, batch, p->LH[v], p->LW[v], kCfg[l], &dummy, nullptr, (float*)&dummy, dgrad_cout(l));
    if (!drs_tapconv_mfma_supported(f, impl) || !drs_tapconv_mfma_supported(g, impl)) {
      DrsErr::set("vgg_plan_create: layer %d (%d -> %d channels at %d x %d) has no MFMA kernel", l, cin_of(l), kCfg[l],
                  p->LH[v], p->LW[v]);
      delete p;
      return DRS_ERR_SHAPE;
    }
  }
  // packed buffer
  size_t cur = 0;
  for (int l = 0; l < kConvs; ++l) {
    p->o_wf[l] = cur; cur += align_up(drs_pack_conv_mfma_bytes(kCfg[l], fwd_cin(l), 9, impl));
    p->o_bf[l] = cur; cur += align_up((size_t)kCfg[l] * 4);
    p->o_wd[l] = cur; cur += align_up(drs_pack_conv_mfma_bytes(dgrad_cout(l), kCfg[l], 9, impl));
  }
  if (p->resize) {
    bicubic_taps(height, p->H0, p->ty_i, p->ty_w);
    bicubic_taps(width, p->W0, p->tx_i, p->tx_w);
    transpose_taps(width, p->W0, p->tx_i, p->tx_w, p->rx_off, p->rx_i, p->rx_w);
    transpose_taps(height, p->H0, p->ty_i, p->ty_w, p->ry_off, p->ry_i, p->ry_w);
  }
  auto tab = [&](size_t n) { const size_t o = cur; cur += align_up(n * 4); return o; };
  p->o_ty_i = tab(p->ty_i.size()); p->o_ty_w = tab(p->ty_w.size());
  p->o_tx_i = tab(p->tx_i.size()); p->o_tx_w = tab(p->tx_w.size());
  p->o_rx_off = tab(p->rx_off.size()); p->o_rx_i = tab(p->rx_i.size()); p->o_rx_w = tab(p->rx_w.size());
  p->o_ry_off = tab(p->ry_off.size()); p->o_ry_i = tab(p->ry_i.size()); p->o_ry_w = tab(p->ry_w.size());
  p->packed_bytes = cur;
  // workspace
  const size_t B = batch, H0 = p->H0, W0 = p->W0;
  cur = 0;
  p->o_x0 = cur; cur += align_up(2 * B * H0 * W0 * 4 * 4);
  for (int i = 0; i < 2; ++i) { p->o_act[i] = cur; cur += align_up(2 * B * H0 * W0 * 64 * 4); }
  p->o_feat = cur; cur += align_up(2 * B * (size_t)(p->LH[4] >> 1) * (p->LW[4] >> 1) * 512 * 4);
  p->o_part = cur; cur += align_up(kRedBlocks * 8);
  for (int l = 0; l < kConvs; ++l) {
    const int v = level_of(l);
    p->o_save[l] = cur; cur += align_up(B * p->LH[v] * p->LW[v] * kCfg[l] * 4);
  }
  for (int i = 0; i < 2; ++i) { p->o_g[i] = cur; cur += align_up(B * H0 * W0 * 64 * 4); }
  p->o_dp = cur; cur += align_up(B * 3 * H0 * W0 * 4);
  p->o_t = cur; cur += align_up(B * 3 * H0 * (size_t)width * 4);
  p->ws_bytes = cur;
  *out = p;
  return DRS_OK;
}

extern "C" void drs_vgg_plan_destroy(drs_vgg_plan* plan) {
  if (!plan) return;
  for (auto& r : plan->ops) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  delete plan;
}
extern "C" size_t drs_vgg_packed_bytes(const drs_vgg_plan* plan) { return plan ? plan->packed_bytes + 256 : 0; }
extern "C" size_t drs_vgg_workspace_bytes(const drs_vgg_plan* plan) { return plan ? plan->ws_bytes + 256 : 0; }

static char* base256(const void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

extern "C" int drs_vgg_pack_weights(drs_vgg_plan* plan, const void* const* params, void* packed, size_t packed_bytes,
                                    drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(plan && params && packed, DRS_ERR_ARG, "vgg_pack_weights: null pointer");
  DRS_REQUIRE(packed_bytes >= drs_vgg_packed_bytes(plan), DRS_ERR_WORKSPACE, "vgg_pack_weights: packed buffer too small");
  for (int i = 0; i < 2 * kConvs; ++i) DRS_REQUIRE(params[i], DRS_ERR_ARG, "vgg_pack_weights: parameter %d is null", i);
  char* pk = base256(packed);
  plan->packed_ok = false;
  {
    DrsPackQueueScope queue;
    for (int l = 0; l < kConvs; ++l) {
      const float* w = (const float*)params[2 * l];
      const float* b = (const float*)params[2 * l + 1];
      // forward: (Cout, Cin, 3, 3); the first layer's 3 input channels pack into a zero-padded 4-channel (one K-chunk) image
      int rc = drs_launch_pack_conv_mfma(w, b, nullptr, nullptr, nullptr, nullptr, 0.f, pk + plan->o_wf[l],
                                         (float*)(pk + plan->o_bf[l]), kCfg[l], cin_of(l), 9, 0, plan->impl, s);
      // data gradient: the same weights read transposed (Cin_d = Cout, Cout_d = Cin) with the taps flipped; the first layer's
      // 3 output channels padded to 32 with zero weights
      if (!rc)
        rc = drs_launch_pack_conv_mfma(w, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, pk + plan->o_wd[l], nullptr,
                                       dgrad_cout(l), kCfg[l], 9, 1, plan->impl, s, {.cout_src = cin_of(l), .flip_taps = 1});
      if (rc) return rc;
    }
    const int rc = queue.flush(s);
    if (rc) return rc;
  }
  auto up = [&](size_t off, const void* src, size_t n) -> int {
    if (n) DRS_CHECK_HIP(hipMemcpyAsync(pk + off, src, n * 4, hipMemcpyHostToDevice, s));
    return DRS_OK;
  };
  int rc = up(plan->o_ty_i, plan->ty_i.data(), plan->ty_i.size());
  if (!rc) rc = up(plan->o_ty_w, plan->ty_w.data(), plan->ty_w.size());
  if (!rc) rc = up(plan->o_tx_i, plan->tx_i.data(), plan->tx_i.size());
  if (!rc) rc = up(plan->o_tx_w, plan->tx_w.data(), plan->tx_w.size());
  if (!rc) rc = up(plan->o_rx_off, plan->rx_off.data(), plan->rx_off.size());
  if (!rc) rc = up(plan->o_rx_i, plan->rx_i.data(), plan->rx_i.size());
  if (!rc) rc = up(plan->o_rx_w, plan->rx_w.data(), plan->rx_w.size());
  if (!rc) rc = up(plan->o_ry_off, plan->ry_off.data(), plan->ry_off.size());
  if (!rc) rc = up(plan->o_ry_i, plan->ry_i.data(), plan->ry_i.size());
  if (!rc) rc = up(plan->o_ry_w, plan->ry_w.data(), plan->ry_w.size());
  if (rc) return rc;
  plan->packed_ptr = packed;
  plan->packed_ok = true;
  plan->saved = 0;
  return DRS_OK;
}

static double conv_flops(int N, int H, int W, int Cin, int Cout) { return 2.0 * N * H * W * (double)Cin * Cout * 9; }

extern "C" int drs_vgg_forward(drs_vgg_plan* plan, const void* packed, const float* pred, const float* target, float* loss,
                               int save, void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(plan && packed && pred && target && loss && workspace, DRS_ERR_ARG, "vgg_forward: null pointer");
  DRS_REQUIRE(plan->packed_ok && plan->packed_ptr == packed, DRS_ERR_STATE, "vgg_forward: weights not packed");
  DRS_REQUIRE(workspace_bytes >= drs_vgg_workspace_bytes(plan), DRS_ERR_WORKSPACE, "vgg_forward: workspace too small");
  char* pk = base256(packed);
  char* ws = base256(workspace);
  plan->nops = 0;
  plan->saved = 0;
  const int B = plan->B, N2 = 2 * B;
  {
    OpScope op(plan, s, "prep", 0.0);
    const long long total = (long long)N2 * plan->H0 * plan->W0;
    DRS_LAUNCH(vgg_prep_kernel, dim3(grid_for(total)), dim3(256), 0, s, pred, target, B, plan->H, plan->W, plan->H0, plan->W0,
               plan->resize, (const int*)(pk + plan->o_ty_i), (const float*)(pk + plan->o_ty_w),
               (const int*)(pk + plan->o_tx_i), (const float*)(pk + plan->o_tx_w), (float4*)(ws + plan->o_x0));
    DRS_CHECK_HIP(hipGetLastError());
  }
  const float* cur = (const float*)(ws + plan->o_x0);
  int ping = 0;
  for (int l = 0; l < kConvs; ++l) {
    const int v = level_of(l), H = plan->LH[v], W = plan->LW[v], Cout = kCfg[l];
    float* y = (float*)(ws + plan->o_act[ping]);
    {
      char name[16];
      snprintf(name, sizeof(name), "conv%d", l + 1);
      OpScope op(plan, s, name, conv_flops(N2, H, W, cin_of(l), Cout));
      TapConv d = vgg_conv(cur, N2, H, W, fwd_cin(l), pk + plan->o_wf[l], (const float*)(pk + plan->o_bf[l]), y, Cout);
      d.relu_pre = 1;
      const int rc = drs_launch_tapconv_mfma(d, plan->impl, s);
      if (rc) return rc;
    }
    if (save)  // the prediction half (images 0 .. B-1) of the ReLU output: relu masks and pool argmaxes of the backward
      DRS_CHECK_HIP(hipMemcpyAsync(ws + plan->o_save[l], y, (size_t)B * H * W * Cout * 4, hipMemcpyDeviceToDevice, s));
    cur = y;
    ping ^= 1;
    if (pool_after(l)) {
      float* o = l == kConvs - 1 ? (float*)(ws + plan->o_feat) : (float*)(ws + plan->o_act[ping]);
      char name[16];
      snprintf(name, sizeof(name), "pool%d", v + 1);
      OpScope op(plan, s, name, 0.0);
      const long long total = (long long)N2 * (H >> 1) * (W >> 1) * (Cout / 4);
      DRS_LAUNCH(vgg_pool_fwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const float4*)cur, (float4*)o, N2, H, W, Cout / 4);
      DRS_CHECK_HIP(hipGetLastError());
      cur = o;
      ping ^= 1;
    }
  }
  {
    OpScope op(plan, s, "loss", 0.0);
    const long long numel = (long long)B * (plan->LH[4] >> 1) * (plan->LW[4] >> 1) * 512;
    double* part = (double*)(ws + plan->o_part);
    DRS_LAUNCH(vgg_loss_partial_kernel, dim3(kRedBlocks), dim3(256), 0, s, (const float*)(ws + plan->o_feat), numel, part);
    DRS_LAUNCH(vgg_loss_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, numel, loss);
    DRS_CHECK_HIP(hipGetLastError());
  }
  plan->saved = save ? 1 : 0;
  return DRS_OK;
}

extern "C" int drs_vgg_backward(drs_vgg_plan* plan, const void* packed, const float* grad_loss, float* dpred, void* workspace,
                                size_t workspace_bytes, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(plan && packed && grad_loss && dpred && workspace, DRS_ERR_ARG, "vgg_backward: null pointer");
  DRS_REQUIRE(plan->packed_ok && plan->packed_ptr == packed, DRS_ERR_STATE, "vgg_backward: weights not packed");
  DRS_REQUIRE(workspace_bytes >= drs_vgg_workspace_bytes(plan), DRS_ERR_WORKSPACE, "vgg_backward: workspace too small");
  DRS_REQUIRE(plan->saved, DRS_ERR_STATE, "vgg_backward: the workspace holds no forward with save = 1");
  char* pk = base256(packed);
  char* ws = base256(workspace);
  plan->nops = 0;
  const int B = plan->B;
  const long long numel = (long long)B * (plan->LH[4] >> 1) * (plan->LW[4] >> 1) * 512;
  float* g[2] = {(float*)(ws + plan->o_g[0]), (float*)(ws + plan->o_g[1])};
  int gi = 0;
  {
    OpScope op(plan, s, "seed", 0.0);
    DRS_LAUNCH(vgg_seed_kernel, dim3(grid_for(numel)), dim3(256), 0, s, (const float*)(ws + plan->o_feat), numel, grad_loss, g[gi]);
    DRS_CHECK_HIP(hipGetLastError());
  }
  // g[gi] holds the gradient w.r.t. the output of layer l's ReLU (or of the pool after it): make it the gradient w.r.t. the
  // convolution's output (pre-ReLU), then convolve it back to layer l's input
  for (int l = kConvs - 1; l >= 0; --l) {
    const int v = level_of(l), H = plan->LH[v], W = plan->LW[v], Cout = kCfg[l];
    const float* y = (const float*)(ws + plan->o_save[l]);
    if (pool_after(l)) {
      char name[16];
      snprintf(name, sizeof(name), "pool%d_bwd", v + 1);
      OpScope op(plan, s, name, 0.0);
      const long long total = (long long)B * H * W * (Cout / 4);
      DRS_LAUNCH(vgg_pool_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const float4*)g[gi], (const float4*)y,
                 (float4*)g[gi ^ 1], B, H, W, Cout / 4);
      DRS_CHECK_HIP(hipGetLastError());
      gi ^= 1;
    } else {
      char name[16];
      snprintf(name, sizeof(name), "relu%d_bwd", l + 1);
      OpScope op(plan, s, name, 0.0);
      const long long n4 = (long long)B * H * W * (Cout / 4);
      DRS_LAUNCH(vgg_relu_mask_kernel, dim3(grid_for(n4)), dim3(256), 0, s, (float4*)g[gi], (const float4*)y, n4);
      DRS_CHECK_HIP(hipGetLastError());
    }
    {
      char name[16];
      snprintf(name, sizeof(name), "conv%d_dgrad", l + 1);
      OpScope op(plan, s, name, conv_flops(B, H, W, Cout, cin_of(l)));
      TapConv d = vgg_conv(g[gi], B, H, W, Cout, pk + plan->o_wd[l], nullptr, g[gi ^ 1], dgrad_cout(l));
      const int rc = drs_launch_tapconv_mfma(d, plan->impl, s);
      if (rc) return rc;
      gi ^= 1;
    }
  }
  {
    OpScope op(plan, s, "prep_bwd", 0.0);
    const int H0 = plan->H0, W0 = plan->W0;
    float* dp = plan->resize ? (float*)(ws + plan->o_dp) : dpred;  // without a resize the normalisation adjoint is the result
    const long long total = (long long)B * 3 * H0 * W0;
    DRS_LAUNCH(vgg_norm_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, s, (const float*)g[gi], 32, dp, B, H0, W0);
    if (plan->resize) {
      float* t = (float*)(ws + plan->o_t);
      const long long lines = (long long)B * 3 * H0;
      DRS_LAUNCH(vgg_bicubic_bwd_x_kernel, dim3(grid_for(lines * plan->W)), dim3(256), 0, s, (const float*)dp, t, lines, W0,
                 plan->W, (const int*)(pk + plan->o_rx_off), (const int*)(pk + plan->o_rx_i), (const float*)(pk + plan->o_rx_w));
      DRS_LAUNCH(vgg_bicubic_bwd_y_kernel, dim3(grid_for((long long)B * 3 * plan->H * plan->W)), dim3(256), 0, s,
                 (const float*)t, dpred, B * 3, H0, plan->H, plan->W, (const int*)(pk + plan->o_ry_off),
                 (const int*)(pk + plan->o_ry_i), (const float*)(pk + plan->o_ry_w));
    }
    DRS_CHECK_HIP(hipGetLastError());
  }
  return DRS_OK;
}

// ---- introspection: the tensors a forward leaves in the workspace (parity tests) --------------------------------------------
// 0: x0 (2B, 4, H0, W0), 1 .. 16: conv1 .. conv16 (B, C, h, w) - the saved prediction-half ReLU outputs, 17: features
namespace {
constexpr int kVggTensors = kConvs + 2;
const char* const kVggTensorNames[kVggTensors] = {"x0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv8",
                                                  "conv9", "conv10", "conv11", "conv12", "conv13", "conv14", "conv15", "conv16",
                                                  "features"};
struct VggTensor { size_t off; int n, c, h, w; };
VggTensor vgg_tensor(const drs_vgg_plan* p, int i) {
  if (i == 0) return {p->o_x0, 2 * p->B, 4, p->H0, p->W0};
  if (i == kVggTensors - 1) return {p->o_feat, 2 * p->B, 512, p->LH[4] >> 1, p->LW[4] >> 1};
  const int l = i - 1, v = level_of(l);
  return {p->o_save[l], p->B, kCfg[l], p->LH[v], p->LW[v]};
}
}  // namespace

extern "C" int drs_vgg_num_tensors(const drs_vgg_plan* plan) { return plan ? kVggTensors : 0; }
extern "C" const char* drs_vgg_tensor_name(const drs_vgg_plan* plan, int i) {
  return (plan && i >= 0 && i < kVggTensors) ? kVggTensorNames[i] : nullptr;
}
extern "C" int drs_vgg_tensor_shape(const drs_vgg_plan* plan, int i, int* n, int* c, int* h, int* w) {
  DRS_REQUIRE(plan && i >= 0 && i < kVggTensors && n && c && h && w, DRS_ERR_ARG, "vgg_tensor_shape: bad index");
  const VggTensor t = vgg_tensor(plan, i);
  *n = t.n; *c = t.c; *h = t.h; *w = t.w;
  return DRS_OK;
}
extern "C" int drs_vgg_read_tensor(const drs_vgg_plan* plan, int i, const void* workspace, float* dst, drs_stream_t stream) {
  DRS_REQUIRE(plan && workspace && dst && i >= 0 && i < kVggTensors, DRS_ERR_ARG, "vgg_read_tensor: bad args");
  DRS_REQUIRE(plan->saved || i == 0 || i == kVggTensors - 1, DRS_ERR_STATE,
              "vgg_read_tensor: %s is kept only by a forward with save = 1", kVggTensorNames[i]);
  const VggTensor t = vgg_tensor(plan, i);
  return drs_launch_nhwc_to_nchw((const float*)(base256(workspace) + t.off), dst, t.n, t.c, t.h, t.w, t.c, 0,
                                 (hipStream_t)stream);
}

extern "C" int drs_vgg_profile_enable(drs_vgg_plan* plan, int on) {
  DRS_REQUIRE(plan, DRS_ERR_ARG, "vgg_profile_enable: null plan");
  plan->prof = on != 0;
  plan->nops = 0;
  return DRS_OK;
}
extern "C" int drs_vgg_profile_num_ops(const drs_vgg_plan* plan) { return plan ? (int)plan->nops : 0; }
extern "C" int drs_vgg_profile_read(drs_vgg_plan* plan, int i, char* name, int name_len, float* ms, double* flops) {
  DRS_REQUIRE(plan && name && ms && flops && i >= 0 && (size_t)i < plan->nops, DRS_ERR_ARG, "vgg_profile_read: bad argument");
  const drs_vgg_plan::OpRec& r = plan->ops[i];
  DRS_CHECK_HIP(hipEventSynchronize(r.e1));
  DRS_CHECK_HIP(hipEventElapsedTime(ms, r.e0, r.e1));
  snprintf(name, (size_t)name_len, "%s", r.name.c_str());
  *flops = r.flops;
  return DRS_OK;
}
