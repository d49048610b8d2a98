// Backward schedule of one training step through the UNet (its own translation unit;
// it works on drs_plan's layer tables and workspace tensors through unet_plan.h).
//
// Mirrors what autograd does for the reference graph (UNet_model_superres.py:337-379 under model.train()), given
// d(loss)/d(output).  Data gradients are tap-convolutions with re-packed weights (same kernels as the forward);
// weight gradients use wgrad_kernel; BatchNorm uses the batch statistics saved by the train-mode forward
// (a DRS_PLAN_FROZEN_BN plan: the running statistics that forward copied into the same slot, and dZ = gamma * rstd * g).
// Requires: a train plan (DRS_PLAN_TRAIN), lr_batch == batch, and the workspace exactly as the last
// drs_unet_forward on this plan left it.

#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <utility>

#include "unet_plan.h"

// Output channels of a layer's data-gradient convolution as the MFMA kernels run it: the layer's Cin, with the 16-channel
// case (gradient w.r.t. x0) padded to the 32-channel tile (zero weights; the gradient tensor has a 32-float pixel stride).
static inline int dgrad_cout(const ConvLayer& L) { return L.Cin == 16 ? 32 : L.Cin; }
static const int kGx0Stride = 32;

// A layer's slot in packed_bwd: room for whichever kernel family's data-gradient image is largest, then the zero bias
// the data-gradient convolutions read.
struct DgradLayout { size_t bias_off, bytes; };
static DgradLayout dgrad_layout(const ConvLayer& L) {
  size_t need = (size_t)L.Cout * L.Cin * L.taps * 4;
  for (int im = DRS_IMPL_MFMA_F32; im <= DRS_IMPL_MFMA_F16; ++im)
    need = std::max(need, drs_pack_conv_mfma_bytes(dgrad_cout(L), L.Cout, L.taps, im));  // roles swapped
  return {align_up(need), align_up(need) + align_up((size_t)std::max(L.Cin, L.Cout) * 4)};
}

extern "C" size_t drs_unet_packed_bwd_bytes(const drs_plan* plan) {
  if (!plan) return 0;
  size_t cur = 0;
  for (const ConvLayer* L : plan->convs) cur += dgrad_layout(*L).bytes;
  return cur + 512;
}

namespace {
// A layer's data-gradient weight image as bwd_pack_dgrad_images packed it: offset of its dgrad_layout slot in packed_bwd,
// run_dgrad's kind (-1: not packed; psi_bwd carries psi's data gradient) and whether it is for the MFMA or direct kernels
struct DgradImage { size_t off = 0; int kind = -1; bool mfma = false; };

// What every step of one backward reads.  wgrad_side is decided on each call.
struct BwdCtx {
  drs_plan* plan;
  const drs_unet_config& cfg;
  hipStream_t s;
  char* pk;   // forward packed image (aligned base)
  char* pkb;  // dgrad weight images (aligned base)
  void* ws;   // workspace (aligned base)
  float* const* grads;
  int impl;                 // arithmetic of the backward products (bwd_impl)
  bool wgrad_mfma;          // weight gradients on the MFMA kernel (else the direct / VALU one)
  bool wgrad_side = false;  // ... and on the plan's side stream
  float *temb, *dtemb;
  double* sums_bwd;  // backward BatchNorm sums region, one slot per layer
  float* red;        // reduction partials
  float* scratch;    // sink for BatchNorm / psi gradients the caller does not want
  int B, H, W, h, w;  // h, w: the LR image
  // grad.R0..R3 written in this call: the first writer stores, later writers accumulate
  bool gR_written[4] = {false, false, false, false};
  std::vector<DgradImage> dgrad;  // per conv layer (index in plan->convs)
  BwdCtx(drs_plan* p, const void* packed, void* packed_bwd, void* workspace, float* const* g, hipStream_t stream, int im)
      : plan(p), cfg(p->cfg), s(stream), pk(aligned_base(packed)), pkb(aligned_base(packed_bwd)),
        ws(aligned_base(workspace)), grads(g), impl(im), wgrad_mfma(im != DRS_IMPL_DIRECT),
        temb((float*)((char*)ws + p->o_temb)), dtemb((float*)((char*)ws + p->o_dtemb)),
        sums_bwd((double*)((char*)ws + p->o_bn_sums + p->bn_sums_bytes)), red((float*)((char*)ws + p->o_red)),
        scratch((float*)((char*)ws + p->o_scratch)), B(cfg.batch), H(cfg.height), W(cfg.width),
        h(cfg.height / cfg.magnification), w(cfg.width / cfg.magnification) {}
  float* TP(int i) const { return plan->tp(ws, i); }
  const float* PARAM(int i) const { return (const float*)plan->param_ptrs[i]; }
  float* G(int i) const { return i >= 0 ? grads[i] : nullptr; }  // grad of param i (null: the caller does not want it)
  // SP-format copy of a layer's dZ (written by its BatchNorm backward when the data gradients run on split bf16), or null
  float* ZSP(const ConvLayer& L) const { return (L.t_Zsp >= 0 && impl == DRS_IMPL_MFMA_BF16X3) ? TP(L.t_Zsp) : nullptr; }
};
}  // namespace

static int conv_index(const drs_plan* plan, const ConvLayer* L) {
  for (size_t i = 0; i < plan->convs.size(); ++i)
    if (plan->convs[i] == L) return (int)i;
  return -1;
}

// Arithmetic of the data-gradient convolutions.  Next to the exact-fp32 FORWARD (the training default) the backward
// PRODUCTS run on split bf16 (16 operand mantissa bits, fp32 accumulation): every gradient norm of the golden step stays
// within 2e-4 of the reference's autograd (4e-5 measured) - the training error of a split-bf16 plan comes from its
// forward activations, not from the backward products.  DRS_TRAIN_BWD_IMPL=mfma_f32 keeps them
// exact, =mfma_bf16x3 forces the split form next to any forward.
static int bwd_impl(int impl) {
  static const char* bwd_env = getenv("DRS_TRAIN_BWD_IMPL");
  if (impl == DRS_IMPL_DIRECT) return impl;
  if (bwd_env && !strcmp(bwd_env, "mfma_f32")) return DRS_IMPL_MFMA_F32;
  if (bwd_env && !strcmp(bwd_env, "mfma_bf16x3")) return DRS_IMPL_MFMA_BF16X3;
  if (!bwd_env && impl == DRS_IMPL_MFMA_F32) return DRS_IMPL_MFMA_BF16X3;
  return impl;
}

// ---- dgrad descriptors: dX = conv^T(dY) expressed as tap convolutions over dY with weights read "transposed" -------
// kind: 0 = stride-1 conv (1x1 / 3x3 p1): same taps, flipped;  1 = 3x3 s2 p1 conv -> ConvTranspose(k3,s2,p1,op1) of dY;
//       2 = ConvTranspose(k3,s2,p1,op1) -> 3x3 s2 p1 conv of dY;  3 = 2x2 s2 conv -> 4 phases of 1x1 with out_scale 2.
static int pack_dgrad(BwdCtx& c, const ConvLayer& L, int kind) {
  DgradImage& im = c.dgrad[conv_index(c.plan, &L)];
  TapConv probe = {};
  probe.Cin = L.Cout; probe.Cout = dgrad_cout(L); probe.ntaps = L.taps;
  im.kind = kind;
  im.mfma = c.impl != DRS_IMPL_DIRECT && drs_tapconv_mfma_supported(probe, c.impl);
  char* dst = c.pkb + im.off;
  float* zero_b = (float*)(dst + dgrad_layout(L).bias_off);
  const float* w = c.PARAM(L.w);
  // forward layout (Cout,Cin,taps) read as a transposed-conv weight (Cin_T = Cout, Cout_T = Cin): kinds 0, 1, 3;
  // ConvTranspose layout (Cin,Cout,taps) read as a plain conv weight (Cout_d = Cin, Cin_d = Cout): kind 2.
  const int transposed_read = kind == 2 ? 0 : 1;
  if (im.mfma)
    // kind 0 (stride-1 convolution): taps flipped in the packed image, so the launch is a standard 3x3 / 1x1
    // convolution and takes the CONV3X3 schedule instead of the generic tap list
    return drs_launch_pack_conv_mfma(w, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, dst, zero_b, dgrad_cout(L), L.Cout,
                                     L.taps, transposed_read, c.impl, c.s, {.cout_src = L.Cin, .flip_taps = kind == 0 ? 1 : 0});
  return drs_launch_pack_conv(w, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, (float*)dst, zero_b, L.Cin, L.Cout, L.taps,
                              transposed_read, 0, c.s);
}

// Every layer's data-gradient weight image up front: one queue, a few batched launches.  The order decides which images
// share a launch.
static int bwd_pack_dgrad_images(BwdCtx& c) {
  const drs_plan* plan = c.plan;
  size_t cur = 0;
  for (const ConvLayer* L : plan->convs) { c.dgrad.push_back(DgradImage{cur}); cur += dgrad_layout(*L).bytes; }
  DrsPackQueueScope pack_queue;
  RUN(pack_dgrad(c, plan->output, 0));
  for (int i = 0; i < 3; ++i) {
    const DecStage& st = plan->dec[i];
    RUN(pack_dgrad(c, st.upconv, 0));
    RUN(pack_dgrad(c, st.transform, 2));
    RUN(pack_dgrad(c, st.conv, 0));
    RUN(pack_dgrad(c, st.result, 0));
    RUN(pack_dgrad(c, st.wx, 3));
    RUN(pack_dgrad(c, st.wg, 0));
    RUN(pack_dgrad(c, st.gate, 0));
    RUN(pack_dgrad(c, plan->downs[i], 1));
  }
  for (int i = 0; i < 4; ++i) {
    const ResBlock& rb = plan->enc[i];
    RUN(pack_dgrad(c, rb.shortcut, 0));
    RUN(pack_dgrad(c, rb.conv2, 0));
    if (rb.has_skip) RUN(pack_dgrad(c, rb.skip, 0));
    RUN(pack_dgrad(c, rb.conv1, 0));
  }
  return pack_queue.flush(c.s);
}

// dX (+)= dgrad of layer L applied to dY.  dY: (N, OHd, OWd, Cout) slice; dX: (N, IH, IW, Cin) slice.
// dY_sp: the same dY in SP format (bn_bwd's second output), or null: 3x3 stride-1 layers then run on the wave-specialised SP
// kernel with the fp32 epilogue (conv_mfma_sp.hip, F32OUT) instead of the fp32-input kernels.
static int run_dgrad(BwdCtx& c, const ConvLayer& L, const float* dY, int dy_cs, int dy_co, int N, int OHd, int OWd,
                     float* dX, int dx_cs, int dx_co, int IH, int IW, bool accumulate, const float* gate = nullptr,
                     const float* dY_sp = nullptr) {
  const DgradImage& im = c.dgrad[conv_index(c.plan, &L)];
  DRS_REQUIRE(im.kind >= 0, DRS_ERR_STATE, "backward: no data-gradient image packed for this layer");
  const float* w = (const float*)(c.pkb + im.off);
  const int impl = im.mfma ? c.impl : DRS_IMPL_DIRECT;
  const int Cd = im.mfma ? dgrad_cout(L) : L.Cin;  // channels the kernel writes (padded ones are zeros)
  auto finish = [&](TapConv& d) {
    d.bias = nullptr;
    d.gate = gate;
    if (accumulate) { d.res = dX; d.res_cs = dx_cs; d.res_co = dx_co; }
    return run_conv(d, impl, c.s);
  };
  if (im.kind == 0) {
    const int K = L.taps == 9 ? 3 : 1, pad = L.taps == 9 ? 1 : 0;
    TapConv d = conv_desc(dY, N, OHd, OWd, L.Cout, dy_cs, dy_co, w, nullptr, dX, Cd, dx_cs, dx_co, K, K, 1, pad);
    if (!im.mfma)
      for (int i = 0; i < d.ntaps; ++i) d.wtap[i] = d.ntaps - 1 - i;  // flipped kernel (the MFMA image is packed flipped)
    if (im.mfma && dY_sp && impl == DRS_IMPL_MFMA_BF16X3 && L.taps == 9 && !gate) {
      d.in = dY_sp; d.in_sp = 1;
      d.zero_line = c.pk + c.plan->o_zero;
      d.fault = (unsigned*)(c.pk + c.plan->o_fault);  // a poll timeout of the wave-specialised kernel reports itself (drs_unet_check_faults)
    }
    return finish(d);
  }
  if (im.kind == 1) {  // dY (N,OHd,OWd) -> dX (N,2*OHd,2*OWd)
    if (im.mfma) {
      TapConv d = convT_fused_desc(dY, N, OHd, OWd, L.Cout, dy_cs, dy_co, w, nullptr, dX, L.Cin, dx_cs, dx_co);
      return finish(d);
    }
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        TapConv d = convT_phase_desc(dY, N, OHd, OWd, L.Cout, dy_cs, dy_co, w, nullptr, dX, L.Cin, dx_cs, dx_co, py, px);
        RUN(finish(d));
      }
    return DRS_OK;
  }
  if (im.kind == 2) {  // dY (N,OHd,OWd) high-res -> dX (N,OHd/2,OWd/2)
    TapConv d = conv_desc(dY, N, OHd, OWd, L.Cout, dy_cs, dy_co, w, nullptr, dX, L.Cin, dx_cs, dx_co, 3, 3, 2, 1);
    return finish(d);
  }
  // kind 3: 2x2 s2 conv: dX[2i+a][2j+b] = W[:, :, a, b]^T dY[i][j]
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      TapConv d = conv_desc(dY, N, OHd, OWd, L.Cout, dy_cs, dy_co, w, nullptr, dX, L.Cin, dx_cs, dx_co, 1, 1, 1, 0);
      d.OH = IH; d.OW = IW; d.out_scale = 2; d.out_oy = a; d.out_ox = b;
      d.wtap[0] = a * 2 + b; d.wtaps_total = 4;
      RUN(finish(d));
    }
  return DRS_OK;
}

// ---- wgrad descriptors ---------------------------------------------------------------------------------------------
static WgradDesc wgrad_conv(const float* A, int a_cs, int a_co, int Ca, int AH, int AW, const float* Bt, int b_cs,
                            int b_co, int Cb, int OH, int OW, int N, int K, int stride, int pad) {
  WgradDesc d = {};
  d.A = A; d.a_cs = a_cs; d.a_co = a_co; d.Ca = Ca; d.AH = AH; d.AW = AW; d.sa = stride;
  d.B = Bt; d.b_cs = b_cs; d.b_co = b_co; d.Cb = Cb; d.BH = OH; d.BW = OW; d.sb = 1;
  d.N = N; d.TH = OH; d.TW = OW; d.ntaps = K * K; d.T_total = K * K;
  for (int ky = 0; ky < K; ++ky)
    for (int kx = 0; kx < K; ++kx) {
      const int i = ky * K + kx;
      d.ay[i] = ky - pad; d.ax[i] = kx - pad; d.by[i] = 0; d.bx[i] = 0; d.wtap[i] = i;
    }
  return d;
}
static WgradDesc wgrad_convT(const float* A, int a_cs, int Ca, int H, int W, const float* Bt, int b_cs, int b_co, int Cb,
                             int N) {
  WgradDesc d = {};
  d.A = A; d.a_cs = a_cs; d.a_co = 0; d.Ca = Ca; d.AH = H; d.AW = W; d.sa = 1;
  d.B = Bt; d.b_cs = b_cs; d.b_co = b_co; d.Cb = Cb; d.BH = 2 * H; d.BW = 2 * W; d.sb = 2;
  d.N = N; d.TH = H; d.TW = W; d.ntaps = 9; d.T_total = 9;
  for (int i = 0; i < 9; ++i) { d.ay[i] = 0; d.ax[i] = 0; d.by[i] = i / 3 - 1; d.bx[i] = i % 3 - 1; d.wtap[i] = i; }
  d.out_transposed = 1;
  return d;
}

static int bias_grad(BwdCtx& c, const ConvLayer& L, const float* dY, int cs, int co, long long npix) {
  if (!c.G(L.b)) return DRS_OK;
  return drs_launch_colsum(dY, cs, co, L.Cout, npix, npix, 0, 0, c.G(L.b), c.s, c.red);
}
// BatchNorm backward of layer L: g = grad w.r.t. the BatchNorm output (before the ReLU mask if relu_pre); Z -> dZ in place
// mask_y: output of a ReLU sitting on g's tensor (g counts as g * (mask_y > 0)), channel stride my_cs
static int bn_bwd(BwdCtx& c, const ConvLayer& L, const float* g, int g_cs, int g_co, int relu_pre, long long npix,
                  const float* mask_y = nullptr, int my_cs = 0) {
  float* stats = (float*)((char*)c.ws + L.stats_off);
  float* dgam = c.G(L.bn) ? c.G(L.bn) : c.scratch;
  float* dbet = c.G(L.bn + 1) ? c.G(L.bn + 1) : c.scratch + 1024;
  // With profiling on (drs_unet_profile_enable) every BatchNorm backward is one op appended to the forward's op list
  // ("<norm>.bwd"; algorithmic bytes: g, Z and the optional mask read once or twice, dZ and its optional SP copy written).
  std::string name = c.plan->params[L.bn].name;
  name = name.substr(0, name.size() - 7) + ".bwd";  // strip ".weight"
  const double tb = 4.0 * npix * L.Cout, reads = (mask_y ? 3.0 : 2.0) * tb, writes = (c.ZSP(L) ? 2.0 : 1.0) * tb;
  if (c.plan->frozen_bn())  // dZ = gamma * rstd * g: sums and dZ in one pass
    return prof_op(c.plan, name, 0, reads + writes, c.s, [&] {
      return drs_launch_bn_bwd_frozen(g, g_cs, g_co, c.TP(L.t_Z), stats, stats + L.Cout, c.PARAM(L.bn), c.PARAM(L.bn + 1),
                                      relu_pre, L.Cout, npix, (double*)c.red, (double*)((char*)c.sums_bwd + L.sums_off), dgam,
                                      dbet, c.s, c.ZSP(L), mask_y, my_cs, 0);
    });
  return prof_op(c.plan, name, 0, 2.0 * reads + writes, c.s, [&] {
    return drs_launch_bn_bwd(g, g_cs, g_co, c.TP(L.t_Z), stats, stats + L.Cout, c.PARAM(L.bn), c.PARAM(L.bn + 1), relu_pre,
                             L.Cout, npix, (double*)c.red, (double*)((char*)c.sums_bwd + L.sums_off), dgam, dbet, c.s,
                             c.ZSP(L), mask_y, my_cs, 0);
  });
}
static hipStream_t wgrad_stream(BwdCtx& c) {  // stream for a weight-gradient launch whose operands are ready on c.s now
  if (!c.wgrad_side) return c.s;
  (void)hipEventRecord(c.plan->ev_fork, c.s);
  (void)hipStreamWaitEvent(c.plan->side, c.plan->ev_fork, 0);
  return c.plan->side;
}
// weight gradient dW and, for a convolution (d.B = dY read at the iteration position), its bias gradient db:
// the MFMA kernel produces sum_p dY[p][co] on the side, the direct path runs colsum
static int wgrad(BwdCtx& c, WgradDesc d, float* dW, float* db) {
  if (!dW)
    return db ? drs_launch_colsum(d.B, d.b_cs, d.b_co, d.Cb, (long long)d.N * d.BH * d.BW, (long long)d.BH * d.BW, 0, 0, db, c.s)
              : DRS_OK;
  d.dW = dW;
  d.dbias = db;
  if (c.wgrad_mfma) { d.partial = (float*)((char*)c.ws + c.plan->o_wgrad); d.partial_bytes = kWgradPartialBytes; }
  return drs_launch_wgrad(d, wgrad_stream(c));
}
static int wgrad(BwdCtx& c, const ConvLayer& L, const WgradDesc& d) { return wgrad(c, d, c.G(L.w), c.G(L.b)); }
// few-channel stem layers (image -> 16 channels): their own kernel (stem_wgrad_kernel, stem_bwd.hip), on the side stream
// like every weight gradient (operands x.nhwc / upsampled_lr_img.nhwc / grad.x0 are not rewritten below; the partial
// rows share the side stream's slice workspace, whose users are stream-ordered).  Direct (VALU) plans keep wgrad_kernel.
static int stem_wgrad(BwdCtx& c, const PlanarConv& L, const WgradDesc& d) {
  if (c.wgrad_mfma && d.Cb == 16 && d.Ca <= kMaxBands)
    return drs_launch_stem_wgrad(d.B, d.b_cs, d.A, d.N, d.Ca, d.AH, d.AW, (float*)((char*)c.ws + c.plan->o_wgrad),
                                 kWgradPartialBytes, c.G(L.w), c.G(L.b), wgrad_stream(c));
  return wgrad(c, d, c.G(L.w), c.G(L.b));
}
// one launch per RRDB layer on the main stream: weight + bias gradient, data gradient, the ReLU mask on it (stem_bwd.hip)
static int small_bwd(BwdCtx& c, const PlanarConv& L, const float* in_nhwc, const float* gout, float* gin, bool accumulate,
                     const float* mask_y) {
  return drs_launch_small_conv_bwd(in_nhwc, gout, c.PARAM(L.w), gin, accumulate ? 1 : 0, mask_y, c.B, c.cfg.cond_channels,
                                   c.h, c.w, c.red, c.plan->red_bytes, c.G(L.w), c.G(L.b), c.s);
}

// zero every requested gradient and the per-image embedding gradients
// (callers usually carve the gradients out of one flat buffer: ranges that touch are cleared with a single memset,
//  whatever their order in the parameter list and whichever parameters in between are not wanted)
static int bwd_zero_grads(BwdCtx& c) {
  std::vector<std::pair<char*, size_t>> rng;
  for (size_t i = 0; i < c.plan->params.size(); ++i)
    if (c.grads[i]) rng.emplace_back((char*)c.grads[i], (size_t)c.plan->params[i].numel * 4);
  std::sort(rng.begin(), rng.end());
  for (size_t i = 0; i < rng.size();) {
    char* begin = rng[i].first;
    char* end = begin + rng[i].second;
    size_t j = i + 1;
    while (j < rng.size() && rng[j].first <= end) { end = std::max(end, rng[j].first + rng[j].second); ++j; }
    DRS_CHECK_HIP(hipMemsetAsync(begin, 0, (size_t)(end - begin), c.s));
    i = j;
  }
  DRS_CHECK_HIP(hipMemsetAsync(c.dtemb, 0, (size_t)c.B * c.plan->temb_total * 4, c.s));
  return DRS_OK;
}

// ---- head: output 1x1 conv (:379).  dout arrives NCHW; bring it to channels-last once. ----
static int bwd_head(BwdCtx& c, const float* dout) {
  const drs_plan* plan = c.plan;
  const int B = c.B, H = c.H, W = c.W, od = c.cfg.out_dim;
  float* dOut = c.TP(plan->g_out);
  RUN(drs_launch_nchw_to_nhwc(dout, dOut, B, od, H, W, od, 0, c.s));
  RUN(wgrad(c, plan->output, wgrad_conv(c.TP(plan->t_X[2]), kUp[3], 0, kUp[3], H, W, dOut, od, 0, od, H, W, B, 1, 1, 0)));
  return run_dgrad(c, plan->output, dOut, od, 0, B, H, W, c.TP(plan->g_X[2]), kUp[3], 0, H, W, false);
}

// ---- decoder stage i (run last stage first) ----
static int bwd_decoder_stage(BwdCtx& c, int i) {
  const drs_plan* plan = c.plan;
  const DecStage& st = plan->dec[i];
  const int B = c.B, Cc = kUp[i], Ch = kUp[i + 1];
  const int lh = c.H >> (3 - i), lw = c.W >> (3 - i), hh = 2 * lh, hw = 2 * lw;
  const long long np_lo = (long long)B * lh * lw, np_hi = (long long)B * hh * hw;
  const float* xres = c.TP(plan->t_R[2 - i]);
  float* gRes = c.TP(plan->g_R[2 - i]);
  const float* xc = i == 0 ? c.TP(plan->t_R[3]) : c.TP(plan->t_X[i - 1]);
  float* gxc = i == 0 ? c.TP(plan->g_R[3]) : c.TP(plan->g_X[i - 1]);
  float* gX = c.TP(plan->g_X[i]);
  float* gCAT = c.TP(plan->g_CAT[i]);
  const float* cat = c.TP(plan->t_CAT[i]);
  // up_conv (:377)
  RUN(wgrad(c, st.upconv, wgrad_conv(cat, Cc + Ch, 0, Cc + Ch, hh, hw, gX, Ch, 0, Ch, hh, hw, B, 3, 1, 1)));
  // (on the SP kernel through an SP copy of gX, round 4: 318 -> 433 us at stage 1 - few K-chunks per item against 192 / 384
  //  fp32 output channels through the general epilogue; the fp32-input kernel stays)
  RUN(run_dgrad(c, st.upconv, gX, Ch, 0, B, hh, hw, gCAT, Cc + Ch, 0, hh, hw, false));
  // transform = ConvTranspose2d (:206): dT = gCAT[:, :Cc]
  RUN(bias_grad(c, st.transform, gCAT, Cc + Ch, 0, np_hi));
  RUN(wgrad(c, wgrad_convT(c.TP(plan->t_U[i]), Cc, Cc, lh, lw, gCAT, Cc + Ch, 0, Cc, B), c.G(st.transform.w), nullptr));
  float* gU = c.TP(plan->g_U[i]);
  RUN(run_dgrad(c, st.transform, gCAT, Cc + Ch, 0, B, hh, hw, gU, Cc, 0, lh, lw, false));
  // ups.conv + BN + ReLU on (x + temb) (:199-205)
  RUN(bn_bwd(c, st.conv, gU, Cc, 0, 1, np_lo));
  {
    WgradDesc d = wgrad_conv(xc, Cc, 0, Cc, lh, lw, c.TP(st.conv.t_Z), Cc, 0, Cc, lh, lw, B, 3, 1, 1);
    d.a_add = c.temb + st.mlp.temb_off; d.a_add_cs = plan->temb_total;
    RUN(wgrad(c, st.conv, d));
  }
  RUN(run_dgrad(c, st.conv, c.TP(st.conv.t_Z), Cc, 0, B, lh, lw, gxc, Cc, 0, lh, lw, false, nullptr, c.ZSP(st.conv)));
  RUN(drs_launch_colsum(gxc, Cc, 0, Cc, np_lo, (long long)lh * lw, 1, plan->temb_total, c.dtemb + st.mlp.temb_off, c.s));
  // attention result: BN (no ReLU) over Zr = up2(psi) * (Wr x) + br  (:105-107): datt = gCAT[:, Cc:]
  RUN(bn_bwd(c, st.result, gCAT, Cc + Ch, Cc, 0, np_hi));
  float* dZr = c.TP(st.result.t_Z);
  {
    WgradDesc d = wgrad_conv(xres, Ch, 0, Ch, hh, hw, dZr, Ch, 0, Ch, hh, hw, B, 1, 1, 0);
    d.a_gate = c.TP(plan->t_PSI[i]);
    RUN(wgrad(c, st.result, d));
  }
  float* E = c.TP(plan->g_E[i]);
  RUN(run_dgrad(c, st.result, dZr, Ch, 0, B, hh, hw, E, Ch, 0, hh, hw, false));
  if (!c.gR_written[2 - i]) { DRS_CHECK_HIP(hipMemsetAsync(gRes, 0, (size_t)np_hi * Ch * 4, c.s)); c.gR_written[2 - i] = true; }
  float* dpsi = c.TP(plan->g_PSI[i]);
  RUN(drs_launch_gate_bwd(xres, E, c.TP(plan->t_PSI[i]), gRes, dpsi, B, lh, lw, Ch, c.s));
  // psi conv + the ReLU in front of it (:103-104)
  float* gP = c.TP(plan->g_P[i]);
  RUN(drs_launch_psi_bwd(c.TP(plan->t_P[i]), c.PARAM(st.psi.w), dpsi, gP, c.G(st.psi.w) ? c.G(st.psi.w) : c.scratch,
                         c.G(st.psi.b) ? c.G(st.psi.b) : c.scratch + 1024, Ch, np_lo, c.red, c.s));
  // w_x (2x2 s2 over x_res) and w_g (1x1 over g): both see gP
  RUN(wgrad(c, st.wx, wgrad_conv(xres, Ch, 0, Ch, hh, hw, gP, Ch, 0, Ch, lh, lw, B, 2, 2, 0)));
  RUN(run_dgrad(c, st.wx, gP, Ch, 0, B, lh, lw, gRes, Ch, 0, hh, hw, true));
  RUN(wgrad(c, st.wg, wgrad_conv(c.TP(plan->t_G[i]), Ch, 0, Ch, lh, lw, gP, Ch, 0, Ch, lh, lw, B, 1, 1, 0)));
  float* gG = c.TP(plan->g_G[i]);
  RUN(run_dgrad(c, st.wg, gP, Ch, 0, B, lh, lw, gG, Ch, 0, lh, lw, false));
  // gating signal: 1x1 conv + BN + ReLU (:222-225)
  RUN(bn_bwd(c, st.gate, gG, Ch, 0, 1, np_lo));
  RUN(wgrad(c, st.gate, wgrad_conv(xc, Cc, 0, Cc, lh, lw, c.TP(st.gate.t_Z), Ch, 0, Ch, lh, lw, B, 1, 1, 0)));
  RUN(run_dgrad(c, st.gate, c.TP(st.gate.t_Z), Ch, 0, B, lh, lw, gxc, Cc, 0, lh, lw, true));
  if (i == 0) c.gR_written[3] = true;  // gxc is grad.R3
  return DRS_OK;
}

// ---- bottleneck / encoder block i (ResConvBlock :153-172), then downs[i-1] (:366) (run last block first) ----
static int bwd_encoder_block(BwdCtx& c, int i) {
  const drs_plan* plan = c.plan;
  const ResBlock& rb = plan->enc[i];
  const int B = c.B, ci = kDown[i], co = kDown[i + 1], hh = c.H >> i, ww = c.W >> i;
  const long long npix = (long long)B * hh * ww;
  const float* u = i == 0 ? c.TP(plan->t_x0) : c.TP(plan->t_D[i - 1]);
  float* gu = i == 0 ? c.TP(plan->g_x0) : c.TP(plan->g_D[i - 1]);
  const int gu_cs = i == 0 ? kGx0Stride : ci;  // grad.x0 keeps a 32-float pixel stride (16 used)
  float* gR = c.TP(plan->g_R[i]);
  // out = relu(shortcut + BN2(conv2(h)))
  // (the block's final ReLU masks gR inside the two BatchNorm backwards that read it: no masking pass over gR)
  const float* Rout = c.TP(plan->t_R[i]);
  RUN(bn_bwd(c, rb.shortcut, gR, co, 0, 0, npix, Rout, co));
  RUN(wgrad(c, rb.shortcut, wgrad_conv(u, ci, 0, ci, hh, ww, c.TP(rb.shortcut.t_Z), co, 0, co, hh, ww, B, 1, 1, 0)));
  RUN(run_dgrad(c, rb.shortcut, c.TP(rb.shortcut.t_Z), co, 0, B, hh, ww, gu, gu_cs, 0, hh, ww, false));
  RUN(bn_bwd(c, rb.conv2, gR, co, 0, 0, npix, Rout, co));
  RUN(wgrad(c, rb.conv2, wgrad_conv(c.TP(plan->t_H[i]), co, 0, co, hh, ww, c.TP(rb.conv2.t_Z), co, 0, co, hh, ww, B, 3, 1, 1)));
  float* gH = c.TP(plan->g_H[i]);
  RUN(run_dgrad(c, rb.conv2, c.TP(rb.conv2.t_Z), co, 0, B, hh, ww, gH, co, 0, hh, ww, false, nullptr, c.ZSP(rb.conv2)));
  // h = relu(BN1(conv1(x))) [+ skip(x)] + temb
  RUN(drs_launch_colsum(gH, co, 0, co, npix, (long long)hh * ww, 1, plan->temb_total, c.dtemb + rb.mlp.temb_off, c.s));
  if (rb.has_skip) {
    RUN(wgrad(c, rb.skip, wgrad_conv(u, ci, 0, ci, hh, ww, gH, co, 0, co, hh, ww, B, 3, 1, 1)));
    RUN(run_dgrad(c, rb.skip, gH, co, 0, B, hh, ww, gu, gu_cs, 0, hh, ww, true));
  }
  RUN(bn_bwd(c, rb.conv1, gH, co, 0, 1, npix));
  RUN(wgrad(c, rb.conv1, wgrad_conv(u, ci, 0, ci, hh, ww, c.TP(rb.conv1.t_Z), co, 0, co, hh, ww, B, 3, 1, 1)));
  RUN(run_dgrad(c, rb.conv1, c.TP(rb.conv1.t_Z), co, 0, B, hh, ww, gu, gu_cs, 0, hh, ww, true, nullptr, c.ZSP(rb.conv1)));
  if (i > 0) {  // downs[i-1]: 3x3 s2 conv from R[i-1] to D[i-1]
    const ConvLayer& L = plan->downs[i - 1];
    const int cd = kDown[i], ph = c.H >> (i - 1), pw = c.W >> (i - 1);
    RUN(wgrad(c, L, wgrad_conv(c.TP(plan->t_R[i - 1]), cd, 0, cd, ph, pw, gu, cd, 0, cd, hh, ww, B, 3, 2, 1)));
    RUN(run_dgrad(c, L, gu, cd, 0, B, hh, ww, c.TP(plan->g_R[i - 1]), cd, 0, ph, pw, c.gR_written[i - 1]));
    c.gR_written[i - 1] = true;
  }
  return DRS_OK;
}

// ---- stem: x0 = conv0(x) + cond (:342-355); conv0's weight gradient ----
static int bwd_stem(BwdCtx& c, const float* x) {
  const int C = c.cfg.image_channels;
  float* xn = c.TP(c.plan->t_xn);  // x as channels-last
  RUN(drs_launch_nchw_to_nhwc(x, xn, c.B, C, c.H, c.W, C, 0, c.s));
  return stem_wgrad(c, c.plan->stem0,
                    wgrad_conv(xn, C, 0, C, c.H, c.W, c.TP(c.plan->g_x0), kGx0Stride, 0, kDown[0], c.H, c.W, c.B, 3, 1, 1));
}

// ---- LR branch: cond = conv_upsampled_lr_img(bicubic(RRDB(lr))) (:342-355) ----
// d(up) = conv^T(gx0), adjoint bicubic, RRDB backward (all CC-channel tensors, channels-last copies)
static int bwd_lr_branch(BwdCtx& c) {
  const drs_plan* plan = c.plan;
  const int B = c.B, H = c.H, W = c.W, CC = c.cfg.cond_channels;
  float* gx0 = c.TP(plan->g_x0);
  float* upn = c.TP(plan->t_upn);  // up-sampled LR encoding as channels-last
  RUN(drs_launch_nchw_to_nhwc(c.TP(plan->t_up), upn, B, CC, H, W, CC, 0, c.s));
  RUN(stem_wgrad(c, plan->stemc, wgrad_conv(upn, CC, 0, CC, H, W, gx0, kGx0Stride, 0, kDown[0], H, W, B, 3, 1, 1)));
  float* gup = c.TP(plan->g_upn);
  // dgrad of the CC -> 16 conditioning convolution (its own LDS-tiled kernel: stem_bwd.hip)
  RUN(drs_launch_stem_dgrad(gx0, kGx0Stride, c.PARAM(plan->stemc.w), gup, B, H, W, CC, c.s));
  float* genc = c.TP(plan->g_lr[3]);  // gradient w.r.t. the LR encoding (h x w)
  RUN(drs_launch_bicubic_bwd(gup, genc, B, CC, c.h, c.w, c.cfg.magnification, c.s));  // (gather form: writes every element)
  // RRDB (:237-260): enc = conv_out(r3) + lr;  r_{b+1} = conv2_b(relu(conv1_b(r_b))) + r_b
  // conv_out: input r3
  float* gr = c.TP(plan->g_lr[2]);  // running gradient w.r.t. r_b
  RUN(small_bwd(c, plan->rrdb[6], c.TP(plan->t_rn[3]), genc, gr, false, nullptr));
  for (int b = 2; b >= 0; --b) {
    // r_{b+1} = conv2(a_b) + r_b, a_b = relu(conv1(r_b)): g(a_b) = conv2^T gr; g(r_b) = gr + conv1^T(g(a_b) * mask)
    float* ga = c.TP(plan->g_lr[0]);
    RUN(small_bwd(c, plan->rrdb[2 * b + 1], c.TP(plan->t_an[b]), gr, ga, false, c.TP(plan->t_an[b])));
    RUN(small_bwd(c, plan->rrdb[2 * b], c.TP(plan->t_rn[b]), ga, gr, true, nullptr));
  }
  return DRS_OK;
}

// ---- time-embedding MLPs ----
static int bwd_time_mlps(BwdCtx& c, const int64_t* t, const int64_t* labels, int label_batch) {
  const drs_plan* plan = c.plan;
  DrsMlpBwdTable tab = {};
  float* dlabel = labels ? c.G(plan->label_emb) : nullptr;
  for (Mlp* m : plan->mlps) {
    // an MLP takes part when any of its four gradients is wanted, or the label gradient (every MLP adds its share to it)
    if (!c.G(m->w1) && !c.G(m->b1) && !c.G(m->w2) && !c.G(m->b2) && !dlabel) continue;
    DRS_REQUIRE(tab.n < 8, DRS_ERR_SHAPE, "backward: more than 8 time MLPs");
    tab.m[tab.n++] = DrsMlpBwd{c.PARAM(m->w1), c.PARAM(m->b1), c.PARAM(m->w2), c.temb + m->temb_off, c.dtemb + m->temb_off,
                               c.G(m->w1), c.G(m->b1), c.G(m->w2), c.G(m->b2), m->dim};
  }
  return drs_launch_time_mlp_bwd((const long long*)t, (const float*)(c.pk + plan->o_inv_freq), tab, plan->temb_total, c.B,
                                 labels ? c.PARAM(plan->label_emb) : nullptr, (const long long*)labels, label_batch,
                                 c.cfg.num_classes, dlabel, c.s);
}

extern "C" int drs_unet_backward(drs_plan* plan, const void* packed, void* packed_bwd, size_t packed_bwd_bytes,
                                 const float* x, const int64_t* t, const float* dout, float* const* grads,
                                 void* workspace, size_t workspace_bytes, drs_stream_t stream) {
  return drs_unet_backward_labels(plan, packed, packed_bwd, packed_bwd_bytes, x, t, nullptr, 0, dout, grads, workspace,
                                  workspace_bytes, stream);
}

extern "C" int drs_unet_backward_labels(drs_plan* plan, const void* packed, void* packed_bwd, size_t packed_bwd_bytes,
                                        const float* x, const int64_t* t, const int64_t* labels, int label_batch,
                                        const float* dout, float* const* grads, void* workspace, size_t workspace_bytes,
                                        drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(plan && packed && packed_bwd && x && t && dout && grads && workspace, DRS_ERR_ARG, "backward: null pointer");
  DRS_REQUIRE(plan->cfg.flags & DRS_PLAN_TRAIN, DRS_ERR_STATE, "backward: not a train plan");
  DRS_REQUIRE(plan->packed_ok && plan->packed_ptr == packed, DRS_ERR_STATE, "backward: weights not packed");
  DRS_REQUIRE(plan->cfg.lr_batch == plan->cfg.batch, DRS_ERR_SHAPE, "backward: lr_img batch must equal the batch");
  const bool has_cond = plan->cfg.variant != DRS_VARIANT_GENERATION;
  DRS_REQUIRE(!labels || (plan->label_emb >= 0 && (label_batch == plan->cfg.batch || label_batch == 1)), DRS_ERR_ARG,
              "backward: labels need the generation variant with num_classes > 0 and label_batch == batch or 1");
  DRS_REQUIRE(workspace_bytes >= plan->ws_bytes, DRS_ERR_WORKSPACE, "backward: workspace too small");
  DRS_REQUIRE(packed_bwd_bytes >= drs_unet_packed_bwd_bytes(plan), DRS_ERR_WORKSPACE, "backward: packed_bwd too small");
  BwdCtx c(plan, packed, packed_bwd, workspace, grads, s, bwd_impl(plan->cfg.impl));
  RUN(bwd_pack_dgrad_images(c));
  RUN(bwd_zero_grads(c));

  // Weight gradients (MFMA kernel, split bf16 by default: DRS_TRAIN_WGRAD_IMPL; direct plans run the VALU kernel in line)
  // never feed the backward chain, and their operands (saved activations, the dY / dZ tensor of the layer) are not touched
  // again once the call is issued: MFMA plans run them on the plan's side stream, overlapping the HBM-bound BatchNorm /
  // mask / column-sum kernels of the main chain (the partial-slice workspace serialises them among themselves).  The main
  // stream waits for the side stream at the end.
  static const bool wgrad_side_env = !(getenv("DRS_WGRAD_STREAM") && atoi(getenv("DRS_WGRAD_STREAM")) == 0);
  c.wgrad_side = wgrad_side_env && c.wgrad_mfma;
  if (c.wgrad_side && !plan->side) {
    DRS_CHECK_HIP(hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking));
    for (hipEvent_t* e : {&plan->ev_fork, &plan->ev_join, &plan->ev_gbias})
      DRS_CHECK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }

  RUN(bwd_head(c, dout));
  for (int i = 2; i >= 0; --i) RUN(bwd_decoder_stage(c, i));
  for (int i = 3; i >= 0; --i) RUN(bwd_encoder_block(c, i));
  RUN(bwd_stem(c, x));
  if (has_cond) RUN(bwd_lr_branch(c));
  RUN(bwd_time_mlps(c, t, labels, label_batch));
  if (c.wgrad_side) {  // all weight gradients are complete before the caller's stream continues (optimizer, next forward)
    DRS_CHECK_HIP(hipEventRecord(plan->ev_join, plan->side));
    DRS_CHECK_HIP(hipStreamWaitEvent(s, plan->ev_join, 0));
  }
  return DRS_OK;
}
