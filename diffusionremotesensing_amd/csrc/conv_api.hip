// C-ABI of include/drs_hip.h: the TapConv builders every schedule uses and the two operator-level entries (NCHW boundary),
// the convolution and the fused up-sampling stage.
#include "unet_plan.h"

// ------------------------------------------------------------------------------------------------
// TapConv builders
// ------------------------------------------------------------------------------------------------
namespace drs_unet {
TapConv conv_desc(const float* in, int N, int H, int W, int Cin, int in_cs, int in_co, const float* w,
                         const float* bias, float* out, int Cout, int out_cs, int out_co, int KH, int KW, int stride,
                         int pad) {
  TapConv d = {};
  d.in = in; d.in_cs = in_cs; d.in_co = in_co;
  d.N = N; d.H = H; d.W = W; d.Cin = Cin;
  d.w = w; d.bias = bias;
  d.out = out; d.out_cs = out_cs; d.out_co = out_co;
  d.OH = (H + 2 * pad - KH) / stride + 1;
  d.OW = (W + 2 * pad - KW) / stride + 1;
  d.Cout = Cout;
  d.TH = d.OH; d.TW = d.OW;
  d.in_stride = stride; d.out_scale = 1; d.out_oy = 0; d.out_ox = 0;
  d.ntaps = KH * KW;
  d.wtaps_total = KH * KW;
  for (int ky = 0; ky < KH; ++ky)
    for (int kx = 0; kx < KW; ++kx) {
      const int i = ky * KW + kx;
      d.dy[i] = ky - pad; d.dx[i] = kx - pad; d.wtap[i] = i;
    }
  return d;
}

// Phase (py,px) of ConvTranspose2d(k=3, s=2, p=1, output_padding=1): out[2*iy - 1 + ky] += in[iy] * w[ky]
// (reference UpConvBlock.transform, UNet_model_superres.py:185).  Even output rows take ky=1 from iy=t; odd rows
// take ky=0 from iy=t+1 and ky=2 from iy=t.  Output is (2H, 2W).
TapConv convT_phase_desc(const float* in, int N, int H, int W, int Cin, int in_cs, int in_co, const float* w,
                                const float* bias, float* out, int Cout, int out_cs, int out_co, int py, int px) {
  TapConv d = {};
  d.in = in; d.in_cs = in_cs; d.in_co = in_co;
  d.N = N; d.H = H; d.W = W; d.Cin = Cin;
  d.w = w; d.bias = bias;
  d.out = out; d.out_cs = out_cs; d.out_co = out_co;
  d.OH = 2 * H; d.OW = 2 * W; d.Cout = Cout;
  d.TH = H; d.TW = W;
  d.in_stride = 1; d.out_scale = 2; d.out_oy = py; d.out_ox = px;
  d.wtaps_total = 9;
  int ydy[2], yk[2], ny, xdx[2], xk[2], nx;
  if (py == 0) { ny = 1; ydy[0] = 0; yk[0] = 1; } else { ny = 2; ydy[0] = 1; yk[0] = 0; ydy[1] = 0; yk[1] = 2; }
  if (px == 0) { nx = 1; xdx[0] = 0; xk[0] = 1; } else { nx = 2; xdx[0] = 1; xk[0] = 0; xdx[1] = 0; xk[1] = 2; }
  int i = 0;
  for (int a = 0; a < ny; ++a)
    for (int b = 0; b < nx; ++b, ++i) {
      d.dy[i] = ydy[a]; d.dx[i] = xdx[b]; d.wtap[i] = yk[a] * 3 + xk[b];
    }
  d.ntaps = i;
  return d;
}

// All four phases in one MFMA launch: TH x TW = input size, out_scale 2, the 9 weight taps in storage order.
TapConv convT_fused_desc(const float* in, int N, int H, int W, int Cin, int in_cs, int in_co, const float* w,
                                const float* bias, float* out, int Cout, int out_cs, int out_co) {
  TapConv d = convT_phase_desc(in, N, H, W, Cin, in_cs, in_co, w, bias, out, Cout, out_cs, out_co, 1, 1);
  d.mode = DRS_TAPMODE_CONVT;
  d.out_oy = 0; d.out_ox = 0;
  d.ntaps = 9;
  for (int i = 0; i < 9; ++i) { d.dy[i] = 0; d.dx[i] = 0; d.wtap[i] = i; }
  return d;
}

// impl is the family the weights of this layer were packed for: no silent switch at launch time
int run_conv(const TapConv& d, int impl, hipStream_t s) {
  if (impl != DRS_IMPL_DIRECT) return drs_launch_tapconv_mfma(d, impl, s);
  return drs_launch_tapconv_direct(d, s);
}
// algorithmic work of one tap-convolution (SURVEY.md 8(d) model: 2*MACs; fp32 input + output + weights)
double conv_flops(const TapConv& d) {
  return 2.0 * d.N * d.TH * d.TW * (double)d.Cout * ((double)d.Cin * d.ntaps + (d.in2 ? d.Cin2 : 0));
}
double conv_bytes(const TapConv& d) {
  const double in = (double)d.N * d.H * d.W * d.Cin;
  const double out = (double)d.N * d.TH * d.TW * d.Cout * (d.mode == DRS_TAPMODE_CONVT ? 4 : 1);
  const double in2 = d.in2 ? (double)d.N * d.H2 * d.W2 * d.Cin2 + (double)d.Cin2 * d.Cout : 0.0;
  return 4.0 * (in + in2 + out + (double)d.ntaps * d.Cin * d.Cout);
}
}  // namespace drs_unet

// ------------------------------------------------------------------------------------------------
// operator-level convolution (NCHW boundary)
// ------------------------------------------------------------------------------------------------
static bool conv_flavour_ok(int KH, int KW, int stride, int pad, int transposed, int out_pad) {
  if (transposed) return KH == 3 && KW == 3 && stride == 2 && pad == 1 && out_pad == 1;
  if (KH == 3 && KW == 3 && pad == 1 && (stride == 1 || stride == 2)) return true;
  if (KH == 1 && KW == 1 && pad == 0 && stride == 1) return true;
  if (KH == 2 && KW == 2 && pad == 0 && stride == 2) return true;
  return false;
}
static void conv_out_hw(int H, int W, int KH, int KW, int stride, int pad, int transposed, int out_pad, int* OH,
                        int* OW) {
  if (transposed) {
    *OH = (H - 1) * stride - 2 * pad + KH + out_pad;
    *OW = (W - 1) * stride - 2 * pad + KW + out_pad;
  } else {
    *OH = (H + 2 * pad - KH) / stride + 1;
    *OW = (W + 2 * pad - KW) / stride + 1;
  }
}

extern "C" size_t drs_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad,
                                             int transposed, int out_pad) {
  int OH, OW;
  conv_out_hw(H, W, KH, KW, stride, pad, transposed, out_pad, &OH, &OW);
  size_t b = 0;
  b += align_up((size_t)N * H * W * Cin * 4);
  b += align_up((size_t)N * OH * OW * Cout * 4);
  b += align_up(drs_pack_conv_mfma_bytes(Cout, Cin, KH * KW, DRS_IMPL_MFMA_BF16X3) + (size_t)Cout * Cin * KH * KW * 4);
  b += align_up((size_t)Cout * 4);
  return b + 256;
}

extern "C" int drs_conv2d_nchw(const float* x, const float* w, const float* b, float* y, int N, int Cin, int H, int W,
                               int Cout, int KH, int KW, int stride, int pad, int transposed, int out_pad, int relu,
                               void* workspace, size_t workspace_bytes, int impl, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return DRS_OK;  // empty batch: nothing to do (torch hands out null pointers for empty tensors)
  DRS_REQUIRE(x && w && y && workspace, DRS_ERR_ARG, "conv2d: null pointer");
  DRS_REQUIRE(N >= 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, DRS_ERR_SHAPE, "conv2d: bad dims");
  DRS_REQUIRE(conv_flavour_ok(KH, KW, stride, pad, transposed, out_pad), DRS_ERR_SHAPE,
              "conv2d: unsupported flavour k=%dx%d s=%d p=%d transposed=%d out_pad=%d", KH, KW, stride, pad, transposed,
              out_pad);
  DRS_REQUIRE(impl >= DRS_IMPL_DIRECT && impl <= DRS_IMPL_MFMA_F16, DRS_ERR_ARG, "conv2d: impl=%d", impl);
  DRS_REQUIRE(workspace_bytes >= drs_conv2d_workspace_bytes(N, Cin, H, W, Cout, KH, KW, stride, pad, transposed, out_pad),
              DRS_ERR_WORKSPACE, "conv2d: workspace too small");
  int OH, OW;
  conv_out_hw(H, W, KH, KW, stride, pad, transposed, out_pad, &OH, &OW);
  DRS_REQUIRE(OH > 0 && OW > 0, DRS_ERR_SHAPE, "conv2d: empty output");
  char* base = aligned_base(workspace);
  float* xin = (float*)base; base += align_up((size_t)N * H * W * Cin * 4);
  float* yout = (float*)base; base += align_up((size_t)N * OH * OW * Cout * 4);
  float* pw = (float*)base;
  base += align_up(drs_pack_conv_mfma_bytes(Cout, Cin, KH * KW, DRS_IMPL_MFMA_BF16X3) + (size_t)Cout * Cin * KH * KW * 4);
  float* pb = (float*)base;
  int rc;
  if ((rc = drs_launch_nchw_to_nhwc(x, xin, N, Cin, H, W, Cin, 0, s))) return rc;

  // decide the kernel family on a probe descriptor, then pack in that family's layout
  TapConv probe = transposed ? convT_fused_desc(xin, N, H, W, Cin, Cin, 0, pw, pb, yout, Cout, Cout, 0)
                             : conv_desc(xin, N, H, W, Cin, Cin, 0, pw, pb, yout, Cout, Cout, 0, KH, KW, stride, pad);
  const bool mfma = impl != DRS_IMPL_DIRECT && drs_tapconv_mfma_supported(probe, impl);
  if (mfma)
    rc = drs_launch_pack_conv_mfma(w, b, nullptr, nullptr, nullptr, nullptr, 0.f, pw, pb, Cout, Cin, KH * KW, transposed,
                                   impl, s);
  else
    rc = drs_launch_pack_conv(w, b, nullptr, nullptr, nullptr, nullptr, 0.f, pw, pb, Cout, Cin, KH * KW, transposed, 0, s);
  if (rc) return rc;
  const int use_impl = mfma ? impl : DRS_IMPL_DIRECT;
  if (!transposed) {
    TapConv d = probe;
    d.relu_pre = relu;
    if ((rc = run_conv(d, use_impl, s))) return rc;
  } else if (mfma) {
    TapConv d = convT_fused_desc(xin, N, H, W, Cin, Cin, 0, pw, pb, yout, Cout, Cout, 0);
    d.relu_pre = relu;
    if ((rc = run_conv(d, use_impl, s))) return rc;
  } else {
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        TapConv d = convT_phase_desc(xin, N, H, W, Cin, Cin, 0, pw, pb, yout, Cout, Cout, 0, py, px);
        d.relu_pre = relu;
        if ((rc = run_conv(d, use_impl, s))) return rc;
      }
  }
  return drs_launch_nhwc_to_nchw(yout, y, N, Cout, OH, OW, Cout, 0, s);
}

// ------------------------------------------------------------------------------------------------
// operator-level fused up-sampling stage (NCHW boundary): y = conv3x3(cat[conv_transpose(h), att])
// ------------------------------------------------------------------------------------------------
namespace drs_unet {
// t_w / t_b: ups.i.transform, v_w / v_b: up_convs.i, out_w / out_b / out_dim: the `output` projection (folded forms), res: the
// weight, bias and BatchNorm gamma, beta, mean, var of attention_blocks.2.result (ah_tmp2), perm: SP output rows of the att-half
int pack_upfuse_stage_images(const UpfuseDst& d, const float* t_w, const float* t_b, const float* v_w, const float* v_b,
                                    const float* out_w, const float* out_b, int out_dim, const float* const* res, float eps,
                                    int Cc, int Ch, int impl, int perm, hipStream_t s) {
  const float *uv_w = v_w, *uv_b = v_b;
  if (d.uf_tmpw) {  // `output` folded into up_convs.2: the composite, its edge weights and its bias are built from the folded layer
    RUN(drs_launch_upfuse_fold_proj(v_w, v_b, out_w, out_b, out_dim, Cc, Ch, d.uf_tmpw, d.uf_tmpb, s));
    uv_w = d.uf_tmpw; uv_b = d.uf_tmpb;
    RUN(drs_launch_upfuse_proj_pack(uv_w, t_w, Cc, Ch, out_dim, d.ufp_w, s));
  }
  RUN(drs_launch_upfuse_pack(uv_w, uv_b, t_w, t_b, Cc, Ch, d.w, d.aux, d.edge, s));
  // att-half: input channels [Cc, Cc + Ch) of up_convs.i, zero bias (it is in the composite's) - or, folded: output o
  // up_convs.2[att half] is ONE 3x3 convolution Ch -> out_dim (reference :377,:379: no activation or normalisation between
  // the two), half the MFMAs of the 32-channel form
  if (!d.ah_tmp)
    return drs_launch_pack_conv_mfma(v_w, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, d.ah_w, d.ah_b, Ch, Ch, 9, 0, impl, s,
                                     {.perm = perm, .cin_total = Cc + Ch, .cin_off = Cc});
  const float* tmp = d.ah_tmp;
  RUN(drs_launch_fold_proj(v_w, Cc + Ch, Cc, Ch, Ch, out_w, out_dim, d.ah_tmp, s));
  if (d.ah_tmp2) {  // ... o attention_blocks.2.result (1x1 + BatchNorm, linear): the convolution then reads psi * x_res
    RUN(drs_launch_fold_result(d.ah_tmp, Ch, res[0], res[1], res[2], res[3], res[4], res[5], eps, d.ah_tmp2, d.ah_tab, s));
    tmp = d.ah_tmp2;
  }
  return drs_launch_pack_conv_mfma(tmp, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, d.ah_w, d.ah_b, 16, Ch, 3, 0, impl, s);
}
}  // namespace drs_unet

// Workspace of drs_upconv_fused_nchw: byte offsets from its 256-aligned base
struct UpfusedWs {
  size_t h, att, part, res;          // SP copies of h and att, att-half partial sums, result (SP)
  size_t w, aux, ah_w, ah_b;         // composite image, edge / bias weights, att-half image and bias
  size_t eh, ev, zero, edge;         // edge vectors, zero line + fault word, edge operand image
  size_t ah_tmp, uf_tmpw, uf_tmpb, ufp_w;  // folded output projection (fuse_w, shapes the direct kernel takes)
  size_t bytes;
};
static UpfusedWs upfused_layout(int N, int Cc, int Ch, int LH, int LW) {
  const size_t hi = (size_t)N * 4 * LH * LW;
  UpfusedWs o;
  size_t b = 0;
  o.h = b; b += align_up((size_t)N * LH * LW * Cc * 4);
  o.att = b; b += align_up(hi * Ch * 4);
  o.part = b; b += align_up(hi * Ch * 4);
  o.res = b; b += align_up(hi * Ch * 4);
  o.w = b; b += align_up(drs_upfuse_weight_bytes(Cc, Ch));
  o.aux = b; b += align_up(drs_upfuse_aux_floats(Cc, Ch) * 4);
  o.ah_w = b; b += align_up(drs_pack_conv_mfma_bytes(Ch, Ch, 9, DRS_IMPL_MFMA_BF16X3));
  o.ah_b = b; b += align_up((size_t)Ch * 4);
  o.eh = b; b += align_up((size_t)N * 2 * 2 * LW * Ch * 4);
  o.ev = b; b += align_up((size_t)N * 2 * 2 * LH * Ch * 4);
  o.zero = b; b += 512;
  o.edge = b; b += align_up(drs_upfuse_edge_image_bytes(Cc, Ch));
  o.ah_tmp = b; b += align_up((size_t)16 * Ch * 9 * 4);
  o.uf_tmpw = b; b += align_up((size_t)32 * (Cc + Ch) * 9 * 4);
  o.uf_tmpb = b; b += align_up((size_t)32 * 4);
  o.ufp_w = b; b += align_up(drs_upfuse_proj_weight_bytes(Cc > 64 ? 64 : Cc));
  o.bytes = b + 256;
  return o;
}
extern "C" size_t drs_upconv_fused_workspace_bytes(int N, int Cc, int Ch, int LH, int LW) { return upfused_layout(N, Cc, Ch, LH, LW).bytes; }
extern "C" int drs_upconv_fused_nchw(const float* h, const float* att, const float* t_w, const float* t_b, const float* v_w,
                                     const float* v_b, const float* post2, const float* fuse_w, const float* fuse_b,
                                     int fuse_dim, float* y, float* y2, int N, int Cc, int Ch, int LH, int LW, void* workspace,
                                     size_t workspace_bytes, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return DRS_OK;
  DRS_REQUIRE(h && att && t_w && t_b && v_w && v_b && y && workspace, DRS_ERR_ARG, "upconv_fused: null pointer");
  DRS_REQUIRE(N > 0 && LH > 0 && LW > 0 && Cc >= 32 && Ch >= 32 && Cc % 32 == 0 && Ch % 32 == 0, DRS_ERR_SHAPE,
              "upconv_fused: N=%d Cc=%d Ch=%d LH=%d LW=%d (channel counts must be multiples of 32)", N, Cc, Ch, LH, LW);
  DRS_REQUIRE(!fuse_w || (Ch == 32 && fuse_dim >= 1 && fuse_dim <= 4 && fuse_b && !post2 && !y2), DRS_ERR_SHAPE,
              "upconv_fused: the fused projection needs Ch == 32, fuse_dim <= 4 and no second output");
  DRS_REQUIRE((post2 == nullptr) == (y2 == nullptr), DRS_ERR_ARG, "upconv_fused: post2 and y2 come together");
  const UpfusedWs o = upfused_layout(N, Cc, Ch, LH, LW);
  DRS_REQUIRE(workspace_bytes >= o.bytes, DRS_ERR_WORKSPACE, "upconv_fused: workspace too small");
  char* base = aligned_base(workspace);
  auto at = [base](size_t off) { return (float*)(base + off); };
  const int OH = 2 * LH, OW = 2 * LW;
  DRS_CHECK_HIP(hipMemsetAsync(base + o.zero, 0, 512, s));
  RUN(drs_launch_nchw_to_sp(h, at(o.h), N, Cc, LH, LW, s));
  RUN(drs_launch_nchw_to_sp(att, at(o.att), N, Ch, OH, OW, s));
  // the projection folded into both launches' weights where the direct kernel takes the att-half (what the plan's stage 2
  // does: DecStage::ah_proj / uf_proj), else as the matrix-pipe epilogue of the 32-channel layer
  bool fold = false;
  TapConv ah = conv_desc(at(o.att), N, OH, OW, Ch, Ch, 0, at(o.ah_w), nullptr, nullptr, 16, 16, 0, 3, 3, 1, 1);
  if (fuse_w) {
    ah.in_sp = 1; ah.zero_line = base + o.zero; ah.proj = 1; ah.fuse_out = y; ah.fuse_dim = fuse_dim;
    fold = drs_conv3x3_direct_sp_proj_supported(ah, DRS_IMPL_MFMA_BF16X3) && drs_upfuse_proj_supported(Cc, Ch, fuse_dim);
  }
  UpfuseDst pd = {base + o.w, at(o.aux), base + o.edge, base + o.ah_w, at(o.ah_b)};
  if (fold) { pd.ah_tmp = at(o.ah_tmp); pd.uf_tmpw = at(o.uf_tmpw); pd.uf_tmpb = at(o.uf_tmpb); pd.ufp_w = base + o.ufp_w; }
  RUN(pack_upfuse_stage_images(pd, t_w, t_b, v_w, v_b, fuse_w, fuse_b, fuse_dim, nullptr, 0.f, Cc, Ch, DRS_IMPL_MFMA_BF16X3,
                               fuse_w ? 0 : 1, s));
  const float* aux = at(o.aux);
  const size_t mat = (size_t)Cc * Ch;
  unsigned* fault = (unsigned*)(base + o.zero + 256);
  UpFuseEdgeDesc e = {};
  e.in = at(o.h); e.in_cs = Cc; e.in_co = 0;
  e.N = N; e.LH = LH; e.LW = LW; e.Cc = Cc; e.Ch = Ch;
  e.rt = aux; e.rl = aux + 5 * mat; e.bt = aux + 11 * mat;
  e.eh = at(o.eh); e.ev = at(o.ev);
  e.wimg = base + o.edge; e.zero_line = base + o.zero;
  RUN(drs_launch_upfuse_edges(e, s));
  if (fold) {
    RUN(drs_launch_conv3x3_direct_sp(ah, s));
  } else {
    TapConv d = conv_desc(at(o.att), N, OH, OW, Ch, Ch, 0, at(o.ah_w), at(o.ah_b), at(o.part), Ch, Ch, 0, 3, 3, 1, 1);
    d.in_sp = d.out_sp = 1; d.zero_line = base + o.zero; d.fault = fault;
    if (fuse_w) {  // projected att-half straight into y (the plan's stage 2)
      d.out = nullptr; d.out_sp = 0;
      d.fuse_w = fuse_w; d.fuse_b = at(o.ah_b); d.fuse_out = y; d.fuse_dim = fuse_dim;
    }
    RUN(drs_launch_tapconv_mfma(d, DRS_IMPL_MFMA_BF16X3, s));
  }
  UpFuseDesc u = {};
  u.in = at(o.h); u.in_cs = Cc; u.in_co = 0;
  u.N = N; u.LH = LH; u.LW = LW; u.Cc = Cc; u.Ch = Ch;
  u.w = base + (fold ? o.ufp_w : o.w);
  u.bias = aux + 11 * mat + 9 * Ch;
  u.res = at(o.part); u.res_cs = Ch; u.res_co = 0;
  u.eh = at(o.eh); u.ev = at(o.ev);
  u.zero_line = base + o.zero; u.fault = fault;
  if (fuse_w) {
    u.res = nullptr; u.fuse_acc = 1;
    if (fold) u.proj = 1;
    else { u.fuse_w = fuse_w; u.fuse_b = fuse_b; }
    u.fuse_out = y; u.fuse_dim = fuse_dim;
  } else {
    u.out = at(o.res); u.out_cs = Ch; u.out_co = 0;
    if (y2) { u.out2 = at(o.att); u.out2_cs = Ch; u.out2_co = 0; u.post2 = post2; u.post2_cs = Ch; }  // (att is consumed by now)
  }
  RUN(fold ? drs_launch_upfuse_proj(u, s) : drs_launch_upfuse(u, s));
  if (!fuse_w) {
    RUN(drs_launch_sp_to_nchw(at(o.res), y, N, Ch, OH, OW, Ch, 0, s));
    if (y2) RUN(drs_launch_sp_to_nchw(at(o.att), y2, N, Ch, OH, OW, Ch, 0, s));
  }
  unsigned word = 0;
  DRS_CHECK_HIP(hipMemcpyAsync(&word, fault, 4, hipMemcpyDeviceToHost, s));
  DRS_CHECK_HIP(hipStreamSynchronize(s));
  DRS_REQUIRE(word == 0, DRS_ERR_HIP, "upconv_fused: a wave-specialised kernel timed out on an LDS counter (protocol fault)");
  return DRS_OK;
}
