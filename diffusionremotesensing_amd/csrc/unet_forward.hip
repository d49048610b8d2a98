// C-ABI of include/drs_hip.h: the launch schedule of one UNet forward (eval and train plans) and the fault check.
#include <stdlib.h>

#include "unet_plan.h"

static int plan_conv(drs_plan* plan, const ConvLayer& L, const TapConv& d_in, hipStream_t s) {
  // second output (TapConv::out2): written by the wave-specialised SP kernel's epilogue; shapes that kernel does not
  // take get it from a separate pass over the first output
  TapConv d = d_in;
  d.fault = plan->fault_ptr;
  if (L.fl_ok && !plan->fl_disabled && !d.w_fl) d.w_fl = aligned_base(plan->packed_ptr) + L.fl_img_off;
  const bool split_out2 = d.out2 && !drs_tapconv_sp_supported(d, plan->cfg.impl) && !drs_tapconv_sp8_supported(d, plan->cfg.impl);
  if (split_out2) d.out2 = nullptr;
  std::string name = plan->params[L.w].name;
  name = name.substr(0, name.size() - 7);  // strip ".weight"
  if (d.out_scale == 2 && d.mode != DRS_TAPMODE_CONVT) name += ".phase" + std::to_string(d.out_oy * 2 + d.out_ox);
  prof_begin(plan, name, conv_flops(d), conv_bytes(d), s);
  int rc = run_conv(d, L.mfma ? plan->cfg.impl : DRS_IMPL_DIRECT, s);
  if (!rc && split_out2)
    rc = drs_launch_sp_add_rowvec(d_in.out, d_in.out2, d_in.post2, d_in.post2_cs, d_in.N, (long long)d_in.OH * d_in.OW,
                                  d_in.Cout, s);
  prof_end(plan, s);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// forward schedule
// ------------------------------------------------------------------------------------------------
namespace {
// What every step of one forward reads.  concurrent / mlp_side are decided on each call (drs_unet_profile_enable changes
// them); xt_only by the time-embedding step, and the bottleneck's probe may clear xt_only[0] again.
struct FwdCtx {
  drs_plan* plan;
  const drs_unet_config& cfg;
  hipStream_t s;
  char* pk;  // packed weights (aligned base)
  void* ws;  // workspace (aligned base)
  float* temb;
  const void* zero_line;
  float* out;
  int B, H, W, sp;  // sp: SP-format activations (eval, split-bf16)
  bool train;
  bool concurrent = false, mlp_side = false;
  bool xt_only[3] = {false, false, false};
  FwdCtx(drs_plan* p, const void* packed, void* workspace, float* o, hipStream_t stream)
      : plan(p), cfg(p->cfg), s(stream), pk(aligned_base(packed)), ws(aligned_base(workspace)),
        temb((float*)((char*)ws + p->o_temb)), zero_line(pk + p->o_zero), out(o), B(cfg.batch), H(cfg.height),
        W(cfg.width), sp(p->sp ? 1 : 0), train((cfg.flags & DRS_PLAN_TRAIN) != 0) {}
  const float* PW(const ConvLayer& L) const { return (const float*)(pk + L.w_off); }
  const float* PB(const ConvLayer& L) const { return (const float*)(pk + L.b_off); }
  float* TP(int i) const { return plan->tp(ws, i); }
  bool keep_all() const { return (cfg.flags & DRS_PLAN_KEEP_ALL) != 0; }
};
}  // namespace

// A convolution followed by BatchNorm.  Eval: BatchNorm is folded into the weights, one launch.  Train: the raw
// convolution writes Z (input add and gate act before the norm and stay in the conv), then batch statistics,
// running-stat update and the normalisation carry the rest of the block's epilogue.
static int conv_bn(FwdCtx& f, const ConvLayer& L, const TapConv& d) {
  if (!f.train) return plan_conv(f.plan, L, d, f.s);
  TapConv zc = d;
  zc.out = f.TP(L.t_Z); zc.out_cs = L.Cout; zc.out_co = 0;
  zc.relu_pre = zc.relu_post = 0; zc.post_add = nullptr; zc.res = nullptr;
  zc.in2 = nullptr; zc.w2 = nullptr; zc.bias2 = nullptr;
  RUN(plan_conv(f.plan, L, zc, f.s));
  float* stats = (float*)((char*)f.ws + L.stats_off);
  const long long ppi = (long long)d.OH * d.OW;
  std::string name = f.plan->params[L.bn].name;
  name = name.substr(0, name.size() - 7);  // strip ".weight"
  // (algorithmic bytes: Z read once for the statistics and once for the normalisation, or only the latter; the output written)
  const double zbytes = 4.0 * d.N * ppi * L.Cout;
  if (f.plan->frozen_bn())  // running statistics into the mean | rstd slot (per forward: they may have been loaded since), no pass over Z
    return prof_op(f.plan, name + ".frozen", 0, 2.0 * zbytes, f.s, [&] {
      return drs_launch_bn_frozen(zc.out, L.Cout, 0, (long long)d.N * ppi, ppi, L.Cout,
                                  (const float*)f.plan->param_ptrs[L.bn], (const float*)f.plan->param_ptrs[L.bn + 1],
                                  (const float*)f.plan->param_ptrs[L.bn + 2], (const float*)f.plan->param_ptrs[L.bn + 3],
                                  f.cfg.bn_eps, stats, stats + L.Cout, d.post_add, d.post_cs, d.res, d.res_cs, d.res_co,
                                  d.out, d.out_cs, d.out_co, d.relu_pre, d.relu_post, f.s);
    });
  return prof_op(f.plan, name + ".train", 0, 3.0 * zbytes, f.s, [&] {
    return drs_launch_bn_train(zc.out, L.Cout, 0, (long long)d.N * ppi, ppi, L.Cout,
                               (const float*)f.plan->param_ptrs[L.bn], (const float*)f.plan->param_ptrs[L.bn + 1],
                               (float*)f.plan->param_ptrs[L.bn + 2], (float*)f.plan->param_ptrs[L.bn + 3], f.cfg.bn_eps,
                               0.1f, (double*)((char*)f.ws + f.plan->o_red), stats, stats + L.Cout, d.post_add, d.post_cs,
                               d.res, d.res_cs, d.res_co, d.out, d.out_cs, d.out_co, d.relu_pre, d.relu_post, f.s);
  });
}
// --- time embeddings for the 7 blocks (reference :338-339 + every time_mlp) and the decoder gates' bias tables ---
// (eval: on the side stream, next to the conditioning branch / conv0; the first consumer is block 0's conv1)
static int fwd_time_embeddings(FwdCtx& f, const int64_t* t, const int64_t* labels, int label_batch) {
  drs_plan* plan = f.plan;
  hipStream_t st_mlp = f.mlp_side ? plan->side : f.s;
  if (f.mlp_side) {
    DRS_CHECK_HIP(hipEventRecord(plan->ev_fork, f.s));  // t / labels were produced on the caller's stream
    DRS_CHECK_HIP(hipStreamWaitEvent(st_mlp, plan->ev_fork, 0));
  }
  const float* inv_freq = (const float*)(f.pk + plan->o_inv_freq);
  const float* label_w = labels ? (const float*)(f.pk + plan->o_label) : nullptr;
  RUN(prof_op(plan, "time_mlp", 0, 0, f.s, [&] {
    return drs_launch_time_mlp_multi(t, inv_freq, f.pk, (const long long*)(f.pk + plan->o_mlp_table), (int)plan->mlps.size(),
                                     256, f.temb, plan->temb_total, f.B, 100, label_w, (const long long*)labels, label_batch,
                                     f.cfg.num_classes, st_mlp);
  }));
  // (the encoder only needs the embeddings; the bias tables are for the decoder's gates)
  if (f.mlp_side) DRS_CHECK_HIP(hipEventRecord(plan->ev_join, st_mlp));
  // Stage inputs that are stored only as x + relu(time_mlp(t)) (xt_only): the fused gate takes the row vector out again
  // through a per-image bias, b'[n] = b - Wg temb[n] (16 x Ch dot products per stage, next to the time MLPs).
  if (plan->sp && !f.train && !f.keep_all()) {
    static const int xt_env = getenv("DRS_XT_ONLY") ? atoi(getenv("DRS_XT_ONLY")) : 1;
    for (int i = 0; i < 3 && xt_env; ++i) {
      const DecStage& st = plan->dec[i];
      // producer: the bottleneck's conv2 on the wave-specialised SP kernel (16-row patches), or the composite kernel of stage i - 1
      const bool producer = i == 0 ? (f.H >> 3) > 8 && (f.W >> 3) > 8 : plan->dec[i - 1].upfuse;
      f.xt_only[i] = st.fused_gate && producer;
      // (stage 0: the bottleneck's conv2 may still decline the second output at its own probe (fwd_encoder_block) and clear
      //  xt_only[0]; the bias table launched here is then one unused 5 us side-stream launch, not an error)
      if (f.xt_only[i])
        RUN(drs_launch_gate_bias((const float*)(f.pk + st.gf_w_off), (const float*)(f.pk + st.gf_b_off),
                                 f.temb + st.mlp.temb_off, plan->temb_total, (float*)((char*)f.ws + st.o_gbias), f.B,
                                 kUp[i], kUp[i + 1], st_mlp));
    }
  }
  if (f.mlp_side) DRS_CHECK_HIP(hipEventRecord(plan->ev_gbias, st_mlp));
  return DRS_OK;
}
// --- LR conditioning branch: RRDB -> bicubic -> conv (reference :345-353), constant per sampling chain ---
static int fwd_lr_branch(FwdCtx& f, const float* lr_img) {
  drs_plan* plan = f.plan;
  const char* pk = f.pk;
  hipStream_t s = f.s;
  const int Bl = f.cfg.lr_batch, CC = f.cfg.cond_channels, H = f.H, W = f.W, mag = f.cfg.magnification;
  const int h = H / mag, w = W / mag;
  prof_begin(plan, "lr_branch", 2.0 * Bl * (7.0 * h * w * CC * CC * 9 + (double)H * W * CC * kDown[0] * 9),
             4.0 * Bl * (15.0 * h * w * CC + (double)H * W * (2 * CC + kDown[0])), s);
  float* a = (float*)((char*)f.ws + plan->o_lr[0]);
  float* b = (float*)((char*)f.ws + plan->o_lr[1]);
  float* r = (float*)((char*)f.ws + plan->o_lr[2]);
  const float* cur = lr_img;
  if (f.train) RUN(drs_launch_nchw_to_nhwc(lr_img, f.TP(plan->t_rn[0]), Bl, CC, h, w, CC, 0, s));
  for (int i = 0; i < 3; ++i) {
    const PlanarConv& c1 = plan->rrdb[2 * i];
    const PlanarConv& c2 = plan->rrdb[2 * i + 1];
    RUN(drs_launch_conv3x3_planar(cur, (const float*)(pk + c1.w_off), (const float*)(pk + c1.b_off), nullptr, a, Bl,
                                  CC, CC, h, w, 1, s));
    float* dst = (cur == b) ? r : b;  // ping-pong so the residual source stays intact
    RUN(drs_launch_conv3x3_planar(a, (const float*)(pk + c2.w_off), (const float*)(pk + c2.b_off), cur, dst, Bl, CC,
                                  CC, h, w, 0, s));
    cur = dst;
    if (f.train) {  // the backward pass reads a_i (ReLU output) and r_{i+1} channels-last
      RUN(drs_launch_nchw_to_nhwc(a, f.TP(plan->t_an[i]), Bl, CC, h, w, CC, 0, s));
      RUN(drs_launch_nchw_to_nhwc(dst, f.TP(plan->t_rn[i + 1]), Bl, CC, h, w, CC, 0, s));
    }
  }
  const PlanarConv& co = plan->rrdb[6];
  RUN(drs_launch_conv3x3_planar(cur, (const float*)(pk + co.w_off), (const float*)(pk + co.b_off), lr_img,
                                f.TP(plan->t_lrenc), Bl, CC, CC, h, w, 0, s));
  const float* upsrc = f.TP(plan->t_lrenc);  // SAR variant: the encoded image is used at its own resolution
  if (mag > 1 || f.train) {
    RUN(drs_launch_bicubic(f.TP(plan->t_lrenc), f.TP(plan->t_up), Bl, CC, h, w, mag, s));
    upsrc = f.TP(plan->t_up);
  }
  RUN(drs_launch_stem(upsrc, (const float*)(pk + plan->stemc.w_off), (const float*)(pk + plan->stemc.b_off),
                      nullptr, 0, f.TP(plan->t_cond), Bl, CC, kDown[0], H, W, s));
  prof_end(plan, s);
  return DRS_OK;
}
// --- x = conv0(x) + cond (reference :342,:355) ---
static int fwd_conv0(FwdCtx& f, const float* x, bool has_cond) {
  drs_plan* plan = f.plan;
  const int B = f.B, C = f.cfg.image_channels, H = f.H, W = f.W;
  return prof_op(plan, "conv0", 2.0 * B * H * W * C * kDown[0] * 9, 4.0 * B * H * W * (C + 2.0 * kDown[0]), f.s, [&] {
    return drs_launch_stem(x, (const float*)(f.pk + plan->stem0.w_off), (const float*)(f.pk + plan->stem0.b_off),
                           has_cond ? f.TP(plan->t_cond) : nullptr, f.cfg.lr_batch, f.TP(plan->t_x0), B, C, kDown[0], H, W,
                           f.s, f.sp);
  });
}
// --- encoder + bottleneck: ResConvBlock i (reference :153-172) in one of three forms, then downs.i (:366) ---
static int fwd_encoder_block(FwdCtx& f, int i) {
  drs_plan* plan = f.plan;
  const ResBlock& rb = plan->enc[i];
  const int B = f.B, ci = kDown[i], co = kDown[i + 1], hh = f.H >> i, ww = f.W >> i;
  const float* xin = f.TP(i == 0 ? plan->t_x0 : plan->t_D[i - 1]);
  // shortcut_conv + BN (1x1) rides inside conv2 as extra K-chunks when both run on the MFMA family ("K-concat")
  const bool fuse_shortcut = !f.train && rb.conv2.mfma && rb.shortcut.mfma;
  if (!fuse_shortcut) {  // shortcut = BNs(conv1x1(x))
    TapConv d = conv_desc(xin, B, hh, ww, ci, ci, 0, f.PW(rb.shortcut), f.PB(rb.shortcut), f.TP(plan->t_S[i]), co, co, 0,
                          1, 1, 1, 0);
    d.in_sp = f.sp; d.out_sp = rb.shortcut.out_sp ? 1 : 0;
    RUN(conv_bn(f, rb.shortcut, d));
  }
  if (i == 0 && rb.dual && fuse_shortcut && f.sp && !f.keep_all() && f.cfg.impl == DRS_IMPL_MFMA_BF16X3 &&
      drs_resblock0_supported(ci, co, hh, ww)) {
    // Block 0 (16 -> 32 -> 32 channels at full resolution) as ONE launch: h stays in LDS (resblock0_sp.hip)
    ResBlock0Desc r0 = {};
    r0.x = xin;
    r0.w1 = f.pk + rb.dual_w_off; r0.b1 = (const float*)(f.pk + rb.dual_b_off);
    r0.temb = f.temb + rb.mlp.temb_off; r0.temb_cs = plan->temb_total;
    r0.w2 = f.PW(rb.conv2); r0.b2 = f.PB(rb.conv2);
    r0.ws = f.PW(rb.shortcut); r0.bs = f.PB(rb.shortcut);
    r0.out = f.TP(plan->t_R[0]);
    r0.N = B; r0.H = hh; r0.W = ww;
    r0.zero_line = f.zero_line; r0.fault = plan->fault_ptr;
    const double px0 = (double)B * hh * ww;
    RUN(prof_op(plan, "conv_blocks.0.fused", 2.0 * px0 * (2.0 * 9 * ci * co + 9.0 * co * co + (double)ci * co),
                4.0 * px0 * (ci + co) + 4.0 * (2.0 * 9 * ci * co + 9.0 * co * co + (double)ci * co), f.s,
                [&] { return drs_launch_resblock0(r0, f.s); }));
  } else {  // the dual launch of conv1 and the skip convolution, or separate launches; then conv2
    bool dual = false;
    if (rb.dual && !f.train && !f.keep_all()) {
      // h = relu(BN1(conv1(x))) + skip(x) + relu(time_mlp(t)) in ONE launch: the skip tensor never exists in HBM
      TapConv d = conv_desc(xin, B, hh, ww, ci, ci, 0, (const float*)(f.pk + rb.dual_w_off),
                            (const float*)(f.pk + rb.dual_b_off), f.TP(plan->t_H[i]), co, co, 0, 3, 3, 1, 1);
      d.dual = 1;
      d.relu_pre = 1;
      d.in_sp = d.out_sp = f.sp; d.zero_line = f.zero_line; d.fault = plan->fault_ptr;
      d.post_add = f.temb + rb.mlp.temb_off; d.post_cs = plan->temb_total;
      if (drs_tapconv_ws_supported(d, f.cfg.impl) || drs_tapconv_sp_supported(d, f.cfg.impl)) {
        const std::string& wn = plan->params[rb.conv1.w].name;
        RUN(prof_op(plan, wn.substr(0, wn.size() - 7) + "+skip", 2.0 * conv_flops(d), conv_bytes(d), f.s,
                    [&] { return drs_launch_tapconv_mfma(d, f.cfg.impl, f.s); }));
        dual = true;
      }
    }
    if (rb.has_skip && !dual) {  // conv_upsampled_lr_img(x_skip), x_skip == block input
      TapConv d = conv_desc(xin, B, hh, ww, ci, ci, 0, f.PW(rb.skip), f.PB(rb.skip), f.TP(plan->t_K0), co, co, 0, 3, 3, 1,
                            1);
      d.in_sp = f.sp; d.zero_line = f.zero_line;
      RUN(plan_conv(plan, rb.skip, d, f.s));
    }
    if (!dual) {  // h = relu(BN1(conv1(x))) [+ skip] + relu(time_mlp(t))
      TapConv d = conv_desc(xin, B, hh, ww, ci, ci, 0, f.PW(rb.conv1), f.PB(rb.conv1), f.TP(plan->t_H[i]), co, co, 0, 3,
                            3, 1, 1);
      d.relu_pre = 1;
      d.in_sp = d.out_sp = f.sp; d.zero_line = f.zero_line;
      d.post_add = f.temb + rb.mlp.temb_off; d.post_cs = plan->temb_total;
      if (rb.has_skip) { d.res = f.TP(plan->t_K0); d.res_cs = co; d.res_co = 0; }
      RUN(conv_bn(f, rb.conv1, d));
    }
    // out = relu(shortcut + BN2(conv2(h)))
    TapConv d = conv_desc(f.TP(plan->t_H[i]), B, hh, ww, co, co, 0, f.PW(rb.conv2), f.PB(rb.conv2), f.TP(plan->t_R[i]),
                          co, co, 0, 3, 3, 1, 1);
    if (fuse_shortcut) {
      d.in2 = xin; d.in2_cs = ci; d.in2_co = 0; d.Cin2 = ci; d.H2 = hh; d.W2 = ww;
      d.w2 = f.PW(rb.shortcut); d.bias2 = f.PB(rb.shortcut);
      d.in2_sp = f.sp;
      if (rb.shortcut.fl_ok && !plan->fl_disabled) d.w2_fl = f.pk + rb.shortcut.fl_img_off;
    } else {
      d.res = f.TP(plan->t_S[i]); d.res_cs = co; d.res_co = 0; d.res_sp = rb.shortcut.out_sp ? 1 : 0;
    }
    d.relu_post = 1;
    d.in_sp = d.out_sp = f.sp; d.zero_line = f.zero_line;
    if (f.sp && i == 3) {  // second output: x + relu(time_mlp(t)) of the first UpConvBlock (its conv then needs no input add)
      d.out2 = f.TP(plan->t_XT[0]); d.out2_cs = co; d.out2_co = 0;
      d.post2 = f.temb + plan->dec[0].mlp.temb_off; d.post2_cs = plan->temb_total;
      if (f.xt_only[0]) {  // both readers of the bottleneck output take x + temb: the plain copy is not written
        TapConv probe = d;
        probe.out = nullptr;
        if (drs_tapconv_sp_supported(probe, f.cfg.impl)) d.out = nullptr;
        else f.xt_only[0] = false;
      }
    }
    RUN(conv_bn(f, rb.conv2, d));
  }
  if (i < 3) {
    TapConv d = conv_desc(f.TP(plan->t_R[i]), B, hh, ww, co, co, 0, f.PW(plan->downs[i]), f.PB(plan->downs[i]),
                          f.TP(plan->t_D[i]), co, co, 0, 3, 3, 2, 1);
    d.in_sp = d.out_sp = f.sp; d.zero_line = f.zero_line;
    RUN(plan_conv(plan, plan->downs[i], d, f.s));
  }
  return DRS_OK;
}
// Input of decoder stage i: the bottleneck's output, then the previous stage's
static float* stage_input(const FwdCtx& f, int i) { return f.TP(i == 0 ? f.plan->t_R[3] : f.plan->t_X[i - 1]); }
// An op of a decoder stage's attention branch: with concurrent stages it runs on the side stream and shares the CUs
static int att_conv(FwdCtx& f, const ConvLayer& L, TapConv d) {
  if (!f.concurrent) return L.bn >= 0 ? conv_bn(f, L, d) : plan_conv(f.plan, L, d, f.s);
  d.shared_cu = 1;
  return plan_conv(f.plan, L, d, f.plan->side);
}
// A decoder stage's attention branch, into cat[:, Cc:] (or psi alone: DecStage::gate_psi).  Two forms: the fused gate, or
// five launches.  With concurrent stages it runs on the side stream, and ev_join marks its end there.
static int fwd_attention(FwdCtx& f, int i) {
  drs_plan* plan = f.plan;
  const DecStage& st = plan->dec[i];
  const int B = f.B, Cc = kUp[i], Ch = kUp[i + 1], lh = f.H >> (3 - i), lw = f.W >> (3 - i);
  const float* xres = f.TP(plan->t_R[2 - i]);  // residual_inputs[-(i+1)]: (B, Ch, 2lh, 2lw)
  hipStream_t sa = f.concurrent ? plan->side : f.s;
  if (st.fused_gate && !f.keep_all()) {
    // gating signal + attention gate in ONE launch (attn_gate_sp.hip): g, g1, p and psi never reach HBM
    AttnGateDesc a = {};
    a.x = f.xt_only[i] ? f.TP(plan->t_XT[i]) : stage_input(f, i); a.x_cs = Cc; a.x_co = 0;
    a.b_gate_img = f.xt_only[i] ? (const float*)((char*)f.ws + st.o_gbias) : nullptr;
    a.xres = xres; a.r_cs = Ch; a.r_co = 0;
    a.out = f.TP(plan->t_CAT[i]); a.out_cs = Cc + Ch; a.out_co = Cc;
    if (st.gate_psi) { a.out = nullptr; a.psi_out = f.TP(plan->t_PSI[i]); }  // (the att-half multiplies by psi itself)
    a.N = B; a.LH = lh; a.LW = lw; a.Cc = Cc; a.Ch = Ch;
    a.w_gate = f.PW(st.gate); a.b_gate = f.PB(st.gate);
    a.w_wg = f.pk + st.fz_wg_off; a.b_wg = f.PB(st.wg);
    a.w_wx = f.pk + st.fz_wx_off; a.b_wx = f.PB(st.wx);
    a.w_psi = f.PW(st.psi); a.b_psi = f.PB(st.psi);
    a.w_res = f.PW(st.result); a.b_res = f.PB(st.result);
    const double px = (double)B * lh * lw;
    RUN(prof_op(plan, "attention_gate." + std::to_string(i), 2.0 * px * Ch * (Cc + 10.0 * Ch), 4.0 * px * (Cc + 8.0 * Ch),
                sa, [&] { return drs_launch_attn_gate(a, sa); }));
  } else {
    // gating = relu(BN(conv1x1(x)))   (:222-225)
    TapConv g = conv_desc(stage_input(f, i), B, lh, lw, Cc, Cc, 0, f.PW(st.gate), f.PB(st.gate), f.TP(plan->t_G[i]), Ch, Ch,
                          0, 1, 1, 1, 0);
    g.relu_pre = 1;
    g.in_sp = g.out_sp = f.sp;
    RUN(att_conv(f, st.gate, g));
    // (fusing w_g into the stride-2 w_x kernel was measured slower: its 16x32 window staging is 4x too large for g;
    //  running w_x early on the side stream, next to the encoder, slowed the encoder kernels more than it saved)
    // g1 = w_g(g)   (:101)
    TapConv g1 = conv_desc(f.TP(plan->t_G[i]), B, lh, lw, Ch, Ch, 0, f.PW(st.wg), f.PB(st.wg), f.TP(plan->t_Q[i]), Ch, Ch,
                           0, 1, 1, 1, 0);
    g1.in_sp = f.sp;
    RUN(att_conv(f, st.wg, g1));
    // relu(g1 + w_x(x))   (:102-103)
    TapConv p = conv_desc(xres, B, 2 * lh, 2 * lw, Ch, Ch, 0, f.PW(st.wx), f.PB(st.wx), f.TP(plan->t_P[i]), Ch, Ch, 0, 2, 2,
                          2, 0);
    p.res = f.TP(plan->t_Q[i]); p.res_cs = Ch; p.res_co = 0;
    p.relu_post = 1;
    p.in_sp = f.sp;
    RUN(att_conv(f, st.wx, p));
    // psi = sigmoid(conv1x1 -> 1 channel)   (:104)
    TapConv psi = conv_desc(f.TP(plan->t_P[i]), B, lh, lw, Ch, Ch, 0, f.PW(st.psi), f.PB(st.psi), f.TP(plan->t_PSI[i]), 1,
                            1, 0, 1, 1, 1, 0);
    psi.sigmoid = 1;
    RUN(att_conv(f, st.psi, psi));
    // attention = BN(conv1x1(nearest2x(psi) * x))  == nearest2x(psi) * (W' x) + b'   (:105-107), into cat[:, Cc:]
    TapConv d = conv_desc(xres, B, 2 * lh, 2 * lw, Ch, Ch, 0, f.PW(st.result), f.PB(st.result), f.TP(plan->t_CAT[i]), Ch,
                          Cc + Ch, Cc, 1, 1, 1, 0);
    d.gate = f.TP(plan->t_PSI[i]);
    d.in_sp = d.out_sp = f.sp;
    RUN(att_conv(f, st.result, d));
  }
  if (f.concurrent) DRS_CHECK_HIP(hipEventRecord(plan->ev_join, sa));
  return DRS_OK;
}
// UpConvBlock: relu(BN(conv(x + relu(time_mlp(t)))))   (:199-205)
static int fwd_ups_conv(FwdCtx& f, int i) {
  drs_plan* plan = f.plan;
  const DecStage& st = plan->dec[i];
  const int Cc = kUp[i], lh = f.H >> (3 - i), lw = f.W >> (3 - i);
  TapConv d = conv_desc(stage_input(f, i), f.B, lh, lw, Cc, Cc, 0, f.PW(st.conv), f.PB(st.conv), f.TP(plan->t_U[i]), Cc,
                        Cc, 0, 3, 3, 1, 1);
  d.relu_pre = 1;
  if (f.sp) {  // the producer of the stage input also wrote x + relu(time_mlp(t)) (TapConv::out2)
    d.in = f.TP(plan->t_XT[i]);
    d.in_sp = d.out_sp = 1; d.zero_line = f.zero_line;
  } else {
    d.in_add = f.temb + st.mlp.temb_off; d.in_add_cs = plan->temb_total;
  }
  d.shared_cu = f.concurrent ? 1 : 0;
  return conv_bn(f, st.conv, d);
}
// ups.i.transform and the x-half of up_convs.i as ONE stride-2 transposed convolution of ups.i.conv's output
// (upfuse_sp.hip; reference :206-207 returns transform(x) with no activation, :377 is a bare convolution): the
// Cc-channel high-resolution tensor is never written.  Three launches: the edge vectors (first row / column of h),
// the att-half of up_convs.i as a plain 3x3 convolution of the attention output, and the composite with the att-half
// as its residual (+ the fused `output` projection in stage 2).
static int fwd_composite_tail(FwdCtx& f, int i, bool edges_aside) {
  drs_plan* plan = f.plan;
  const DecStage& st = plan->dec[i];
  const int B = f.B, Cc = kUp[i], Ch = kUp[i + 1], lh = f.H >> (3 - i), lw = f.W >> (3 - i);
  const float* aux = (const float*)(f.pk + st.uf_aux_off);
  const size_t mat = (size_t)Cc * Ch;
  float* eh = (float*)((char*)f.ws + st.o_eh);
  float* ev = (float*)((char*)f.ws + st.o_ev);
  UpFuseEdgeDesc e = {};
  e.in = f.TP(plan->t_U[i]); e.in_cs = Cc; e.in_co = 0;
  e.N = B; e.LH = lh; e.LW = lw; e.Cc = Cc; e.Ch = Ch;
  e.rt = aux; e.rl = aux + 5 * mat; e.bt = aux + 11 * mat;
  e.eh = eh; e.ev = ev;
  e.wimg = f.pk + st.uf_edge_off; e.zero_line = f.zero_line;
  const double epix = (double)B * 2.0 * (lh + lw);
  hipStream_t se = edges_aside ? plan->side : f.s;  // (profiled forwards have no side stream: edges_aside is false there)
  RUN(prof_op(plan, "up_convs." + std::to_string(i) + ".edges", 2.0 * epix * 2.5 * Cc * Ch, 4.0 * epix * (Cc + 4.0 * Ch),
              se, [&] { return drs_launch_upfuse_edges(e, se); }));
  if (edges_aside) DRS_CHECK_HIP(hipEventRecord(plan->ev_edge_out[i], plan->side));
  if (f.concurrent) DRS_CHECK_HIP(hipStreamWaitEvent(f.s, plan->ev_join, 0));  // the attention half of cat.i is complete
  TapConv d = conv_desc(f.TP(plan->t_CAT[i]), B, 2 * lh, 2 * lw, Ch, Cc + Ch, Cc, (const float*)(f.pk + st.ah_w_off),
                        (const float*)(f.pk + st.ah_b_off), i < 2 ? f.TP(st.t_PA) : nullptr, Ch, Ch, 0, 3, 3, 1, 1);
  d.in_sp = 1; d.out_sp = 1; d.zero_line = f.zero_line; d.fault = plan->fault_ptr;
  if (i < 2 && st.ah_fl_ok && !plan->fl_disabled) d.w_fl = f.pk + st.ah_fl_img_off;
  const double ah_flops = conv_flops(d), ah_bytes = conv_bytes(d);  // (the reference's op, whatever form runs)
  if (i == 2 && st.ah_proj) {
    // projection folded into the weights (pack time): a Ch -> out_dim 3x3 convolution straight into the caller's tensor
    d.out = nullptr; d.out_sp = 0; d.bias = nullptr;
    d.Cout = 16; d.out_cs = 16;
    d.proj = 1;
    if (st.gate_psi) {  // `result` folded in: the input is the skip tensor, gated by psi inside the kernel
      d.in = f.TP(plan->t_R[2 - i]); d.in_cs = Ch; d.in_co = 0;
      d.gate = f.TP(plan->t_PSI[i]);
      d.bias = (const float*)(f.pk + st.ah_tab_off);
    }
    d.fuse_out = f.out; d.fuse_dim = f.cfg.out_dim; d.fuse_b = nullptr;
    RUN(prof_op(plan, "up_convs.2.att", ah_flops, ah_bytes, f.s, [&] { return drs_launch_conv3x3_direct_sp(d, f.s); }));
  } else {
    if (i == 2) {
      // the `output` projection is linear: the att-half is projected HERE (its own fused-projection epilogue, zero bias)
      // into the caller's output tensor and the composite kernel adds its part: 12.6 MB written and read back instead
      // of the 134 MB of 32-channel partial sums
      d.out = nullptr; d.out_sp = 0;
      d.fuse_w = (const float*)(f.pk + plan->o_out_w);
      d.fuse_b = (const float*)(f.pk + st.ah_b_off);  // zeros
      d.fuse_out = f.out;
      d.fuse_dim = f.cfg.out_dim;
    }
    RUN(prof_op(plan, "up_convs." + std::to_string(i) + ".att", ah_flops, ah_bytes, f.s,
                [&] { return drs_launch_tapconv_mfma(d, f.cfg.impl, f.s); }));
  }
  UpFuseDesc u = {};
  u.in = f.TP(plan->t_U[i]); u.in_cs = Cc; u.in_co = 0;
  u.N = B; u.LH = lh; u.LW = lw; u.Cc = Cc; u.Ch = Ch;
  u.w = f.pk + (st.uf_proj ? st.ufp_w_off : st.uf_w_off);  // the folded composite on the streaming kernel: its own operand image
  u.bias = aux + 11 * mat + 9 * Ch;
  if (i < 2) { u.res = f.TP(st.t_PA); u.res_cs = Ch; u.res_co = 0; }
  u.eh = eh; u.ev = ev;
  u.zero_line = f.zero_line; u.fault = plan->fault_ptr;
  if (i == 2) {  // output 1x1 conv (:379) rides in the epilogue; the 32-channel tensor is never written
    u.res = nullptr; u.fuse_acc = 1;
    u.proj = st.uf_proj ? 1 : 0;  // the projection (and its bias) is inside the composite weights / bias / edge vectors
    if (!st.uf_proj) {
      u.fuse_w = (const float*)(f.pk + plan->o_out_w);
      u.fuse_b = (const float*)(f.pk + plan->o_out_b);
    }
    u.fuse_out = f.out;
    u.fuse_dim = f.cfg.out_dim;
  } else {
    if (!f.xt_only[i + 1]) { u.out = f.TP(plan->t_X[i]); u.out_cs = Ch; u.out_co = 0; }
    u.out2 = f.TP(plan->t_XT[i + 1]); u.out2_cs = Ch; u.out2_co = 0;  // x + temb of the next stage's UpConvBlock
    u.post2 = f.temb + plan->dec[i + 1].mlp.temb_off; u.post2_cs = plan->temb_total;
  }
  if (edges_aside) DRS_CHECK_HIP(hipStreamWaitEvent(f.s, plan->ev_edge_out[i], 0));
  const double opix = (double)B * 4.0 * lh * lw;
  // executed work: 6.25 composite taps per output pixel; bytes: h + att-half partial sums + result (+ weights)
  return prof_op(plan, "up_convs." + std::to_string(i) + ".fused", 2.0 * opix * 6.25 * Cc * Ch,
                 4.0 * (opix / 4.0 * Cc + 2.0 * opix * Ch + 25.0 * Cc * Ch), f.s,
                 [&] { return st.uf_proj ? drs_launch_upfuse_proj(u, f.s) : drs_launch_upfuse(u, f.s); });
}
// Stage 2 writes the caller's output itself when the `output` 1x1 convolution (:379) rides in its last launch's epilogue
static bool output_fused(const drs_plan* plan) {
  return plan->dec[2].upfuse || (plan->dec[2].upconv.mfma && plan->cfg.out_dim <= 4);
}
// transform: ConvTranspose2d, into cat[:, :Cc]   (:206, :376), then up_conv over the concatenation (:377)
static int fwd_unfused_tail(FwdCtx& f, int i) {
  drs_plan* plan = f.plan;
  const DecStage& st = plan->dec[i];
  const int B = f.B, Cc = kUp[i], Ch = kUp[i + 1], lh = f.H >> (3 - i), lw = f.W >> (3 - i);
  float* cat = f.TP(plan->t_CAT[i]);
  if (st.transform.mfma) {  // 4 phases in one launch
    TapConv d = convT_fused_desc(f.TP(plan->t_U[i]), B, lh, lw, Cc, Cc, 0, f.PW(st.transform), f.PB(st.transform), cat, Cc,
                                 Cc + Ch, 0);
    d.shared_cu = f.concurrent ? 1 : 0;
    d.in_sp = d.out_sp = f.sp; d.zero_line = f.zero_line;
    RUN(plan_conv(plan, st.transform, d, f.s));
  } else
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        TapConv d = convT_phase_desc(f.TP(plan->t_U[i]), B, lh, lw, Cc, Cc, 0, f.PW(st.transform), f.PB(st.transform), cat,
                                     Cc, Cc + Ch, 0, py, px);
        RUN(plan_conv(plan, st.transform, d, f.s));
      }
  if (f.concurrent) DRS_CHECK_HIP(hipStreamWaitEvent(f.s, plan->ev_join, 0));  // both halves of cat.i are complete
  // up_conv over the concatenation (:377), no norm / activation
  TapConv d = conv_desc(cat, B, 2 * lh, 2 * lw, Cc + Ch, Cc + Ch, 0, f.PW(st.upconv), f.PB(st.upconv), f.TP(plan->t_X[i]),
                        Ch, Ch, 0, 3, 3, 1, 1);
  if (i == 2 && output_fused(plan)) {  // output 1x1 conv (:379) rides in the epilogue
    d.fuse_w = (const float*)(f.pk + plan->o_out_w);
    d.fuse_b = (const float*)(f.pk + plan->o_out_b);
    d.fuse_out = f.out;
    d.fuse_dim = f.cfg.out_dim;
    if (!(f.cfg.flags & (DRS_PLAN_KEEP_ALL | DRS_PLAN_TRAIN))) d.out = nullptr;  // the wide tensor is only a parity tap
  }
  d.in_sp = f.sp; d.zero_line = f.zero_line;
  d.out_sp = st.upconv.out_sp ? 1 : 0;
  if (f.sp && i < 2) {  // second output for the next stage's UpConvBlock
    d.out2 = f.TP(plan->t_XT[i + 1]); d.out2_cs = Ch; d.out2_co = 0;
    d.post2 = f.temb + plan->dec[i + 1].mlp.temb_off; d.post2_cs = plan->temb_total;
  }
  return plan_conv(plan, st.upconv, d, f.s);
}

extern "C" int drs_unet_forward(drs_plan* plan, const void* packed, const float* x, const int64_t* t,
                                const float* lr_img, float* out, void* workspace, size_t workspace_bytes, int flags,
                                drs_stream_t stream) {
  return drs_unet_forward_labels(plan, packed, x, t, lr_img, nullptr, 0, out, workspace, workspace_bytes, flags, stream);
}

extern "C" int drs_unet_forward_labels(drs_plan* plan, const void* packed, const float* x, const int64_t* t,
                                       const float* lr_img, const int64_t* labels, int label_batch, float* out,
                                       void* workspace, size_t workspace_bytes, int flags, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(plan && packed && x && t && out && workspace, DRS_ERR_ARG, "forward: null pointer");
  DRS_REQUIRE(plan->packed_ok && plan->packed_ptr == packed, DRS_ERR_STATE,
              "forward: weights not packed into this buffer (call drs_unet_pack_weights first)");
  DRS_REQUIRE(workspace_bytes >= plan->ws_bytes, DRS_ERR_WORKSPACE, "forward: workspace %zu < %zu", workspace_bytes,
              plan->ws_bytes);
  const bool reuse_cond = (flags & DRS_FWD_REUSE_COND) != 0;
  const bool has_cond = plan->cfg.variant != DRS_VARIANT_GENERATION;
  DRS_REQUIRE(!has_cond || reuse_cond || lr_img, DRS_ERR_ARG, "forward: conditioning image is null");
  DRS_REQUIRE(!labels || (plan->label_emb >= 0 && (label_batch == plan->cfg.batch || label_batch == 1)), DRS_ERR_ARG,
              "forward: labels need the generation variant with num_classes > 0 and label_batch == batch or 1");
  FwdCtx f(plan, packed, workspace, out, s);
  plan->fault_ptr = (unsigned*)(f.pk + plan->o_fault);
  if (plan->profiling) {
    for (auto& r : plan->ops) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    plan->ops.clear();
  }
  LaunchLogScope launch_log(plan);

  // DRS_CONCURRENT: 1 / 0 force the two-stream decoder stages (below) on / off.  Default: on for the fp32-activation plans
  // (their kernels run two blocks per CU and leave room for a partner); off for SP plans, whose wave-specialised kernels own
  // a whole CU (154 KB of LDS, 12 waves) and whose attention gate is one fused launch: measured 498 vs 469 steps/s.
  static const int concurrent_env = getenv("DRS_CONCURRENT") ? atoi(getenv("DRS_CONCURRENT")) : -1;
  const bool serial = f.train || plan->profiling || f.cfg.impl == DRS_IMPL_DIRECT;
  f.concurrent = (concurrent_env < 0 ? !plan->sp : concurrent_env != 0) && !serial;
  // the time MLPs (one small latency-bound launch) run next to conv0 in every eval plan unless DRS_CONCURRENT=0
  f.mlp_side = concurrent_env != 0 && !serial;
  if ((f.concurrent || f.mlp_side) && !plan->side) {
    DRS_CHECK_HIP(hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking));
    for (hipEvent_t* e : {&plan->ev_fork, &plan->ev_join, &plan->ev_gbias, &plan->ev_edge_in[0], &plan->ev_edge_out[0],
                          &plan->ev_edge_in[1], &plan->ev_edge_out[1], &plan->ev_edge_in[2], &plan->ev_edge_out[2]})
      DRS_CHECK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }

  RUN(fwd_time_embeddings(f, t, labels, label_batch));
  if (has_cond && !reuse_cond) RUN(fwd_lr_branch(f, lr_img));
  RUN(fwd_conv0(f, x, has_cond));
  if (f.mlp_side) DRS_CHECK_HIP(hipStreamWaitEvent(s, plan->ev_join, 0));  // time embeddings are ready
  for (int i = 0; i < 4; ++i) RUN(fwd_encoder_block(f, i));
  if (f.mlp_side) DRS_CHECK_HIP(hipStreamWaitEvent(s, plan->ev_gbias, 0));  // per-image gating biases (side stream) are ready

  // --- decoder (reference :372-377) ---
  // Eval plans run the attention branch of a stage (gating, w_g, w_x, psi, result: HBM-bound 1x1 / 2x2 kernels) on a
  // second stream NEXT TO the up-sampling branch (3x3 conv + ConvTranspose: MFMA / LDS-bound): both only read the stage
  // input and the skip tensor and write disjoint channel slices of cat.i.  Every kernel of the pair is launched with
  // one block per CU, so a block of each fits on every CU at once (2 x 80 KB of LDS) and the two use complementary
  // resources.  Train plans and profiled runs keep the serial order.
  for (int i = 0; i < 3; ++i) {
    const DecStage& st = plan->dec[i];
    if (f.concurrent) {
      DRS_CHECK_HIP(hipEventRecord(plan->ev_fork, s));
      DRS_CHECK_HIP(hipStreamWaitEvent(plan->side, plan->ev_fork, 0));
    }
    // Order inside a stage.  A composite stage whose plan owns a side stream computes its edge vectors THERE, next to
    // the attention gate: they only need ups.i.conv's output, are three tiny launches' worth of latency (35 us per
    // forward on the main stream) and occupy a fraction of the CUs.  So: UpConvBlock conv, [edges || gate], att-half,
    // composite.  Everything else keeps the reference's order (gate first).
    const bool edges_aside = st.upfuse && f.mlp_side && !f.concurrent;
    if (edges_aside) {
      RUN(fwd_ups_conv(f, i));
      DRS_CHECK_HIP(hipEventRecord(plan->ev_edge_in[i], s));
      DRS_CHECK_HIP(hipStreamWaitEvent(plan->side, plan->ev_edge_in[i], 0));
      RUN(fwd_attention(f, i));
    } else {
      RUN(fwd_attention(f, i));
      RUN(fwd_ups_conv(f, i));
    }
    RUN(st.upfuse ? fwd_composite_tail(f, i, edges_aside) : fwd_unfused_tail(f, i));
  }
  if (!output_fused(plan)) {  // output 1x1 conv (:379), straight to the caller's NCHW tensor
    TapConv d = conv_desc(f.TP(plan->t_X[2]), f.B, f.H, f.W, kUp[3], kUp[3], 0, f.PW(plan->output), f.PB(plan->output), out,
                          f.cfg.out_dim, f.cfg.out_dim, 0, 1, 1, 1, 0);
    d.out_nchw = 1;
    RUN(plan_conv(plan, plan->output, d, s));
  }
  return DRS_OK;
}

// Synchronises `stream` and reports whether a wave of the wave-specialised kernels ran into its bounded poll since the
// weights were last packed into `packed` (a protocol bug: the forward's output is then incomplete).
extern "C" int drs_unet_check_faults(drs_plan* plan, const void* packed, drs_stream_t stream) {
  DRS_REQUIRE(plan && packed, DRS_ERR_ARG, "check_faults: null pointer");
  DRS_REQUIRE(plan->packed_ok && plan->packed_ptr == packed, DRS_ERR_STATE, "check_faults: weights not packed into this buffer");
  unsigned words[5] = {0, 0, 0, 0, 0};
  DRS_CHECK_HIP(hipMemcpyAsync(words, aligned_base(packed) + plan->o_fault, sizeof(words), hipMemcpyDeviceToHost, (hipStream_t)stream));
  DRS_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  const unsigned word = words[0];
  DRS_REQUIRE((word & 1u) == 0, DRS_ERR_HIP, "a wave-specialised kernel timed out on an LDS counter (protocol fault); results are incomplete");
  if (word & 2u) {  // the FL kernel's movers met an activation block whose maximum fp16 cannot hold
    plan->fl_disabled = true;
    DRS_CHECK_HIP(hipMemsetAsync(aligned_base(packed) + plan->o_fault, 0, 32, (hipStream_t)stream));
    DRS_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    DrsErr::set("an activation left fp16's range in the FL arithmetic (last report: layer Cin=%u Cout=%u, %u rows, %s input, block %u "
                "round %u lane %u, block scale exponent %u): the forward(s) since the last check are invalid; this plan now runs the "
                "split-bf16 kernels - run the forward / chain again", words[1] >> 16, words[1] & 0xffffu, words[2] >> 16,
                (words[2] & 1u) ? "second (1x1)" : "3x3", words[3] >> 16, (words[3] >> 8) & 0xffu, words[3] & 0xffu, words[4]);
    return DRS_ERR_RANGE;
  }
  return DRS_OK;
}
