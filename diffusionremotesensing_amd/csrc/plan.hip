// C-ABI of include/drs_hip.h: creation of the whole-UNet plan (parameters, kernel forms, packed-buffer and workspace layout)
// and its introspection calls.
#include <stdlib.h>
#include <algorithm>
#include <memory>

#include "unet_plan.h"

// ---- plan creation: one step per job, in this order ----
static std::string cond_encoder_name(const drs_unet_config& c) { return c.variant == DRS_VARIANT_SAR_TO_NDVI ? "SAR_encoder" : "LR_encoder"; }
// The parameters in a fixed canonical order (names = reference state_dict keys; the order is the ABI's), each layer entered in
// the convs / planars / mlps registry the packing and the schedules walk as it is made (same order)
static void plan_params(drs_plan* p) {
  const drs_unet_config& cfg = p->cfg;
  const int C = cfg.image_channels, CC = cfg.cond_channels;  // CC: conditioning image channels
  const bool has_cond = cfg.variant != DRS_VARIANT_GENERATION;
  const std::string enc_name = cond_encoder_name(cfg);
  const std::string cond_name = cfg.variant == DRS_VARIANT_SAR_TO_NDVI ? "conv_SAR_img" : "conv_upsampled_lr_img";
  const std::string skip_name = cfg.variant == DRS_VARIANT_GENERATION ? "conv_skip" : cond_name;
  p->stem0 = p->mk_planar("conv0", kDown[0], C);
  p->planars.push_back(&p->stem0);
  if (has_cond) {
    for (int i = 0; i < 3; ++i) {
      p->rrdb[2 * i] = p->mk_planar(enc_name + ".blocks." + std::to_string(i) + ".conv1", CC, CC);
      p->rrdb[2 * i + 1] = p->mk_planar(enc_name + ".blocks." + std::to_string(i) + ".conv2", CC, CC);
    }
    p->rrdb[6] = p->mk_planar(enc_name + ".conv_out", CC, CC);
    p->stemc = p->mk_planar(cond_name, kDown[0], CC);
    for (PlanarConv& L : p->rrdb) p->planars.push_back(&L);
    p->planars.push_back(&p->stemc);
  }
  if (cfg.variant == DRS_VARIANT_GENERATION && cfg.num_classes > 0)
    p->label_emb = p->P("label_emb.weight", (int64_t)cfg.num_classes * 100);
  for (int i = 0; i < 4; ++i) {
    const std::string pfx = i < 3 ? "conv_blocks." + std::to_string(i) : std::string("bottle_neck");
    const int ci = kDown[i], co = kDown[i + 1];
    ResBlock& rb = p->enc[i];
    rb.mlp = p->mk_mlp(pfx + ".time_mlp", co);
    rb.conv1 = p->mk_conv(pfx + ".conv1.0", co, ci, 9, pfx + ".batch_norm1");
    rb.conv2 = p->mk_conv(pfx + ".conv2.0", co, co, 9, pfx + ".batch_norm2");
    rb.shortcut = p->mk_conv(pfx + ".shortcut_conv.0", co, ci, 1, pfx + ".shortcut_batch_norm");
    rb.has_skip = (i == 0);
    if (rb.has_skip) rb.skip = p->mk_conv(pfx + "." + skip_name, co, ci, 9);
    if (i < 3) p->downs[i] = p->mk_conv("downs." + std::to_string(i), co, co, 9);
    p->convs.insert(p->convs.end(), {&rb.conv1, &rb.conv2, &rb.shortcut});
    if (rb.has_skip) p->convs.push_back(&rb.skip);
    if (i < 3) p->convs.push_back(&p->downs[i]);
    p->mlps.push_back(&rb.mlp);
  }
  for (int i = 0; i < 3; ++i) {
    const std::string si = std::to_string(i);
    const int Cc = kUp[i], Ch = kUp[i + 1];
    DecStage& d = p->dec[i];
    d.gate = p->mk_conv("gating_signals." + si + ".conv", Ch, Cc, 1, "gating_signals." + si + ".batch_norm");
    d.wg = p->mk_conv("attention_blocks." + si + ".w_g.0", Ch, Ch, 1);
    d.wx = p->mk_conv("attention_blocks." + si + ".w_x.0", Ch, Ch, 4);
    d.psi = p->mk_conv("attention_blocks." + si + ".psi.0", 1, Ch, 1);
    d.result = p->mk_conv("attention_blocks." + si + ".result.0", Ch, Ch, 1, "attention_blocks." + si + ".result.1");
    d.mlp = p->mk_mlp("ups." + si + ".time_mlp", Cc);
    d.conv = p->mk_conv("ups." + si + ".conv", Cc, Cc, 9, "ups." + si + ".batch_norm");
    d.transform = p->mk_conv("ups." + si + ".transform", Cc, Cc, 9, "", true);
    d.upconv = p->mk_conv("up_convs." + si, Ch, Cc + Ch, 9);
    p->convs.insert(p->convs.end(), {&d.gate, &d.wg, &d.wx, &d.psi, &d.result, &d.conv, &d.transform, &d.upconv});
    p->mlps.push_back(&d.mlp);
  }
  p->output = p->mk_conv("output", cfg.out_dim, kUp[3], 1);
  p->convs.push_back(&p->output);
}

// Every shape- and switch-dependent decision: SP activations, each layer's kernel family and form, the fused forms of the
// decoder stages and which layers get FL images.  (No byte offsets: plan_packed_layout places what is decided here.)
static void plan_kernel_forms(drs_plan* p) {
  static const bool sp_env = !(getenv("DRS_SP") && atoi(getenv("DRS_SP")) == 0);
  static const bool gp_env = !(getenv("DRS_GATE_PSI") && atoi(getenv("DRS_GATE_PSI")) == 0);
  static const bool fl_env = !(getenv("DRS_FL") && atoi(getenv("DRS_FL")) == 0);
  const drs_unet_config& cfg = p->cfg;
  const bool train = (cfg.flags & DRS_PLAN_TRAIN) != 0, keep_all = (cfg.flags & DRS_PLAN_KEEP_ALL) != 0;
  p->sp = sp_env && !train && cfg.impl == DRS_IMPL_MFMA_BF16X3;
  for (ConvLayer* L : p->convs) {  // kernel family per layer: decided on shape alone
    TapConv probe = {};
    probe.Cin = L->Cin; probe.Cout = L->Cout; probe.ntaps = L->taps;
    L->mfma = cfg.impl != DRS_IMPL_DIRECT && drs_tapconv_mfma_supported(probe, cfg.impl);
  }
  for (ResBlock& rb : p->enc) {
    // (the shortcut rides inside conv2 as extra K-chunks: same accumulator rows, same permutation)
    rb.conv1.out_sp = rb.conv2.out_sp = rb.shortcut.out_sp = p->sp;
    rb.dual = rb.has_skip && !train && cfg.impl == DRS_IMPL_MFMA_BF16X3 && rb.conv1.Cout == 32 && rb.skip.Cout == 32 &&
              rb.skip.Cin == rb.conv1.Cin;
  }
  for (ConvLayer& L : p->downs) L.out_sp = p->sp;
  for (int i = 0; i < 3; ++i) {
    DecStage& d = p->dec[i];
    const int Cc = kUp[i], Ch = kUp[i + 1];
    d.gate.out_sp = d.result.out_sp = d.conv.out_sp = d.transform.out_sp = p->sp;
    d.upconv.out_sp = p->sp && i < 2;  // up_convs.2 feeds the fused / direct output projection in fp32
    d.fused_gate = p->sp && drs_attn_gate_supported(Cc, Ch);
    // (KEEP_ALL plans stay unfused: ups.i is a parity tap; stage 2 needs the fused output projection: its result is fp32)
    d.upfuse = p->sp && !keep_all && (i < 2 || (Ch == 32 && cfg.out_dim <= 4)) &&
               drs_upfuse_supported(Cc, Ch, cfg.height >> (3 - i), cfg.width >> (3 - i));
    if (i < 2 || !d.upfuse) continue;
    // stage 2: the `output` projection folded into the att-half's weights where the direct kernel takes that layer
    TapConv probe = conv_desc((const float*)256, cfg.batch, cfg.height, cfg.width, Ch, Cc + Ch, Cc, (const float*)256, nullptr, nullptr,
                              16, 16, 0, 3, 3, 1, 1);
    probe.in_sp = 1; probe.zero_line = (const void*)256; probe.proj = 1; probe.fuse_out = (float*)256; probe.fuse_dim = cfg.out_dim;
    d.ah_proj = drs_conv3x3_direct_sp_proj_supported(probe, cfg.impl);
    // the composite's folded form needs the att-half in the output tensor first (fuse_acc): both or neither
    d.uf_proj = d.ah_proj && drs_upfuse_proj_supported(Cc, Ch, cfg.out_dim);
    d.gate_psi = gp_env && d.ah_proj && d.fused_gate && Ch == 32 && !keep_all && !(cfg.height & 1) && !(cfg.width & 1);
  }
  p->fl = fl_env && p->sp;  // FL images (conv_mfma_fl.hip) for the layers the wave-specialised kernel takes at 64 channels per item
  if (!p->fl) return;
  for (ConvLayer* L : p->convs)
    if ((L->taps == 9 || L->taps == 1) && !L->transposed && L->Cout % 64 == 0 && L->Cin % 32 == 0) L->fl_slot = p->fl_slots++;
  for (int i = 0; i < 2; ++i)
    if (p->dec[i].upfuse && kUp[i + 1] % 64 == 0) p->dec[i].ah_fl_slot = p->fl_slots++;
}

// Offsets in the packed buffer of everything drs_unet_pack_weights writes
static void plan_packed_layout(drs_plan* p) {
  const drs_unet_config& cfg = p->cfg;
  size_t cur = 0;
  p->o_inv_freq = cur; cur += align_up(50 * 4);
  for (ConvLayer* L : p->convs) {
    L->w_off = cur;  // room for whichever kernel family's image is largest
    size_t need = (size_t)L->Cout * L->Cin * L->taps * 4;
    for (int im = DRS_IMPL_MFMA_F32; im <= DRS_IMPL_MFMA_F16; ++im) need = std::max(need, drs_pack_conv_mfma_bytes(L->Cout, L->Cin, L->taps, im));
    cur += align_up(need);
    L->b_off = cur; cur += align_up((size_t)L->Cout * 4);
  }
  for (ResBlock& rb : p->enc) {
    if (!rb.dual) continue;
    rb.dual_w_off = cur; cur += align_up(drs_pack_conv_mfma_bytes(64, rb.conv1.Cin, 9, DRS_IMPL_MFMA_BF16X3));
    rb.dual_b_off = cur; cur += align_up((size_t)64 * 4);
  }
  for (DecStage& d : p->dec) {
    if (!d.fused_gate) continue;
    d.fz_wg_off = cur; cur += align_up(drs_pack_conv_mfma_bytes(d.wg.Cout, d.wg.Cin, 1, DRS_IMPL_MFMA_BF16X3));
    d.fz_wx_off = cur; cur += align_up(drs_pack_conv_mfma_bytes(d.wx.Cout, d.wx.Cin, 4, DRS_IMPL_MFMA_BF16X3));
    d.gf_w_off = cur; cur += align_up((size_t)d.gate.Cout * d.gate.Cin * 4);
    d.gf_b_off = cur; cur += align_up((size_t)d.gate.Cout * 4);
  }
  for (int i = 0; i < 3; ++i) {
    DecStage& d = p->dec[i];
    if (!d.upfuse) continue;
    const int Cc = kUp[i], Ch = kUp[i + 1];
    d.uf_w_off = cur; cur += align_up(drs_upfuse_weight_bytes(Cc, Ch));
    d.uf_aux_off = cur; cur += align_up(drs_upfuse_aux_floats(Cc, Ch) * 4);
    d.uf_edge_off = cur; cur += align_up(drs_upfuse_edge_image_bytes(Cc, Ch));
    d.ah_w_off = cur; cur += align_up(drs_pack_conv_mfma_bytes(Ch, Ch, 9, DRS_IMPL_MFMA_BF16X3));
    d.ah_b_off = cur; cur += align_up((size_t)Ch * 4);
    if (d.ah_proj) { d.ah_tmp_off = cur; cur += align_up((size_t)16 * Ch * 9 * 4); }
    if (d.gate_psi) {
      d.ah_tmp2_off = cur; cur += align_up((size_t)16 * Ch * 3 * 4);
      d.ah_tab_off = cur; cur += align_up((size_t)36 * 4);
    }
    if (d.uf_proj) {
      d.uf_tmpw_off = cur; cur += align_up((size_t)32 * (Cc + Ch) * 9 * 4);
      d.uf_tmpb_off = cur; cur += align_up((size_t)32 * 4);
      d.ufp_w_off = cur; cur += align_up(drs_upfuse_proj_weight_bytes(Cc));
    }
  }
  if (p->fl) {
    for (ConvLayer* L : p->convs)
      if (L->fl_slot >= 0) { L->fl_img_off = cur; cur += align_up(drs_fl_image_bytes(L->Cout, L->Cin, L->taps)); }
    for (int i = 0; i < 2; ++i)
      if (p->dec[i].ah_fl_slot >= 0) { p->dec[i].ah_fl_img_off = cur; cur += align_up(drs_fl_image_bytes(kUp[i + 1], kUp[i + 1], 9)); }
    p->o_fl_flags = cur; cur += align_up((size_t)p->fl_slots * 8);  // [range flag, largest |weight|] per image
  }
  for (PlanarConv* L : p->planars) {
    L->w_off = cur; cur += align_up((size_t)L->Cout * L->Cin * 9 * 4);
    L->b_off = cur; cur += align_up((size_t)L->Cout * 4);
  }
  for (Mlp* m : p->mlps) {
    m->o_w1 = cur; cur += align_up((size_t)m->dim * 100 * 4);
    m->o_b1 = cur; cur += align_up((size_t)m->dim * 4);
    m->o_w2 = cur; cur += align_up((size_t)m->dim * m->dim * 4);
    m->o_b2 = cur; cur += align_up((size_t)m->dim * 4);
  }
  p->o_mlp_table = cur; cur += align_up(p->mlps.size() * 6 * sizeof(long long));
  p->o_label = cur; cur += align_up((size_t)(cfg.num_classes > 0 ? cfg.num_classes : 0) * 100 * 4);
  p->o_out_w = cur; cur += align_up((size_t)cfg.out_dim * kUp[3] * 4);
  p->o_out_b = cur; cur += align_up((size_t)cfg.out_dim * 4);
  p->o_zero = cur; cur += 256;  // a line of zeros: source of out-of-image pixels for LDS-DMA staging
  p->o_fault = cur; cur += 256;  // TapConv::fault word of the wave-specialised kernels (drs_unet_check_faults)
  p->packed_bytes = cur;
}

// The forward's tensors and per-forward tables (every plan), from workspace offset `ws` on
static void plan_eval_workspace(drs_plan* p, size_t& ws) {
  const drs_unet_config& cfg = p->cfg;
  const int B = cfg.batch, Bl = cfg.lr_batch, H = cfg.height, W = cfg.width, h = H / cfg.magnification, w = W / cfg.magnification;
  const int CCw = cfg.cond_channels > 0 ? cfg.cond_channels : 1;
  for (int i = 0; i < 3; ++i) { p->o_lr[i] = ws; ws += align_up((size_t)Bl * CCw * h * w * 4); }
  p->o_temb = ws; ws += align_up((size_t)B * p->temb_total * 4);
  p->t_lrenc = p->T(cond_encoder_name(cfg), ws, Bl, CCw, h, w, true);
  p->t_up = p->T("upsampled_lr_img", ws, Bl, CCw, H, W, true);
  p->t_cond = p->T("cond", ws, Bl, kDown[0], H, W);
  p->t_x0 = p->T("x0", ws, B, kDown[0], H, W);
  for (int i = 0; i < 4; ++i) {
    const int co = kDown[i + 1], hh = H >> i, ww = W >> i;
    const std::string nm = i < 3 ? "conv_blocks." + std::to_string(i) : std::string("bottle_neck");
    p->t_S[i] = p->T(nm + ".shortcut", ws, B, co, hh, ww);
    if (i == 0) p->t_K0 = p->T(nm + ".skip", ws, B, co, hh, ww);
    p->t_H[i] = p->T(nm + ".h", ws, B, co, hh, ww);
    p->t_R[i] = p->T(nm, ws, B, co, hh, ww);
    if (i < 3) p->t_D[i] = p->T("downs." + std::to_string(i), ws, B, co, hh / 2, ww / 2);
  }
  for (int i = 0; i < 3; ++i) {
    const std::string si = std::to_string(i);
    const int Cc = kUp[i], Ch = kUp[i + 1];
    const int lh = H >> (3 - i), lw = W >> (3 - i);
    p->t_G[i] = p->T("gating_signals." + si, ws, B, Ch, lh, lw);
    p->t_Q[i] = p->T("attention_blocks." + si + ".g1", ws, B, Ch, lh, lw);
    p->t_P[i] = p->T("attention_blocks." + si + ".relu", ws, B, Ch, lh, lw);
    p->t_PSI[i] = p->T("attention_blocks." + si + ".psi", ws, B, 1, lh, lw);
    p->t_U[i] = p->T("ups." + si + ".conv", ws, B, Cc, lh, lw);
    p->t_CAT[i] = p->T("cat." + si, ws, B, Cc + Ch, 2 * lh, 2 * lw);
    p->Tview("ups." + si, p->t_CAT[i], Cc, 0);
    p->Tview("attention_blocks." + si, p->t_CAT[i], Ch, Cc);
    p->t_X[i] = p->T("up_convs." + si, ws, B, Ch, 2 * lh, 2 * lw);
  }
  if (!p->sp) return;
  for (int i = 0; i < 3; ++i) p->t_XT[i] = p->T("ups." + std::to_string(i) + ".in", ws, B, kUp[i], H >> (3 - i), W >> (3 - i));
  auto mark = [&](int t) { p->tensors[t].sp = true; };
  for (int i = 0; i < 3; ++i) {
    DecStage& d = p->dec[i];
    if (d.fused_gate) { d.o_gbias = ws; ws += align_up((size_t)B * kUp[i + 1] * 4); }
    if (!d.upfuse) continue;
    const int lh = H >> (3 - i), lw = W >> (3 - i), Ch = kUp[i + 1];
    if (i < 2) {  // (stage 2 hands its att-half over projected, through the output tensor)
      d.t_PA = p->T("up_convs." + std::to_string(i) + ".att_half", ws, B, Ch, 2 * lh, 2 * lw);
      mark(d.t_PA);
    }
    d.o_eh = ws; ws += align_up((size_t)B * 2 * (2 * lw) * Ch * 4);
    d.o_ev = ws; ws += align_up((size_t)B * 2 * (2 * lh) * Ch * 4);
  }
  mark(p->t_x0);
  for (int i = 0; i < 4; ++i) { mark(p->t_H[i]); mark(p->t_R[i]); if (i < 3) mark(p->t_D[i]); }
  for (int i = 0; i < 3; ++i) { mark(p->t_G[i]); mark(p->t_U[i]); mark(p->t_CAT[i]); mark(p->t_XT[i]); if (i < 2) mark(p->t_X[i]); }
  for (WsTensor& t : p->tensors)  // channel-slice views of the concat buffers
    for (int i = 0; i < 3; ++i)
      if (t.off == p->tensors[p->t_CAT[i]].off) t.sp = true;
}

// Train plans: pre-BatchNorm tensors and statistics, reduction regions, and the backward's gradients and scratch
static void plan_train_workspace(drs_plan* p, size_t& ws) {
  const drs_unet_config& cfg = p->cfg;
  const int B = cfg.batch, H = cfg.height, W = cfg.width, h = H / cfg.magnification, w = W / cfg.magnification;
  const int CCw = cfg.cond_channels > 0 ? cfg.cond_channels : 1;
  size_t sums_cur = 0;
  auto addz = [&](ConvLayer& L, const std::string& nm, int hh, int ww) {
    L.stats_off = ws; ws += align_up(2 * (size_t)L.Cout * 4);
    L.sums_off = sums_cur; sums_cur += 2 * (size_t)L.Cout * sizeof(double);
    L.t_Z = p->T(nm + ".pre_bn", ws, B, L.Cout, hh, ww);
    if (L.taps == 9 && L.Cout % 32 == 0 && hh > 8) L.t_Zsp = p->T(nm + ".dz_sp", ws, B, L.Cout, hh, ww);
  };
  for (int i = 0; i < 4; ++i) {
    const std::string nm = i < 3 ? "conv_blocks." + std::to_string(i) : std::string("bottle_neck");
    addz(p->enc[i].conv1, nm + ".conv1", H >> i, W >> i);
    addz(p->enc[i].conv2, nm + ".conv2", H >> i, W >> i);
    addz(p->enc[i].shortcut, nm + ".shortcut_conv", H >> i, W >> i);
  }
  for (int i = 0; i < 3; ++i) {
    const std::string si = std::to_string(i);
    const int lh = H >> (3 - i), lw = W >> (3 - i);
    addz(p->dec[i].gate, "gating_signals." + si, lh, lw);
    addz(p->dec[i].result, "attention_blocks." + si + ".result", 2 * lh, 2 * lw);
    addz(p->dec[i].conv, "ups." + si + ".conv_bn", lh, lw);
  }
  p->bn_sums_bytes = align_up(sums_cur);
  p->o_bn_sums = ws; ws += 2 * p->bn_sums_bytes;  // [forward | backward]
  p->red_bytes = std::max((size_t)kRedBlocks * 2 * 1024 * sizeof(double), (size_t)1024 * (9 * CCw * CCw + CCw) * 4);
  p->o_red = ws; ws += align_up(p->red_bytes);
  p->o_dtemb = ws; ws += align_up((size_t)B * p->temb_total * 4);
  p->o_scratch = ws; ws += align_up(64 * 1024);
  p->o_wgrad = ws; ws += align_up(kWgradPartialBytes);  // partial dW slices of the MFMA weight-gradient kernel
  p->g_out = p->T("grad.out", ws, B, cfg.out_dim, H, W);
  p->g_x0 = p->T("grad.x0", ws, B, 32, H, W);  // 16 channels at a 32-float pixel stride (unet_backward.hip: kGx0Stride)
  p->t_xn = p->T("x.nhwc", ws, B, cfg.image_channels, H, W);
  p->t_upn = p->T("upsampled_lr_img.nhwc", ws, B, CCw, H, W);
  p->g_upn = p->T("grad.upsampled_lr_img", ws, B, CCw, H, W);
  for (int i = 0; i < 4; ++i) p->g_lr[i] = p->T("grad.lr." + std::to_string(i), ws, B, CCw, h, w);
  for (int i = 0; i < 4; ++i) p->t_rn[i] = p->T("LR_encoder.r" + std::to_string(i) + ".nhwc", ws, B, CCw, h, w);
  for (int i = 0; i < 3; ++i) p->t_an[i] = p->T("LR_encoder.a" + std::to_string(i) + ".nhwc", ws, B, CCw, h, w);
  for (int i = 0; i < 4; ++i) {
    const int co = kDown[i + 1], hh = H >> i, ww = W >> i;
    p->g_R[i] = p->T("grad.R" + std::to_string(i), ws, B, co, hh, ww);
    p->g_H[i] = p->T("grad.H" + std::to_string(i), ws, B, co, hh, ww);
    if (i < 3) p->g_D[i] = p->T("grad.D" + std::to_string(i), ws, B, co, hh / 2, ww / 2);
  }
  for (int i = 0; i < 3; ++i) {
    const int Cc = kUp[i], Ch = kUp[i + 1];
    const int lh = H >> (3 - i), lw = W >> (3 - i);
    p->g_G[i] = p->T("grad.G" + std::to_string(i), ws, B, Ch, lh, lw);
    p->g_P[i] = p->T("grad.P" + std::to_string(i), ws, B, Ch, lh, lw);
    p->g_PSI[i] = p->T("grad.psi" + std::to_string(i), ws, B, 1, lh, lw);
    p->g_U[i] = p->T("grad.U" + std::to_string(i), ws, B, Cc, lh, lw);
    p->g_E[i] = p->T("grad.E" + std::to_string(i), ws, B, Ch, 2 * lh, 2 * lw);
    p->g_CAT[i] = p->T("grad.cat" + std::to_string(i), ws, B, Cc + Ch, 2 * lh, 2 * lw);
    p->g_X[i] = p->T("grad.X" + std::to_string(i), ws, B, Ch, 2 * lh, 2 * lw);
  }
}

extern "C" int drs_unet_plan_create(drs_plan** out, const drs_unet_config* cfg) {
  DRS_REQUIRE(out && cfg, DRS_ERR_ARG, "plan_create: null pointer");
  DRS_REQUIRE(cfg->batch >= 1 && (cfg->lr_batch == cfg->batch || cfg->lr_batch == 1), DRS_ERR_SHAPE,
              "plan_create: batch=%d lr_batch=%d (lr batch must equal batch or be 1)", cfg->batch, cfg->lr_batch);
  DRS_REQUIRE(cfg->image_channels >= 1 && cfg->image_channels <= kMaxBands && cfg->out_dim >= 1 && cfg->out_dim <= kMaxBands,
              DRS_ERR_SHAPE, "plan_create: image_channels=%d out_dim=%d (each 1..%d)", cfg->image_channels, cfg->out_dim,
              kMaxBands);
  DRS_REQUIRE(cfg->magnification >= 1 && cfg->height > 0 && cfg->width > 0 && cfg->height % 8 == 0 &&
                  cfg->width % 8 == 0 && cfg->height % cfg->magnification == 0 && cfg->width % cfg->magnification == 0,
              DRS_ERR_SHAPE, "plan_create: H=%d W=%d must be divisible by 8 and by magnification=%d", cfg->height,
              cfg->width, cfg->magnification);
  DRS_REQUIRE(cfg->impl >= DRS_IMPL_DIRECT && cfg->impl <= DRS_IMPL_MFMA_F16, DRS_ERR_ARG, "plan_create: impl=%d",
              cfg->impl);
  DRS_REQUIRE(cfg->variant >= DRS_VARIANT_SUPERRES && cfg->variant <= DRS_VARIANT_GENERATION, DRS_ERR_ARG,
              "plan_create: variant=%d", cfg->variant);
  DRS_REQUIRE(cfg->num_classes >= 0, DRS_ERR_ARG, "plan_create: num_classes=%d", cfg->num_classes);
  DRS_REQUIRE(!(cfg->flags & DRS_PLAN_FROZEN_BN) || (cfg->flags & DRS_PLAN_TRAIN), DRS_ERR_ARG,
              "plan_create: DRS_PLAN_FROZEN_BN needs DRS_PLAN_TRAIN (flags=%d; an eval plan folds the running statistics)",
              cfg->flags);
  std::unique_ptr<drs_plan> p(new drs_plan());
  p->cfg = *cfg;
  if (p->cfg.bn_eps <= 0.f) p->cfg.bn_eps = 1e-5f;
  if (p->cfg.variant == DRS_VARIANT_SUPERRES && p->cfg.cond_channels == 0) p->cfg.cond_channels = cfg->image_channels;
  if (p->cfg.variant == DRS_VARIANT_GENERATION) p->cfg.cond_channels = 0;
  const int CC = p->cfg.cond_channels;
  DRS_REQUIRE(p->cfg.variant == DRS_VARIANT_GENERATION || (CC >= 1 && CC <= kMaxBands), DRS_ERR_SHAPE,
              "plan_create: cond_channels=%d (1..%d)", CC, kMaxBands);
  DRS_REQUIRE(p->cfg.variant != DRS_VARIANT_SAR_TO_NDVI || cfg->magnification == 1, DRS_ERR_SHAPE,
              "plan_create: the SAR_TO_NDVI variant has no up-sampling (magnification must be 1)");
  plan_params(p.get());
  plan_kernel_forms(p.get());
  plan_packed_layout(p.get());
  size_t ws = 0;
  plan_eval_workspace(p.get(), ws);
  if (cfg->flags & DRS_PLAN_TRAIN) plan_train_workspace(p.get(), ws);
  p->ws_bytes = ws + 256;
  *out = p.release();
  return DRS_OK;
}

extern "C" void drs_unet_plan_destroy(drs_plan* plan) {
  if (!plan) return;
  if (plan->side) {
    (void)hipStreamSynchronize(plan->side);
    // (a failing destroy would leave a sticky HIP error for the caller's next runtime call to trip over)
    if (plan->ev_fork) (void)hipEventDestroy(plan->ev_fork);
    if (plan->ev_join) (void)hipEventDestroy(plan->ev_join);
    if (plan->ev_gbias) (void)hipEventDestroy(plan->ev_gbias);
    for (int i = 0; i < 3; ++i) {
      if (plan->ev_edge_in[i]) (void)hipEventDestroy(plan->ev_edge_in[i]);
      if (plan->ev_edge_out[i]) (void)hipEventDestroy(plan->ev_edge_out[i]);
    }
    (void)hipStreamDestroy(plan->side);
  }
  delete plan;
}
extern "C" int drs_unet_num_params(const drs_plan* plan) { return plan ? (int)plan->params.size() : 0; }
extern "C" const char* drs_unet_param_name(const drs_plan* plan, int i) {
  return (plan && i >= 0 && i < (int)plan->params.size()) ? plan->params[i].name.c_str() : nullptr;
}
extern "C" int64_t drs_unet_param_numel(const drs_plan* plan, int i) {
  return (plan && i >= 0 && i < (int)plan->params.size()) ? plan->params[i].numel : -1;
}
extern "C" size_t drs_unet_packed_bytes(const drs_plan* plan) { return plan ? plan->packed_bytes + 256 : 0; }
extern "C" size_t drs_unet_workspace_bytes(const drs_plan* plan) { return plan ? plan->ws_bytes : 0; }

// ------------------------------------------------------------------------------------------------
// introspection
// ------------------------------------------------------------------------------------------------
extern "C" int drs_unet_num_tensors(const drs_plan* plan) { return plan ? (int)plan->tensors.size() : 0; }
extern "C" const char* drs_unet_tensor_name(const drs_plan* plan, int i) {
  return (plan && i >= 0 && i < (int)plan->tensors.size()) ? plan->tensors[i].name.c_str() : nullptr;
}
extern "C" int drs_unet_tensor_shape(const drs_plan* plan, int i, int* n, int* c, int* h, int* w) {
  DRS_REQUIRE(plan && i >= 0 && i < (int)plan->tensors.size() && n && c && h && w, DRS_ERR_ARG, "tensor_shape: bad index");
  const WsTensor& t = plan->tensors[i];
  *n = t.n; *c = t.c; *h = t.h; *w = t.w;
  return DRS_OK;
}
extern "C" int drs_unet_read_tensor(const drs_plan* plan, int i, const void* workspace, float* dst, drs_stream_t stream) {
  DRS_REQUIRE(plan && workspace && dst && i >= 0 && i < (int)plan->tensors.size(), DRS_ERR_ARG, "read_tensor: bad args");
  const WsTensor& t = plan->tensors[i];
  const float* src = (const float*)(aligned_base(workspace) + t.off);
  if (t.planar) {
    DRS_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)t.n * t.c * t.h * t.w * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DRS_OK;
  }
  if (t.sp) return drs_launch_sp_to_nchw(src, dst, t.n, t.c, t.h, t.w, t.cs, t.co, (hipStream_t)stream);
  return drs_launch_nhwc_to_nchw(src, dst, t.n, t.c, t.h, t.w, t.cs, t.co, (hipStream_t)stream);
}
