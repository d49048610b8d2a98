// C-ABI of include/drs_hip.h: packing the parameters of a UNet plan into the images its kernels read.
#include "unet_plan.h"

// ---- weight packing: one step per layer family, in this order (it decides which jobs share a batched launch) ----
namespace {
struct PackCtx {  // base: the packed buffer's aligned base
  drs_plan* plan; const void* const* params; char* base; hipStream_t s;
  const float* F(int i) const { return (const float*)params[i]; }
};
}  // namespace

// Every convolution in its kernel family's layout (eval plans: BatchNorm folded in)
static int pack_layers(const PackCtx& c) {
  const drs_plan* plan = c.plan;
  for (const ConvLayer* L : plan->convs) {
    const float *g = nullptr, *be = nullptr, *rm = nullptr, *rv = nullptr;
    if (L->bn >= 0 && !(plan->cfg.flags & DRS_PLAN_TRAIN)) { g = c.F(L->bn); be = c.F(L->bn + 1); rm = c.F(L->bn + 2); rv = c.F(L->bn + 3); }
    if (L->mfma)
      RUN(drs_launch_pack_conv_mfma(c.F(L->w), c.F(L->b), g, be, rm, rv, plan->cfg.bn_eps, c.base + L->w_off, (float*)(c.base + L->b_off),
                                    L->Cout, L->Cin, L->taps, L->transposed ? 1 : 0, plan->cfg.impl, c.s, {.perm = L->out_sp}));
    else
      RUN(drs_launch_pack_conv(c.F(L->w), c.F(L->b), g, be, rm, rv, plan->cfg.bn_eps, (float*)(c.base + L->w_off),
                               (float*)(c.base + L->b_off), L->Cout, L->Cin, L->taps, L->transposed ? 1 : 0, 0, c.s));
  }
  return DRS_OK;
}

// conv1 (+BatchNorm1) and the skip convolution of a dual block as one 64-channel image, channels [0, 32) and [32, 64): two
// partial jobs, like the skip half alone would be, so that they share a launch and an image
static int pack_dual_pairs(const PackCtx& c) {
  const drs_plan* plan = c.plan;
  for (const ResBlock& rb : plan->enc) {
    if (!rb.dual) continue;
    const ConvLayer &a = rb.conv1, &b = rb.skip;
    char* w = c.base + rb.dual_w_off;
    float* bias = (float*)(c.base + rb.dual_b_off);
    RUN(drs_launch_pack_conv_mfma(c.F(a.w), c.F(a.b), c.F(a.bn), c.F(a.bn + 1), c.F(a.bn + 2), c.F(a.bn + 3), plan->cfg.bn_eps, w, bias,
                                  64, a.Cin, 9, 0, plan->cfg.impl, c.s, {.cout_src = 32, .partial = 1, .perm = plan->sp}));
    RUN(drs_launch_pack_conv_mfma(c.F(b.w), c.F(b.b), nullptr, nullptr, nullptr, nullptr, 0.f, w, bias, 64, b.Cin, 9, 0,
                                  plan->cfg.impl, c.s, {.cout_src = 32, .co_off = 32, .partial = 1, .perm = plan->sp}));
  }
  return DRS_OK;
}

// Fused attention gates: w_g and w_x once more with the SP output-row permutation, and the fp32 gating weights
static int pack_fused_gates(const PackCtx& c) {
  const drs_plan* plan = c.plan;
  for (const DecStage& d : plan->dec) {
    if (!d.fused_gate) continue;
    // (no bias destination: the layers' own jobs - same batched launch - write d.wg.b_off / d.wx.b_off; two jobs of one launch
    //  storing to one slot was benign only while both computed bit-identical values)
    RUN(drs_launch_pack_conv_mfma(c.F(d.wg.w), c.F(d.wg.b), nullptr, nullptr, nullptr, nullptr, 0.f, c.base + d.fz_wg_off, nullptr,
                                  d.wg.Cout, d.wg.Cin, 1, 0, plan->cfg.impl, c.s, {.perm = 1}));
    RUN(drs_launch_pack_conv_mfma(c.F(d.wx.w), c.F(d.wx.b), nullptr, nullptr, nullptr, nullptr, 0.f, c.base + d.fz_wx_off, nullptr,
                                  d.wx.Cout, d.wx.Cin, 4, 0, plan->cfg.impl, c.s, {.perm = 1}));
    // fp32 [Cc][Ch] gating weights, BatchNorm folded (per-image bias of a stage input stored as x + temb)
    const ConvLayer& G = d.gate;
    RUN(drs_launch_pack_conv(c.F(G.w), c.F(G.b), c.F(G.bn), c.F(G.bn + 1), c.F(G.bn + 2), c.F(G.bn + 3), plan->cfg.bn_eps,
                             (float*)(c.base + d.gf_w_off), (float*)(c.base + d.gf_b_off), G.Cout, G.Cin, 1, 0, 0, c.s));
  }
  return DRS_OK;
}

// Decoder stage i on the composite kernel: SP att-half rows in stages 0 / 1; stage 2 hands its att-half over projected
static int pack_upfuse_stage(const PackCtx& c, int i) {
  const drs_plan* plan = c.plan;
  const DecStage& d = plan->dec[i];
  auto at = [&c](bool used, size_t off) { return used ? (float*)(c.base + off) : nullptr; };
  const UpfuseDst dst = {c.base + d.uf_w_off, at(true, d.uf_aux_off), c.base + d.uf_edge_off, c.base + d.ah_w_off,
                         at(true, d.ah_b_off), at(d.ah_proj, d.ah_tmp_off), at(d.gate_psi, d.ah_tmp2_off),
                         at(d.gate_psi, d.ah_tab_off), at(d.uf_proj, d.uf_tmpw_off), at(d.uf_proj, d.uf_tmpb_off),
                         at(d.uf_proj, d.ufp_w_off)};
  const ConvLayer& R = d.result;
  const float* res[6] = {c.F(R.w), c.F(R.b), c.F(R.bn), c.F(R.bn + 1), c.F(R.bn + 2), c.F(R.bn + 3)};
  return pack_upfuse_stage_images(dst, c.F(d.transform.w), c.F(d.transform.b), c.F(d.upconv.w), c.F(d.upconv.b),
                                  c.F(plan->output.w), c.F(plan->output.b), plan->cfg.out_dim, res, plan->cfg.bn_eps, kUp[i],
                                  kUp[i + 1], plan->cfg.impl, i < 2 ? 1 : 0, c.s);
}

// Parameters kept verbatim in the packed image: one gather-copy launch (44 hipMemcpyAsync calls before round 4), and the
// table the time-MLP kernel reads them through
static int pack_verbatim(const PackCtx& c) {
  drs_plan* plan = c.plan;
  std::vector<DrsCopyJob> copies;
  auto keep = [&](size_t off, int param, long long words) { copies.push_back({c.F(param), (float*)(c.base + off), words}); };
  for (PlanarConv* L : plan->planars) {
    keep(L->w_off, L->w, (long long)L->Cout * L->Cin * 9);
    keep(L->b_off, L->b, L->Cout);
  }
  std::vector<long long>& table = plan->mlp_table_host;  // (outlives the async copy)
  table.clear();
  for (Mlp* m : plan->mlps) {
    keep(m->o_w1, m->w1, (long long)m->dim * 100);
    keep(m->o_b1, m->b1, m->dim);
    keep(m->o_w2, m->w2, (long long)m->dim * m->dim);
    keep(m->o_b2, m->b2, m->dim);
    const long long row[6] = {(long long)m->o_w1, (long long)m->o_b1, (long long)m->o_w2, (long long)m->o_b2, m->dim, m->temb_off};
    table.insert(table.end(), row, row + 6);
  }
  DRS_CHECK_HIP(hipMemcpyAsync(c.base + plan->o_mlp_table, table.data(), table.size() * sizeof(long long), hipMemcpyHostToDevice, c.s));
  if (plan->label_emb >= 0) keep(plan->o_label, plan->label_emb, (long long)plan->cfg.num_classes * 100);
  keep(plan->o_out_w, plan->output.w, (long long)plan->cfg.out_dim * kUp[3]);
  keep(plan->o_out_b, plan->output.b, plan->cfg.out_dim);
  return drs_launch_gather_copy(copies.data(), (int)copies.size(), c.s);
}

// FL images from the split-bf16 images just packed + the range check of the folded weights: a layer whose weights fp16 cannot
// hold keeps the split-bf16 kernel (the flags cross to the host here: one stream synchronisation per pack of an eval plan)
static int pack_fl_images(const PackCtx& c) {
  drs_plan* plan = c.plan;
  unsigned* flags = (unsigned*)(c.base + plan->o_fl_flags);
  DRS_CHECK_HIP(hipMemsetAsync(flags, 0, (size_t)plan->fl_slots * 8, c.s));
  for (const ConvLayer* L : plan->convs)
    if (L->fl_slot >= 0 && L->mfma)
      RUN(drs_launch_fl_repack(c.base + L->w_off, c.base + L->fl_img_off, L->Cout, L->Cin, L->taps, flags + 2 * L->fl_slot, c.s));
  for (const DecStage& d : plan->dec)  // (att-halves of stages 0 / 1: Ch -> Ch)
    if (d.ah_fl_slot >= 0)
      RUN(drs_launch_fl_repack(c.base + d.ah_w_off, c.base + d.ah_fl_img_off, d.upconv.Cout, d.upconv.Cout, 9, flags + 2 * d.ah_fl_slot, c.s));
  std::vector<unsigned> host((size_t)plan->fl_slots * 2 + 2, 0u);
  DRS_CHECK_HIP(hipMemcpyAsync(host.data(), flags, (size_t)plan->fl_slots * 8, hipMemcpyDeviceToHost, c.s));
  DRS_CHECK_HIP(hipStreamSynchronize(c.s));
  for (ConvLayer* L : plan->convs) L->fl_ok = L->fl_slot >= 0 && L->mfma && host[2 * L->fl_slot] == 0u;
  for (DecStage& d : plan->dec) d.ah_fl_ok = d.ah_fl_slot >= 0 && host[2 * d.ah_fl_slot] == 0u;
  return DRS_OK;
}

extern "C" int drs_unet_pack_weights(drs_plan* plan, const void* const* params, const float* inv_freq_host,
                                     void* packed, size_t packed_bytes, drs_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  DRS_REQUIRE(plan && params && inv_freq_host && packed, DRS_ERR_ARG, "pack_weights: null pointer");
  DRS_REQUIRE(packed_bytes >= drs_unet_packed_bytes(plan), DRS_ERR_WORKSPACE, "pack_weights: packed buffer too small");
  for (size_t i = 0; i < plan->params.size(); ++i)
    DRS_REQUIRE(params[i], DRS_ERR_ARG, "pack_weights: param %s is null", plan->params[i].name.c_str());
  const PackCtx c{plan, params, aligned_base(packed), s};
  DRS_CHECK_HIP(hipMemcpyAsync(c.base + plan->o_inv_freq, inv_freq_host, 50 * 4, hipMemcpyHostToDevice, s));
  DrsPackQueueScope pack_queue;  // the MFMA operand images of all layers: a few batched launches at the end (drs_common.h)
  RUN(pack_layers(c));
  RUN(pack_dual_pairs(c));
  RUN(pack_fused_gates(c));
  for (int i = 0; i < 3; ++i)
    if (plan->dec[i].upfuse) RUN(pack_upfuse_stage(c, i));
  RUN(pack_verbatim(c));
  RUN(pack_queue.flush(s));
  if (plan->fl) RUN(pack_fl_images(c));
  DRS_CHECK_HIP(hipMemsetAsync(c.base + plan->o_zero, 0, 512, s));  // zero line + fault word
  plan->param_ptrs.assign(params, params + plan->params.size());
  plan->packed_ok = true;
  plan->packed_ptr = packed;
  return DRS_OK;
}
