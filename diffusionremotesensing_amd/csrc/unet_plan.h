// The UNet plan as the host translation units share it: runtime.hip has the error state, conv_api.hip the TapConv builders
// and the operator entries, plan.hip plan creation, plan_pack.hip weight packing, unet_profile.hip the profiler and launch log,
// unet_forward.hip / unet_backward.hip the two schedules.  Host code only: no kernel file includes this header (a kernel file
// defines its own file-local structs and statics).
#pragma once
#include <string>
#include <vector>

#include "drs_common.h"

namespace drs_unet {

static inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
static inline char* aligned_base(const void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// A step of the weight packing or of the forward / backward (unet_backward.hip) schedule returns its first non-zero status
#define RUN(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// ------------------------------------------------------------------------------------------------
// TapConv builders and the convolution launch (conv_api.hip)
// ------------------------------------------------------------------------------------------------
TapConv conv_desc(const float* in, int N, int H, int W, int Cin, int in_cs, int in_co, const float* w, const float* bias,
                  float* out, int Cout, int out_cs, int out_co, int KH, int KW, int stride, int pad);
TapConv convT_phase_desc(const float* in, int N, int H, int W, int Cin, int in_cs, int in_co, const float* w, const float* bias,
                         float* out, int Cout, int out_cs, int out_co, int py, int px);
TapConv convT_fused_desc(const float* in, int N, int H, int W, int Cin, int in_cs, int in_co, const float* w, const float* bias,
                         float* out, int Cout, int out_cs, int out_co);
int run_conv(const TapConv& d, int impl, hipStream_t s);
double conv_flops(const TapConv& d);
double conv_bytes(const TapConv& d);

// Where the weights of one fused up-sampling stage go (upfuse_sp.hip: ups.i.transform composed with the x-half of up_convs.i,
// and the att-half of up_convs.i as its own Ch -> Ch 3x3 convolution).  The optional ones select the folded forms of the top
// stage (DecStage::ah_proj: ah_tmp, gate_psi: ah_tmp2 / ah_tab, uf_proj: uf_tmpw / uf_tmpb / ufp_w).
struct UpfuseDst {
  void* w; float* aux; void* edge;  // composite operand image, edge / bias weights, edge operand image
  void* ah_w; float* ah_b;          // att-half operand image, zero bias
  float *ah_tmp = nullptr, *ah_tmp2 = nullptr, *ah_tab = nullptr, *uf_tmpw = nullptr, *uf_tmpb = nullptr;
  void* ufp_w = nullptr;
};
int pack_upfuse_stage_images(const UpfuseDst& d, const float* t_w, const float* t_b, const float* v_w, const float* v_b,
                             const float* out_w, const float* out_b, int out_dim, const float* const* res, float eps, int Cc,
                             int Ch, int impl, int perm, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// UNet plan
// ------------------------------------------------------------------------------------------------

struct Param { std::string name; int64_t numel; };

struct ConvLayer {
  int w = -1, b = -1, bn = -1;  // param indices; bn = index of gamma (beta, mean, var follow)
  int Cout = 0, Cin = 0, taps = 0;
  bool transposed = false, mfma = false;
  bool out_sp = false;  // this layer stores its output in SP format: weights packed with the output-channel permutation
  size_t w_off = 0, b_off = 0;
  // eval split-bf16 plans: "FL" operand images of a wide 3x3 / 1x1 layer (conv_mfma_fl.hip: fp16 main + block-scaled fp6 cross
  // terms, derived from the packed split-bf16 images), fl_slot = its range flag (-1: no FL image); fl_ok: the folded weights
  // passed the pack-time fp16 range check
  size_t fl_img_off = 0;
  int fl_slot = -1;
  bool fl_ok = false;
  int t_Z = -1;         // train plans: pre-BatchNorm tensor
  int t_Zsp = -1;       // train plans, 3x3 stride-1 layers: SP-format copy of dZ for the wave-specialised data-gradient convolution
  size_t stats_off = 0;  // train plans: saved batch mean / rstd (2 x Cout floats) in the workspace
  size_t sums_off = 0;   // train plans: this layer's fp64 reduction slots (2 x Cout) inside the forward / backward sums regions
};
struct PlanarConv { int w = -1, b = -1; int Cout = 0, Cin = 0; size_t w_off = 0, b_off = 0; };
struct Mlp { int w1, b1, w2, b2, dim; size_t o_w1, o_b1, o_w2, o_b2; int temb_off; };

struct WsTensor {
  std::string name;
  size_t off;  // bytes into workspace
  int n, c, h, w;
  int cs, co;   // channel stride / offset (NHWC); planar tensors have cs = 0
  bool planar;
  bool sp = false;  // SP format (split bf16 hi | lo per 32-channel group, drs_common.h)
};

struct ResBlock {
  ConvLayer conv1, conv2, shortcut, skip; bool has_skip; Mlp mlp;
  // eval split-bf16 plans: conv1 (+BN1) and the skip convolution packed as ONE 2*Cout-channel operand image (TapConv::dual)
  bool dual = false;
  size_t dual_w_off = 0, dual_b_off = 0;
};
struct DecStage {
  ConvLayer gate, wg, wx, psi, result, conv, transform, upconv; Mlp mlp;
  // fused attention gate (attn_gate_sp.hip): w_g and w_x once more with the SP output-row permutation
  bool fused_gate = false;
  size_t fz_wg_off = 0, fz_wx_off = 0;
  // the stage input is stored ONLY as x + relu(time_mlp(t)) (what ups.i.conv reads) when the fused gate can take the row
  // vector out through a per-image bias: fp32 BatchNorm-folded gating weights [Cc][Ch] + bias, per-forward bias table
  size_t gf_w_off = 0, gf_b_off = 0, o_gbias = 0;
  // ups.i.transform composed with the x-half of up_convs.i (upfuse_sp.hip): composite operand image, edge / bias weights,
  // and the att-half of up_convs.i packed as its own Ch -> Ch 3x3 convolution (no bias: it is in the composite's)
  bool upfuse = false;
  size_t uf_w_off = 0, uf_aux_off = 0, uf_edge_off = 0, ah_w_off = 0, ah_b_off = 0;
  size_t ah_fl_img_off = 0;  // FL images of the att-half (stages 0 / 1)
  int ah_fl_slot = -1;
  bool ah_fl_ok = false;
  // stage 2: the `output` projection folded into the att-half's weights (conv3x3_direct_sp.hip, TapConv::proj): a 16-row image,
  // ah_tmp = the fp32 contraction it is packed from
  bool ah_proj = false;
  size_t ah_tmp_off = 0;
  // ... and into the composite's (UpFuseDesc::proj), on the streaming kernel (upfuse_proj_sp.hip): the folded up_convs.2
  // x-half the composite is packed from, and that kernel's own operand image
  bool uf_proj = false;
  size_t uf_tmpw_off = 0, uf_tmpb_off = 0, ufp_w_off = 0;
  // ... and the attention block's `result` convolution folded in as well: the gate stops at psi (attn_gate_sp.hip, PSI_ONLY), the
  // att-half reads the skip tensor and multiplies by psi behind its MFMAs: `att` of the top stage never exists
  bool gate_psi = false;
  size_t ah_tmp2_off = 0, ah_tab_off = 0;
  int t_PA = -1;                  // att-half partial sums (SP), B x Ch x 2lh x 2lw
  size_t o_eh = 0, o_ev = 0;      // workspace: edge vectors of this forward
};

}  // namespace drs_unet

// (drs_plan is the C-ABI's opaque type, so it is defined at global scope; it and the host files name drs_unet's types and
//  helpers unqualified)
using namespace drs_unet;

struct drs_plan {
  drs_unet_config cfg;
  std::vector<Param> params;
  std::vector<ConvLayer*> convs;
  std::vector<PlanarConv*> planars;
  std::vector<Mlp*> mlps;
  std::vector<WsTensor> tensors;

  PlanarConv rrdb[7];
  PlanarConv stem0, stemc;  // conv0, conv_upsampled_lr_img (raw torch layout)
  ResBlock enc[4];          // conv_blocks.0..2, bottle_neck
  ConvLayer downs[3];
  DecStage dec[3];
  ConvLayer output;

  size_t packed_bytes = 0, ws_bytes = 0;
  size_t o_inv_freq = 0, o_mlp_table = 0, o_out_w = 0, o_out_b = 0, o_label = 0, o_zero = 0, o_fault = 0;
  // eval plans of the split-bf16 implementation keep every MFMA-consumed activation in SP format (drs_common.h)
  bool sp = false;
  // train plans with DRS_PLAN_FROZEN_BN: every BatchNorm normalises with the running statistics (read-only), forward and backward
  bool frozen_bn() const { return (cfg.flags & DRS_PLAN_FROZEN_BN) != 0; }
  int t_XT[3] = {-1, -1, -1};  // x + relu(time_mlp(t)) of UpConvBlock i (reference :199), second output of its producer
  int label_emb = -1;  // param index of label_emb.weight (generation variant)
  int temb_total = 0;
  std::vector<long long> mlp_table_host;
  std::vector<const void*> param_ptrs;  // as given to the last drs_unet_pack_weights
  // train plans: fp64 totals of the BatchNorm reductions, one (2 x Cout) slot per layer, a region for the forward statistics
  // followed by one for the backward sums; o_red = per-block partial sums of whichever reduction is running on the main
  // stream (BatchNorm statistics, BatchNorm backward, bias-gradient column sums: kRedBlocks x 2 x 1024 doubles).  Partials +
  // a small finishing kernel replaced per-block atomics onto the same 2 x Cout addresses: 512 blocks x 90 ns per serialised
  // atomic = a 46 us floor under every one of those launches, whatever the tensor size (round 3: 63 of them per step).
  // (also the partial rows of the few-channel LR / SAR encoder backward: 1024 x (9 CC^2 + CC) floats, stem_bwd.hip)
  size_t o_bn_sums = 0, bn_sums_bytes = 0, o_red = 0, red_bytes = 0;
  // FL arithmetic (conv_mfma_fl.hip) for the layers the wave-specialised SP kernel takes at 64 channels per item; per-layer range
  // flags (device words, one per FL image: bit 0 = a folded weight outside what fp16 holds) are read back at pack time
  bool fl = false;
  bool fl_disabled = false;  // an activation left fp16's range (drs_unet_check_faults): the plan stays on the split-bf16 kernels
  int fl_slots = 0;
  size_t o_fl_flags = 0;
  bool packed_ok = false;
  const void* packed_ptr = nullptr;
  unsigned* fault_ptr = nullptr;  // device word of the current forward's packed buffer (TapConv::fault)

  // optional per-op timing (drs_unet_profile_*): events recorded on the forward's stream
  struct OpRec { std::string name; double flops, bytes; hipEvent_t e0, e1; };
  bool profiling = false;
  std::vector<OpRec> ops;
  // launch log of the last profiled forward (drs_note_launch): one entry per kernel launch, in host launch order
  struct LaunchRec { std::string op, kernel; };
  std::vector<LaunchRec> launches;
  std::string cur_op;  // op of the schedule whose prof_begin / prof_end bracket is open ("" between ops)

  // workspace offsets
  size_t o_lr[3], o_up, o_temb;
  int t_cond, t_x0, t_S[4], t_K0, t_H[4], t_R[4], t_D[3];
  int t_G[3], t_Q[3], t_P[3], t_PSI[3], t_U[3], t_CAT[3], t_X[3];
  int t_lrenc, t_up;
  // train plans: gradients of activations and channels-last copies of the 3-channel tensors (backward only)
  int g_out = -1, g_X[3], g_CAT[3], g_U[3], g_G[3], g_P[3], g_PSI[3], g_E[3], g_R[4], g_D[3], g_H[4], g_x0 = -1;
  int t_xn = -1, t_upn = -1, g_upn = -1, g_lr[4], t_rn[4], t_an[3];
  size_t o_dtemb = 0, o_scratch = 0, o_wgrad = 0;
  // second stream of the eval forward: the attention branch of a decoder stage runs next to the up-sampling branch
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_gbias = nullptr;
  hipEvent_t ev_edge_in[3] = {nullptr, nullptr, nullptr}, ev_edge_out[3] = {nullptr, nullptr, nullptr};  // edge vectors of a composite stage: side stream

  int P(const std::string& name, int64_t numel) {
    params.push_back({name, numel});
    return (int)params.size() - 1;
  }
  ConvLayer mk_conv(const std::string& pfx, int Cout, int Cin, int taps, const std::string& bn_pfx = "",
                    bool transposed = false) {
    ConvLayer L;
    L.Cout = Cout; L.Cin = Cin; L.taps = taps; L.transposed = transposed;
    L.w = P(pfx + ".weight", (int64_t)Cout * Cin * taps);
    L.b = P(pfx + ".bias", Cout);
    if (!bn_pfx.empty()) {
      L.bn = P(bn_pfx + ".weight", Cout);
      P(bn_pfx + ".bias", Cout);
      P(bn_pfx + ".running_mean", Cout);
      P(bn_pfx + ".running_var", Cout);
    }
    return L;
  }
  PlanarConv mk_planar(const std::string& pfx, int Cout, int Cin) {
    PlanarConv L;
    L.Cout = Cout; L.Cin = Cin;
    L.w = P(pfx + ".weight", (int64_t)Cout * Cin * 9);
    L.b = P(pfx + ".bias", Cout);
    return L;
  }
  Mlp mk_mlp(const std::string& pfx, int dim) {
    Mlp m;
    m.dim = dim;
    m.w1 = P(pfx + ".0.weight", (int64_t)dim * 100);
    m.b1 = P(pfx + ".0.bias", dim);
    m.w2 = P(pfx + ".2.weight", (int64_t)dim * dim);
    m.b2 = P(pfx + ".2.bias", dim);
    m.temb_off = temb_total;
    temb_total += dim;
    return m;
  }
  int T(const std::string& name, size_t& cursor, int n, int c, int h, int w, bool planar = false) {
    WsTensor t{name, cursor, n, c, h, w, planar ? 0 : c, 0, planar, false};
    cursor += align_up((size_t)n * c * h * w * 4);
    tensors.push_back(t);
    return (int)tensors.size() - 1;
  }
  int Tview(const std::string& name, int base, int c, int co) {
    WsTensor t = tensors[base];
    t.name = name; t.c = c; t.co = co;
    tensors.push_back(t);
    return (int)tensors.size() - 1;
  }
  float* tp(void* ws, int i) const { return (float*)((char*)ws + tensors[i].off); }
};

namespace drs_unet {

static const size_t kWgradPartialBytes = 64ull << 20;
static const int kRedBlocks = DRS_RED_BLOCKS;  // blocks of a partial-sum reduction (drs_common.h)
static const int kDown[5] = {16, 32, 64, 128, 256};
static const int kUp[5] = {256, 128, 64, 32, 16};

// ------------------------------------------------------------------------------------------------
// per-op timing and launch log (unet_profile.hip)
// ------------------------------------------------------------------------------------------------
void prof_begin(drs_plan* plan, const std::string& name, double flops, double bytes, hipStream_t s);
void prof_end(drs_plan* plan, hipStream_t s);
struct LaunchLogScope {  // active for the duration of one drs_unet_forward of a profiling plan
  explicit LaunchLogScope(drs_plan* p);
  ~LaunchLogScope();
};

// A profiled op that is not a layer's TapConv (plan_conv brackets those itself)
template <class Launch>
static int prof_op(drs_plan* plan, const std::string& name, double flops, double bytes, hipStream_t s, Launch launch) {
  prof_begin(plan, name, flops, bytes, s);
  const int rc = launch();
  prof_end(plan, s);
  return rc;
}

}  // namespace drs_unet
