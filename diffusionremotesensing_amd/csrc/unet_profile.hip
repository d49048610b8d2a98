// C-ABI of include/drs_hip.h: per-op timing of a UNet plan's forward and the launch log of a profiled forward.
#include <stdio.h>
#include <stdlib.h>
#include <cxxabi.h>

#include "unet_plan.h"

namespace drs_unet {
void prof_begin(drs_plan* plan, const std::string& name, double flops, double bytes, hipStream_t s) {
  if (!plan->profiling) return;
  drs_plan::OpRec r{name, flops, bytes, nullptr, nullptr};
  (void)hipEventCreate(&r.e0);
  (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, s);
  plan->ops.push_back(r);
  plan->cur_op = name;
}
void prof_end(drs_plan* plan, hipStream_t s) {
  if (!plan->profiling) return;
  (void)hipEventRecord(plan->ops.back().e1, s);
  plan->cur_op.clear();
}
}  // namespace drs_unet

// Launch log (DRS_LAUNCH, drs_common.h): the plan whose profiled forward is running on this host thread, if any.
static thread_local drs_plan* tls_logged_plan = nullptr;
void drs_note_launch(const void* kernel_fn, const char* expr) {
  drs_plan* plan = tls_logged_plan;
  if (!plan) return;
  const char* nm = hipKernelNameRefByPtr(kernel_fn, nullptr);  // mangled name of the device function
  std::string kname = nm ? nm : expr;
  int status = 0;
  if (char* dm = abi::__cxa_demangle(kname.c_str(), nullptr, nullptr, &status)) {
    if (status == 0) kname = dm;
    free(dm);
  }
  plan->launches.push_back({plan->cur_op, kname});
}
namespace drs_unet {
LaunchLogScope::LaunchLogScope(drs_plan* p) { if (p && p->profiling) { p->launches.clear(); p->cur_op.clear(); tls_logged_plan = p; } }
LaunchLogScope::~LaunchLogScope() { tls_logged_plan = nullptr; }
}  // namespace drs_unet

// ------------------------------------------------------------------------------------------------
// per-op timing
// ------------------------------------------------------------------------------------------------
extern "C" int drs_unet_profile_enable(drs_plan* plan, int on) {
  DRS_REQUIRE(plan, DRS_ERR_ARG, "profile_enable: null plan");
  plan->profiling = on != 0;
  return DRS_OK;
}
extern "C" int drs_unet_profile_num_ops(const drs_plan* plan) { return plan ? (int)plan->ops.size() : 0; }
extern "C" int drs_unet_profile_read(drs_plan* plan, int i, char* name, int name_len, float* ms, double* flops,
                                     double* bytes) {
  DRS_REQUIRE(plan && i >= 0 && i < (int)plan->ops.size() && name && ms && flops && bytes, DRS_ERR_ARG,
              "profile_read: bad args");
  drs_plan::OpRec& r = plan->ops[i];
  DRS_CHECK_HIP(hipEventSynchronize(r.e1));
  DRS_CHECK_HIP(hipEventElapsedTime(ms, r.e0, r.e1));
  snprintf(name, name_len, "%s", r.name.c_str());
  *flops = r.flops;
  *bytes = r.bytes;
  return DRS_OK;
}

extern "C" int drs_unet_profile_num_launches(const drs_plan* plan) { return plan ? (int)plan->launches.size() : 0; }
extern "C" int drs_unet_profile_launch(const drs_plan* plan, int i, char* op, int op_len, char* kernel, int kernel_len) {
  DRS_REQUIRE(plan && i >= 0 && i < (int)plan->launches.size() && op && kernel && op_len > 0 && kernel_len > 0, DRS_ERR_ARG,
              "profile_launch: bad args");
  snprintf(op, op_len, "%s", plan->launches[i].op.c_str());
  snprintf(kernel, kernel_len, "%s", plan->launches[i].kernel.c_str());
  return DRS_OK;
}
