// C-ABI of include/drs_hip.h: the library's error state and ABI version, and the per-device kernel set-up every launcher calls.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <mutex>
#include <utility>

#include "drs_common.h"

// ------------------------------------------------------------------------------------------------
// error state
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void DrsErr::set(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* drs_last_error(void) { return g_err; }
extern "C" int drs_abi_version(void) { return 8; }

int drs_kernel_prepare(const void* kernel, int max_dynamic_lds, int* num_cu) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, bool> attr_set;  // (device, kernel) -> dynamic-LDS attribute applied
  static std::map<int, int> cus;                                  // device -> CU count
  int dev = 0;
  DRS_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = cus.find(dev);
  if (it == cus.end()) {
    int n = 0;
    DRS_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    it = cus.emplace(dev, n).first;
  }
  *num_cu = it->second;
  bool& done = attr_set[std::make_pair(dev, kernel)];
  if (!done && max_dynamic_lds > 0) {
    DRS_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, max_dynamic_lds));
    done = true;
  }
  return DRS_OK;
}
