// update_rule.hip -- libdialupdate.so: the K4a kernel of the elite update rule (update_rule.h: elite_weights_kernel) and the launcher
// libdialhip.so looks up.  dial_mpc_amd/_lib.py builds it with the product flags (build_update_rule); the IEEE measurement variant
// links this unit into libdialhip_ieee.so itself.
#include <hip/hip_runtime.h>

#define DIAL_UPDATE_RULE_KERNEL 1
#include "update_rule.h"

extern "C" __attribute__((visibility("default"))) hipError_t dial_update_rule_launch_v1(hipStream_t st, int plans, const float* rews, int B, int K,
                                                                                         float* weights, const float* gathered, int per,
                                                                                         float* rews_out) {
  hipLaunchKernelGGL(elite_weights_kernel, dim3(plans), dim3(UR_THREADS), 0, st, rews, B, K, weights, gathered, per, rews_out);
  return hipGetLastError();
}
