// reward_defer.hip -- libdialdefer.so: the Go2's rollout kernel with the step rewards evaluated once per rollout
// (reward_defer_kernel.h) and the table libdialhip.so looks up.  dial_mpc_amd/_lib.py builds it with the product flags
// (build_reward_defer); the IEEE measurement variant links this unit into libdialhip_ieee.so itself.
#include "reward_defer_kernel.h"

template __global__ void rollout_defer_kernel<DimsGo2>(const CModel<DimsGo2>*, const dial_task*, const dial_cfg*, dial::RolloutIO, int, int);

extern "C" __attribute__((visibility("default"))) const dial_reward_defer_ops* dial_reward_defer_ops_v1(void) {
  static const dial_reward_defer_ops ops = {DIAL_REWARD_DEFER_ABI_VERSION, sizeof(dial_task), sizeof(dial_cfg), sizeof(dial::RolloutIO),
                                            sizeof(CModel<DimsGo2>), &reward_defer_launch<DimsGo2>, &reward_defer_occupancy<DimsGo2>};
  return &ops;
}
