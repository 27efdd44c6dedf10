// plugin.hip -- the translation unit of a task plugin (dial_mpc_amd/plugin.py builds it): the rollout / env.step / env.reset kernels
// of ONE model's compile-time dimensions with a user reward fused in, and the table of host functions libdialhip.so calls for
// them (plugin_ops.h, dial_create_plugin).  The build generates two files next to its objects:
//   dial_plugin_dims.h    #define DIAL_PLUGIN_NQ ... DIAL_PLUGIN_NFRI  (the model's dimensions)
//   dial_user_reward.hip  the user's definition of dial_user_reward (user_reward.h states the contract)
#include "plugin_ops.h"
#include "dial_plugin_dims.h"
#include "dial_user_reward.hip"

// one wavefront per workgroup (the capacity-dimension kernel's shape): the mean-trajectory relay applies, no split launches
#define DIAL_PLUGIN_WPB 1
using DimsPlugin = DimsUser<DIAL_PLUGIN_NQ, DIAL_PLUGIN_NV, DIAL_PLUGIN_NU, DIAL_PLUGIN_NB, DIAL_PLUGIN_NJ, DIAL_PLUGIN_NG, DIAL_PLUGIN_NS,
                            DIAL_PLUGIN_NC, DIAL_PLUGIN_NL, DIAL_PLUGIN_NFRI>;

template __global__ void rollout_kernel<DimsPlugin, DIAL_PLUGIN_WPB, 3, false, false>(const CModel<DimsPlugin>*, const dial_task*, const dial_cfg*,
                                                                                  dial::RolloutIO, int, int, int*);
template __global__ void rollout_kernel<DimsPlugin, DIAL_PLUGIN_WPB, 3, true, false>(const CModel<DimsPlugin>*, const dial_task*, const dial_cfg*,
                                                                                 dial::RolloutIO, int, int, int*);
template __global__ void rollout_kernel<DimsPlugin, DIAL_PLUGIN_WPB, 3, false, true>(const CModel<DimsPlugin>*, const dial_task*, const dial_cfg*,
                                                                                 dial::RolloutIO, int, int, int*);
template __global__ void env_step_kernel<DimsPlugin>(const CModel<DimsPlugin>*, const dial_task*, float*, const float*, float*, float*, float*,
                                                      const float*);
template __global__ void env_reset_kernel<DimsPlugin>(const CModel<DimsPlugin>*, const float*, const float*, float*, float*, float*);

extern "C" __attribute__((visibility("default"))) const dial_plugin_ops* dial_plugin_ops_v1(void) {
  return PluginOps<DimsPlugin, DIAL_PLUGIN_WPB>::table();
}
