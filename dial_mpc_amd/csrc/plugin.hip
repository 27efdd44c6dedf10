// plugin.hip -- the translation unit of a task plugin (dial_mpc_amd/plugin.py builds it): the rollout / env.step / env.reset kernels
// of ONE model's compile-time dimensions with a user reward fused in, and the table of host functions libdialhip.so calls for
// them (plugin_ops.h, dial_create_plugin).  The build generates two files next to its objects:
//   dial_plugin_dims.h    #define DIAL_PLUGIN_NQ ... DIAL_PLUGIN_NFRI  (the model's dimensions)
//   dial_user_reward.hip  the user's definition of dial_user_reward (user_reward.h states the contract)
// and, for a plugin with a user control law (-DDIAL_PLUGIN_USER_CTRL=1), a third:
//   dial_user_control.hip the user's definition of dial_user_control (user_control.h states the contract)
// Such a plugin carries one more kernel, user_control_kernel, and exports a second table (plugin_ops.h: dial_plugin_ctrl).
// Every plugin exports a third, dial_plugin_table (the reference table of dial_set_user_table: host code only, no kernel).
// A plugin built with a plant (-DDIAL_PLUGIN_PLANT=1) carries plant_kernel<DimsPlugin> (plant_kernel.h: the kernel of the built-in
// families, with the law as a third control mode) and exports a fourth, dial_plugin_plant (plant_plugin.h: dial_plant_step on the
// plugin's contexts).  -DDIAL_PLUGIN_PLANT_DIST=1 next to it (build_plugin(plant_disturbance=True)) adds plant_dist_kernel<DimsPlugin>
// (plant_dist_kernel.h: velocity kicks and actuator errors, dial_set_plant_disturbance) and a fifth table, dial_plugin_plant_dist.
// -DDIAL_PLUGIN_PLANT_VAR=1 next to DIAL_PLUGIN_PLANT (build_plugin(plant_models=True)) adds plant_var_kernel<DimsPlugin>
// (plant_var_kernel.h: per-plant model constants, dial_set_plant_models) and a sixth table, dial_plugin_plant_var.
// -DDIAL_PLUGIN_PLAN_VAR=1 (build_plugin(plan_models=True), with or without a plant) adds rollout_var_kernel<DimsPlugin>
// (plan_var_kernel.h: per-plan / per-sample planner models, dial_set_plan_models) and a seventh table, dial_plugin_plan_var.
// -DDIAL_PLUGIN_PLAN_ENS=1 (build_plugin(plan_ensemble=True), after every other define) adds rollout_ens_kernel<DimsPlugin>
// (plan_ens_kernel.h: robust planning over a model ensemble, dial_set_plan_ensemble) and an eighth table, dial_plugin_plan_ens; the
// aggregation kernel of such a context is libdialplanens.so's.
#include "plugin_ops.h"
#ifndef DIAL_PLUGIN_PLANT
#define DIAL_PLUGIN_PLANT 0
#endif
#ifndef DIAL_PLUGIN_PLANT_DIST
#define DIAL_PLUGIN_PLANT_DIST 0
#endif
#if DIAL_PLUGIN_PLANT_DIST && !DIAL_PLUGIN_PLANT
#error "DIAL_PLUGIN_PLANT_DIST needs DIAL_PLUGIN_PLANT"
#endif
#ifndef DIAL_PLUGIN_PLANT_VAR
#define DIAL_PLUGIN_PLANT_VAR 0
#endif
#if DIAL_PLUGIN_PLANT_VAR && !DIAL_PLUGIN_PLANT
#error "DIAL_PLUGIN_PLANT_VAR needs DIAL_PLUGIN_PLANT"
#endif
#if DIAL_PLUGIN_PLANT
#include "plant_plugin.h"
#endif
#if DIAL_PLUGIN_PLANT_DIST
#include "plant_dist_kernel.h"
#endif
#if DIAL_PLUGIN_PLANT_VAR
#include "plant_var_kernel.h"
#endif
#ifndef DIAL_PLUGIN_PLAN_VAR
#define DIAL_PLUGIN_PLAN_VAR 0
#endif
#if DIAL_PLUGIN_PLAN_VAR
#include "plan_var_kernel.h"
#endif
#ifndef DIAL_PLUGIN_PLAN_ENS
#define DIAL_PLUGIN_PLAN_ENS 0
#endif
#if DIAL_PLUGIN_PLAN_ENS
#include "plan_ens_kernel.h"
#endif
#include "dial_plugin_dims.h"
#include "dial_user_reward.hip"
#ifndef DIAL_PLUGIN_USER_CTRL
#define DIAL_PLUGIN_USER_CTRL 0
#endif
#if DIAL_PLUGIN_USER_CTRL
#include "dial_user_control.hip"
#endif

// one wavefront per workgroup (the capacity-dimension kernel's shape): the mean-trajectory relay applies, no split launches
#define DIAL_PLUGIN_WPB 1
using DimsPlugin = DimsUser<DIAL_PLUGIN_NQ, DIAL_PLUGIN_NV, DIAL_PLUGIN_NU, DIAL_PLUGIN_NB, DIAL_PLUGIN_NJ, DIAL_PLUGIN_NG, DIAL_PLUGIN_NS,
                            DIAL_PLUGIN_NC, DIAL_PLUGIN_NL, DIAL_PLUGIN_NFRI, DIAL_PLUGIN_USER_CTRL != 0>;

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

// the reference table's host function (plugin_ops.h: dial_plugin_table): every plugin exports it, with or without a law
// (-DDIAL_PLUGIN_NO_TABLE: a plugin as the sources before the table built it -- the tests' stand-in for an older plugin)
#ifndef DIAL_PLUGIN_NO_TABLE
extern "C" __attribute__((visibility("default"))) const dial_plugin_table* dial_plugin_table_v1(void) {
  return PluginTable<DimsPlugin>::table();
}
#endif

#if DIAL_PLUGIN_USER_CTRL
template __global__ void user_control_kernel<DimsPlugin>(const CModel<DimsPlugin>*, const float*, const float*, float*, const float*);

extern "C" __attribute__((visibility("default"))) const dial_plugin_ctrl* dial_plugin_ctrl_v1(void) {
  return PluginCtrl<DimsPlugin>::table();
}
#endif

#if DIAL_PLUGIN_PLANT
template __global__ void plant_kernel<DimsPlugin>(const CModel<DimsPlugin>*, float*, double*, const float*, const float*, int, double, double,
                                                   int, int, float*);

extern "C" __attribute__((visibility("default"))) const dial_plugin_plant* dial_plugin_plant_v1(void) {
  return PluginPlant<DimsPlugin>::table();
}
#endif

#if DIAL_PLUGIN_PLANT_DIST
template __global__ void plant_dist_kernel<DimsPlugin>(const CModel<DimsPlugin>*, float*, double*, const float*, const float*, int, double, double,
                                                        int, int, float*, const float*, int);

extern "C" __attribute__((visibility("default"))) const dial_plugin_plant_dist* dial_plugin_plant_dist_v1(void) {
  return PluginPlantDist<DimsPlugin>::table();
}
#endif

#if DIAL_PLUGIN_PLANT_VAR
template __global__ void plant_var_kernel<DimsPlugin>(const CModel<DimsPlugin>*, float*, double*, const float*, const float*, int, double, double,
                                                       int, int, float*, const float*, int, const int32_t*);

extern "C" __attribute__((visibility("default"))) const dial_plugin_plant_var* dial_plugin_plant_var_v1(void) {
  return PluginPlantVar<DimsPlugin>::table();
}
#endif

#if DIAL_PLUGIN_PLAN_VAR
template __global__ void rollout_var_kernel<DimsPlugin>(const CModel<DimsPlugin>*, const dial_task*, const dial_cfg*, dial::RolloutIO, int, int,
                                                         const int32_t*, int);

extern "C" __attribute__((visibility("default"))) const dial_plugin_plan_var* dial_plugin_plan_var_v1(void) {
  return PluginPlanVar<DimsPlugin>::table();
}
#endif

#if DIAL_PLUGIN_PLAN_ENS
template __global__ void rollout_ens_kernel<DimsPlugin>(const CModel<DimsPlugin>*, const dial_task*, const dial_cfg*, dial::RolloutIO, int, int, int,
                                                         const int32_t*, float*);

extern "C" __attribute__((visibility("default"))) const dial_plugin_plan_ens* dial_plugin_plan_ens_v1(void) {
  return PluginPlanEns<DimsPlugin>::table();
}
#endif
