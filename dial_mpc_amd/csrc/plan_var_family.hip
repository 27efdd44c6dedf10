// plan_var_family.hip -- the rollout kernel with per-plan / per-sample model constants (plan_var_kernel.h) of ONE robot family
// (-DDIAL_FAMILY=0..6, plant_family.hip's families and per-family flags).  dial_mpc_amd/_lib.py links the units into libdialplanvar.so
// (build_plan_var); family 0's unit also holds the table libdialhip.so looks up (dial_plan_var_ops_v1), indexed by dial_ctx::inst.
#include "kernel_list.h"
#include "plan_var_kernel.h"

#if DIAL_FAMILY == 0
#define DIAL_PLAN_D DimsGo2
#elif DIAL_FAMILY == 1
#define DIAL_PLAN_D DimsH1
#elif DIAL_FAMILY == 2
#define DIAL_PLAN_D DimsH1Loco
#elif DIAL_FAMILY == 3
#define DIAL_PLAN_D DimsAllegro
#elif DIAL_FAMILY == 4
#define DIAL_PLAN_D DimsMax
#elif DIAL_FAMILY == 5
#define DIAL_PLAN_D DimsGo2Crate
#elif DIAL_FAMILY == 6
#define DIAL_PLAN_D DimsH1PushCrate
#else
#error "DIAL_FAMILY must be 0 .. 6"
#endif

#define DIAL_PLAN_VAR_ARGS \
  size_t, hipStream_t, const void*, const dial_task*, const dial_cfg*, const dial::RolloutIO*, int, int, const int32_t*, int

template __global__ void rollout_var_kernel<DIAL_PLAN_D>(const CModel<DIAL_PLAN_D>*, const dial_task*, const dial_cfg*, dial::RolloutIO, int, int,
                                                          const int32_t*, int);
template hipError_t plan_var_launch<DIAL_PLAN_D>(DIAL_PLAN_VAR_ARGS);

#if DIAL_FAMILY == 0
extern template hipError_t plan_var_launch<DimsMax>(DIAL_PLAN_VAR_ARGS);
extern template hipError_t plan_var_launch<DimsH1>(DIAL_PLAN_VAR_ARGS);
extern template hipError_t plan_var_launch<DimsH1Loco>(DIAL_PLAN_VAR_ARGS);
extern template hipError_t plan_var_launch<DimsAllegro>(DIAL_PLAN_VAR_ARGS);
extern template hipError_t plan_var_launch<DimsGo2Crate>(DIAL_PLAN_VAR_ARGS);
extern template hipError_t plan_var_launch<DimsH1PushCrate>(DIAL_PLAN_VAR_ARGS);

extern "C" __attribute__((visibility("default"))) const dial_plan_var_ops* dial_plan_var_ops_v1(void) {
  static const dial_plan_var_ops ops = {
      DIAL_PLAN_VAR_ABI_VERSION,
      sizeof(dial_model), sizeof(dial_task), sizeof(dial_cfg), sizeof(dial::RolloutIO),
      {sizeof(CModel<DimsMax>), sizeof(CModel<DimsGo2>), sizeof(CModel<DimsH1>), sizeof(CModel<DimsH1Loco>), sizeof(CModel<DimsAllegro>),
       sizeof(CModel<DimsGo2Crate>), sizeof(CModel<DimsH1PushCrate>)},
      {&plan_var_launch<DimsMax>, &plan_var_launch<DimsGo2>, &plan_var_launch<DimsH1>, &plan_var_launch<DimsH1Loco>,
       &plan_var_launch<DimsAllegro>, &plan_var_launch<DimsGo2Crate>, &plan_var_launch<DimsH1PushCrate>}};
  return &ops;
}
#endif
