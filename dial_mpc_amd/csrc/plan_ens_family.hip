// plan_ens_family.hip -- the ensemble rollout kernel (plan_ens_kernel.h: dial_set_plan_ensemble) of ONE robot family
// (-DDIAL_FAMILY=0..6, plant_family.hip's families and per-family flags).  dial_mpc_amd/_lib.py links the units and
// plan_ens_aggregate.hip into libdialplanens.so (build_plan_ens); family 0's unit also holds the table libdialhip.so looks up
// (dial_plan_ens_ops_v1), indexed by dial_ctx::inst.
#include "kernel_list.h"
#include "plan_ens_kernel.h"

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

#define DIAL_PLAN_ENS_ARGS \
  size_t, hipStream_t, const void*, const dial_task*, const dial_cfg*, const dial::RolloutIO*, int, int, int, const int32_t*, float*

template __global__ void rollout_ens_kernel<DIAL_PLAN_D>(const CModel<DIAL_PLAN_D>*, const dial_task*, const dial_cfg*, dial::RolloutIO, int, int,
                                                          int, const int32_t*, float*);
template hipError_t plan_ens_launch<DIAL_PLAN_D>(DIAL_PLAN_ENS_ARGS);

#if DIAL_FAMILY == 0
extern template hipError_t plan_ens_launch<DimsMax>(DIAL_PLAN_ENS_ARGS);
extern template hipError_t plan_ens_launch<DimsH1>(DIAL_PLAN_ENS_ARGS);
extern template hipError_t plan_ens_launch<DimsH1Loco>(DIAL_PLAN_ENS_ARGS);
extern template hipError_t plan_ens_launch<DimsAllegro>(DIAL_PLAN_ENS_ARGS);
extern template hipError_t plan_ens_launch<DimsGo2Crate>(DIAL_PLAN_ENS_ARGS);
extern template hipError_t plan_ens_launch<DimsH1PushCrate>(DIAL_PLAN_ENS_ARGS);

extern "C" __attribute__((visibility("default"))) const dial_plan_ens_ops* dial_plan_ens_ops_v1(void) {
  static const dial_plan_ens_ops ops = {
      DIAL_PLAN_ENS_ABI_VERSION,
      sizeof(dial_model), sizeof(dial_task), sizeof(dial_cfg), sizeof(dial::RolloutIO),
      {sizeof(CModel<DimsMax>), sizeof(CModel<DimsGo2>), sizeof(CModel<DimsH1>), sizeof(CModel<DimsH1Loco>), sizeof(CModel<DimsAllegro>),
       sizeof(CModel<DimsGo2Crate>), sizeof(CModel<DimsH1PushCrate>)},
      {&plan_ens_launch<DimsMax>, &plan_ens_launch<DimsGo2>, &plan_ens_launch<DimsH1>, &plan_ens_launch<DimsH1Loco>,
       &plan_ens_launch<DimsAllegro>, &plan_ens_launch<DimsGo2Crate>, &plan_ens_launch<DimsH1PushCrate>},
      &dial_plan_ens_aggregate};
  return &ops;
}
#endif
