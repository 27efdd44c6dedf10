// plant_var_family.hip -- the plant kernel with per-plant model constants (plant_var_kernel.h) of ONE robot family (-DDIAL_FAMILY=0..6,
// plant_family.hip's families and per-family flags).  dial_mpc_amd/_lib.py links the units into libdialplantvar.so (build_plant_var);
// family 0's unit also holds the table libdialhip.so looks up (dial_plant_var_ops_v1), indexed by dial_ctx::inst.
#include "kernel_list.h"
#include "plant_var_kernel.h"

#if DIAL_FAMILY == 0
#define DIAL_PLANT_D DimsGo2
#elif DIAL_FAMILY == 1
#define DIAL_PLANT_D DimsH1
#elif DIAL_FAMILY == 2
#define DIAL_PLANT_D DimsH1Loco
#elif DIAL_FAMILY == 3
#define DIAL_PLANT_D DimsAllegro
#elif DIAL_FAMILY == 4
#define DIAL_PLANT_D DimsMax
#elif DIAL_FAMILY == 5
#define DIAL_PLANT_D DimsGo2Crate
#elif DIAL_FAMILY == 6
#define DIAL_PLANT_D DimsH1PushCrate
#else
#error "DIAL_FAMILY must be 0 .. 6"
#endif

#define DIAL_PLANT_VAR_ARGS                                                                                                                   \
  const void*, size_t, hipStream_t, float*, double*, const float*, const float*, int, double, double, int, int, float*, int, const float*, int, \
      const int32_t*

template __global__ void plant_var_kernel<DIAL_PLANT_D>(const CModel<DIAL_PLANT_D>*, float*, double*, const float*, const float*, int, double,
                                                         double, int, int, float*, const float*, int, const int32_t*);
template hipError_t plant_var_launch<DIAL_PLANT_D>(DIAL_PLANT_VAR_ARGS);

#if DIAL_FAMILY == 0
extern template hipError_t plant_var_launch<DimsMax>(DIAL_PLANT_VAR_ARGS);
extern template hipError_t plant_var_launch<DimsH1>(DIAL_PLANT_VAR_ARGS);
extern template hipError_t plant_var_launch<DimsH1Loco>(DIAL_PLANT_VAR_ARGS);
extern template hipError_t plant_var_launch<DimsAllegro>(DIAL_PLANT_VAR_ARGS);
extern template hipError_t plant_var_launch<DimsGo2Crate>(DIAL_PLANT_VAR_ARGS);
extern template hipError_t plant_var_launch<DimsH1PushCrate>(DIAL_PLANT_VAR_ARGS);

extern "C" __attribute__((visibility("default"))) const dial_plant_var_ops* dial_plant_var_ops_v1(void) {
  static const dial_plant_var_ops ops = {
      DIAL_PLANT_VAR_ABI_VERSION,
      sizeof(dial_model), sizeof(dial_task),
      {sizeof(CModel<DimsMax>), sizeof(CModel<DimsGo2>), sizeof(CModel<DimsH1>), sizeof(CModel<DimsH1Loco>), sizeof(CModel<DimsAllegro>),
       sizeof(CModel<DimsGo2Crate>), sizeof(CModel<DimsH1PushCrate>)},
      {&plant_var_launch<DimsMax>, &plant_var_launch<DimsGo2>, &plant_var_launch<DimsH1>, &plant_var_launch<DimsH1Loco>,
       &plant_var_launch<DimsAllegro>, &plant_var_launch<DimsGo2Crate>, &plant_var_launch<DimsH1PushCrate>}};
  return &ops;
}
#endif
