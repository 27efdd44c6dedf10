// plan_var_kernel.h -- the rollout kernel with PER-PLAN or PER-SAMPLE MODEL CONSTANTS (the rollout launches of a context with planner
// models bound by dial_set_plan_models): one wavefront per workgroup, a plain grid of B workgroups, workgroup b runs batch rollout b
// through dial::rollout_sample -- the per-sample body of every rollout kernel (rollout_driver.h), nothing of the physics is restated
// here -- on ITS OWN block of constants,
//   (const char*)gm + model_of[row] * stride,   stride = (sizeof(CModel<D>) + 15) / 16 * 16,
// out of V blocks the host built from V models (mjcf.vary_model makes them; dial_hip.hip: plant_model_block), instead of the one
// shared block.  row is the rollout's plan g (per_sample == 0: plan g of a grouped launch plans with models[model_of[g]], one-plan
// launches read row 0) or its index nl in its plan (per_sample != 0: sample nl of EVERY plan rolls out under models[model_of[nl]],
// row Nsample is the mean trajectory's -- domain-randomised sampling); g and nl are computed as rollout_sample computes them.  The
// index is read once, made a scalar (readfirstlane) and applied before stage_model, exactly as plant_var_kernel.h does; the
// capacity-dimension instantiation, which reads its constants from global memory, reads through the same offset pointer.
// No queue, no relay, no pair layout, no split launch, no interleaved mean trajectory, no state trace: the launch-level mechanisms of
// rollout_kernel.h all assume ONE block of constants per launch (or per workgroup of several wavefronts).  w.launder follows the rule
// of rollout_kernel<D, 1, 3>, the instantiation this kernel is compared with bit for bit (tests/test_gpu_plan_models.py).
// Per-plan task parameters of a task plugin (io.plan_params) still overwrite the staged block's user_params in rollout_sample: the
// block in LDS is this wavefront's own copy.
// model_of and per_sample are arguments of this kernel alone: RolloutIO, dial_cfg, dial_task and the arguments of every other kernel
// stay as they are.  The kernel is opt-in and lives in code objects of its own:
//   - libdialplanvar.so (plan_var_family.hip, one translation unit per robot family), looked up by libdialhip.so through the table
//     below (dlopen on first use) -- libdialhip.so and the plant libraries gain no kernel;
//   - a task plugin built with -DDIAL_PLUGIN_PLAN_VAR=1 (build_plugin(plan_models=True)): the same kernel at ONE model's
//     compile-time dimensions behind a seventh optional table (dial_plugin_plan_var_v1).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rollout_kernel.h"

#define DIAL_PLAN_VAR_ABI_VERSION 1
#define DIAL_PLAN_VAR_SYMBOL "dial_plan_var_ops_v1"
#define DIAL_PLAN_VAR_INSTS 7   // dial_ctx::inst 0 .. 6 (7 is a task plugin: its own table)

// dcm: V blocks of constants `stride` bytes apart; model_of: device int32 rows with 0 <= model_of[r] < V (the host checked both the
// values and that the launch reads no row past the end); lds: the constants + ONE workspace; the grid is B workgroups
typedef hipError_t (*dial_plan_var_launch_fn)(size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                                              const dial::RolloutIO* io, int B, int ws_words, const int32_t* model_of, int per_sample);

struct dial_plan_var_ops {
  int abi_version;                                  // DIAL_PLAN_VAR_ABI_VERSION
  size_t sizeof_model, sizeof_task;                 // (ABI check)
  size_t sizeof_cfg, sizeof_io;
  size_t cmodel_bytes[DIAL_PLAN_VAR_INSTS];         // sizeof(CModel<D>) per instantiation (ABI check)
  dial_plan_var_launch_fn launch[DIAL_PLAN_VAR_INSTS];   // (a null entry: that family has no per-model rollout kernel)
};
typedef const dial_plan_var_ops* (*dial_plan_var_entry)(void);

template <class D>
__global__ void __launch_bounds__(64, 3)
rollout_var_kernel(const CModel<D>* __restrict__ gm, const dial_task* __restrict__ tg, const dial_cfg* __restrict__ cfg,
                   dial::RolloutIO io, int B, int ws_words, const int32_t* __restrict__ model_of, int per_sample) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Ws s;
  const int n = (int)blockIdx.x;
  // this rollout's block of constants: its plan g and local index nl as rollout_sample computes them, one scalar index per workgroup,
  // applied before the staging copy (and, for the instantiation that keeps its constants in global memory, to the pointer every
  // later read goes through)
  const int g = io.plan_rollouts ? n / io.plan_rollouts : 0, nl = n - g * io.plan_rollouts;
  constexpr size_t kStride = (sizeof(CModel<D>) + 15) / 16 * 16;
  const int mi = __builtin_amdgcn_readfirstlane(model_of[per_sample ? nl : g]);
  gm = reinterpret_cast<const CModel<D>*>(reinterpret_cast<const char*>(gm) + (size_t)mi * kStride);
  const CModel<D>* m = stage_model<D, 1>(gm, smem, s, io.Hn1, ws_words, io.con_cap, io.T);
  if constexpr (D::gen)   // this wavefront's overflow area: its slot of the grid
    s.ovf = io.ovf ? io.ovf + (size_t)blockIdx.x * io.ovf_words : nullptr;
  if (n >= B) return;
  Wave w;
  w.lane = threadIdx.x & 63;
  w.lane_r = w.lane;
  // (rollout_kernel<D, 1, 3>'s rule: OCC = 3, no queue)
  w.launder = D::gen || DIAL_LAUNDER_STATIC || (DIAL_LAUNDER_H1 && std::is_same<typename D::Topo, TopoH1>::value);
#ifdef DIAL_PROFILE
  w.acc = reinterpret_cast<unsigned long long*>(smem + (ws_words + (D::is_static ? (int)((sizeof(CModel<D>) + 15) / 16) * 4 : 0) + 2) / 2 * 2);
  if (w.lane < 32) w.acc[w.lane] = 0;
  __syncthreads();
#endif
  dial::rollout_sample<false>(w, m, tg, cfg, s, io, n, -1, -1, true);
}

template <class D>
hipError_t plan_var_launch(size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                           const dial::RolloutIO* io, int B, int ws_words, const int32_t* model_of, int per_sample) {
  if (lds > 64 * 1024) {   // more than the default dynamic-LDS limit of a launch: opt in
    hipError_t e = hipFuncSetAttribute((const void*)rollout_var_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rollout_var_kernel<D>, dim3(B), dim3(64), lds, st, (const CModel<D>*)dcm, dtask, dcfg, *io, B, ws_words, model_of,
                     per_sample);
  return hipGetLastError();
}

// ---- task plugins: the seventh optional table (plugin.hip -DDIAL_PLUGIN_PLAN_VAR=1)
#ifndef DIAL_PLUGIN_PLAN_VAR_VERSION
#define DIAL_PLUGIN_PLAN_VAR_VERSION 1
#endif
#define DIAL_PLUGIN_PLAN_VAR_SYMBOL "dial_plugin_plan_var_v1"
struct dial_plugin_plan_var {
  int version;                      // DIAL_PLUGIN_PLAN_VAR_VERSION
  int nq, nv, nu;                   // of the instantiation
  size_t cmodel_bytes;              // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check; the blocks' stride follows)
  dial_plan_var_launch_fn launch;   // lds = the constants + one rollout workspace of the context
};
typedef const dial_plugin_plan_var* (*dial_plugin_plan_var_entry)(void);

template <class D>
struct PluginPlanVar {
  static_assert(D::user, "a task plugin's instantiation");
  static const dial_plugin_plan_var* table() {
    static const dial_plugin_plan_var tab = {DIAL_PLUGIN_PLAN_VAR_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), &plan_var_launch<D>};
    return &tab;
  }
};
