// plan_ens_kernel.h -- the rollout kernel of ROBUST PLANNING OVER A MODEL ENSEMBLE (the rollout launch of dial_reverse_once[_rng] and
// dial_reverse_once_batch[_rng] on a context with an ensemble bound by dial_set_plan_ensemble): every candidate action sequence of
// every plan is rolled out under EVERY model hypothesis of its plan, in one launch of R x M x (N + 1) one-wavefront workgroups,
// hypothesis-major.  Workgroup b is rollout (r, g, nl):
//   r  = b / (M (N + 1))              the hypothesis slab,
//   g  = (b mod M (N + 1)) / (N + 1)  the plan,
//   nl = b mod (N + 1)                the plan's sample (nl = N: its mean trajectory).
// It starts from plan g's state, Ybar and noise scale, builds the nodes of plan g's sample nl -- the same eps row, or Philox key
// g N + nl, for every r -- and runs on the constants of models[hyp[g R + r]],
//   (const char*)gm + hyp[g R + r] * stride,   stride = (sizeof(CModel<D>) + 15) / 16 * 16,
// out of V blocks the host built (dial_hip.hip: model_blocks).  Its mean reward goes to row (r M + g)(N + 1) + nl of the raw buffer
// [R][M][N + 1] the binding owns.  Slab r = 0 -- hypothesis 0, the plan's NOMINAL model -- also writes the candidate nodes, the step
// rewards and, when the caller wants bars, the per-step states to rows g (N + 1) + nl of the context's scratch: exactly the dense
// grouped layout, so that the softmax / weighted-sum tail runs unchanged on it.  Slabs r >= 1 write their reward only: the scratch
// holds M plans, not M R.
// The body is dial::rollout_sample -- nothing of the physics is restated -- and neither RolloutIO nor rollout_sample know about
// ensembles: the kernel hands rollout_sample a PRIVATE ONE-PLAN VIEW of the launch (plan_rollouts = 0; state, Ybar, noise_scale, eps
// and plan_params advanced to plan g; n_offset advanced by g N; the output pointers advanced to the rows above, or null) and the
// local index nl.  The index is read once, made a scalar (readfirstlane) and applied before stage_model, as plan_var_kernel.h does;
// w.launder follows the rule of rollout_kernel<D, 1, 3>, the instantiation this kernel is compared with bit for bit
// (tests/test_gpu_plan_ensemble.py).  No queue, no relay, no pair layout, no state trace.
// The kernel lives in code objects of its own:
//   - libdialplanens.so (plan_ens_family.hip, one translation unit per robot family, and plan_ens_aggregate.hip: the aggregation
//     kernel), looked up by libdialhip.so through the table below (dlopen on first bind);
//   - a task plugin built with -DDIAL_PLUGIN_PLAN_ENS=1 (build_plugin(plan_ensemble=True)): the same kernel at ONE model's
//     compile-time dimensions behind an eighth optional table (dial_plugin_plan_ens_v1).  The aggregation kernel of a plugin context
//     is libdialplanens.so's.
//
// THE AGGREGATION (plan_ens_aggregate.hip): one thread per candidate (g, nl) reads its R raw rewards x_0 .. x_{R-1} (stride
// M (N + 1)) and writes the caller's rews[g (N + 1) + nl]:
//   DIAL_ENSEMBLE_MEAN  the fp64 sum in index order r = 0 .. R - 1, divided by (double)R, rounded once to fp32;
//   DIAL_ENSEMBLE_MIN   the smallest x_r;
//   DIAL_ENSEMBLE_CVAR  the k smallest values in ascending order, ties broken by the lower r, summed in fp64 in that order, divided
//                       by (double)k, rounded once to fp32; k = clamp(ceil((double)alpha R), 1, R) is computed on the host.
// The device code is compiled with -fno-honor-nans: A NaN AMONG A CANDIDATE'S REWARDS LEAVES ITS MIN / CVAR AGGREGATE UNSPECIFIED
// (the plan's softmax is NaN in that case anyway).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rollout_kernel.h"

#define DIAL_PLAN_ENS_ABI_VERSION 1
#define DIAL_PLAN_ENS_SYMBOL "dial_plan_ens_ops_v1"
#define DIAL_PLAN_ENS_INSTS 7   // dial_ctx::inst 0 .. 6 (7 is a task plugin: its own table)

// dcm: V blocks of constants `stride` bytes apart; hyp: device int32 [rows >= M][R] with 0 <= hyp[..] < V (the host checked); io: the
// GROUPED launch's arguments (dense plans; n_noise = N); raw: [R][M][N + 1]; lds: the constants + ONE workspace; the grid is
// R x M x (N + 1) workgroups
typedef hipError_t (*dial_plan_ens_launch_fn)(size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                                              const dial::RolloutIO* io, int M, int R, int ws_words, const int32_t* hyp, float* raw);
// raw [R][MB] -> out [MB] (MB = M (N + 1) candidates); mode: DIAL_ENSEMBLE_*; k: the CVaR tail's size, 1 <= k <= R
typedef hipError_t (*dial_plan_ens_aggregate_fn)(hipStream_t st, const float* raw, float* out, int R, int MB, int mode, int k);

struct dial_plan_ens_ops {
  int abi_version;                                  // DIAL_PLAN_ENS_ABI_VERSION
  size_t sizeof_model, sizeof_task;                 // (ABI check)
  size_t sizeof_cfg, sizeof_io;
  size_t cmodel_bytes[DIAL_PLAN_ENS_INSTS];         // sizeof(CModel<D>) per instantiation (ABI check)
  dial_plan_ens_launch_fn launch[DIAL_PLAN_ENS_INSTS];   // (a null entry: that family has no ensemble rollout kernel)
  dial_plan_ens_aggregate_fn aggregate;
};
typedef const dial_plan_ens_ops* (*dial_plan_ens_entry)(void);

extern "C" hipError_t dial_plan_ens_aggregate(hipStream_t st, const float* raw, float* out, int R, int MB, int mode, int k);

template <class D>
__global__ void __launch_bounds__(64, 3)
rollout_ens_kernel(const CModel<D>* __restrict__ gm, const dial_task* __restrict__ tg, const dial_cfg* __restrict__ cfg,
                   dial::RolloutIO io, int M, int R, int ws_words, const int32_t* __restrict__ hyp, float* __restrict__ raw) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Ws s;
  // rollout (r, g, nl) of the hypothesis-major grid: scalars
  const int P = io.n_noise + 1, MB = M * P;
  const int b = (int)blockIdx.x;
  const int r = b / MB, gl = b - r * MB, g = gl / P, nl = gl - g * P;
  constexpr size_t kStride = (sizeof(CModel<D>) + 15) / 16 * 16;
  const int mi = __builtin_amdgcn_readfirstlane(hyp[g * R + r]);
  gm = reinterpret_cast<const CModel<D>*>(reinterpret_cast<const char*>(gm) + (size_t)mi * kStride);
  const CModel<D>* m = stage_model<D, 1>(gm, smem, s, io.Hn1, ws_words, io.con_cap, io.T);
  if constexpr (D::gen)   // this wavefront's overflow area: its slot of the grid
    s.ovf = io.ovf ? io.ovf + (size_t)blockIdx.x * io.ovf_words : nullptr;
  if (r >= R) return;
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
  // the private one-plan view: plan g as a launch of its own, sample nl its rollout nl
  const int nu = dim_nu(m), nq = dim_nq(m), nv = dim_nv(m), nx = (dim_nb(m) - 1) * 3;
  const size_t row0 = (size_t)g * P;   // plan g's first row of the dense grouped scratch
  const bool nominal = r == 0;
  dial::RolloutIO v = io;
  v.plan_rollouts = 0;
  v.state = io.state + (size_t)g * (nq + 2 * nv + DIAL_INFO_N);
  v.Ybar = io.Ybar + (size_t)g * io.Hn1 * nu;
  v.noise_scale = io.noise_scale + g * io.ns;
  v.eps = io.eps ? io.eps + (size_t)g * io.n_noise * io.Hn1 * nu : nullptr;
  v.n_offset = io.n_offset + g * io.n_noise;
  v.rews = raw + ((size_t)r * M + g) * P;
  v.Y0s = nominal && io.Y0s ? io.Y0s + row0 * io.Hn1 * nu : nullptr;
  v.rewss = nominal && io.rewss ? io.rewss + row0 * io.T : nullptr;
  v.qss = nominal && io.qss ? io.qss + row0 * io.T * nq : nullptr;
  v.qdss = nominal && io.qdss ? io.qdss + row0 * io.T * nv : nullptr;
  v.xss = nominal && io.xss ? io.xss + row0 * io.T * nx : nullptr;
  v.plan_params = io.plan_params ? io.plan_params + (size_t)g * DIAL_USER_PARAMS : nullptr;
  dial::rollout_sample<false>(w, m, tg, cfg, s, v, nl, -1, -1, true);
}

template <class D>
hipError_t plan_ens_launch(size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                           const dial::RolloutIO* io, int M, int R, int ws_words, const int32_t* hyp, float* raw) {
  if (lds > 64 * 1024) {   // more than the default dynamic-LDS limit of a launch: opt in
    hipError_t e = hipFuncSetAttribute((const void*)rollout_ens_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rollout_ens_kernel<D>, dim3(R * M * (io->n_noise + 1)), dim3(64), lds, st, (const CModel<D>*)dcm, dtask, dcfg, *io, M, R,
                     ws_words, hyp, raw);
  return hipGetLastError();
}

// ---- task plugins: the eighth optional table (plugin.hip -DDIAL_PLUGIN_PLAN_ENS=1)
#ifndef DIAL_PLUGIN_PLAN_ENS_VERSION
#define DIAL_PLUGIN_PLAN_ENS_VERSION 1
#endif
#define DIAL_PLUGIN_PLAN_ENS_SYMBOL "dial_plugin_plan_ens_v1"
struct dial_plugin_plan_ens {
  int version;                      // DIAL_PLUGIN_PLAN_ENS_VERSION
  int nq, nv, nu;                   // of the instantiation
  size_t cmodel_bytes;              // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check; the blocks' stride follows)
  dial_plan_ens_launch_fn launch;   // lds = the constants + one rollout workspace of the context
};
typedef const dial_plugin_plan_ens* (*dial_plugin_plan_ens_entry)(void);

template <class D>
struct PluginPlanEns {
  static_assert(D::user, "a task plugin's instantiation");
  static const dial_plugin_plan_ens* table() {
    static const dial_plugin_plan_ens tab = {DIAL_PLUGIN_PLAN_ENS_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), &plan_ens_launch<D>};
    return &tab;
  }
};
