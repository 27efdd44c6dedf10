// plant_var_kernel.h -- the plant kernel with PER-PLANT MODEL CONSTANTS (dial_plant_step with models bound by dial_set_plant_models):
// plant_kernel.h's step loop (one wavefront per plant, constants staged once, state resident in LDS across the K steps, fp64 clock,
// plant_row / plant_ddiv_rn for the row, the same three control modes) in which workgroup b stages ITS OWN block of constants,
//   (const char*)gm + model_of[b] * stride,   stride = (sizeof(CModel<D>) + 15) / 16 * 16,
// out of V blocks the host built from V models (masses, inertias, friction, damping, ... : mjcf.vary_model), instead of the one shared
// block.  The index is read once, made a scalar (readfirstlane) and applied before stage_model; the capacity-dimension
// instantiation, which reads its constants from global memory, reads through the same offset pointer.  A disturbance buffer
// (dial_set_plant_disturbance) may be bound next to the models: `dist` non-null runs plant_dist_kernel.h's kicks and fma(gain, c, bias),
// dist == nullptr runs plant_kernel.h's plain `s.ctrl[a] = c` -- one wave-uniform test per launch, never gain 1 / bias 0 rows
// (fma(1, -0.f, 0) is +0).
// The loop is RESTATED here, as in plant_dist_kernel.h and for its reason: sharing one __forceinline__ body moves the pinned register
// allocation of plant_kernel in every family.  A change to the step loop must be made in ALL THREE headers (plant_kernel.h,
// plant_dist_kernel.h, this one); tests/test_gpu_plant_models.py compares this kernel with the other two bit for bit.
// The kernel is opt-in and lives in code objects of its own:
//   - libdialplantvar.so (plant_var_family.hip, one translation unit per robot family), looked up by libdialhip.so through the table
//     below (dlopen on first use) -- libdialplant.so, libdialplantdist.so and libdialhip.so gain no kernel;
//   - a task plugin built with -DDIAL_PLUGIN_PLANT_VAR=1 (build_plugin(plant_models=True)): the same kernel at ONE model's
//     compile-time dimensions behind a sixth optional table (dial_plugin_plant_var_v1).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "plant_kernel.h"

#define DIAL_PLANT_VAR_ABI_VERSION 1
#define DIAL_PLANT_VAR_SYMBOL "dial_plant_var_ops_v1"

// plant_dist_kernel.h's launch signature (dist may be null: no disturbance) plus the index: dcm V blocks of constants `stride`
// bytes apart, model_of device int32[M] with 0 <= model_of[b] < V (the host checked it before the upload)
typedef hipError_t (*dial_plant_var_launch_fn)(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time,
                                               const float* ctrl, int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M,
                                               const float* dist, int n_events, const int32_t* model_of);

struct dial_plant_var_ops {
  int abi_version;                               // DIAL_PLANT_VAR_ABI_VERSION
  size_t sizeof_model, sizeof_task;              // (ABI check)
  size_t cmodel_bytes[DIAL_PLANT_INSTS];         // sizeof(CModel<D>) per instantiation (ABI check)
  dial_plant_var_launch_fn launch[DIAL_PLANT_INSTS];   // (a null entry: that family has no per-plant-model kernel)
};
typedef const dial_plant_var_ops* (*dial_plant_var_entry)(void);

template <class D>
__global__ void __launch_bounds__(64)
plant_var_kernel(const CModel<D>* __restrict__ gm, float* states, double* tclk, const float* __restrict__ plan_time,
                 const float* __restrict__ ctrl, int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace,
                 const float* __restrict__ dist, int n_events, const int32_t* __restrict__ model_of) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Ws s;
  // this plant's block of constants: one scalar index per workgroup, applied before the staging copy (and, for the instantiation
  // that keeps its constants in global memory, to the pointer every later read goes through)
  constexpr size_t kStride = (sizeof(CModel<D>) + 15) / 16 * 16;
  const int mi = __builtin_amdgcn_readfirstlane(model_of[blockIdx.x]);
  gm = reinterpret_cast<const CModel<D>*>(reinterpret_cast<const char*>(gm) + (size_t)mi * kStride);
  const CModel<D>* m = stage_model<D>(gm, smem, s, 0, 0);
  Wave w;
  w.lane = threadIdx.x;
  w.lane_r = w.lane;
  w.launder = D::gen;
  const int b = (int)blockIdx.x, nq = dim_nq(m), nv = dim_nv(m), nu = dim_nu(m);
  const int W = 1 + nq + nv + nu;
  float* state = states + (size_t)b * (nq + 2 * nv + DIAL_INFO_N);
  const float* rows = ctrl + (size_t)b * T * nu;
  const bool pd = (flags & DIAL_PLANT_PD) != 0, hold = (flags & DIAL_PLANT_HOLD_FIRST) != 0;
  const bool law = D::user_ctrl && (flags & DIAL_PLANT_LAW) != 0;
  // a bound disturbance: this plant's row; gain / bias of actuator `lane` once per launch, in registers.  disturbed is a kernel
  // argument compared with null -- a scalar, the same for every wavefront of the launch; without one the event count is zero.
  const bool disturbed = dist != nullptr;
  const int ne = disturbed ? n_events : 0;
  const float* drow = disturbed ? dist + (size_t)b * (size_t)DIAL_PLANT_DIST_ROW(nu, nv, n_events) : nullptr;
  const float* events = disturbed ? drow + 2 * nu : nullptr;
  float gain = 1.f, bias = 0.f;
  if (disturbed && w.lane < nu) { gain = drow[w.lane]; bias = drow[nu + w.lane]; }
  dial::init_world(w, s);
  dial::init_square(w, m, s);
  dial::load_state(w, m, s, state);
  double t = tclk[b];   // (wave-uniform: every lane runs the same fp64 clock)
  const double pt = (double)plan_time[b];
  const float cdt = (float)ctrl_dt;
  for (int k = 0; k < K; k++) {
    // kicks (plant_dist_kernel.h), before the control; no event loop without a bound disturbance (ne == 0)
    for (int e = 0; e < ne; e++) {
      const float* ev = events + e * (2 + nv);
      const bool fires = t >= (double)ev[0] && t < (double)ev[1];   // (t1 <= t0, NaN: never)
      if (__builtin_amdgcn_readfirstlane((int)fires)) w.items(nv, [&](int i) { s.qvel[i] = s.qvel[i] + ev[2 + i]; });
    }
    const float* row = rows + (size_t)(hold ? 0 : plant_row(t, pt, ctrl_dt, T)) * nu;
    bool done = false;
    if constexpr (D::user_ctrl) {
      if (law) {
        const int step = __builtin_amdgcn_readfirstlane(plant_law_step(t, ctrl_dt));
        const float* trow = nullptr;
        int tindex = 0;
        if (m->table_rows > 0) {
          tindex = dial::table_row_index(step, m->table_row0, m->table_rows, m->table_mode);
          trow = m->table + (size_t)tindex * m->table_cols;
        }
        w.items(nu, [&](int a) {
          DialControlIn in = dial::control_in(m, (float)step, s.qpos, s.qvel, row, trow, tindex);
          in.dt = cdt;
          const float c = dial_user_control(in, a, m->user_params, s.info + DIAL_INFO_USER);
          s.ctrl[a] = disturbed ? __fmaf_rn(gain, c, bias) : c;
        });
        done = true;
      }
    }
    if (!done)
      w.items(nu, [&](int a) {
        float c = row[a];
        if (pd) {   // act2tau on the joint target itself, at the plant rate; an actuator error applies to the clipped torque
          const float q_err = c - s.qpos[7 + a];
          c = dm::clip(m->kp[a] * q_err - m->kd[a] * s.qvel[6 + a], m->tau_range[a][0], m->tau_range[a][1]);
        }
        s.ctrl[a] = disturbed ? __fmaf_rn(gain, c, bias) : c;   // (an explicit fma: the contraction flags cannot change it)
      });
    if (trace) {   // the state BEFORE the step (kicked qvel) and the ctrl the actuators receive
      float* tr = trace + ((size_t)b * K + k) * W;
      const float tf = (float)t;
      w.items(W, [&](int i) {
        tr[i] = i == 0 ? tf : (i <= nq ? s.qpos[i - 1] : (i <= nq + nv ? s.qvel[i - 1 - nq] : s.ctrl[i - 1 - nq - nv]));
      });
    }
#ifndef DIAL_EMU
    if (w.launder) { asm volatile("" : "+v"(w.lane)); w.lane_r = w.lane; }   // (as env_step's physics-frame loop)
#endif
    dial::forward(w, m, s);
    dial::euler(w, m, s);
    t += sim_dt;
  }
  dial::store_state(w, m, s, state);
  if (threadIdx.x == 0) tclk[b] = t;
}

template <class D>
hipError_t plant_var_launch(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time, const float* ctrl,
                            int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M, const float* dist, int n_events,
                            const int32_t* model_of) {
  hipLaunchKernelGGL(plant_var_kernel<D>, dim3(M), dim3(64), lds, st, (const CModel<D>*)dcm, states, t, plan_time, ctrl, T, ctrl_dt, sim_dt, K,
                     flags, trace, dist, n_events, model_of);
  return hipGetLastError();
}

// ---- task plugins: the sixth optional table (plugin.hip -DDIAL_PLUGIN_PLANT_VAR=1)
#ifndef DIAL_PLUGIN_PLANT_VAR_VERSION
#define DIAL_PLUGIN_PLANT_VAR_VERSION 1
#endif
#define DIAL_PLUGIN_PLANT_VAR_SYMBOL "dial_plugin_plant_var_v1"
struct dial_plugin_plant_var {
  int version;                       // DIAL_PLUGIN_PLANT_VAR_VERSION
  int nq, nv, nu;                    // of the instantiation
  size_t cmodel_bytes;               // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check; the blocks' stride follows)
  dial_plant_var_launch_fn launch;   // lds = the env.step workspace of the context
};
typedef const dial_plugin_plant_var* (*dial_plugin_plant_var_entry)(void);

template <class D>
struct PluginPlantVar {
  static_assert(D::user && D::NU <= 64, "a task plugin's instantiation; one lane per actuator");
  static const dial_plugin_plant_var* table() {
    static const dial_plugin_plant_var tab = {DIAL_PLUGIN_PLANT_VAR_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), &plant_var_launch<D>};
    return &tab;
  }
};
