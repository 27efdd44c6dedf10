// plant_plugin.h -- the plant simulator of a task plugin (dial_plant_step on a dial_create_plugin context): plant_kernel.h's kernel at
// ONE model's compile-time dimensions, with the plugin's user control law (user_control.h) as a third control mode.  A plugin built
// with -DDIAL_PLUGIN_PLANT=1 (dial_mpc_amd/plugin.py: build_plugin(plant=True)) instantiates plant_user_kernel and exports a FOURTH
// optional table under a symbol of its own; dial_plugin_ops, dial_plugin_ctrl, dial_plugin_table and their versions stay as they
// are, and a plugin built without the flag carries neither the kernel nor the symbol (dial_plant_step then refuses its contexts).
// libdialhip.so includes this header for the table's layout only: it instantiates no kernel of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "plant_kernel.h"

#ifndef DIAL_PLUGIN_PLANT_VERSION   // (overridable on a plugin's command line: the tests build one that reports another version)
#define DIAL_PLUGIN_PLANT_VERSION 1
#endif
#define DIAL_PLUGIN_PLANT_SYMBOL "dial_plugin_plant_v1"
struct dial_plugin_plant {
  int version;                     // DIAL_PLUGIN_PLANT_VERSION
  int nq, nv, nu;                  // of the instantiation (the row strides of the launch below)
  size_t cmodel_bytes;             // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check)
  size_t sizeof_control_in;        // sizeof(DialControlIn)
  int has_law;                     // the plugin carries a user control law: DIAL_PLANT_LAW is available
  dial_plant_launch_fn launch;     // plant_kernel.h's launch signature; lds = the env.step workspace of the context
};
typedef const dial_plugin_plant* (*dial_plugin_plant_entry)(void);

// The control step the plant's clock is in, as DIAL_PLANT_LAW hands it to the law (DialControlIn::step): trunc(t / ctrl_dt) with the
// correctly rounded fp64 quotient (plant_ddiv_rn: the truncation must not depend on the translation unit's flags), 0 when the
// quotient is not >= 0 (negative clocks, NaN) and capped at 2^24, the last counter a float holds exactly.  Written so that no
// out-of-range double reaches the int conversion.  deploy/plant.py: law_step restates it on the host.
__device__ __forceinline__ int plant_law_step(double t, double ctrl_dt) {
  const double q = plant_ddiv_rn(t, ctrl_dt);
  if (!(q >= 0.0)) return 0;
  if (q >= 16777216.0) return 1 << 24;
  return (int)q;
}

// plant_kernel's contract (one wavefront per plant, K physics steps per launch, constants staged once, the state resident in LDS,
// the fp64 clock, the row rule, the trace row of the state BEFORE the step, the info words untouched) with three control modes:
// DIAL_PLANT_CTRL and DIAL_PLANT_PD exactly as plant_kernel, and -- a plugin with a law only -- DIAL_PLANT_LAW: the row is a
// normalised action, and lane a evaluates dial_user_control at EVERY sim step from the plant's current qpos / qvel.  The law's value
// is the step's ctrl (and the trace's); the actuators apply it as they apply any ctrl.  What the law sees beyond user_control.h's
// list: step = plant_law_step(t, ctrl_dt), dt = (float)ctrl_dt, act = the picked row (global memory), info_user = the state's slots
// as they are, params = the shared parameters, the table row of that step straight from global memory (no ring: the plant has no
// reward that would read it after the physics).  Per step the control phase issues two kinds of global loads, the row and the table
// row; everything else the law reads is LDS (the staged constants, the state).
template <class D>
__global__ void __launch_bounds__(64)
plant_user_kernel(const CModel<D>* __restrict__ gm, float* states, double* tclk, const float* __restrict__ plan_time,
                  const float* __restrict__ ctrl, int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace) {
  static_assert(D::user && D::NU <= 64, "a task plugin's instantiation; one lane per actuator");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Ws s;
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
  dial::init_world(w, s);
  dial::init_square(w, m, s);
  dial::load_state(w, m, s, state);
  double t = tclk[b];   // (wave-uniform: every lane runs the same fp64 clock)
  const double pt = (double)plan_time[b];
  const float cdt = (float)ctrl_dt;
  for (int k = 0; k < K; k++) {
    const float* row = rows + (size_t)(hold ? 0 : plant_row(t, pt, ctrl_dt, T)) * nu;
    bool done = false;
    if constexpr (D::user_ctrl) {
      if (law) {
        // once per step and a scalar: the table's row index (an integer modulo under DIAL_TABLE_WRAP) is computed on it
        const int step = __builtin_amdgcn_readfirstlane(plant_law_step(t, ctrl_dt));
        const float* trow = nullptr;
        int tindex = 0;
        if (m->table_rows > 0) {
          tindex = dial::table_row_index(step, m->table_row0, m->table_rows, m->table_mode);
          trow = m->table + (size_t)tindex * m->table_cols;
        }
        w.items(nu, [&](int a) {
          DialControlIn in = dial::control_in(m, (float)step, s.qpos, s.qvel, row, trow, tindex);
          in.dt = cdt;   // (the constants' dt is the plant context's: sim_dt)
          s.ctrl[a] = dial_user_control(in, a, m->user_params, s.info + DIAL_INFO_USER);
        });
        done = true;
      }
    }
    if (!done)
      w.items(nu, [&](int a) {
        float c = row[a];
        if (pd) {   // act2tau (base_env.py:53-66) on the joint target itself, at the plant rate
          const float q_err = c - s.qpos[7 + a];
          c = dm::clip(m->kp[a] * q_err - m->kd[a] * s.qvel[6 + a], m->tau_range[a][0], m->tau_range[a][1]);
        }
        s.ctrl[a] = c;
      });
    if (trace) {   // dial_sim.py's record row: the state BEFORE the step and the ctrl the step applies
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
struct PluginPlant {
  static hipError_t launch(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time, const float* ctrl,
                           int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M) {
    hipLaunchKernelGGL(plant_user_kernel<D>, dim3(M), dim3(64), lds, st, (const CModel<D>*)dcm, states, t, plan_time, ctrl, T, ctrl_dt, sim_dt,
                       K, flags, trace);
    return hipGetLastError();
  }
  static const dial_plugin_plant* table() {
    static const dial_plugin_plant tab = {DIAL_PLUGIN_PLANT_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), sizeof(DialControlIn),
                                          D::user_ctrl ? 1 : 0, &launch};
    return &tab;
  }
};
