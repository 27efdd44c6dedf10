// plant_kernel.h -- the plant simulator's kernel (dial_plant_step, deploy/dial_sim.py): M plants, one wavefront (one 64-lane
// workgroup) each, K physics steps per launch.  Each step applies one row of the plan the planner published and runs the env.step's
// own physics -- forward + euler through the generic control path (no control tables, no reward, no act2joint, no gait clock;
// the info words are left untouched).  The constants are staged once, the state (qpos, qvel, qacc_warmstart) stays resident in
// LDS across the K steps; the clock is fp64, the row follows dial_sim.py's row rule (plant_row), and the trace row holds the state
// BEFORE the step with the ctrl the step applies.  ONE kernel serves the built-in robot families and the task plugins:
//   - libdialplant.so (plant_family.hip, one translation unit per robot family) -- never libdialhip.so, whose code objects stay as
//     shipped; libdialhip.so reaches these launches through the table below (dlopen);
//   - a task plugin built with a plant (plugin.hip -DDIAL_PLUGIN_PLANT=1): the same kernel at ONE model's compile-time dimensions,
//     reached through plant_plugin.h's table.
// Control modes: DIAL_PLANT_CTRL (the row is the ctrl) and DIAL_PLANT_PD (the row is a joint target, act2tau at the plant rate) for
// every instantiation, and -- a plugin with a user control law only (Dims::user_ctrl; for every built-in Dims the branch vanishes) --
// DIAL_PLANT_LAW: the row is a normalised action, and lane a evaluates dial_user_control (user_control.h) at EVERY sim step from the
// plant's current qpos / qvel.  The law's value is the step's ctrl (and the trace's); the actuators apply it as they apply any ctrl.
// What the law sees beyond user_control.h's list: step = plant_law_step(t, ctrl_dt), dt = (float)ctrl_dt, act = the picked row
// (global memory), info_user = the state's slots as they are, params = the shared parameters, the table row of that step straight
// from global memory (no ring: the plant has no reward that would read it after the physics).  Per step the law's control phase
// issues two kinds of global loads, the row and the table row; everything else the law reads is LDS (the staged constants, the state).
// The step loop below is RESTATED in plant_dist_kernel.h (velocity kicks, actuator errors) and in plant_var_kernel.h (per-plant model
// constants), because sharing one inlined body moves this kernel's pinned register allocation: a change to the loop must be made in
// all three headers (plant_kernel.h, plant_dist_kernel.h, plant_var_kernel.h); the GPU tests compare them bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "rollout_kernel.h"

#define DIAL_PLANT_ABI_VERSION 1
#define DIAL_PLANT_SYMBOL "dial_plant_ops_v1"
#define DIAL_PLANT_INSTS 7   // dial_ctx::inst 0 .. 6 (generic, Go2, H1, H1 loco, Allegro, Go2 crate, H1 push crate)

// fp64 x / y correctly rounded on the device whatever the translation unit's flags say: -freciprocal-math (the product build) lowers
// `x / y` to x * rcp(y) refined without the scale / fix-up steps, which can land one ulp off -- and the row rule below truncates the
// quotient, so that one ulp can change the row.  This is the instruction sequence the compiler emits for an IEEE division.
__device__ __forceinline__ double plant_ddiv_rn(double x, double y) {
  bool flag;
  const double den = __builtin_amdgcn_div_scale(x, y, false, &flag);
  const double num = __builtin_amdgcn_div_scale(x, y, true, &flag);
  const double r0 = __builtin_amdgcn_rcp(den);
  const double r1 = __builtin_fma(r0, __builtin_fma(-den, r0, 1.0), r0);
  const double r2 = __builtin_fma(r1, __builtin_fma(-den, r1, 1.0), r1);
  const double q0 = num * r2;
  return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(-den, q0, num), r2, q0, flag), y, x);
}

// dial_sim.py's row rule in fp64: delta = t - plan_time, int(delta / ctrl_dt) (truncation toward zero), and the last row when that
// is >= n_acts or < 0.  Written so that no out-of-range double reaches the int conversion.
__host__ __device__ inline int plant_row(double t, double plan_time, double ctrl_dt, int n_acts) {
#ifdef __HIP_DEVICE_COMPILE__
  const double q = plant_ddiv_rn(t - plan_time, ctrl_dt);
#else
  const double q = (t - plan_time) / ctrl_dt;
#endif
  if (!(q < (double)n_acts) || q <= -1.0) return n_acts - 1;   // (NaN included)
  return (int)q;
}

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

typedef hipError_t (*dial_plant_launch_fn)(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time,
                                           const float* ctrl, int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M);

struct dial_plant_ops {
  int abi_version;                               // DIAL_PLANT_ABI_VERSION
  size_t sizeof_model, sizeof_task;              // (ABI check)
  size_t cmodel_bytes[DIAL_PLANT_INSTS];         // sizeof(CModel<D>) per instantiation (ABI check)
  dial_plant_launch_fn launch[DIAL_PLANT_INSTS];
};
typedef const dial_plant_ops* (*dial_plant_entry)(void);

template <class D>
__global__ void __launch_bounds__(64)
plant_kernel(const CModel<D>* __restrict__ gm, float* states, double* tclk, const float* __restrict__ plan_time, const float* __restrict__ ctrl,
             int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace) {
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
hipError_t plant_launch(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time, const float* ctrl, int T,
                        double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M) {
  hipLaunchKernelGGL(plant_kernel<D>, dim3(M), dim3(64), lds, st, (const CModel<D>*)dcm, states, t, plan_time, ctrl, T, ctrl_dt, sim_dt, K,
                     flags, trace);
  return hipGetLastError();
}
