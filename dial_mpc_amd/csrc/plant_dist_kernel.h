// plant_dist_kernel.h -- the DISTURBED plant kernel (dial_plant_step with a buffer bound by dial_set_plant_disturbance): plant_kernel.h's
// step loop (one wavefront per plant, constants staged once, state resident in LDS across the K steps, fp64 clock, plant_row /
// plant_ddiv_rn for the row, the same three control modes) with per-plant velocity kicks and actuator errors.  include/dial_mpc.h
// states the semantics and the row layout (dial_set_plant_disturbance).  The loop is RESTATED here, not shared with plant_kernel:
// moving plant_kernel's loop into a __forceinline__ body that both kernels call -- even as a pure wrapper, with or without
// __restrict__ on the body's parameters -- changes the register allocation of plant_kernel in every family (Go2 182 -> 178 VGPRs,
// Go2 crate 136 -> 140, ...), and libdialplant.so's code objects are pinned (tests/golden/plant_kernel_resources.txt).  A change
// to plant_kernel's loop must be made here too; tests/test_gpu_plant_dist.py compares the two bit for bit under identity data.
// plant_var_kernel.h (per-plant model constants) restates the loop a third time, kicks and actuator errors included: a change to the
// loop must be made in all three headers (plant_kernel.h, plant_dist_kernel.h, plant_var_kernel.h).
// The kernel is opt-in and lives in code objects of its own:
//   - libdialplantdist.so (plant_dist_family.hip, one translation unit per robot family), looked up by libdialhip.so through the
//     table below (dlopen on first use) -- libdialplant.so and libdialhip.so gain no kernel;
//   - a task plugin built with -DDIAL_PLUGIN_PLANT_DIST=1 (build_plugin(plant_disturbance=True)): the same kernel at ONE model's
//     compile-time dimensions behind a fifth optional table (dial_plugin_plant_dist_v1).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "plant_kernel.h"

#define DIAL_PLANT_DIST_ABI_VERSION 1
#define DIAL_PLANT_DIST_SYMBOL "dial_plant_dist_ops_v1"

// plant_kernel.h's launch signature plus the bound buffer: dist [M][DIAL_PLANT_DIST_ROW(nu, nv, n_events)], 0 <= n_events <= DIAL_PLANT_MAX_EVENTS
typedef hipError_t (*dial_plant_dist_launch_fn)(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time,
                                                const float* ctrl, int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M,
                                                const float* dist, int n_events);

struct dial_plant_dist_ops {
  int abi_version;                               // DIAL_PLANT_DIST_ABI_VERSION
  size_t sizeof_model, sizeof_task;              // (ABI check)
  size_t cmodel_bytes[DIAL_PLANT_INSTS];         // sizeof(CModel<D>) per instantiation (ABI check)
  dial_plant_dist_launch_fn launch[DIAL_PLANT_INSTS];
};
typedef const dial_plant_dist_ops* (*dial_plant_dist_entry)(void);

template <class D>
__global__ void __launch_bounds__(64)
plant_dist_kernel(const CModel<D>* __restrict__ gm, float* states, double* tclk, const float* __restrict__ plan_time,
                  const float* __restrict__ ctrl, int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace,
                  const float* __restrict__ dist, int n_events) {
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
  // this plant's row; gain / bias of actuator `lane` once per launch, in registers (nu <= 64: one lane per actuator)
  const float* drow = dist + (size_t)b * (size_t)DIAL_PLANT_DIST_ROW(nu, nv, n_events);
  const float* events = drow + 2 * nu;
  float gain = 1.f, bias = 0.f;
  if (w.lane < nu) { gain = drow[w.lane]; bias = drow[nu + w.lane]; }
  dial::init_world(w, s);
  dial::init_square(w, m, s);
  dial::load_state(w, m, s, state);
  double t = tclk[b];   // (wave-uniform: every lane runs the same fp64 clock)
  const double pt = (double)plan_time[b];
  const float cdt = (float)ctrl_dt;
  for (int k = 0; k < K; k++) {
    // kicks, before the control: the PD law, a user law and the trace row see the kicked velocity.  The window test is one scalar
    // decision per event (two scalar loads, the wave-uniform clock); dv is read only when the event fires.
    for (int e = 0; e < n_events; e++) {
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
          s.ctrl[a] = __fmaf_rn(gain, dial_user_control(in, a, m->user_params, s.info + DIAL_INFO_USER), bias);
        });
        done = true;
      }
    }
    if (!done)
      w.items(nu, [&](int a) {
        float c = row[a];
        if (pd) {   // act2tau on the joint target itself, at the plant rate; the actuator error applies to the clipped torque
          const float q_err = c - s.qpos[7 + a];
          c = dm::clip(m->kp[a] * q_err - m->kd[a] * s.qvel[6 + a], m->tau_range[a][0], m->tau_range[a][1]);
        }
        s.ctrl[a] = __fmaf_rn(gain, c, bias);   // (an explicit fma: the contraction flags cannot change it)
      });
    if (trace) {   // the state BEFORE the step (kicked qvel) and the ctrl the actuators receive (disturbed)
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
hipError_t plant_dist_launch(const void* dcm, size_t lds, hipStream_t st, float* states, double* t, const float* plan_time, const float* ctrl,
                             int T, double ctrl_dt, double sim_dt, int K, int flags, float* trace, int M, const float* dist, int n_events) {
  hipLaunchKernelGGL(plant_dist_kernel<D>, dim3(M), dim3(64), lds, st, (const CModel<D>*)dcm, states, t, plan_time, ctrl, T, ctrl_dt, sim_dt, K,
                     flags, trace, dist, n_events);
  return hipGetLastError();
}

// ---- task plugins: the fifth optional table (plugin.hip -DDIAL_PLUGIN_PLANT_DIST=1)
#ifndef DIAL_PLUGIN_PLANT_DIST_VERSION
#define DIAL_PLUGIN_PLANT_DIST_VERSION 1
#endif
#define DIAL_PLUGIN_PLANT_DIST_SYMBOL "dial_plugin_plant_dist_v1"
struct dial_plugin_plant_dist {
  int version;                        // DIAL_PLUGIN_PLANT_DIST_VERSION
  int nq, nv, nu;                     // of the instantiation (the strides of a disturbance row)
  size_t cmodel_bytes;                // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check)
  dial_plant_dist_launch_fn launch;   // lds = the env.step workspace of the context
};
typedef const dial_plugin_plant_dist* (*dial_plugin_plant_dist_entry)(void);

template <class D>
struct PluginPlantDist {
  static_assert(D::user && D::NU <= 64, "a task plugin's instantiation; one lane per actuator");
  static const dial_plugin_plant_dist* table() {
    static const dial_plugin_plant_dist tab = {DIAL_PLUGIN_PLANT_DIST_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), &plant_dist_launch<D>};
    return &tab;
  }
};
