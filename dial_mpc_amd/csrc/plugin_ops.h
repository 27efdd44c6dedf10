// plugin_ops.h -- the host side of ONE kernel instantiation as a table of functions: what a task plugin (plugin.hip, built by
// dial_mpc_amd/plugin.py for one model and one user reward) exports and libdialhip.so calls for a context of dial_create_plugin.
// The table carries the per-instantiation work of dial_create and of the launches -- sizing and filling the constants, the
// dynamic-LDS opt-in, the occupancy query, the rollout / env.step / env.reset launches -- so that the library keeps everything
// else (the queue / relay decisions of launch_rollout, K4 / K5, the sharded and grouped entry points) for plugin contexts too.
// The plugin is built from the same csrc sources as the library (its cache key hashes them), and the table records the sizes of
// the structs that cross the boundary; dial_create_plugin refuses a plugin whose ABI version or sizes differ.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <new>

#include "rollout_kernel.h"

// 2: env_step takes the per-state task parameters, RolloutIO gained plan_params (dial_set_plan_params)
#define DIAL_PLUGIN_ABI_VERSION 2
#define DIAL_PLUGIN_SYMBOL "dial_plugin_ops_v1"

// what dial_create's `upload` computes for an instantiation: LDS layout and the generic feature set's contact cap
struct dial_plugin_layout {
  int cm_bytes;      // constants staged in LDS (16-byte multiple)
  int ws_words;      // one rollout's workspace (wavefront)
  int ws0_words;     // env.step / env.reset workspace (no node array)
  int con_cap;       // touching-contact cap of the capped workspace (0: no cap)
  int ovf_words;     // words of one overflow area (con_cap > 0)
};

struct dial_plugin_ops {
  int abi_version;                 // DIAL_PLUGIN_ABI_VERSION
  int dims[10];                    // nq nv nu nbody njnt ngeom nsite ncon nlim nfri of the instantiation
  int wpb;                         // wavefronts per workgroup of its rollout kernel
  size_t cmodel_bytes;             // sizeof(CModel<D>)
  size_t sizeof_model, sizeof_task, sizeof_cfg, sizeof_derived, sizeof_io;   // (ABI check)
  // does the model fit the instantiation exactly (dimensions, impedance table, pyramidal cones)?  0 = yes, else a reason
  const char* (*check)(const dial_model* m, const dial_derived* dv);
  int (*layout)(const dial_model* m, const dial_cfg* cfg, int opt_con_cap, dial_plugin_layout* out);
  // the constants (host copy, cmodel_bytes) with the user parameters params[0 .. n) (the rest zero)
  void (*fill)(void* host_cm, const dial_model* m, const dial_task* t, const dial_derived* dv, const float* params, int n);
  void (*set_params)(void* host_cm, const float* params, int n);
  hipError_t (*set_lds)(size_t lds_rollout);   // dynamic-LDS opt-in of the rollout kernels (> 64 KiB)
  hipError_t (*occupancy)(int* blocks_per_cu, size_t lds_rollout);
  // variant 0 plain grid, 1 rollout queue (next != nullptr), 2 state trace
  hipError_t (*rollout)(int variant, int blocks, size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                        const dial::RolloutIO* io, int B, int ws_words, int* next);
  // plan_params: [n, DIAL_USER_PARAMS] per-state task parameters (state b reads row b), or nullptr (the shared ones)
  hipError_t (*env_step)(int n, size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, float* state, const float* action,
                         float* xpos_out, float* xquat_out, float* ctrl_out, const float* plan_params);
  hipError_t (*env_reset)(int n, size_t lds, hipStream_t st, const void* dcm, const float* qpos, const float* qvel, float* state,
                          float* xpos_out, float* xquat_out);
};

typedef const dial_plugin_ops* (*dial_plugin_entry)(void);

// A plugin built with a user control law (user_control.h) exports a SECOND table under a second symbol; dial_plugin_ops and its ABI
// version stay as they are, and a plugin without a law does not export the symbol (dial_create_plugin: the context has no law).
#define DIAL_PLUGIN_CTRL_VERSION 1
#define DIAL_PLUGIN_CTRL_SYMBOL "dial_plugin_ctrl_v1"
struct dial_plugin_ctrl {
  int version;                     // DIAL_PLUGIN_CTRL_VERSION
  int nq, nv, nu;                  // of the instantiation (the row strides of the launch below)
  size_t cmodel_bytes;             // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check)
  size_t sizeof_control_in;        // sizeof(DialControlIn)
  // the law for n rows: states [n, nq + 2 nv + DIAL_INFO_N] packed, actions [n, nu] -> ctrl_out [n, nu]; row g reads row g of
  // plan_params ([n, DIAL_USER_PARAMS]) or, nullptr, the shared parameters of the constants
  hipError_t (*user_control)(int n, hipStream_t st, const void* dcm, const float* states, const float* actions, float* ctrl_out,
                             const float* plan_params);
};
typedef const dial_plugin_ctrl* (*dial_plugin_ctrl_entry)(void);

// The user control law outside a step: one 64-lane workgroup per row of (packed state, action), lane a evaluates actuator a exactly as
// env_step's control phase does -- same inputs (the row's qpos / qvel / step counter / info_user slots), constants read from global
// memory (nothing is staged: a row is one call of the law per lane).
template <class D>
__global__ void __launch_bounds__(64)
user_control_kernel(const CModel<D>* __restrict__ gm, const float* __restrict__ states, const float* __restrict__ actions,
                    float* __restrict__ ctrl_out, const float* __restrict__ plan_params) {
  static_assert(D::user_ctrl && D::NU <= 64, "a task plugin's instantiation with a control law; one lane per actuator");
  const int g = (int)blockIdx.x, a = (int)threadIdx.x;
  if (a >= D::NU) return;
  const float* const st = states + (size_t)g * (D::NQ + 2 * D::NV + DIAL_INFO_N);
  const float* const info = st + D::NQ + 2 * D::NV;
  const float* const params = plan_params ? plan_params + (size_t)g * DIAL_USER_PARAMS : gm->user_params;
  // the reference table: nothing is staged here either -- the row of this state's counter straight from global memory
  const float* trow = nullptr;
  int tindex = 0;
  if (gm->table_rows > 0) {
    tindex = dial::table_row_index((int)info[DIAL_INFO_STEP], gm->table_row0, gm->table_rows, gm->table_mode);
    trow = gm->table + (size_t)tindex * gm->table_cols;
  }
  const DialControlIn in = dial::control_in(gm, info[DIAL_INFO_STEP], st, st + D::NQ, actions + (size_t)g * D::NU, trow, tindex);
  ctrl_out[(size_t)g * D::NU + a] = dial_user_control(in, a, params, info + DIAL_INFO_USER);
}

template <class D>
struct PluginCtrl {
  static hipError_t user_control(int n, hipStream_t st, const void* dcm, const float* states, const float* actions, float* ctrl_out,
                                 const float* plan_params) {
    hipLaunchKernelGGL(user_control_kernel<D>, dim3(n), dim3(64), 0, st, (const CModel<D>*)dcm, states, actions, ctrl_out, plan_params);
    return hipGetLastError();
  }
  static const dial_plugin_ctrl* table() {
    static const dial_plugin_ctrl ctl = {DIAL_PLUGIN_CTRL_VERSION, D::NQ, D::NV, D::NU, sizeof(CModel<D>), sizeof(DialControlIn), &user_control};
    return &ctl;
  }
};

// The reference table (dial_set_user_table): a THIRD optional table under a third symbol, exported by every plugin built from
// sources that know the table, with or without a law; dial_plugin_ops, dial_plugin_ctrl and their versions stay as they are.  The
// binding lives in the plugin's constants (cmodel.h: CModelUser), so the kernels take no new argument: set_table writes it into the
// host copy, which dial_set_user_table uploads.
#ifndef DIAL_PLUGIN_TABLE_VERSION   // (overridable on a plugin's command line: the tests build one that reports another version)
#define DIAL_PLUGIN_TABLE_VERSION 1
#endif
#define DIAL_PLUGIN_TABLE_SYMBOL "dial_plugin_table_v1"
struct dial_plugin_table {
  int version;                     // DIAL_PLUGIN_TABLE_VERSION
  size_t cmodel_bytes;             // sizeof(CModel<D>): the same constants as dial_plugin_ops' (ABI check)
  size_t sizeof_reward_in, sizeof_control_in;   // sizeof(DialRewardIn), sizeof(DialControlIn)
  // bind dev_table [rows, cols] (device memory) with offset row0 and mode DIAL_TABLE_*, or unbind (nullptr, rows 0); the caller
  // (dial_set_user_table) has validated the arguments
  void (*set_table)(void* host_cm, const float* dev_table, int rows, int cols, int row0, int mode);
};
typedef const dial_plugin_table* (*dial_plugin_table_entry)(void);

template <class D>
struct PluginTable {
  static void set_table(void* host_cm, const float* dev_table, int rows, int cols, int row0, int mode) {
    CModel<D>* c = (CModel<D>*)host_cm;
    const bool on = dev_table && rows > 0;
    // row0 as the device adds it to a step counter (rollout_body.h: table_row_index): no overflow for counters within +-2^24
    int r0 = 0;
    if (on && mode == DIAL_TABLE_WRAP) r0 = ((row0 % rows) + rows) % rows;
    else if (on) r0 = row0 < -(1 << 30) ? -(1 << 30) : (row0 > (1 << 30) ? (1 << 30) : row0);
    c->table = on ? dev_table : nullptr;
    c->table_rows = on ? rows : 0;
    c->table_cols = on ? cols : 0;
    c->table_row0 = r0;
    c->table_mode = on ? mode : 0;
    c->table_half = 0;
    c->table_cur = 0;
    c->table_nidx = 0;
    c->table_nr = 0;
  }
  static const dial_plugin_table* table() {
    static const dial_plugin_table tab = {DIAL_PLUGIN_TABLE_VERSION, sizeof(CModel<D>), sizeof(DialRewardIn), sizeof(DialControlIn), &set_table};
    return &tab;
  }
};

// ---- the table of one instantiation D (rollout kernels with WPB wavefronts per workgroup, occupancy target 3)
template <class D, int WPB>
struct PluginOps {
  static const char* check(const dial_model* m, const dial_derived* dv) {
    (void)dv;
    if (m->cone != DIAL_CONE_PYRAMIDAL) return "task plugins support pyramidal friction cones only (the model's cone is elliptic)";
    if (kbi_unique_rows(m) > DIAL_KBI_ROWS) return "the model has more distinct (solref, solimp) rows than the impedance table holds (DIAL_KBI_ROWS)";
    if (!dims_match<D>(m)) return "the model's dimensions differ from the plugin's (rebuild the plugin for this model)";
    return nullptr;
  }
  // dial_create's `upload` for the generic feature set at compile-time dimensions (dial_hip.hip)
  static int layout(const dial_model* model, const dial_cfg* cfg, int opt_con_cap, dial_plugin_layout* out) {
    Ws s;
    const int nnode = cfg ? cfg->Hnode + 1 : 0;
    out->ws0_words = ws_carve(s, (float*)0, model->nq, model->nv, model->nu, model->nbody, model->njnt, model->ngeom, model->nsite,
                              model->ncon, model->nefc, 0, dial::kNeedL<D>, D::square, 0, 0, D::NVP);
    out->cm_bytes = (int)(((sizeof(CModel<D>) + 15) / 16) * 16);
    out->con_cap = 0;
    out->ovf_words = 0;
    const bool given = opt_con_cap != 0;
    int cap = given ? opt_con_cap : 14;
    if (cfg && cap > 0 && model->ncon > cap) {
      if (!given) {   // the largest cap in 20 .. 4 with which NINE wavefronts (and their constants) fit a CU
        const size_t budget = WPB > 1 ? ((size_t)160 * 1024 / (9 / WPB) - out->cm_bytes) / WPB / 16 * 16
                                      : ((size_t)160 * 1024 / 9 - out->cm_bytes) / 16 * 16;
        for (int c = 20; c >= 4; c--) {
          Ws st;
          const int wds = ws_carve(st, (float*)0, model->nq, model->nv, model->nu, model->nbody, model->njnt, model->ngeom, model->nsite,
                                   model->ncon, model->nefc, nnode, dial::kNeedL<D>, D::square, 0, c, D::NVP);
          cap = c;
          if ((size_t)wds * sizeof(float) <= budget) break;
        }
      }
      out->con_cap = cap;
      Ws so;
      out->ovf_words = ws_overflow(so, (float*)0, model->nv, model->ncon, model->nefc);
    }
    out->ws_words = ws_carve(s, (float*)0, model->nq, model->nv, model->nu, model->nbody, model->njnt, model->ngeom, model->nsite,
                             model->ncon, model->nefc, nnode, dial::kNeedL<D>, D::square, 0, out->con_cap, D::NVP, 0);
    return DIAL_OK;
  }
  static void set_params(void* host_cm, const float* params, int n) {
    CModel<D>* c = (CModel<D>*)host_cm;
    for (int k = 0; k < DIAL_USER_PARAMS; k++) c->user_params[k] = (params && k < n) ? params[k] : 0.f;
  }
  static void fill(void* host_cm, const dial_model* m, const dial_task* t, const dial_derived* dv, const float* params, int n) {
    CModel<D>* c = new (host_cm) CModel<D>();
    fill_cmodel(c, m, t, dv);
    if constexpr (D::user_ctrl) { for (int a = 0; a < D::NU; a++) c->act_dofadr[a] = m->act_dofadr[a]; }
    set_params(c, params, n);
  }
  static hipError_t set_lds(size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void*)rollout_kernel<D, WPB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rollout_kernel<D, WPB, 3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rollout_kernel<D, WPB, 3, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return e;
  }
  static hipError_t occupancy(int* nb, size_t lds) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, rollout_kernel<D, WPB>, 64 * WPB, lds); }
  static hipError_t rollout(int variant, int blocks, size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, const dial_cfg* dcfg,
                            const dial::RolloutIO* io, int B, int ws_words, int* next) {
    const CModel<D>* cm = (const CModel<D>*)dcm;
    if (variant == 2)
      hipLaunchKernelGGL((rollout_kernel<D, WPB, 3, false, true>), dim3(blocks), dim3(64 * WPB), lds, st, cm, dtask, dcfg, *io, B, ws_words, (int*)nullptr);
    else if (variant == 1)
      hipLaunchKernelGGL((rollout_kernel<D, WPB, 3, true>), dim3(blocks), dim3(64 * WPB), lds, st, cm, dtask, dcfg, *io, B, ws_words, next);
    else
      hipLaunchKernelGGL((rollout_kernel<D, WPB, 3, false>), dim3(blocks), dim3(64 * WPB), lds, st, cm, dtask, dcfg, *io, B, ws_words, (int*)nullptr);
    return hipGetLastError();
  }
  static hipError_t env_step(int n, size_t lds, hipStream_t st, const void* dcm, const dial_task* dtask, float* state, const float* action,
                             float* xpos_out, float* xquat_out, float* ctrl_out, const float* plan_params) {
    hipLaunchKernelGGL(env_step_kernel<D>, dim3(n), dim3(64), lds, st, (const CModel<D>*)dcm, dtask, state, action, xpos_out, xquat_out, ctrl_out,
                       plan_params);
    return hipGetLastError();
  }
  static hipError_t env_reset(int n, size_t lds, hipStream_t st, const void* dcm, const float* qpos, const float* qvel, float* state,
                              float* xpos_out, float* xquat_out) {
    hipLaunchKernelGGL(env_reset_kernel<D>, dim3(n), dim3(64), lds, st, (const CModel<D>*)dcm, qpos, qvel, state, xpos_out, xquat_out);
    return hipGetLastError();
  }
  static const dial_plugin_ops* table() {
    static const dial_plugin_ops ops = {
        DIAL_PLUGIN_ABI_VERSION,
        {D::NQ, D::NV, D::NU, D::NB, D::NJ, D::NG, D::NS, D::NC, D::NL, D::NFRI},
        WPB, sizeof(CModel<D>),
        sizeof(dial_model), sizeof(dial_task), sizeof(dial_cfg), sizeof(dial_derived), sizeof(dial::RolloutIO),
        &check, &layout, &fill, &set_params, &set_lds, &occupancy, &rollout, &env_step, &env_reset};
    return &ops;
  }
};
