// user_reward.h -- the contract of a user reward (DIAL_TASK_USER), the one function a custom environment writes in HIP.
//
//   DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* params, float* info_user);
//
// A task plugin (dial_mpc_amd/plugin.py) compiles it into the rollout / env.step / env.reset kernels of ONE model, at that model's
// compile-time dimensions (cmodel.h: DimsUser).  It is evaluated once per control step, on ONE lane of the wavefront, after the
// step's physics (rollout_body.h: env_step); its return value is the step's reward (info[DIAL_INFO_REWARD], the per-step rewards of a
// rollout, the mean rewards that weight the samples).
//
// What it sees, and when (the rule every built-in reward follows -- brax's pipeline_state after mjx.step):
//   POST-integration (the state the step ends in):  qpos [nq], qvel [nv]
//   PRE-integration forward quantities (kinematics / collision of the last forward() before the integrator: the state the step
//   started from when n_frames == 1, see below):     xpos [nbody][3], xquat [nbody][4] (w x y z), spos [nsite][3],
//                                                    cdist [ncon], cpos [ncon][3] (per static contact slot of the model)
//   the step's control:                              act [nu]  (the normalised action in [-1, 1] the planner chose)
//                                                    ctrl [nu] (what was applied: torques, or joint targets under position control)
//   step:  the step counter BEFORE this step (0 on the first step after env.reset); dt: the control step in seconds
//          (n_frames x timestep, fp32).
// n_frames > 1 (a control step of several physics sub-steps): the pre-integration quantities are those of the LAST sub-step's
// forward(), i.e. of the state before the last sub-step -- brax's pipeline_state after the last mjx.step.  They coincide with the
// state the step started from only when n_frames == 1.
// Body / site / contact indices are the model's own.  Body 0 is the world: xpos[0..2] = 0, xquat[0..3] = (1, 0, 0, 0); the robot's
// first body is body 1.  Every array is read-only.
// cdist / cpos hold every static contact slot, touching or not: the narrow phase's signed distance and midpoint, recomputed by
// every forward() (never left over from an earlier step or sample).  One exception: a plane-box, capsule-box or box-box slot that
// the broad phase puts more than 1 cm (DIAL_BOX_PARK_DIST) from touching is PARKED -- cdist is above 1 cm, either a lower bound of
// the distance (the broad phase's gap) or 1.0; cpos is the box's centre for a plane-box slot and the midpoint of the two geoms'
// centres for a capsule-box or box-box slot.  Compare cdist with a threshold below 1 cm; read cpos only for slots within it.
//   params:    the DIAL_USER_PARAMS task parameters (dial_create_plugin / dial_set_user_params; unset entries are zero).
//   info_user: DIAL_INFO_USER_N read / write floats of the env info (slots DIAL_INFO_USER ...).  Zero after env.reset; they persist
//              from step to step of a rollout and across env.step, like upstream's state.info.
//   the reference table (dial_set_user_table; optional): one device-resident float table [table_rows][table_cols] per context, data
//   that changes from step to step -- a motion clip, a footstep or contact schedule, feed-forward torques, scheduled gains.
//     row [table_cols]   the row of THIS control step, already on chip; row_index: which row of the table that is
//     table, table_rows, table_cols   the whole table in global memory, for look-ahead (table[i * table_cols + j]); such a read
//                        is a global load on the reward lane, after the physics: the step's own row is cheaper through `row`
//   Row of a step: r = (int)step + row0 with `step` as above (the counter BEFORE the step), then
//     DIAL_TABLE_CLAMP:  row_index = min(max(r, 0), table_rows - 1)      DIAL_TABLE_WRAP:  row_index = ((r % rows) + rows) % rows
//   so step k of a rollout from a state with counter s0 reads row s0 + k + row0, and the states of a grouped launch or of an
//   env.step batch each read by their own counter.  The control law of the same control step (user_control.h) sees the SAME row.
//   The row is valid whenever the reward runs (it does not depend on forward()).  With no table bound: table == row == nullptr,
//   table_rows == table_cols == 0, row_index == 0.  The table is read-only; its contents are the caller's and may change between
//   launches (never during one).
// The function must be deterministic and free of side effects beyond info_user: it runs in every sample of every rollout.
#pragma once
#include "../../include/dial_mpc.h"

#ifndef DIAL_DEV
#define DIAL_DEV __device__ __forceinline__
#endif

static_assert(DIAL_INFO_LAST_CTRL + DIAL_MAX_U <= DIAL_INFO_USER && DIAL_INFO_USER + DIAL_INFO_USER_N <= DIAL_INFO_N,
              "the user slots of the env info overlap the built-in ones");

struct DialRewardIn {
  int nq, nv, nu, nbody, nsite, ncon;
  float step, dt;
  const float *qpos, *qvel;                       // post-integration
  const float *xpos, *xquat, *spos, *cdist, *cpos;   // pre-integration forward quantities
  const float *ctrl, *act;                        // the step's control
  // (appended: reward sources that predate the reference table compile unchanged)
  const float* row;                               // the step's row of the reference table [table_cols], nullptr without a table
  int row_index;                                  // which row that is
  const float* table;                             // the whole table [table_rows][table_cols] in global memory, or nullptr
  int table_rows, table_cols;
};

// defined by the plugin's reward source (the plugin's translation unit only; no kernel of libdialhip.so calls it)
DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* params, float* info_user);
