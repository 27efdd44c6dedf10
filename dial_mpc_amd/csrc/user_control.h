// user_control.h -- the contract of a user control law, the optional second function a custom environment writes in HIP.
//
//   DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user);
//
// A task plugin built with a law (dial_mpc_amd/plugin.py: build_plugin(..., control_src=)) compiles it into the rollout / env.step
// kernels of ONE model in place of BaseEnv's act2joint + "joint target or PD torque" block (rollout_body.h: env_step), and into
// user_control_kernel (plugin_ops.h), which evaluates it for rows of (packed state, action) so that no host code restates it.
//
// It returns ctrl[a], the value actuator `a` receives.  The model's actuators apply it exactly as they apply the built-in law's
// output: gear, the ctrlrange clip where the actuator is limited, motor or position actuator.  The value is what the reward sees as
// in.ctrl[a], what env.step returns as ctrl, and what the step leaves in info[DIAL_INFO_LAST_CTRL + a].  With a law present the
// kernels ignore the task's position_control, kp and kd; the law may still read kp and kd.
//
// When and where: ONCE per control step, before the step's n_frames physics sub-steps (like the built-in law), on lane `a` for all
// a < nu concurrently.  The function reads and does not write; it must be deterministic.
//
// What it sees:
//   nq, nv, nu        the model's dimensions
//   step, dt          the step counter BEFORE this step (0 on the first step after env.reset); the control step in seconds
//   qpos [nq], qvel [nv]   the state the control step STARTS from
//   act [nu]          the normalised action in [-1, 1] the planner chose
//   act_qposadr [nu], act_dofadr [nu]   actuator a's joint: its position is qpos[act_qposadr[a]], its velocity qvel[act_dofadr[a]]
//   the task's control constants as BaseEnv fills them (dial_task): action_scale, kp [nu], kd [nu], joint_range [nu][2] (the
//   sampling range), phys_range [nu][2] (the joint limits), tau_range [nu][2] (the actuators' ctrlrange), joint_offset [nu]
//   params:    the DIAL_USER_PARAMS task parameters the reward gets too (the per-plan row where rows are bound)
//   info_user: READ-ONLY view of the DIAL_INFO_USER_N slots as the reward left them on the previous step; zero after env.reset
//   the reference table (dial_set_user_table; optional), exactly as the reward of the same control step sees it (user_reward.h
//   states the index rule): row [table_cols] the step's row, picked by `step`; row_index; table / table_rows / table_cols the whole
//   table in global memory for look-ahead.  Unlike poses the row IS valid at control time -- it depends on the step counter only,
//   not on forward().  With no table bound: table == row == nullptr, table_rows == table_cols == 0, row_index == 0.
// What it does NOT see, and why: body / site poses (xpos, xquat, spos), contact distances and points, velocities of bodies.  They
// are results of forward(), and at control time they are not valid: the first step after a state was loaded (the start of every
// rollout, every env.step) has not run forward() yet, so the workspace holds either nothing or another sample's values.  A law that
// needs a pose computes it from qpos, or has the reward leave it in info_user for the next step.
#pragma once
#include <stdint.h>

#include "../../include/dial_mpc.h"

#ifndef DIAL_DEV
#define DIAL_DEV __device__ __forceinline__
#endif

struct DialControlIn {
  int nq, nv, nu;
  float step, dt;
  const float *qpos, *qvel;                            // the state the control step starts from
  const float* act;
  const int32_t *act_qposadr, *act_dofadr;
  float action_scale;
  const float *kp, *kd;
  const float *joint_range, *phys_range, *tau_range;   // [nu][2]: lo, hi
  const float* joint_offset;
  // (appended: control sources that predate the reference table compile unchanged)
  const float* row;                                    // the step's row of the reference table [table_cols], nullptr without one
  int row_index;
  const float* table;                                  // [table_rows][table_cols] in global memory, or nullptr
  int table_rows, table_cols;
};

// defined by the plugin's control source (the plugin's translation unit only; no kernel of libdialhip.so calls it)
DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user);
