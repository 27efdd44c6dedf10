// BaseEnv's torque law restated as a user control law (contract: dial_mpc_amd/csrc/user_control.h): act2joint, then the PD torque on
// qpos[7 + a] / qvel[6 + a], clipped to tau_range -- what every kernel runs when an env has no law.  A starting point for a law of
// your own, and the law tools/bench_custom_env.py --control-law times against the plugin without one.
DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user) {
  (void)params;
  (void)info_user;
  const float an = (in.act[a] * in.action_scale + 1.0f) / 2.0f;
  float jt = (in.joint_range[2 * a] + in.joint_offset[a]) + an * (in.joint_range[2 * a + 1] - in.joint_range[2 * a]);
  jt = fminf(fmaxf(jt, in.phys_range[2 * a]), in.phys_range[2 * a + 1]);
  const float tau = in.kp[a] * (jt - in.qpos[7 + a]) - in.kd[a] * in.qvel[6 + a];
  return fminf(fmaxf(tau, in.tau_range[2 * a]), in.tau_range[2 * a + 1]);
}
