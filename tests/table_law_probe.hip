// Probe control law of the reference-table tests (tests/table_cases.py): mode 0 of tests/control_probe.hip -- BaseEnv's torque law
// restated: act2joint, then the PD law on qpos[7 + a] / qvel[6 + a], clipped to tau_range, in the expression order of
// rollout_body.h: env_step -- applied to act[a] + row[a], the action plus column a of the step's table row (act[a] alone with no table
// bound).  With a table of nu columns the physics is the built-in law's under the actions us + rows.
DIAL_DEV float tlaw_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user) {
  (void)params; (void)info_user;
  const float act = in.row != nullptr && a < in.table_cols ? in.act[a] + in.row[a] : in.act[a];
  const float an = (act * in.action_scale + 1.0f) / 2.0f;
  const float jt = tlaw_clip((in.joint_range[2 * a] + in.joint_offset[a]) + an * (in.joint_range[2 * a + 1] - in.joint_range[2 * a]),
                             in.phys_range[2 * a], in.phys_range[2 * a + 1]);
  const float q_err = jt - in.qpos[7 + a];
  return tlaw_clip(in.kp[a] * q_err - in.kd[a] * in.qvel[6 + a], in.tau_range[2 * a], in.tau_range[2 * a + 1]);
}
