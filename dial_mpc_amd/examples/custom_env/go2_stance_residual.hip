// Go2: residual control around the stance pose -- the control law of the custom-env example go2_stance_residual.py.
// The contract (what each input is, what is not available at control time) is in dial_mpc_amd/csrc/user_control.h.
//   target  = home pose + action_scale * act * half the joint's sampling span, clipped to the joint limits
//   torque  = kp (target - q) - kd qd on the actuator's OWN joint (act_qposadr / act_dofadr), clipped to tau_range
// joint_offset holds the home keyframe's joint angles (the env's task_dict fills it).  act = 0 holds the stance.
DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user) {
  (void)params;
  (void)info_user;
  const float half_span = 0.5f * (in.joint_range[2 * a + 1] - in.joint_range[2 * a]);
  const float target = fminf(fmaxf(in.joint_offset[a] + in.action_scale * in.act[a] * half_span, in.phys_range[2 * a]), in.phys_range[2 * a + 1]);
  const float tau = in.kp[a] * (target - in.qpos[in.act_qposadr[a]]) - in.kd[a] * in.qvel[in.act_dofadr[a]];
  return fminf(fmaxf(tau, in.tau_range[2 * a]), in.tau_range[2 * a + 1]);
}
