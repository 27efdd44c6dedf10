// Go2: walk forward at vx while holding the trunk at a height -- the reward of the custom-env example (go2_height_walk.py).
// The contract (what each input is, pre- or post-integration) is in dial_mpc_amd/csrc/user_reward.h.
//   params: 0 vx [m/s]  1 trunk height [m]  2 w_vel  3 w_height  4 w_upright  5 w_ctrl
//   info_user: 0 the trunk's forward velocity of the last step, 1 steps taken since env.reset
DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* p, float* info_user) {
  const int trunk = 1;                                    // body 1: the Go2's free-floating trunk ("base")
  const float* q = in.xquat + 4 * trunk;                  // (w, x, y, z), pre-integration
  const float zx = 2.f * (q[1] * q[3] + q[0] * q[2]);     // the trunk's z axis in the world frame
  const float zy = 2.f * (q[2] * q[3] - q[0] * q[1]);
  const float zz = 1.f - 2.f * (q[1] * q[1] + q[2] * q[2]);
  const float e_vel = in.qvel[0] - p[0];                  // free joint: world-frame linear velocity, post-integration
  const float e_h = in.xpos[3 * trunk + 2] - p[1];
  const float upright = zx * zx + zy * zy + (zz - 1.f) * (zz - 1.f);
  float tau2 = 0.f;
  for (int a = 0; a < in.nu; a++) tau2 += in.ctrl[a] * in.ctrl[a];
  info_user[0] = in.qvel[0];
  info_user[1] += 1.f;
  return -p[2] * e_vel * e_vel - p[3] * e_h * e_h - p[4] * upright - p[5] * tau2;
}
