// Go2: track a joint-space clip from the reference table -- the reward of the custom-env example go2_track_clip.py.
// The contract (what each input is, the table's row of a step) is in dial_mpc_amd/csrc/user_reward.h.
//   in.row: this control step's row of the clip: 0 .. 11 joint targets [rad] (the actuators' order), 12 the trunk's height [m]
//   params: 0 w_joint  1 w_height  2 w_upright  3 w_ctrl
// Only + - * (no divide, square root or transcendental): the terms are weighted squared errors.
DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* p, float* info_user) {
  (void)info_user;
  const int trunk = 1;                                    // body 1: the Go2's free-floating trunk ("base")
  const float* q = in.xquat + 4 * trunk;                  // (w, x, y, z), pre-integration
  const float zx = 2.f * (q[1] * q[3] + q[0] * q[2]);     // the trunk's z axis in the world frame
  const float zy = 2.f * (q[2] * q[3] - q[0] * q[1]);
  const float zz = 1.f - 2.f * (q[1] * q[1] + q[2] * q[2]);
  const float upright = zx * zx + zy * zy + (zz - 1.f) * (zz - 1.f);
  float e_joint = 0.f;                                    // post-integration joint angles against the step's targets
  for (int a = 0; a < 12; a++) { const float e = in.qpos[7 + a] - in.row[a]; e_joint += e * e; }
  const float e_h = in.xpos[3 * trunk + 2] - in.row[12];
  float tau2 = 0.f;
  for (int a = 0; a < in.nu; a++) tau2 += in.ctrl[a] * in.ctrl[a];
  return -p[0] * e_joint - p[1] * e_h * e_h - p[2] * upright - p[3] * tau2;
}
