// The reward every synthetic model's plugin carries (tests/synthetic_cases.py): a weighted sum of one element of each reward input,
// the LAST element of every array, so that a wrong stride or dimension of the plugin's instantiation shows.  Restated in NumPy by
// synthetic_cases.mirror_reward.  params: 0 .. 5 the weights of qpos, qvel, xpos, xquat, ctrl, act.
DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* p, float* info_user) {
  const float a = in.qpos[in.nq - 1], b = in.qvel[in.nv - 1];
  const float c = in.xpos[3 * in.nbody - 1], d = in.xquat[4 * in.nbody - 4];
  const float e = in.ctrl[in.nu - 1], f = in.act[in.nu - 1];
  info_user[0] += 1.f;
  return p[0] * a + p[1] * b + p[2] * c + p[3] * d + p[4] * e + p[5] * f;
}
