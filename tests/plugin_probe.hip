// Probe reward of the plugin tests (tests/plugin_cases.py): returns ONE element of the reward's inputs (csrc/user_reward.h), chosen
// at run time, so that one plugin per model reads every input without a rebuild.
//   selector: (field, index).  info_user[0] > 0: from info_user[0], info_user[1] (written into the packed state before an env.step;
//             the probe never writes these two slots, so the selector persists); else from params[0], params[1] (rollouts).
//   field:    1 qpos  2 qvel  3 xpos  4 xquat  5 spos  6 cdist  7 cpos  8 ctrl  9 act  (index: the flat element of the array)
//             10 step  11 dt  12 nq  13 nv  14 nu  15 nbody  16 nsite  17 ncon  18 the info_user counter (after this step's update)
//   info_user[2]: steps taken since env.reset (incremented every step); info_user[3]: the value returned by the previous step.
//   An index outside its array, or an unknown field, returns PROBE_BAD (the probe reads nothing out of bounds).
#define PROBE_BAD (-12345.f)

DIAL_DEV float probe_at(const float* a, int n, int i) { return i >= 0 && i < n ? a[i] : PROBE_BAD; }

DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* params, float* info_user) {
  const bool own = info_user[0] > 0.f;
  const int field = (int)(own ? info_user[0] : params[0]);
  const int i = (int)(own ? info_user[1] : params[1]);
  info_user[2] += 1.f;
  float v = PROBE_BAD;
  switch (field) {
    case 1: v = probe_at(in.qpos, in.nq, i); break;
    case 2: v = probe_at(in.qvel, in.nv, i); break;
    case 3: v = probe_at(in.xpos, 3 * in.nbody, i); break;
    case 4: v = probe_at(in.xquat, 4 * in.nbody, i); break;
    case 5: v = probe_at(in.spos, 3 * in.nsite, i); break;
    case 6: v = probe_at(in.cdist, in.ncon, i); break;
    case 7: v = probe_at(in.cpos, 3 * in.ncon, i); break;
    case 8: v = probe_at(in.ctrl, in.nu, i); break;
    case 9: v = probe_at(in.act, in.nu, i); break;
    case 10: v = in.step; break;
    case 11: v = in.dt; break;
    case 12: v = (float)in.nq; break;
    case 13: v = (float)in.nv; break;
    case 14: v = (float)in.nu; break;
    case 15: v = (float)in.nbody; break;
    case 16: v = (float)in.nsite; break;
    case 17: v = (float)in.ncon; break;
    case 18: v = info_user[2]; break;
    default: break;
  }
  info_user[3] = v;
  return v;
}
