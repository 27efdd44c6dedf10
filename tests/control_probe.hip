// Probe control law of the user-control tests (tests/control_cases.py): ONE law with a mode chosen at run time, so that one plugin
// per model serves every check without a rebuild.  The reward next to it is tests/plugin_probe.hip, which owns params[0], params[1].
//   params[2]  mode
//     0  BaseEnv's torque law restated: act2joint, then the PD law on qpos[7 + a] / qvel[6 + a], clipped to tau_range (the
//        expression order of rollout_body.h: env_step)
//     1  BaseEnv's position law restated: ctrl = act2joint
//     2  pass-through: ctrl = act[a]
//     3  mode 0's law on the actuator's OWN joint: qpos[act_qposadr[a]] / qvel[act_dofadr[a]]
//     4  field probe: the input element selected by (params[3], params[4]) = (field, index)
//          1 qpos  2 qvel  3 act  4 step  5 dt  6 nq  7 nv  8 nu  9 act_qposadr  10 act_dofadr  11 action_scale  12 kp  13 kd
//          14 joint_range  15 phys_range  16 tau_range (flat [nu][2])  17 joint_offset  18 info_user  19 the actuator index a
//        An index outside its array, or an unknown field, gives CPROBE_BAD (the probe reads nothing out of bounds).
//   params[5]  every mode's result is scaled by 1 + params[5] (per-plan rows become visible)
#define CPROBE_BAD (-12345.f)

DIAL_DEV float cprobe_at(const float* a, int n, int i) { return i >= 0 && i < n ? a[i] : CPROBE_BAD; }
DIAL_DEV float cprobe_ati(const int32_t* a, int n, int i) { return i >= 0 && i < n ? (float)a[i] : CPROBE_BAD; }
DIAL_DEV float cprobe_clip(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

DIAL_DEV float cprobe_act2joint(const DialControlIn& in, int a) {
  const float an = (in.act[a] * in.action_scale + 1.0f) / 2.0f;
  const float jt = (in.joint_range[2 * a] + in.joint_offset[a]) + an * (in.joint_range[2 * a + 1] - in.joint_range[2 * a]);
  return cprobe_clip(jt, in.phys_range[2 * a], in.phys_range[2 * a + 1]);
}

DIAL_DEV float cprobe_pd(const DialControlIn& in, int a, float q, float qd) {
  const float q_err = cprobe_act2joint(in, a) - q;
  return cprobe_clip(in.kp[a] * q_err - in.kd[a] * qd, in.tau_range[2 * a], in.tau_range[2 * a + 1]);
}

DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* params, const float* info_user) {
  const int mode = (int)params[2];
  float v = CPROBE_BAD;
  if (mode == 0) v = cprobe_pd(in, a, in.qpos[7 + a], in.qvel[6 + a]);
  else if (mode == 1) v = cprobe_act2joint(in, a);
  else if (mode == 2) v = in.act[a];
  else if (mode == 3) v = cprobe_pd(in, a, in.qpos[in.act_qposadr[a]], in.qvel[in.act_dofadr[a]]);
  else if (mode == 4) {
    const int i = (int)params[4];
    switch ((int)params[3]) {
      case 1: v = cprobe_at(in.qpos, in.nq, i); break;
      case 2: v = cprobe_at(in.qvel, in.nv, i); break;
      case 3: v = cprobe_at(in.act, in.nu, i); break;
      case 4: v = in.step; break;
      case 5: v = in.dt; break;
      case 6: v = (float)in.nq; break;
      case 7: v = (float)in.nv; break;
      case 8: v = (float)in.nu; break;
      case 9: v = cprobe_ati(in.act_qposadr, in.nu, i); break;
      case 10: v = cprobe_ati(in.act_dofadr, in.nu, i); break;
      case 11: v = in.action_scale; break;
      case 12: v = cprobe_at(in.kp, in.nu, i); break;
      case 13: v = cprobe_at(in.kd, in.nu, i); break;
      case 14: v = cprobe_at(in.joint_range, 2 * in.nu, i); break;
      case 15: v = cprobe_at(in.phys_range, 2 * in.nu, i); break;
      case 16: v = cprobe_at(in.tau_range, 2 * in.nu, i); break;
      case 17: v = cprobe_at(in.joint_offset, in.nu, i); break;
      case 18: v = cprobe_at(info_user, DIAL_INFO_USER_N, i); break;
      case 19: v = (float)a; break;
      default: break;
    }
  }
  return v * (1.0f + params[5]);
}
