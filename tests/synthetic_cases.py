"""The synthetic robots of tests/synthetic/ (MJCF written for this project): tree shapes, joint kinds and actuator mixes that no shipped
robot has, each compiled by mjcf.compile_mjcf and wrapped in a CustomEnv like a user's own model.  Shared by
tests/test_synthetic_models.py (CPU: compiler tables, first-principles pins, host emulator) and tests/test_gpu_synthetic_models.py.

  chain_mixed  rotated free base with an off-centre rotated inertial frame; a body with a slide AND a hinge (anchors off the origin);
               a body with no joint inside the chain; a hinge on a rotated body; motors with gear 2 / 1 and a position actuator
  fixed_arm    no free joint: five hinges with mixed axes on rotated frames, then a slide; a tip sphere that reaches the floor
  two_trees    a free-base robot with two limbs and a SECOND free body; contact candidates between the trees and to the floor
  wide_base    six limbs of unequal depth on one free base (nv = 21), twelve floor contact candidates that all touch the base dofs
  deep_chain   a free base with one chain of six single-dof bodies: the 12-dof path limit (deep_chain_7: one more, refused)

A case carries two tasks: `ptask`, the CustomEnv's own (DIAL_TASK_USER: the plugin's reward, tests/synthetic/zoo_reward.hip), and
`otask`, the same control settings under the Go2 walk task (a built-in kind the oracle and the capacity-dimension kernel run).  The walk
task is VALID for the two models with four sites (WALK: feet mapped to those sites; walk_task_reads_in_range checks it) and compared
with its rewards; for the others it has no feet and only the physics is compared (PhysicsOnly: the kernels' walk reward unrolls over
four feet, the oracle's over task.nfeet)."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

from dial_mpc_amd import _abi
from dial_mpc_amd.config.base_env_config import BaseEnvConfig
from dial_mpc_amd.envs.custom_env import CustomEnv

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "synthetic")
MODELS = ("chain_mixed", "fixed_arm", "two_trees", "wide_base", "deep_chain")
WALK = ("chain_mixed", "wide_base")          # four sites: the Go2 walk task is valid with its feet mapped to them
REWARD = os.path.join(HERE, "zoo_reward.hip")
WEIGHTS = (0.5, 0.25, 2.0, 1.5, 0.125, 0.75)   # of qpos, qvel, xpos, xquat, ctrl, act (zoo_reward.hip)
M = _abi.MACROS
NI_REWARD = M["DIAL_INFO_REWARD"]


def xml_path(name):
    return os.path.join(HERE, name + ".xml")


def deep_chain_7(tmp_dir):
    """deep_chain with a seventh link (13 dofs on the path to it), written to tmp_dir -> its path."""
    text = open(xml_path("deep_chain")).read()
    link = ('<body name="l7" pos="0.08 0 0"><inertial pos="0.04 0 0" mass="0.2" diaginertia="0.0001 0.0003 0.0003"/>'
            '<joint name="j7" axis="0 0 1"/></body>')
    assert "<!-- seventh link -->" in text and "<!-- seventh actuator -->" in text
    text = text.replace("<!-- seventh link -->", link).replace("<!-- seventh actuator -->", '<position name="j7" joint="j7" kp="20"/>')
    text = text.replace('qpos="0 0 0.12 1 0 0 0 0 0 0 0 0 0"', 'qpos="0 0 0.12 1 0 0 0 0 0 0 0 0 0 0"')
    path = os.path.join(str(tmp_dir), "deep_chain_7.xml")
    with open(path, "w") as f:
        f.write(text)
    return path


@dataclass
class ZooConfig(BaseEnvConfig):
    dt: float = 0.02            # four physics steps of 0.005 s per control step
    timestep: float = 0.005
    leg_control: str = "position"
    kp: float = 30.0            # (BaseEnvConfig's default gains)
    kd: float = 1.0
    w_qpos: float = WEIGHTS[0]
    w_qvel: float = WEIGHTS[1]
    w_xpos: float = WEIGHTS[2]
    w_xquat: float = WEIGHTS[3]
    w_ctrl: float = WEIGHTS[4]
    w_act: float = WEIGHTS[5]


def env_class(path):
    """A CustomEnv subclass for the MJCF at `path`, as a user would write it."""
    name = os.path.splitext(os.path.basename(path))[0]
    return type("Zoo_" + name, (CustomEnv,), dict(model_path=path, reward_hip=REWARD,
                                                  user_params=("w_qpos", "w_qvel", "w_xpos", "w_xquat", "w_ctrl", "w_act")))


def mirror_reward(model, state, xpos, xquat, ctrl, act, w=WEIGHTS):
    """zoo_reward.hip in NumPy on what env.step / a rollout returns: the post-integration packed state, the pre-integration body
    frames (bodies 1 ..: the last body's z and w), the applied ctrl and the action."""
    nq, nv = model.nq, model.nv
    state, xpos, xquat = np.asarray(state, np.float64), np.asarray(xpos, np.float64).reshape(-1, 3), np.asarray(xquat, np.float64).reshape(-1, 4)
    return (w[0] * state[nq - 1] + w[1] * state[nq + nv - 1] + w[2] * xpos[-1, 2] + w[3] * xquat[-1, 0]
            + w[4] * float(np.asarray(ctrl)[-1]) + w[5] * float(np.asarray(act)[-1]))


@functools.lru_cache(maxsize=None)
def load(name, control="position", N=15, H=4):
    """The case of one model: env, compiled dict, model struct under DIAL_LS_SWAP, plugin task, oracle task, cfg (N + 1 rollouts of
    H + 1 control steps)."""
    from conftest import LS_SWAP, with_solver
    from dial_mpc_amd.core.dial_config import DialConfig
    from dial_mpc_amd.core.dial_core import make_cfg
    env = env_class(xml_path(name))(ZooConfig(leg_control=control))
    md = env.sys.model
    model = with_solver(env.make_model(), ls_rule=LS_SWAP)
    ptask = env.make_task()
    assert ptask.kind == M["DIAL_TASK_USER"] and ptask.n_frames == 4
    otask = walk_task(md, ptask, feet=name in WALK, home_z=float(env._init_q[2]))
    cfg = make_cfg(DialConfig(Nsample=N, Hsample=H, Hnode=min(4, H)))
    return dict(name=name, control=control, env=env, md=md, model=model, ptask=ptask, otask=otask, cfg=cfg, walk=name in WALK)


def walk_task(md, ptask, feet, home_z):
    """`ptask` as a Go2 walk task: body 1 the torso, the feet on sites 0 .. 3 (feet=True) or no feet at all."""
    t = type(ptask).from_buffer_copy(ptask)
    _abi.fill(t, dict(kind=M["DIAL_TASK_GO2_WALK"], torso_x=0, upright_x=0, nfeet=4 if feet else 0, feet_site=[0, 1, 2, 3] if feet else [],
                      foot_radius=0.02, gait_duty=0.6, gait_cadence=2.0, gait_amp=0.05, gait_phase=[0.0, 0.5, 0.5, 0.0],
                      cmd_vel=[0.4, 0.1, 0.0], cmd_ang_vel=[0.0, 0.0, 0.3], ramp_up_time=1.0, done_height=0.02,
                      init_pos_tar=[0.0, 0.0, home_z], n_stage=0, jump_dt=1.0))
    return t


def walk_task_reads_in_range(model, task):
    """None when everything the Go2 walk reward, its info update and its `done` test index lies inside the model's own arrays, else
    the first violation as text: the torso / upright bodies, four feet sites, qpos[7 + a] and qvel[6 + a] of every actuator."""
    if task.nfeet != 4:
        return f"nfeet = {task.nfeet}: the kernels' walk reward unrolls over four feet"
    for f in range(4):
        if not 0 <= task.feet_site[f] < model.nsite:
            return f"feet_site[{f}] = {task.feet_site[f]} with nsite = {model.nsite}"
    for what, x in (("torso_x", task.torso_x), ("upright_x", task.upright_x)):
        if not 0 <= x + 1 < model.nbody:
            return f"{what} = {x} with nbody = {model.nbody}"
    if model.njnt < 1 or model.jnt_type[0] != M["DIAL_JNT_FREE"] or model.jnt_qposadr[0] != 0:
        return "joint 0 is not a free base joint (the reward reads the base quaternion and velocity)"
    if 7 + model.nu > model.nq or 6 + model.nu > model.nv:
        return f"qpos[7 + a] / qvel[6 + a], a < {model.nu}, with nq = {model.nq}, nv = {model.nv}"
    return None


class PhysicsOnly:
    """An oracle whose env.step reports reward 0: with a zero `rewss` it takes the reward out of conftest.transition_parity, which
    then gates q, qd and x.pos alone (a plugin's reward is the user's; it is compared with its NumPy restatement instead)."""

    def __init__(self, oracle, ni):
        self._o, self._ni = oracle, ni

    def env_step(self, state, action):
        st, xpos, xquat, ctrl = self._o.env_step(state, action)
        st[self._ni + NI_REWARD] = 0
        return st, xpos, xquat, ctrl


def oracles(c, task="otask"):
    import oracle as O
    return O.Oracle(c["model"], c[task], c["cfg"], np.float64), O.Oracle(c["model"], c[task], c["cfg"], np.float32)


# ------------------------------------------------------------------------------------------------------------------ class F
@functools.lru_cache(maxsize=None)
def smooth_cases(name, control="position"):
    """(q, v, us) of the model's four class-F rollout cases: smooth_ref.rollout_cases_for on its env (free joints lifted by
    1 + 2 k m; fixed_arm's joint states are kept by the fp64 oracle only where the tip clears the floor by margin + 1 cm)."""
    import smooth_ref as S
    c = load(name, control)
    o64, _ = oracles(c)
    return S.rollout_cases_for(name, c["env"], c["model"], c["otask"], c["cfg"], o64)


# ------------------------------------------------------------------------------------------------------------------ in contact
CONTACT_T, CONTACT_B = 8, 16


def _free_joints(model):
    return [(int(model.jnt_qposadr[j]), int(model.jnt_dofadr[j])) for j in range(model.njnt) if model.jnt_type[j] == M["DIAL_JNT_FREE"]]


@functools.lru_cache(maxsize=None)
def contact_cases(name):
    """Two start states (qpos, qvel, float32) and controls us [2, 16, 8, nu] of the in-contact gate, position control:
      state 0  RESTING on its contacts: the fp64 oracle holds the keyframe's joint angles for 3 s from the keyframe (fixed_arm: it
               holds a pose whose tip target lies below the floor);
      state 1  the same pose 3 cm higher, moving down at 0.3 m/s (fixed_arm: its lift joint turned until the tip is 2 - 5 cm above
               the floor, turning back at 0.5 rad/s).
    us = the action that holds the resting pose + uniform noise in +- 0.3, clipped to +- 1."""
    import smooth_ref as S
    c = load(name, "position", N=CONTACT_B - 1, H=CONTACT_T - 1)
    model, task, env = c["model"], c["otask"], c["env"]
    o64, _ = oracles(c)
    nq, nv = model.nq, model.nv
    q0 = np.asarray(env._init_q, np.float64).copy()
    free = _free_joints(model)
    if not free:   # fixed_arm: reach down
        q0 = np.array([0.3, 0.75, 1.0, 0.2, -0.6, 0.2])   # (the tip sphere 3.5 cm below the floor)
    def hold_of(pose):   # position actuators hold the pose's angle; a motor reads its "target" as a force: zero
        pose = np.array(pose, np.float64)
        for a in range(model.nu):
            if not c["md"]["act_isposition"][a]:
                pose[int(model.act_qposadr[a])] = 0.0
        return np.clip(S.hold_action(model, task, pose), -1, 1)
    hold = hold_of(q0)
    st = o64.env_reset(q0, np.zeros(nv))[0]
    for k in range(500):   # 3 s at least, then until it is at rest (10 s at most)
        st = o64.env_step(st, hold)[0]
        if k >= 149 and np.abs(st[nq:nq + nv]).max() < 0.02:
            break
    rest_q, rest_v = st[:nq].copy(), st[nq:nq + nv].copy()
    d = o64.forward_dump(rest_q, rest_v)
    assert (d["con_dist"] < 0).any(), f"{name}: nothing touches in the resting state"
    assert np.abs(rest_v).max() < 0.05, f"{name}: not at rest after 10 s ({np.abs(rest_v).max():.3g})"
    up_q, up_v = rest_q.copy(), np.zeros(nv)
    if free:
        for qa, da in free:
            up_q[qa + 2] += 0.03
            up_v[da + 2] = -0.3
    else:
        lift, gap = 1, None
        step = np.zeros(nq)
        step[lift] = 0.002
        if o64.forward_dump(rest_q + step, up_v)["con_dist"].min() < o64.forward_dump(rest_q - step, up_v)["con_dist"].min():
            step = -step   # (the direction that raises the tip)
        for k in range(1, 200):
            trial = rest_q + k * step
            gap = float(o64.forward_dump(trial, up_v)["con_dist"].min())
            if gap >= 0.03:
                break
        assert 0.02 <= gap <= 0.05, (name, gap)
        up_q, up_v[lift] = trial, -0.5 * np.sign(step[lift])
    q = np.array([rest_q, up_q], np.float32)
    v = np.array([rest_v, up_v], np.float32)
    hold_rest = hold_of(rest_q if free else q0)
    us = hold_rest + np.random.default_rng(23).uniform(-0.3, 0.3, (2, CONTACT_B, CONTACT_T, model.nu))
    return c, q, v, np.clip(us, -1, 1).astype(np.float32)


def falling_case(c):
    """THE two_trees falling case: the keyframe pose with the robot's lowest geom 3 cm above the floor, the second body 1 cm above the
    trunk's capsule (two capsule-capsule candidates inside their margin at the start), every velocity uniform in +- 1, |us| <= 0.3."""
    model = c["model"]
    o64, _ = oracles(c)
    q = np.asarray(c["env"]._init_q, np.float64).copy()
    q[2] -= o64.forward_dump(q, np.zeros(model.nv))["con_dist"][:8].min() - 0.03
    q[13] = q[2] + 0.10
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, model.nv)
    us = rng.uniform(-0.3, 0.3, (CONTACT_B, CONTACT_T, model.nu)).astype(np.float32)
    return q.astype(np.float32), v.astype(np.float32), us


def jittered_oracle_run(o32, s0, us, ni, seed, mag=1.0):
    """The fp32 oracle as a stand-in device: every env.step starts from the previous step's state jittered by <= `mag` ulp in qpos /
    qvel / qacc_warmstart.  Returns (rewss, qss, qdss, xss) [B, T, ...] and the UNjittered packed states after every step [B, T, nstate]
    -- the arguments of conftest.transition_parity."""
    rng = np.random.default_rng(seed)
    B, T = us.shape[:2]
    nstate = len(s0)
    nq, nv = o32.nq, o32.nv
    rewss, qss, qdss = np.zeros((B, T), np.float32), np.zeros((B, T, nq), np.float32), np.zeros((B, T, nv), np.float32)
    xss, trace = np.zeros((B, T, o32.nx), np.float32), np.zeros((B, T, nstate), np.float32)
    for b in range(B):
        st = np.array(s0, np.float32)
        for t in range(T):
            stj = st.copy()
            stj[:ni] += (rng.integers(-1, 2, size=ni) * mag * np.spacing(np.abs(st[:ni]))).astype(np.float32)
            st, xpos, _, _ = o32.env_step(stj, us[b, t])
            trace[b, t], rewss[b, t], qss[b, t], qdss[b, t], xss[b, t] = st, st[ni + NI_REWARD], st[:nq], st[nq:nq + nv], xpos.reshape(-1)
    return (rewss, qss, qdss, xss), trace


def contact_gate(c, o32, s0, us, got, trace, physics_only):
    """conftest.transition_parity (1 x TOL per transition from the device's own traced state, <= 64 ulp witnesses) over EVERY rollout,
    unchecked: the report, for the caller's assertions on `unwitnessed` and `witnessed_share`."""
    from conftest import transition_parity
    model = c["model"]
    ni = model.nq + 2 * model.nv
    if physics_only:
        o32, got = PhysicsOnly(o32, ni), (np.zeros_like(got[0]),) + tuple(got[1:])
    return transition_parity(o32, s0, us, got, trace, range(us.shape[0]), model.nq, model.nv, check=False)


WITNESS_CAP = 0.10        # the largest share the project grants (conftest.TRANSITION_WITNESS_FRAC: 0.098)
REFERENCE_CAP = 0.05      # the fp32 oracle against itself under 1 ulp of jitter
