"""Shared pieces of the user-control-law tests (tests/test_custom_control.py on the CPU, tests/test_gpu_custom_control.py on the GPU):
the probe law of tests/control_probe.hip built into the plugins of two models of tests/plugin_cases.py (next to the probe reward of
tests/plugin_probe.hip), the parameter vector both probes read, a host evaluation of the probe's PD modes in fp64, and the Go2 with
permuted actuators under a law."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from plugin_cases import HERE, case_model_dict, probe_source

CONTROL = os.path.join(HERE, "control_probe.hip")
MODELS = ("go2", "h1_push_crate")          # go2_nf4 shares go2's plugin (n_frames is task data)
# field codes of the law's mode 4 (control_probe.hip)
CF = dict(qpos=1, qvel=2, act=3, step=4, dt=5, nq=6, nv=7, nu=8, act_qposadr=9, act_dofadr=10, action_scale=11, kp=12, kd=13,
          joint_range=14, phys_range=15, tau_range=16, joint_offset=17, info_user=18, lane=19)
CPROBE_BAD = -12345.0
PERM = np.r_[3:12, 0:3]                     # tests/test_plugin_matrix.py: the front-right leg's three actuators moved to the end


def control_source():
    return open(CONTROL).read()


def params(mode, field=0, idx=0, cfield=0, cidx=0, scale=0.0):
    """The task parameters of the two probes: [reward field, reward index, law mode, law field, law index, law scale - 1]."""
    return [float(field), float(idx), float(mode), float(cfield), float(cidx), float(scale)]


def build_control_plugins(names=MODELS, jobs=4):
    """Build (or find in the cache) the plugins with the probe reward AND the probe law -> {name: path}."""
    from dial_mpc_amd.plugin import build_plugin
    names = list(names)
    rew, law = probe_source(), control_source()
    with ThreadPoolExecutor(max_workers=min(jobs, 4)) as ex:
        paths = list(ex.map(lambda n: build_plugin(case_model_dict(n), rew, control_src=law), names))
    return dict(zip(names, paths))


def task_consts(task, nu):
    """The control constants of a dial_task as the kernels hold them (fp32)."""
    from dial_mpc_amd import _abi
    g = lambda k: np.asarray(_abi.as_numpy(task, k), np.float32)   # noqa: E731
    return dict(action_scale=np.float32(task.action_scale), kp=g("kp")[:nu], kd=g("kd")[:nu], joint_range=g("joint_range")[:nu],
                phys_range=g("phys_range")[:nu], tau_range=g("tau_range")[:nu], joint_offset=g("joint_offset")[:nu])


def host_pd(k, qpos, qvel, act, qadr, dadr):
    """Modes 0 / 3 of the probe law in fp64 from the kernel's own fp32 inputs -> (ctrl [nu], bound [nu]).
    bound = 16 * 2^-24 * (kp (|lo| + |hi| + |q|) + kd |qd|): the chain act2joint -> PD has at most 11 fp32 roundings, each relative
    to a partial result no larger than that sum.  The comparison is made after the tau_range clip (a clip never widens a difference)."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    act, q, qd = f(act), f(qpos)[qadr], f(qvel)[dadr]
    jr, pr, tr = f(k["joint_range"]), f(k["phys_range"]), f(k["tau_range"])
    kp, kd = f(k["kp"]), f(k["kd"])
    an = (act * float(k["action_scale"]) + 1.0) / 2.0
    jt = np.clip((jr[:, 0] + f(k["joint_offset"])) + an * (jr[:, 1] - jr[:, 0]), pr[:, 0], pr[:, 1])
    tau = np.clip(kp * (jt - q) - kd * qd, tr[:, 0], tr[:, 1])
    bound = 16.0 * 2.0 ** -24 * (kp * (np.abs(jr[:, 0]) + np.abs(jr[:, 1]) + np.abs(q)) + kd * np.abs(qd))
    return tau, bound


def host_act2joint(k, act):
    """Mode 1 of the probe law in fp64."""
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    jr, pr = f(k["joint_range"]), f(k["phys_range"])
    an = (f(act) * float(k["action_scale"]) + 1.0) / 2.0
    return np.clip((jr[:, 0] + f(k["joint_offset"])) + an * (jr[:, 1] - jr[:, 0]), pr[:, 0], pr[:, 1])


def load_position_case(N=16, H=12):
    """plugin_cases.load_case("go2") under leg_control: position (the same plugin: the control mode is task data)."""
    import yaml
    from conftest import LS_SWAP, with_solver
    from dial_mpc_amd import _abi
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path("unitree_go2_trot.yaml")))
    d.update(Nsample=N, Hsample=H, leg_control="position")
    dc, _, env = load_dial_and_env(d)
    md = dict(env.sys.model)
    model = with_solver(_abi.make_model(md), ls_rule=LS_SWAP)
    otask = env.make_task()
    assert otask.position_control == 1
    ptask = type(otask).from_buffer_copy(otask)
    ptask.kind = _abi.MACROS["DIAL_TASK_USER"]
    return dict(name="go2_pos", dc=dc, env=env, md=md, model=model, ptask=ptask, otask=otask, cfg=make_cfg(dc))


def permuted_go2_env(leg_control, with_law=True, base=None):
    """The permuted-actuator Go2 of tests/test_plugin_matrix.py (its make_system recipe), optionally with the probe law.  Actuator a
    drives joint PERM[a], so the per-actuator control constants (sampling range, joint limits, torque range) are permuted with it;
    `base` (an env of the unpermuted Go2) provides the sampling range."""
    from dial_mpc_amd.envs.custom_env import CustomEnv
    from dial_mpc_amd.envs.unitree_go2_env import UnitreeGo2EnvConfig

    class Permuted(CustomEnv):
        model_path = "../dial_mpc_amd/models/unitree_go2/mjx_scene_force.json"
        reward_hip = "plugin_probe.hip"
        control_hip = "control_probe.hip" if with_law else ""

        def make_system(self, config):
            sys_ = super().make_system(config)
            m = sys_.model
            for k in [k for k in m if k.startswith("act_")]:
                m[k] = np.asarray(m[k])[PERM]
            return sys_

        def __init__(self, config):
            super().__init__(config)
            self.physical_joint_range = np.asarray(self.physical_joint_range)[PERM]
            self.joint_range = self.physical_joint_range if base is None else np.asarray(base.joint_range)[PERM]
            self.joint_torque_range = np.asarray(self.sys.model["act_ctrlrange"], dtype=np.float64)

    if base is None:
        return Permuted(UnitreeGo2EnvConfig(leg_control=leg_control))
    import copy
    cfg = copy.copy(base._config)
    cfg.leg_control = leg_control
    return Permuted(cfg)
