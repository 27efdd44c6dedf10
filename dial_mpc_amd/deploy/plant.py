"""The plant of ``dial-mpc-sim`` on the HIP path: the env's own compiled scene stepped at ``sim_dt`` by the plant kernel
(csrc/plant_kernel.h, ``dial_plant_step``), with the reference's rules for which row of the published plan each step applies
(dial_mpc/deploy/dial_sim.py).

``ctrl_row`` and ``sync_steps`` restate those rules on the host in fp64; the kernel picks its rows with the same arithmetic and the
GPU tests compare the two bit for bit.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np


def ctrl_row(t: float, plan_time, ctrl_dt: float, n_acts: int) -> int:
    """dial_sim.py's async rule: delta = t - plan_time (fp64; plan_time is the float32 read from plan_time_shm),
    int(delta / ctrl_dt), and the last row when that is >= n_acts or < 0."""
    q = (float(t) - float(np.float32(plan_time))) / float(ctrl_dt)
    if not math.isfinite(q):
        return n_acts - 1
    k = int(q)
    if k >= n_acts or k < 0:
        k = n_acts - 1
    return k


def sync_steps(t: float, plan_time, ctrl_dt: float, sim_dt: float) -> int:
    """dial_sim.py's sync rule: how many sim steps `while t <= plan_time + ctrl_dt: step; t += sim_dt` runs (fp64)."""
    limit = float(np.float32(plan_time)) + float(ctrl_dt)
    n = 0
    t = float(t)
    while t <= limit:
        t += float(sim_dt)
        n += 1
    return n


def law_step(t: float, ctrl_dt: float) -> int:
    """The control step the clock t is in, as DIAL_PLANT_LAW hands it to a custom env's control law (csrc/plant_kernel.h:
    plant_law_step): the fp64 quotient t / ctrl_dt truncated toward zero, 0 when the quotient is not >= 0 (negative clocks, NaN),
    at most 2^24."""
    q = float(t) / float(ctrl_dt)
    if not q >= 0.0:
        return 0
    if q >= 16777216.0:
        return 1 << 24
    return int(q)


class Plant:
    """M copies of an env's plant, stepped on the GPU.  ``leg_control``: "torque" -- the rows are the actuators' ctrl as they are
    (DIAL_PLANT_CTRL, dial_sim.py's ``data.ctrl = tau_shared[k]``); "position" -- the rows are joint targets, turned into torques by
    the env's PD law at every sim step (DIAL_PLANT_PD), or, on models whose actuators are position actuators (the Allegro), handed to
    them as their ctrl (DIAL_PLANT_CTRL).  A custom environment (envs/custom_env.py) is stepped by the plant kernel of its own task
    plugin (csrc/plant_kernel.h at the model's dimensions, behind csrc/plant_plugin.h's table); "position" there needs the PD law's
    joint indexing (torque_joint_convention), and an env with a
    control law (control_hip) has a third mode, "law": the rows are normalised actions and the law runs at every sim step from the
    plant's current state (DIAL_PLANT_LAW; law_step is the step counter it sees)."""

    def __init__(self, env, sim_dt: float, leg_control: str = "torque", M: int = 1, device: Optional[int] = None):
        import torch
        from dial_mpc_amd import _lib
        from dial_mpc_amd.envs.custom_env import CustomEnv, torque_joint_convention
        custom = isinstance(env, CustomEnv)
        if leg_control not in ("torque", "position", "law"):
            raise ValueError(f"sim_leg_control must be 'torque', 'position' or 'law', not {leg_control!r}")
        if leg_control == "law" and not (custom and env.control_hip):
            raise ValueError(f"sim_leg_control: law needs a custom environment with a control law (control_hip); {type(env).__name__} has none")
        nu = int(env.sys.nu)
        positional = bool(np.any(np.asarray(env.make_model().act_isposition)[:nu]))
        if leg_control == "law":
            self.flags = _lib.PLANT_LAW
        elif leg_control == "torque" or positional:
            self.flags = _lib.PLANT_CTRL
        else:
            if custom:
                torque_joint_convention(env.sys.model)
            self.flags = _lib.PLANT_PD
        self.env, self.sim_dt, self.M = env, float(sim_dt), int(M)
        self.ctrl_dt = float(env._config.dt)
        self._hold = _lib.PLANT_HOLD_FIRST
        self.ctx = env.make_plant(self.sim_dt, device=device)
        self.nq, self.nv, self.nu = self.ctx.nq, self.ctx.nv, self.ctx.nu
        self.width = 1 + self.nq + self.nv + self.nu          # trace / record row: [t, qpos, qvel, ctrl]
        self.dev = self.ctx.torch_device
        self._torch = torch
        self.reset()

    def reset(self):
        """Every plant at the env's initial pose (the home keyframe; env.reset's), zero velocity, t = 0."""
        torch = self._torch
        q0 = np.asarray(self.env._init_q, np.float32)
        qpos = torch.as_tensor(np.tile(q0, (self.M, 1)), device=self.dev)
        qvel = torch.zeros((self.M, self.nv), dtype=torch.float32, device=self.dev)
        self.states = self.ctx.env_reset_batch(qpos, qvel)
        self.t_dev = torch.zeros(self.M, dtype=torch.float64, device=self.dev)
        self.t = 0.0          # host mirror of the clock (plant 0): advanced by the same fp64 additions as the kernel's

    def step(self, ctrl, plan_time, K: int = 1, hold_first: bool = False, record: bool = False):
        """K sim steps of every plant.  ctrl: [T, nu] or [M, T, nu] rows (host array or device tensor), plan_time: scalar or [M].
        hold_first: apply row 0 at every step (sync mode).  record: return the [M, K, 1 + nq + nv + nu] trace (host float32)."""
        torch = self._torch
        c = torch.as_tensor(ctrl, dtype=torch.float32, device=self.dev)
        if c.dim() == 2:
            c = c.unsqueeze(0).expand(self.M, -1, -1)
        c = c.contiguous()
        pt = torch.as_tensor(np.broadcast_to(np.asarray(plan_time, np.float32), (self.M,)).copy(), device=self.dev)
        trace = torch.empty((self.M, int(K), self.width), dtype=torch.float32, device=self.dev) if record else None
        flags = self.flags | (self._hold if hold_first else 0)
        self.ctx.plant_step(self.states, self.t_dev, pt, c, self.ctrl_dt, self.sim_dt, int(K), flags, trace)
        for _ in range(int(K)):
            self.t += self.sim_dt
        return trace.cpu().numpy() if record else None

    def qpos_qvel(self, m: int = 0) -> np.ndarray:
        """[qpos, qvel] of plant m (host float32; synchronises): what the sim publishes to state_shm."""
        return self.states[m, : self.nq + self.nv].cpu().numpy()
