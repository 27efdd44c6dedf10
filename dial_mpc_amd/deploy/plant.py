"""The plant of ``dial-mpc-sim`` on the HIP path: the env's own compiled scene stepped at ``sim_dt`` by the plant kernel
(csrc/plant_kernel.h, ``dial_plant_step``), with the reference's rules for which row of the published plan each step applies
(dial_mpc/deploy/dial_sim.py).

``ctrl_row`` and ``sync_steps`` restate those rules on the host in fp64; the kernel picks its rows with the same arithmetic and the
GPU tests compare the two bit for bit.

Plant disturbances (``dial_set_plant_disturbance``, csrc/plant_dist_kernel.h): per plant, timed velocity kicks and an actuator
gain / bias.  ``event_fires`` restates the kernel's window test, ``disturbance_row`` packs one plant's row, and ``Plant`` binds
them (``Plant(..., disturbance=)``, ``set_disturbance``, ``shove``).  A kick's ``dv`` is in generalised velocity coordinates and
the model's units: behind a free base joint dofs 0-2 are the base's linear velocity in the WORLD frame (m/s), dofs 3-5 its angular
velocity in the BODY frame (rad/s), the rest joint rates.

Model mismatch (``dial_set_plant_models``, csrc/plant_var_kernel.h): per plant, another set of model constants -- masses, inertias,
centres of mass, sliding friction, damping, armature, friction loss (``mjcf.vary_model`` makes such variants and recomputes what
derives from them).  ``Plant(..., models=[...], model_of=[...])`` / ``set_models`` bind V variants and the index that picks one per
plant; the planner's model is untouched.  Kicks and actuator errors combine with it.  Still the planner's: the structure of the
model (bodies, joints, the contact list) and its geometry (geom sizes and positions) -- a payload body or another foot radius is
another compiled scene.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from dial_mpc_amd import _abi


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


MAX_EVENTS = _abi.MACROS["DIAL_PLANT_MAX_EVENTS"]   # event slots of one plant's row (include/dial_mpc.h: 16)


def event_fires(t: float, t0, t1) -> bool:
    """The disturbed kernel's window test: the event with the float32 bounds t0, t1 fires at the sim step whose clock BEFORE the
    step is t (fp64) when t >= (double)t0 and t < (double)t1.  t1 <= t0 (the all-zero slot) and NaN never fire."""
    t, a, b = float(t), float(np.float32(t0)), float(np.float32(t1))
    return bool(t >= a and t < b)


def disturbance_row(nu: int, nv: int, gain=None, bias=None, events=None) -> np.ndarray:
    """One plant's disturbance row as dial_set_plant_disturbance takes it: float32 [2 nu + E (2 + nv)] =
    gain[nu] | bias[nu] | E x { t0, t1, dv[nv] }.  gain / bias: a scalar or [nu] (None: 1 / 0, the perfect actuator); events: a
    list of (t0, t1, dv[nv]), applied in this order, E = len(events) <= 16 (pad with (0, 0, zeros) for a common E: that slot
    never fires).  Raises ValueError on non-finite values, other shapes or more than 16 events."""
    nu, nv = int(nu), int(nv)
    events = [] if events is None else list(events)
    if len(events) > MAX_EVENTS:
        raise ValueError(f"{len(events)} events; a plant's disturbance row holds at most DIAL_PLANT_MAX_EVENTS = {MAX_EVENTS}")

    def per_actuator(x, default, what):
        a = np.asarray(default if x is None else x, dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != nu):
            raise ValueError(f"actuator {what}: a scalar or [nu = {nu}] values; got shape {a.shape}")
        a = np.broadcast_to(a, (nu,)).astype(np.float32)
        if not np.isfinite(a).all():
            raise ValueError(f"actuator {what}: non-finite value")
        return a
    row = np.zeros(2 * nu + len(events) * (2 + nv), np.float32)
    row[:nu] = per_actuator(gain, 1.0, "gain")
    row[nu:2 * nu] = per_actuator(bias, 0.0, "bias")
    for e, ev in enumerate(events):
        if len(ev) != 3:
            raise ValueError(f"event {e}: (t0, t1, dv[nv]) is needed; got {len(ev)} items")
        t0, t1, dv = ev
        dv = np.asarray(dv, dtype=np.float64)
        if dv.shape != (nv,):
            raise ValueError(f"event {e}: dv has shape {dv.shape}; [nv = {nv}] generalised velocities are needed")
        slot = np.concatenate([[float(t0), float(t1)], dv]).astype(np.float32)
        if not np.isfinite(slot).all():
            raise ValueError(f"event {e}: non-finite window or dv")
        o = 2 * nu + e * (2 + nv)
        row[o:o + 2 + nv] = slot
    return row


class Plant:
    """M copies of an env's plant, stepped on the GPU.  ``leg_control``: "torque" -- the rows are the actuators' ctrl as they are
    (DIAL_PLANT_CTRL, dial_sim.py's ``data.ctrl = tau_shared[k]``); "position" -- the rows are joint targets, turned into torques by
    the env's PD law at every sim step (DIAL_PLANT_PD), or, on models whose actuators are position actuators (the Allegro), handed to
    them as their ctrl (DIAL_PLANT_CTRL).  A custom environment (envs/custom_env.py) is stepped by the plant kernel of its own task
    plugin (csrc/plant_kernel.h at the model's dimensions, behind csrc/plant_plugin.h's table); "position" there needs the PD law's
    joint indexing (torque_joint_convention), and an env with a
    control law (control_hip) has a third mode, "law": the rows are normalised actions and the law runs at every sim step from the
    plant's current state (DIAL_PLANT_LAW; law_step is the step counter it sees)."""

    def __init__(self, env, sim_dt: float, leg_control: str = "torque", M: int = 1, device: Optional[int] = None, disturbance=None,
                 models=None, model_of=None):
        """disturbance: None (the undisturbed plant, the context and kernels as they were), True (a context that can take
        disturbances: set_disturbance / shove later) or a dict of set_disturbance's arguments (gain, bias, events), bound at once.
        models: None (every plant runs the env's own model), True (a context that can take per-plant models: set_models later; only a
        custom environment needs to know in advance, it picks another plugin) or a list of model dicts with model_of, bound at once
        (set_models' arguments)."""
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
        self._dist_capable = disturbance is not None and disturbance is not False
        self._models_capable = (models is not None and models is not False) or not custom
        kw = dict(disturbance=True) if self._dist_capable else {}
        if models is not None and models is not False:
            kw["models"] = True
        self.ctx = env.make_plant(self.sim_dt, device=device, **kw)
        self.nq, self.nv, self.nu = self.ctx.nq, self.ctx.nv, self.ctx.nu
        self.width = 1 + self.nq + self.nv + self.nu          # trace / record row: [t, qpos, qvel, ctrl]
        self.dev = self.ctx.torch_device
        self._torch = torch
        self._gain = self._bias = None       # [M, nu] float32, or None: 1 / 0
        self._events = [[] for _ in range(self.M)]   # per plant: (t0, t1, dv[nv]) in firing order
        self._dist = None                    # the bound device tensor
        self.reset()
        if isinstance(disturbance, dict):
            self.set_disturbance(**disturbance)
        self.model_of = None                 # int32 [M] while plant models are bound
        if models is not None and models is not False and models is not True:
            self.set_models(models, model_of)

    # ---- model mismatch (dial_set_plant_models)
    def set_models(self, models, model_of=None):
        """Bind per-plant models: `models` a list of V compiled model dicts (mjcf.vary_model(env.sys.model, ...)), `model_of` [M]
        indices into it (None: V == M, plant b runs model b).  Each dict gets timestep = sim_dt, as make_plant gives the env's own
        model.  models None unbinds: every plant runs the env's model again.  reset() keeps the binding.  Returns the index bound."""
        if models is None:
            self.ctx.set_plant_models(None)
            self.model_of = None
            return None
        if not self._models_capable:
            raise ValueError("this Plant of a custom environment was created without per-plant models: pass models=True (or the list) to Plant")
        from dial_mpc_amd import _lib
        models = list(models)
        index = _lib.plant_model_index(model_of, len(models), self.M)
        structs = []
        for m in models:
            st = _abi.make_model(m)
            st.timestep = float(self.sim_dt)
            structs.append(st)
        self.model_of = self.ctx.set_plant_models(structs, index)
        return self.model_of

    # ---- disturbances (dial_set_plant_disturbance)
    def _per_plant(self, x, what):
        a = np.asarray(x, dtype=np.float64)
        if a.ndim > 2 or (a.ndim >= 1 and a.shape[-1] != self.nu) or (a.ndim == 2 and a.shape[0] != self.M):
            raise ValueError(f"actuator {what}: a scalar, [nu = {self.nu}] or [M = {self.M}, nu] values; got shape {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"actuator {what}: non-finite value")
        return np.broadcast_to(a, (self.M, self.nu)).astype(np.float32)

    def set_disturbance(self, gain=None, bias=None, events=None):
        """Replace the plants' disturbances and bind them.  gain / bias: a scalar, [nu] (every plant) or [M, nu]; None: 1 / 0.
        events: a list of (plant or None, t0, t1, dv[nv]) -- plant None: every plant -- fired in list order, at most 16 per plant
        (see disturbance_row; the windows are on the plant's own clock, which reset() sets to 0).  All three None: unbind, the
        undisturbed kernel runs again.  Needs Plant(..., disturbance=True or a dict)."""
        if not self._dist_capable:
            raise ValueError("this Plant was created without disturbances: pass disturbance=True (or a dict of gain / bias / events) to Plant")
        if gain is None and bias is None and events is None:
            self._gain = self._bias = None
            self._events = [[] for _ in range(self.M)]
            self._dist = self.ctx.set_plant_disturbance(None)
            return None
        self._gain = None if gain is None else self._per_plant(gain, "gain")
        self._bias = None if bias is None else self._per_plant(bias, "bias")
        per = [[] for _ in range(self.M)]
        for ev in (events or []):
            if len(ev) != 4:
                raise ValueError(f"an event is (plant or None, t0, t1, dv[nv]); got {len(ev)} items")
            m, t0, t1, dv = ev
            if m is not None and not 0 <= int(m) < self.M:
                raise ValueError(f"event for plant {m}; this Plant has M = {self.M}")
            for k in (range(self.M) if m is None else [int(m)]):
                per[k].append((t0, t1, dv))
        self._events = per
        return self._bind()

    def _bind(self):
        E = max(len(p) for p in self._events)
        pad = (0.0, 0.0, np.zeros(self.nv))   # (t1 <= t0: never fires)
        rows = np.stack([disturbance_row(self.nu, self.nv, None if self._gain is None else self._gain[m],
                                         None if self._bias is None else self._bias[m], self._events[m] + [pad] * (E - len(self._events[m])))
                         for m in range(self.M)])
        self._dist = self.ctx.set_plant_disturbance(self._torch.as_tensor(rows, device=self.dev), E)
        return self._dist

    def shove(self, t: float, duration: float, dvel6, plant: Optional[int] = None):
        """Shove the base: over the sim steps whose clocks lie in [t, t + duration) the base's velocity changes by dvel6 IN ALL --
        [vx, vy, vz] in the world frame (m/s), [wx, wy, wz] in the body frame (rad/s) -- in n = max(1, round(duration / sim_dt))
        equal per-step increments dvel6 / n (float32), as one more event of `plant` (None: every plant) after those already there.
        The window is [t - sim_dt / 2, t - sim_dt / 2 + n sim_dt): accumulated clocks land next to multiples of sim_dt on either
        side, and the half step keeps exactly n of them inside.  Needs a free base joint.  Returns (t0, t1, dv) as bound."""
        m = self.env.sys.model
        if not (int(m["njnt"]) > 0 and int(np.asarray(m["jnt_type"]).ravel()[0]) == 0 and self.nv >= 6):
            raise ValueError("shove needs a free base joint (dofs 0-5 of the model): this model has none; use set_disturbance(events=) "
                             "with a dv in the model's own coordinates")
        d6 = np.asarray(dvel6, dtype=np.float64)
        if d6.shape != (6,) or not np.isfinite(d6).all():
            raise ValueError(f"shove: dvel6 is [vx, vy, vz, wx, wy, wz], finite; got shape {d6.shape}")
        if not (math.isfinite(t) and math.isfinite(duration) and duration >= 0.0):
            raise ValueError("shove: t and duration must be finite, duration >= 0")
        n = max(1, int(round(float(duration) / self.sim_dt)))
        dv = np.zeros(self.nv)
        dv[:6] = d6 / n
        t0 = float(t) - 0.5 * self.sim_dt
        ev = (t0, t0 + n * self.sim_dt, dv)
        if not self._dist_capable:
            raise ValueError("this Plant was created without disturbances: pass disturbance=True to Plant")
        if plant is not None and not 0 <= int(plant) < self.M:
            raise ValueError(f"shove of plant {plant}; this Plant has M = {self.M}")
        for k in (range(self.M) if plant is None else [int(plant)]):
            if len(self._events[k]) >= MAX_EVENTS:
                raise ValueError(f"plant {k} already has {MAX_EVENTS} events (DIAL_PLANT_MAX_EVENTS)")
            self._events[k].append(ev)
        self._bind()
        return (np.float32(ev[0]), np.float32(ev[1]), dv.astype(np.float32))

    def reset(self):
        """Every plant at the env's initial pose (the home keyframe; env.reset's), zero velocity, t = 0.  A bound disturbance stays
        bound (its windows are on the clock that starts again at 0), and so do bound plant models."""
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
