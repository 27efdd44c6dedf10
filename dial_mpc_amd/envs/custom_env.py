"""``CustomEnv`` -- a user environment on the HIP path: the user's model, the user's reward (one HIP device function, the
contract of csrc/user_reward.h) and a vector of float task parameters, compiled into a task plugin for that model
(dial_mpc_amd/plugin.py) the first time the env plans or steps.

A subclass sets
  ``model_path``   an MJCF (compiled by dial_mpc_amd/mjcf.py) or a compiled-model JSON; relative paths are taken from the
                   directory of the module that defines the subclass,
  ``reward_hip``   the reward's HIP source, or the path of a ``.hip`` file (relative as above),
  ``user_params``  names of float fields of its config dataclass; their values, in this order, are the reward's ``params``,
  ``init_keyframe`` the model keyframe env.reset starts from (default "home"),
  ``control_hip``  optional: a control law as HIP source or the path of a ``.hip`` file (the contract of csrc/user_control.h),
  ``make_table()`` optional: a reference table [rows, cols] of data that changes from step to step (a motion clip, a schedule,
                   feed-forward torques); every control step hands the reward and the law one row, picked by the state's step
                   counter -- ``table_row(step, table_row0, rows, table_mode)``.  ``table_mode`` "clamp" (default) or "wrap",
and registers itself with ``dial_mpc_amd.envs.register_environment`` / ``register_config``.  Without ``control_hip`` control is
BaseEnv's (act2joint / act2tau with the config's leg_control, kp, kd, action_scale); the sampling range is the joint range of the
model unless the subclass sets ``self.joint_range``: actuator a's row is the range of the joint IT drives (``actuator_joint_range``;
BaseEnv's ``jnt_range[1:]`` where the first joint is a free base and the actuators follow the joints in order).  A model no task plugin
can serve (implicit damping, elliptic cones, a dof path of more than 12, two actuators on a dof) is refused in ``__init__``
(``plugin.check_model``).  Under ``leg_control: torque`` the PD law reads actuator a's joint as
qpos[7 + a] / qvel[6 + a] (BaseEnv.act2tau): the model must have a free base joint and actuators that drive dofs 6, 7, ... in
order; a model that does not is refused (``torque_joint_convention``).

With ``control_hip`` the law replaces that block in every kernel of the plugin: it returns what each actuator receives, from the
state the control step starts from, the action, the actuators' joint addresses and the task's control constants.  leg_control,
kp and kd then decide nothing by themselves (the law may read kp and kd), the joint convention above is not required, and the
host never restates the law: ``control(state, acts)`` and ``act2tau`` evaluate it on the device.
"""
from __future__ import annotations

import inspect
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from dial_mpc_amd import _abi, mjcf
from dial_mpc_amd.envs.base_env import BaseEnv, BaseEnvConfig, System

TASK_USER = _abi.MACROS["DIAL_TASK_USER"]


def torque_joint_convention(model: Dict[str, Any]) -> None:
    """Raise ValueError unless torque control's joint indexing fits `model`: the PD law of BaseEnv.act2tau (and of every kernel)
    reads actuator a's joint position / velocity at qpos[7 + a] / qvel[6 + a], while the force goes to the actuator's own dof
    (act_qposadr / act_dofadr) -- so the model needs a free base joint first and actuator a on qpos 7 + a, dof 6 + a."""
    nu = int(model["nu"])
    qadr = np.asarray(model["act_qposadr"]).ravel()[:nu]
    dadr = np.asarray(model["act_dofadr"]).ravel()[:nu]
    free = int(model["njnt"]) > 0 and int(np.asarray(model["jnt_type"]).ravel()[0]) == mjcf.JNT_FREE and int(np.asarray(model["jnt_qposadr"]).ravel()[0]) == 0
    bad = [a for a in range(nu) if int(qadr[a]) != 7 + a or int(dadr[a]) != 6 + a]
    if not free or bad:
        what = "joint 0 is not a free base joint" if not free else (
            f"actuator {bad[0]} drives qpos {int(qadr[bad[0]])} / dof {int(dadr[bad[0]])}")
        raise ValueError("leg_control: torque needs actuator a to drive qpos[7 + a] / qvel[6 + a] after a free base joint (the joint "
                         f"indexing of BaseEnv.act2tau); {what}.  Reorder the model's actuators or use leg_control: position")


def actuator_joint_range(model: Dict[str, Any]) -> np.ndarray:
    """[nu, 2]: the range of the joint each actuator drives (slide / hinge joints: the joint whose qpos address is act_qposadr)."""
    qadr = np.asarray(model["jnt_qposadr"]).ravel().tolist()
    rng = np.asarray(model["jnt_range"], dtype=np.float64).reshape(-1, 2)
    return np.array([rng[qadr.index(int(a))] for a in np.asarray(model["act_qposadr"]).ravel()[:int(model["nu"])]]).reshape(-1, 2)


def table_row(step: int, row0: int, rows: int, mode="clamp") -> int:
    """The reference-table row of the control step whose step counter is `step` (the counter BEFORE the step): the host restatement
    of the kernels' rule (csrc/user_reward.h).  r = step + row0; "clamp": min(max(r, 0), rows - 1); "wrap": r modulo rows."""
    from dial_mpc_amd import _lib
    if rows < 1:
        raise ValueError(f"table_row: rows = {rows}; a table has at least one row")
    r = int(step) + int(row0)
    if _lib.table_mode(mode) == _lib.TABLE_MODES["wrap"]:
        return r % rows   # (Python's modulo is the non-negative one)
    return min(max(r, 0), rows - 1)


class CustomEnv(BaseEnv):
    task_kind = TASK_USER
    model_path: str = ""
    reward_hip: str = ""
    control_hip: str = ""
    user_params: Sequence[str] = ()
    init_keyframe: str = "home"
    table_mode: str = "clamp"
    table_row0: int = 0

    def __init__(self, config: BaseEnvConfig):
        if not self.model_path or not self.reward_hip:
            raise TypeError(f"{type(self).__name__}: a CustomEnv subclass sets model_path and reward_hip")
        super().__init__(config)
        from dial_mpc_amd.plugin import check_model
        check_model(self.sys.model)   # what no plugin can serve (implicit damping, elliptic cones, tree shapes) is refused here
        if config.leg_control == "torque" and not self.control_hip:   # (a control law indexes its own joints)
            torque_joint_convention(self.sys.model)
        # BaseEnv takes the joints after the first one, a free base joint, as the actuated ones.  A model whose first joint is
        # not free, or whose actuators skip joints: actuator a's ranges are those of ITS joint (the same rows where BaseEnv's fit)
        self.physical_joint_range = actuator_joint_range(self.sys.model)
        self.joint_range = self.physical_joint_range
        self._init_q = np.asarray(self.sys.model["keyframes"][self.init_keyframe], dtype=np.float64)
        self._plugin = None

    @classmethod
    def _resolve(cls, p: str) -> str:
        if os.path.isabs(p):
            return p
        return os.path.join(os.path.dirname(os.path.abspath(inspect.getfile(cls))), p)

    def make_system(self, config: BaseEnvConfig) -> System:
        path = self._resolve(self.model_path)
        model = mjcf.compile_mjcf(path) if path.endswith(".xml") else mjcf.model_from_json(open(path).read())
        return System(model).tree_replace({"opt.timestep": config.timestep})

    def _source(self, src: str) -> str:
        if "\n" not in src and src.endswith(".hip"):
            return open(self._resolve(src)).read()
        return src

    def reward_source(self) -> str:
        return self._source(self.reward_hip)

    def control_source(self):
        """The control law's HIP source, or None when the env uses BaseEnv's control."""
        return self._source(self.control_hip) if self.control_hip else None

    def user_param_vector(self) -> List[float]:
        return [float(getattr(self._config, name)) for name in self.user_params]

    def task_dict(self) -> Dict[str, Any]:
        return dict(super().task_dict(), nfeet=0)

    def plugin_path(self, plan_models: bool = False, plan_ensemble: bool = False) -> str:
        """Build (or find in the cache) this env's task plugin.  plan_models=True: the plugin that also carries the rollout kernel with
        per-plan / per-sample model constants (build_plugin(plan_models=True); Context.set_plan_models needs it) -- another library,
        the default one stays as it is.  plan_ensemble=True: the plugin that carries the ensemble rollout kernel
        (build_plugin(plan_ensemble=True); Context.set_plan_ensemble needs it), again a library of its own; with both, both kernels."""
        if plan_ensemble:
            cache = getattr(self, "_plan_ens_plugins", None)
            if cache is None:
                cache = self._plan_ens_plugins = {}
            if bool(plan_models) not in cache:
                from dial_mpc_amd.plugin import build_plugin
                extra = dict(plan_models=True) if plan_models else {}
                cache[bool(plan_models)] = build_plugin(self.sys.model, self.reward_source(), control_src=self.control_source(),
                                                        plan_ensemble=True, **extra)
            return cache[bool(plan_models)]
        if plan_models:
            if getattr(self, "_plan_var_plugin", None) is None:
                from dial_mpc_amd.plugin import build_plugin
                self._plan_var_plugin = build_plugin(self.sys.model, self.reward_source(), control_src=self.control_source(), plan_models=True)
            return self._plan_var_plugin
        if self._plugin is None:
            from dial_mpc_amd.plugin import build_plugin
            self._plugin = build_plugin(self.sys.model, self.reward_source(), control_src=self.control_source())
        return self._plugin

    def plant_plugin_path(self, disturbance: bool = False, models: bool = False) -> str:
        """Build (or find in the cache) this env's task plugin WITH the plant simulator's kernel (build_plugin(plant=True)): the plugin
        of make_plant's context.  Another library than plugin_path()'s, which stays as it is.  disturbance=True: the plugin that also
        carries the disturbed plant kernel (build_plugin(plant_disturbance=True)), a third library.  models=True: the plugin that
        carries the plant kernel with per-plant model constants (build_plugin(plant_models=True)), with disturbance=True both."""
        if models:
            cache = getattr(self, "_plant_var_plugins", None)
            if cache is None:
                cache = self._plant_var_plugins = {}
            if bool(disturbance) not in cache:
                from dial_mpc_amd.plugin import build_plugin
                cache[bool(disturbance)] = build_plugin(self.sys.model, self.reward_source(), control_src=self.control_source(),
                                                        plant_disturbance=bool(disturbance), plant_models=True)
            return cache[bool(disturbance)]
        if disturbance:
            if getattr(self, "_plant_dist_plugin", None) is None:
                from dial_mpc_amd.plugin import build_plugin
                self._plant_dist_plugin = build_plugin(self.sys.model, self.reward_source(), control_src=self.control_source(),
                                                       plant_disturbance=True)
            return self._plant_dist_plugin
        if getattr(self, "_plant_plugin", None) is None:
            from dial_mpc_amd.plugin import build_plugin
            self._plant_plugin = build_plugin(self.sys.model, self.reward_source(), control_src=self.control_source(), plant=True)
        return self._plant_plugin

    def make_plant(self, sim_dt: float, device: Optional[int] = None, disturbance: bool = False, models: bool = False):
        """The context of the plant simulator (deploy/plant.py, dial_plant_step) of this env: its model with timestep = sim_dt, its
        task with one physics step per step (n_frames = 1, dt = sim_dt), on the plant-enabled plugin with the env's parameters and
        reference table.  disturbance=True: on the plugin that also carries the disturbed kernel (set_plant_disturbance needs it);
        models=True: on the plugin that carries the per-plant-model kernel (set_plant_models needs it)."""
        from dial_mpc_amd import _lib
        model = self.make_model()
        model.timestep = float(sim_dt)
        task = self.make_task()
        task.n_frames, task.dt = 1, float(sim_dt)
        return _lib.Context(model, task, None, self._device_or(device), **self.context_kwargs(plant=True, disturbance=disturbance, models=models))

    def control(self, state, acts):
        """The control law for T actions from one state, in one launch: acts [T, nu] (or [nu]) -> device tensor [T, nu] of what the
        actuators would receive if env.step ran from `state` with each action -- the law sees the state's qpos / qvel, step counter and
        user info slots.  Needs control_hip."""
        import torch
        if not self.control_hip:
            raise TypeError(f"{type(self).__name__} has no control law (control_hip); use act2joint / act2tau")
        ctx = self._context()
        packed = state.packed if hasattr(state, "packed") else state
        packed = torch.as_tensor(packed, dtype=torch.float32, device=ctx.torch_device)
        acts = torch.as_tensor(acts, dtype=torch.float32, device=ctx.torch_device).reshape(-1, self.sys.nu).contiguous()
        return ctx.user_control(packed.reshape(1, -1).expand(acts.shape[0], -1).contiguous(), acts)

    def act2tau(self, act, pipeline_state):
        """With control_hip: the law on the device from pipeline_state's qpos / qvel, at step 0 and with ZERO user info slots (a
        pipeline_state carries no env info) -> numpy [nu].  A law that reads the step counter or the slots: use control(state, acts)."""
        if not self.control_hip:
            return super().act2tau(act, pipeline_state)
        import torch
        from dial_mpc_amd.envs.base_env import _to_numpy
        ctx = self._context()
        nq, nv = self.sys.nq, self.sys.nv
        packed = np.zeros(ctx.state_size, np.float32)
        packed[:nq] = np.asarray(_to_numpy(pipeline_state.qpos), dtype=np.float32)
        packed[nq:nq + nv] = np.asarray(_to_numpy(pipeline_state.qvel), dtype=np.float32)
        return self.control(torch.as_tensor(packed, device=ctx.torch_device), np.asarray(_to_numpy(act), dtype=np.float32))[0].cpu().numpy()

    def make_table(self) -> Optional[np.ndarray]:
        """The env's reference table [rows, cols <= DIAL_USER_TABLE_COLS] (float), or None (default): no table."""
        return None

    def _table(self) -> Optional[np.ndarray]:
        """The table contexts of this env bind: what set_table gave last, else make_table(); validated, float32."""
        from dial_mpc_amd import _lib
        t = self._table_override if getattr(self, "_table_override", None) is not None else self.make_table()
        return None if t is None else _lib.user_table_array(t)

    def context_kwargs(self, plant: bool = False, disturbance: bool = False, models: bool = False, plan_models: bool = False,
                       plan_ensemble: bool = False) -> Dict[str, Any]:
        """What a _lib.Context of this env needs beyond (model, task, cfg): its plugin (plant=True: the plant-enabled one, with
        disturbance=True the one that also carries the disturbed plant kernel, with models=True the per-plant-model kernel;
        plan_models=True: the planner's plugin with the per-model rollout kernel, Context.set_plan_models needs it;
        plan_ensemble=True: the planner's plugin with the ensemble rollout kernel, Context.set_plan_ensemble needs it), parameters
        and reference table."""
        from dial_mpc_amd import _lib
        plant = plant or disturbance or models
        if plant and plan_models:
            raise ValueError("context_kwargs: plan_models=True is for the planner's context, plant / disturbance / models for the plant's")
        if plant and plan_ensemble:
            raise ValueError("context_kwargs: plan_ensemble=True is for the planner's context, plant / disturbance / models for the plant's")
        if plant:
            path = self.plant_plugin_path(disturbance, models)
        else:
            path = self.plugin_path(plan_models, plan_ensemble=True) if plan_ensemble else self.plugin_path(plan_models)
        kw = dict(plugin=path, user_params=self.user_param_vector())
        table = self._table()
        if table is not None:
            kw.update(user_table=table, table_row0=int(self.table_row0), table_mode=_lib.table_mode(self.table_mode))
        return kw

    def set_table(self, table):
        """Another reference table (None: back to make_table()): contexts created from now on bind it, and this env's own context
        rebinds it now.  Returns the bound device tensor of the env's own context (None before the env has one)."""
        from dial_mpc_amd import _lib
        self._table_override = None if table is None else _lib.user_table_array(table)
        if self._ctx is None:
            return None
        return self._ctx.set_user_table(self._table(), int(self.table_row0), self.table_mode)

    def set_user_params(self, **values) -> None:
        """Change config fields listed in user_params; contexts created from now on, and this env's own, use them."""
        for k, v in values.items():
            if k not in self.user_params:
                raise KeyError(f"{k!r} is not one of {list(self.user_params)}")
            setattr(self._config, k, float(v))
        if self._ctx is not None:
            self._ctx.set_user_params(self.user_param_vector())

    def plan_params(self, **fields) -> np.ndarray:
        """Per-plan task parameters: {name: [M values]} for names in user_params -> rows [M, len(user_params)], ordered as
        user_params (what set_plan_params / step_batch / MBDPI.reverse_once_batch take).  A field not given keeps the config's
        value in every row."""
        if not fields:
            raise ValueError("plan_params: give at least one field as a list of per-plan values")
        cols = {}
        for k, v in fields.items():
            if k not in self.user_params:
                raise KeyError(f"{k!r} is not one of {list(self.user_params)}")
            cols[k] = np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel()
        lens = {k: len(v) for k, v in cols.items()}
        M = next(iter(lens.values()))
        if M < 1 or any(n != M for n in lens.values()):
            raise ValueError(f"plan_params: every field needs the same number (>= 1) of per-plan values; got {lens}")
        base = self.user_param_vector()
        rows = np.tile(np.asarray(base, dtype=np.float32), (M, 1))
        for j, name in enumerate(self.user_params):
            if name in cols:
                rows[:, j] = cols[name]
        return rows

    def step_batch(self, states, actions, user_params=None):
        """env.step of M states in one launch; user_params: per-state task parameters [M, n] (plan_params), state g's reward
        reads row g -- bound for this call only, the shared parameters apply again afterwards."""
        if user_params is None:
            return super().step_batch(states, actions)
        ctx = self._context()
        ctx.set_plan_params(user_params)
        try:
            return super().step_batch(states, actions)
        finally:
            ctx.set_plan_params(None)

    def _context(self):
        if self._ctx is None:
            from dial_mpc_amd import _lib
            self._ctx = _lib.Context(self.make_model(), self.make_task(), None, getattr(self, "_device", None), **self.context_kwargs())
        return self._ctx
