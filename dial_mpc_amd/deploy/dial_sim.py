"""Plant simulator process (``dial-mpc-sim``): the reference's ``DialSim`` (dial_mpc/deploy/dial_sim.py) on the HIP path.

The plant is the env's own compiled scene stepped at ``sim_dt`` by the plant kernel (deploy/plant.py, csrc/plant_kernel.h), not the
full-MuJoCo scene the YAML's ``scene_name`` names (this package does not compile those, and MuJoCo is not a dependency): sim2sim here
exposes the timing, zero-order-hold and latency mismatch between planner and plant, not model mismatch.  No viewer.

Protocol: the six shared-memory segments of dial_plan.py, created here (``open_segments(create=True)``) and unlinked on exit.
Async mode: every sim step applies the row of the published plan that the planner's latency selects (plant.ctrl_row), paced at
sim_dt / real_time_factor of wall time.  Sync mode: after each published plan, the steps up to plan_time + ctrl_dt apply row 0
(plant.sync_steps), in one launch.

``sim_disturbance`` (optional) disturbs the plant, not the planner's model: an actuator gain / bias (a weak or offset motor) and
timed shoves of the base (deploy/plant.py: Plant.shove; csrc/plant_dist_kernel.h).

``sim_model`` (optional) gives the plant another model than the planner's: mjcf.vary_model's arguments -- mass_scale, com_offset,
friction_scale, damping_scale, armature_scale, frictionloss_scale -- applied to the env's compiled scene on the plant side only
(deploy/plant.py: Plant.set_models; csrc/plant_var_kernel.h).  The model's structure and geometry stay the planner's.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import time
from dataclasses import dataclass
from typing import Any, Dict, Optional

import numpy as np

from dial_mpc_amd.deploy.dial_plan import open_segments
from dial_mpc_amd.deploy.plant import Plant, ctrl_row, sync_steps


@dataclass
class DialSimConfig:
    robot_name: str
    scene_name: str
    sim_leg_control: str
    plot: bool
    record: bool
    real_time_factor: float
    sim_dt: float
    sync_mode: bool
    # plant disturbances (sim_disturbance_settings reads it); None: the undisturbed plant
    #   {actuator_gain: float | [nu], actuator_bias: float | [nu], shoves: [{t, duration, dv: [6]}], seed: int, gain_range: [lo, hi]}
    sim_disturbance: Optional[Dict[str, Any]] = None
    # plant-side model mismatch (sim_model_settings reads it); None: the plant runs the planner's model
    #   {mass_scale: float | {body: s}, com_offset: {body: [3]}, friction_scale, damping_scale, armature_scale, frictionloss_scale}
    sim_model: Optional[Dict[str, Any]] = None


_DISTURBANCE_KEYS = ("actuator_gain", "actuator_bias", "shoves", "seed", "gain_range")


def sim_disturbance_settings(block: Dict[str, Any], nu: int):
    """A `sim_disturbance` block -> (gain [nu], bias [nu], shoves [(t, duration, dv6)]).  actuator_gain / actuator_bias: one value
    for every actuator or a list of nu; gain_range: [lo, hi] draws one gain per actuator, uniformly, from numpy's default_rng(seed)
    (seed defaults to 0) and multiplies actuator_gain; shoves: Plant.shove's arguments (dv: the base's total velocity change,
    [vx, vy, vz] world frame in m/s, [wx, wy, wz] body frame in rad/s).  Raises ValueError on unknown keys and bad shapes."""
    if not isinstance(block, dict):
        raise ValueError(f"sim_disturbance is a mapping; got {type(block).__name__}")
    unknown = sorted(set(block) - set(_DISTURBANCE_KEYS))
    if unknown:
        raise ValueError(f"sim_disturbance: unknown keys {unknown}; known: {list(_DISTURBANCE_KEYS)}")

    def per_actuator(key, default):
        a = np.asarray(block.get(key, default), dtype=np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != nu) or not np.isfinite(a).all():
            raise ValueError(f"sim_disturbance.{key}: one finite value or a list of nu = {nu}; got {block.get(key)!r}")
        return np.broadcast_to(a, (nu,)).copy()
    gain, bias = per_actuator("actuator_gain", 1.0), per_actuator("actuator_bias", 0.0)
    if block.get("gain_range") is not None:
        r = np.asarray(block["gain_range"], dtype=np.float64)
        if r.shape != (2,) or not np.isfinite(r).all() or r[0] > r[1]:
            raise ValueError(f"sim_disturbance.gain_range: [lo, hi] with lo <= hi; got {block['gain_range']!r}")
        gain = gain * np.random.default_rng(int(block.get("seed") or 0)).uniform(r[0], r[1], nu)
    shoves = []
    for i, sh in enumerate(block.get("shoves") or []):
        if not isinstance(sh, dict) or set(sh) != {"t", "duration", "dv"} or np.asarray(sh["dv"], dtype=np.float64).shape != (6,):
            raise ValueError(f"sim_disturbance.shoves[{i}]: {{t, duration, dv: [6]}} is needed; got {sh!r}")
        shoves.append((float(sh["t"]), float(sh["duration"]), np.asarray(sh["dv"], dtype=np.float64)))
    return gain, bias, shoves


_MODEL_KEYS = ("mass_scale", "com_offset", "friction_scale", "damping_scale", "armature_scale", "frictionloss_scale")


def sim_model_settings(block: Dict[str, Any], model: Dict[str, Any]) -> Dict[str, Any]:
    """A `sim_model` block -> the plant's model: mjcf.vary_model(model, **block).  Raises ValueError on unknown keys and on whatever
    vary_model refuses (unknown bodies, non-positive scales)."""
    from dial_mpc_amd.mjcf import vary_model
    if not isinstance(block, dict):
        raise ValueError(f"sim_model is a mapping; got {type(block).__name__}")
    unknown = sorted(set(block) - set(_MODEL_KEYS))
    if unknown:
        raise ValueError(f"sim_model: unknown keys {unknown}; known: {list(_MODEL_KEYS)}")
    try:
        return vary_model(model, **{k: v for k, v in block.items() if v is not None})
    except ValueError as e:
        raise ValueError(f"sim_model: {e}") from None


class DialSim:
    def __init__(self, sim_config: DialSimConfig, env_config, dial_config, env, shm_prefix: str = "", device: Optional[int] = None):
        from dial_mpc_amd.utils.io_utils import get_model_path
        self.record = sim_config.record
        self.data = []
        self.ctrl_dt = env_config.dt
        self.real_time_factor = sim_config.real_time_factor
        self.sim_dt = sim_config.sim_dt
        self.n_acts = dial_config.Hsample + 1
        self.sync_mode = sim_config.sync_mode
        self.leg_control = sim_config.sim_leg_control
        if self.leg_control == "law":
            raise ValueError("[dial-mpc-sim] sim_leg_control: law is not supported here: the six shared-memory segments carry joint targets "
                             "(acts_shm) and actuator values (tau_shm), no normalised actions.  Use sim_leg_control: torque -- the planner "
                             "publishes the env's control law as tau_shm -- or step a deploy.plant.Plant(env, sim_dt, 'law') in process")
        if sim_config.plot:
            print("[dial-mpc-sim] plot: true is not supported (no viewer / plots on this path); continuing without")
        scene = get_model_path(sim_config.robot_name, sim_config.scene_name)
        if not os.path.exists(os.path.splitext(scene)[0] + ".json"):
            print(f"[dial-mpc-sim] scene {sim_config.scene_name} is not a compiled scene of this package: simulating the env's own "
                  f"scene ({type(env).__name__}) at sim_dt = {self.sim_dt}")
        model_kw = {}
        if sim_config.sim_model is not None:   # one mismatched model for the one plant (V = 1)
            model_kw = dict(models=[sim_model_settings(sim_config.sim_model, env.sys.model)], model_of=[0])
            print(f"[dial-mpc-sim] plant model mismatch: {sim_config.sim_model}")
        if sim_config.sim_disturbance is None:
            self.plant = Plant(env, self.sim_dt, self.leg_control, M=1, device=device, **model_kw)
        else:
            gain, bias, shoves = sim_disturbance_settings(sim_config.sim_disturbance, int(env.sys.nu))
            self.plant = Plant(env, self.sim_dt, self.leg_control, M=1, device=device, disturbance=dict(gain=gain, bias=bias), **model_kw)
            for t, duration, dv in shoves:
                self.plant.shove(t, duration, dv)
            print(f"[dial-mpc-sim] plant disturbance: actuator gain {np.round(gain, 3).tolist()}, bias {np.round(bias, 3).tolist()}, "
                  f"{len(shoves)} shove(s)")
        self.nq, self.nv, self.nu = self.plant.nq, self.plant.nv, self.plant.nu
        self.default_u = np.zeros(self.nu, np.float32)   # (the compiled scenes' home keyframes carry no ctrl)
        self._seg = open_segments(self.nq, self.nv, self.nu, self.n_acts, create=True, prefix=shm_prefix)
        self.time_shared = self._seg["time_shm"][1]
        self.state_shared = self._seg["state_shm"][1]
        self.acts_shared = self._seg["acts_shm"][1]
        self.refs_shared = self._seg["refs_shm"][1]
        self.plan_time_shared = self._seg["plan_time_shm"][1]
        self.tau_shared = self._seg["tau_shm"][1]
        self.time_shared[0] = 0.0
        self.acts_shared[:] = self.default_u
        self.refs_shared[:] = 0.0
        self.tau_shared[:] = 0.0
        self.plan_time_shared[0] = -self.ctrl_dt
        self.publish()

    @property
    def t(self) -> float:
        return self.plant.t

    def _rows(self):
        return self.acts_shared if self.leg_control == "position" else self.tau_shared

    def publish(self):
        self.state_shared[:] = self.plant.qpos_qvel()
        self.time_shared[:] = self.plant.t

    def _advance(self, plan_time, K: int, hold_first: bool):
        trace = self.plant.step(self._rows().copy(), plan_time, K=K, hold_first=hold_first, record=self.record)
        if self.record:
            self.data.extend(trace[0])
        self.publish()

    def step_async(self) -> bool:
        """One sim step of the async loop (dial_sim.py's else-branch); False while no plan has been published."""
        t0 = time.time()
        plan_time = self.plan_time_shared[0]
        if plan_time < 0.0:
            time.sleep(0.01)
            return False
        delta_time = self.t - float(plan_time)
        if delta_time > self.ctrl_dt / self.real_time_factor:
            print(f"[WARN] Delayed by {delta_time * 1000.0:.1f} ms")
        self._advance(plan_time, 1, hold_first=False)   # (the kernel picks ctrl_row(t, plan_time, ctrl_dt, n_acts) itself)
        duration = time.time() - t0
        if duration < self.sim_dt / self.real_time_factor:
            time.sleep(self.sim_dt / self.real_time_factor - duration)
        else:
            print("[WARN] Sim loop overruns")
        return True

    def step_sync(self, poll: float = 0.0005) -> int:
        """The sync loop's steps for the plan published last (row 0 up to plan_time + ctrl_dt), in one launch; sleeps `poll`
        seconds and returns 0 when there is nothing to do yet."""
        plan_time = self.plan_time_shared[0]
        K = sync_steps(self.t, plan_time, self.ctrl_dt, self.sim_dt)
        if K == 0:
            if poll:
                time.sleep(poll)
            return 0
        self._advance(plan_time, K, hold_first=True)
        return K

    def main_loop(self, duration: Optional[float] = None):
        """Run until `duration` seconds of SIM time have passed (None: forever)."""
        while duration is None or self.t < duration - 0.5 * self.sim_dt:
            if self.sync_mode:
                self.step_sync()
            else:
                self.step_async()

    def save_record(self, output_dir: str) -> Optional[str]:
        if not self.record:
            return None
        os.makedirs(output_dir)
        path = os.path.join(output_dir, "states.npy")
        np.save(path, np.array(self.data, dtype=np.float32).reshape(-1, self.plant.width))
        return path

    def close(self):
        for shm, _ in self._seg.values():
            shm.close()
            try:
                shm.unlink()
            except FileNotFoundError:   # (an attached process's resource tracker may have removed it already)
                pass


def main(args=None):
    import yaml
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.examples import deploy_examples
    from dial_mpc_amd.utils.io_utils import get_example_path, load_dataclass_from_dict
    parser = argparse.ArgumentParser()
    group = parser.add_mutually_exclusive_group(required=True)
    group.add_argument("--config", type=str, default=None, help="Path to config file")
    group.add_argument("--example", type=str, default=None, help="Example to run")
    group.add_argument("--list-examples", action="store_true", help="List available examples")
    parser.add_argument("--custom-env", type=str, default=None, help="Custom environment to import dynamically")
    parser.add_argument("--shm-prefix", type=str, default="", help="Prefix of the shared-memory segment names")
    parser.add_argument("--duration", type=float, default=None, help="Seconds of simulated time to run (default: forever)")
    args = parser.parse_args(args)
    if args.custom_env is not None:
        sys.path.append(os.getcwd())
        importlib.import_module(args.custom_env)
    if args.list_examples:
        print("Available examples:")
        for example in deploy_examples:
            print(f"  - {example}")
        return 0
    if args.example is not None:
        if args.example not in deploy_examples:
            print(f"Example {args.example} not found.")
            return 1
        config_dict = yaml.safe_load(open(get_example_path(args.example + ".yaml"), "r"))
    else:
        config_dict = yaml.safe_load(open(args.config, "r"))
    sim_config = load_dataclass_from_dict(DialSimConfig, config_dict)
    dial_config, env_config, env = load_dial_and_env(config_dict)
    sim = DialSim(sim_config, env_config, dial_config, env, shm_prefix=args.shm_prefix)
    try:
        sim.main_loop(args.duration)
    except KeyboardInterrupt:
        pass
    finally:
        if sim.record:
            timestamp = time.strftime("%Y%m%d-%H%M%S")
            out = sim.save_record(os.path.join(dial_config.output_dir, f"sim_{dial_config.env_name}_{env_config.task_name}_{timestamp}"))
            print(f"[dial-mpc-sim] record: {out}")
        sim.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
