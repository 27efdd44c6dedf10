"""Shared pieces of the planner-model tests (tests/test_plan_models_host.py on the CPU, tests/test_gpu_plan_models.py on the GPU): the
shapes (N = 8 samples, H = 4, M = 3 plans), the two indices, the variants of every case (tests/plant_models_cases.py's), the start
states (the plant-model tests': the env's initial pose plus seeded perturbations and 0.3 m/s of lateral base velocity, so that friction
acts), the controls of the given-controls launches, the fp32 oracle's check that every non-identity variant changes a reward from
them, and the Go2 probe plugin built WITH the per-model rollout kernel (build_plugin(plan_models=True): csrc/plan_var_kernel.h behind
the seventh table)."""
from __future__ import annotations

import numpy as np

import plant_models_cases as PM
from plugin_cases import case_model_dict, probe_source

PLAN_VAR_SYMBOL = "dial_plugin_plan_var_v1"
N, H, M = 8, 4, 3
PER_PLAN = [2, 0, 3]
PER_SAMPLE = [0, 1, 2, 3, 3, 2, 1, 0, 1]   # N + 1 rows, the mean trajectory's last
EXAMPLES = PM.EXAMPLES
STATE_SEED, US_SEED = 3, 7


def load(example):
    """(dial_config, env, model struct (DIAL_LS_SWAP where the cone allows), task, cfg, model dict) of an example at N = 8, H = 4."""
    from conftest import setup_case
    dc, env, model, task, cfg = setup_case(example, N, H, per_rollout=True)
    return dc, env, model, task, cfg, env.sys.model


def structs(model, md, example):
    """The V = 4 variants as DialModel structs with the case's timestep and solver settings."""
    return [PM.variant_struct(model, v) for v in PM.variants(md, example)]


def start(model, env):
    """qpos [M, nq], qvel [M, nv] of the M plans; one-plan launches start from row 1 (a perturbed pose)."""
    qpos, qvel = PM.start_qpos_qvel(model, env, STATE_SEED)
    return qpos[:M], qvel[:M]


def controls(model):
    """[N + 1, T, nu] normalised actions of the given-controls launches (dial_rollout)."""
    return np.random.default_rng(US_SEED).uniform(-0.6, 0.6, (N + 1, H + 1, model.nu)).astype(np.float32)


def oracle_rewards(example):
    """The fp32 oracle's [V, N + 1, T] step rewards: every variant from the one-plan start state under `controls`."""
    import oracle as O
    _, env, model, task, _, md = load(example)
    qpos, qvel = start(model, env)
    us = controls(model)
    out = []
    for st in structs(model, md, example):
        o32 = O.Oracle(st, task, None, np.float32)
        out.append(o32.rollout(o32.env_reset(qpos[1], qvel[1])[0], us)[0])
    return np.stack(out)


def build_plan_plugin(model="go2", **kw):
    """The probe plugin of a model of plugin_cases.CASES with the per-model rollout kernel (found in the cache after the first build)."""
    from dial_mpc_amd.plugin import build_plugin
    return build_plugin(case_model_dict(model), probe_source(), plan_models=True, **kw)
