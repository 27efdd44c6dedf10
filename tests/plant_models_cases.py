"""Shared pieces of the plant-model tests (tests/test_plant_models_host.py on the CPU, tests/test_gpu_plant_models.py on the GPU):
the variant set of every case, the shapes, rows, clocks and start states of tests/test_gpu_plant_dist.py restated (M = 8 plants, K = 4
steps at sim_dt = 0.005) with 0.3 m/s of lateral base velocity added so that friction acts, the fp32 oracle's check that every
non-identity variant moves the plant, and the Go2 probe plugin built WITH the per-plant-model plant kernel
(build_plugin(plant_models=True): csrc/plant_var_kernel.h behind the sixth table)."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from plant_plugin_cases import law_source
from plugin_cases import case_model_dict, probe_source

VAR_SYMBOL = "dial_plugin_plant_var_v1"
SIM_DT, CTRL_DT, T, R = 0.005, 0.02, 17, 64.0
M, K = 8, 4
MODEL_OF = [0, 1, 2, 3, 3, 2, 1, 0]
EXAMPLES = ["unitree_go2_trot", "unitree_h1_jog", "unitree_h1_loco", "allegro_reorient", "unitree_go2_crate_climb", "unitree_h1_push_crate"]


def variant_args(example):
    """The four variants of a case, as mjcf.vary_model's arguments: identity; the first moving body (the trunk, the pelvis, the
    Allegro's cube) 1.3 times as dense with its centre of mass 0.02 m forward; half the sliding friction; twice the damping with 1.5
    times the armature.  The Allegro's start states have no sliding contact within K steps (the fp32 oracle's plants with half the
    friction equal the identity's bit for bit), so its third variant is another change of floats that does matter: two distal finger
    links half as dense."""
    third = dict(mass_scale={"ff_distal": 0.5, "th_distal": 0.5}) if example == "allegro_reorient" else dict(friction_scale=0.5)
    return [dict(),
            dict(mass_scale={1: 1.3}, com_offset={1: [0.02, 0.0, 0.0]}),
            third,
            dict(damping_scale=2.0, armature_scale=1.5)]


def variants(model_dict, example):
    from dial_mpc_amd.mjcf import vary_model
    return [vary_model(model_dict, **kw) for kw in variant_args(example)]


def variant_struct(model, md):
    """The DialModel of a variant dict with the non-physical settings of the case's struct `model` (timestep = sim_dt, the line-search
    rule the case selected): what the reference context and the binding both get."""
    from dial_mpc_amd import _abi
    st = _abi.make_model(md)
    st.timestep = model.timestep
    st.ls_rule, st.iterations, st.ls_iterations = model.ls_rule, model.iterations, model.ls_iterations
    return st


def act_q(model):
    return [int(model.act_qposadr[a]) for a in range(model.nu)]


def free_joint_dof(model):
    """First dof of the model's first free joint (the base, the Allegro's cube)."""
    for j in range(model.njnt):
        if model.jnt_type[j] == 0:
            return int(model.jnt_dofadr[j])
    raise AssertionError("the case has no free joint")


def start_qpos_qvel(model, env, seed):
    """tests/test_gpu_plant_dist.py's start states (the env's initial pose plus seeded perturbations of the actuated joints and of every
    velocity; plant 0: the pose itself) with 0.3 m/s added to the free body's lateral (y) velocity, plant 0 included."""
    rng = np.random.default_rng(seed)
    qpos = np.tile(np.asarray(env._init_q, np.float32), (M, 1))
    qvel = np.zeros((M, model.nv), np.float32)
    qpos[1:, act_q(model)] += rng.uniform(-0.1, 0.1, (M - 1, model.nu)).astype(np.float32)
    qvel[1:] = rng.uniform(-0.3, 0.3, (M - 1, model.nv)).astype(np.float32)
    qvel[:, free_joint_dof(model) + 1] += np.float32(0.3)
    return qpos, qvel


def rows(model, env, target, seed):
    """[M, T, nu] dyadic rows: torques k / 8, or -- target -- joint targets near the initial pose on a 1/256 grid."""
    rng = np.random.default_rng(seed)
    if target:
        base = np.round(np.asarray(env._init_q, np.float64)[act_q(model)] * 256) / 256
        return (base + rng.integers(-64, 65, (M, T, model.nu)) / 256).astype(np.float32)
    return (rng.integers(-160, 161, (M, T, model.nu)) / 8).astype(np.float32)


def clocks():
    t = np.array([0.005 * (m % 9) + 0.3 for m in range(M)])
    plan_time = np.float32(t - 0.003 * (np.arange(M) % 11) - 0.02 * (np.arange(M) % 3))
    return t, plan_time


def positional(model):
    return any(model.act_isposition[a] for a in range(model.nu))


def oracle_final_states(example, seed=3):
    """The fp32 oracle's [V, M, nq + nv] after K plant steps in DIAL_PLANT_CTRL mode: every variant from every start state, the rows
    picked by ctrl_row on the host clock -- tests/test_gpu_plant.py's mapping (joint_range = phys_range = [-R, R], so that
    act2joint(c / R) = c for dyadic c)."""
    import oracle as O
    from conftest import setup_case
    from dial_mpc_amd.deploy.plant import ctrl_row
    _, env, model, task, _ = setup_case(example, 8, 4, per_rollout=True)
    model.timestep = SIM_DT
    task.n_frames, task.dt = 1, SIM_DT
    task.position_control, task.action_scale = 1, 1.0
    for a in range(model.nu):
        task.joint_offset[a] = 0.0
        task.joint_range[a][0], task.joint_range[a][1] = -R, R
        task.phys_range[a][0], task.phys_range[a][1] = -R, R
    qpos, qvel = start_qpos_qvel(model, env, seed)
    rws = rows(model, env, positional(model), seed + 1)
    t, plan_time = clocks()
    out = []
    for md in variants(env.sys.model, example):
        o32 = O.Oracle(variant_struct(model, md), task, None, np.float32)
        fin = []
        for m in range(M):
            tm, ks = t[m], []
            for _ in range(K):
                ks.append(ctrl_row(tm, plan_time[m], CTRL_DT, T))
                tm += SIM_DT
            _, qs, qds, _ = o32.rollout(o32.env_reset(qpos[m], qvel[m])[0], (rws[m, ks] / np.float32(R))[None])
            fin.append(np.concatenate([qs[0, -1], qds[0, -1]]))
        out.append(np.stack(fin))
    return np.stack(out)


def build_var_plugin(model="go2", law=None, disturbance=False):
    """The probe plugin of a model of plugin_cases.CASES with the per-plant-model plant kernel (found in the cache after the first build)."""
    from dial_mpc_amd.plugin import build_plugin
    return build_plugin(case_model_dict(model), probe_source(), control_src=law_source(law), plant_models=True, plant_disturbance=disturbance)


def build_var_plugins(variants_=(("go2", None), ("go2", "probe"))):
    variants_ = list(variants_)
    with ThreadPoolExecutor(max_workers=2) as ex:
        paths = list(ex.map(lambda v: build_var_plugin(*v), variants_))
    return dict(zip(variants_, paths))
