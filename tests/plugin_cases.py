"""The model matrix of the task-plugin tests (tests/test_plugin_matrix.py on the CPU, tests/test_gpu_plugin_matrix.py on the GPU):
every shipped pyramidal model and a few derived ones, each with the probe reward of tests/plugin_probe.hip compiled in.

A case is (the example whose env provides the model, the control and the oracle's built-in task; a transform of the compiled model
dict; yaml overrides).  The plugin context runs a copy of the built-in task with kind = DIAL_TASK_USER: same control law, same
n_frames / dt, the probe's reward.  Physics does not depend on the reward, so the fp32 oracle of the built-in task is the reference.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PROBE = os.path.join(HERE, "plugin_probe.hip")

# probe field codes (plugin_probe.hip)
F = dict(qpos=1, qvel=2, xpos=3, xquat=4, spos=5, cdist=6, cpos=7, ctrl=8, act=9, step=10, dt=11,
         nq=12, nv=13, nu=14, nbody=15, nsite=16, ncon=17, counter=18)
PROBE_BAD = -12345.0


def _efc_rows(m):
    """Constraint rows of a pyramidal model: limits, dry friction, 2 (condim - 1) per contact candidate."""
    return int(m["nlim"]) + int(m.get("nfri", 0)) + int(sum(2 * (int(d) - 1) for d in np.asarray(m["con_dim"]).ravel()))


def keep_contacts(model_dict, keep):
    """The model with only the contact candidates `keep` (indices into the static contact list)."""
    m = dict(model_dict)
    n = int(m["ncon"])
    keep = list(keep)
    for k in list(m):
        if k.startswith("con_") and np.asarray(m[k]).shape[:1] == (n,):
            m[k] = np.asarray(m[k])[keep]
    m["ncon"] = len(keep)
    m["nefc"] = _efc_rows(m)
    return m


def go2_three_contacts(md):
    """The Go2 without the contact candidate of one foot (the existing custom-env test's derived model)."""
    return keep_contacts(md, [0, 1, 2])


def go2_free(md):
    """The Go2 with no contact candidates and no joint limits: ncon = nlim = nefc = 0 (a body falling freely, joints unlimited)."""
    m = keep_contacts(md, [])
    m["nlim"] = 0
    m["lim_jnt"] = np.zeros(0, np.int64)
    m["jnt_limited"] = np.zeros_like(np.asarray(m["jnt_limited"]))
    m["nefc"] = _efc_rows(m)
    return m


def go2_no_sites(md):
    """The Go2 without sites (nsite = 0)."""
    m = dict(md)
    for k in ("site_bodyid", "site_pos", "site_quat"):
        a = np.asarray(m[k])
        m[k] = a[:0]
    m["nsite"] = 0
    return m


# name -> (example, model transform, yaml overrides)
CASES = {
    "go2": ("unitree_go2_trot", None, {}),
    "go2_crate": ("unitree_go2_crate_climb", None, {}),
    "h1_walk": ("unitree_h1_jog", None, {}),
    "h1_loco": ("unitree_h1_loco", None, {}),
    "h1_push_crate": ("unitree_h1_push_crate", None, {}),
    "go2_3con": ("unitree_go2_trot", go2_three_contacts, {}),
    "go2_free": ("unitree_go2_trot", go2_free, {}),
    "go2_nosite": ("unitree_go2_trot", go2_no_sites, {}),
    # the Go2 plugin again (n_frames is task data): 4 physics sub-steps of 0.005 s per 0.02 s control step
    "go2_nf4": ("unitree_go2_trot", None, dict(timestep=0.005, dt=0.02)),
}
# the GPU checks that bear on contacts / the capped workspace run on these
CRATES = ("go2_crate", "h1_push_crate")


def load_case(name, N=16, H=12):
    """(dial_config, env, model dict for the plugin, plugin model struct (DIAL_LS_SWAP), plugin task, oracle task, cfg)."""
    from dial_mpc_amd import _abi
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    from dial_mpc_amd.utils.io_utils import get_example_path
    from conftest import LS_SWAP, with_solver
    example, transform, over = CASES[name]
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    d.update(over)
    d["Nsample"], d["Hsample"] = N, H
    dc, _, env = load_dial_and_env(d)
    md = dict(env.sys.model)
    if transform is not None:
        md = transform(md)
    model = with_solver(_abi.make_model(md), ls_rule=LS_SWAP)
    otask = env.make_task()
    ptask = type(otask).from_buffer_copy(otask)
    ptask.kind = _abi.MACROS["DIAL_TASK_USER"]
    return dict(name=name, dc=dc, env=env, md=md, model=model, ptask=ptask, otask=otask, cfg=make_cfg(dc))


def case_model_dict(name):
    """The compiled model dict of a case (no config or task: enough to build or refuse its plugin)."""
    from dial_mpc_amd.envs.base_env import load_model
    example, transform, over = CASES[name]
    files = {"unitree_go2_trot": ("unitree_go2", "mjx_scene_force.json"),
             "unitree_go2_crate_climb": ("unitree_go2", "mjx_scene_force_crate.json"),
             "unitree_h1_jog": ("unitree_h1", "mjx_scene_h1_walk.json"),
             "unitree_h1_loco": ("unitree_h1", "mjx_scene_h1_loco.json"),
             "unitree_h1_push_crate": ("unitree_h1", "mjx_scene_h1_push_crate.json")}
    md = dict(load_model(*files[example]))
    return md if transform is None else transform(md)


def probe_source():
    return open(PROBE).read()


def build_matrix(names=None, jobs=4):
    """Build (or find in the cache) the probe plugin of every case, at most `jobs` hipcc processes at once -> {name: path}."""
    from dial_mpc_amd.plugin import build_plugin
    names = list(CASES) if names is None else list(names)
    src = probe_source()
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        paths = list(ex.map(lambda n: build_plugin(case_model_dict(n), src), names))
    return dict(zip(names, paths))
