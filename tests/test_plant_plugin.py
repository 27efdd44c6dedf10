"""The plant simulator of custom environments without a GPU: a task plugin built with plant=True cross-compiles with exactly one more
kernel (plant_kernel at the plugin's Dims: the kernel of the built-in families, csrc/plant_kernel.h) and a fourth table, with and
without a control law; a plugin built without the flag stays as it was; the
Python surface (the DIAL_PLANT_LAW flag, deploy.plant.law_step, Plant's argument errors that need no device)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from plant_plugin_cases import MODELS, build_plant_plugins, law_step_loop
from plugin_cases import build_matrix
from test_custom_env import LLVM, ROOT, _disasm

PLANT_SYMBOL = "dial_plugin_plant_v1"


@pytest.fixture(scope="module")
def plugins():
    return build_plant_plugins()   # (five builds, four at a time; the GPU suite finds them in the cache)


def _dyn_syms(so):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], stdout=subprocess.PIPE, text=True).stdout


def _exports(syms, name):
    return re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+" + name + "$", syms, flags=re.M) is not None


def _kernel_names(so, outdir):
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    import disasm_lib
    cos = disasm_lib.code_objects(so, outdir)
    return cos, [k["name"] for co in cos for k in disasm_lib.kernel_notes(co)]


@pytest.mark.parametrize("law", [None, "probe"], ids=["no-law", "law"])
@pytest.mark.parametrize("model", MODELS)
def test_plant_plugin_has_one_more_kernel_and_the_fourth_table(plugins, model, law, tmp_path):
    from dial_mpc_amd import plugin
    assert plugin.PLANT_SYMBOL == PLANT_SYMBOL
    so = plugins[(model, law)]
    syms = _dyn_syms(so)
    assert _exports(syms, "dial_plugin_ops_v1") and _exports(syms, "dial_plugin_table_v1") and _exports(syms, PLANT_SYMBOL), syms
    assert _exports(syms, "dial_plugin_ctrl_v1") == (law is not None)
    cos, names = _kernel_names(so, str(tmp_path))
    assert len(cos) == 1
    count = lambda k: sum(k + "I8DimsUser" in n for n in names)   # noqa: E731
    assert count("rollout_kernel") == 3 and count("env_step_kernel") == 1 and count("env_reset_kernel") == 1, names
    assert count("plant_kernel") == 1 and count("user_control_kernel") == (1 if law else 0), names
    assert not any("plant_user_kernel" in n for n in names), names   # (one plant kernel: no copy of it under a name of the plugin's)
    assert len(names) == len(set(names)) == (7 if law else 6), names
    h = ctypes.CDLL(so, mode=ctypes.RTLD_LOCAL)
    entry = getattr(h, PLANT_SYMBOL)
    entry.restype = ctypes.POINTER(ctypes.c_int)
    assert entry()[0] == 1   # (version: the table's first field)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), _disasm(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_default_plugin_is_unchanged(plugins, tmp_path):
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin, plugin_key
    from plugin_cases import case_model_dict, probe_source
    so = build_matrix(["go2"])["go2"]
    assert so != plugins[("go2", None)] and so == build_plugin(case_model_dict("go2"), probe_source(), plant=False)
    syms = _dyn_syms(so)
    assert _exports(syms, "dial_plugin_ops_v1") and "dial_plugin_plant" not in syms
    cos, names = _kernel_names(so, str(tmp_path))
    assert len(cos) == 1 and len(names) == 5 and not any("plant" in n for n in names), names
    # the flag is part of the cache key, and of nothing else: the key of a default plugin is the key of its flags as they were
    md, rew, flags = case_model_dict("go2"), probe_source(), list(_COMMON + _FAST)
    assert os.path.basename(os.path.dirname(so)) == plugin_key(md, rew, flags)[:24]
    assert os.path.basename(os.path.dirname(plugins[("go2", None)])) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1"])[:24]


def test_plant_law_flag_and_header():
    from dial_mpc_amd import _abi, _lib
    assert _abi.MACROS["DIAL_PLANT_LAW"] == _lib.PLANT_LAW == 8
    flags = [_lib.PLANT_CTRL, _lib.PLANT_PD, _lib.PLANT_HOLD_FIRST, _lib.PLANT_LAW]
    assert flags == [1, 2, 4, 8]
    text = open(os.path.join(ROOT, "dial_mpc_amd", "csrc", "plant_plugin.h")).read()
    assert re.search(r"#ifndef DIAL_PLUGIN_PLANT_VERSION[^\n]*\n#define DIAL_PLUGIN_PLANT_VERSION 1\n#endif", text)
    assert '#define DIAL_PLUGIN_PLANT_SYMBOL "' + PLANT_SYMBOL + '"' in text


def test_law_step_agrees_with_a_loop_restatement():
    """law_step(t, ctrl_dt) = trunc(t / ctrl_dt) in fp64, 0 for negative clocks and NaN, at most 2^24: against a search over the
    integers, on clocks accumulated by 0.005 (their quotients by 0.02 sit next to integers, on either side), just below / above
    multiples, negative, NaN, infinite and past the cap."""
    from dial_mpc_amd.deploy.plant import law_step
    ts, t = [], 0.0
    for _ in range(4000):
        ts.append(t)
        t += 0.005
    below = above = 0
    for t in ts:
        for dt in (0.02, 0.005, 0.0125):
            n = law_step(t, dt)
            assert isinstance(n, int) and n == law_step_loop(t, dt), (t, dt, n)
        n, exact = law_step(t, 0.02), round(t / 0.02)
        if abs(t / 0.02 - exact) < 1e-9 and exact > 0:
            below += n == exact - 1
            above += n == exact
    assert below > 0 and above > 0, (below, above)   # the accumulated clocks do land on both sides of an integer quotient
    for t in (-0.0, -1e-300, -0.005, -7.3, float("nan"), -float("inf")):
        assert law_step(t, 0.02) == law_step_loop(t, 0.02) == 0, t
    for t in (np.nextafter(0.04, 0.0), 0.04, np.nextafter(0.04, 1.0), 1e-320):
        assert law_step(t, 0.02) == law_step_loop(t, 0.02), t
    cap = 1 << 24
    assert law_step(cap * 0.02, 0.02) == cap and law_step(1e30, 0.02) == cap and law_step(float("inf"), 0.02) == cap
    assert law_step((cap - 1) * 0.5, 0.5) == cap - 1 == law_step_loop((cap - 1) * 0.5, 0.5)
    assert law_step(np.float32(0.3), np.float64(0.02)) == int(float(np.float32(0.3)) / 0.02)
    assert not math.isnan(law_step(float("nan"), 0.02))


def _example_env(name):
    import importlib
    import yaml
    import dial_mpc_amd.envs as dial_envs
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    mod = "dial_mpc_amd.examples.custom_env." + name
    for dep in ("dial_mpc_amd.examples.custom_env.go2_height_walk", mod):   # (registered again: an earlier module's teardown removed it)
        importlib.reload(sys.modules[dep]) if dep in sys.modules else importlib.import_module(dep)
    try:
        d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", name + "_deploy.yaml")))
        return d, load_dial_and_env(d)
    finally:
        dial_envs._envs.clear()
        dial_envs._envs.update(saved[0])
        dial_envs._configs.clear()
        dial_envs._configs.update(saved[1])


def test_plant_argument_errors_without_a_device():
    """Plant refuses, before it creates anything on a device: an unknown mode, "law" for an env without a control law (built-in or
    custom), "position" for a custom env whose actuators do not follow the PD law's joint indexing."""
    from conftest import setup_case
    from control_cases import permuted_go2_env
    from dial_mpc_amd.deploy.plant import Plant
    _, builtin, _, _, _ = setup_case("unitree_go2_trot", 8, 4)
    with pytest.raises(ValueError, match="'torque', 'position' or 'law'"):
        Plant(builtin, 0.005, "velocity")
    with pytest.raises(ValueError, match="control law"):
        Plant(builtin, 0.005, "law")
    _, (_, _, walk) = _example_env("go2_height_walk")
    assert not walk.control_hip
    with pytest.raises(ValueError, match="control law"):
        Plant(walk, 0.005, "law")
    with pytest.raises(ValueError, match="'torque', 'position' or 'law'"):
        Plant(walk, 0.005, "")
    with pytest.raises(ValueError, match=r"qpos\[7 \+ a\]"):
        Plant(permuted_go2_env("position", with_law=False), 0.005, "position")


def test_deploy_examples_and_the_sim_refusal():
    """The two deploy configs load (planner, env and plant-side settings), are no members of the example lists, and DialSim refuses
    sim_leg_control: law with a message before it opens a segment or a device."""
    from dial_mpc_amd.deploy.dial_sim import DialSim, DialSimConfig
    from dial_mpc_amd.examples import deploy_examples, examples
    from dial_mpc_amd.utils.io_utils import load_dataclass_from_dict
    for name in ("go2_height_walk", "go2_stance_residual"):
        d, (dial_config, env_config, env) = _example_env(name)
        sim = load_dataclass_from_dict(DialSimConfig, d)
        assert sim.sim_dt == 0.005 and sim.sim_leg_control == "torque" and env_config.dt == 0.02
        assert bool(env.control_hip) == (name == "go2_stance_residual")
        assert not any(name in e for e in list(deploy_examples) + list(examples))
    sim.sim_leg_control = "law"
    prefix = "zz_plant_plugin_refusal_"
    with pytest.raises(ValueError, match="sim_leg_control: law"):
        DialSim(sim, env_config, dial_config, env, shm_prefix=prefix)
    assert not [f for f in os.listdir("/dev/shm") if f.startswith(prefix)]


def test_custom_env_plant_surface():
    """CustomEnv.context_kwargs(plant=True) names the plant-enabled plugin (another library than plugin_path()'s) with the env's
    parameters; the C header documents the flag and the library exports nothing new."""
    from dial_mpc_amd import _abi, _lib
    _, (_, _, env) = _example_env("go2_stance_residual")
    kw, kwp = env.context_kwargs(), env.context_kwargs(plant=True)
    assert kwp["plugin"] == env.plant_plugin_path() != kw["plugin"] == env.plugin_path()
    assert kwp["user_params"] == kw["user_params"] == env.user_param_vector()
    assert _exports(_dyn_syms(kwp["plugin"]), PLANT_SYMBOL) and PLANT_SYMBOL not in _dyn_syms(kw["plugin"])
    assert "DIAL_PLANT_LAW" in open(_abi.HEADER).read()
    lib = _dyn_syms(_lib.LIB_PATH)
    assert _exports(lib, "dial_plant_step") and "dial_plugin_plant" not in lib
