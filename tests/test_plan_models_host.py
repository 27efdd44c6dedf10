"""Planner model ensembles without a GPU: the entry point and its macros in the header and in _abi, the index validator of both
modes, the plan_models block of the closed-loop driver's YAML, libdialplanvar.so's code objects (the table's symbol, one
rollout_var_kernel per family, no scratch in the Go2's, the DPP hazard, the recorded resources), the task plugin built with
plan_models=True next to its unchanged siblings, and the fp32 oracle's check that every variant of tests/plan_models_cases.py changes
a reward from the start states and controls the GPU tests use."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import plan_models_cases as C
from plugin_cases import build_matrix, case_model_dict, probe_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_header_macros_and_binding():
    from dial_mpc_amd import _abi, _lib
    assert _abi.MACROS["DIAL_MAX_PLAN_MODELS"] == _lib.MAX_PLAN_MODELS == 1024
    assert _abi.MACROS["DIAL_PLAN_MODELS_PER_PLAN"] == _lib.PLAN_MODEL_MODES["plan"] == 0
    assert _abi.MACROS["DIAL_PLAN_MODELS_PER_SAMPLE"] == _lib.PLAN_MODEL_MODES["sample"] == 1
    text = open(_abi.HEADER).read()
    assert "int dial_set_plan_models(dial_ctx* ctx, const dial_model* models, int V, const int32_t* model_of, int rows, int mode);" in text
    assert "dial_set_plan_models" in _lib.EXPORTED and hasattr(_lib.Context, "set_plan_models")
    lib = ctypes.CDLL(_lib.build())
    assert lib.dial_set_plan_models(None, None, 0, None, 0, 0) == _abi.MACROS["DIAL_ERR_ARG"]   # a null context, on any machine


def test_plan_model_index_both_modes():
    from dial_mpc_amd import _lib
    idx = _lib.plan_model_index(C.PER_PLAN, 4, C.M, "plan")
    assert idx.dtype == np.int32 and idx.flags["C_CONTIGUOUS"] and idx.tolist() == C.PER_PLAN
    idx = _lib.plan_model_index(np.array(C.PER_SAMPLE, np.int64), 4, C.N + 1, "sample")
    assert idx.dtype == np.int32 and idx.tolist() == C.PER_SAMPLE
    # the defaults: per plan g % V; per sample n % V for the noisy samples and 0 for the mean trajectory
    assert _lib.plan_model_index(None, 3, 5, "plan").tolist() == [0, 1, 2, 0, 1]
    assert _lib.plan_model_index(None, 4, 3).tolist() == [0, 1, 2]
    assert _lib.plan_model_index(None, 3, 9, "sample").tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 0]
    assert _lib.plan_model_index(None, 4, 6, "sample").tolist() == [0, 1, 2, 3, 0, 0]
    assert _lib.plan_model_index(None, 1, 1, "plan").tolist() == [0]
    for bad in [dict(model_of=[0, 4, 1], V=4, rows=3), dict(model_of=[-1, 0, 0], V=4, rows=3), dict(model_of=[0.0, 1.0, 2.0], V=4, rows=3),
                dict(model_of=[[0, 1, 2]], V=4, rows=3), dict(model_of=[0, 1], V=4, rows=3), dict(model_of=[], V=4, rows=0),
                dict(model_of=None, V=0, rows=3), dict(model_of=None, V=1025, rows=3), dict(model_of=None, V=2, rows=0),
                dict(model_of=None, V=2, rows=3, per="rollout"), dict(model_of=C.PER_SAMPLE[:-1], V=4, rows=C.N + 1, per="sample"),
                dict(model_of=None, V=2, rows=1, per="sample"), dict(model_of=None, V=2, rows=10 ** 6, per="plan")]:
        with pytest.raises(ValueError, match="plan models"):
            _lib.plan_model_index(**bad)


def test_plan_models_yaml_block():
    import yaml
    from dial_mpc_amd.core.dial_core import plan_models_settings
    md = case_model_dict("go2")
    block = yaml.safe_load("""
per: sample
variants:
  - {}
  - {mass_scale: {base: 1.2}}
  - {friction_scale: 0.6}
""")
    models, index, per = plan_models_settings(block, md, 1, 8)
    assert per == "sample" and len(models) == 3 and index.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 0]
    assert np.array_equal(models[0]["body_mass"], md["body_mass"]) and models[0] is not md
    assert models[1]["body_mass"][1] == 1.2 * md["body_mass"][1] and np.array_equal(models[1]["con_friction"], md["con_friction"])
    assert np.allclose(np.asarray(models[2]["con_friction"])[:, 0], 0.6 * np.asarray(md["con_friction"])[:, 0], rtol=1e-15)
    models, index, per = plan_models_settings(dict(variants=[{}, dict(mass_scale={"base": 1.4})], model_of=[1, 1, 0]), md, 3, 8)
    assert per == "plan" and len(models) == 2 and index.tolist() == [1, 1, 0]
    assert plan_models_settings(dict(variants=[{}, {}]), md, 5, 8)[1].tolist() == [0, 1, 0, 1, 0]
    for bad, match in [(dict(variants=[{}], mode="plan"), "unknown keys"), (dict(per="rollout", variants=[{}]), "per = "),
                       (dict(per="plan"), "variants"), (dict(variants=[]), "variants"), ([{}], "mapping"),
                       (dict(variants=[{}, dict(mass=2.0)]), "variant 1"), (dict(variants=[dict(mass_scale={"no_such_body": 2.0})]), "variant 0"),
                       (dict(variants=[{}, {}], model_of=[0, 1]), "model_of"), (dict(variants=[{}, {}], model_of=[0, 1, 2]), "outside"),
                       (dict(per="sample", variants=[{}], model_of=[0] * 8), "model_of")]:
        with pytest.raises(ValueError, match=match):
            plan_models_settings(bad, md, 3, 8)
    # the shipped example documents the block, commented out: absent means nothing is bound
    from dial_mpc_amd.utils.io_utils import get_example_path
    text = open(get_example_path("unitree_go2_trot.yaml")).read()
    assert "# plan_models:" in text and "plan_models" not in yaml.safe_load(text)


def _dyn_syms(so):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], stdout=subprocess.PIPE, text=True).stdout


def _exports(syms, name):
    return re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+" + name + "$", syms, flags=re.M) is not None


def _disasm_lib():
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    import disasm_lib
    return disasm_lib


def _golden(name):
    return [tuple(line.split()) for line in open(os.path.join(ROOT, "tests", "golden", name)) if line.strip() and not line.startswith("#")]


def test_plan_var_library_one_kernel_per_family_and_its_record():
    """libdialplanvar.so is built by _lib.build(): the table's symbol, seven code objects with one rollout_var_kernel each -- of the
    same seven Dims as libdialplant.so's record --, no scratch and no spilled VGPR in the Go2's (its parent rollout_kernel<DimsGo2, 1, 3>
    has none), and this commit's own record line for line.  The older libraries gain no such kernel."""
    from dial_mpc_amd import _lib
    _lib.build()
    assert os.path.exists(_lib.PLAN_VAR_LIB_PATH), "libdialplanvar.so is not built (dial_mpc_amd._lib.build())"
    assert _exports(_dyn_syms(_lib.PLAN_VAR_LIB_PATH), "dial_plan_var_ops_v1")
    for older in (_lib.PLANT_LIB_PATH, _lib.PLANT_DIST_LIB_PATH, _lib.PLANT_VAR_LIB_PATH, _lib.LIB_PATH):
        assert "rollout_var" not in _dyn_syms(older) and "plan_var_ops" not in _dyn_syms(older), older
    disasm_lib = _disasm_lib()
    with tempfile.TemporaryDirectory() as d:
        cos = disasm_lib.code_objects(_lib.PLAN_VAR_LIB_PATH, d)
        got = [(os.path.basename(co), k["name"][:60], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"])
               for co in cos for k in disasm_lib.kernel_notes(co)]
    assert len(cos) == 7 and len(got) == 7 and all(r[1].startswith("_Z18rollout_var_kernelI4DimsI") for r in got), got
    parent = _golden("plant_kernel_resources.txt")
    assert len(parent) == 7
    for mine, theirs in zip(got, parent):
        assert mine[0] == theirs[0]
        n = min(len(mine[1]) - len("_Z18rollout_var_kernel"), len(theirs[1]) - len("_Z12plant_kernel"))
        assert n > 30 and mine[1][len("_Z18rollout_var_kernel"):][:n] == theirs[1][len("_Z12plant_kernel"):][:n], (mine, theirs)   # the same Dims
    shipped = [r for r in _golden("shipped_kernel_resources.txt") if r[0] == "co1.o" and r[1].startswith("_Z14rollout_kernel")]
    assert shipped[0][3:] == ("0", "45", "0")            # rollout_kernel<DimsGo2, 1, 3>: no spilled VGPR, no scratch
    assert int(got[0][3]) == 0 and int(got[0][5]) == 0, got[0]     # ... and none here
    assert [tuple(str(x) for x in r) for r in got] == _golden("plan_var_kernel_resources.txt")


def test_plan_var_kernels_respect_the_dpp_hazard(tmp_path):
    from dial_mpc_amd import _lib
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(_lib.PLAN_VAR_LIB_PATH, str(tmp_path))
    assert len(cos) == 7
    for co in cos:
        listing = disasm_lib.disassemble(co)
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), listing], capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout[-3000:]
        assert "rollout_var_kernel" in open(listing).read()


def _kernel_names(so, outdir):
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(so, outdir)
    return cos, [k["name"] for co in cos for k in disasm_lib.kernel_notes(co)]


def test_plan_plugin_has_one_more_kernel_the_seventh_table_and_its_own_key(tmp_path):
    """build_plugin(plan_models=True): the default plugin's flags plus the one define, so another key; one kernel and one symbol more.
    The plugins built without it keep their keys; with plant_models=True next to it the define comes last and both tables are there."""
    from dial_mpc_amd import plugin
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin, plugin_key
    assert plugin.PLAN_VAR_SYMBOL == C.PLAN_VAR_SYMBOL
    md, rew, flags = case_model_dict("go2"), probe_source(), list(_COMMON + _FAST)
    sibling = build_matrix(["go2"])["go2"]
    so = C.build_plan_plugin("go2")
    both = C.build_plan_plugin("go2", plant_models=True)
    key = lambda p: os.path.basename(os.path.dirname(p))   # noqa: E731
    assert key(sibling) == plugin_key(md, rew, flags)[:24]
    assert key(so) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLAN_VAR=1"])[:24]
    assert key(both) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1", "-DDIAL_PLUGIN_PLANT_VAR=1", "-DDIAL_PLUGIN_PLAN_VAR=1"])[:24]
    assert len({key(sibling), key(so), key(both)}) == 3 and build_plugin(md, rew, plan_models=False) == sibling
    syms, sib_syms, both_syms = _dyn_syms(so), _dyn_syms(sibling), _dyn_syms(both)
    for name in ("dial_plugin_ops_v1", "dial_plugin_table_v1"):
        assert _exports(syms, name) and _exports(sib_syms, name), name
    assert _exports(syms, C.PLAN_VAR_SYMBOL) and C.PLAN_VAR_SYMBOL not in sib_syms and "dial_plugin_plant" not in syms
    assert _exports(both_syms, C.PLAN_VAR_SYMBOL) and _exports(both_syms, "dial_plugin_plant_var_v1") and _exports(both_syms, "dial_plugin_plant_v1")
    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
    cos, names = _kernel_names(so, str(tmp_path / "a"))
    _, sib_names = _kernel_names(sibling, str(tmp_path / "b"))
    assert len(cos) == 1 and len(names) == len(set(names)) == len(sib_names) + 1, names
    extra = sorted(set(names) - set(sib_names))
    assert set(sib_names) <= set(names) and len(extra) == 1 and "rollout_var_kernelI8DimsUser" in extra[0], extra
    h = ctypes.CDLL(so, mode=ctypes.RTLD_LOCAL)
    entry = getattr(h, C.PLAN_VAR_SYMBOL)
    entry.restype = ctypes.POINTER(ctypes.c_int)
    assert list(entry()[0:4]) == [1, 19, 18, 12]   # version, nq, nv, nu
    disasm_lib = _disasm_lib()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), disasm_lib.disassemble(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_custom_env_picks_the_plan_models_plugin(monkeypatch):
    """CustomEnv.plugin_path(plan_models=True) / context_kwargs(plan_models=True) ask build_plugin for that build and leave the default
    plugin's request as it is."""
    from dial_mpc_amd import plugin
    from dial_mpc_amd.envs.custom_env import CustomEnv
    calls = []
    monkeypatch.setattr(plugin, "build_plugin", lambda model, reward, **kw: calls.append(kw) or f"/p/{len(calls)}")
    env = CustomEnv.__new__(CustomEnv)
    env._plugin = None
    monkeypatch.setattr(CustomEnv, "sys", type("S", (), dict(model={})), raising=False)
    monkeypatch.setattr(CustomEnv, "reward_source", lambda self: "r")
    monkeypatch.setattr(CustomEnv, "control_source", lambda self: None)
    monkeypatch.setattr(CustomEnv, "user_param_vector", lambda self: [])
    monkeypatch.setattr(CustomEnv, "_table", lambda self: None)
    assert env.plugin_path() == "/p/1" and env.plugin_path(plan_models=True) == "/p/2" and env.plugin_path(plan_models=True) == "/p/2"
    assert calls == [dict(control_src=None), dict(control_src=None, plan_models=True)]
    assert env.context_kwargs(plan_models=True)["plugin"] == "/p/2" and env.context_kwargs()["plugin"] == "/p/1"
    with pytest.raises(ValueError, match="plan_models"):
        env.context_kwargs(plant=True, plan_models=True)


@pytest.mark.parametrize("example", C.EXAMPLES)
def test_every_variant_changes_a_reward_on_the_fp32_oracle(example):
    """What tests/test_gpu_plan_models.py relies on, checked before any GPU run: from its start state and controls every non-identity
    variant changes the step rewards of at least one rollout."""
    rews = C.oracle_rewards(example)
    assert rews.shape == (4, C.N + 1, C.H + 1) and np.isfinite(rews).all()
    for v in (1, 2, 3):
        assert (rews[v] != rews[0]).any(axis=1).any(), (example, v)
    assert len({rews[v].tobytes() for v in range(4)}) == 4
