"""Robust planning over a model ensemble without a GPU: the two entry points and their macros in the header and in _lib, the
hypothesis index, the plan_ensemble block of the closed-loop driver's YAML, libdialplanens.so's code objects (the table's symbol, one
rollout_ens_kernel per family and the aggregation kernel in a code object of its own, no scratch in the Go2's nor in the
aggregation's, the DPP hazard, the recorded resources), the task plugin built with plan_ensemble=True next to its unchanged siblings,
and the NumPy fp64 statement of the aggregation (tests/ensemble_ref.py) against hand-computed cases."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import ensemble_ref as E
import plan_models_cases as C
from plugin_cases import build_matrix, case_model_dict, probe_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
PLAN_ENS_SYMBOL = "dial_plugin_plan_ens_v1"


def test_header_macros_and_binding():
    from dial_mpc_amd import _abi, _lib
    assert _abi.MACROS["DIAL_MAX_ENSEMBLE"] == _lib.MAX_ENSEMBLE == 32
    assert _abi.MACROS["DIAL_ENSEMBLE_MEAN"] == _lib.ENSEMBLE_AGGREGATES["mean"] == 0
    assert _abi.MACROS["DIAL_ENSEMBLE_MIN"] == _lib.ENSEMBLE_AGGREGATES["min"] == 1
    assert _abi.MACROS["DIAL_ENSEMBLE_CVAR"] == _lib.ENSEMBLE_AGGREGATES["cvar"] == 2
    assert sorted(_lib.ENSEMBLE_AGGREGATES) == ["cvar", "mean", "min"]
    text = open(_abi.HEADER).read()
    assert ("int dial_set_plan_ensemble(dial_ctx* ctx, const dial_model* models, int V, const int32_t* hyp /* [rows][R] */,\n"
            "                           int rows, int R, int aggregate, float alpha);") in text
    assert "int dial_get_ensemble_rewards(dial_ctx* ctx, float* out /* device, [R][M][Nsample+1] */, int M, void* stream);" in text
    assert "UNSPECIFIED" in text   # the NaN clause of MIN / CVAR
    for name in ("dial_set_plan_ensemble", "dial_get_ensemble_rewards"):
        assert name in _lib.EXPORTED
    assert hasattr(_lib.Context, "set_plan_ensemble") and hasattr(_lib.Context, "ensemble_rewards")
    lib = ctypes.CDLL(_lib.build())
    lib.dial_set_plan_ensemble.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_float]
    lib.dial_get_ensemble_rewards.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.dial_last_error.argtypes = [ctypes.c_void_p]
    lib.dial_last_error.restype = ctypes.c_char_p
    arg = _abi.MACROS["DIAL_ERR_ARG"]
    assert lib.dial_set_plan_ensemble(None, None, 0, None, 0, 0, 0, 0.0) == arg   # a null context, on any machine
    assert lib.dial_last_error(None).decode().startswith("dial_set_plan_ensemble: ")
    assert lib.dial_get_ensemble_rewards(None, None, 1, None) == arg


def test_plan_ensemble_index():
    from dial_mpc_amd import _lib
    idx = _lib.plan_ensemble_index(None, 3, 2)
    assert idx.dtype == np.int32 and idx.flags["C_CONTIGUOUS"] and idx.tolist() == [[0, 1, 2], [0, 1, 2]]
    assert _lib.plan_ensemble_index(None, 1, 1).tolist() == [[0]]
    assert _lib.plan_ensemble_index(None, 4, 1, R=4).shape == (1, 4)
    hyp = [[0, 1, 2], [3, 0, 1], [2, 2, 3]]
    idx = _lib.plan_ensemble_index(np.array(hyp, np.int64), 4, 3, R=3)
    assert idx.dtype == np.int32 and idx.flags["C_CONTIGUOUS"] and idx.tolist() == hyp
    assert _lib.plan_ensemble_index(hyp, 4, 3).tolist() == hyp
    assert _lib.plan_ensemble_index([2, 0], 3, 3).tolist() == [[2, 0]] * 3   # one list shared by all plans
    assert _lib.plan_ensemble_index(np.array(hyp).T[:, ::-1], 4, 3).flags["C_CONTIGUOUS"]
    for bad in [dict(hyp=[[0, 4, 1]], V=4, rows=1), dict(hyp=[[-1, 0]], V=4, rows=1), dict(hyp=[[0.0, 1.0]], V=4, rows=1),
                dict(hyp=[[[0, 1]]], V=4, rows=1), dict(hyp=hyp, V=4, rows=2), dict(hyp=hyp, V=4, rows=3, R=2), dict(hyp=[], V=4, rows=1),
                dict(hyp=[[]], V=4, rows=1), dict(hyp=None, V=0, rows=1), dict(hyp=None, V=1025, rows=1), dict(hyp=None, V=2, rows=0),
                dict(hyp=None, V=2, rows=10 ** 6), dict(hyp=None, V=3, rows=1, R=2), dict(hyp=None, V=33, rows=1),
                dict(hyp=[list(range(33))], V=40, rows=1)]:
        with pytest.raises(ValueError, match="plan ensemble"):
            _lib.plan_ensemble_index(**bad)


def test_plan_ensemble_yaml_block():
    import yaml
    from dial_mpc_amd.core.dial_core import _plan_models_kw, plan_ensemble_settings
    md = case_model_dict("go2")
    block = yaml.safe_load("""
variants:
  - {}
  - {mass_scale: {base: 1.2}}
  - {mass_scale: {base: 1.4}}
aggregate: cvar
alpha: 0.5
""")
    kw = plan_ensemble_settings(block, md, 2)
    assert sorted(kw) == ["aggregate", "alpha", "hyp", "models"] and kw["aggregate"] == "cvar" and kw["alpha"] == 0.5
    assert len(kw["models"]) == 3 and kw["hyp"].tolist() == [[0, 1, 2], [0, 1, 2]]
    assert np.array_equal(kw["models"][0]["body_mass"], md["body_mass"]) and kw["models"][0] is not md
    assert kw["models"][2]["body_mass"][1] == 1.4 * md["body_mass"][1]
    kw = plan_ensemble_settings(dict(variants=[{}, dict(friction_scale=0.6)], hypotheses=[1, 0, 1]), md, 4)
    assert kw["aggregate"] == "mean" and kw["alpha"] == 1.0 and kw["hyp"].tolist() == [[1, 0, 1]] * 4
    kw = plan_ensemble_settings(dict(variants=[{}, {}], hypotheses=[[0, 1], [1, 1]], aggregate="min"), md, 2)
    assert kw["aggregate"] == "min" and kw["hyp"].tolist() == [[0, 1], [1, 1]]
    for bad, match in [(dict(variants=[{}], mode="mean"), "unknown keys"), (dict(variants=[{}], aggregate="max"), "aggregate"),
                       (dict(aggregate="mean"), "variants"), (dict(variants=[]), "variants"), ([{}], "mapping"),
                       (dict(variants=[{}, dict(mass=2.0)]), "variant 1"), (dict(variants=[dict(mass_scale={"no_such_body": 2.0})]), "variant 0"),
                       (dict(variants=[{}, {}], hypotheses=[0, 2]), "outside"), (dict(variants=[{}, {}], hypotheses=[[0, 1]]), "hypotheses"),
                       (dict(variants=[{}, {}], hypotheses=[0.5, 1]), "hypotheses"), (dict(variants=[{}], hypotheses=[0] * 33), "DIAL_MAX_ENSEMBLE"),
                       (dict(variants=[{}], aggregate="cvar", alpha=0.0), "alpha"), (dict(variants=[{}], aggregate="cvar", alpha=1.5), "alpha"),
                       (dict(variants=[{}], alpha="half"), "alpha")]:
        with pytest.raises(ValueError, match=match):
            plan_ensemble_settings(bad, md, 3)
    # both blocks present: refused before anything is compiled; and the shipped example documents the block, commented out
    with pytest.raises(ValueError, match="plan_models and plan_ensemble"):
        _plan_models_kw(dict(plan_models=dict(variants=[{}]), plan_ensemble=dict(variants=[{}])), None, None, 1)
    from dial_mpc_amd.utils.io_utils import get_example_path
    text = open(get_example_path("unitree_go2_trot.yaml")).read()
    assert "# plan_ensemble:" in text and "plan_ensemble" not in yaml.safe_load(text)


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


def test_plan_ens_library_kernels_and_its_record():
    """libdialplanens.so is built by _lib.build(): the table's symbol; seven family code objects with one rollout_ens_kernel each --
    of the same seven Dims as libdialplant.so's record -- and an eighth with the aggregation kernel alone; no scratch and no spilled
    VGPR in the Go2's (its parent rollout_kernel<DimsGo2, 1, 3> has none), no scratch in the aggregation's; this commit's own record
    line for line.  The older libraries gain neither kernel nor symbol."""
    from dial_mpc_amd import _lib
    _lib.build()
    assert os.path.exists(_lib.PLAN_ENS_LIB_PATH), "libdialplanens.so is not built (dial_mpc_amd._lib.build())"
    assert _exports(_dyn_syms(_lib.PLAN_ENS_LIB_PATH), "dial_plan_ens_ops_v1")
    for older in (_lib.PLANT_LIB_PATH, _lib.PLANT_DIST_LIB_PATH, _lib.PLANT_VAR_LIB_PATH, _lib.PLAN_VAR_LIB_PATH, _lib.LIB_PATH):
        assert "rollout_ens" not in _dyn_syms(older) and "plan_ens_ops" not in _dyn_syms(older), older
    disasm_lib = _disasm_lib()
    with tempfile.TemporaryDirectory() as d:
        cos = disasm_lib.code_objects(_lib.PLAN_ENS_LIB_PATH, d)
        got = [(os.path.basename(co), k["name"][:60], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"])
               for co in cos for k in disasm_lib.kernel_notes(co)]
    assert len(cos) == 8 and len(got) == 8, got
    fam, agg = got[:7], got[7]
    assert all(r[1].startswith("_Z18rollout_ens_kernelI4DimsI") for r in fam), fam
    assert [r[0] for r in fam] == [f"co{k}.o" for k in range(7)] and agg[0] == "co7.o" and agg[1] == "plan_ens_aggregate_kernel"
    parent = _golden("plant_kernel_resources.txt")
    assert len(parent) == 7
    for mine, theirs in zip(fam, parent):
        assert mine[0] == theirs[0]
        n = min(len(mine[1]) - len("_Z18rollout_ens_kernel"), len(theirs[1]) - len("_Z12plant_kernel"))
        assert n > 30 and mine[1][len("_Z18rollout_ens_kernel"):][:n] == theirs[1][len("_Z12plant_kernel"):][:n], (mine, theirs)   # the same Dims
    shipped = [r for r in _golden("shipped_kernel_resources.txt") if r[0] == "co1.o" and r[1].startswith("_Z14rollout_kernel")]
    assert shipped[0][3:] == ("0", "45", "0")            # rollout_kernel<DimsGo2, 1, 3>: no spilled VGPR, no scratch
    assert int(fam[0][3]) == 0 and int(fam[0][5]) == 0, fam[0]     # ... and none here
    assert int(agg[3]) == 0 and int(agg[5]) == 0, agg              # the aggregation: no per-thread array went to scratch
    assert [tuple(str(x) for x in r) for r in got] == _golden("plan_ens_kernel_resources.txt")


def test_plan_ens_kernels_respect_the_dpp_hazard(tmp_path):
    from dial_mpc_amd import _lib
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(_lib.PLAN_ENS_LIB_PATH, str(tmp_path))
    assert len(cos) == 8
    for co in cos[:7]:
        listing = disasm_lib.disassemble(co)
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), listing], capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout[-3000:]
        assert "rollout_ens_kernel" in open(listing).read()


def _kernel_names(so, outdir):
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(so, outdir)
    return cos, [k["name"] for co in cos for k in disasm_lib.kernel_notes(co)]


def build_ens_plugin(model="go2", **kw):
    from dial_mpc_amd.plugin import build_plugin
    return build_plugin(case_model_dict(model), probe_source(), plan_ensemble=True, **kw)


def test_ens_plugin_has_one_more_kernel_the_eighth_table_and_its_own_key(tmp_path):
    """build_plugin(plan_ensemble=True): the default plugin's flags plus the one define, so another key; one kernel and one symbol
    more.  The plugins built without it keep their keys; next to plan_models=True the define comes last and both tables are there."""
    from dial_mpc_amd import plugin
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin, plugin_key
    assert plugin.PLAN_ENS_SYMBOL == PLAN_ENS_SYMBOL
    md, rew, flags = case_model_dict("go2"), probe_source(), list(_COMMON + _FAST)
    sibling = build_matrix(["go2"])["go2"]
    var = C.build_plan_plugin("go2")
    so = build_ens_plugin("go2")
    both = build_ens_plugin("go2", plan_models=True)
    key = lambda p: os.path.basename(os.path.dirname(p))   # noqa: E731
    assert key(sibling) == plugin_key(md, rew, flags)[:24]
    assert key(var) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLAN_VAR=1"])[:24]
    assert key(so) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLAN_ENS=1"])[:24]
    assert key(both) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLAN_VAR=1", "-DDIAL_PLUGIN_PLAN_ENS=1"])[:24]
    assert len({key(sibling), key(var), key(so), key(both)}) == 4 and build_plugin(md, rew, plan_ensemble=False) == sibling
    syms, sib_syms, var_syms, both_syms = _dyn_syms(so), _dyn_syms(sibling), _dyn_syms(var), _dyn_syms(both)
    for name in ("dial_plugin_ops_v1", "dial_plugin_table_v1"):
        assert _exports(syms, name) and _exports(sib_syms, name), name
    assert _exports(syms, PLAN_ENS_SYMBOL) and PLAN_ENS_SYMBOL not in sib_syms and PLAN_ENS_SYMBOL not in var_syms
    assert "dial_plugin_plant" not in syms and C.PLAN_VAR_SYMBOL not in syms
    assert _exports(both_syms, PLAN_ENS_SYMBOL) and _exports(both_syms, C.PLAN_VAR_SYMBOL)
    n_syms = lambda t: len(re.findall(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+dial_plugin_\w+$", t, flags=re.M))   # noqa: E731
    assert n_syms(syms) == n_syms(sib_syms) + 1
    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
    cos, names = _kernel_names(so, str(tmp_path / "a"))
    _, sib_names = _kernel_names(sibling, str(tmp_path / "b"))
    assert len(cos) == 1 and len(names) == len(set(names)) == len(sib_names) + 1, names
    extra = sorted(set(names) - set(sib_names))
    assert set(sib_names) <= set(names) and len(extra) == 1 and "rollout_ens_kernelI8DimsUser" in extra[0], extra
    h = ctypes.CDLL(so, mode=ctypes.RTLD_LOCAL)
    entry = getattr(h, PLAN_ENS_SYMBOL)
    entry.restype = ctypes.POINTER(ctypes.c_int)
    assert list(entry()[0:4]) == [1, 19, 18, 12]   # version, nq, nv, nu
    disasm_lib = _disasm_lib()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), disasm_lib.disassemble(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_custom_env_picks_the_plan_ensemble_plugin(monkeypatch):
    """CustomEnv.plugin_path(plan_ensemble=True) / context_kwargs(plan_ensemble=True) ask build_plugin for that build and leave the
    requests of the default plugin and of the plan_models plugin as they are."""
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
    assert env.plugin_path() == "/p/1" and env.plugin_path(plan_ensemble=True) == "/p/2" and env.plugin_path(plan_ensemble=True) == "/p/2"
    assert env.plugin_path(plan_models=True) == "/p/3" and env.plugin_path(plan_models=True, plan_ensemble=True) == "/p/4"
    assert calls == [dict(control_src=None), dict(control_src=None, plan_ensemble=True), dict(control_src=None, plan_models=True),
                     dict(control_src=None, plan_ensemble=True, plan_models=True)]
    assert env.context_kwargs(plan_ensemble=True)["plugin"] == "/p/2" and env.context_kwargs()["plugin"] == "/p/1"
    with pytest.raises(ValueError, match="plan_ensemble"):
        env.context_kwargs(plant=True, plan_ensemble=True)


# ---- the aggregation's statement against cases worked out by hand (fp32 inputs chosen so that every sum below is exact in fp64)
def _f32(*rows):
    return np.array(rows, np.float32)


def test_ensemble_ref_mean_min_cvar_by_hand():
    raw = _f32([1.0, -2.0, 0.5], [3.0, -2.0, 0.25], [2.0, 4.0, -1.0])   # R = 3, three candidates (columns)
    assert E.aggregate(raw, "mean").tolist() == [2.0, 0.0, np.float32(-0.25 / 3.0)]
    assert E.aggregate(raw, "mean").dtype == np.float32
    assert E.aggregate(raw, "min").tolist() == [1.0, -2.0, -1.0]
    # alpha R = 1.5 -> k = 2: the two smallest of each column
    assert E.cvar_k(0.5, 3) == 2
    assert E.aggregate(raw, "cvar", 0.5).tolist() == [1.5, -2.0, -0.375]
    # k = 1 is the minimum, k = R the mean, bit for bit
    assert E.cvar_k(0.1, 3) == 1 and E.cvar_k(1.0, 3) == 3
    assert E.aggregate(raw, "cvar", 0.1).tobytes() == E.aggregate(raw, "min").tobytes()
    sorted_mean = np.array([(1.0 + 2.0 + 3.0) / 3.0, (-2.0 + -2.0 + 4.0) / 3.0, (-1.0 + 0.25 + 0.5) / 3.0]).astype(np.float32)
    assert E.aggregate(raw, "cvar", 1.0).tobytes() == sorted_mean.tobytes()
    # shapes: [R, M, N + 1] -> [M, N + 1]; R = 1 returns the values themselves in every mode
    raw3 = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert E.aggregate(raw3, "min").shape == (3, 4) and np.array_equal(E.aggregate(raw3, "min"), raw3[0])
    for mode in E.AGGREGATES:
        assert E.aggregate(raw3[:1], mode, 0.3).tobytes() == raw3[0].tobytes()


def test_ensemble_ref_tail_size_ties_and_rounding():
    # alpha R an exact integer is not rounded up: 0.5 x 4 = 2, 0.25 x 4 = 1, 0.75 x 4 = 3; just above it is
    assert [E.cvar_k(a, 4) for a in (0.5, 0.25, 0.75, 1.0)] == [2, 1, 3, 4]
    assert E.cvar_k(0.5 + 2.0 ** -20, 4) == 3 and E.cvar_k(2.0 ** -30, 4) == 1 and E.cvar_k(1.0, 32) == 32
    assert E.cvar_k(0.1, 10) == 2   # 0.1 as fp32 is a little above 1 / 10: the C ABI takes a float
    # ties: equal values enter the tail in index order -- the SUM does not depend on which of two equal values is taken, so the
    # tie rule is visible only through the order of summation; with k = 3 of [1, big, 1, -big, 1 + 2^-23] the ascending order is
    # -big, 1 (r = 0), 1 (r = 2)
    big = np.float32(2.0 ** 60)
    col = _f32([1.0], [big], [1.0], [-big], [1.0 + 2.0 ** -23])
    assert E.cvar_k(0.5, 5) == 3 and E.cvar_k(0.6, 5) == 4   # (0.6 as fp32 is a little above 3 / 5)
    want = np.float32((float(-big) + 1.0 + 1.0) / 3.0)
    assert E.aggregate(col, "cvar", 0.5).tolist() == [want]
    assert E.aggregate(col, "min").tolist() == [-big]
    # the mean is summed in INDEX order in fp64 and rounded once: 2^20 + 2^-20 - 2^20 keeps the small term (fp32 would lose it)
    col = _f32([2.0 ** 20], [2.0 ** -20], [-2.0 ** 20])
    assert E.aggregate(col, "mean").tolist() == [np.float32(2.0 ** -20 / 3.0)]
    # ... while cvar with k = R sums the same values in ASCENDING order: (-2^20 + 2^-20) + 2^20 is exact in fp64 too
    assert E.aggregate(col, "cvar", 1.0).tolist() == [np.float32(2.0 ** -20 / 3.0)]
    # one rounding: the fp64 mean of three fp32 values, not an fp32 sum
    col = _f32([1.0], [2.0 ** -24], [2.0 ** -24])
    assert E.aggregate(col, "mean").tolist() == [np.float32((1.0 + 2.0 ** -23) / 3.0)]
    assert np.float32((1.0 + 2.0 ** -23) / 3.0) != np.float32(np.float32(1.0) / np.float32(3.0))
