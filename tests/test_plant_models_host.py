"""Plant model mismatch without a GPU: mjcf.vary_model (identity, the scaling law M -> s M, recomputed constants, refusals), the fp32
oracle's check that every variant of tests/plant_models_cases.py moves its plant, the index helper, Plant.set_models on a fake
context, the sim_model block of dial-mpc-sim's config, the new entry point, libdialplantvar.so's code objects (one plant_var_kernel
per family, no scratch where the undisturbed kernel has none, the DPP hazard, the recorded resources) and the task plugin built with
plant_models=True next to its unchanged siblings."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from plant_dist_cases import build_dist_plugins
from plant_models_cases import EXAMPLES, M, MODEL_OF, SIM_DT, VAR_SYMBOL, build_var_plugin, build_var_plugins, oracle_final_states
from plant_plugin_cases import build_plant_plugins
from plugin_cases import build_matrix, case_model_dict, probe_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
DERIVED = ("meaninertia", "body_invweight0", "dof_invweight0")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nz = a != 0
    assert np.array_equal(nz, b != 0)
    return float(np.max(np.abs(a[nz] - b[nz]) / np.abs(a[nz]))) if nz.any() else 0.0


@pytest.mark.parametrize("case", ["go2", "h1_push_crate"])
def test_vary_model_without_arguments_reproduces_the_model(case):
    from dial_mpc_amd.mjcf import vary_model
    m = case_model_dict(case)
    v = vary_model(m)
    assert v is not m and set(v) == set(m)
    for k in m:
        if k in DERIVED:
            assert _rel(m[k], v[k]) <= 1e-12, k   # the shipped derived constants, recomputed
        elif isinstance(m[k], np.ndarray):
            assert np.array_equal(m[k], v[k]) and v[k] is not m[k], k
        else:
            assert v[k] == m[k], k
    v["body_mass"][1] = 0.0   # a copy: the source is untouched
    assert m["body_mass"][1] != 0.0


@pytest.mark.parametrize("case", ["go2", "h1_push_crate"])
def test_scaling_every_mass_and_armature_scales_the_derived_constants(case):
    """M -> s M exactly (every body's mass and inertia and every armature times s), so meaninertia -> s meaninertia and both
    invweight0 arrays -> invweight0 / s: 1e-10 relative is the fp64 inverse's rounding, not a measured number."""
    from dial_mpc_amd.mjcf import vary_model
    m, s = case_model_dict(case), 2.0
    v = vary_model(m, mass_scale=s, armature_scale=s)
    assert np.array_equal(v["body_mass"], s * np.asarray(m["body_mass"])) and np.array_equal(v["body_inertia"], s * np.asarray(m["body_inertia"]))
    assert _rel(s * m["meaninertia"], v["meaninertia"]) <= 1e-10
    assert _rel(np.asarray(m["body_invweight0"]) / s, v["body_invweight0"]) <= 1e-10
    assert _rel(np.asarray(m["dof_invweight0"]) / s, v["dof_invweight0"]) <= 1e-10


def test_a_trunk_only_scale_recomputes_the_constants_of_a_foot():
    from dial_mpc_amd.mjcf import vary_model
    m = case_model_dict("go2")
    trunk = m["names"]["body"][1]
    foot = int(m["nbody"]) - 1
    v = vary_model(m, mass_scale={trunk: 1.3}, com_offset={trunk: [0.02, 0.0, 0.0]})
    assert np.array_equal(vary_model(m, mass_scale={1: 1.3}, com_offset={1: [0.02, 0.0, 0.0]})["body_invweight0"], v["body_invweight0"])
    assert v["body_mass"][1] == 1.3 * m["body_mass"][1] and np.array_equal(v["body_mass"][2:], np.asarray(m["body_mass"])[2:])
    assert np.array_equal(v["body_inertia"][1], 1.3 * np.asarray(m["body_inertia"])[1])
    assert np.array_equal(v["body_ipos"][1], np.asarray(m["body_ipos"])[1] + [0.02, 0.0, 0.0])
    assert v["body_invweight0"][foot, 0] != m["body_invweight0"][foot, 0]   # recomputed, not copied
    assert v["meaninertia"] > m["meaninertia"] and v["dof_invweight0"][0] < m["dof_invweight0"][0]
    # the other arguments touch their own arrays only
    f = vary_model(m, friction_scale={2: 0.5})
    want = np.array(m["con_friction"], np.float64)
    want[2, 0:2] *= 0.5
    assert np.array_equal(f["con_friction"], want) and np.array_equal(f["body_invweight0"], m["body_invweight0"])
    d = vary_model(m, damping_scale=2.0, armature_scale=np.full(int(m["nv"]), 1.5))
    assert np.array_equal(d["dof_damping"], 2.0 * np.asarray(m["dof_damping"])) and np.array_equal(d["dof_armature"], 1.5 * np.asarray(m["dof_armature"]))
    p = case_model_dict("h1_push_crate")
    assert int(p["nfri"]) == 1 and np.array_equal(vary_model(p, frictionloss_scale=3.0)["fri_loss"], 3.0 * np.asarray(p["fri_loss"]))


def test_vary_model_refusals():
    from dial_mpc_amd.mjcf import vary_model
    m = case_model_dict("go2")
    for bad in [dict(mass_scale=0.0), dict(mass_scale=-1.0), dict(mass_scale=float("nan")), dict(mass_scale=float("inf")),
                dict(mass_scale={"no_such_body": 1.2}), dict(mass_scale={99: 1.2}), dict(mass_scale={1: 0.0}), dict(mass_scale=[1.0, 2.0]),
                dict(com_offset={"no_such_body": [0, 0, 0]}), dict(com_offset={1: [0, 0]}), dict(com_offset={1: [0, float("nan"), 0]}),
                dict(com_offset=[0.1, 0, 0]), dict(friction_scale=0.0), dict(friction_scale={17: 0.5}), dict(friction_scale={0: -0.5}),
                dict(damping_scale=[1.0, 2.0]), dict(damping_scale=-2.0), dict(armature_scale=float("inf")), dict(armature_scale=np.zeros(18)),
                dict(frictionloss_scale=0.0), dict(frictionloss_scale=[1.0])]:
        with pytest.raises(ValueError):
            vary_model(m, **bad)
    assert "payload" in vary_model.__doc__ and "geom sizes" in vary_model.__doc__   # what is out of scope is said


@pytest.mark.parametrize("example", EXAMPLES)
def test_every_variant_moves_its_plant_on_the_fp32_oracle(example):
    """What tests/test_gpu_plant_models.py relies on, checked before any GPU run: from its start states every non-identity variant
    leaves the identity plant within K steps, for every one of the M plants."""
    fin = oracle_final_states(example)
    assert fin.shape[:2] == (4, M) and np.isfinite(fin).all()
    for v in (1, 2, 3):
        assert (fin[v] != fin[0]).any(axis=1).all(), (example, v)


def test_index_helper_header_macros_and_binding():
    from dial_mpc_amd import _abi, _lib
    assert _abi.MACROS["DIAL_MAX_PLANT_MODELS"] == _lib.MAX_PLANT_MODELS == 1024
    text = open(_abi.HEADER).read()
    assert "int dial_set_plant_models(dial_ctx* ctx, const dial_model* models, int V, const int32_t* model_of, int M);" in text
    idx = _lib.plant_model_index(MODEL_OF, 4, M)
    assert idx.dtype == np.int32 and idx.flags["C_CONTIGUOUS"] and idx.tolist() == MODEL_OF
    assert _lib.plant_model_index(None, 3).tolist() == [0, 1, 2] and _lib.plant_model_index(None, 3, 3).tolist() == [0, 1, 2]
    assert _lib.plant_model_index(np.array([0, 0, 0], np.int64), 1).tolist() == [0, 0, 0]
    for bad in [dict(model_of=[0, 4], V=4), dict(model_of=[-1], V=4), dict(model_of=[0.0, 1.0], V=4), dict(model_of=[[0, 1]], V=4),
                dict(model_of=[], V=4), dict(model_of=None, V=3, M=4), dict(model_of=[0, 1], V=2, M=3), dict(model_of=None, V=0),
                dict(model_of=None, V=1025)]:
        with pytest.raises(ValueError, match="plant models"):
            _lib.plant_model_index(**bad)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dial_set_plant_models") and "dial_set_plant_models" in _lib.EXPORTED
    assert _lib.load().dial_set_plant_models(None, None, 0, None, 0) == _abi.MACROS["DIAL_ERR_ARG"]   # (a null context: no device needed)
    assert _lib.load().dial_last_error(None).decode().startswith("dial_set_plant_models: ")
    csrc = os.path.join(ROOT, "dial_mpc_amd", "csrc")
    var = open(os.path.join(csrc, "plant_var_kernel.h")).read()
    assert '#define DIAL_PLANT_VAR_SYMBOL "dial_plant_var_ops_v1"' in var and '#define DIAL_PLUGIN_PLANT_VAR_SYMBOL "dial_plugin_plant_var_v1"' in var
    for h in ("plant_kernel.h", "plant_dist_kernel.h", "plant_var_kernel.h"):   # the three restated loops name each other
        head = open(os.path.join(csrc, h)).read().split("#pragma once")[0]
        assert all(n in head for n in ("plant_kernel.h", "plant_dist_kernel.h", "plant_var_kernel.h")), h


class _FakeCtx:
    def __init__(self, nq, nv, nu):
        import torch
        self.nq, self.nv, self.nu, self.torch_device = nq, nv, nu, torch.device("cpu")
        self.bound = []

    def env_reset_batch(self, qpos, qvel):
        import torch
        return torch.cat([qpos, qvel, torch.zeros_like(qvel)], dim=1)

    def set_plant_models(self, models, model_of=None):
        self.bound.append(None if models is None else ([float(m.timestep) for m in models], [float(m.body_mass[1]) for m in models],
                                                       np.asarray(model_of).tolist()))
        return model_of


class _FakeEnv:
    def __init__(self, md):
        from types import SimpleNamespace
        self.sys = SimpleNamespace(nu=int(md["nu"]), model=md)
        self._config = SimpleNamespace(dt=0.02)
        self._init_q = np.zeros(int(md["nq"]))
        self.ctx = _FakeCtx(int(md["nq"]), int(md["nv"]), int(md["nu"]))
        self.asked = []

    def make_model(self):
        from dial_mpc_amd import _abi
        return _abi.make_model(self.sys.model)

    def make_plant(self, sim_dt, device=None, **kw):
        self.asked.append(kw)
        return self.ctx


def test_plant_set_models_on_a_fake_context():
    from dial_mpc_amd.deploy.plant import Plant
    from dial_mpc_amd.mjcf import vary_model
    md = case_model_dict("go2")
    env = _FakeEnv(md)
    heavy, light = vary_model(md, mass_scale={1: 1.5}), vary_model(md, mass_scale={1: 0.5})
    mass = float(np.float32(md["body_mass"][1]))
    p = Plant(env, SIM_DT, "torque", M=4, models=[md, heavy], model_of=[0, 1, 1, 0])
    assert env.asked == [dict(models=True)]
    ts, masses, index = env.ctx.bound[-1]
    assert ts == [float(np.float32(SIM_DT))] * 2 and index == [0, 1, 1, 0] and p.model_of.tolist() == index   # each dict gets timestep = sim_dt
    assert masses == [mass, float(np.float32(1.5 * md["body_mass"][1]))]
    p.reset()
    assert len(env.ctx.bound) == 1 and p.model_of.tolist() == index   # reset() keeps the binding
    p.set_models([md, heavy, light, md])                              # M models map one to one
    assert env.ctx.bound[-1][2] == [0, 1, 2, 3]
    for bad in [dict(models=[md, heavy]), dict(models=[md], model_of=[0, 0, 1, 0]), dict(models=[md], model_of=[0, 0])]:
        with pytest.raises(ValueError, match="plant models"):
            p.set_models(**bad)
    assert p.set_models(None) is None and env.ctx.bound[-1] is None and p.model_of is None
    q = Plant(env, SIM_DT, "torque", M=2)   # a built-in env needs no preparation: models may be bound later
    assert env.asked[-1] == {}
    q.set_models([heavy], [0, 0])
    assert env.ctx.bound[-1][2] == [0, 0]
    both = Plant(env, SIM_DT, "torque", M=2, disturbance=True, models=True)
    assert env.asked[-1] == dict(disturbance=True, models=True) and both.model_of is None


def test_sim_model_block_of_the_config():
    import yaml
    from dial_mpc_amd.deploy.dial_sim import DialSimConfig, sim_model_settings
    from dial_mpc_amd.utils.io_utils import get_example_path, load_dataclass_from_dict
    md = case_model_dict("go2")
    for name in ("unitree_go2_trot_deploy", "unitree_go2_seq_jump_deploy", "unitree_h1_loco_deploy"):
        text = open(get_example_path(name + ".yaml")).read()
        assert "# sim_model:" in text and "#   friction_scale: 0.6" in text
        d = yaml.safe_load(text)
        assert load_dataclass_from_dict(DialSimConfig, d).sim_model is None   # absent: the plant as it was
        block = yaml.safe_load("\n".join(l[2:] for l in text.splitlines() if l.startswith("# sim_model:") or l.startswith("#   ")))["sim_model"]
        assert set(block) == {"mass_scale", "com_offset", "friction_scale", "damping_scale", "armature_scale"}
        if "go2" in name:   # the commented block names real bodies
            v = sim_model_settings(block, md)
            assert v["body_mass"][1] == 1.3 * md["body_mass"][1] and np.array_equal(v["con_friction"][:, 0], 0.6 * np.asarray(md["con_friction"])[:, 0])
    assert load_dataclass_from_dict(DialSimConfig, dict(d, sim_model=dict(friction_scale=0.5))).sim_model == dict(friction_scale=0.5)
    for bad in [dict(mass=2.0), [1.0], dict(mass_scale={"no_such_body": 2.0}), dict(friction_scale=-1.0)]:
        with pytest.raises(ValueError, match="sim_model"):
            sim_model_settings(bad, md)


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


def test_plant_var_library_one_kernel_per_family_no_new_scratch_and_its_record():
    """libdialplantvar.so: the table's symbol, seven code objects with one plant_var_kernel each -- of the same seven Dims as
    libdialplant.so's record --, no scratch and no spilled VGPR in a family whose UNDISTURBED kernel is recorded without scratch, and
    this commit's own record line for line.  The older libraries gain no such kernel."""
    from dial_mpc_amd import _lib
    assert os.path.exists(_lib.PLANT_VAR_LIB_PATH), "libdialplantvar.so is not built (dial_mpc_amd._lib.build())"
    assert _exports(_dyn_syms(_lib.PLANT_VAR_LIB_PATH), "dial_plant_var_ops_v1")
    for older in (_lib.PLANT_LIB_PATH, _lib.PLANT_DIST_LIB_PATH, _lib.LIB_PATH):
        assert "plant_var" not in _dyn_syms(older), older
    disasm_lib = _disasm_lib()
    with tempfile.TemporaryDirectory() as d:
        cos = disasm_lib.code_objects(_lib.PLANT_VAR_LIB_PATH, d)
        got = [(os.path.basename(co), k["name"][:60], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"], k["private_segment_fixed_size"])
               for co in cos for k in disasm_lib.kernel_notes(co)]
    assert len(cos) == 7 and len(got) == 7 and all(r[1].startswith("_Z16plant_var_kernelI4DimsI") for r in got), got
    parent = _golden("plant_kernel_resources.txt")
    assert len(parent) == 7
    for mine, theirs in zip(got, parent):
        assert mine[0] == theirs[0]
        n = min(len(mine[1]) - len("_Z16plant_var_kernel"), len(theirs[1]) - len("_Z12plant_kernel"))
        assert n > 30 and mine[1][len("_Z16plant_var_kernel"):][:n] == theirs[1][len("_Z12plant_kernel"):][:n], (mine, theirs)   # the same Dims
        if int(theirs[5]) == 0:
            assert int(mine[5]) == 0 and int(mine[3]) == 0, (mine, theirs)   # no scratch, no spilled VGPR
    assert [tuple(str(x) for x in r) for r in got] == _golden("plant_var_kernel_resources.txt")


def test_plant_var_kernels_respect_the_dpp_hazard(tmp_path):
    from dial_mpc_amd import _lib
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(_lib.PLANT_VAR_LIB_PATH, str(tmp_path))
    assert len(cos) == 7
    for co in cos:
        listing = disasm_lib.disassemble(co)
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), listing], capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout[-3000:]
        assert "plant_var_kernel" in open(listing).read()


def _kernel_names(so, outdir):
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(so, outdir)
    return cos, [k["name"] for co in cos for k in disasm_lib.kernel_notes(co)]


@pytest.mark.parametrize("law", [None, "probe"], ids=["no-law", "law"])
def test_var_plugin_has_one_more_kernel_and_the_sixth_table(law, tmp_path):
    from dial_mpc_amd import plugin
    assert plugin.PLANT_VAR_SYMBOL == VAR_SYMBOL
    so = build_var_plugins([("go2", law)])[("go2", law)]
    sibling = build_plant_plugins([("go2", law)])[("go2", law)]
    assert so != sibling
    syms, sib_syms = _dyn_syms(so), _dyn_syms(sibling)
    for name in ("dial_plugin_ops_v1", "dial_plugin_table_v1", "dial_plugin_plant_v1"):
        assert _exports(syms, name) and _exports(sib_syms, name), name
    assert _exports(syms, VAR_SYMBOL) and VAR_SYMBOL not in sib_syms and "dial_plugin_plant_dist_v1" not in syms
    assert _exports(syms, "dial_plugin_ctrl_v1") == _exports(sib_syms, "dial_plugin_ctrl_v1") == (law is not None)
    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
    cos, names = _kernel_names(so, str(tmp_path / "a"))
    _, sib_names = _kernel_names(sibling, str(tmp_path / "b"))
    assert len(cos) == 1 and len(names) == len(set(names)) == len(sib_names) + 1 == (8 if law else 7), names
    extra = sorted(set(names) - set(sib_names))
    assert set(sib_names) <= set(names) and len(extra) == 1 and "plant_var_kernelI8DimsUser" in extra[0], extra
    h = ctypes.CDLL(so, mode=ctypes.RTLD_LOCAL)
    entry = getattr(h, VAR_SYMBOL)
    entry.restype = ctypes.POINTER(ctypes.c_int)
    assert list(entry()[0:4]) == [1, 19, 18, 12]   # version, nq, nv, nu
    disasm_lib = _disasm_lib()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), disasm_lib.disassemble(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_plugin_cache_keys_of_the_older_builds_are_unchanged(tmp_path):
    """The new define is part of the key of the plugin that asks for it and of nothing else; with plant_disturbance=True next to it the
    plugin carries both kernels and both tables."""
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin, plugin_key
    md, rew, flags = case_model_dict("go2"), probe_source(), list(_COMMON + _FAST)
    default = build_matrix(["go2"])["go2"]
    plant = build_plant_plugins([("go2", None)])[("go2", None)]
    dist = build_dist_plugins([("go2", None)])[("go2", None)]
    var = build_var_plugin("go2", None)
    both = build_var_plugin("go2", None, disturbance=True)
    key = lambda so: os.path.basename(os.path.dirname(so))   # noqa: E731
    assert key(default) == plugin_key(md, rew, flags)[:24]
    assert key(plant) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1"])[:24]
    assert key(dist) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1", "-DDIAL_PLUGIN_PLANT_DIST=1"])[:24]
    assert key(var) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1", "-DDIAL_PLUGIN_PLANT_VAR=1"])[:24]
    assert key(both) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1", "-DDIAL_PLUGIN_PLANT_DIST=1", "-DDIAL_PLUGIN_PLANT_VAR=1"])[:24]
    assert len({key(default), key(plant), key(dist), key(var), key(both)}) == 5
    assert build_plugin(md, rew, plant=True, plant_models=True) == var == build_plugin(md, rew, plant_models=True)
    syms = _dyn_syms(both)
    assert _exports(syms, VAR_SYMBOL) and _exports(syms, "dial_plugin_plant_dist_v1")
    _, names = _kernel_names(both, str(tmp_path))
    assert sum("plant_var_kernelI8DimsUser" in n for n in names) == 1 and sum("plant_dist_kernelI8DimsUser" in n for n in names) == 1
