"""Plant disturbances without a GPU: the host restatement of the kernel's window test (deploy.plant.event_fires), the packer
(disturbance_row), Plant.set_disturbance / shove on a fake context, the sim_disturbance block of dial-mpc-sim's config, the new entry
point, libdialplantdist.so's code objects (one plant_dist_kernel per family, no scratch where the undisturbed kernel has none, the DPP
hazard, the recorded resources) and the task plugin built with plant_disturbance=True next to its unchanged siblings."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import yaml

from plant_dist_cases import DIST_SYMBOL, build_dist_plugins
from plant_plugin_cases import build_plant_plugins
from plugin_cases import build_matrix, case_model_dict, probe_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dial_mpc_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
SIM_DT = 0.005


# ---- the window test, literally: one comparison per branch, on the float32 bounds widened to fp64
def _ref_fires(t, t0_f32, t1_f32):
    lo, hi = float(t0_f32), float(t1_f32)
    if t != t or lo != lo or hi != hi:
        return False
    if t < lo:
        return False
    if t < hi:
        return True
    return False


def test_event_fires_matches_a_literal_loop():
    """Clocks accumulated by 0.005 over 10^4 steps (they land next to multiples of 0.005 on either side); windows whose bounds sit
    on a step time's float32, one float32 below and one above it, so that the comparison against the widened bound decides."""
    from dial_mpc_amd.deploy.plant import event_fires
    f32 = np.float32
    clocks, t = [], 0.0
    for _ in range(10000):
        clocks.append(t)
        t += SIM_DT
    checked = fired = 0
    sides = set()
    for k in list(range(0, 10000, 97)) + [1, 2, 3, 9999]:
        at = f32(clocks[k])
        for t0 in (np.nextafter(at, f32(-np.inf)), at, np.nextafter(at, f32(np.inf))):
            for t1 in (t0, np.nextafter(at, f32(np.inf)), f32(clocks[k] + 2.5 * SIM_DT)):
                for j in range(max(0, k - 2), min(10000, k + 5)):
                    got, want = event_fires(clocks[j], t0, t1), _ref_fires(clocks[j], t0, t1)
                    assert isinstance(got, bool) and got == want, (k, j, t0, t1)
                    checked += 1
                    fired += got
            sides.add(float(at) < clocks[k])
    assert checked > 5000 and 500 < fired < checked and sides == {True, False}   # the float32 of a clock lands on both sides of it
    # a window of n steps, placed half a step early (Plant.shove's rule), holds exactly n of the accumulated clocks
    for k, n in [(40, 1), (777, 4), (9000, 20)]:
        t0 = clocks[k] - 0.5 * SIM_DT
        assert sum(event_fires(c, f32(t0), f32(t0 + n * SIM_DT)) for c in clocks) == n
    # never: t1 <= t0 (the all-zero slot included), NaN bounds or clock; negative clocks compare like any other
    nan = float("nan")
    for t in (0.0, -0.0, 0.3, -1.0):
        assert not event_fires(t, 0.0, 0.0) and not event_fires(t, 0.5, 0.5) and not event_fires(t, 0.5, 0.25)
        assert not event_fires(t, nan, 1.0) and not event_fires(t, -1.0, nan) and not event_fires(t, nan, nan)
    assert not event_fires(nan, -1.0, 1.0)
    assert event_fires(-0.005, -0.01, 0.0) and not event_fires(0.0, -0.01, 0.0) and event_fires(float(f32(-0.01)), -0.01, 0.0)
    assert event_fires(0.0, 0.0, 1e-30) and event_fires(-0.0, 0.0, 1.0) and not event_fires(-1e-300, 0.0, 1.0)
    assert event_fires(0.3, 0.3, 0.31) == (0.3 >= float(f32(0.3)))   # the bound is the float32, not the decimal


def test_disturbance_row_layout_broadcasting_and_refusals():
    from dial_mpc_amd import _abi, _lib
    from dial_mpc_amd.deploy import plant
    from dial_mpc_amd.deploy.plant import disturbance_row
    nu, nv = 3, 5
    assert plant.MAX_EVENTS == _abi.MACROS["DIAL_PLANT_MAX_EVENTS"] == _lib.PLANT_MAX_EVENTS == 16
    text = open(_abi.HEADER).read()
    assert "#define DIAL_PLANT_DIST_ROW(nu, nv, E) (2 * (nu) + (E) * (2 + (nv)))" in text
    r = disturbance_row(nu, nv)
    assert r.dtype == np.float32 and r.tolist() == [1, 1, 1, 0, 0, 0] and len(r) == _lib.plant_dist_row(nu, nv, 0)
    r = disturbance_row(nu, nv, gain=0.5, bias=[1, 2, 3])
    assert r.tolist() == [0.5, 0.5, 0.5, 1, 2, 3]
    ev = [(0.25, 0.5, np.arange(nv)), (1.0, 1.5, -np.arange(nv) / 4)]
    r = disturbance_row(nu, nv, [2, 3, 4], None, ev)
    assert len(r) == 2 * nu + 2 * (2 + nv) == _lib.plant_dist_row(nu, nv, 2)
    assert r[:6].tolist() == [2, 3, 4, 0, 0, 0]
    assert r[6:13].tolist() == [0.25, 0.5, 0, 1, 2, 3, 4] and r[13:20].tolist() == [1.0, 1.5, 0, -0.25, -0.5, -0.75, -1.0]
    assert len(disturbance_row(nu, nv, events=[(0, 0, np.zeros(nv))] * 16)) == _lib.plant_dist_row(nu, nv, 16)
    for bad in [dict(gain=[1, 2]), dict(bias=np.ones((2, 3))), dict(gain=float("nan")), dict(bias=[0, float("inf"), 0]),
                dict(events=[(0, 1, np.zeros(nv - 1))]), dict(events=[(0, 1)]), dict(events=[(float("nan"), 1, np.zeros(nv))]),
                dict(events=[(0, 1, [0, 0, float("inf"), 0, 0])]), dict(events=[(0, 0, np.zeros(nv))] * 17)]:
        with pytest.raises(ValueError):
            disturbance_row(nu, nv, **bad)


class _FakeCtx:
    """What Plant needs of a _lib.Context, on the CPU: it records what gets bound."""

    def __init__(self, nq, nv, nu):
        import torch
        self.nq, self.nv, self.nu, self.torch_device = nq, nv, nu, torch.device("cpu")
        self.bound = []

    def env_reset_batch(self, qpos, qvel):
        import torch
        return torch.cat([qpos, qvel, torch.zeros_like(qvel)], dim=1)

    def set_plant_disturbance(self, dist, n_events=0):
        self.bound.append(None if dist is None else (dist.numpy().copy(), int(n_events)))
        return dist


class _FakeEnv:
    """A free base joint and nu hinge actuators behind it; make_plant hands out the fake context."""

    def __init__(self, nu=2, free=True):
        from types import SimpleNamespace
        nq, nv = (7 if free else 1) + nu, (6 if free else 1) + nu
        model = dict(njnt=1 + nu, jnt_type=[0 if free else 3] + [3] * nu, nq=nq, nv=nv, nu=nu)
        self.sys = SimpleNamespace(nu=nu, model=model)
        self._config = SimpleNamespace(dt=0.02)
        self._init_q = np.zeros(nq)
        self.ctx = _FakeCtx(nq, nv, nu)
        self.asked = []

    def make_model(self):
        from types import SimpleNamespace
        return SimpleNamespace(act_isposition=[0] * self.sys.nu)

    def make_plant(self, sim_dt, device=None, **kw):
        self.asked.append(kw)
        return self.ctx


def test_plant_set_disturbance_and_shove_arithmetic():
    from dial_mpc_amd.deploy.plant import Plant, disturbance_row, event_fires
    env = _FakeEnv(nu=2)
    nu, nv = 2, 8
    plain = Plant(env, SIM_DT, "torque", M=2)
    assert env.asked == [{}] and env.ctx.bound == []           # the undisturbed plant asks for nothing new
    with pytest.raises(ValueError, match="disturbance=True"):
        plain.set_disturbance(gain=0.5)
    with pytest.raises(ValueError, match="disturbance=True"):
        plain.shove(0.1, 0.01, np.ones(6))
    M = 3
    p = Plant(env, SIM_DT, "torque", M=M, disturbance=dict(gain=[0.5, 2.0], bias=0.25))
    assert env.asked[-1] == dict(disturbance=True)
    rows, E = env.ctx.bound[-1]
    assert E == 0 and rows.shape == (M, 2 * nu) and rows.dtype == np.float32
    assert np.array_equal(rows, np.tile(np.float32([0.5, 2.0, 0.25, 0.25]), (M, 1)))
    # per-plant gains, an event for every plant and one for plant 1 alone, in list order; shorter lists padded with a slot that never fires
    g = np.float32([[1, 1], [0.5, 0.75], [1.25, 1]])
    dv_all, dv_one = np.arange(nv) / 64.0, -np.arange(nv) / 32.0
    p.set_disturbance(gain=g, events=[(None, 0.1, 0.2, dv_all), (1, 0.3, 0.4, dv_one)])
    rows, E = env.ctx.bound[-1]
    assert E == 2 and rows.shape == (M, 2 * nu + 2 * (2 + nv))
    pad = (0.0, 0.0, np.zeros(nv))
    for m in range(M):
        ev = [(0.1, 0.2, dv_all)] + ([(0.3, 0.4, dv_one)] if m == 1 else [pad])
        assert np.array_equal(rows[m], disturbance_row(nu, nv, g[m], None, ev)), m
    assert not event_fires(0.0, *rows[0, 2 * nu + 2 + nv:2 * nu + 2 + nv + 2])
    # a shove of 0.1 s at t = 1.0: 20 steps, dv = dvel6 / 20 in float32 on dofs 0-5, zero on the joints, half a step early
    d6 = np.array([0.0, 0.8, 0.0, 0.1, 0.0, -0.2])
    t0, t1, dv = p.shove(1.0, 0.1, d6, plant=2)
    assert t0 == np.float32(1.0 - 0.5 * SIM_DT) and t1 == np.float32(1.0 - 0.5 * SIM_DT + 20 * SIM_DT)
    assert dv.dtype == np.float32 and np.array_equal(dv[:6], (d6 / 20).astype(np.float32)) and not dv[6:].any()
    rows, E = env.ctx.bound[-1]
    assert E == 2 and np.array_equal(rows[2, 2 * nu + 2 + nv:], np.concatenate([[t0, t1], dv]))   # plant 2's second slot
    assert np.array_equal(rows[0, 2 * nu + 2 + nv:], np.zeros(2 + nv, np.float32))                 # the others: still the pad
    clocks, t = [], 0.0
    for _ in range(400):
        clocks.append(t)
        t += SIM_DT
    assert sum(event_fires(c, t0, t1) for c in clocks) == 20
    acc = np.zeros(6, np.float32)
    for _ in range(20):
        acc += dv[:6]
    assert np.allclose(acc, d6, rtol=0, atol=20 * 2.0 ** -24)   # 20 float32 additions of values below 1: half an ulp of 1 each at most
    # durations below a step are one step; every plant when plant is None; the 17th event is refused
    t0, t1, dv = p.shove(0.5, 0.0, d6)
    assert np.array_equal(dv[:6], d6.astype(np.float32)) and sum(event_fires(c, t0, t1) for c in clocks) == 1
    assert env.ctx.bound[-1][1] == 3
    for bad in [dict(dvel6=np.ones(5)), dict(dvel6=[0, 0, 0, 0, 0, float("nan")]), dict(duration=-0.1), dict(plant=3), dict(t=float("inf"))]:
        with pytest.raises(ValueError):
            p.shove(**{**dict(t=0.2, duration=0.01, dvel6=d6), **bad})
    q = Plant(env, SIM_DT, "torque", M=1, disturbance=True)
    for i in range(16):
        q.shove(0.01 * i, 0.005, d6)
    with pytest.raises(ValueError, match="16"):
        q.shove(1.0, 0.005, d6)
    with pytest.raises(ValueError):
        q.set_disturbance(events=[(0, 0.0, 1.0, np.zeros(nv))] * 17)
    # reset keeps the binding; all-None unbinds
    n = len(env.ctx.bound)
    q.reset()
    assert len(env.ctx.bound) == n and q.t == 0.0
    q.set_disturbance()
    assert env.ctx.bound[-1] is None
    with pytest.raises(ValueError, match="free base joint"):
        Plant(_FakeEnv(nu=2, free=False), SIM_DT, "torque", disturbance=True).shove(0.0, 0.01, d6)


_DEPLOY = ("unitree_go2_trot_deploy", "unitree_go2_seq_jump_deploy", "unitree_h1_loco_deploy")


def test_dial_sim_config_takes_the_disturbance_block():
    from dial_mpc_amd.deploy.dial_sim import DialSimConfig, sim_disturbance_settings
    from dial_mpc_amd.utils.io_utils import get_example_path, load_dataclass_from_dict
    for example in _DEPLOY:
        d = yaml.safe_load(open(get_example_path(example + ".yaml")))
        cfg = load_dataclass_from_dict(DialSimConfig, d)
        assert cfg.sim_disturbance is None and cfg.sim_dt == 0.005
    block = yaml.safe_load("""
sim_disturbance:
  actuator_gain: 0.8
  actuator_bias: [0.5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -0.5]
  gain_range: [0.9, 1.1]
  seed: 3
  shoves:
    - {t: 1.0, duration: 0.1, dv: [0, 0.8, 0, 0, 0, 0]}
""")
    cfg = load_dataclass_from_dict(DialSimConfig, {**d, **block})
    assert cfg.sim_disturbance == block["sim_disturbance"]
    gain, bias, shoves = sim_disturbance_settings(cfg.sim_disturbance, 12)
    draw = np.random.default_rng(3).uniform(0.9, 1.1, 12)
    assert np.array_equal(gain, 0.8 * draw) and len(set(gain.tolist())) == 12 and (gain >= 0.72).all() and (gain <= 0.88).all()
    assert bias.tolist() == [0.5] + [0.0] * 10 + [-0.5]
    assert len(shoves) == 1 and shoves[0][:2] == (1.0, 0.1) and shoves[0][2].tolist() == [0, 0.8, 0, 0, 0, 0]
    gain, bias, shoves = sim_disturbance_settings({}, 12)
    assert gain.tolist() == [1.0] * 12 and bias.tolist() == [0.0] * 12 and shoves == []
    for bad in [dict(actuator_gain=[1, 2]), dict(mass_scale=1.2), dict(gain_range=[1.1, 0.9]), dict(gain_range=[1.0]),
                dict(shoves=[dict(t=0, duration=0.1, dv=[1, 2, 3])]), dict(shoves=[dict(t=0, dv=[0] * 6)]), dict(actuator_bias=float("nan"))]:
        with pytest.raises(ValueError, match="sim_disturbance"):
            sim_disturbance_settings(bad, 12)


def test_libdialhip_exports_dial_set_plant_disturbance():
    from dial_mpc_amd import _abi, _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dial_set_plant_disturbance") and "dial_set_plant_disturbance" in _lib.EXPORTED
    assert "int dial_set_plant_disturbance(dial_ctx* ctx, const float* dist, int M, int n_events);" in open(_abi.HEADER).read()
    assert _lib.load().dial_set_plant_disturbance(None, None, 0, 0) == _abi.MACROS["DIAL_ERR_ARG"]   # (a null context: no device needed)
    assert _lib.load().dial_last_error(None).decode().startswith("dial_set_plant_disturbance: ")


def _dyn_syms(so):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], stdout=subprocess.PIPE, text=True).stdout


def _exports(syms, name):
    return re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+" + name + "$", syms, flags=re.M) is not None


def _disasm_lib():
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    import disasm_lib
    return disasm_lib


def _resources(lib, d):
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(lib, d)
    return cos, [(os.path.basename(co), k["name"][:60], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"],
                  k["private_segment_fixed_size"]) for co in cos for k in disasm_lib.kernel_notes(co)]


def _golden(name):
    return [tuple(line.split()) for line in open(os.path.join(ROOT, "tests", "golden", name)) if line.strip() and not line.startswith("#")]


def test_plant_dist_library_one_kernel_per_family_no_new_scratch_and_its_record():
    """libdialplantdist.so: the table's symbol, seven code objects with one plant_dist_kernel each -- of the same seven Dims as
    libdialplant.so's record --, no scratch in a family whose UNDISTURBED kernel is recorded without scratch (the gate is the parent's
    record, tests/golden/plant_kernel_resources.txt), and this commit's own record line for line."""
    from dial_mpc_amd import _lib
    assert os.path.exists(_lib.PLANT_DIST_LIB_PATH), "libdialplantdist.so is not built (dial_mpc_amd._lib.build())"
    assert _exports(_dyn_syms(_lib.PLANT_DIST_LIB_PATH), "dial_plant_dist_ops_v1")
    assert "plant_dist" not in _dyn_syms(_lib.PLANT_LIB_PATH) and "plant_dist" not in _dyn_syms(_lib.LIB_PATH).replace("dial_set_plant_disturbance", "")
    with tempfile.TemporaryDirectory() as d:
        cos, got = _resources(_lib.PLANT_DIST_LIB_PATH, d)
    assert len(cos) == 7 and len(got) == 7 and all(r[1].startswith("_Z17plant_dist_kernelI4DimsI") for r in got), got
    parent = _golden("plant_kernel_resources.txt")
    assert len(parent) == 7
    for mine, theirs in zip(got, parent):
        assert mine[0] == theirs[0]
        assert theirs[1][len("_Z12plant_kernel"):].startswith(mine[1][len("_Z17plant_dist_kernel"):]), (mine, theirs)   # the same Dims
        if int(theirs[5]) == 0:
            assert int(mine[5]) == 0 and int(mine[3]) == 0, (mine, theirs)   # no scratch, no spilled VGPR
    assert got == _golden("plant_dist_kernel_resources.txt")


def test_plant_dist_kernels_respect_the_dpp_hazard(tmp_path):
    from dial_mpc_amd import _lib
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(_lib.PLANT_DIST_LIB_PATH, str(tmp_path))
    assert len(cos) == 7
    for co in cos:
        listing = disasm_lib.disassemble(co)
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), listing], capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout[-3000:]
        assert "plant_dist_kernel" in open(listing).read()


def _kernel_names(so, outdir):
    disasm_lib = _disasm_lib()
    cos = disasm_lib.code_objects(so, outdir)
    return cos, [k["name"] for co in cos for k in disasm_lib.kernel_notes(co)]


@pytest.mark.parametrize("law", [None, "probe"], ids=["no-law", "law"])
def test_dist_plugin_has_one_more_kernel_and_the_fifth_table(law, tmp_path):
    from dial_mpc_amd import plugin
    assert plugin.PLANT_DIST_SYMBOL == DIST_SYMBOL
    so = build_dist_plugins([("go2", law)])[("go2", law)]
    sibling = build_plant_plugins([("go2", law)])[("go2", law)]
    assert so != sibling
    syms, sib_syms = _dyn_syms(so), _dyn_syms(sibling)
    for name in ("dial_plugin_ops_v1", "dial_plugin_table_v1", "dial_plugin_plant_v1"):
        assert _exports(syms, name) and _exports(sib_syms, name), name
    assert _exports(syms, DIST_SYMBOL) and DIST_SYMBOL not in sib_syms
    assert _exports(syms, "dial_plugin_ctrl_v1") == _exports(sib_syms, "dial_plugin_ctrl_v1") == (law is not None)
    os.makedirs(tmp_path / "a"), os.makedirs(tmp_path / "b")
    cos, names = _kernel_names(so, str(tmp_path / "a"))
    _, sib_names = _kernel_names(sibling, str(tmp_path / "b"))
    assert len(cos) == 1 and len(names) == len(set(names)) == len(sib_names) + 1 == (8 if law else 7), names
    extra = sorted(set(names) - set(sib_names))
    assert set(sib_names) <= set(names) and len(extra) == 1 and "plant_dist_kernelI8DimsUser" in extra[0], extra
    h = ctypes.CDLL(so, mode=ctypes.RTLD_LOCAL)
    entry = getattr(h, DIST_SYMBOL)
    entry.restype = ctypes.POINTER(ctypes.c_int)
    assert list(entry()[0:4]) == [1, 19, 18, 12]   # version, nq, nv, nu
    disasm_lib = _disasm_lib()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), disasm_lib.disassemble(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_plugin_cache_keys_of_the_older_builds_are_unchanged():
    """The new define is part of the key of the plugin that asks for it and of nothing else: the default and the plant=True plugins'
    keys are the keys of their flag lists as they were."""
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin, plugin_key
    md, rew, flags = case_model_dict("go2"), probe_source(), list(_COMMON + _FAST)
    default = build_matrix(["go2"])["go2"]
    plant = build_plant_plugins([("go2", None)])[("go2", None)]
    dist = build_dist_plugins([("go2", None)])[("go2", None)]
    key = lambda so: os.path.basename(os.path.dirname(so))   # noqa: E731
    assert key(default) == plugin_key(md, rew, flags)[:24]
    assert key(plant) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1"])[:24]
    assert key(dist) == plugin_key(md, rew, flags + ["-DDIAL_PLUGIN_PLANT=1", "-DDIAL_PLUGIN_PLANT_DIST=1"])[:24]
    assert len({key(default), key(plant), key(dist)}) == 3
    assert build_plugin(md, rew, plant=True, plant_disturbance=True) == dist == build_plugin(md, rew, plant_disturbance=True)
