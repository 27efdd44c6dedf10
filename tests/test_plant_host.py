"""Plant simulator (deploy/plant.py, deploy/dial_sim.py, libdialplant.so): the host-side rules, the configuration, the shared-memory
segments and the built library -- everything that needs no GPU."""
import os
import subprocess
import sys
import tempfile
import uuid

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dial_mpc_amd", "csrc")


# ---- a literal transcription of dial_sim.py's arithmetic (main_loop), with the float32 plan_time widened to fp64
def _ref_async_row(t, plan_time_f32, ctrl_dt, n_acts):
    delta_time = t - float(plan_time_f32)
    delta_step = int(delta_time / ctrl_dt)
    if delta_step >= n_acts or delta_step < 0:
        delta_step = n_acts - 1
    return delta_step


def _ref_sync_steps(t, plan_time_f32, ctrl_dt, sim_dt):
    n = 0
    while t <= (float(plan_time_f32) + ctrl_dt):
        n += 1
        t += sim_dt
    return n


def test_ctrl_row_matches_dial_sim():
    from dial_mpc_amd.deploy.plant import ctrl_row
    ctrl_dt, T = 0.02, 17
    f32 = np.float32
    assert ctrl_row(0.0, f32(-ctrl_dt), ctrl_dt, T) == _ref_async_row(0.0, f32(-ctrl_dt), ctrl_dt, T) == 0   # the initial plan_time
    for t, pt in [(0.0, 0.1), (0.0, 0.011), (0.3, 0.31), (1.0, 5.0)]:      # negative delta: truncation toward zero, or the last row
        assert ctrl_row(t, f32(pt), ctrl_dt, T) == _ref_async_row(t, f32(pt), ctrl_dt, T)
    assert ctrl_row(0.0, f32(0.1), ctrl_dt, T) == T - 1 and ctrl_row(0.3, f32(0.31), ctrl_dt, T) == 0
    for t in (T * ctrl_dt, T * ctrl_dt + 1e-12, (T - 1) * ctrl_dt, 10.0, 1e9):   # at and past n_acts * ctrl_dt
        assert ctrl_row(t, f32(0.0), ctrl_dt, T) == _ref_async_row(t, f32(0.0), ctrl_dt, T)
    assert ctrl_row(T * ctrl_dt + 1e-9, f32(0.0), ctrl_dt, T) == T - 1
    # the clock accumulated over 10^4 steps of 0.005 (the quotient lands next to integers again and again), plan times that lag it
    t, rows, hits = 0.0, [], 0
    rng = np.random.default_rng(0)
    for i in range(10000):
        pt = f32(round(t - (i % 7) * 0.005, 3) if i % 3 else t - rng.uniform(0, 0.4))
        got, want = ctrl_row(t, pt, ctrl_dt, T), _ref_async_row(t, pt, ctrl_dt, T)
        assert got == want, (i, t, pt)
        rows.append(got)
        t += 0.005
    assert len(set(rows)) >= 5


def test_sync_steps_matches_dial_sim():
    from dial_mpc_amd.deploy.plant import sync_steps
    ctrl_dt, sim_dt = 0.02, 0.005
    assert sync_steps(0.0, np.float32(-ctrl_dt), ctrl_dt, sim_dt) == _ref_sync_steps(0.0, np.float32(-ctrl_dt), ctrl_dt, sim_dt)
    t, total = 0.0, 0
    for tick in range(2500):   # a sync run: each plan is published at the plant's own clock
        pt = np.float32(t)
        n = sync_steps(t, pt, ctrl_dt, sim_dt)
        assert n == _ref_sync_steps(t, pt, ctrl_dt, sim_dt) and 4 <= n <= 5, (tick, t, n)
        for _ in range(n):
            t += sim_dt
        total += n
    assert sync_steps(t, np.float32(t - 1.0), ctrl_dt, sim_dt) == 0   # an old plan: nothing to do until a new one arrives


# the reference's plant-side values of the three deploy examples
_DEPLOY = {"unitree_go2_trot_deploy": ("unitree_go2", "scene.xml"), "unitree_go2_seq_jump_deploy": ("unitree_go2", "scene.xml"),
           "unitree_h1_loco_deploy": ("unitree_h1", "scene_h1_loco.xml")}


@pytest.mark.parametrize("example", sorted(_DEPLOY))
def test_dial_sim_config_loads_the_deploy_examples(example):
    from dial_mpc_amd.deploy.dial_sim import DialSimConfig
    from dial_mpc_amd.examples import deploy_examples
    from dial_mpc_amd.utils.io_utils import get_example_path, load_dataclass_from_dict
    assert example in deploy_examples
    cfg = load_dataclass_from_dict(DialSimConfig, yaml.safe_load(open(get_example_path(example + ".yaml"))))
    assert (cfg.robot_name, cfg.scene_name) == _DEPLOY[example]
    assert cfg.sim_leg_control == "torque" and cfg.plot is False and cfg.record is False
    assert cfg.real_time_factor == 1.0 and cfg.sim_dt == 0.005 and cfg.sync_mode is False


@pytest.mark.parametrize("prefix", ["", "plant_test_"])
def test_segments_are_what_the_publisher_attaches_to(prefix):
    from dial_mpc_amd.deploy import dial_plan, dial_sim
    assert dial_sim.open_segments is dial_plan.open_segments   # one definition of the protocol
    prefix = prefix + uuid.uuid4().hex[:8] + "_" if prefix else ""
    if not prefix and any(os.path.exists(os.path.join("/dev/shm", n)) for n in dial_plan.SEGMENTS):
        pytest.skip("unprefixed segments exist on this host (a plant is running)")
    nq, nv, nu, T = 19, 18, 12, 17
    own = dial_plan.open_segments(nq, nv, nu, T, create=True, prefix=prefix)
    try:
        peer = dial_plan.open_segments(nq, nv, nu, T, create=False, prefix=prefix)
        shapes = {"time_shm": (1,), "state_shm": (nq + nv,), "acts_shm": (T, nu), "refs_shm": (T, nu, 3), "plan_time_shm": (1,),
                  "tau_shm": (T, nu)}
        assert set(own) == set(dial_plan.SEGMENTS) == set(shapes)
        for name, shape in shapes.items():
            shm, arr = own[name]
            assert shm.name.lstrip("/") == prefix + name and arr.shape == shape and arr.dtype == np.float32
            assert shm.size >= int(np.prod(shape)) * 32                   # the reference's 8x over-allocation
            arr.reshape(-1)[-1] = 7.0
            assert peer[name][1].reshape(-1)[-1] == 7.0
        for shm, _ in peer.values():
            shm.close()
    finally:
        for shm, _ in own.values():
            shm.close()
            shm.unlink()


def test_libdialhip_exports_dial_plant_step():
    import ctypes
    from dial_mpc_amd import _abi, _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dial_plant_step") and "dial_plant_step" in _lib.EXPORTED
    assert (_abi.MACROS["DIAL_PLANT_CTRL"], _abi.MACROS["DIAL_PLANT_PD"], _abi.MACROS["DIAL_PLANT_HOLD_FIRST"]) == (1, 2, 4)
    assert (_lib.PLANT_CTRL, _lib.PLANT_PD, _lib.PLANT_HOLD_FIRST) == (1, 2, 4)


def _plant_code_objects(d):
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    import disasm_lib
    lib = os.path.join(CSRC, "libdialplant.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("libdialplant.so not built or no llvm-objdump")
    return disasm_lib, disasm_lib.code_objects(lib, d)


def test_plant_library_has_one_kernel_per_family_and_its_recorded_resources():
    want = [tuple(line.split()) for line in open(os.path.join(ROOT, "tests", "golden", "plant_kernel_resources.txt"))
            if line.strip() and not line.startswith("#")]
    with tempfile.TemporaryDirectory() as d:
        disasm_lib, cos = _plant_code_objects(d)
        got = [(os.path.basename(co), k["name"][:60], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"],
                k["private_segment_fixed_size"]) for co in cos for k in disasm_lib.kernel_notes(co)]
    assert len(cos) == 7 and len(got) == 7 and all(r[1].startswith("_Z12plant_kernel") for r in got)
    assert len({r[1] for r in got}) == 7
    assert got == want


def test_plant_kernels_respect_the_dpp_hazard(tmp_path):
    disasm_lib, cos = _plant_code_objects(str(tmp_path))
    for co in cos:
        listing = disasm_lib.disassemble(co)
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), listing],
                             capture_output=True, text=True)
        assert chk.returncode == 0, chk.stdout[-3000:]
        assert "plant_kernel" in open(listing).read()


def test_sim2sim_forwards_its_arguments(monkeypatch):
    """--list-examples runs the plant's listing alone (no GPU, no segments)."""
    out = subprocess.run([sys.executable, "-m", "dial_mpc_amd.core.dial_sim2sim", "--list-examples"], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "unitree_go2_trot_deploy" in out.stdout
