"""GPU tests of the plant simulator: dial_plant_step (csrc/plant_kernel.h in libdialplant.so) against the fp32 oracle, its bit identities
on the device, its argument checks, and dial-mpc-sim in a closed loop with the planner -- in one process and as two processes."""
import os
import shutil
import subprocess
import sys
import uuid

import numpy as np
import pytest
import yaml

from conftest import KNIFE_EDGE_FRAC, TOL, _within, setup_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DT, CTRL_DT, T, R = 0.005, 0.02, 17, 64.0   # R: the joint range [-R, R] of the oracle's task (a power of two: act2joint is exact)


def _dev(x, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda:0")


GEN = dict(force_generic=1)   # dial_options: the capacity-dimension instantiation (DimsMax, kernel instantiation 0) and its plant kernel


def _case(example, pd):
    """(model, task) of the example at sim_dt with one physics step per step, and the oracle's action mapping made the identity up to
    the factor R: joint_offset 0, joint_range = phys_range = [-R, R], action_scale 1 -> act2joint(c / R) = c for dyadic c."""
    _, env, model, task, _ = setup_case(example, 8, 4, per_rollout=True)
    model.timestep = SIM_DT
    task.n_frames, task.dt = 1, SIM_DT
    task.position_control = 0 if pd else 1
    task.action_scale = 1.0
    for a in range(model.nu):
        task.joint_offset[a] = 0.0
        task.joint_range[a][0], task.joint_range[a][1] = -R, R
        task.phys_range[a][0], task.phys_range[a][1] = -R, R
    return env, model, task


def _act_q(model):
    """qpos addresses of the actuated joints."""
    return [int(model.act_qposadr[a]) for a in range(model.nu)]


def _start_states(ctx, env, M, seed):
    """The env's initial pose plus seeded perturbations of the actuated joints and of every velocity (plant 0: the pose itself)."""
    rng = np.random.default_rng(seed)
    q0 = np.asarray(env._init_q, np.float32)
    qpos = np.tile(q0, (M, 1))
    qvel = np.zeros((M, ctx.nv), np.float32)
    qpos[1:, _act_q(ctx.model)] += rng.uniform(-0.1, 0.1, (M - 1, ctx.nu)).astype(np.float32)
    qvel[1:] = rng.uniform(-0.3, 0.3, (M - 1, ctx.nv)).astype(np.float32)
    return ctx.env_reset_batch(_dev(qpos), _dev(qvel))


def _rows(env, M, pd, seed):
    """[M, T, nu] dyadic rows: torques k / 8 (CTRL; the actuators' own ctrlrange clip applies) or joint targets near the initial pose on a
    1/256 grid (PD, and the Allegro's position actuators)."""
    rng = np.random.default_rng(seed)
    model = env.make_model()
    nu = model.nu
    if pd or any(model.act_isposition[a] for a in range(nu)):
        q0 = np.asarray(env._init_q, np.float64)[_act_q(model)]
        base = np.round(q0 * 256) / 256
        return (base + rng.integers(-64, 65, (M, T, nu)) / 256).astype(np.float32)
    return (rng.integers(-160, 161, (M, T, nu)) / 8).astype(np.float32)


def _clocks(M):
    t = np.array([0.005 * (m % 9) + 0.3 for m in range(M)])
    plan_time = np.float32(t - 0.003 * (np.arange(M) % 11) - 0.02 * (np.arange(M) % 3))
    return t, plan_time


# the kernel instantiation each case's plant runs on (dial_hip.hip: dial_ctx::inst)
INST = {"unitree_go2_trot": 1, "unitree_h1_jog": 2, "unitree_h1_loco": 3, "allegro_reorient": 4, "unitree_go2_crate_climb": 5,
        "unitree_h1_push_crate": 6}
PLANT_CASES = [pytest.param(ex, pd, None, id=f"{ex}-{pd}")
               for ex, pd in [("unitree_go2_trot", False), ("unitree_h1_jog", False), ("unitree_h1_loco", False), ("allegro_reorient", False),
                              ("unitree_go2_crate_climb", False), ("unitree_go2_trot", True), ("unitree_h1_jog", True),
                              ("unitree_h1_loco", True), ("unitree_go2_crate_climb", True), ("unitree_h1_push_crate", False),
                              ("unitree_h1_push_crate", True)]]
PLANT_CASES += [pytest.param(ex, pd, GEN, id=f"{ex}-{pd}-generic")
                for ex, pd in [("unitree_go2_trot", False), ("unitree_go2_trot", True), ("unitree_h1_loco", False)]]


@pytest.mark.parametrize("example,pd,options", PLANT_CASES)
def test_plant_matches_the_oracle(example, pd, options):
    """K = 4 steps at sim_dt = 0.005 of 64 plants against Oracle.rollout (fp32) over the same steps, each step's row chosen by
    ctrl_row on the host clock.  Gate per plant and step: within the per-rollout tolerance, or the whole plant reproduced by the oracle
    under <= 64 ulp of state jitter (rollout_jitter); the witnessed share is capped like the rollout tests'.
    options=GEN: the same on the capacity-dimension plant kernel (plant_kernel<DimsMax>), and then its final state after one K = 16
    launch without a trace against the oracle's state after the same 16 steps, under the same rule."""
    import oracle as O
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import ctrl_row
    env, model, task = _case(example, pd)
    M, K = 64, 4
    ctx = _lib.Context(model, task, None, device=0, options=options)
    assert ctx.debug_last_launch()["inst"] == (0 if options else INST[example])
    o32 = O.Oracle(model, task, None, np.float32)
    states = _start_states(ctx, env, M, seed=1)
    s0 = states.cpu().numpy().copy()
    rows = _rows(env, M, pd, seed=2)
    t, plan_time = _clocks(M)
    trace = _dev(np.zeros((M, K, 1 + ctx.nq + ctx.nv + ctx.nu)))
    ctx.plant_step(states, _dev(t, np.float64), _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, K, _lib.PLANT_PD if pd else _lib.PLANT_CTRL, trace)
    got_s, tr = states.cpu().numpy(), trace.cpu().numpy()
    nq, nv = ctx.nq, ctx.nv
    gpu_q = np.concatenate([tr[:, 1:, 1:1 + nq], got_s[:, None, :nq]], axis=1)           # state after step k, k = 0 .. K-1
    gpu_qd = np.concatenate([tr[:, 1:, 1 + nq:1 + nq + nv], got_s[:, None, nq:nq + nv]], axis=1)
    witnessed = []
    for m in range(M):
        tm, ks = t[m], []
        for _ in range(K):
            ks.append(ctrl_row(tm, plan_time[m], CTRL_DT, T))
            tm += SIM_DT
        us = (rows[m, ks] / np.float32(R))[None]

        def follows(roll):
            return _within(gpu_q[m], roll[1][0], TOL["q"]).all() and _within(gpu_qd[m], roll[2][0], TOL["qd"]).all()
        if follows(o32.rollout(s0[m], us)):
            continue
        assert any(follows(o32.rollout_jitter(s0[m], us, noise_seed=7919 * (j + 1), noise_mag=64.0)) for j in range(16)), \
            f"{example} {'PD' if pd else 'CTRL'}: plant {m} leaves the oracle and no jittered oracle run follows it"
        witnessed.append(m)
    assert len(witnessed) <= max(1, int(KNIFE_EDGE_FRAC[example] * M)), witnessed
    assert np.isfinite(got_s).all()
    if options:
        K2 = 16
        states = _start_states(ctx, env, M, seed=1)
        tt = _dev(t, np.float64)
        ctx.plant_step(states, tt, _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, K2, _lib.PLANT_PD if pd else _lib.PLANT_CTRL)
        got_s, t_end = states.cpu().numpy(), tt.cpu().numpy()
        verdicts = []
        for m in range(M):
            tm, ks = t[m], []
            for _ in range(K2):
                ks.append(ctrl_row(tm, plan_time[m], CTRL_DT, T))
                tm += SIM_DT
            assert t_end[m] == tm, m
            us = (rows[m, ks] / np.float32(R))[None]
            v = _final_follows_oracle(o32, s0[m], us, got_s[m, :nq], got_s[m, nq:nq + nv])
            assert v != "unwitnessed", f"{example} generic: plant {m}'s state after {K2} steps leaves the oracle and no jittered run follows it"
            verdicts.append(v)
        assert sum(v == "witnessed" for v in verdicts) <= max(1, int(KNIFE_EDGE_FRAC[example] * M)), verdicts


def _final_follows_oracle(o32, s0, us, q, qd):
    """A plant's final q / qd against the oracle's state after the same steps (Oracle.rollout): within the per-rollout tolerance
    (None), or reproduced by one of 16 oracle runs under <= 64 ulp of state jitter ("witnessed"), or neither ("unwitnessed")."""
    def follows(roll):
        return _within(q, roll[1][0][-1], TOL["q"]).all() and _within(qd, roll[2][0][-1], TOL["qd"]).all()
    if follows(o32.rollout(s0, us)):
        return None
    if any(follows(o32.rollout_jitter(s0, us, noise_seed=7919 * (j + 1), noise_mag=64.0)) for j in range(16)):
        return "witnessed"
    return "unwitnessed"


def _plant_ctx(example, options=None):
    from dial_mpc_amd import _lib
    env, model, task = _case(example, False)
    return env, _lib.Context(model, task, None, device=0, options=options)


@pytest.mark.parametrize("example,options", [pytest.param(ex, None, id=ex) for ex in ["unitree_go2_trot", "unitree_h1_loco", "unitree_go2_crate_climb",
                                                                                     "allegro_reorient", "unitree_h1_push_crate"]]
                         + [pytest.param("unitree_go2_trot", GEN, id="unitree_go2_trot-generic")])
def test_plant_bit_identities(example, options):
    """M plants in one launch = each plant alone; one K = 4 launch = four K = 1 launches (warm start included)."""
    import torch
    from dial_mpc_amd import _lib
    env, ctx = _plant_ctx(example, options)
    assert ctx.debug_last_launch()["inst"] == (0 if options else INST[example])
    M = 8
    s0 = _start_states(ctx, env, M, seed=3)
    rows, (t, plan_time) = _dev(_rows(env, M, False, seed=4)), _clocks(M)
    pt = _dev(plan_time)
    a, ta = s0.clone(), _dev(t, np.float64)
    ctx.plant_step(a, ta, pt, rows, CTRL_DT, SIM_DT, 4, _lib.PLANT_CTRL)
    for m in range(M):
        b, tb = s0[m:m + 1].clone(), _dev(t[m:m + 1], np.float64)
        ctx.plant_step(b, tb, pt[m:m + 1].contiguous(), rows[m:m + 1].contiguous(), CTRL_DT, SIM_DT, 4, _lib.PLANT_CTRL)
        assert torch.equal(a[m:m + 1], b) and torch.equal(ta[m:m + 1], tb), m
    c, tc = s0.clone(), _dev(t, np.float64)
    for _ in range(4):
        ctx.plant_step(c, tc, pt, rows, CTRL_DT, SIM_DT, 1, _lib.PLANT_CTRL)
    assert torch.equal(a, c) and torch.equal(ta, tc)


def test_plant_rows_and_clock_follow_the_host_rules():
    """DIAL_PLANT_CTRL: the trace's ctrl columns are the rows ctrl_row picks on the host, the advanced clock equals the host's fp64
    loop bit for bit and the trace's clock column is that clock rounded to float32 -- over 64 steps from clocks accumulated by 0.005
    (quotients next to integers) with plan times that lag them; sync mode (DIAL_PLANT_HOLD_FIRST) applies row 0 throughout."""
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import ctrl_row
    env, ctx = _plant_ctx("unitree_go2_trot")
    M, K, nu = 16, 64, ctx.nu
    states = _start_states(ctx, env, M, seed=5)
    rows = np.zeros((M, T, nu), np.float32)
    rows += (np.arange(T, dtype=np.float32) * 0.25 - 2.0)[None, :, None]      # row r carries the value r / 4 - 2 in every column
    t0 = np.zeros(M)
    for m in range(M):
        for _ in range(37 * m):
            t0[m] += SIM_DT
    plan_time = np.float32([t0[m] - [0.0, 0.005, 0.02, 0.0125, 0.3][m % 5] for m in range(M)])
    for flags in (_lib.PLANT_CTRL, _lib.PLANT_CTRL | _lib.PLANT_HOLD_FIRST):
        tt = _dev(t0, np.float64)
        trace = _dev(np.zeros((M, K, 1 + ctx.nq + ctx.nv + nu)))
        ctx.plant_step(states.clone(), tt, _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, K, flags, trace)
        tr, t_end = trace.cpu().numpy(), tt.cpu().numpy()
        for m in range(M):
            tm = t0[m]
            for k in range(K):
                r = 0 if flags & _lib.PLANT_HOLD_FIRST else ctrl_row(tm, plan_time[m], CTRL_DT, T)
                assert np.array_equal(tr[m, k, -nu:], rows[m, r]), (flags, m, k, r, tr[m, k, -1])
                assert tr[m, k, 0] == np.float32(tm), (m, k)
                tm += SIM_DT
            assert t_end[m] == tm, (m, t_end[m], tm)


def test_plant_argument_validation(tmp_path):
    import torch
    from dial_mpc_amd import _abi, _lib
    env, ctx = _plant_ctx("unitree_go2_trot")
    lib, h = ctx.lib, ctx.h
    st = _start_states(ctx, env, 2, seed=0)
    t = _dev([0.0, 0.0], np.float64)
    pt = _dev([0.0, 0.0])
    rows = _dev(np.zeros((2, T, ctx.nu)))
    ok = dict(states=st.data_ptr(), t=t.data_ptr(), pt=pt.data_ptr(), ctrl=rows.data_ptr(), T=T, K=1, flags=_lib.PLANT_CTRL, M=2,
              sim_dt=SIM_DT)
    stream = torch.cuda.current_stream().cuda_stream

    def call(c, **over):
        a = {**ok, **over}
        return lib.dial_plant_step(c, a["states"], a["t"], a["pt"], a["ctrl"], a["T"], CTRL_DT, a["sim_dt"], a["K"], a["flags"], None,
                                   a["M"], stream)
    ARG, UNSUP = _abi.MACROS["DIAL_ERR_ARG"], _abi.MACROS["DIAL_ERR_UNSUPPORTED"]
    assert call(h) == 0
    bad = [dict(states=None), dict(t=None), dict(pt=None), dict(ctrl=None), dict(K=0), dict(T=0), dict(M=0),
           dict(M=_abi.MACROS["DIAL_MAX_PLANTS"] + 1), dict(flags=0), dict(flags=_lib.PLANT_CTRL | _lib.PLANT_PD), dict(flags=8 | 1),
           dict(sim_dt=0.01), dict(sim_dt=0.02)]
    for b in bad:
        assert call(h, **b) == ARG, b
        assert lib.dial_last_error(h).decode().startswith("dial_plant_step: "), b
    assert lib.dial_plant_step(None, *[None] * 4, T, CTRL_DT, SIM_DT, 1, 1, None, 1, None) == ARG
    # position actuators (the Allegro): DIAL_PLANT_PD is refused
    a_env, a_model, a_task = _case("allegro_reorient", False)
    actx = _lib.Context(a_model, a_task, None, device=0)
    ast = _start_states(actx, a_env, 1, seed=0)
    with pytest.raises(_lib.DialHipError, match="position actuators"):
        actx.plant_step(ast, _dev([0.0], np.float64), _dev([0.0]), _dev(np.zeros((1, T, actx.nu))), CTRL_DT, SIM_DT, 1, _lib.PLANT_PD)
    # the IEEE measurement build has no plant
    _, model, task = _case("unitree_go2_trot", False)
    ictx = _lib.Context(model, task, None, device=0, lib_path=_lib.IEEE_LIB_PATH)
    with pytest.raises(_lib.DialHipError, match="IEEE measurement build") as e:
        ictx.plant_step(_start_states(ictx, env, 1, 0), _dev([0.0], np.float64), _dev([0.0]), _dev(np.zeros((1, T, ictx.nu))), CTRL_DT,
                        SIM_DT, 1, _lib.PLANT_CTRL)
    assert f"({UNSUP})" in str(e.value)
    # a library without libdialplant.so next to it
    lone = tmp_path / "libdialhip.so"
    shutil.copy(_lib.LIB_PATH, lone)
    lctx = _lib.Context(model, task, None, device=0, lib_path=str(lone))
    with pytest.raises(_lib.DialHipError, match="libdialplant.so") as e:
        lctx.plant_step(_start_states(lctx, env, 1, 0), _dev([0.0], np.float64), _dev([0.0]), _dev(np.zeros((1, T, lctx.nu))), CTRL_DT,
                        SIM_DT, 1, _lib.PLANT_CTRL)
    assert f"({UNSUP})" in str(e.value)


def test_plant_refuses_task_plugin_contexts():
    import importlib
    from dial_mpc_amd import _abi, _lib
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    import dial_mpc_amd.envs as dial_envs
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    mod = "dial_mpc_amd.examples.custom_env.go2_height_walk"
    importlib.reload(sys.modules[mod]) if mod in sys.modules else importlib.import_module(mod)
    try:
        d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk.yaml")))
        _, _, env = load_dial_and_env(d)
        model, task = env.make_model(), env.make_task()
        model.timestep = SIM_DT
        task.n_frames, task.dt = 1, SIM_DT
        ctx = _lib.Context(model, task, None, device=0, **env.context_kwargs())
        st = ctx.env_reset_batch(_dev(np.asarray(env._init_q, np.float32)[None]), _dev(np.zeros((1, ctx.nv))))
        with pytest.raises(_lib.DialHipError, match="task-plugin") as e:
            ctx.plant_step(st, _dev([0.0], np.float64), _dev([0.0]), _dev(np.zeros((1, T, ctx.nu))), CTRL_DT, SIM_DT, 1, _lib.PLANT_CTRL)
        assert f"({_abi.MACROS['DIAL_ERR_UNSUPPORTED']})" in str(e.value)
    finally:
        dial_envs._envs.clear()
        dial_envs._envs.update(saved[0])
        dial_envs._configs.clear()
        dial_envs._configs.update(saved[1])


def _upright(quat):
    w, x, y, z = quat
    return 1.0 - 2.0 * (x * x + y * y)   # z component of the body's up axis


def _closed_loop(example, ticks, fake: bool):
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.deploy.dial_plan import MBDPublisher
    from dial_mpc_amd.deploy.dial_sim import DialSim, DialSimConfig
    from dial_mpc_amd.utils.io_utils import get_example_path, load_dataclass_from_dict
    from fake_plant import FakePlant
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    d["sync_mode"] = True
    dial_config, env_config, env = load_dial_and_env(d)
    prefix = "p" + uuid.uuid4().hex[:8] + "_"
    qs = []
    if fake:
        plant = FakePlant(env, dial_config, shm_prefix=prefix)
        pub = MBDPublisher(env, env_config, dial_config, shm_prefix=prefix)

        def on_tick(k):
            plant.step_with_action(pub.Y[0])
            qs.append(plant.state.pipeline_state.qpos.cpu().numpy().copy())
    else:
        plant = DialSim(load_dataclass_from_dict(DialSimConfig, d), env_config, dial_config, env, shm_prefix=prefix)
        pub = MBDPublisher(env, env_config, dial_config, shm_prefix=prefix)

        def on_tick(k):
            assert plant.step_sync(poll=0) > 0
            qs.append(plant.plant.qpos_qvel()[: plant.nq].copy())
    try:
        pub.main_loop(max_ticks=ticks, on_tick=on_tick)
        pub.close()
    finally:
        plant.close()
    return np.array(qs)


def test_closed_loop_in_process():
    """DialSim (sync mode) and MBDPublisher in one process, 100 ticks: Go2 trot stays finite, above 0.2 m and upright, and makes at
    least half the forward progress of the same loop against FakePlant (the env stepped once per tick); H1 loco stands.
    Measured on an MI355X: Go2 min trunk height 0.216 m, min upright 0.980, progress 1.691 m (FakePlant 1.400 m); H1 loco min
    height 0.966 m, min upright 0.991."""
    q = _closed_loop("unitree_go2_trot_deploy", 100, fake=False)
    qf = _closed_loop("unitree_go2_trot_deploy", 100, fake=True)
    prog, prog_fake = q[-1, 0] - q[0, 0], qf[-1, 0] - qf[0, 0]
    print(f"go2 trot: min height {q[:, 2].min():.3f} m, min upright {min(_upright(x[3:7]) for x in q):.3f}, "
          f"progress {prog:.3f} m (FakePlant {prog_fake:.3f} m)")
    assert np.isfinite(q).all() and q[:, 2].min() > 0.2 and min(_upright(x[3:7]) for x in q) > 0.7
    assert prog_fake > 0 and prog >= 0.5 * prog_fake
    h = _closed_loop("unitree_h1_loco_deploy", 100, fake=False)
    print(f"h1 loco: min height {h[:, 2].min():.3f} m, min upright {min(_upright(x[3:7]) for x in h):.3f}")
    assert np.isfinite(h).all() and h[:, 2].min() > 0.7 and min(_upright(x[3:7]) for x in h) > 0.7


def test_sim2sim_two_processes(tmp_path):
    """dial_sim2sim with the Go2 trot deploy example for 2 s of sim time, record on: both children exit 0, the record has one
    [t, qpos, qvel, ctrl] row per sim step with t stepping by sim_dt, the robot stands, no segment is left behind."""
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path("unitree_go2_trot_deploy.yaml")))
    d["record"], d["output_dir"] = True, str(tmp_path / "out")
    cfg = tmp_path / "go2_trot_deploy.yaml"
    cfg.write_text(yaml.safe_dump(d))
    prefix = "s" + uuid.uuid4().hex[:8] + "_"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "dial_mpc_amd.core.dial_sim2sim", "--config", str(cfg), "--duration", "2",
                          "--shm-prefix", prefix], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    leftover = [f for f in os.listdir("/dev/shm") if f.startswith(prefix)]
    assert not leftover, leftover
    recs = [os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "out") for f in fs if f == "states.npy"]
    assert len(recs) == 1, out.stdout[-2000:]
    data = np.load(recs[0])
    nq, nv, nu = 19, 18, 12
    assert data.ndim == 2 and data.shape[1] == 1 + nq + nv + nu and data.shape[0] >= 390, data.shape
    assert np.allclose(np.diff(data[:, 0]), SIM_DT, atol=2e-6)
    assert np.isfinite(data).all() and data[-1, 1 + 2] > 0.2 and _upright(data[-1, 4:8]) > 0.7
    print(f"sim2sim: {data.shape[0]} steps, final height {data[-1, 3]:.3f} m, x {data[-1, 1]:.3f} m")
