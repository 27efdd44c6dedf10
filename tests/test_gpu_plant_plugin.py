"""GPU tests of the plant simulator of custom environments: dial_plant_step on contexts of task plugins built with plant=True
(csrc/plant_kernel.h: plant_kernel at the plugin's Dims, behind csrc/plant_plugin.h's table) -- DIAL_PLANT_CTRL / DIAL_PLANT_PD
against the fp32 oracle on the Go2 and the H1 push-crate
scene, DIAL_PLANT_LAW (the plugin's control law at every sim step) against the oracle's built-in PD law, the law's inputs bit for
bit through the trace's ctrl columns, the bit identities of all three modes, the refusals, and the go2_height_walk example in a
closed loop with the planner -- in one process and as dial-mpc-sim2sim."""
import importlib
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest
import yaml

from conftest import KNIFE_EDGE_FRAC, TOL, _within
from control_cases import CF, CPROBE_BAD, PERM, host_pd, params, task_consts
from dial_mpc_amd import _abi
from plant_plugin_cases import PLPROBE_BAD, build_plant_plugin, build_plant_plugins
from plugin_cases import build_matrix, load_case
from test_gpu_plant import CTRL_DT, R, ROOT, SIM_DT, T, _clocks, _dev, _rows, _start_states, _upright

pytestmark = pytest.mark.gpu

M_ = _abi.MACROS
IU, IUN = M_["DIAL_INFO_USER"], M_["DIAL_INFO_USER_N"]
ARG, UNSUP = M_["DIAL_ERR_ARG"], M_["DIAL_ERR_UNSUPPORTED"]
EXAMPLE = {"go2": "unitree_go2_trot", "h1_push_crate": "unitree_h1_push_crate"}   # the oracle's built-in task; KNIFE_EDGE_FRAC's key


@pytest.fixture(scope="module")
def plugins():
    return build_plant_plugins()


_loaded = {}


def _sim_case(name, pd=False, identity=True):
    """plugin_cases.load_case at sim rate: timestep = sim_dt, one physics step per step, in the plugin's task (kind USER) and in the
    oracle's built-in task.  identity: the oracle's action mapping made the identity up to the factor R, as tests/test_gpu_plant.py
    does (joint_offset 0, joint_range = phys_range = [-R, R], action_scale 1); pd: the oracle's task applies its PD law to the target,
    else hands it to the actuators as their ctrl.  identity=False: both tasks keep their true control constants."""
    if name not in _loaded:
        _loaded[name] = load_case(name, N=8, H=4)
    c = dict(_loaded[name])
    c["model"] = type(c["model"]).from_buffer_copy(c["model"])
    c["model"].timestep = SIM_DT
    for k in ("ptask", "otask"):
        t = c[k] = type(c[k]).from_buffer_copy(c[k])
        t.n_frames, t.dt = 1, SIM_DT
        t.position_control = 0 if pd else 1
        if identity:
            t.action_scale = 1.0
            for a in range(c["model"].nu):
                t.joint_offset[a] = 0.0
                t.joint_range[a][0], t.joint_range[a][1] = -R, R
                t.phys_range[a][0], t.phys_range[a][1] = -R, R
    return c


def _ctx(c, path, p=(), **kw):
    from dial_mpc_amd import _lib
    return _lib.Context(c["model"], c["ptask"], None, device=0, plugin=path, user_params=list(p), **kw)


def _picked(t0, plan_time, K, hold=False):
    """(rows the K steps from clock t0 apply, their clocks, the clock after them) by the host's rules."""
    from dial_mpc_amd.deploy.plant import ctrl_row
    tm, ks, ts = t0, [], []
    for _ in range(K):
        ks.append(0 if hold else ctrl_row(tm, plan_time, CTRL_DT, T))
        ts.append(tm)
        tm += SIM_DT
    return ks, ts, tm


def _oracle_gate(example, o32, s0, us_of, got_s, tr, nq, nv, t, plan_time, K, what):
    """The gate of test_plant_matches_the_oracle: per plant, every step within conftest.TOL of Oracle.rollout over the rows the host
    rule picks, or the whole plant reproduced by one of 16 oracle runs under <= 64 ulp of state jitter; the witnessed share is capped."""
    M = s0.shape[0]
    gpu_q = np.concatenate([tr[:, 1:, 1:1 + nq], got_s[:, None, :nq]], axis=1)
    gpu_qd = np.concatenate([tr[:, 1:, 1 + nq:1 + nq + nv], got_s[:, None, nq:nq + nv]], axis=1)
    witnessed = []
    for m in range(M):
        ks, _, _ = _picked(t[m], plan_time[m], K)
        us = us_of(m, ks)[None]

        def follows(roll):
            return _within(gpu_q[m], roll[1][0], TOL["q"]).all() and _within(gpu_qd[m], roll[2][0], TOL["qd"]).all()
        if follows(o32.rollout(s0[m], us)):
            continue
        assert any(follows(o32.rollout_jitter(s0[m], us, noise_seed=7919 * (j + 1), noise_mag=64.0)) for j in range(16)), \
            f"{what}: plant {m} leaves the oracle and no jittered oracle run follows it"
        witnessed.append(m)
    print(f"{what}: {len(witnessed)} of {M} plants witnessed")
    assert len(witnessed) <= max(1, int(KNIFE_EDGE_FRAC[example] * M)), witnessed
    assert np.isfinite(got_s).all()


@pytest.mark.parametrize("name,pd", [("go2", False), ("go2", True), ("h1_push_crate", False), ("h1_push_crate", True)])
def test_plugin_plant_matches_the_oracle(plugins, name, pd):
    """4. K = 4 steps at sim_dt = 0.005 of 64 plants on the plugin's plant kernel (task kind USER) against Oracle.rollout (fp32) of
    the built-in task over the same steps, exactly as test_plant_matches_the_oracle: identity action mapping with R = 64, dyadic
    rows, rows chosen by ctrl_row on the host clock, the same gate and the same cap on witnessed plants."""
    import oracle as O
    from dial_mpc_amd import _lib
    c = _sim_case(name, pd)
    M, K = 64, 4
    ctx = _ctx(c, plugins[(name, None)])
    assert ctx.debug_last_launch()["inst"] == 7
    o32 = O.Oracle(c["model"], c["otask"], None, np.float32)
    states = _start_states(ctx, c["env"], M, seed=1)
    s0 = states.cpu().numpy().copy()
    rows = _rows(c["env"], M, pd, seed=2)
    t, plan_time = _clocks(M)
    trace = _dev(np.zeros((M, K, 1 + ctx.nq + ctx.nv + ctx.nu)))
    ctx.plant_step(states, _dev(t, np.float64), _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, K, _lib.PLANT_PD if pd else _lib.PLANT_CTRL, trace)
    _oracle_gate(EXAMPLE[name], o32, s0, lambda m, ks: rows[m, ks] / np.float32(R), states.cpu().numpy(), trace.cpu().numpy(),
                 ctx.nq, ctx.nv, t, plan_time, K, f"{name} {'PD' if pd else 'CTRL'}")


def test_plugin_plant_law_matches_the_oracles_pd(plugins):
    """5. DIAL_PLANT_LAW with the probe law's mode 0 (BaseEnv's torque law restated) on the Go2, the task with its true constants,
    rows uniform in [-0.8, 0.8]: the plant against the oracle running its built-in PD law at n_frames = 1, dt = sim_dt over the rows
    ctrl_row picks -- the same gate as above -- and the first step's ctrl against the law in fp64 within control_cases.host_pd's bound."""
    import oracle as O
    from dial_mpc_amd import _lib
    c = _sim_case("go2", pd=True, identity=False)
    M, K = 64, 4
    ctx = _ctx(c, plugins[("go2", "probe")], params(0))
    nq, nv, nu = ctx.nq, ctx.nv, ctx.nu
    o32 = O.Oracle(c["model"], c["otask"], None, np.float32)
    states = _start_states(ctx, c["env"], M, seed=11)
    s0 = states.cpu().numpy().copy()
    rows = np.random.default_rng(12).uniform(-0.8, 0.8, (M, T, nu)).astype(np.float32)
    t, plan_time = _clocks(M)
    trace = _dev(np.zeros((M, K, 1 + nq + nv + nu)))
    ctx.plant_step(states, _dev(t, np.float64), _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, K, _lib.PLANT_LAW, trace)
    tr = trace.cpu().numpy()
    k = task_consts(c["ptask"], nu)
    worst = 0.0
    for m in range(M):
        ks, _, _ = _picked(t[m], plan_time[m], K)
        tau, bound = host_pd(k, s0[m, :nq], s0[m, nq:nq + nv], rows[m, ks[0]], 7 + np.arange(nu), 6 + np.arange(nu))
        err = np.abs(tr[m, 0, -nu:].astype(np.float64) - tau)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (m, err.tolist(), bound.tolist())
        assert np.array_equal(tr[m, 0, 1:1 + nq + nv], s0[m, :nq + nv])   # the trace row is the state before the step
    print(f"go2 LAW: first step's ctrl within {worst:.3f} of host_pd's bound")
    _oracle_gate(EXAMPLE["go2"], o32, s0, lambda m, ks: rows[m, ks], states.cpu().numpy(), tr, nq, nv, t, plan_time, K, "go2 LAW")


def _accumulated_clocks(M):
    t0 = np.zeros(M)
    for m in range(M):
        for _ in range(37 * m):
            t0[m] += SIM_DT
    plan_time = np.float32([t0[m] - [0.0, 0.005, 0.02, 0.0125, 0.3][m % 5] for m in range(M)])
    return t0, plan_time


def test_law_inputs_through_the_trace(plugins):
    """6. The probe law's field mode: every lane returns one element of the law's input, so the trace's ctrl columns show what the
    law saw at each of 64 steps of 16 plants, from clocks accumulated by 0.005 (quotients by ctrl_dt next to integers).  Bit for bit:
    step = law_step(t_k, ctrl_dt) and dt = float32(ctrl_dt); qpos / qvel are the trace's own pre-step values; act is the row the row
    rule picked (row 0 under DIAL_PLANT_HOLD_FIRST, with the same step rule); info_user are the state's slots, which -- like every
    info word -- the launch leaves as they were; the table row under clamp and wrap with a non-zero row0 is
    table[table_row(step, ...)] (tests/plant_law_probe.hip)."""
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import law_step
    from dial_mpc_amd.envs.custom_env import table_row
    c = _sim_case("go2", pd=True, identity=False)
    M, K = 16, 64
    ctx = _ctx(c, plugins[("go2", "probe")], params(4))
    nq, nv, nu = ctx.nq, ctx.nv, ctx.nu
    info = nq + 2 * nv
    base = _start_states(ctx, c["env"], M, seed=5)
    slots = (np.arange(M * IUN, dtype=np.float32).reshape(M, IUN) * 0.5 - 7.0)
    base[:, info + IU:info + IU + IUN] = _dev(slots)
    rows = ((np.arange(T)[None, :, None] * 32 + np.arange(nu)[None, None, :]) / 1024.0 + np.arange(M)[:, None, None]).astype(np.float32)
    t0, plan_time = _accumulated_clocks(M)

    def run(cx, flags):
        st, tt = base.clone(), _dev(t0, np.float64)
        trace = _dev(np.zeros((M, K, 1 + nq + nv + nu)))
        cx.plant_step(st, tt, _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, K, flags, trace)
        return trace.cpu().numpy(), tt.cpu().numpy(), st.cpu().numpy()

    def probe(field, idx=0, flags=_lib.PLANT_LAW):
        ctx.set_user_params(params(4, 0, 0, CF[field], idx))
        return run(ctx, flags)

    clocks = [_picked(t0[m], plan_time[m], K) for m in range(M)]
    steps = np.array([[law_step(tk, CTRL_DT) for tk in clocks[m][1]] for m in range(M)])
    assert steps.min() == 0 and steps.max() > 100 and len({int(s) for s in steps.ravel()}) > 100
    for flags in (_lib.PLANT_LAW, _lib.PLANT_LAW | _lib.PLANT_HOLD_FIRST):
        tr, t_end, st = probe("step", flags=flags)
        for m in range(M):
            assert np.array_equal(tr[m, :, -nu:], np.repeat(np.float32(steps[m])[:, None], nu, 1)), (flags, m)
            assert np.array_equal(tr[m, :, 0], np.float32(clocks[m][1])) and t_end[m] == clocks[m][2], (flags, m)
        assert np.array_equal(st[:, info:], base.cpu().numpy()[:, info:])   # the info words are not written
        tr, _, _ = probe("act", 5, flags=flags)
        for m in range(M):
            ks = _picked(t0[m], plan_time[m], K, hold=bool(flags & _lib.PLANT_HOLD_FIRST))[0]
            assert np.array_equal(tr[m, :, -nu:], np.repeat(rows[m, ks, 5][:, None], nu, 1)), (flags, m)
    tr, _, _ = probe("dt")
    assert np.float32(CTRL_DT) != np.float32(SIM_DT) and np.all(tr[:, :, -nu:] == np.float32(CTRL_DT))
    for field, idx, col in [("qpos", 2, 1 + 2), ("qpos", 7 + 4, 1 + 7 + 4), ("qvel", 0, 1 + nq), ("qvel", 6 + 9, 1 + nq + 6 + 9)]:
        tr, _, _ = probe(field, idx)
        assert np.isfinite(tr).all()
        assert np.array_equal(tr[:, :, -nu:], np.repeat(tr[:, :, col:col + 1], nu, 2)), (field, idx)
        assert len(np.unique(tr[:, :, col])) > M   # (the state moves: the law reads the plant's CURRENT state at every step)
    for idx in (0, 3, IUN - 1, IUN):
        tr, _, _ = probe("info_user", idx)
        want = slots[:, idx] if idx < IUN else np.full(M, np.float32(CPROBE_BAD))
        assert np.array_equal(tr[:, :, -nu:], np.broadcast_to(want[:, None, None], (M, K, nu))), idx
    tr, _, _ = probe("lane")
    assert np.array_equal(tr[:, :, -nu:], np.broadcast_to(np.arange(nu, dtype=np.float32), (M, K, nu)))
    tr, _, _ = probe("nq")
    assert np.all(tr[:, :, -nu:] == nq)
    # the reference table's row, read straight from global memory
    tctx = _ctx(c, plugins[("go2", "table")], [0.0, 0.0, 0.0])
    tr, _, _ = run(tctx, _lib.PLANT_LAW)
    assert np.all(tr[:, :, -nu:] == np.float32(PLPROBE_BAD))   # no table bound
    for rows_n, row0, mode in [(150, -3, "clamp"), (7, 5, "wrap"), (1, 9, "clamp")]:
        table = (np.arange(rows_n, dtype=np.float32)[:, None] * 100.0 + np.arange(nu, dtype=np.float32)[None, :])
        tctx.set_user_table(table, row0, mode)
        idx = np.array([[table_row(int(s), row0, rows_n, mode) for s in steps[m]] for m in range(M)])
        if rows_n == 150:
            assert idx.min() == 0 and idx.max() == rows_n - 1 and len(np.unique(idx)) == rows_n   # both clamps and everything between
        for pmode, want in [(0, table[idx]), (1, np.repeat(idx[:, :, None], nu, 2).astype(np.float32)),
                            (4, np.broadcast_to(table[-1], (M, K, nu)))]:
            tctx.set_user_params([0.0, 0.0, float(pmode)])
            tr, _, _ = run(tctx, _lib.PLANT_LAW)
            assert np.array_equal(tr[:, :, -nu:], want), (rows_n, row0, mode, pmode)


@pytest.mark.parametrize("name,mode", [("go2", "CTRL"), ("go2", "PD"), ("go2", "LAW"), ("h1_push_crate", "LAW")])
def test_plugin_plant_bit_identities(plugins, name, mode):
    """7. M plants in one launch = each plant alone; one K = 4 launch = four K = 1 launches (warm start included); the advanced
    clock = the host's fp64 loop.  On the plugin with the probe law, in each of the three modes (LAW: the restated torque law)."""
    import torch
    from dial_mpc_amd import _lib
    c = _sim_case(name, pd=True, identity=False)
    ctx = _ctx(c, plugins[(name, "probe")], params(0))
    flags = dict(CTRL=_lib.PLANT_CTRL, PD=_lib.PLANT_PD, LAW=_lib.PLANT_LAW)[mode]
    M = 8
    s0 = _start_states(ctx, c["env"], M, seed=3)
    if mode == "LAW":
        rows = _dev(np.random.default_rng(4).uniform(-0.8, 0.8, (M, T, ctx.nu)))
    else:
        rows = _dev(_rows(c["env"], M, mode == "PD", seed=4))
    t, plan_time = _clocks(M)
    pt = _dev(plan_time)
    a, ta = s0.clone(), _dev(t, np.float64)
    ctx.plant_step(a, ta, pt, rows, CTRL_DT, SIM_DT, 4, flags)
    assert torch.isfinite(a).all() and not torch.equal(a[:, :ctx.nq], s0[:, :ctx.nq])
    for m in range(M):
        b, tb = s0[m:m + 1].clone(), _dev(t[m:m + 1], np.float64)
        ctx.plant_step(b, tb, pt[m:m + 1].contiguous(), rows[m:m + 1].contiguous(), CTRL_DT, SIM_DT, 4, flags)
        assert torch.equal(a[m:m + 1], b) and torch.equal(ta[m:m + 1], tb), m
    cst, tc = s0.clone(), _dev(t, np.float64)
    for _ in range(4):
        ctx.plant_step(cst, tc, pt, rows, CTRL_DT, SIM_DT, 1, flags)
    assert torch.equal(a, cst) and torch.equal(ta, tc)
    t_end = ta.cpu().numpy()
    for m in range(M):
        assert t_end[m] == _picked(t[m], plan_time[m], 4)[2], m


def test_plugin_plant_refusals(plugins):
    """8. What dial_plant_step and dial_create_plugin refuse, each with its code and a message that starts with its entry point's name."""
    from conftest import setup_case
    from dial_mpc_amd import _lib
    c = _sim_case("go2")
    zeros = lambda cx, n=1: (_dev([0.0] * n, np.float64), _dev([0.0] * n), _dev(np.zeros((n, T, cx.nu))))   # noqa: E731

    def refused(cx, flags, code, match):
        st = _start_states(cx, c["env"], 1, seed=0)
        with pytest.raises(_lib.DialHipError, match=match) as e:
            cx.plant_step(st, *zeros(cx), CTRL_DT, SIM_DT, 1, flags)
        assert f"({code})" in str(e.value) and cx.lib.dial_last_error(cx.h).decode().startswith("dial_plant_step: "), str(e.value)

    # a plugin built the ordinary way: no plant, whatever the mode asks for
    plain = _ctx(c, build_matrix(["go2"])["go2"])
    refused(plain, _lib.PLANT_CTRL, UNSUP, r"dial_plant_step: task-plugin.*build_plugin\(plant=True\)")
    refused(plain, _lib.PLANT_PD, UNSUP, r"dial_plant_step: task-plugin.*build_plugin\(plant=True\)")
    # DIAL_PLANT_LAW: combined with another mode, on a built-in context, on a plugin without a law, with per-plan rows bound
    law = _ctx(c, plugins[("go2", "probe")], params(0))
    nolaw = _ctx(c, plugins[("go2", None)])
    _, _, bmodel, btask, _ = setup_case("unitree_go2_trot", 8, 4, per_rollout=True)
    bmodel.timestep = SIM_DT
    btask.n_frames, btask.dt = 1, SIM_DT
    builtin = _lib.Context(bmodel, btask, None, device=0)
    for combo in (_lib.PLANT_LAW | _lib.PLANT_CTRL, _lib.PLANT_LAW | _lib.PLANT_PD, _lib.PLANT_LAW | 16, _lib.PLANT_HOLD_FIRST):
        refused(law, combo, ARG, "exactly one of")
    refused(builtin, _lib.PLANT_LAW, ARG, "without a task plugin")
    refused(nolaw, _lib.PLANT_LAW, ARG, "without a user control law")
    refused(plain, _lib.PLANT_LAW, ARG, "without a user control law")
    law.set_plan_params(np.zeros((1, 6), np.float32))
    refused(law, _lib.PLANT_LAW, ARG, "per-plan task parameters")
    st = _start_states(law, c["env"], 1, seed=0)
    law.plant_step(st, *zeros(law), CTRL_DT, SIM_DT, 1, _lib.PLANT_CTRL)    # (the other modes read no parameters)
    law.set_plan_params(None)
    law.plant_step(st, *zeros(law), CTRL_DT, SIM_DT, 1, _lib.PLANT_LAW)
    # the argument checks of the built-in plant hold for a plugin context too
    refused(law, 0, ARG, "exactly one of")
    with pytest.raises(_lib.DialHipError, match="sim_dt differs"):
        law.plant_step(st, *zeros(law), CTRL_DT, 0.01, 1, _lib.PLANT_LAW)
    # DIAL_PLANT_PD on a plugin context whose actuators do not follow the PD law's joint indexing (the Go2 with permuted actuators)
    md = dict(c["md"])
    for k in [k for k in md if k.startswith("act_")]:
        md[k] = np.asarray(md[k])[PERM]
    pmodel = _abi.make_model(md)
    pmodel.timestep = SIM_DT
    perm = _lib.Context(pmodel, c["ptask"], None, device=0, plugin=plugins[("go2", None)])
    refused(perm, _lib.PLANT_PD, ARG, r"qpos\[7 \+ a\]")
    pst = _start_states(perm, c["env"], 1, seed=0)
    perm.plant_step(pst, *zeros(perm), CTRL_DT, SIM_DT, 1, _lib.PLANT_CTRL)
    # the IEEE measurement build carries no plant, with or without the plugin's table
    ieee = _lib.Context(c["model"], c["ptask"], None, device=0, plugin=plugins[("go2", None)], lib_path=_lib.IEEE_LIB_PATH)
    ist = _start_states(ieee, c["env"], 1, seed=0)
    with pytest.raises(_lib.DialHipError, match="dial_plant_step: the IEEE measurement build") as e:
        ieee.plant_step(ist, *zeros(ieee), CTRL_DT, SIM_DT, 1, _lib.PLANT_CTRL)
    assert f"({UNSUP})" in str(e.value)
    # a plugin whose plant table reports another version
    stale = build_plant_plugin("go2", None, version=99)
    with pytest.raises(_lib.DialHipError, match=r"dial_create_plugin: stale plugin: its plant table reports version 99") as e:
        _ctx(c, stale)
    assert f"({ARG})" in str(e.value)


# ---- 9. the go2_height_walk example in a closed loop
EX_MOD = "dial_mpc_amd.examples.custom_env.go2_height_walk"
EX_CFG = os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk_deploy.yaml")


def test_custom_env_closed_loop_in_process():
    """DialSim (sync mode: Plant on the plugin's plant kernel) and MBDPublisher in one process, 10 ticks, Nsample reduced: the robot
    stays finite, above 0.2 m and upright, and the plant's clock advances by about one control step per tick.
    Measured on an MI355X: min trunk height 0.255 m, min upright 0.999, t = 0.230 s after 10 ticks."""
    import dial_mpc_amd.envs as dial_envs
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.deploy.dial_plan import MBDPublisher
    from dial_mpc_amd.deploy.dial_sim import DialSim, DialSimConfig
    from dial_mpc_amd.utils.io_utils import load_dataclass_from_dict
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    importlib.reload(sys.modules[EX_MOD]) if EX_MOD in sys.modules else importlib.import_module(EX_MOD)
    plant = None
    try:
        d = yaml.safe_load(open(EX_CFG))
        d.update(Nsample=256, sync_mode=True)
        dial_config, env_config, env = load_dial_and_env(d)
        prefix = "q" + uuid.uuid4().hex[:8] + "_"
        plant = DialSim(load_dataclass_from_dict(DialSimConfig, d), env_config, dial_config, env, shm_prefix=prefix)
        assert plant.plant.ctx.plugin == env.plant_plugin_path() != env.plugin_path()
        pub = MBDPublisher(env, env_config, dial_config, shm_prefix=prefix)
        qs = []

        def on_tick(k):
            assert plant.step_sync(poll=0) > 0
            qs.append(plant.plant.qpos_qvel()[: plant.nq].copy())
        pub.main_loop(max_ticks=10, on_tick=on_tick)
        pub.close()
        q = np.array(qs)
        print(f"go2_height_walk: min height {q[:, 2].min():.3f} m, min upright {min(_upright(x[3:7]) for x in q):.3f}, t = {plant.t:.3f} s")
        assert q.shape[0] == 10 and np.isfinite(q).all() and q[:, 2].min() > 0.2 and min(_upright(x[3:7]) for x in q) > 0.7
        # (sync_steps: a tick runs while t <= plan_time + ctrl_dt, i.e. four or five sim steps -- one control step, or one sim step more)
        assert 10 * CTRL_DT <= plant.t <= 10 * (CTRL_DT + SIM_DT) + SIM_DT
    finally:
        if plant is not None:
            plant.close()
        dial_envs._envs.clear()
        dial_envs._envs.update(saved[0])
        dial_envs._configs.clear()
        dial_envs._configs.update(saved[1])


def test_custom_env_sim2sim_two_processes(tmp_path):
    """dial-mpc-sim2sim --custom-env go2_height_walk for 0.1 s of sim time, record on: exit status 0, one [t, qpos, qvel, ctrl] row
    per sim step, the robot stands, no segment is left behind."""
    d = yaml.safe_load(open(EX_CFG))
    d.update(Nsample=256, record=True, output_dir=str(tmp_path / "out"))
    cfg = tmp_path / "go2_height_walk_deploy.yaml"
    cfg.write_text(yaml.safe_dump(d))
    prefix = "r" + uuid.uuid4().hex[:8] + "_"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "dial_mpc_amd.core.dial_sim2sim", "--custom-env", EX_MOD, "--config", str(cfg),
                          "--duration", "0.1", "--shm-prefix", prefix], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert not [f for f in os.listdir("/dev/shm") if f.startswith(prefix)]
    recs = [os.path.join(r, f) for r, _, fs in os.walk(tmp_path / "out") for f in fs if f == "states.npy"]
    assert len(recs) == 1, out.stdout[-2000:]
    data = np.load(recs[0])
    nq, nv, nu = 19, 18, 12
    assert data.ndim == 2 and data.shape[1] == 1 + nq + nv + nu and data.shape[0] >= 19, data.shape
    assert np.allclose(np.diff(data[:, 0]), SIM_DT, atol=2e-6)
    assert np.isfinite(data).all() and data[-1, 1 + 2] > 0.2 and _upright(data[-1, 4:8]) > 0.7
