"""GPU tests of plant disturbances: dial_plant_step with a buffer bound by dial_set_plant_disturbance (csrc/plant_dist_kernel.h in
libdialplantdist.so, and in a task plugin built with plant_disturbance=True) against the UNDISTURBED plant kernel, bit for bit --
identity data, kicks composed with host additions between undisturbed launches, the actuator error against rows disturbed on the host
and against a single-rounded fma of the undisturbed ctrl, per-plant independence -- and the refusals.
M = 8 plants, K = 4 steps at sim_dt = 0.005, the dyadic rows and clocks of tests/test_gpu_plant.py restated here."""
import math
import shutil
from fractions import Fraction

import numpy as np
import pytest

from conftest import setup_case
from control_cases import params
from dial_mpc_amd import _abi
from plant_dist_cases import build_dist_plugin, pack
from plant_plugin_cases import build_plant_plugin
from plugin_cases import load_case

pytestmark = pytest.mark.gpu

SIM_DT, CTRL_DT, T, R = 0.005, 0.02, 17, 64.0
M, K = 8, 4
ARG, UNSUP = _abi.MACROS["DIAL_ERR_ARG"], _abi.MACROS["DIAL_ERR_UNSUPPORTED"]
GEN = dict(force_generic=1)   # dial_options: the capacity-dimension instantiation (DimsMax, kernel instantiation 0)
# the kernel instantiation each built-in case's plant runs on (dial_ctx::inst)
INST = {"unitree_go2_trot": 1, "unitree_h1_jog": 2, "unitree_h1_loco": 3, "allegro_reorient": 4, "unitree_go2_crate_climb": 5,
        "unitree_h1_push_crate": 6}
ALL_INSTS = ["unitree_go2_trot", "unitree_h1_jog", "unitree_h1_loco", "allegro_reorient", "unitree_go2_crate_climb", "unitree_h1_push_crate",
             "generic", "plugin"]
KICK_CASES = ["unitree_go2_trot", "unitree_h1_loco", "allegro_reorient", "unitree_h1_push_crate", "generic", "plugin"]


def _dev(x, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda:0")


_made = {}


def _make(case):
    """(env, context) of a case, one per module run: an example's name (its own instantiation), "generic" (the Go2 on the
    capacity-dimension kernel), "plugin" / "plugin-law" (the Go2 probe plugin with the disturbed plant kernel, without / with the probe
    law in its torque-law mode) and "plugin-plant-only" (the plant=True sibling, which has no disturbed kernel).  The model runs at
    sim_dt with one physics step per step, as env.make_plant builds it."""
    from dial_mpc_amd import _lib
    if case in _made:
        return _made[case]
    if case.startswith("plugin"):
        c = load_case("go2", N=8, H=4)
        model, task = type(c["model"]).from_buffer_copy(c["model"]), type(c["ptask"]).from_buffer_copy(c["ptask"])
        model.timestep = SIM_DT
        task.n_frames, task.dt = 1, SIM_DT
        law = "probe" if case == "plugin-law" else None
        path = build_plant_plugin("go2", None) if case == "plugin-plant-only" else build_dist_plugin("go2", law)
        ctx = _lib.Context(model, task, None, device=0, plugin=path, user_params=params(0) if law else [])
        assert ctx.debug_last_launch()["inst"] == 7
        env = c["env"]
    else:
        example = "unitree_go2_trot" if case == "generic" else case
        _, env, model, task, _ = setup_case(example, 8, 4, per_rollout=True)
        model.timestep = SIM_DT
        task.n_frames, task.dt = 1, SIM_DT
        ctx = _lib.Context(model, task, None, device=0, options=GEN if case == "generic" else None)
        assert ctx.debug_last_launch()["inst"] == (0 if case == "generic" else INST[example])
    _made[case] = (env, ctx)
    return env, ctx


def _act_q(model):
    return [int(model.act_qposadr[a]) for a in range(model.nu)]


def _positional(ctx):
    return any(ctx.model.act_isposition[a] for a in range(ctx.nu))


def _start_states(ctx, env, seed):
    """The env's initial pose plus seeded perturbations of the actuated joints and of every velocity (plant 0: the pose itself)."""
    rng = np.random.default_rng(seed)
    qpos = np.tile(np.asarray(env._init_q, np.float32), (M, 1))
    qvel = np.zeros((M, ctx.nv), np.float32)
    qpos[1:, _act_q(ctx.model)] += rng.uniform(-0.1, 0.1, (M - 1, ctx.nu)).astype(np.float32)
    qvel[1:] = rng.uniform(-0.3, 0.3, (M - 1, ctx.nv)).astype(np.float32)
    return ctx.env_reset_batch(_dev(qpos), _dev(qvel))


def _rows(ctx, env, target, seed):
    """[M, T, nu] dyadic rows: torques k / 8, or -- target -- joint targets near the initial pose on a 1/256 grid."""
    rng = np.random.default_rng(seed)
    if target:
        base = np.round(np.asarray(env._init_q, np.float64)[_act_q(ctx.model)] * 256) / 256
        return (base + rng.integers(-64, 65, (M, T, ctx.nu)) / 256).astype(np.float32)
    return (rng.integers(-160, 161, (M, T, ctx.nu)) / 8).astype(np.float32)


def _clocks():
    t = np.array([0.005 * (m % 9) + 0.3 for m in range(M)])
    plan_time = np.float32(t - 0.003 * (np.arange(M) % 11) - 0.02 * (np.arange(M) % 3))
    return t, plan_time


def _step_clocks(t):
    """[M, K] the clock of every plant before each of the K steps, by the kernel's own fp64 additions."""
    out = np.zeros((M, K))
    for m in range(M):
        tm = t[m]
        for k in range(K):
            out[m, k] = tm
            tm += SIM_DT
    return out


def _window(clock):
    """A float32 window that holds `clock` and no other step's clock: half a step to either side."""
    return float(np.float32(clock - 0.5 * SIM_DT)), float(np.float32(clock + 0.5 * SIM_DT))


def _run(ctx, s0, t, plan_time, rows, flags, k=K, sel=slice(None)):
    """One launch of k steps from copies of (s0, t) -> (states, clocks, trace), device tensors."""
    st, tt = s0[sel].clone(), _dev(t[sel], np.float64)
    n = st.shape[0]
    trace = _dev(np.zeros((n, k, 1 + ctx.nq + ctx.nv + ctx.nu)))
    ctx.plant_step(st, tt, _dev(plan_time[sel]), rows[sel].contiguous(), CTRL_DT, SIM_DT, k, flags, trace)
    return st, tt, trace


def _bind(ctx, gains, biases, events):
    rows, E = pack(ctx.nu, ctx.nv, gains, biases, events)
    return ctx.set_plant_disturbance(_dev(rows), E)


def _modes(case, ctx):
    from dial_mpc_amd import _lib
    if case == "plugin-law":
        return [("LAW", _lib.PLANT_LAW)]
    return [("CTRL", _lib.PLANT_CTRL)] + ([] if _positional(ctx) else [("PD", _lib.PLANT_PD)])


def _mode_rows(case, ctx, env, mode, seed):
    if mode == "LAW":
        return np.random.default_rng(seed).uniform(-0.8, 0.8, (M, T, ctx.nu)).astype(np.float32)
    return _rows(ctx, env, mode == "PD" or _positional(ctx), seed)


@pytest.mark.parametrize("case", ALL_INSTS + ["plugin-law"])
def test_identity_data_gives_the_undisturbed_plant(case):
    """Gain 1, bias 0 and three event slots whose windows miss every step (one long past, one far ahead, one empty; each with a
    non-zero dv, so that a firing would show): states, clocks and trace equal the unbound run with torch.equal, in every mode the
    case has."""
    import torch
    env, ctx = _make(case)
    s0 = _start_states(ctx, env, seed=3)
    t, plan_time = _clocks()
    dv = (np.arange(ctx.nv) + 1) / 64.0
    events = [[(0.1, 0.2, dv), (10.0, 11.0, -dv), (0.32, 0.32, dv)] for _ in range(M)]
    ones, zeros = np.ones((M, ctx.nu)), np.zeros((M, ctx.nu))
    try:
        for mode, flags in _modes(case, ctx):
            rows = _dev(_mode_rows(case, ctx, env, mode, seed=4))
            ctx.set_plant_disturbance(None)
            a = _run(ctx, s0, t, plan_time, rows, flags)
            _bind(ctx, ones, zeros, events)
            b = _run(ctx, s0, t, plan_time, rows, flags)
            assert torch.isfinite(a[0]).all() and not torch.equal(a[0][:, :ctx.nq], s0[:, :ctx.nq]), mode
            for what, x, y in zip(("states", "clocks", "trace"), a, b):
                assert torch.equal(x, y), (case, mode, what)
    finally:
        ctx.set_plant_disturbance(None)


@pytest.mark.parametrize("case", KICK_CASES)
def test_kicks_compose_with_host_additions_between_undisturbed_launches(case):
    """Plant m's event fires at step m % 4 only (its window: that step's clock +- half a step), dv on a 1/64 grid over all dofs (the
    Allegro: over the cube's dofs); plant 0 has a second, overlapping event.  ONE disturbed K = 4 launch equals, bit for bit, the
    undisturbed sequence: per step, a float32 `qvel += dv` on the host for the plants that fire (plant 0: its two events in index
    order), then one undisturbed K = 1 launch -- final states, clocks and every trace row (the clock, the kicked qvel, the ctrl)."""
    import torch
    from dial_mpc_amd import _lib
    env, ctx = _make(case)
    nq, nv, nu = ctx.nq, ctx.nv, ctx.nu
    s0 = _start_states(ctx, env, seed=5)
    rows = _dev(_rows(ctx, env, _positional(ctx), seed=6))
    t, plan_time = _clocks()
    clocks = _step_clocks(t)
    rng = np.random.default_rng(7)
    dofs = np.arange(nv)
    if case == "allegro_reorient":
        dofs = np.array(sorted(set(range(nv)) - {int(ctx.model.act_dofadr[a]) for a in range(nu)}))
        assert len(dofs) == 6   # the cube's free joint
    events, fire = [], []
    for m in range(M):
        k = m % 4
        dv = np.zeros(nv)
        dv[dofs] = rng.integers(-8, 9, len(dofs)) / 64.0
        evs = [(*_window(clocks[m, k]), dv)]
        if m == 0:
            dv2 = np.zeros(nv)
            dv2[dofs] = rng.integers(-8, 9, len(dofs)) / 64.0
            # (a narrower window inside the first one: both fire at that step, neither at another)
            evs.append((float(np.float32(clocks[m, k] - 0.4 * SIM_DT)), float(np.float32(clocks[m, k] + 0.4 * SIM_DT)), dv2))
        events.append(evs)
        fire.append(k)
    from dial_mpc_amd.deploy.plant import event_fires
    for m in range(M):   # the host restatement agrees on which steps fire
        for k in range(K):
            assert [event_fires(clocks[m, k], e[0], e[1]) for e in events[m]] == [k == fire[m]] * len(events[m]), (m, k)
    try:
        _bind(ctx, np.ones((M, nu)), np.zeros((M, nu)), events)
        got_s, got_t, got_tr = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)
        ctx.set_plant_disturbance(None)
        plain_s, _, _ = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)
        assert not torch.equal(got_s, plain_s)   # the kicks do something
        st, tt = s0.clone(), _dev(t, np.float64)
        pt = _dev(plan_time)
        for k in range(K):
            host = st.cpu().numpy()
            for m in range(M):
                if fire[m] == k:
                    for _, _, dv in events[m]:
                        host[m, nq:nq + nv] = host[m, nq:nq + nv] + dv.astype(np.float32)   # one float32 addition per dof, in index order
            st = _dev(host)
            trace = _dev(np.zeros((M, 1, 1 + nq + nv + nu)))
            ctx.plant_step(st, tt, pt, rows, CTRL_DT, SIM_DT, 1, _lib.PLANT_CTRL, trace)
            assert torch.equal(got_tr[:, k], trace[:, 0]), (case, k)
        assert torch.equal(got_s, st) and torch.equal(got_t, tt), case
        assert torch.isfinite(got_s).all()
    finally:
        ctx.set_plant_disturbance(None)


def _gain_bias(nu, seed):
    rng = np.random.default_rng(seed)
    return rng.choice([0.5, 0.75, 1.25], (M, nu)), rng.integers(-16, 17, (M, nu)) / 8.0


@pytest.mark.parametrize("case", ["unitree_go2_trot", "unitree_h1_push_crate", "generic", "plugin"])
def test_actuator_error_in_ctrl_mode_is_the_row_disturbed_on_the_host(case):
    """DIAL_PLANT_CTRL: gains from {0.5, 0.75, 1.25}, biases on a 1/8 grid and torque rows k / 8, |k| <= 160: gain row + bias is
    exact in fp32 (checked against fp64).  The disturbed run on `rows` equals the unbound run on gain rows + bias bit for bit --
    states, clocks and the trace, whose ctrl columns are the disturbed values."""
    import torch
    from dial_mpc_amd import _lib
    env, ctx = _make(case)
    s0 = _start_states(ctx, env, seed=8)
    rows = _rows(ctx, env, False, seed=9)
    gain, bias = _gain_bias(ctx.nu, seed=10)
    exact = gain[:, None, :] * rows.astype(np.float64) + bias[:, None, :]
    rows2 = exact.astype(np.float32)
    assert np.array_equal(rows2.astype(np.float64), exact) and not np.array_equal(rows2, rows)
    t, plan_time = _clocks()
    try:
        _bind(ctx, gain, bias, [[] for _ in range(M)])
        a = _run(ctx, s0, t, plan_time, _dev(rows), _lib.PLANT_CTRL)
        ctx.set_plant_disturbance(None)
        b = _run(ctx, s0, t, plan_time, _dev(rows2), _lib.PLANT_CTRL)
        for what, x, y in zip(("states", "clocks", "trace"), a, b):
            assert torch.equal(x, y), (case, what)
        assert torch.isfinite(a[0]).all()
    finally:
        ctx.set_plant_disturbance(None)


def _round_f32(x: Fraction) -> np.float32:
    """The float32 nearest to the rational x, ties to even."""
    c = np.float32(float(x))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))


def _fma_f32(g, c, b) -> np.float32:
    """fma(g, c, b) with ONE rounding to float32: math.fma where Python has it and its fp64 result is exact (the rounding to
    float32 is then the only one), else exact rational arithmetic."""
    exact = Fraction(float(g)) * Fraction(float(c)) + Fraction(float(b))
    if hasattr(math, "fma"):
        r = math.fma(float(g), float(c), float(b))
        if Fraction(r) == exact:
            return np.float32(r)
    return _round_f32(exact)


@pytest.mark.parametrize("case,mode", [("unitree_go2_trot", "PD"), ("unitree_h1_loco", "PD"), ("generic", "PD"), ("plugin", "PD"),
                                       ("plugin-law", "LAW")])
def test_actuator_error_in_pd_and_law_mode_is_one_fma_of_the_undisturbed_ctrl(case, mode):
    """Step 0 starts from identical states, so the mode's own ctrl c (the PD torque after its clip, the law's value) is the unbound
    run's trace ctrl; the disturbed trace's ctrl columns are fma(gain, c, bias) rounded once.  The state columns of both rows are the
    same, and the disturbed plant then moves differently."""
    import torch
    from dial_mpc_amd import _lib
    env, ctx = _make(case)
    nq, nv, nu = ctx.nq, ctx.nv, ctx.nu
    flags = dict(PD=_lib.PLANT_PD, LAW=_lib.PLANT_LAW)[mode]
    s0 = _start_states(ctx, env, seed=11)
    rows = _dev(_mode_rows(case, ctx, env, mode, seed=12))
    gain, bias = _gain_bias(nu, seed=13)
    t, plan_time = _clocks()
    try:
        ctx.set_plant_disturbance(None)
        plain_s, _, plain_tr = _run(ctx, s0, t, plan_time, rows, flags, k=1)
        _bind(ctx, gain, bias, [[] for _ in range(M)])
        got_s, _, got_tr = _run(ctx, s0, t, plan_time, rows, flags, k=1)
    finally:
        ctx.set_plant_disturbance(None)
    p, g = plain_tr[:, 0].cpu().numpy(), got_tr[:, 0].cpu().numpy()
    assert np.array_equal(p[:, :1 + nq + nv], g[:, :1 + nq + nv])
    c = p[:, -nu:]
    assert np.isfinite(c).all() and len(np.unique(c)) > M and np.abs(c).max() > 0.5   # real torques, not a degenerate case
    want = np.array([[_fma_f32(np.float32(gain[m, a]), c[m, a], np.float32(bias[m, a])) for a in range(nu)] for m in range(M)], np.float32)
    assert np.array_equal(g[:, -nu:], want), (case, np.argwhere(g[:, -nu:] != want)[:4].tolist())
    assert torch.isfinite(got_s).all() and not torch.equal(got_s, plain_s)


@pytest.mark.parametrize("case", ["unitree_go2_trot", "generic", "plugin"])
def test_plants_of_one_launch_are_independent(case):
    """M plants with different gains, biases and events in one launch = each plant alone with its own row bound (M = 1)."""
    import torch
    from dial_mpc_amd import _lib
    env, ctx = _make(case)
    s0 = _start_states(ctx, env, seed=14)
    rows = _dev(_rows(ctx, env, False, seed=15))
    gain, bias = _gain_bias(ctx.nu, seed=16)
    t, plan_time = _clocks()
    clocks = _step_clocks(t)
    rng = np.random.default_rng(17)
    events = [[(*_window(clocks[m, (m + j) % K]), rng.integers(-8, 9, ctx.nv) / 64.0) for j in range(1 + m % 3)] for m in range(M)]
    packed, E = pack(ctx.nu, ctx.nv, gain, bias, events)
    assert E == 3
    try:
        dist = ctx.set_plant_disturbance(_dev(packed), E)
        a = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)
        for m in range(M):
            ctx.set_plant_disturbance(dist[m:m + 1].contiguous(), E)
            b = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL, sel=slice(m, m + 1))
            for what, x, y in zip(("states", "clocks", "trace"), a, b):
                assert torch.equal(x[m:m + 1], y), (case, m, what)
    finally:
        ctx.set_plant_disturbance(None)


def test_refusals_and_unbinding(tmp_path):
    import torch
    from dial_mpc_amd import _lib
    env, ctx = _make("unitree_go2_trot")
    nu, nv = ctx.nu, ctx.nv
    lib, h = ctx.lib, ctx.h
    s0 = _start_states(ctx, env, seed=18)
    rows = _dev(_rows(ctx, env, False, seed=19))
    t, plan_time = _clocks()
    buf = _dev(np.tile(np.r_[np.full(nu, 0.5), np.zeros(nu)], (M, 1)))

    def refused(rc, code):
        assert rc == code and lib.dial_last_error(h).decode().startswith("dial_set_plant_disturbance: "), (rc, lib.dial_last_error(h))
    refused(lib.dial_set_plant_disturbance(h, buf.data_ptr(), M, 17), ARG)
    refused(lib.dial_set_plant_disturbance(h, buf.data_ptr(), M, -1), ARG)
    refused(lib.dial_set_plant_disturbance(h, buf.data_ptr(), 0, 0), ARG)
    refused(lib.dial_set_plant_disturbance(h, buf.data_ptr(), _abi.MACROS["DIAL_MAX_PLANTS"] + 1, 0), ARG)
    refused(lib.dial_set_plant_disturbance(h, None, M, 0), ARG)
    refused(lib.dial_set_plant_disturbance(h, None, 0, 1), ARG)
    with pytest.raises(_lib.DialHipError, match="n_events = 17") as e:
        ctx.set_plant_disturbance(_dev(np.zeros((M, _lib.plant_dist_row(nu, nv, 17)))), 17)
    assert f"({ARG})" in str(e.value)
    with pytest.raises(ValueError, match="rows of"):
        ctx.set_plant_disturbance(_dev(np.zeros((M, 2 * nu + 1))), 0)
    plain = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)   # none of the refused calls bound anything
    try:
        ctx.set_plant_disturbance(buf, 0)
        assert ctx._plant_dist is buf   # (the wrapper keeps the tensor alive)
        halved = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)
        assert not torch.equal(halved[0], plain[0])
        with pytest.raises(_lib.DialHipError, match="bound plant disturbance has 8 rows") as e:   # M mismatch at step time
            _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL, sel=slice(0, 4))
        assert f"({ARG})" in str(e.value) and "dial_plant_step: " in str(e.value)
        ctx.set_plant_disturbance(None)   # unbinding restores the old path, for any M
        again = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)
        for x, y in zip(plain, again):
            assert torch.equal(x, y)
        four = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL, sel=slice(0, 4))
        assert torch.equal(four[0], plain[0][:4])
    finally:
        ctx.set_plant_disturbance(None)
    # a plugin built with plant=True only has no disturbed kernel: binding is refused, its plant still steps
    penv, pctx = _make("plugin-plant-only")
    with pytest.raises(_lib.DialHipError, match="dial_plugin_plant_dist_v1") as e:
        pctx.set_plant_disturbance(buf, 0)
    assert f"({UNSUP})" in str(e.value)
    ps0 = _start_states(pctx, penv, seed=18)
    assert torch.isfinite(_run(pctx, ps0, t, plan_time, rows, _lib.PLANT_CTRL)[0]).all()
    # the IEEE measurement build has no plant, and a library without libdialplantdist.so next to it cannot bind
    ictx = _lib.Context(ctx.model, ctx.task, None, device=0, lib_path=_lib.IEEE_LIB_PATH)
    with pytest.raises(_lib.DialHipError, match="IEEE measurement build") as e:
        ictx.set_plant_disturbance(buf, 0)
    assert f"({UNSUP})" in str(e.value)
    lone = tmp_path / "libdialhip.so"
    shutil.copy(_lib.LIB_PATH, lone)
    shutil.copy(_lib.PLANT_LIB_PATH, tmp_path / "libdialplant.so")
    lctx = _lib.Context(ctx.model, ctx.task, None, device=0, lib_path=str(lone))
    with pytest.raises(_lib.DialHipError, match="libdialplantdist.so") as e:
        lctx.set_plant_disturbance(buf, 0)
    assert f"({UNSUP})" in str(e.value)
    ls0 = _start_states(lctx, env, seed=18)
    for x, y in zip(plain, _run(lctx, ls0, t, plan_time, rows, _lib.PLANT_CTRL)):   # ... while its undisturbed plant is what it was
        assert torch.equal(x, y)
