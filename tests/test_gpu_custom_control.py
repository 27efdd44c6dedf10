"""User control laws on the GPU: the probe law of tests/control_probe.hip (a mode per check, chosen by a task parameter) next to the
probe reward of tests/plugin_probe.hip, on the Go2, the Go2 with four physics sub-steps per control step and the H1 push-crate scene
(tests/plugin_cases.py).  The law's inputs, its value against an fp64 evaluation, the physics against the fp32 oracle's built-in law,
rollouts, launch paths, per-plan parameter rows, a Go2 with permuted actuators, dial_user_control and the env surface, the example."""
import numpy as np
import pytest

from conftest import LS_SWAP, TOL, _within, perturbed_state, seeded_inputs, with_solver
from control_cases import (CF, CPROBE_BAD, PERM, build_control_plugins, host_act2joint, host_pd, load_position_case, params,
                           permuted_go2_env, task_consts)
from dial_mpc_amd import _abi
from plugin_cases import F, build_matrix, load_case
from test_gpu_custom_env import _physics_gate

pytestmark = pytest.mark.gpu

H = 12
M_ = _abi.MACROS
IU, IUN, IREW, ISTEP, ILAST = M_["DIAL_INFO_USER"], M_["DIAL_INFO_USER_N"], M_["DIAL_INFO_REWARD"], M_["DIAL_INFO_STEP"], M_["DIAL_INFO_LAST_CTRL"]


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


@pytest.fixture(scope="module")
def plugins():
    p = build_control_plugins()
    p["go2_nf4"] = p["go2"]
    return p


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = load_position_case(N=16, H=H) if name == "go2_pos" else load_case(name, N=16, H=H)
    return _cases[name]


def _ctx(c, path, p, cfg=True, **opts):
    from dial_mpc_amd import _lib
    return _lib.Context(c["model"], c["ptask"], c["cfg"] if cfg else None, plugin=path, user_params=list(p), options=opts)


def _adr(c):
    m = c["model"]
    return (np.asarray(_abi.as_numpy(m, "act_qposadr")).ravel()[:m.nu].astype(int),
            np.asarray(_abi.as_numpy(m, "act_dofadr")).ravel()[:m.nu].astype(int))


def _start(c, ctx, seed=None):
    q, qd = (c["env"]._init_q, np.zeros(c["model"].nv)) if seed is None else perturbed_state(c["env"], seed)
    return ctx.env_reset(_dev(q), _dev(qd))[0]


@pytest.mark.parametrize("name", ["go2", "h1_push_crate"])
def test_law_inputs_through_env_step(plugins, name):
    """1. Mode 4: every element of every input of the law, one env_step_batch from a perturbed state with one row of per-plan
    parameters per (field, index).  Every lane returns the selected element, so ctrl_out[row] is that element nu times (field `lane`:
    the actuator index).  qpos / qvel are the state the step STARTS from; a second step from the returned states shows the step counter
    advancing and the law reading the slots the reward wrote on the step before."""
    c = _case(name)
    m = c["model"]
    nq, nv, nu = m.nq, m.nv, m.nu
    info = nq + 2 * nv
    k = task_consts(c["ptask"], nu)
    qadr, dadr = _adr(c)
    ctx = _ctx(c, plugins[name], params(4), cfg=False)
    s0 = _start(c, ctx, seed=2).cpu().numpy()
    s0[info + ISTEP] = 5.0
    slots = np.float32([F["ctrl"], 2, 3.0, 7.5, -2.25, 9.0])   # slots 0, 1: the reward probe's own selector (ctrl[2]); 2: its counter
    s0[info + IU:info + IU + IUN] = slots
    act = np.random.default_rng(21).uniform(-0.8, 0.8, nu).astype(np.float32)
    want = dict(qpos=s0[:nq], qvel=s0[nq:nq + nv], act=act, act_qposadr=qadr, act_dofadr=dadr, kp=k["kp"], kd=k["kd"],
                joint_range=k["joint_range"].ravel(), phys_range=k["phys_range"].ravel(), tau_range=k["tau_range"].ravel(),
                joint_offset=k["joint_offset"], info_user=slots)
    scalars = dict(step=5.0, dt=np.float32(c["ptask"].dt), nq=nq, nv=nv, nu=nu, action_scale=k["action_scale"])
    rows = [(f, i) for f, v in want.items() for i in range(len(v) + 1)] + [(f, 0) for f in scalars] + [("lane", 0), ("qpos", -1)]
    R = len(rows)
    assert R <= M_["DIAL_MAX_PLANS"]
    ctx.set_plan_params(np.float32([params(4, 0, 0, CF[f], i) for f, i in rows]))
    S = np.repeat(s0[None], R, 0)
    A = np.repeat(act[None], R, 0)
    out, _, _, ctrl = [t.cpu().numpy() for t in ctx.env_step_batch(_dev(S), _dev(A))]
    for r, (f, i) in enumerate(rows):
        if f == "lane":
            exp = np.arange(nu, dtype=np.float32)
        elif f in scalars:
            exp = np.full(nu, np.float32(scalars[f]))
        else:
            exp = np.full(nu, np.float32(want[f][i]) if 0 <= i < len(want[f]) else np.float32(CPROBE_BAD))
        assert np.array_equal(ctrl[r], exp), (f, i, ctrl[r].tolist(), exp.tolist())
    # what the law returned is what the reward saw as ctrl, what the step left in the info, and the step advanced
    assert np.array_equal(out[:, info + IREW], ctrl[:, 2]) and np.array_equal(out[:, info + ILAST:info + ILAST + nu], ctrl)
    assert np.all(out[:, info + ISTEP] == 6.0) and np.all(out[:, info + IU + 2] == 4.0)
    # second step: the counter, and the slots as the reward left them (slot 2: its step count; slot 3: the value it returned)
    _, _, _, ctrl2 = [t.cpu().numpy() for t in ctx.env_step_batch(_dev(out), _dev(A))]
    at = {fi: r for r, fi in enumerate(rows)}
    assert np.all(ctrl2[at[("step", 0)]] == 6.0) and np.all(ctrl2[at[("info_user", 2)]] == 4.0)
    r3 = at[("info_user", 3)]
    assert np.all(ctrl[r3] == 7.5) and np.all(ctrl2[r3] == out[r3, info + IREW]) and out[r3, info + IREW] == 7.5
    r0 = at[("qpos", 0)]
    assert np.all(ctrl2[r0] == out[r0, 0])   # the second step's law read the first step's result


def _step(ctx, p, s, a):
    import torch
    ctx.set_user_params(p)
    st, _, _, ctrl = ctx.env_step(s, _dev(a))
    torch.cuda.synchronize()
    return st.cpu().numpy(), ctrl.cpu().numpy()


def test_same_plugin_bit_for_bit(plugins):
    """2. One plugin, one state: the own-joint PD law (mode 3) gives ctrl c; the pass-through law (mode 2) fed c as the action gives
    the same ctrl and a bit-identical next state -- the physics behind the law is one binary.  Mode 0 (7 + a / 6 + a indexing) equals
    mode 3 on the Go2, whose actuators follow that convention."""
    c = _case("go2")
    ctx = _ctx(c, plugins["go2"], params(3), cfg=False)
    s0 = _start(c, ctx, seed=1)
    act = np.random.default_rng(22).uniform(-0.8, 0.8, c["model"].nu).astype(np.float32)
    st3, c3 = _step(ctx, params(3), s0, act)
    st2, c2 = _step(ctx, params(2), s0, c3)
    assert np.any(c3 != 0.0) and np.array_equal(c2, c3) and np.array_equal(st2, st3)
    st0, c0 = _step(ctx, params(0), s0, act)
    assert np.array_equal(c0, c3) and np.array_equal(st0, st3)


def _law_values(c, ctx, mode, seeds=(0, 1, 2, 3)):
    """ctrl_out of env.step in `mode` from perturbed states, with the host's fp64 value and bound -> worst error / bound."""
    m = c["model"]
    nq, nv, nu = m.nq, m.nv, m.nu
    k = task_consts(c["ptask"], nu)
    qadr, dadr = (7 + np.arange(nu), 6 + np.arange(nu)) if mode == 0 else _adr(c)
    rng = np.random.default_rng(23)
    worst, firsts = 0.0, []
    for seed in seeds:
        s0 = _start(c, ctx, seed=seed)
        act = rng.uniform(-0.9, 0.9, nu).astype(np.float32)
        _, ctrl = _step(ctx, params(mode), s0, act)
        s = s0.cpu().numpy()
        want, bound = host_pd(k, s[:nq], s[nq:nq + nv], act, qadr, dadr)
        err = np.abs(ctrl.astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (mode, seed, int(np.argmax(err / bound)), float(err.max()))
        firsts.append((s, act, ctrl, want, bound))
    return worst, firsts


@pytest.mark.parametrize("name", ["go2", "h1_push_crate"])
def test_value_of_the_law(plugins, name):
    """3. Modes 0 and 3 against the formula in fp64 from the kernel's own fp32 inputs, after the tau_range clip, within
    16 * 2^-24 * (kp (|lo| + |hi| + |q|) + kd |qd|) per actuator (control_cases.host_pd)."""
    c = _case(name)
    ctx = _ctx(c, plugins[name], params(0), cfg=False)
    for mode in (0, 3):
        worst, firsts = _law_values(c, ctx, mode)
        clipped = sum(int(np.sum((f[3] == task_consts(c["ptask"], c["model"].nu)["tau_range"][:, 0]) |
                                 (f[3] == task_consts(c["ptask"], c["model"].nu)["tau_range"][:, 1]))) for f in firsts)
        print(f"{name} mode {mode}: worst |ctrl - fp64| / bound = {worst:.3g} ({clipped} clipped values)")


def _oracle(c):
    import oracle as O
    return O.Oracle(c["model"], c["otask"], c["cfg"], np.float32)


@pytest.mark.parametrize("name,mode", [("go2", 0), ("go2_pos", 1), ("go2_nf4", 0)])
def test_physics_matches_the_oracles_built_in_law(plugins, name, mode):
    """4. The restated built-in law (mode 0 torque, mode 1 position) against the fp32 oracle running ITS built-in law: the inputs of
    test_gpu_custom_env.test_plugin_physics_matches_oracle (seed 4, uniform +-0.8, DIAL_LS_SWAP), its gate, conftest.TOL, at most 1
    diverged rollout of 16.  go2_nf4 (4 physics sub-steps per control step): the law runs once per control step -- the first step's
    ctrl equals the host's value from the START state, and the rollout passes the same gate (a law evaluated per sub-step would not).
    First-step bound: test 3's for the torque law; for the position law 16 * 2^-24 * (|lo| + |hi|) of the sampling range -- act2joint is
    6 fp32 roundings, each relative to a partial result no larger than that sum."""
    c = _case(name)
    m, cfg = c["model"], c["cfg"]
    T = cfg.Hsample + 1
    assert c["ptask"].n_frames == (4 if name == "go2_nf4" else 1) and c["ptask"].position_control == (1 if name == "go2_pos" else 0)
    ctx = _ctx(c, plugins["go2"], params(mode, F["ctrl"], 0))
    o32 = _oracle(c)
    s0, _, _ = o32.env_reset(c["env"]._init_q, np.zeros(m.nv))
    us = np.random.default_rng(4).uniform(-0.8, 0.8, (16, T, m.nu)).astype(np.float32)
    got = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
    ref = o32.rollout(s0, us)
    k = task_consts(c["ptask"], m.nu)
    for b in range(16):   # the first step's ctrl[0] (the probe reward), from the start state
        if mode == 1:
            want, bound = host_act2joint(k, us[b, 0])[0], 16.0 * 2.0 ** -24 * float(np.abs(k["joint_range"][0]).sum())
        else:
            w, bd = host_pd(k, s0[:m.nq], s0[m.nq:m.nq + m.nv], us[b, 0], 7 + np.arange(m.nu), 6 + np.arange(m.nu))
            want, bound = w[0], bd[0]
        assert abs(float(got[0][b, 0]) - want) <= bound, (b, float(got[0][b, 0]), want)
    bad = _physics_gate(got[1:], ref[1:], 16, T, max_diverged=1)
    print(f"{name} mode {mode}: {bad} of 16 rollouts outside the gate")


def test_rollouts_see_the_law(plugins):
    """5. H1 push crate (nu = 19, the generic set, a dry-friction row), mode 3, the probe reward returning ctrl[i]: rewss[b, t] is the
    law's value for actuator i at step t, i.e. the host evaluation from the rollout's OWN q / qd of step t - 1 (the start state for
    t = 0) and the step's action, within test 3's bound.  Actuators 0, 7 and 18."""
    c = _case("h1_push_crate")
    m, cfg = c["model"], c["cfg"]
    nq, nv, nu, T = m.nq, m.nv, m.nu, cfg.Hsample + 1
    k = task_consts(c["ptask"], nu)
    qadr, dadr = _adr(c)
    ctx = _ctx(c, plugins["h1_push_crate"], params(3))
    s0 = _start(c, ctx, seed=5)
    s0n = s0.cpu().numpy()
    us = np.random.default_rng(9).uniform(-0.8, 0.8, (16, T, nu)).astype(np.float32)
    worst = 0.0
    for i in (0, 7, 18):
        ctx.set_user_params(params(3, F["ctrl"], i))
        rewss, qss, qdss, _ = [t.cpu().numpy() for t in ctx.rollout(s0, _dev(us))]
        for b in range(16):
            for t in range(T):
                q, qd = (s0n[:nq], s0n[nq:nq + nv]) if t == 0 else (qss[b, t - 1], qdss[b, t - 1])
                want, bound = host_pd(k, q, qd, us[b, t], qadr, dadr)
                e = abs(float(rewss[b, t]) - want[i])
                worst = max(worst, e / bound[i])
                assert e <= bound[i], (i, b, t, float(rewss[b, t]), want[i])
    print(f"h1_push_crate: worst |rollout ctrl - fp64| / bound = {worst:.3g}")


def test_launch_paths_queue_and_trace(plugins):
    """6. One Go2 batch through the rollout queue and through the state-trace launch equals the plain launch bit for bit (mode 3, the
    probe reward returning ctrl[1]); the paths are forced as test_gpu_plugin_matrix.test_launch_paths_queue_and_trace forces them."""
    from dial_mpc_amd import _lib
    from test_gpu_plugin_matrix import _plan, _same
    c0 = load_case("go2", N=64, H=H)
    probe = _lib.Context(c0["model"], c0["ptask"], c0["cfg"], plugin=plugins["go2"])
    slots = probe.lib.dial_debug_resident_rollouts(probe.h, 10 ** 6)
    del probe
    N = slots + slots // 2
    c = load_case("go2", N=N, H=H)
    ins = seeded_inputs(c["dc"], c["model"].nu, seed=6, Ybar_scale=0.2)
    p = params(3, F["ctrl"], 1)
    ctx = _ctx(c, plugins["go2"], p)
    assert 0 < ctx.lib.dial_debug_resident_rollouts(ctx.h, N + 1) < N + 1
    q = _plan(ctx, _start(c, ctx), ins)
    assert ctx.debug_last_launch()["queue"] == 1
    ctx1 = _ctx(c, plugins["go2"], p, no_queue=1)
    assert ctx1.lib.dial_debug_resident_rollouts(ctx1.h, N + 1) == 0
    plain = _plan(ctx1, _start(c, ctx1), ins)
    assert ctx1.debug_last_launch()["queue"] == 0 and np.all(np.isfinite(plain[0]["rews"])) and plain[0]["rewss"].std() > 0
    _same(q, plain, "queue")
    ctx.set_state_trace(N + 1)
    qt = _plan(ctx, _start(c, ctx), ins)
    assert ctx.debug_last_launch()["trace"] == 1
    _same(qt, plain, "trace")


def test_per_plan_rows(plugins):
    """7. Per-plan parameter rows reach the law: M = 3 grouped plans that share state, noise and mean, with the law's scale
    (params[5]) 0, 0.5 and 1 and the probe reward returning ctrl[1] -- plan g's first-step rewards are (1 + scale_g) x plan 0's (one
    fp32 product).  env_step_batch and dial_user_control with the same rows bound: row g's scaling for state g; more states than
    rows are refused."""
    import torch
    from dial_mpc_amd._lib import DialHipError
    from test_gpu_plugin_matrix import _scratch_rows
    N, M = 16, 3
    c = _case("go2")
    nu = c["model"].nu
    scales = np.float32([0.0, 0.5, 1.0])
    rows = np.float32([params(3, F["ctrl"], 1, scale=s) for s in scales])
    ctx = _ctx(c, plugins["go2"], params(3, F["ctrl"], 1), plan_cap=M)
    s0 = _start(c, ctx, seed=3)
    eps, sigma, Ybar = seeded_inputs(c["dc"], nu, seed=2, Ybar_scale=0.2)
    ctx.set_plan_params(rows)
    ctx.reverse_once_batch(torch.stack([s0] * M).contiguous(), _dev(np.stack([Ybar] * M)), _dev(np.stack([sigma] * M)), _dev(np.stack([eps] * M)))
    torch.cuda.synchronize()
    ctx.status()
    first = _scratch_rows(ctx, M * (N + 1))["rewss"].reshape(M, N + 1, -1)[:, :, 0]
    assert np.all(first[0] != 0.0) and np.all(np.isfinite(first))
    for g in range(M):
        assert np.array_equal(first[g], first[0] * (np.float32(1.0) + scales[g])), g
    act = np.random.default_rng(25).uniform(-0.8, 0.8, nu).astype(np.float32)
    S, A = torch.stack([s0] * M).contiguous(), _dev(np.repeat(act[None], M, 0))
    _, _, _, cs = ctx.env_step_batch(S, A)
    cu = ctx.user_control(S, A)
    cs, cu = cs.cpu().numpy(), cu.cpu().numpy()
    for g in range(M):
        assert np.array_equal(cs[g], cs[0] * (np.float32(1.0) + scales[g])) and np.array_equal(cu[g], cs[g]), g
    with pytest.raises(DialHipError, match=r"dial_user_control: n = 4 exceeds the 3 rows"):
        ctx.user_control(torch.stack([s0] * 4).contiguous(), _dev(np.repeat(act[None], 4, 0)))
    ctx.set_plan_params(None)
    assert np.array_equal(ctx.user_control(S, A).cpu().numpy(), np.repeat(cs[:1], M, 0))   # the shared parameters again


def test_permuted_go2_under_the_law(plugins):
    """8. The Go2 with permuted actuators (refused under torque control without a law) with the own-joint law and permuted actions
    reproduces the unpermuted Go2's step: ctrl equal after un-permuting, the next state within conftest.TOL (the two runs sum the
    actuator forces in a different order)."""
    from dial_mpc_amd import _lib
    c = _case("go2")
    m = c["model"]
    nq, nv, nu = m.nq, m.nv, m.nu
    envp = permuted_go2_env("torque", base=c["env"])
    assert envp.plugin_path() == plugins["go2"]           # same dimensions, same two sources: the same plugin
    mp = with_solver(envp.make_model(), ls_rule=LS_SWAP)
    assert list(np.asarray(_abi.as_numpy(mp, "act_dofadr")).ravel()[:3]) == [9, 10, 11]
    ctx = _ctx(c, plugins["go2"], params(3), cfg=False)
    ctxp = _lib.Context(mp, envp.make_task(), None, plugin=plugins["go2"], user_params=params(3))
    rng = np.random.default_rng(26)
    for seed in (0, 4):
        q, qd = perturbed_state(c["env"], seed)
        s0 = ctx.env_reset(_dev(q), _dev(qd))[0]
        sp = s0.clone()                                   # one start state for both runs (warm start included)
        act = rng.uniform(-0.8, 0.8, nu).astype(np.float32)
        st, ctrl = _step(ctx, params(3), s0, act)
        stp, ctrlp = _step(ctxp, params(3), sp, act[PERM])
        assert np.any(ctrl != 0.0) and np.array_equal(ctrlp, ctrl[PERM])
        assert _within(stp[:nq], st[:nq], TOL["q"]).all() and _within(stp[nq:nq + nv], st[nq:nq + nv], TOL["qd"]).all()


def test_user_control_entry_and_env_surface(plugins):
    """9. dial_user_control: 13 rows of one state equal the ctrl_out of 13 env.steps from that state, bit for bit; CustomEnv.control
    and act2tau agree with env.step on an env with a law; contexts without a law are refused with DIAL_ERR_ARG and the reason."""
    import torch
    from dial_mpc_amd import _lib
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.envs.state import State
    c = _case("go2")
    nu = c["model"].nu
    ctx = _ctx(c, plugins["go2"], params(3), cfg=False)
    s0 = _start(c, ctx, seed=6)
    s0[c["model"].nq + 2 * c["model"].nv + ISTEP] = 4.0
    us = np.random.default_rng(27).uniform(-0.9, 0.9, (13, nu)).astype(np.float32)
    steps = np.stack([_step(ctx, params(3), s0, u)[1] for u in us])
    got = ctx.user_control(torch.stack([s0] * 13).contiguous(), _dev(us)).cpu().numpy()
    assert np.any(steps != 0.0) and np.array_equal(got, steps)
    # the env surface, on the permuted Go2 (its parameters are all zero: mode 0 of the probe)
    envp = permuted_go2_env("torque", base=c["env"])
    q, qd = perturbed_state(c["env"], 6)
    st = State.from_reset(envp, envp._context(), q, qd)
    want = np.stack([envp.step(st, u).pipeline_state.ctrl.cpu().numpy() for u in us])
    ctl = envp.control(st, us)
    assert tuple(ctl.shape) == (13, nu) and np.any(want != 0.0) and np.array_equal(ctl.cpu().numpy(), want)
    assert np.array_equal(envp.control(st, us[3]).cpu().numpy(), want[3:4])
    tau = envp.act2tau(us[5], st.pipeline_state)
    assert tau.shape == (nu,) and np.array_equal(tau, want[5])
    err = M_["DIAL_ERR_ARG"]
    nolaw = _lib.Context(c["model"], c["ptask"], None, plugin=build_matrix(["go2"])["go2"])
    with pytest.raises(DialHipError, match=rf"dial_user_control failed \({err}\): .*built without a user control law"):
        nolaw.user_control(torch.stack([s0] * 2).contiguous(), _dev(us[:2]))
    builtin = _lib.Context(c["model"], c["otask"], None)
    with pytest.raises(DialHipError, match=rf"dial_user_control failed \({err}\): .*no task plugin"):
        builtin.user_control(torch.stack([s0] * 2).contiguous(), _dev(us[:2]))
    with pytest.raises(DialHipError, match=rf"dial_user_control failed \({err}\): .*n must be at least 1"):
        ctx._check(ctx.lib.dial_user_control(ctx.h, s0.data_ptr(), _dev(us).data_ptr(), 0, _dev(us).data_ptr(), None), "dial_user_control")


def test_example_env_plans(plugins):
    """10. The stance-residual example (go2_stance_residual.py) plans three ticks with MBDPI at N = 16: finite rewards, a clean
    status, and a zero action holds the stance pose's torque (the law's target is the home keyframe)."""
    import importlib
    import sys
    import torch
    import yaml
    import dial_mpc_amd.envs as dial_envs
    from dial_mpc_amd.core.dial_core import MBDPI, _generator, load_dial_and_env
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    try:
        name = "dial_mpc_amd.examples.custom_env.go2_stance_residual"
        mod = sys.modules.get(name)
        mod = importlib.reload(mod) if mod is not None else importlib.import_module(name)
        d = yaml.safe_load(open(mod.__file__[:-3] + ".yaml"))
        d.update(Nsample=16, Ndiffuse_init=2)
        dc, _, env = load_dial_and_env(d)
        mbdpi = MBDPI(dc, env)
        rng = _generator(dc.seed, mbdpi.device)
        state = env.reset(rng)
        hold = env.control(state, np.zeros(mbdpi.nu, np.float32)).cpu().numpy()
        assert np.all(np.abs(hold) < 1e-3), hold        # at the home keyframe with zero velocity a zero action asks for no torque
        Y0 = torch.zeros((dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=mbdpi.device)
        for t in range(3):
            state = env.step(state, Y0[0])
            Y0 = mbdpi.shift(Y0)
            for i in range(dc.Ndiffuse_init if t == 0 else dc.Ndiffuse):
                rng, Y0, info = mbdpi.reverse_once(state, rng, Y0, mbdpi.sigma_control * dc.traj_diffuse_factor ** i)
            torch.cuda.synchronize()
            mbdpi.ctx.status()
            assert np.isfinite(float(state.reward)) and torch.isfinite(info["rews"]).all() and torch.isfinite(Y0).all()
    finally:
        dial_envs._envs.clear()
        dial_envs._envs.update(saved[0])
        dial_envs._configs.clear()
        dial_envs._configs.update(saved[1])
