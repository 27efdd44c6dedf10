"""Reference tables of custom environments on the GPU: the probe reward of tests/table_probe.hip (one value of what the reward sees of
the table, chosen by a task parameter) on the Go2 and the Go2 crate scene (the capped workspace with its global overflow area), the
probe law of tests/table_law_probe.hip on the Go2, and the example go2_track_clip.  Rows against the host rule bit for bit, batched
env.step with per-state counters, the launch paths of a plugin context against the plain launch, the law's row through the physics
of the fp32 oracle, the example's reward against fp64, and the argument checks of dial_set_user_table."""
import sys

import numpy as np
import pytest
import yaml

from conftest import perturbed_state, seeded_inputs
from dial_mpc_amd import _abi
from plugin_cases import load_case
from table_cases import MODELS, TF, TPROBE_NONE, build_stale_plugins, build_table_plugins, dyadic_table
from test_gpu_custom_env import _physics_gate
from test_gpu_plugin_matrix import _scratch_rows

pytestmark = pytest.mark.gpu

H = 12
M_ = _abi.MACROS
IREW, ISTEP = M_["DIAL_INFO_REWARD"], M_["DIAL_INFO_STEP"]
ERR_ARG = M_["DIAL_ERR_ARG"]
MODES = ("clamp", "wrap")


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


@pytest.fixture(scope="module")
def plugins():
    return build_table_plugins()


_cases = {}


def _case(name, N=16):
    if (name, N) not in _cases:
        _cases[(name, N)] = load_case(name, N=N, H=H)
    return _cases[(name, N)]


def _ctx(c, path, params=(0, 0), cfg=True, **opts):
    from dial_mpc_amd import _lib
    return _lib.Context(c["model"], c["ptask"], c["cfg"] if cfg else None, plugin=path, user_params=list(params), options=opts)


def _info(c):
    return c["model"].nq + 2 * c["model"].nv


def _start(c, ctx, counter=0.0, seed=None):
    """The keyframe (or a perturbed state) after env.reset, with the step counter set -> host array."""
    q, qd = (c["env"]._init_q, np.zeros(c["model"].nv)) if seed is None else perturbed_state(c["env"], seed)
    s = ctx.env_reset(_dev(q), _dev(qd))[0].cpu().numpy()
    s[_info(c) + ISTEP] = counter
    return s


def _rows(table, s0, T, row0, mode):
    from dial_mpc_amd.envs.custom_env import table_row
    return np.array([table_row(s0 + t, row0, table.shape[0], mode) for t in range(T)])


@pytest.mark.parametrize("name", MODELS)
def test_rows_reach_the_reward(plugins, name):
    """1. A [9, 5] table of distinct dyadic values; 17 rollouts of 13 steps from states with counter 0, 5 and 7 (the window crosses the
    table's end), row0 0 and -3, both modes: rewss[b, t] is exactly the host rule's element for row[j] (every column), table[i] and
    row_index, and table_rows / table_cols are the bound sizes.  The physics (qss, qdss, xss) is bit-identical to the same context's
    before binding, and after set_user_table(None) the probe returns its sentinel.  go2_crate runs with con_cap = 1: every touching
    step of the capped workspace goes through the overflow area."""
    c = _case(name)
    m, T = c["model"], H + 1
    ctx = _ctx(c, plugins[name], params=(TF["row"], 0), **(dict(con_cap=1) if name == "go2_crate" else {}))
    table = dyadic_table(9, 5, seed=1)
    assert len(np.unique(table)) == table.size
    us = _dev(np.random.default_rng(3).uniform(-0.5, 0.5, (17, T, m.nu)))
    checked = 0
    for s0c in (0, 5, 7):
        s0 = _dev(_start(c, ctx, counter=s0c))
        ctx.set_user_table(None)
        base = [t.cpu().numpy() for t in ctx.rollout(s0, us)]
        assert np.all(base[0] == np.float32(TPROBE_NONE))
        assert np.all(np.isfinite(base[1]))
        for row0 in (0, -3):
            for mode in MODES:
                bound = ctx.set_user_table(table, row0=row0, mode=mode)
                assert tuple(bound.shape) == (9, 5) and bound.is_cuda
                idx = _rows(table, s0c, T, row0, mode)
                if mode == "wrap" or s0c == 7:
                    assert len(set(idx)) < T   # (the window really leaves the table: rows repeat)
                probes = [((TF["row"], j), table[idx, j]) for j in range(5)]
                probes += [((TF["table"], i), np.full(T, table.ravel()[i])) for i in (0, 17, 44)]
                probes += [((TF["row_index"], 0), idx.astype(np.float32)), ((TF["table_rows"], 0), np.full(T, 9.0)),
                           ((TF["table_cols"], 0), np.full(T, 5.0))]
                for p, want in probes:
                    ctx.set_user_params(p)
                    got = [t.cpu().numpy() for t in ctx.rollout(s0, us)]
                    assert np.array_equal(got[0], np.broadcast_to(np.float32(want), (17, T))), (s0c, row0, mode, p, got[0][0].tolist())
                    checked += 1
                for k in (1, 2, 3):
                    assert np.array_equal(got[k], base[k]), (s0c, row0, mode, ("qss", "qdss", "xss")[k - 1])
        ctx.set_user_table(None)
        ctx.set_user_params((TF["row"], 0))
        assert np.all(ctx.rollout(s0, us)[0].cpu().numpy() == np.float32(TPROBE_NONE))
    assert checked == 3 * 2 * 2 * 11


@pytest.mark.parametrize("name", MODELS)
def test_env_step_batch_reads_each_states_own_row(plugins, name):
    """2. env_step_batch of 8 states with 8 different counters: state g's reward is the element of ITS row.  Rebinding another table
    between two launches takes effect; rewriting the bound tensor in place, without a new call, takes effect on the next launch."""
    import torch
    c = _case(name)
    m = c["model"]
    ctx = _ctx(c, plugins[name], params=(TF["row"], 3), cfg=False)
    counters = [0, 1, 2, 5, 8, 9, 20, 3]
    S = np.stack([_start(c, ctx, counter=k, seed=g % 3) for g, k in enumerate(counters)])
    A = np.random.default_rng(5).uniform(-0.5, 0.5, (8, m.nu)).astype(np.float32)
    from dial_mpc_amd.envs.custom_env import table_row

    def rewards():
        out = ctx.env_step_batch(_dev(S), _dev(A))[0].cpu().numpy()
        assert np.array_equal(out[:, _info(c) + ISTEP], np.float32(counters) + 1)
        return out[:, _info(c) + IREW]

    t1, t2, t3 = dyadic_table(9, 5, seed=1), dyadic_table(7, 4, seed=2), dyadic_table(7, 4, seed=3)
    for mode in MODES:
        ctx.set_user_table(t1, row0=-1, mode=mode)
        assert np.array_equal(rewards(), np.float32([t1[table_row(k, -1, 9, mode), 3] for k in counters])), mode
        bound = ctx.set_user_table(t2, row0=2, mode=mode)      # rebinding
        want2 = np.float32([t2[table_row(k, 2, 7, mode), 3] for k in counters])
        assert np.array_equal(rewards(), want2), mode
        bound.copy_(torch.as_tensor(t3))                        # in place, no new call
        want3 = np.float32([t3[table_row(k, 2, 7, mode), 3] for k in counters])
        assert not np.array_equal(want2, want3) and np.array_equal(rewards(), want3), mode
    # a device tensor is bound as it is
    mine = _dev(t1)
    assert ctx.set_user_table(mine, mode="wrap").data_ptr() == mine.data_ptr()
    assert np.array_equal(rewards(), np.float32([t1[k % 9, 3] for k in counters]))


def _plan(ctx, s0, ins):
    """One reverse_once: the outputs and the scratch the launch paths are compared on."""
    import torch
    eps, sigma, Ybar = ins
    out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
    torch.cuda.synchronize()
    ctx.status()
    sc = ctx.debug_scratch()
    r = {k: out[k].cpu().numpy().copy() for k in ("Ybar", "rews", "qbar", "qdbar", "xbar")}
    r.update({k: np.array(sc[k]) for k in ("rewss", "qss", "qdss", "xss", "Y0s", "weights")})
    return r


def _same(a, b, what):
    for k in a:
        # (the probe gives every sample the same rewards: the softmax weights and Ybar are NaN on both sides)
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


TABLE, ROW0, S0C = dyadic_table(9, 5, seed=1), -3, 5


def _bind(ctx, mode="wrap"):
    ctx.set_user_table(TABLE, row0=ROW0, mode=mode)
    return ctx


def _expect(T, counter=S0C, mode="wrap", col=2):
    return np.float32(TABLE[_rows(TABLE, counter, T, ROW0, mode), col])


@pytest.mark.parametrize("name", MODELS)
def test_launch_paths_queue_and_trace(plugins, name):
    """3a. The rollout queue (N beyond the resident rollouts, forced as tests/test_gpu_plugin_matrix.py forces it) and the state-trace
    launch == the plain launch (no_queue=1), bit for bit, and every rollout of the queue -- first or later item of its wavefront --
    reads the rows of the host rule.  go2_crate runs with con_cap = 1: a queue wavefront reuses its overflow area across items.
    (The probe gives every sample the same rewards, so the softmax weights and Ybar are NaN on both sides: the comparison rests on
    rewss, qss, qdss, xss and Y0s.)"""
    from dial_mpc_amd import _lib
    opts = dict(con_cap=1) if name == "go2_crate" else {}
    c0 = _case(name, N=64)
    probe = _lib.Context(c0["model"], c0["ptask"], c0["cfg"], plugin=plugins[name], options=opts)
    slots = probe.lib.dial_debug_resident_rollouts(probe.h, 10 ** 6)
    del probe
    N = slots + slots // 2
    c = load_case(name, N=N, H=H)
    T = H + 1
    ins = seeded_inputs(c["dc"], c["model"].nu, seed=6, Ybar_scale=0.2)
    p = (TF["row"], 2)
    ctx = _bind(_ctx(c, plugins[name], params=p, **opts))
    assert 0 < ctx.lib.dial_debug_resident_rollouts(ctx.h, N + 1) < N + 1
    s0 = _dev(_start(c, ctx, counter=S0C))
    q = _plan(ctx, s0, ins)
    assert ctx.debug_last_launch()["queue"] == 1
    assert np.array_equal(q["rewss"], np.broadcast_to(_expect(T), (N + 1, T)))
    ctx1 = _bind(_ctx(c, plugins[name], params=p, no_queue=1, **opts))
    assert ctx1.lib.dial_debug_resident_rollouts(ctx1.h, N + 1) == 0
    _same(q, _plan(ctx1, s0, ins), "queue")
    ctx.set_state_trace(N + 1)   # (a traced launch takes neither the queue nor the spread grid)
    qt = _plan(ctx, s0, ins)
    assert ctx.debug_last_launch()["trace"] == 1
    _same(q, qt, "trace")


@pytest.mark.parametrize("name", MODELS)
def test_launch_paths_relay(plugins, name):
    """3b. The mean-trajectory relay (relay_always=1: the last rollout runs as pieces on different wavefronts, each of which loads
    its own first row from the state it is handed) == no_relay=1, bit for bit; the relayed rollout reads the host rule's rows.
    (Equal rewards in every sample: weights and Ybar are NaN on both sides, the comparison rests on rewss, qss, qdss, xss, Y0s.)"""
    c = _case(name, N=64)
    T = H + 1
    ins = seeded_inputs(c["dc"], c["model"].nu, seed=4, Ybar_scale=0.2)
    for mode in MODES:
        ref_ctx = _bind(_ctx(c, plugins[name], params=(TF["row"], 2), no_relay=1), mode)
        s0 = _dev(_start(c, ref_ctx, counter=S0C))
        ref = _plan(ref_ctx, s0, ins)
        assert ref_ctx.debug_last_launch()["relay"] == 0
        ctx = _bind(_ctx(c, plugins[name], params=(TF["row"], 2), relay_always=1), mode)
        got = _plan(ctx, s0, ins)
        assert ctx.debug_last_launch()["relay"] == 1
        _same(got, ref, ("relay", mode))
        assert np.array_equal(got["rewss"], np.broadcast_to(_expect(T, mode=mode), (65, T))), mode


@pytest.mark.parametrize("name", MODELS)
def test_launch_paths_grouped_plans(plugins, name):
    """3c. A grouped launch of M = 4 plans whose states carry the counters 0, 3, 6, 9: plan g == the single-plan launch from state g,
    bit for bit, and reads the rows of ITS counter (no per-plan offset: the state carries it).  (Equal rewards in every sample of a
    plan: weights and Ybar are NaN on both sides, the comparison rests on rewss, qss, qdss and xss.)"""
    import torch
    N, M = 16, 4
    c = _case(name)
    T, nu = H + 1, c["model"].nu
    outs = ("Ybar", "rews", "qbar", "qdbar", "xbar")
    ctx = _bind(_ctx(c, plugins[name], params=(TF["row"], 2), plan_cap=M))
    counters = (0, 3, 6, 9)
    S = [_dev(_start(c, ctx, counter=k, seed=g)) for g, k in enumerate(counters)]
    ins = [seeded_inputs(c["dc"], nu, seed=k, Ybar_scale=0.2) for k in range(M)]
    singles = []
    for s0, (eps, sigma, Ybar) in zip(S, ins):
        out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
        torch.cuda.synchronize()
        one = {k: out[k].cpu().numpy().copy() for k in outs}
        one.update(_scratch_rows(ctx, N + 1))
        singles.append(one)
    assert not np.array_equal(singles[0]["qss"], singles[1]["qss"]) and not np.array_equal(singles[0]["rewss"], singles[1]["rewss"])
    outb = ctx.reverse_once_batch(torch.stack(S).contiguous(), _dev(np.stack([i[2] for i in ins])),
                                  _dev(np.stack([i[1] for i in ins])), _dev(np.stack([i[0] for i in ins])))
    torch.cuda.synchronize()
    sc = _scratch_rows(ctx, M * (N + 1))
    for g in range(M):
        for k in outs:
            assert np.array_equal(outb[k][g].cpu().numpy(), singles[g][k], equal_nan=True), (g, k)
        for k, v in sc.items():
            assert np.array_equal(v[g * (N + 1):(g + 1) * (N + 1)], singles[g][k], equal_nan=True), (g, k)
        assert np.array_equal(singles[g]["rewss"], np.broadcast_to(_expect(T, counter=counters[g]), (N + 1, T))), g


def _grid(rng, shape):
    """Uniform on the grid k / 256 within +-0.4: sums of two such values are exact in fp32."""
    return (rng.integers(-102, 103, shape) / 256.0).astype(np.float32)


def test_the_law_reads_the_row(plugins):
    """4. The Go2 torque case of test_gpu_custom_control.test_physics_matches_the_oracles_built_in_law with the probe law of
    tests/table_law_probe.hip: the built-in torque law applied to act + row.  us and the table's 12 columns are uniform on the grid
    k / 256 within +-0.4, so act + row is exact and within +-0.8 (the range that test uses): the GPU rollouts under the table must pass
    that test's gate (_physics_gate, conftest.TOL, at most 1 diverged rollout of 16) against Oracle.rollout(s0, us + rows).  Then
    dial_user_control on the rollout's own states returns env.step's ctrl bit for bit, and the row matters to both."""
    import oracle as O
    c = _case("go2")
    m, cfg = c["model"], c["cfg"]
    nq, nv, nu, T = m.nq, m.nv, m.nu, cfg.Hsample + 1
    assert c["ptask"].n_frames == 1 and c["ptask"].position_control == 0
    ctx = _ctx(c, plugins["go2_law"], params=(TF["row_index"], 0))
    o32 = O.Oracle(c["model"], c["otask"], c["cfg"], np.float32)
    s0, _, _ = o32.env_reset(c["env"]._init_q, np.zeros(nv))
    rng = np.random.default_rng(4)
    us = _grid(rng, (16, T, nu))
    table = _grid(rng, (20, nu))
    ctx.set_user_table(table, row0=0, mode="clamp")       # counter 0: step t reads row t
    got = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
    assert np.array_equal(got[0], np.broadcast_to(np.arange(T, dtype=np.float32), (16, T)))   # the reward of the step sees the same row
    acts = us + table[None, :T, :]
    assert np.array_equal(acts.astype(np.float64), us.astype(np.float64) + table[None, :T, :].astype(np.float64))
    assert np.abs(acts).max() <= 0.8
    ref = o32.rollout(s0, acts)
    bad = _physics_gate(got[1:], ref[1:], 16, T, max_diverged=1)
    print(f"law reading the row: {bad} of 16 rollouts outside the gate")
    # dial_user_control == env.step's ctrl on the rollout's own states: state (b, t - 1) with counter t, action us[b, t]
    pick = [(b, t) for b in (0, 7, 15) for t in (1, 4, 12)]
    S = np.repeat(np.asarray(s0, np.float32)[None], len(pick), 0)
    for r, (b, t) in enumerate(pick):
        S[r, :nq], S[r, nq:nq + nv], S[r, _info(c) + ISTEP] = got[1][b, t - 1], got[2][b, t - 1], t
    A = np.stack([us[b, t] for b, t in pick])
    ctrl_step = ctx.env_step_batch(_dev(S), _dev(A))[3].cpu().numpy()
    ctrl_law = ctx.user_control(_dev(S), _dev(A)).cpu().numpy()
    assert np.array_equal(ctrl_step, ctrl_law)
    ctx.set_user_table(None)
    ctrl_none = ctx.user_control(_dev(S), _dev(A)).cpu().numpy()
    assert np.array_equal(ctrl_none, ctx.env_step_batch(_dev(S), _dev(A))[3].cpu().numpy())
    assert not np.array_equal(ctrl_none, ctrl_law)


# ---- 5. the example

EX_MOD = "dial_mpc_amd.examples.custom_env.go2_track_clip"


@pytest.fixture()
def example():
    """The example env at N = 16, H = 12; the env registry is left as it was found."""
    import importlib
    import os
    import dial_mpc_amd.envs as dial_envs
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    mod = sys.modules.get(EX_MOD)
    mod = importlib.import_module(EX_MOD) if mod is None else importlib.reload(mod)
    d = yaml.safe_load(open(os.path.join(os.path.dirname(mod.__file__), "go2_track_clip.yaml")))
    d["Nsample"], d["Hsample"] = 16, H
    dc, _, env = load_dial_and_env(d)
    yield dict(dc=dc, env=env, cfg=make_cfg(dc))
    dial_envs._envs.clear()
    dial_envs._envs.update(saved[0])
    dial_envs._configs.clear()
    dial_envs._configs.update(saved[1])


def _node2u(W, Y, fused):
    """The planner's controls u[b, t, a] = sum_k W[t, k] Y[b, k, a] as the rollout kernel accumulates them in fp32, k ascending
    from 0: fused multiply-adds (one rounding per node; the product of two fp32 values is exact in fp64) or separate multiplies and
    adds.  The caller checks the result against the device bit for bit."""
    acc = np.zeros((Y.shape[0], W.shape[0], Y.shape[2]), np.float32)
    for k in range(W.shape[1]):
        w, y = W[None, :, k, None], Y[:, None, k, :]
        if fused:
            acc = (w.astype(np.float64) * y.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = (acc + (w * y).astype(np.float32)).astype(np.float32)
    return acc


def test_example_reward_against_fp64(example):
    """5. go2_track_clip, N = 16, H = 12, one reverse_once with the state trace.  Every per-step reward of every rollout is recomputed
    in numpy fp64 from the traced states and the table, and must agree within (n + 4) * 2^-24 * sum |term| with n the reward's term
    count (each term one weighted square; the bound is computed from the terms themselves).  The reward has no divide, square root or
    transcendental, so the fast-math function flags play no part.

    What the reward read that the trace does not hold -- the trunk's pre-integration pose and the applied torques -- comes from
    replaying every traced step through env_step_batch (state before the step, the step's action): the replay must reproduce the traced
    state bit for bit, which makes its xpos / xquat / ctrl the values the rollout's reward saw.  The actions are the planner's
    W x nodes, accumulated as the kernel does (either contraction; the one that reproduces the trace is used)."""
    from dial_mpc_amd import _lib
    env, cfg, dc = example["env"], example["cfg"], example["dc"]
    ctx = _lib.Context(env.make_model(), env.make_task(), cfg, **env.context_kwargs())
    nq, nv, nu, N, T = ctx.nq, ctx.nv, ctx.nu, 16, H + 1
    table = env.make_table()
    p = np.float64(np.float32(env.user_param_vector()))
    counter = 93                                  # the 13-step window wraps round the 100-row clip
    s0 = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(nv)))[0].cpu().numpy()
    s0[nq + 2 * nv + ISTEP] = counter
    trace = ctx.set_state_trace(N + 1)
    out = _plan(ctx, _dev(s0), seeded_inputs(dc, nu, seed=8, Ybar_scale=0.2))
    assert np.all(np.isfinite(out["Ybar"])) and np.all(np.isfinite(out["rewss"]))
    tr = trace.cpu().numpy()
    before = np.concatenate([np.broadcast_to(s0, (N + 1, 1, s0.size)), tr[:, :-1]], axis=1).reshape(-1, s0.size)
    W = np.asarray(_abi.as_numpy(cfg, "W"), np.float32)[:T, :cfg.Hnode + 1]
    replay = None
    for fused in (True, False):
        acts = _node2u(W, out["Y0s"], fused).reshape(-1, nu)
        st, xpos, xquat, ctrl = [t.cpu().numpy() for t in ctx.env_step_batch(_dev(before), _dev(acts))]
        if np.array_equal(st, tr.reshape(-1, s0.size)):
            replay = (xpos[:, 0], xquat[:, 0], ctrl)
            break
    assert replay is not None, "the replay of the traced steps does not reproduce the trace"
    xpos1, xquat1, ctrl = [a.astype(np.float64) for a in replay]
    from dial_mpc_amd.envs.custom_env import table_row
    worst = 0.0
    rew = out["rewss"].astype(np.float64).ravel()
    qpos = tr.reshape(-1, s0.size)[:, :nq].astype(np.float64)
    for i in range((N + 1) * T):
        row = table[table_row(counter + i % T, 0, 100, "wrap")].astype(np.float64)
        w, x, y, z = xquat1[i]
        zx, zy, zz = 2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)
        terms = [p[0] * (qpos[i, 7 + a] - row[a]) ** 2 for a in range(12)]
        terms += [p[1] * (xpos1[i, 2] - row[12]) ** 2]
        terms += [p[2] * zx * zx, p[2] * zy * zy, p[2] * (zz - 1) ** 2]
        terms += [p[3] * ctrl[i, a] ** 2 for a in range(nu)]
        n = len(terms)
        bound = (n + 4) * 2.0 ** -24 * sum(abs(t) for t in terms)
        err = abs(rew[i] + sum(terms))
        worst = max(worst, err / bound)
        assert err <= bound, (i // T, i % T, rew[i], -sum(terms), err, bound)
    assert n == 28
    print(f"go2_track_clip: worst |device - fp64| / bound = {worst:.3g} over {(N + 1) * T} rewards")


def test_dial_set_user_table_validates_its_arguments(plugins):
    """6. Every refusal of dial_set_user_table: DIAL_ERR_ARG and a message that starts with its name; a refused call leaves the
    binding as it was.  A plugin without the table symbol gives a working context whose dial_set_user_table answers
    DIAL_ERR_UNSUPPORTED, and dial_create_plugin refuses a plugin whose table entry reports another version."""
    from dial_mpc_amd import _lib
    c = _case("go2")
    ctx = _ctx(c, plugins["go2"], params=(TF["row_index"], 0), cfg=False)
    lib = ctx.lib
    dev = _dev(dyadic_table(9, 5))
    ptr = dev.data_ptr()

    def refused(h, *args):
        rc = lib.dial_set_user_table(h, *args)
        msg = lib.dial_last_error(h).decode()
        assert rc == ERR_ARG and msg.startswith("dial_set_user_table: "), (args, rc, msg)
        return msg

    refused(None, ptr, 9, 5, 0, 0)                                    # null context
    for rows in (0, -1, (1 << 24) + 1):
        refused(ctx.h, ptr, rows, 5, 0, 0)                            # rows outside 1 .. 1 << 24 with a table
    for cols in (0, -2, M_["DIAL_USER_TABLE_COLS"] + 1):
        refused(ctx.h, ptr, 9, cols, 0, 0)                            # cols outside 1 .. DIAL_USER_TABLE_COLS
    for rows in (1, 9, -1):
        refused(ctx.h, None, rows, 5, 0, 0)                           # a null table with rows != 0
    for mode in (-1, 2, 7):
        refused(ctx.h, ptr, 9, 5, 0, mode)                            # an unknown mode
    # the limits themselves are accepted, and a refused call leaves the binding alone
    wide = _dev(np.zeros((2, M_["DIAL_USER_TABLE_COLS"])))
    assert lib.dial_set_user_table(ctx.h, wide.data_ptr(), 2, M_["DIAL_USER_TABLE_COLS"], 0, 1) == 0
    assert lib.dial_set_user_table(ctx.h, ptr, 9, 5, 2, 0) == 0
    refused(ctx.h, ptr, 9, 5, 0, 9)
    s = _start(c, ctx, counter=3)
    a = np.zeros((1, c["model"].nu), np.float32)
    assert ctx.env_step_batch(_dev(s[None]), _dev(a))[0].cpu().numpy()[0, _info(c) + IREW] == 5.0
    assert lib.dial_set_user_table(ctx.h, None, 0, 0, 0, 0) == 0      # unbind
    assert ctx.env_step_batch(_dev(s[None]), _dev(a))[0].cpu().numpy()[0, _info(c) + IREW] == np.float32(TPROBE_NONE)
    # stand-ins for plugins of older sources
    stale = build_stale_plugins()
    old = _ctx(c, stale["no_table"], params=(TF["row_index"], 0), cfg=False)
    rc = lib.dial_set_user_table(old.h, ptr, 9, 5, 0, 0)
    msg = lib.dial_last_error(old.h).decode()
    assert rc == M_["DIAL_ERR_UNSUPPORTED"] and msg.startswith("dial_set_user_table: ") and "dial_plugin_table_v1" in msg, (rc, msg)
    with pytest.raises(_lib.DialHipError, match="dial_set_user_table"):
        old.set_user_table(dyadic_table(9, 5))
    assert old.env_step_batch(_dev(s[None]), _dev(a))[0].cpu().numpy()[0, _info(c) + IREW] == np.float32(TPROBE_NONE)   # (it still steps)
    with pytest.raises(_lib.DialHipError, match="reference-table entry reports version 99"):
        _ctx(c, stale["version"], cfg=False)
    # a built-in (non-plugin) context
    built_in = _lib.Context(c["model"], c["otask"], None)
    msg = refused(built_in.h, ptr, 9, 5, 0, 0)
    assert "task plugin" in msg
    with pytest.raises(_lib.DialHipError, match="dial_set_user_table"):
        built_in.set_user_table(dyadic_table(9, 5))
    with pytest.raises(_lib.DialHipError):
        _lib.Context(c["model"], c["otask"], None, user_table=dyadic_table(9, 5))
