"""Per-plan task parameters of task-plugin contexts on the GPU (dial_set_plan_params): plan g of a grouped launch / state g of a batched
env.step reads row g of the bound parameters, single-plan launches row 0.  Held to bit identity with single-plan runs whose shared
parameters (dial_set_user_params) are that row, on every launch path a plugin context takes; the example reward's values against its
numpy mirror; the closed-loop driver's --env-param against single closed loops."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import perturbed_state, seeded_inputs
from test_gpu_custom_env import EX_MOD, EX_YAML, ROOT, _mirror_reward, _registry  # noqa: F401  (the registry fixture)

pytestmark = pytest.mark.gpu

BARS = ("Ybar", "rews", "qbar", "qdbar", "xbar")
VX = (0.2, 0.5, 0.8, 1.1)
HEIGHT = (0.25, 0.3, 0.35, 0.28)


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _example(N=64, H=16, **over):
    import importlib
    importlib.import_module(EX_MOD)
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    d = yaml.safe_load(open(EX_YAML))
    d.update(over, Nsample=N, Hsample=H)
    dc, _, env = load_dial_and_env(d)
    return dc, env, make_cfg(dc)


@pytest.fixture(scope="module")
def ex():
    dc, env, cfg = _example()
    return dict(dc=dc, env=env, cfg=cfg, plugin=env.plugin_path(), params=env.user_param_vector())


def _ctx(ex, M=1, with_cfg=True, **opts):
    from dial_mpc_amd import _lib
    env = ex["env"]
    return _lib.Context(env.make_model(), env.make_task(), ex["cfg"] if with_cfg else None, plugin=ex["plugin"], user_params=ex["params"],
                        options=dict(opts, plan_cap=M))


def _rows(ex, M):
    """M distinct parameter rows of the example: vx and height per plan, the config's weights."""
    env = ex["env"]
    return env.plan_params(vx=[VX[g % 4] + 0.05 * (g // 4) for g in range(M)], height=[HEIGHT[g % 4] for g in range(M)])


def _plans(ctx, ex, M, seed=0, dc=None):
    """M distinct plans: perturbed start states, Ybar, noise scales and explicit noise."""
    dc = ex["dc"] if dc is None else dc
    env, nu = ex["env"], ctx.nu
    qs, qds = zip(*[perturbed_state(env, seed + g) for g in range(M)])
    states = ctx.env_reset_batch(_dev(np.stack(qs)), _dev(np.stack(qds)))
    rng = np.random.default_rng(100 + seed)
    _, sigma, _ = seeded_inputs(dc, nu)
    Ybars = 0.3 * rng.uniform(-1, 1, (M, dc.Hnode + 1, nu))
    scales = np.stack([sigma * (1.0 + 0.25 * (g % 4)) for g in range(M)])
    eps = rng.standard_normal((M, dc.Nsample, dc.Hnode + 1, nu))
    return states, _dev(Ybars), _dev(scales), _dev(eps)


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().copy() if v is not None else None) for k, v in out.items()}


def _same(a, b, what):
    for k in BARS:
        if a.get(k) is None or b.get(k) is None:
            assert a.get(k) is None and b.get(k) is None, (what, k)
            continue
        assert np.array_equal(a[k], b[k]), (what, k)


def _singles(ctx, rows, states, Ybars, scales, eps, want_bars=True):
    """Plan g alone on `ctx` (no binding) with the shared parameters set to row g."""
    out = []
    for g in range(len(rows)):
        ctx.set_user_params(rows[g])
        out.append(_host(ctx.reverse_once(states[g].contiguous(), Ybars[g].contiguous(), scales[g].contiguous(), eps[g].contiguous(),
                                          want_bars=want_bars)))
    return out


def test_batch_with_rows_equals_single_plans(ex):
    """1. Grouped reverse_once (explicit noise), M = 4 rows, full and lean == four single plans under set_user_params(row g); then
    the in-kernel RNG: M = 4 against single plans on rng_fill's rows of the global sample index, and M = 1 against reverse_once_rng
    under the same binding."""
    M = 4
    rows = _rows(ex, M)
    ctx = _ctx(ex, M=M)
    states, Ybars, scales, eps = _plans(ctx, ex, M)
    for want_bars in (True, False):
        ctx.set_plan_params(rows)
        batch = _host(ctx.reverse_once_batch(states, Ybars, scales, eps, want_bars=want_bars))
        ctx.set_plan_params(None)
        one = _singles(ctx, rows, states, Ybars, scales, eps, want_bars)
        for g in range(M):
            _same({k: (v[g] if v is not None else None) for k, v in batch.items()}, one[g], ("explicit", want_bars, g))
        assert len({float(one[g]["rews"][-1]) for g in range(M)}) == M   # the rows do change the plans' rewards
    # in-kernel noise: plan g draws global samples g N .. (g + 1) N - 1
    N, seed, counter = ex["dc"].Nsample, 11, 3
    ctx.set_plan_params(rows)
    batch = _host(ctx.reverse_once_batch_rng(states, Ybars, scales, seed, counter))
    ctx.set_plan_params(None)
    for g in range(M):
        ctx.set_user_params(rows[g])
        one = _host(ctx.reverse_once(states[g].contiguous(), Ybars[g].contiguous(), scales[g].contiguous(),
                                     ctx.rng_fill(seed, counter, g * N, N)))
        _same({k: (v[g] if v is not None else None) for k, v in batch.items()}, one, ("rng", g))
    # M = 1 under a binding is reverse_once_rng under the same binding: row 0, which differs from the shared parameters
    ctx.set_user_params(ex["params"])
    ctx.set_plan_params(rows[2:])
    b1 = _host(ctx.reverse_once_batch_rng(states[:1].contiguous(), Ybars[:1].contiguous(), scales[:1].contiguous(), seed, counter))
    s1 = _host(ctx.reverse_once_rng(states[0].contiguous(), Ybars[0].contiguous(), scales[0].contiguous(), seed, counter))
    _same({k: (v[0] if v is not None else None) for k, v in b1.items()}, s1, "rng M = 1")
    ctx.set_plan_params(None)
    ctx.set_user_params(rows[2])
    ref = _host(ctx.reverse_once_rng(states[0].contiguous(), Ybars[0].contiguous(), scales[0].contiguous(), seed, counter))
    _same(s1, ref, "row 0 == shared parameters set to it")
    ctx.set_user_params(ex["params"])
    shared = _host(ctx.reverse_once_rng(states[0].contiguous(), Ybars[0].contiguous(), scales[0].contiguous(), seed, counter))
    assert not np.array_equal(shared["rews"], s1["rews"])


def test_probe_plugin_reads_each_plans_row():
    """2. The probe reward (tests/plugin_probe.hip): plan g's row selects a different reward input; each plan's rewards == a single plan
    run with that selector as the shared parameters."""
    from dial_mpc_amd import _lib
    from plugin_cases import F, build_matrix, load_case
    path = build_matrix(["go2"])["go2"]
    c = load_case("go2", N=64, H=12)
    sel = np.array([[F["qpos"], 2], [F["qvel"], 0], [F["xpos"], 5], [F["ctrl"], 3]], np.float32)
    M = len(sel)
    ctx = _lib.Context(c["model"], c["ptask"], c["cfg"], plugin=path, user_params=[0, 0], options=dict(plan_cap=M))
    ex = dict(env=c["env"], dc=c["dc"])
    states, Ybars, scales, eps = _plans(ctx, ex, M, seed=20, dc=c["dc"])
    ctx.set_plan_params(sel)
    batch = _host(ctx.reverse_once_batch(states, Ybars, scales, eps))
    ctx.set_plan_params(None)
    one = _singles(ctx, sel, states, Ybars, scales, eps)
    for g in range(M):
        _same({k: v[g] for k, v in batch.items()}, one[g], ("probe", g))
    assert len({float(batch["rews"][g][0]) for g in range(M)}) == M


def test_example_rewards_per_row_match_numpy_mirror(ex):
    """3. env_step_batch with per-state vx / height: each state's reward == go2_height_walk.hip restated in numpy with ITS row, on the
    device's own returned states (tolerance of test_gpu_custom_env.test_rewards_match_numpy_mirror); the rows' rewards differ."""
    from dial_mpc_amd import _abi
    IREW = _abi.MACROS["DIAL_INFO_REWARD"]
    M = 4
    rows = _rows(ex, M)
    ctx = _ctx(ex, with_cfg=False)
    nq, nv, nb = ctx.nq, ctx.nv, ctx.nbody
    states = ctx.env_reset_batch(_dev(np.tile(ex["env"]._init_q, (M, 1))), _dev(np.zeros((M, nv))))
    acts = np.random.default_rng(7).uniform(-0.5, 0.5, (6, ctx.nu)).astype(np.float32)
    ctx.set_plan_params(rows)
    for t in range(6):
        states, xpos, xquat, ctrl = ctx.env_step_batch(states, _dev(np.tile(acts[t], (M, 1))))
        s, xp, xq, c = (v.cpu().numpy() for v in (states, xpos, xquat, ctrl))
        rews = []
        for g in range(M):
            want = _mirror_reward(rows[g], s[g, nq:nq + nv], xp[g].reshape(nb - 1, 3)[0], xq[g].reshape(nb - 1, 4)[0], c[g])
            got = float(s[g, nq + 2 * nv + IREW])
            assert abs(got - want) <= 1e-4 * abs(want) + 1e-5, (t, g, got, want)
            rews.append(got)
        assert len(set(rews)) == M, (t, rews)   # same state, same action: only the rows differ


def test_env_step_batch_with_rows_equals_single_steps(ex):
    """4. CustomEnv.step_batch(states, actions, user_params=rows) over several steps (info_user persists) == env.step of each state
    under set_user_params(row g)."""
    import torch
    env = ex["env"]
    M = 4
    rows = _rows(ex, M)
    start = [env.reset() for _ in range(M)]
    for g in range(M):
        q, qd = perturbed_state(env, 50 + g)
        start[g].packed[:env.sys.model["nq"]] = _dev(q)
    acts = _dev(np.random.default_rng(8).uniform(-0.6, 0.6, (5, M, len(env.joint_range))))
    batch = [s.replace() for s in start]
    traj = []
    for t in range(5):
        batch = env.step_batch(batch, acts[t], user_params=rows)
        traj.append([b.packed.clone() for b in batch])
    for g in range(M):
        env.set_user_params(vx=float(rows[g][0]), height=float(rows[g][1]))
        st = start[g].replace()
        for t in range(5):
            st = env.step(st, acts[t, g].contiguous())
            assert torch.equal(st.packed, traj[t][g]), (g, t)
    env.set_user_params(vx=ex["params"][0], height=ex["params"][1])


def test_rollout_queue_state_trace_and_relay_with_rows(ex):
    """5. A grouped launch beyond the resident rollouts (the rollout queue: one wavefront runs rollouts of different plans), one with
    the state trace bound (its traced states included), and a single-plan launch on the mean-trajectory relay -- each with rows bound
    == the single plans under set_user_params."""
    probe = _ctx(ex)
    slots = probe.lib.dial_debug_resident_rollouts(probe.h, 10 ** 6)
    del probe
    N = ex["dc"].Nsample
    M = (slots + slots // 2) // (N + 1) + 1
    rows = _rows(ex, M)
    ctx = _ctx(ex, M=M)
    assert 0 < ctx.lib.dial_debug_resident_rollouts(ctx.h, M * (N + 1)) < M * (N + 1)   # the queue runs
    states, Ybars, scales, eps = _plans(ctx, ex, M, seed=60)
    ctx.set_plan_params(rows)
    batch = _host(ctx.reverse_once_batch(states, Ybars, scales, eps))
    ctx.set_plan_params(None)
    one = _singles(ctx, rows, states, Ybars, scales, eps)
    for g in range(M):
        _same({k: v[g] for k, v in batch.items()}, one[g], ("queue", g))
    # state trace (plain grid, TRACE instantiation)
    Mt = 4
    trace = ctx.set_state_trace(Mt * (N + 1))
    ctx.set_plan_params(rows[:Mt])
    tb = _host(ctx.reverse_once_batch(states[:Mt].contiguous(), Ybars[:Mt].contiguous(), scales[:Mt].contiguous(), eps[:Mt].contiguous()))
    tr_b = trace.cpu().numpy().copy()
    ctx.set_plan_params(None)
    for g in range(Mt):
        _same({k: v[g] for k, v in tb.items()}, one[g], ("trace", g))
        ctx.set_user_params(rows[g])
        ctx.reverse_once(states[g].contiguous(), Ybars[g].contiguous(), scales[g].contiguous(), eps[g].contiguous())
        assert np.array_equal(tr_b[g * (N + 1):(g + 1) * (N + 1)], trace.cpu().numpy()[:N + 1]), ("traced states", g)
    ctx.set_state_trace(None)
    # the relay (relay_always: the mean trajectory in pieces) of a single-plan launch reads row 0
    rctx = _ctx(ex, relay_always=1)
    assert rctx.lib.dial_debug_resident_rollouts(rctx.h, N + 1) >= N + 1 + ex["dc"].Hsample + 1   # everything resident: the relay runs
    rctx.set_plan_params(rows[1:3])
    got = _host(rctx.reverse_once(states[0].contiguous(), Ybars[0].contiguous(), scales[0].contiguous(), eps[0].contiguous()))
    rctx.set_plan_params(None)
    rctx.set_user_params(rows[1])
    ref = _host(rctx.reverse_once(states[0].contiguous(), Ybars[0].contiguous(), scales[0].contiguous(), eps[0].contiguous()))
    _same(got, ref, "relay")


def test_unbinding_restores_the_shared_parameters(ex):
    """6. After set_plan_params(None), grouped plans, single plans and batched env.steps are bit-identical to a context that never
    bound rows."""
    M = 4
    rows = _rows(ex, M)
    fresh, used = _ctx(ex, M=M), _ctx(ex, M=M)
    states, Ybars, scales, eps = _plans(fresh, ex, M, seed=70)
    used.set_plan_params(rows)
    _host(used.reverse_once_batch(states, Ybars, scales, eps))
    used.env_step_batch(states, _dev(np.zeros((M, used.nu))))
    used.set_plan_params(None)
    _same(_host(used.reverse_once_batch(states, Ybars, scales, eps)), _host(fresh.reverse_once_batch(states, Ybars, scales, eps)), "batch")
    _same(_host(used.reverse_once(states[1].contiguous(), Ybars[1].contiguous(), scales[1].contiguous(), eps[1].contiguous())),
          _host(fresh.reverse_once(states[1].contiguous(), Ybars[1].contiguous(), scales[1].contiguous(), eps[1].contiguous())), "single")
    acts = _dev(np.random.default_rng(3).uniform(-0.5, 0.5, (M, used.nu)))
    a, b = used.env_step_batch(states, acts), fresh.env_step_batch(states, acts)
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())


def test_binding_errors_name_the_reason(ex):
    """7. M > rows (grouped launch, batched env.step), a shipped context, rows = 0 or > DIAL_MAX_PLANS with a pointer; and the planner
    refuses rows on a built-in env."""
    import torch
    from conftest import setup_case
    from dial_mpc_amd import _abi, _lib
    M = 4
    ctx = _ctx(ex, M=M)
    states, Ybars, scales, eps = _plans(ctx, ex, M, seed=80)
    ctx.set_plan_params(_rows(ex, 2))
    with pytest.raises(_lib.DialHipError, match="exceeds the 2 rows"):
        ctx.reverse_once_batch(states, Ybars, scales, eps)
    with pytest.raises(_lib.DialHipError, match="exceeds the 2 rows"):
        ctx.env_step_batch(states[:3].contiguous(), _dev(np.zeros((3, ctx.nu))))
    ctx.reverse_once_batch(states[:2].contiguous(), Ybars[:2].contiguous(), scales[:2].contiguous(), eps[:2].contiguous())   # M = rows: fine
    rows = torch.zeros((2, _abi.MACROS["DIAL_USER_PARAMS"]), device="cuda")
    for n in (0, -1, _abi.MACROS["DIAL_MAX_PLANS"] + 1):
        assert ctx.lib.dial_set_plan_params(ctx.h, rows.data_ptr(), n) == -1
        assert "outside 1 .. DIAL_MAX_PLANS" in ctx.lib.dial_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", 64, 8)
    shipped = _lib.Context(model, task, cfg)
    with pytest.raises(_lib.DialHipError, match="no task plugin"):
        shipped.set_plan_params(np.zeros((2, 3)))
    from dial_mpc_amd.core.dial_core import MBDPI
    mb = MBDPI(dc, env, n_plans=2)
    with pytest.raises(ValueError, match="task plugin"):
        mb.reverse_once_batch([env.reset(), env.reset()], 0, np.zeros((2, dc.Hnode + 1, model.nu)), mb.sigma_control,
                              user_params=np.zeros((2, 1)))


def test_closed_loop_env_param_equals_single_loops(ex, tmp_path):
    """8. dial-mpc --custom-env <example> --n-envs 4 --env-param vx=... for 5 ticks (a fresh child process) == four single closed loops
    with those vx, planned on the same noise (the batched driver's draws, plan g's slice), bit for bit on the executed states and the
    predictions."""
    import torch
    from dial_mpc_amd.core.dial_core import MBDPI, result_arrays
    ticks, M, vx = 5, 4, (0.3, 0.6, 0.9, 1.2)
    d = yaml.safe_load(open(EX_YAML))
    d.update(output_dir=str(tmp_path / "out"), Nsample=256, Ndiffuse_init=3, Ndiffuse=2)
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(d))
    penv = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "dial_mpc_amd.core.dial_core", "--custom-env", EX_MOD, "--config", str(p), "--n-steps", str(ticks),
                        "--n-envs", str(M), "--env-param", "vx=" + ",".join(str(v) for v in vx)],
                       cwd=ROOT, env=penv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    files = sorted(os.listdir(tmp_path / "out"))
    got_s = np.load(str(tmp_path / "out" / [f for f in files if f.endswith("_states.npy")][0]))
    got_p = np.load(str(tmp_path / "out" / [f for f in files if f.endswith("_predictions.npy")][0]))
    assert got_s.shape[:2] == (M, ticks) and got_p.shape[:2] == (M, ticks)
    dc, env, _ = _example(N=256, Ndiffuse_init=3, Ndiffuse=2)
    mbdpi = MBDPI(dc, env)
    gen = torch.Generator(device=mbdpi.device)   # the batched driver's noise: one [M, N, Hn1, nu] draw per iteration, in order
    gen.manual_seed(int(dc.seed))
    eps_tab = {}
    for t in range(ticks):
        for i in range(dc.Ndiffuse_init if t == 0 else dc.Ndiffuse):
            eps_tab[(t, i)] = torch.randn((M, dc.Nsample, dc.Hnode + 1, mbdpi.nu), generator=gen, device=mbdpi.device, dtype=torch.float32)
    for g in range(M):
        env.set_user_params(vx=vx[g])
        mbdpi.ctx.set_user_params(env.user_param_vector())
        state = env.reset()
        Y0 = torch.zeros((dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=mbdpi.device)
        rollout, infos = [], []
        for t in range(ticks):
            state = env.step(state, Y0[0])
            rollout.append(state)
            Y0 = mbdpi.shift(Y0)
            n_diffuse = dc.Ndiffuse_init if t == 0 else dc.Ndiffuse
            factors = mbdpi.sigma_control[None, :] * (dc.traj_diffuse_factor ** torch.arange(n_diffuse, device=mbdpi.device))[:, None]
            for i in range(n_diffuse):
                _, Y0, info = mbdpi.reverse_once(state, None, Y0, factors[i], eps=eps_tab[(t, i)][g].contiguous(),
                                                 want_bars=(i == n_diffuse - 1))
            infos.append(info)
        s_arr, p_arr = result_arrays(rollout, infos)
        assert np.array_equal(s_arr, got_s[g]), g
        assert np.array_equal(p_arr, got_p[g]), g
    assert not np.array_equal(got_s[0], got_s[3])
