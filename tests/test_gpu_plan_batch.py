"""Grouped planning on the GPU: M independent reverse_once iterations of one context in one launch (dial_reverse_once_batch) against
M single-plan calls, bit for bit where both run the same kernel instantiation, and against the fp32 oracle where they do not."""
import ctypes

import numpy as np
import pytest

from conftest import seeded_inputs, setup_case, witness_parity
from dial_mpc_amd.utils.synthetic import perturbed_state

pytestmark = pytest.mark.gpu

BARS = ("Ybar", "qbar", "qdbar", "xbar")


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _plans(ctx, env, dc, model, M, seed=0):
    """M distinct plans: perturbed start states, Ybar, noise scales and noise."""
    qs, qds = zip(*[perturbed_state(env, seed + g) for g in range(M)])
    states = ctx.env_reset_batch(_dev(np.stack(qs)), _dev(np.stack(qds)))
    rng = np.random.default_rng(100 + seed)
    _, sigma, _ = seeded_inputs(dc, model.nu)
    Ybars = (0.3 * rng.uniform(-1, 1, (M, dc.Hnode + 1, model.nu))).astype(np.float32)
    scales = np.stack([sigma * (1.0 + 0.25 * g) for g in range(M)]).astype(np.float32)
    eps = rng.standard_normal((M, dc.Nsample, dc.Hnode + 1, model.nu)).astype(np.float32)
    return states, _dev(Ybars), _dev(scales), _dev(eps)


def _equal(a, b):
    import torch
    return a is None and b is None or torch.equal(a, b)


@pytest.mark.parametrize("example,H", [("unitree_go2_trot", 8), ("unitree_h1_jog", 16), ("unitree_h1_loco", 20),
                                       ("allegro_reorient", 8)])
def test_batch_equals_single_plans_bit_for_bit(example, H):
    from dial_mpc_amd import _lib
    N, M = 64, 4
    dc, env, model, task, cfg = setup_case(example, N, H)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
    states, Ybars, scales, eps = _plans(ctx, env, dc, model, M)
    for want_bars in (True, False):
        out = ctx.reverse_once_batch(states, Ybars, scales, eps, want_bars=want_bars)
        for g in range(M):
            one = ctx.reverse_once(states[g].contiguous(), Ybars[g].contiguous(), scales[g].contiguous(), eps[g].contiguous(),
                                   want_bars=want_bars)
            assert _equal(out["rews"][g], one["rews"]), (g, want_bars)
            for k in BARS:
                got = out[k][g] if out[k] is not None else None
                assert _equal(got, one[k]), (g, k, want_bars)
        assert (out["qbar"] is None) == (not want_bars)


@pytest.mark.parametrize("example,H", [("unitree_go2_trot", 8), ("unitree_h1_jog", 16), ("allegro_reorient", 8)])
def test_in_kernel_noise_is_rng_fill_of_the_global_sample_index(example, H):
    """(H1: C = 114 elements per sample, the last Philox quad is cut after two.)  The candidate nodes the rollouts drew are
    clip(rng_fill sigma + Ybar) with node 0 held at clip(Ybar[0]), the mean row clip(Ybar), plan by plan."""
    import torch
    import planner_ref as R
    from dial_mpc_amd import _lib
    N, M, seed, counter = 64, 3, 4242, 7
    dc, env, model, task, cfg = setup_case(example, N, H)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
    states, Ybars, scales, _ = _plans(ctx, env, dc, model, M, seed=3)
    got = {k: v.clone() if v is not None else None for k, v in ctx.reverse_once_batch_rng(states, Ybars, scales, seed, counter).items()}
    nodes = R.download(ctx, "Y0s", M * (N + 1)).reshape(M, N + 1, -1)
    eps = ctx.rng_fill(seed, counter, 0, M * N).reshape(M, N, dc.Hnode + 1, model.nu).contiguous()
    for g in range(M):
        want, mag, _ = R.candidate_nodes(eps[g].cpu().numpy().reshape(N, -1), Ybars[g].cpu().numpy(), scales[g].cpu().numpy(), model.nu)
        assert np.all(np.abs(nodes[g] - want) <= 2 * R.U * mag), g      # (one fp32 multiply-add, or a multiply and an add)
    ref = ctx.reverse_once_batch(states, Ybars, scales, eps)
    for k in ("rews",) + BARS:
        assert torch.equal(got[k], ref[k]), k
    one = ctx.reverse_once_rng(states[0].contiguous(), Ybars[0].contiguous(), scales[0].contiguous(), seed, counter)
    for k in ("rews",) + BARS:
        assert torch.equal(got[k][0], one[k]), k
    assert not torch.equal(got["rews"][1], got["rews"][0])


def _batch_scratch(ctx, rows):
    """Host copies of the rollout scratch of the last launch, `rows` batch rollouts (debug_scratch with the grouped row count)."""
    import torch
    from dial_mpc_amd import _lib
    ptrs = [ctypes.c_void_p() for _ in range(6)]
    assert ctx.lib.dial_debug_scratch(ctx.h, *[ctypes.byref(p) for p in ptrs]) == 0
    T = ctx.cfg.Hsample + 1
    shapes = [(rows, T), (rows, T, ctx.nq), (rows, T, ctx.nv), (rows, T, ctx.nx)]
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    out = []
    for p, shp in zip(ptrs[1:5], shapes):
        host = np.empty(shp, np.float32)
        rc = hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), p, ctypes.c_size_t(host.nbytes), ctypes.c_int(2))
        if rc != 0:
            raise _lib.DialHipError(f"hipMemcpy failed ({rc})")
        out.append(host)
    return out


def test_large_go2_batch_matches_the_oracle():
    """N = 2048, M = 4: 8196 rollouts -- beyond the resident set, on the pair kernel's rollout queue.  Every plan's rollouts (a
    sample of each, the mean trajectory included) follow the fp32 oracle of THAT plan's inputs, step by step."""
    import oracle as O
    from dial_mpc_amd import _lib
    N, H, M = 2048, 16, 4
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, H, per_rollout=True)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
    assert ctx.lib.dial_debug_resident_rollouts(ctx.h, M * (N + 1)) < M * (N + 1)
    states, Ybars, scales, eps = _plans(ctx, env, dc, model, M, seed=11)
    out = ctx.reverse_once_batch(states, Ybars, scales, eps)
    rewss, qss, qdss, xss = _batch_scratch(ctx, M * (N + 1))
    o32 = O.Oracle(model, task, cfg, np.float32)
    pick = np.concatenate([np.random.default_rng(5).choice(N, 96, replace=False), [N]])
    for g in range(M):
        s0 = states[g].cpu().numpy()
        ro = o32.reverse_once(s0, Ybars[g].cpu().numpy(), scales[g].cpu().numpy(), eps[g].cpu().numpy(), full=True)
        rows = g * (N + 1) + pick
        rep = witness_parity(o32, s0, ro["us"][pick], (rewss[rows], qss[rows], qdss[rows], xss[rows]), "unitree_go2_trot",
                             model.nq + 2 * model.nv)
        assert rep["rollouts"] == len(pick)
        assert np.isfinite(out["Ybar"][g].cpu().numpy()).all()
        if rep["witnessed"] == 0:
            assert np.allclose(out["rews"][g].cpu().numpy()[pick], ro["rews"][pick], rtol=5e-4, atol=5e-4)


def test_degenerate_plan_is_nan_alone():
    """Plan 1 with noise scale 0: its N + 1 rollouts are one trajectory, std = 0, and its Ybar is NaN (the reference's 0/0).  The other
    plans are untouched: equal to their single-plan results."""
    import torch
    from dial_mpc_amd import _lib
    N, M = 63, 4   # N + 1 = 64: the mean of equal rewards is exact
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, 8)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
    states, Ybars, scales, eps = _plans(ctx, env, dc, model, M, seed=21)
    scales[1].zero_()
    out = ctx.reverse_once_batch(states, Ybars, scales, eps)
    rews1 = out["rews"][1].cpu().numpy()
    assert (rews1 == rews1[-1]).all()
    for k in BARS:
        assert torch.isnan(out[k][1]).all(), k
    for g in (0, 2, 3):
        one = ctx.reverse_once(states[g].contiguous(), Ybars[g].contiguous(), scales[g].contiguous(), eps[g].contiguous())
        for k in ("rews",) + BARS:
            assert torch.isfinite(out[k][g]).all() and torch.equal(out[k][g], one[k]), (g, k)


@pytest.mark.parametrize("example", ["unitree_go2_trot", "unitree_h1_jog"])
def test_shift_and_env_step_batches_equal_single_calls(example):
    import torch
    from dial_mpc_amd import _lib
    M = 5
    dc, env, model, task, cfg = setup_case(example, 16, 8)
    ctx = _lib.Context(model, task, cfg)
    rng = np.random.default_rng(9)
    Y = _dev(rng.uniform(-1, 1, (M, dc.Hnode + 1, model.nu)))
    Ys = ctx.shift_batch(Y)
    for g in range(M):
        assert torch.equal(Ys[g], ctx.shift(Y[g].contiguous())), g
    states, _, _, _ = _plans(ctx, env, dc, model, M, seed=30)
    acts = _dev(rng.uniform(-1, 1, (M, model.nu)))
    st, xpos, xquat, ctrl = ctx.env_step_batch(states, acts)
    for g in range(M):
        s1, x1, q1, c1 = ctx.env_step(states[g].contiguous(), acts[g].contiguous())
        for a, b in ((st[g], s1), (xpos[g], x1), (xquat[g], q1), (ctrl[g], c1)):
            assert torch.equal(a, b), g


def test_batched_closed_loop_equals_single_loops():
    """Five ticks of three closed loops planned together (explicit noise) == three single-plan loops on the same noise."""
    import torch
    from dial_mpc_amd.core.dial_core import MBDPI, batched_loop
    M, ticks = 3, 5
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", 64, 8)
    dc.Ndiffuse_init, dc.Ndiffuse = 3, 2
    mbdpi = MBDPI(dc, env, n_plans=M)
    gen = torch.Generator(device=mbdpi.device)
    gen.manual_seed(123)
    eps_tab = {(t, i): torch.randn((M, dc.Nsample, dc.Hnode + 1, mbdpi.nu), generator=gen, device=mbdpi.device)
               for t in range(ticks) for i in range(dc.Ndiffuse_init)}
    qs, qds = zip(*[perturbed_state(env, 40 + g) for g in range(M)])
    start = [env.reset() for _ in range(M)]
    for g in range(M):   # distinct start states: the keyframe's state with a perturbed pose
        start[g].packed[:model.nq] = _dev(qs[g])
        start[g].packed[model.nq:model.nq + model.nv] = _dev(qds[g])
    rollouts, infos, _ = batched_loop(mbdpi, env, [s.replace() for s in start], ticks, eps_fn=lambda t, i: eps_tab[(t, i)])
    for g in range(M):
        state = start[g].replace()
        Y0 = torch.zeros((dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=mbdpi.device)
        for t in range(ticks):
            state = env.step(state, Y0[0])
            assert torch.equal(state.packed, rollouts[t][g].packed), (g, t)
            Y0 = mbdpi.shift(Y0)
            n_diffuse = dc.Ndiffuse_init if t == 0 else dc.Ndiffuse
            factors = mbdpi.sigma_control[None, :] * (dc.traj_diffuse_factor ** torch.arange(n_diffuse, device=mbdpi.device))[:, None]
            for i in range(n_diffuse):
                _, Y0, info = mbdpi.reverse_once(state, None, Y0, factors[i], eps=eps_tab[(t, i)][g].contiguous(),
                                                 want_bars=(i == n_diffuse - 1))
            assert torch.equal(info["xbar"], infos[t]["xbar"][g]), (g, t)
            assert torch.equal(info["rews"], infos[t]["rews"][g]), (g, t)


def test_grouped_call_errors_name_the_reason():
    from dial_mpc_amd import _lib
    N, M = 32, 2
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, 8)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
    states, Ybars, scales, eps = _plans(ctx, env, dc, model, M + 1)
    outs = ctx._out_batch(M + 1, True)

    def call(c, m, ns):
        return c.lib.dial_reverse_once_batch(c.h, states.data_ptr(), Ybars.data_ptr(), scales.data_ptr(), ns, eps.data_ptr(), m,
                                             outs["Ybar"].data_ptr(), outs["rews"].data_ptr(), None, None, None, None)

    Hn1 = dc.Hnode + 1
    for c, m, ns, words in ((ctx, M + 1, Hn1, "plan capacity"), (ctx, 0, Hn1, "plan capacity"), (ctx, M, 3, "ns")):
        assert call(c, m, ns) == -1
        assert words in c.lib.dial_last_error(c.h).decode()
    sharded = _lib.Context(model, task, cfg, n_local_cap=N // 2, options=dict(plan_cap=M))
    assert call(sharded, M, Hn1) == -1
    assert "sharded" in sharded.lib.dial_last_error(sharded.h).decode()
    with pytest.raises(_lib.DialHipError, match="plan capacity"):
        ctx.reverse_once_batch(states, Ybars, scales, eps)
    assert call(ctx, M, Hn1) == 0   # within the capacity: fine
