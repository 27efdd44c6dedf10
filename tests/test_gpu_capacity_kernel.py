"""The capacity-dimension kernels (DimsMax, kernel instantiation 0) on the GPU against the fp32 oracle.

DimsMax is what every model that is none of the built-in robots runs on, and what dial_create falls back to (more than eight
impedance parameter sets, a Go2 task with n_frames != 1, dial_options.force_generic).  Its known failure mode is device code
generation (tools/isa/llvm_sink_bug.md: the LDS and the global-memory overflow copies of the constraint code), which the host wave
emulator cannot see -- so here every launch path of the device-compiled kernel is run and held to the oracle or, where a path must
not change a bit, to the plain launch: env.reset / env.step (single and batched), rollouts, reverse_once stage by stage, the
overflow area, the rollout queue, the state-trace instantiation, the mean-trajectory relay, grouped plans and the natural
fall-backs.  Every test asserts through Context.debug_last_launch which instantiation and launch path actually ran."""
import copy

import numpy as np
import pytest

from conftest import (CASES, TOL, agg_tol, perturbed_state, seeded_inputs, setup_case, transition_parity, transition_sample,
                      witness_parity)

pytestmark = pytest.mark.gpu

GEN = dict(force_generic=1)
LEGGED = [c for c in CASES if not c[0].startswith("allegro")]   # Go2 trot, Go2 seq-jump, H1 jog, H1 loco at the CASES sizes
CRATE, PUSH = "unitree_go2_crate_climb", "unitree_h1_push_crate"
SCRATCH = ("rewss", "qss", "qdss", "xss", "Y0s")


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _ctx(model, task, cfg, **opts):
    from dial_mpc_amd import _lib
    return _lib.Context(model, task, cfg, options={**GEN, **opts})


def _launch(ctx, **want):
    """The context's last rollout launch (debug_last_launch) must have the named fields; instantiation 0 unless stated."""
    got = ctx.debug_last_launch()
    for k, v in {"inst": 0, **want}.items():
        assert got[k] == v, (k, v, got)
    return got


def _start_states(example, env, o64):
    """(q, qd) start states: the keyframe and two perturbed states; the crate scenes' own touching poses."""
    if example == CRATE:
        from test_crate_climb import touching_state
        return [(np.array(env._init_q, np.float64), np.zeros(env.sys.nv))] + [touching_state(env, o64, s) for s in (0, 1)]
    if example == PUSH:
        from test_push_crate import pushing_state
        return [(np.array(env._init_q, np.float64), np.zeros(env.sys.nv))] + [pushing_state(env, o64, s) for s in (0, 1)]
    return [(np.array(env._init_q, np.float64), np.zeros(env.sys.nv))] + [perturbed_state(env, s) for s in (0, 1)]


MODELS = [(ex, N, H) for ex, N, H in LEGGED] + [(CRATE, 64, 8), (PUSH, 64, 8)]


def _state_gate(s_g, s_o, nq, nv):
    """test_gpu_parity.py::test_env_reset_and_step_match_oracle's gate of a packed state after env.reset: qacc_warmstart (the third
    block) is a difference of forces, its absolute error scales with the largest acceleration."""
    nqv = nq + nv
    atol = np.full(s_o.shape, 5e-4)
    atol[nqv:nqv + nv] = 5e-4 * max(1.0, float(np.abs(s_o[nqv:nqv + nv]).max()) * 1e-2)
    err = np.abs(s_g - s_o)
    assert np.all(err <= atol + 2e-4 * np.abs(s_o)), float(err.max())


@pytest.mark.parametrize("example,N,H", MODELS)
def test_env_reset_and_step_match_oracle(example, N, H):
    """env_reset_kernel / env_step_kernel<DimsMax>, one state and M = 3 states per launch (env_reset_batch / env_step_batch), under
    test_gpu_parity.py's gate: 10 steps of seeded actions, q within 1e-3, ctrl within 1e-3 rel + 2e-2, info.step counted."""
    import oracle as O
    dc, env, model, task, cfg = setup_case(example, N, H, per_rollout=True)
    o32, o64 = O.Oracle(model, task, cfg, np.float32), O.Oracle(model, task, cfg, np.float64)
    ctx = _ctx(model, task, cfg)
    _launch(ctx, blocks=0)                                            # the instantiation, before any rollout launch
    nq, nv = model.nq, model.nv
    starts = _start_states(example, env, o64)
    # one state per launch, from the keyframe
    s_o, xp_o, xq_o = o32.env_reset(env._init_q, np.zeros(nv))
    s_g, xp_g, xq_g = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(nv)))
    _state_gate(s_g.cpu().numpy(), s_o, nq, nv)
    assert np.allclose(xp_g.cpu().numpy(), xp_o, atol=1e-6) and np.allclose(xq_g.cpu().numpy(), xq_o, atol=1e-6)
    rng = np.random.default_rng(2)
    for _ in range(10):
        a = rng.uniform(-0.5, 0.5, model.nu).astype(np.float32)
        s_o, xp_o, xq_o, c_o = o32.env_step(s_o, a)
        s_g, xp_g, xq_g, c_g = ctx.env_step(s_g, _dev(a))
    sg = s_g.cpu().numpy()
    assert np.allclose(sg[:nq], s_o[:nq], atol=1e-3)
    assert np.allclose(c_g.cpu().numpy(), c_o, rtol=1e-3, atol=2e-2)
    assert sg[nq + 2 * nv] == 10.0                                    # info.step
    # M = 3 states per launch: the keyframe, and two perturbed (crate scenes: touching) states
    M = len(starts)
    S_g = ctx.env_reset_batch(_dev(np.stack([q for q, _ in starts])), _dev(np.stack([qd for _, qd in starts])))
    S_o = [o32.env_reset(q, qd)[0] for q, qd in starts]
    for m in range(M):
        _state_gate(S_g[m].cpu().numpy(), S_o[m], nq, nv)
    for _ in range(10):
        A = rng.uniform(-0.5, 0.5, (M, model.nu)).astype(np.float32)
        steps = [o32.env_step(S_o[m], A[m]) for m in range(M)]
        S_o = [st[0] for st in steps]
        S_g, XP_g, _, C_g = ctx.env_step_batch(S_g, _dev(A))
    Sg, Cg = S_g.cpu().numpy(), C_g.cpu().numpy()
    for m in range(M):
        assert np.allclose(Sg[m, :nq], S_o[m][:nq], atol=1e-3), (m, float(np.abs(Sg[m, :nq] - S_o[m][:nq]).max()))
        assert np.allclose(Cg[m], steps[m][3], rtol=1e-3, atol=2e-2), m
        assert Sg[m, nq + 2 * nv] == 10.0
    _launch(ctx, blocks=0)


@pytest.mark.parametrize("example,N,H", MODELS)
def test_rollouts_match_oracle(example, N, H):
    """dial_rollout on DimsMax's plain grid: 16 rollouts of seeded controls from the keyframe and two other start states, every
    rollout and step under the witness gate."""
    import oracle as O
    dc, env, model, task, cfg = setup_case(example, N, H, per_rollout=True)
    o32, o64 = O.Oracle(model, task, cfg, np.float32), O.Oracle(model, task, cfg, np.float64)
    ctx = _ctx(model, task, cfg)
    rng = np.random.default_rng(4)
    for q, qd in _start_states(example, env, o64):
        s0, _, _ = o32.env_reset(q, qd)
        us = rng.uniform(-0.8, 0.8, (16, H + 1, model.nu)).astype(np.float32)
        r_g = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
        _launch(ctx, blocks=16, wpb=1, queue=0, relay=0, trace=0, rollouts=16)
        witness_parity(o32, s0, us, r_g, example, model.nq + 2 * model.nv)


@pytest.mark.parametrize("example,N,H", LEGGED)
def test_reverse_once_matches_oracle_stagewise(example, N, H):
    """test_gpu_parity.py's stage-wise comparison on DimsMax: K1 exact to one fused multiply-add, K2 + K3 under the witness gate,
    the aggregates against the oracle where no rollout needed a witness, K4 recomputed in fp64 from the device's own rollouts."""
    import oracle as O
    dc, env, model, task, cfg = setup_case(example, N, H, per_rollout=True)
    o32 = O.Oracle(model, task, cfg, np.float32)
    ctx = _ctx(model, task, cfg)
    s0, _, _ = o32.env_reset(env._init_q, np.zeros(model.nv))
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=0, Ybar_scale=0.2)
    ro = o32.reverse_once(s0, Ybar, sigma, eps, full=True)
    out = ctx.reverse_once(_dev(s0), _dev(Ybar), _dev(sigma), _dev(eps))
    _launch(ctx, blocks=N + 1, queue=0, relay=0, trace=0, rollouts=N + 1)
    sc = ctx.debug_scratch()
    Y0s_ref = np.clip(np.concatenate([eps * sigma[None, :, None] + Ybar, Ybar[None]], 0), -1, 1)
    Y0s_ref[:-1, 0] = np.clip(Ybar[0], -1, 1)
    assert np.allclose(sc["Y0s"], Y0s_ref, rtol=0, atol=2.5e-7)          # K1
    rep = witness_parity(o32, s0, ro["us"], (sc["rewss"], sc["qss"], sc["qdss"], sc["xss"]), example, model.nq + 2 * model.nv)
    if rep["witnessed"] == 0:
        assert np.allclose(out["rews"].cpu().numpy(), ro["rews"], rtol=5e-4, atol=5e-4)
        assert np.allclose(sc["weights"], ro["weights"], **TOL["weights"])
        assert np.allclose(out["Ybar"].cpu().numpy(), ro["Ybar"], **agg_tol(example, "Ybar"))
        assert np.allclose(out["qbar"].cpu().numpy(), ro["qbar"], **agg_tol(example, "bar"))
        assert np.allclose(out["qdbar"].cpu().numpy(), ro["qdbar"], **agg_tol(example, "qdbar"))
        assert np.allclose(out["xbar"].cpu().numpy(), ro["xbar"], **agg_tol(example, "bar"))
    assert abs(sc["weights"].sum() - 1) < 1e-4
    rews_g = out["rews"].cpu().numpy().astype(np.float64)
    logp = (rews_g - rews_g[-1]) / rews_g.std() / float(cfg.temp_sample)
    w_ref = np.exp(logp - logp.max())
    w_ref /= w_ref.sum()
    assert np.allclose(sc["weights"], w_ref, rtol=2e-3, atol=1e-7)
    assert np.allclose(out["Ybar"].cpu().numpy(), np.einsum("n,nka->ka", w_ref, sc["Y0s"].astype(np.float64)), atol=2e-5)
    assert np.allclose(out["qbar"].cpu().numpy(), np.einsum("n,nti->ti", w_ref, sc["qss"].astype(np.float64)), atol=2e-5)
    assert np.allclose(out["qdbar"].cpu().numpy(), np.einsum("n,nti->ti", w_ref, sc["qdss"].astype(np.float64)), atol=5e-4)
    assert np.allclose(out["xbar"].cpu().numpy(), np.einsum("n,nti->ti", w_ref, sc["xss"].astype(np.float64)), atol=2e-5)


def _run(ctx, s0, Ybar, sigma, eps):
    """reverse_once, then host copies of its outputs and of the rollout scratch."""
    import torch
    out = ctx.reverse_once(_dev(s0), _dev(Ybar), _dev(sigma), _dev(eps))
    torch.cuda.synchronize()
    ctx.status()
    sc = ctx.debug_scratch()
    return {k: out[k].cpu().numpy() for k in ("Ybar", "rews", "qbar", "qdbar", "xbar")}, {k: np.array(sc[k]) for k in SCRATCH}


def _bit_equal(a, b, what):
    for k in a[0]:
        assert np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)), (what, k)
    for k in a[1]:
        assert np.array_equal(a[1][k].view(np.uint32), b[1][k].view(np.uint32)), (what, k, float(np.abs(a[1][k] - b[1][k]).max()))


def _touching(o64, model, q, qd):
    d = o64.forward_dump(q, qd)
    return int(np.sum(d["con_dist"] - np.array([model.con_margin[c] for c in range(model.ncon)]) < 0))


@pytest.mark.parametrize("example,N,H", [c for c in LEGGED if c[0] in ("unitree_go2_trot", "unitree_h1_jog")])
@pytest.mark.parametrize("cap", [1, 2])
def test_overflow_area_is_bit_identical_and_matches_oracle(example, N, H, cap):
    """con_cap = 1 / 2 with four feet on the ground: every standing step runs the constraint code's second copy on the overflow area
    in global memory.  Bit-identical to the full-size LDS workspace (con_cap < 0: no overflow areas at all), and the capped run
    under the oracle's witness gate, from the keyframe at rest and with perturbed velocities (both standing on four contacts)."""
    import oracle as O
    dc, env, model, task, cfg = setup_case(example, N, H, per_rollout=True)
    o32, o64 = O.Oracle(model, task, cfg, np.float32), O.Oracle(model, task, cfg, np.float64)
    capped, full = _ctx(model, task, cfg, con_cap=cap), _ctx(model, task, cfg, con_cap=-1)
    assert capped.lib.dial_lds_bytes(capped.h) < full.lib.dial_lds_bytes(full.h)
    q0 = np.array(env._init_q, np.float64)
    for seed, (q, qd) in enumerate([(q0, np.zeros(model.nv)), (q0, perturbed_state(env, 0)[1])]):
        assert _touching(o64, model, q, qd) > cap, "the start state must overflow the cap"
        s0, _, _ = o32.env_reset(q, qd)
        eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=seed, Ybar_scale=0.2)
        a = _run(capped, s0, Ybar, sigma, eps)
        _launch(capped, con_cap=cap, queue=0, relay=0, blocks=N + 1)
        b = _run(full, s0, Ybar, sigma, eps)
        _launch(full, con_cap=0, queue=0, relay=0, blocks=N + 1)
        _bit_equal(a, b, f"con_cap={cap} vs no cap")
        ro = o32.reverse_once(s0, Ybar, sigma, eps, full=True)
        witness_parity(o32, s0, ro["us"], tuple(a[1][k] for k in ("rewss", "qss", "qdss", "xss")), example, model.nq + 2 * model.nv)


@pytest.mark.parametrize("cap", [0, 1])
def test_rollout_queue_beyond_the_resident_set(cap):
    """A batch larger than DimsMax's resident set runs through the rollout queue (rollout_kernel<DimsMax, 1, 3, true>): bit-identical
    run to run and against one wavefront per rollout (no_queue), and the oracle's on a sample that includes the last rollouts (drawn
    from the queue) -- with the default cap and with con_cap = 1 (queue wavefronts on their overflow areas)."""
    import oracle as O
    example, H = "unitree_go2_trot", 8
    dc, env, model, task, cfg = setup_case(example, 64, H, per_rollout=True)
    probe = _ctx(model, task, cfg, con_cap=cap)
    slots = probe.lib.dial_debug_resident_rollouts(probe.h, 1 << 20)
    del probe
    assert slots > 0
    N = slots + 300                                                   # beyond the resident set by a good margin
    dc, env, model, task, cfg = setup_case(example, N, H, per_rollout=True)
    ctx = _ctx(model, task, cfg, con_cap=cap)
    assert ctx.lib.dial_debug_resident_rollouts(ctx.h, N + 1) == slots < N + 1
    o32 = O.Oracle(model, task, cfg, np.float32)
    s0, _, _ = o32.env_reset(env._init_q, np.zeros(model.nv))
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=3, Ybar_scale=0.1)
    runs = []
    for _ in range(2):
        runs.append(_run(ctx, s0, Ybar, sigma, eps))
        _launch(ctx, queue=1, blocks=slots, wpb=1, relay=0, rollouts=N + 1, con_cap=cap)
    _bit_equal(runs[0], runs[1], "run to run")
    ctx1 = _ctx(model, task, cfg, con_cap=cap, no_queue=1)
    one = _run(ctx1, s0, Ybar, sigma, eps)
    _launch(ctx1, queue=0, blocks=N + 1, con_cap=cap)
    _bit_equal(runs[0], one, "queue vs no_queue")
    # the sample's controls from K1 restated on the host (candidate nodes, held first node, mean row), interpolated as the oracle does
    idx = np.concatenate([np.random.default_rng(0).choice(N - 32, 96, replace=False), np.arange(N - 31, N + 1)])
    sc = runs[0][1]
    Y0s_ref = np.clip(np.concatenate([eps * sigma[None, :, None] + Ybar, Ybar[None]], 0), -1, 1)
    Y0s_ref[:-1, 0] = np.clip(Ybar[0], -1, 1)
    assert np.allclose(sc["Y0s"][idx], Y0s_ref[idx], rtol=0, atol=2.5e-7)
    W = np.array([[cfg.W[t][k] for k in range(dc.Hnode + 1)] for t in range(H + 1)], np.float32)
    us = np.einsum("tk,nka->nta", W, Y0s_ref[idx].astype(np.float32)).astype(np.float32)
    rep = witness_parity(o32, s0, us, tuple(sc[k][idx] for k in ("rewss", "qss", "qdss", "xss")), example, model.nq + 2 * model.nv)
    assert rep["rollouts"] == len(idx)


@pytest.mark.parametrize("example,N,H,cap", [("unitree_go2_trot", 64, 8, 0), ("unitree_go2_trot", 64, 8, 1), ("unitree_h1_jog", 32, 16, 0)])
def test_state_trace_instantiation(example, N, H, cap):
    """set_state_trace switches to rollout_kernel<DimsMax, 1, 3, false, true>: its rows are the plain launch's qss / qdss, the
    rollouts are bit-identical with and without the trace, and a transition_parity pass from the device's own traced states holds
    under the shipped line-search rule."""
    import oracle as O
    dc, env, model, task, cfg = setup_case(example, N, H)
    o32 = O.Oracle(model, task, cfg, np.float32)
    ctx = _ctx(model, task, cfg, con_cap=cap)
    eff_cap = cap                                                     # (con_cap 0 on these models: no overflow areas)
    q, qd = perturbed_state(env, 2)
    s0, _, _ = o32.env_reset(q, qd)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=1, Ybar_scale=0.2)
    plain = _run(ctx, s0, Ybar, sigma, eps)
    _launch(ctx, trace=0, con_cap=eff_cap)
    trace_dev = ctx.set_state_trace(N + 1)
    traced = _run(ctx, s0, Ybar, sigma, eps)
    _launch(ctx, trace=1, queue=0, relay=0, blocks=N + 1, con_cap=eff_cap)
    _bit_equal(plain, traced, "with vs without the state trace")
    tr = trace_dev.cpu().numpy()
    nq, nv = model.nq, model.nv
    assert np.array_equal(tr[:, :, :nq], plain[1]["qss"]) and np.array_equal(tr[:, :, nq:nq + nv], plain[1]["qdss"])
    assert np.array_equal(tr[:, :, nq + 2 * nv], np.broadcast_to(np.arange(1, H + 2, dtype=np.float32), (N + 1, H + 1)))   # info.step
    W = np.array([[cfg.W[t][k] for k in range(dc.Hnode + 1)] for t in range(H + 1)], np.float32)
    us = np.einsum("tk,nka->nta", W, plain[1]["Y0s"]).astype(np.float32)
    got = tuple(plain[1][k] for k in ("rewss", "qss", "qdss", "xss"))
    transition_parity(o32, s0, us, got, tr, transition_sample(N, 24, 0), nq, nv, example=example)
    ctx.set_state_trace(None)
    _run(ctx, s0, Ybar, sigma, eps)
    _launch(ctx, trace=0)


@pytest.mark.parametrize("example,N,H", [("unitree_go2_trot", 256, 16), ("unitree_h1_jog", 128, 12)])
@pytest.mark.parametrize("cap", [0, 1])
def test_mean_trajectory_relay(example, N, H, cap):
    """DimsMax relays (one wavefront per workgroup): with relay_always the mean trajectory runs as ceil(T / 3) pieces on as many
    wavefronts, each with its own overflow area -- bit-identical to no_relay over three chained iterations, with the default cap and
    with con_cap = 1 (every touching step of every piece on the overflow area: ADVICE round 3)."""
    import torch
    dc, env, model, task, cfg = setup_case(example, N, H)
    ctx = _ctx(model, task, cfg, con_cap=cap, relay_always=1)
    ctx0 = _ctx(model, task, cfg, con_cap=cap, no_relay=1)
    pieces = (H + 1 + 2) // 3
    s0, _, _ = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(model.nv)))
    s0 = s0.cpu().numpy()
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=4, Ybar_scale=0.1)
    for it in range(3):                                               # the turn flag re-arms itself between launches
        a = _run(ctx, s0, Ybar, sigma, eps)
        _launch(ctx, relay=1, queue=0, blocks=N + pieces, con_cap=cap, rollouts=N + 1)
        b = _run(ctx0, s0, Ybar, sigma, eps)
        _launch(ctx0, relay=0, queue=0, blocks=N + 1, con_cap=cap)
        _bit_equal(a, b, f"relay vs no_relay, iteration {it}")
        assert np.isfinite(a[1]["rewss"]).all()
        Ybar = a[0]["Ybar"]
    torch.cuda.synchronize()
    ctx.status()


@pytest.mark.parametrize("example,N,H", [("unitree_go2_trot", 64, 8), ("unitree_h1_jog", 32, 16)])
def test_grouped_plans_equal_single_plans(example, N, H):
    """plan_cap = 3, con_cap = 1: dial_reverse_once_batch from three different states (overflow slots sized plan_cap x B_cap) equals
    three single-plan calls bit for bit."""
    import torch
    dc, env, model, task, cfg = setup_case(example, N, H)
    M = 3
    ctx = _ctx(model, task, cfg, con_cap=1, plan_cap=M)
    qs, qds = zip(*[perturbed_state(env, 10 + g) for g in range(M)])
    states = ctx.env_reset_batch(_dev(np.stack(qs)), _dev(np.stack(qds)))
    rng = np.random.default_rng(7)
    _, sigma, _ = seeded_inputs(dc, model.nu)
    Ybars = _dev(0.3 * rng.uniform(-1, 1, (M, dc.Hnode + 1, model.nu)))
    scales = _dev(np.stack([sigma * (1.0 + 0.25 * g) for g in range(M)]))
    eps = _dev(rng.standard_normal((M, N, dc.Hnode + 1, model.nu)))
    out = {k: v.clone() for k, v in ctx.reverse_once_batch(states, Ybars, scales, eps).items()}
    _launch(ctx, con_cap=1, queue=0, relay=0, blocks=M * (N + 1), rollouts=M * (N + 1))
    for g in range(M):
        one = ctx.reverse_once(states[g].contiguous(), Ybars[g].contiguous(), scales[g].contiguous(), eps[g].contiguous())
        _launch(ctx, con_cap=1, blocks=N + 1, rollouts=N + 1)
        for k in ("Ybar", "rews", "qbar", "qdbar", "xbar"):
            assert torch.equal(out[k][g], one[k]), (g, k)
    assert torch.isfinite(out["rews"]).all()


def _twelve_sets(model0):
    model = copy.deepcopy(model0)
    for l in range(model.nlim):
        model.jnt_solimp[model.lim_jnt[l]][0] = 0.9 - 0.002 * l          # every limited joint its own (solref, solimp) row
    return model


@pytest.mark.parametrize("case", ["n_frames=2", "twelve impedance sets"])
def test_natural_fallbacks_dispatch_to_the_capacity_kernel(case):
    """Without force_generic, dial_create picks DimsMax for a Go2 trot at two physics steps per control step and for a Go2 whose
    limit rows carry twelve distinct impedance parameter sets; both under the witness gate, rollouts and reverse_once."""
    import oracle as O
    from dial_mpc_amd import _lib
    N, H = 64, 8
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, H, per_rollout=True)
    q0 = np.array(env._init_q, np.float64)
    if case == "n_frames=2":
        model.timestep = task.dt / 2
        task.n_frames = 2
    else:
        model = _twelve_sets(model)
        for l in range(0, model.nlim, 2):                             # several joints past their limits: the rows matter
            j = model.lim_jnt[l]
            q0[model.jnt_qposadr[j]] = model.jnt_range[j][1] + 0.02
    ctx = _lib.Context(model, task, cfg)
    _launch(ctx, blocks=0)
    o32 = O.Oracle(model, task, cfg, np.float32)
    rng = np.random.default_rng(6)
    for q, qd in ((q0, np.zeros(model.nv)), perturbed_state(env, 0)):
        s0, _, _ = o32.env_reset(q, qd)
        us = rng.uniform(-0.8, 0.8, (16, H + 1, model.nu)).astype(np.float32)
        r_g = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
        _launch(ctx, blocks=16, queue=0, relay=0)
        witness_parity(o32, s0, us, r_g, "unitree_go2_trot", model.nq + 2 * model.nv)
    s0, _, _ = o32.env_reset(q0, np.zeros(model.nv))
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=0, Ybar_scale=0.2)
    ro = o32.reverse_once(s0, Ybar, sigma, eps, full=True)
    _, sc = _run(ctx, s0, Ybar, sigma, eps)
    _launch(ctx, blocks=N + 1)
    witness_parity(o32, s0, ro["us"], tuple(sc[k] for k in ("rewss", "qss", "qdss", "xss")), "unitree_go2_trot", model.nq + 2 * model.nv)


def test_force_generic_is_refused_for_elliptic_cones():
    """The capacity-dimension kernel has no elliptic-cone solver: force_generic on the Allegro hand fails with DIAL_ERR_UNSUPPORTED
    instead of being ignored; without it the hand gets its own instantiation (4)."""
    from dial_mpc_amd import _abi, _lib
    dc, env, model, task, cfg = setup_case("allegro_reorient", 64, 8)
    for c in (cfg, None):                                             # (planner contexts and env / plant-only ones alike)
        with pytest.raises(_lib.DialHipError, match="elliptic-cone models need a dimension-specialised instantiation") as e:
            _ctx(model, task, c)
        assert f"({_abi.MACROS['DIAL_ERR_UNSUPPORTED']})" in str(e.value)
    ctx = _lib.Context(model, task, cfg)
    _launch(ctx, inst=4, blocks=0)
