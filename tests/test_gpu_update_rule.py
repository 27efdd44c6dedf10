"""GPU tests of the update rules (dial_set_update_rule / dial_get_weights; csrc/update_rule.h: elite_weights_kernel).

1. The kernel on synthetic rewards, bit for bit against tests/update_rule_ref.py (the contract in NumPy): sizes on both sides of its
   64-lane wavefronts and 1024-index chunks up to the weights buffer's 65537, elite counts at both ends, reward profiles that put the
   K-th place inside a tie group, across a chunk boundary, among NaNs, signed zeros, infinities and denormals; the same rewards
   through the sharded phase B's packing pass.
2. Every planning path: reverse_once (explicit and in-kernel noise), grouped plans, a bound ensemble, a task plugin.  The rollouts are
   untouched, so the rewards equal the softmax context's bit for bit; the weights are the reference of those rewards; the bars are the
   K4b sums of those weights (tests/planner_ref.py's bounds), and under the best-sample rule the best candidate's rows themselves.
3. Binding, errors.  4. A short closed loop under both rules."""
import numpy as np
import pytest

import planner_ref as R
from conftest import setup_case
from update_rule_ref import elite_weights_ref

pytestmark = pytest.mark.gpu

N_GLOBAL, N_LOCAL = 65536, 64
SIZES = (2, 3, 64, 65, 1024, 1025, 2049, 65537)
SEGS = ("Y0s", "qss", "qdss", "xss")
_CTX = {}


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    _CTX.clear()


def _sharded():
    """One dial_create_sharded context (Go2): W_cap = 65537 weights."""
    from dial_mpc_amd import _lib
    if "sharded" not in _CTX:
        dc, env, model, task, cfg = setup_case("unitree_go2_trot", N_GLOBAL, 4)
        _CTX["sharded"] = (_lib.Context(model, task, cfg, n_local_cap=N_LOCAL), dc, model)
    return _CTX["sharded"]


def _elite_counts(B):
    return sorted({1, min(2, B), -(-B // 10), max(1, B - 1), B})


# ------------------------------------------------------------------------------------------------------------- 1. the kernel
def _spread(B, count, rng):
    """`count` indices spread over every 1024-index chunk of 0 .. B - 1, with a run across 1023 / 1024 where B reaches it."""
    count = max(0, min(B, count))
    run = [i for i in range(1020, 1028) if i < B][:count]
    rest = np.setdiff1d(np.arange(B), run)
    extra = rest[np.unique(np.linspace(0, rest.size - 1, count - len(run)).astype(np.int64))] if count > len(run) and rest.size else []
    return np.unique(np.concatenate([run, extra]).astype(np.int64))


def _profile(name, B, K, rng):
    r = rng.standard_normal(B).astype(np.float32)
    if name == "equal":
        r[:] = 0.25
    elif name == "two_low":        # fewer ones than K: the K-th place lies among the zeros, which fill every chunk
        r[:] = 0.0
        r[_spread(B, K // 2, rng)] = 1.0
    elif name == "two_high":       # more ones than K, spread over every chunk and across 1023 / 1024: the K-th place lies among them
        r[:] = 0.0
        r[_spread(B, 2 * K + 3, rng)] = 1.0
    elif name == "zeros":          # -0 and +0 are one tie group, below the ones and above the minus ones
        r = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0], np.float32), B)
    elif name == "inf":
        r[rng.integers(0, B, max(1, B // 7))] = np.inf
        r[rng.integers(0, B, max(1, B // 5))] = -np.inf
    elif name == "nan_few":        # K below and above the count of numbers as K runs to B
        r[[0, B // 2, B - 1]] = np.nan
    elif name == "nan_many":
        r[rng.random(B) < 0.6] = np.nan
        r[[0, B // 2, B - 1]] = np.nan
        neg = np.isnan(r) & (rng.random(B) < 0.5)            # NaNs of either sign and other payloads
        r.view(np.uint32)[neg] = 0xFFC00001
    elif name == "denormal":
        bits = rng.integers(1, 0x800000, B).astype(np.uint32) | (rng.integers(0, 2, B).astype(np.uint32) << 31)
        r = bits.view(np.float32).copy()
        r[rng.integers(0, B, 2)] = 0.0
    elif name == "increasing":
        r = np.arange(B, dtype=np.float32) - B / 2
    elif name == "decreasing":
        r = B / 2 - np.arange(B, dtype=np.float32)
    else:
        assert name == "normal"
    return np.ascontiguousarray(r, np.float32)


PROFILES = ["normal", "equal", "two_low", "two_high", "zeros", "inf", "nan_few", "nan_many", "denormal", "increasing", "decreasing"]


def _gathered(rews, n_total, world):
    per = -(-n_total // world)
    g = np.zeros((world, per + 1), np.float32)
    for k in range(world):
        part = rews[k * per:min((k + 1) * per, n_total)]
        g[k, :part.size] = part
        g[k, per] = rews[n_total] if k == 0 else np.float32(123.0)   # only rank 0's copy of the mean reward is read
    return g.reshape(-1), per


@pytest.mark.parametrize("profile", PROFILES)
def test_elite_weights_match_the_reference_bit_for_bit(profile):
    import torch
    ctx, dc, model = _sharded()
    Hn1, nu = dc.Hnode + 1, model.nu
    packed = torch.empty(ctx.packed_size(), dtype=torch.float32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    eps0, Ybar = torch.zeros((N_GLOBAL, Hn1, nu), **f32), torch.zeros((Hn1, nu), **f32)
    sigma, Yout, rews_all = torch.ones(Hn1, **f32), torch.empty((Hn1, nu), **f32), torch.empty(N_GLOBAL + 1, **f32)
    rng = np.random.default_rng(PROFILES.index(profile))
    try:
        for B in SIZES:
            for K in _elite_counts(B):
                r = _profile(profile, B, K, rng)
                ref = elite_weights_ref(r, K)
                ctx.set_update_rule("elite", K)
                ctx.shard_reduce(_dev(r), B - 1, 0, 0, False, packed)
                w = ctx.weights(1).cpu().numpy()[0, :B]
                assert int(np.count_nonzero(_bits(w))) == K, (profile, B, K)
                assert np.array_equal(_bits(w), _bits(ref)), (profile, B, K, np.flatnonzero(_bits(w) != _bits(ref))[:8])
                # the same rewards as an all-gather of 4 ranks delivers them: packed on the way, the same weights
                g, per = _gathered(r, B - 1, 4)
                rews_all.fill_(-7.0)
                ctx.shard_ybar_gathered(_dev(g), 4, per, B - 1, eps0, Ybar, sigma, rews_all, Yout)
                wg = ctx.weights(1).cpu().numpy()[0, :B]
                assert np.array_equal(_bits(wg), _bits(ref)), (profile, B, K, "gathered")
                assert np.array_equal(_bits(rews_all.cpu().numpy()[:B]), _bits(r)), (profile, B, K, "packing")
                if B <= N_GLOBAL:
                    assert float(rews_all[B]) == -7.0, (profile, B, K, "packing wrote past n_total + 1")
    finally:
        ctx.set_update_rule("mppi")


# ------------------------------------------------------------------------------------------------------------- 2. planning paths
M = 3


def _plan(N):
    """Go2 trot at Nsample = N, H = 4, plan capacity 3: an mppi context (never rebound), one to rebind, and shared inputs."""
    from dial_mpc_amd import _lib
    from dial_mpc_amd.utils.synthetic import perturbed_state
    key = ("plan", N)
    if key not in _CTX:
        dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, 4)
        ref = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
        ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
        qs, qds = zip(*[perturbed_state(env, g) for g in range(M)])
        rng = np.random.default_rng(N)
        Hn1 = dc.Hnode + 1
        inp = dict(states=ref.env_reset_batch(_dev(np.stack(qs)), _dev(np.stack(qds))),
                   Ybars=_dev(0.3 * rng.uniform(-1, 1, (M, Hn1, model.nu))),
                   scales=_dev(np.stack([np.full(Hn1, 0.2 + 0.1 * g) for g in range(M)])),
                   eps=_dev(rng.standard_normal((M, N, Hn1, model.nu))))
        _CTX[key] = dict(dc=dc, env=env, model=model, task=task, cfg=cfg, ref=ref, ctx=ctx, inp=inp)
    return _CTX[key]


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items() if v is not None}


def _once(ctx, inp, g=0):
    return _host(ctx.reverse_once(inp["states"][g].contiguous(), inp["Ybars"][g].contiguous(), inp["scales"][g].contiguous(),
                                  inp["eps"][g].contiguous()))


def _check_bars(out, w, rows, inp, g, nu):
    """out's bars against the fp64 sums of weights w over the scratch rows of one plan (a dict of [N + 1, C] arrays)."""
    for s, k in zip(SEGS, ("Ybar", "qbar", "qdbar", "xbar")):
        ref, bound = R.wsum_ref(w, rows[s])
        err = out[k].reshape(-1) - ref
        assert np.all(np.abs(err) <= bound), (k, R.worst(err, bound))
    ref, bound = R.ybar_ref(w, inp["eps"][g].cpu().numpy().reshape(w.size - 1, -1), inp["Ybars"][g].cpu().numpy(),
                            inp["scales"][g].cpu().numpy(), nu)
    err = out["Ybar"].reshape(-1) - ref
    assert np.all(np.abs(err) <= bound), ("Ybar from the noise", R.worst(err, bound))


@pytest.mark.parametrize("N", [63, 127])
@pytest.mark.parametrize("method,K", [("cem", 7), ("ps", 1)])
def test_reverse_once_under_the_elite_rule(N, method, K):
    c = _plan(N)
    ctx, inp, nu = c["ctx"], c["inp"], c["model"].nu
    base = _once(c["ref"], inp)
    ctx.set_update_rule("elite", K)
    try:
        out = _once(ctx, inp)
        w = ctx.weights(1).cpu().numpy()[0]
    finally:
        ctx.set_update_rule("mppi")
    assert np.array_equal(_bits(out["rews"]), _bits(base["rews"]))             # the rollouts are untouched
    assert np.array_equal(_bits(w), _bits(elite_weights_ref(out["rews"], K)))
    assert not np.array_equal(out["Ybar"], base["Ybar"])
    rows = {s: R.download(ctx, s, N + 1) for s in SEGS}
    _check_bars(out, w, rows, inp, 0, nu)
    if method == "ps":   # 1.0 x plus exact zeros: the best candidate's own rows (x + 0 turns a -0 into +0, as the sum does)
        best = int(np.flatnonzero(w)[0])
        assert w[best] == 1.0 and out["rews"][best] == out["rews"].max()
        for s, k in zip(SEGS, ("Ybar", "qbar", "qdbar", "xbar")):
            assert np.array_equal(_bits(out[k].reshape(-1)), _bits(rows[s][best] + np.float32(0))), k


def test_in_kernel_noise_gives_the_same_weights():
    N = 63
    c = _plan(N)
    ctx, inp = c["ctx"], c["inp"]
    seed, counter = 0x5EED_0000_0007, 5
    st, Yb, sc = inp["states"][1].contiguous(), inp["Ybars"][1].contiguous(), inp["scales"][1].contiguous()
    ctx.set_update_rule("elite", 7)
    try:
        a = _host(ctx.reverse_once_rng(st, Yb, sc, seed, counter))
        wa = ctx.weights(1).cpu().numpy()[0]
        b = _host(ctx.reverse_once(st, Yb, sc, ctx.rng_fill(seed, counter, 0, N)))
        wb = ctx.weights(1).cpu().numpy()[0]
    finally:
        ctx.set_update_rule("mppi")
    assert np.array_equal(_bits(wa), _bits(wb)) and np.count_nonzero(wa) == 7
    assert np.array_equal(_bits(wa), _bits(elite_weights_ref(a["rews"], 7)))
    assert np.array_equal(_bits(a["rews"]), _bits(b["rews"]))


def test_grouped_plans_rank_their_own_rewards():
    import torch
    N, K = 63, 7
    c = _plan(N)
    ctx, inp = c["ctx"], c["inp"]
    ctx.set_update_rule("elite", K)
    try:
        out = _host(ctx.reverse_once_batch(inp["states"], inp["Ybars"], inp["scales"], inp["eps"]))
        w = ctx.weights(M).cpu().numpy()
        scales0 = inp["scales"].clone()
        scales0[2] = 0.0                       # plan 2 without noise: every candidate is the mean trajectory, all rewards equal
        flat = _host(ctx.reverse_once_batch(inp["states"], inp["Ybars"], scales0, inp["eps"]))
        wf = ctx.weights(M).cpu().numpy()
        torch.cuda.synchronize()
    finally:
        ctx.set_update_rule("mppi")
    assert not np.any(out["rews"][1] == out["rews"][0])
    for g in range(M):
        assert np.array_equal(_bits(w[g]), _bits(elite_weights_ref(out["rews"][g], K))), g
    assert len({tuple(np.flatnonzero(w[g])) for g in range(M)}) == M
    assert np.all(flat["rews"][2] == flat["rews"][2][0])
    assert np.all(np.isfinite(wf)) and np.array_equal(np.flatnonzero(wf[2]), np.arange(K))
    assert np.array_equal(_bits(wf[2]), _bits(elite_weights_ref(flat["rews"][2], K)))
    for k in ("rews", "Ybar", "qbar", "qdbar", "xbar"):   # the other plans: untouched
        assert np.array_equal(_bits(flat[k][:2]), _bits(out[k][:2])), k
        assert np.all(np.isfinite(flat[k][2])), k
    assert np.array_equal(_bits(wf[:2]), _bits(w[:2]))


def test_ensemble_weights_rank_the_aggregated_rewards():
    import plant_models_cases as PM
    from dial_mpc_amd import _lib
    N, K = 63, 7
    c = _plan(N)
    inp = c["inp"]
    structs = [PM.variant_struct(c["model"], v) for v in PM.variants(c["env"].sys.model, "unitree_go2_trot")[:2]]
    ctx = _lib.Context(c["model"], c["task"], c["cfg"], options=dict(plan_cap=M))
    ctx.set_plan_ensemble(structs, None, "min")
    ctx.set_update_rule("elite", K)
    out = _once(ctx, inp, 1)
    w = ctx.weights(1).cpu().numpy()[0]
    raw = ctx.ensemble_rewards(1).cpu().numpy()[:, 0]
    assert np.array_equal(out["rews"], raw.min(0)) and not np.array_equal(raw[0], raw[1])
    assert np.array_equal(_bits(w), _bits(elite_weights_ref(out["rews"], K)))
    ref, bound = R.wsum_ref(w, R.download(ctx, "Y0s", N + 1))
    assert np.all(np.abs(out["Ybar"].reshape(-1) - ref) <= bound)


def test_task_plugin_context_takes_the_rule():
    from dial_mpc_amd import _lib
    from plugin_cases import F, build_matrix, load_case
    N, K = 63, 7
    c = load_case("go2", N=N, H=4)
    ctx = _lib.Context(c["model"], c["ptask"], c["cfg"], plugin=build_matrix(["go2"])["go2"], user_params=[F["qvel"], 1])
    p = _plan(N)
    inp = p["inp"]
    base = _once(ctx, inp, 1)
    ctx.set_update_rule("elite", K)
    out = _once(ctx, inp, 1)
    w = ctx.weights(1).cpu().numpy()[0]
    assert np.array_equal(_bits(out["rews"]), _bits(base["rews"]))
    assert np.array_equal(_bits(w), _bits(elite_weights_ref(out["rews"], K)))
    ref, bound = R.wsum_ref(w, R.download(ctx, "Y0s", N + 1))
    assert np.all(np.abs(out["Ybar"].reshape(-1) - ref) <= bound)


# ------------------------------------------------------------------------------------------------------------- 3. binding
def test_back_to_mppi_is_the_context_that_never_left():
    N = 63
    c = _plan(N)
    ctx, inp = c["ctx"], c["inp"]
    base = _once(c["ref"], inp, 2)
    wbase = c["ref"].weights(1).cpu().numpy()
    ctx.set_update_rule("elite", 5)
    elite = _once(ctx, inp, 2)
    ctx.set_update_rule("mppi", 99999)              # n_elite is ignored for mppi
    back = _once(ctx, inp, 2)
    wback = ctx.weights(1).cpu().numpy()
    for k in base:
        assert np.array_equal(_bits(back[k]), _bits(base[k])), k
    assert np.array_equal(_bits(wback), _bits(wbase))
    assert abs(float(wbase.sum()) - 1.0) < 1e-4 and np.count_nonzero(wbase) > 5   # dial_get_weights under mppi: the softmax weights
    assert not np.array_equal(elite["Ybar"], base["Ybar"])
    bbase = _host(c["ref"].reverse_once_batch(inp["states"], inp["Ybars"], inp["scales"], inp["eps"]))
    bback = _host(ctx.reverse_once_batch(inp["states"], inp["Ybars"], inp["scales"], inp["eps"]))
    for k in bbase:
        assert np.array_equal(_bits(bback[k]), _bits(bbase[k])), k
    assert np.array_equal(_bits(ctx.weights(M).cpu().numpy()), _bits(c["ref"].weights(M).cpu().numpy()))


def test_planner_set_update_takes_effect_on_the_next_call():
    import torch
    from dial_mpc_amd.core.dial_core import MBDPI
    from dial_mpc_amd.utils.synthetic import perturbed_state
    c = _plan(63)
    dc, env, inp = c["dc"], c["env"], c["inp"]
    assert (dc.update_method, dc.n_elite) == ("mppi", 0)
    mb = MBDPI(dc, env)
    st, Yb, sc, eps = inp["states"][0].contiguous(), inp["Ybars"][0], inp["scales"][0], inp["eps"][0].contiguous()
    _, Y1, i1 = mb.reverse_once(st, 0, Yb, sc, eps=eps)
    w1 = mb.weights().cpu().numpy()
    assert mb.set_update("cem", elite_frac=0.1) == 7 and (mb.update_method, mb.n_elite) == ("cem", 7)     # ceil(6.3)
    _, Y2, i2 = mb.reverse_once(st, 0, Yb, sc, eps=eps)
    w2 = mb.weights().cpu().numpy()
    assert mb.set_update("ps") == 1
    _, Y3, i3 = mb.reverse_once(st, 0, Yb, sc, eps=eps)
    w3 = mb.weights().cpu().numpy()
    torch.cuda.synchronize()
    rews = i1["rews"].cpu().numpy()
    assert w1.shape == (64,) and np.count_nonzero(w1) > 7
    assert np.array_equal(_bits(w2), _bits(elite_weights_ref(rews, 7))) and np.array_equal(_bits(w3), _bits(elite_weights_ref(rews, 1)))
    assert np.array_equal(_bits(i2["rews"].cpu().numpy()), _bits(rews))
    assert not np.array_equal(Y1.cpu().numpy(), Y2.cpu().numpy()) and not np.array_equal(Y2.cpu().numpy(), Y3.cpu().numpy())
    with pytest.raises(KeyError):
        mb.set_update("softmax")
    import dataclasses
    mb2 = MBDPI(dataclasses.replace(dc, update_method="cem", n_elite=5), env, n_plans=2)     # bound at construction
    assert mb2.n_elite == 5
    _, Yb2, ib = mb2.reverse_once_batch(inp["states"][:2], 0, inp["Ybars"][:2], inp["scales"][:2], eps=inp["eps"][:2].contiguous())
    wb = mb2.weights().cpu().numpy()
    assert wb.shape == (2, 64)
    for g in range(2):
        assert np.array_equal(_bits(wb[g]), _bits(elite_weights_ref(ib["rews"][g].cpu().numpy(), 5)))


def test_errors():
    import torch
    from dial_mpc_amd import _abi, _lib
    ARG = _abi.MACROS["DIAL_ERR_ARG"]
    c = _plan(63)
    ctx = _lib.Context(c["model"], c["task"], c["cfg"])
    lib, N = ctx.lib, 63

    def fails(rc, prefix, who=ctx):
        assert rc == ARG, rc
        msg = lib.dial_last_error(who.h if who is not None else None).decode()
        assert msg.startswith(prefix), msg
    out = torch.zeros((1, N + 1), dtype=torch.float32, device="cuda")
    fails(lib.dial_get_weights(ctx.h, out.data_ptr(), 1, None), "dial_get_weights: ")      # before any launch
    fails(lib.dial_set_update_rule(ctx.h, 2, 1), "dial_set_update_rule: ")
    fails(lib.dial_set_update_rule(ctx.h, -1, 1), "dial_set_update_rule: ")
    fails(lib.dial_set_update_rule(ctx.h, 1, 0), "dial_set_update_rule: ")
    fails(lib.dial_set_update_rule(ctx.h, 1, N + 2), "dial_set_update_rule: ")
    fails(lib.dial_set_update_rule(None, 1, 1), "dial_set_update_rule: ", who=None)
    assert lib.dial_set_update_rule(ctx.h, 1, N + 1) == 0 and lib.dial_set_update_rule(ctx.h, 0, 0) == 0
    nocfg = _lib.Context(c["model"], c["task"], None)
    fails(lib.dial_set_update_rule(nocfg.h, 1, 1), "dial_set_update_rule: ", who=nocfg)
    with pytest.raises(_lib.DialHipError, match="dial_set_update_rule: "):
        ctx.set_update_rule("elite", 0)
    with pytest.raises(ValueError):
        ctx.set_update_rule("cem", 3)
    _once(ctx, c["inp"])
    assert lib.dial_get_weights(ctx.h, out.data_ptr(), 1, None) == 0
    fails(lib.dial_get_weights(ctx.h, out.data_ptr(), 2, None), "dial_get_weights: ")      # another M
    fails(lib.dial_get_weights(ctx.h, None, 1, None), "dial_get_weights: ")
    # a sharded call with fewer candidates than the bound elite count
    sh, _, _ = _sharded()
    packed = torch.empty(sh.packed_size(), dtype=torch.float32, device="cuda")
    sh.set_update_rule("elite", 100)
    try:
        with pytest.raises(_lib.DialHipError, match="dial_set_update_rule: the bound elite count 100 exceeds"):
            sh.shard_reduce(_dev(np.zeros(65)), 64, 0, 0, False, packed)
        assert sh.lib.dial_shard_reduce(sh.h, _dev(np.zeros(65)).data_ptr(), 64, 0, 0, 0, packed.data_ptr(), None) == ARG
        sh.shard_reduce(_dev(np.zeros(100)), 99, 0, 0, False, packed)                      # K == n_total + 1: allowed
        assert np.count_nonzero(sh.weights(1).cpu().numpy()[0, :100]) == 100
    finally:
        sh.set_update_rule("mppi")


# ------------------------------------------------------------------------------------------------------------- 4. closed loop
@pytest.mark.parametrize("method", ["cem", "ps"])
def test_closed_loop_smoke(method):
    """Go2 trot, N = 255, H = 8, 20 ticks of dial_core's loop under the rule: clean status, finite states and plans."""
    import dataclasses

    import torch
    from dial_mpc_amd.core.dial_core import MBDPI, _generator
    key = "loop"
    if key not in _CTX:
        dc, env, model, task, cfg = setup_case("unitree_go2_trot", 255, 8)
        _CTX[key] = (dc, env)
    dc, env = _CTX[key]
    dc = dataclasses.replace(dc, update_method=method, Ndiffuse=2, Ndiffuse_init=4)
    mb = MBDPI(dc, env)
    assert mb.n_elite == (26 if method == "cem" else 1)
    rng = _generator(dc.seed, mb.device)
    state = env.reset(rng)
    Y0 = torch.zeros((dc.Hnode + 1, mb.nu), dtype=torch.float32, device=mb.device)
    for t in range(20):
        state = env.step(state, Y0[0])
        Y0 = mb.shift(Y0)
        n_diffuse = dc.Ndiffuse_init if t == 0 else dc.Ndiffuse
        factors = mb.sigma_control[None, :] * (dc.traj_diffuse_factor ** torch.arange(n_diffuse, device=mb.device))[:, None]
        for i in range(n_diffuse):
            rng, Y0, info = mb.reverse_once(state, rng, Y0, factors[i], want_bars=(i == n_diffuse - 1))
        torch.cuda.synchronize()
        mb.ctx.status()
        assert bool(torch.isfinite(state.packed).all()) and bool(torch.isfinite(Y0).all()), t
        assert bool(torch.isfinite(info["xbar"]).all()) and bool(torch.isfinite(info["rews"]).all()), t
    w = mb.weights().cpu().numpy()
    assert np.count_nonzero(w) == mb.n_elite and abs(float(w.sum()) - 1.0) < 1e-5
