"""The kernels that turn rollouts into a plan -- in-kernel noise (philox.h, rng_fill_kernel), the K4a softmax (weights_kernel), the
K4b weighted sums (wsum_*_kernel), the mean action regenerated from the noise (ybar_*_kernel) and the K5 shift (shift_kernel) --
against plain fp64 NumPy restatements (tests/philox_ref.py, tests/planner_ref.py), on synthetic inputs chosen for the shapes and edges
where such kernels go wrong: every shipped model's row widths (the H1's C = 114 ends in a partial Philox quad), sizes on both sides of
the reductions' chunk and block boundaries, hard reward profiles, rows of mixed sign and scale.  Every gate is an error bound derived
from the kernel's own summation order (planner_ref.py); the worst error of each test, as a fraction of its bound, is printed."""
import numpy as np
import pytest

import philox_ref as P
import planner_ref as R
from conftest import setup_case

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
# Box-Muller's error on the device, in units of planner_ref.ulp_sensitivity (approximate fp32 log / sqrt / sin / cos against fp64).
# Measured on an MI355X over the draws of test_rng_fill_matches_the_philox_restatement: worst 0.673 (Go2, H1 and Allegro alike).
PHILOX_K = 2.0
WRONG_WORD = 1e-3     # any draw further than this from the restatement is a different number, not a rounding

# (example, Hsample) per shipped model; contexts are created with Nsample = N_GLOBAL and scratch rows for N_LOCAL local samples
MODELS = {"go2": ("unitree_go2_trot", 16), "h1": ("unitree_h1_jog", 16), "allegro": ("allegro_reorient", 8),
          "crate": ("unitree_go2_crate_climb", 25)}
N_GLOBAL, N_LOCAL = 65536, 4096
_CTX = {}


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _ctx(key, temp=1.0):
    """One dial_create_sharded context per (model, temperature): W_cap = 65537 weights, B_cap = 4097 rows of scratch."""
    from dial_mpc_amd import _lib
    if (key, temp) not in _CTX:
        example, H = MODELS[key]
        dc, env, model, task, cfg = setup_case(example, N_GLOBAL, H)
        cfg.temp_sample = temp
        _CTX[(key, temp)] = (_lib.Context(model, task, cfg, n_local_cap=N_LOCAL), dc, model)
    return _CTX[(key, temp)]


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    _CTX.clear()


def _weights(ctx, n):
    return R.download(ctx, "weights", n).reshape(-1)


# ------------------------------------------------------------------------------------------------------------- 1. Philox + Box-Muller
def _check_draws(got, seed, counter, n_begin, n_count, C):
    z, r, t, L = P.normals(seed, counter, n_begin, n_count, C)
    err = np.abs(got.astype(np.float64) - z)
    assert err.max() < WRONG_WORD, ("a draw is a different number", float(err.max()), np.unravel_index(err.argmax(), err.shape))
    one = r == 0                                     # u1 == 1 exactly: z == 0 on both sides
    assert np.all(got[one] == 0)
    s = R.ulp_sensitivity(r, t, L, z)
    ratio = np.where(one, 0.0, err / np.where(one, 1.0, s))
    assert ratio.max() <= PHILOX_K, (float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return float(ratio.max())


@pytest.mark.parametrize("key", ["go2", "h1", "allegro"])
def test_rng_fill_matches_the_philox_restatement(key):
    ctx, dc, model = _ctx(key)
    C = (dc.Hnode + 1) * model.nu
    cases = [(0x1234_5678_9ABC, 0, 0, 8192),                        # counter 0
             (0xFFFF_FFFF_0000_0001, 0xFFFFFFFF, 1_000_003, 4096),  # seed with high word set, counter 0xFFFFFFFF
             (0x9E37_79B9_7F4A_7C15, 7, INT_MAX - 2048, 2048),     # n_begin up to INT_MAX - n_count
             (5, 3, INT_MAX - 1, 1)]
    worst = 0.0
    for seed, counter, n_begin, n_count in cases:
        got = ctx.rng_fill(seed, counter, n_begin, n_count).cpu().numpy().reshape(n_count, C)
        worst = max(worst, _check_draws(got, seed, counter, n_begin, n_count, C))
    # (seed, iteration 5, sample 5359985, quad 0): word 0 is 0xffffff73, u1 rounds to exactly 1 and the first pair is exactly 0
    got = ctx.rng_fill(0x9E37_79B9_7F4A_7C15, 5, 5359985, 1).cpu().numpy().reshape(-1)
    assert got[0] == 0 and got[1] == 0 and got[2] != 0
    _check_draws(got.reshape(1, C), 0x9E37_79B9_7F4A_7C15, 5, 5359985, 1, C)
    print(f"\n{key}: rng_fill vs Philox restatement: worst {worst:.3g} of PHILOX_K = {PHILOX_K} sensitivity units")


# ------------------------------------------------------------------------------------------------------------- 2. K4a softmax
def _profile(name, B, rng):
    r = rng.standard_normal(B)
    if name == "uniform":
        r = rng.uniform(-3.0, 1.0, B)
    elif name == "offset":                   # cancellation in the fp32 mean and std
        r = -1e3 + rng.uniform(-1e-2, 1e-2, B)
    elif name == "outliers":                 # at temp 0.05 all but the outliers' weights underflow
        r[B // 3] = 8.0
        r[0] = 6.5
    elif name == "mean_max":
        r[-1] = r.max() + 0.5
    elif name == "mean_min":
        r[-1] = r.min() - 0.5
    elif name == "ties":
        r = rng.integers(0, 4, B).astype(np.float64)
        r[0], r[-1] = 3.0, 0.0
    return r.astype(np.float32)


PROFILES = ["uniform", "offset", "outliers", "mean_max", "mean_min", "ties"]


@pytest.mark.parametrize("profile", PROFILES)
def test_softmax_matches_fp64(profile):
    """weights_kernel on synthetic rewards (driven through dial_shard_reduce with an empty shard) against dial_core.py:121-128 in fp64
    on the same fp32 rewards, at sizes around its 1024-thread block and up to 65537."""
    import torch
    ctx, dc, model = _ctx("go2", temp=0.05)
    packed = torch.empty(ctx.packed_size(), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(PROFILES.index(profile))
    worst = 0.0
    for B in (2, 64, 65, 1023, 1024, 1025, 2049, 4097, 65537):
        r = _profile(profile, B, rng)
        ctx.shard_reduce(_dev(r), B - 1, 0, 0, False, packed)
        w = _weights(ctx, B)
        ref, _, _ = R.softmax_ref(r, 0.05)
        bound = R.softmax_bound(r, 0.05)
        assert np.all(np.isfinite(w)) and np.all(w >= 0), (profile, B)
        assert np.all(np.abs(w - ref) <= bound), (profile, B, R.worst(w - ref, bound))
        top = r == r.max()
        assert np.all(w[top] == w.max()) and r[np.argmax(w)] == r.max(), (profile, B)
        worst = max(worst, R.worst(w - ref, bound))
    print(f"\nsoftmax {profile}: worst {worst:.3g} of the bound")


# ------------------------------------------------------------------------------------------------------------- 3. K4b weighted sums
SEGS = ("Y0s", "qss", "qdss", "xss")


def _rows(rng, n, C):
    """Rows of mixed sign and scale: N(0, 1) times 10^[-3, 3) per row and 10^[-1, 1) per column."""
    return (rng.standard_normal((n, C)) * 10.0 ** rng.uniform(-3, 3, (n, 1)) * 10.0 ** rng.uniform(-1, 1, (1, C))).astype(np.float32)


@pytest.mark.parametrize("key", ["go2", "h1", "allegro", "crate"])
def test_weighted_sums_match_fp64(key):
    """dial_shard_reduce on rows uploaded into the scratch: every shard size around the 64 row chunks (n_local = 63 / 127 / 4096 put
    rows into chunk 63, 64 / 2048 leave it empty), the mean row in and out, a shard that starts inside the global sample range."""
    import torch
    ctx, dc, model = _ctx(key)
    rng = np.random.default_rng(7)
    n_total, n_begin = N_GLOBAL, 12347
    rews = rng.standard_normal(n_total + 1).astype(np.float32)
    widths = [R.row_width(ctx, s) for s in SEGS]
    packed = torch.empty(ctx.packed_size(), dtype=torch.float32, device="cuda")
    worst = 0.0
    for n_local in (0, 1, 63, 64, 65, 127, 2048, 4096):
        X = {s: _rows(rng, n_local + 1, C) for s, C in zip(SEGS, widths)}
        for s in SEGS:
            R.upload(ctx, s, X[s], N_LOCAL + 1)
        for include_mean in (False, True):
            ctx.shard_reduce(_dev(rews), n_total, n_begin, n_local, include_mean, packed)
            w = _weights(ctx, n_total + 1)
            wr = np.concatenate([w[n_begin:n_begin + n_local], [w[n_total] if include_mean else 0.0]])
            out, o = packed.cpu().numpy().astype(np.float64), 0
            for s, C in zip(SEGS, widths):
                ref, bound = R.wsum_ref(wr, X[s])
                err = out[o:o + C] - ref
                assert np.all(np.abs(err) <= bound), (key, n_local, include_mean, s, R.worst(err, bound))
                worst = max(worst, R.worst(err, bound))
                o += C
    print(f"\n{key}: K4b weighted sums: worst {worst:.3g} of the bound")


def test_grouped_weighted_sums_use_each_plans_rows():
    """dial_reverse_once_batch, M = 3: plan g's bars are the fp64 sum over plan g's own rows and weights (blockIdx.z / w_stride)."""
    from dial_mpc_amd import _lib
    from dial_mpc_amd.utils.synthetic import perturbed_state
    N, H, M = 64, 8, 3
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, H)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=M))
    qs, qds = zip(*[perturbed_state(env, g) for g in range(M)])
    states = ctx.env_reset_batch(_dev(np.stack(qs)), _dev(np.stack(qds)))
    rng = np.random.default_rng(3)
    Hn1 = dc.Hnode + 1
    Ybars = _dev(0.3 * rng.uniform(-1, 1, (M, Hn1, model.nu)))
    scales = _dev(np.stack([np.full(Hn1, 0.2 + 0.1 * g) for g in range(M)]))
    eps = _dev(rng.standard_normal((M, N, Hn1, model.nu)))
    out = ctx.reverse_once_batch(states, Ybars, scales, eps)
    rows = M * (N + 1)
    w = _weights(ctx, rows).reshape(M, N + 1)
    X = {s: R.download(ctx, s, rows).reshape(M, N + 1, -1) for s in SEGS}
    rews = out["rews"].cpu().numpy()
    worst = 0.0
    for g in range(M):
        ref_w, bound_w = R.softmax_ref(rews[g], cfg.temp_sample)[0], R.softmax_bound(rews[g], cfg.temp_sample)
        assert np.all(np.abs(w[g] - ref_w) <= bound_w), g
        for s, k in zip(SEGS, ("Ybar", "qbar", "qdbar", "xbar")):
            ref, bound = R.wsum_ref(w[g], X[s][g])
            err = out[k][g].cpu().numpy().reshape(-1) - ref
            assert np.all(np.abs(err) <= bound), (g, k, R.worst(err, bound))
            worst = max(worst, R.worst(err, bound))
    assert not np.array_equal(X["Y0s"][0], X["Y0s"][1])
    print(f"\ngrouped K4b: worst {worst:.3g} of the bound")


# ------------------------------------------------------------------------------------------------------------- 4. mean action
def _gathered(rews, n_total, world):
    per = -(-n_total // world)
    g = np.zeros((world, per + 1), np.float32)
    for k in range(world):
        part = rews[k * per:min((k + 1) * per, n_total)]
        g[k, :part.size] = part
        g[k, per] = rews[n_total] if k == 0 else np.float32(123.0)   # only rank 0's copy of the mean reward is read
    return g.reshape(-1), per


@pytest.mark.parametrize("key", ["go2", "h1", "allegro"])
def test_mean_action_matches_fp64(key):
    """dial_shard_ybar / _rng / _gathered[_rng]: Ybar_out[c] = sum_n w_n clip(k == 0 ? Ybar[a] : eps sigma_k + Ybar[c]) with the mean row
    clip(Ybar), at sample counts around the 128 row chunks, per-node (non-constant) and scalar noise scales, Ybar partly outside
    [-1, 1]; the in-kernel noise against the Philox restatement, and bit for bit against dial_shard_ybar fed with dial_rng_fill."""
    import torch
    ctx, dc, model = _ctx(key)
    nu, Hn1 = model.nu, dc.Hnode + 1
    C = Hn1 * nu
    rng = np.random.default_rng(11)
    Ybar = rng.uniform(-1.4, 1.4, (Hn1, nu)).astype(np.float32)
    f32 = dict(dtype=torch.float32, device="cuda")
    worst = dict(eps=0.0, rng=0.0)
    seed, counter = 0xABCD_0000_1234, 9
    for n_total in (1, 5, 127, 128, 129, 2048, 65536):
        rews = rng.standard_normal(n_total + 1).astype(np.float32)
        eps = rng.standard_normal((n_total, C)).astype(np.float32)
        z, r, t, L = P.normals(seed, counter, 0, n_total, C)
        z_err = PHILOX_K * R.ulp_sensitivity(r, t, L, z)
        z_err[r == 0] = 0.0
        for sigma in ((0.25 * 0.8 ** np.arange(Hn1)[::-1]).astype(np.float32), np.array([0.4], np.float32)):
            out = torch.empty((Hn1, nu), **f32)
            ctx.shard_ybar(_dev(rews), n_total, _dev(eps), _dev(Ybar), _dev(sigma), out)
            w = _weights(ctx, n_total + 1)
            ref, bound = R.ybar_ref(w, eps, Ybar, sigma, nu)
            err = out.cpu().numpy().reshape(-1) - ref
            assert np.all(np.abs(err) <= bound), (key, n_total, sigma.size, "eps", R.worst(err, bound))
            worst["eps"] = max(worst["eps"], R.worst(err, bound))
            world = min(3, n_total)
            gath, per = _gathered(rews, n_total, world)
            out_g, rews_g = torch.empty((Hn1, nu), **f32), torch.empty(n_total + 1, **f32)
            ctx.shard_ybar_gathered(_dev(gath), world, per, n_total, _dev(eps), _dev(Ybar), _dev(sigma), rews_g, out_g)
            assert torch.equal(out_g, out) and np.array_equal(rews_g.cpu().numpy(), rews)
            # in-kernel noise
            out_r = torch.empty((Hn1, nu), **f32)
            ctx.shard_ybar_rng(_dev(rews), n_total, seed, counter, _dev(Ybar), _dev(sigma), out_r)
            ref, bound = R.ybar_ref(w, z, Ybar, sigma, nu, eps_err=z_err)
            err = out_r.cpu().numpy().reshape(-1) - ref
            assert np.all(np.abs(err) <= bound), (key, n_total, sigma.size, "rng", R.worst(err, bound))
            worst["rng"] = max(worst["rng"], R.worst(err, bound))
            fill = ctx.rng_fill(seed, counter, 0, n_total)
            out_f = torch.empty((Hn1, nu), **f32)
            ctx.shard_ybar(_dev(rews), n_total, fill, _dev(Ybar), _dev(sigma), out_f)
            assert torch.equal(out_r, out_f), (key, n_total, sigma.size)
            ctx.shard_ybar_gathered_rng(_dev(gath), world, per, n_total, seed, counter, _dev(Ybar), _dev(sigma), rews_g, out_g)
            assert torch.equal(out_g, out_r)
    print(f"\n{key}: mean action: worst {worst['eps']:.3g} (eps), {worst['rng']:.3g} (in-kernel noise) of the bound")


class _OneRank:
    """torch.distributed stand-in for world 1: the collectives are copies."""
    ReduceOp = type("ReduceOp", (), {"SUM": "sum"})

    @staticmethod
    def all_gather_into_tensor(out, inp):
        out.copy_(inp)

    @staticmethod
    def all_reduce(t, op=None):
        return t


@pytest.mark.parametrize("example,N,H", [("unitree_h1_jog", 256, 16), ("allegro_reorient", 128, 8)])
def test_lean_sharded_mean_action_matches_fused(example, N, H):
    """The lean sharded iteration (rollouts without nodes / states, the mean action regenerated by ybar_*_kernel) against the fused
    reverse_once (nodes summed by K4b) on the H1 (partial quad) and the Allegro: same rewards bit for bit, Ybar within the two
    kernels' summation bounds."""
    import torch
    from dial_mpc_amd import _lib
    from dial_mpc_amd.core.sharding import sharded_reverse_once
    dc, env, model, task, cfg = setup_case(example, N, H)
    ctx = _lib.Context(model, task, cfg)
    s0, _, _ = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(model.nv)))
    Hn1, T = dc.Hnode + 1, H + 1
    rng = np.random.default_rng(21)
    Ybar = _dev(rng.uniform(-1.2, 1.2, (Hn1, model.nu)))
    sigma = _dev(0.3 * 0.85 ** np.arange(Hn1)[::-1])
    eps = _dev(rng.standard_normal((N, Hn1, model.nu)))
    worst = 0.0
    for rng_key in (None, (0x5EED_0000_0001, 4)):
        e = None if rng_key else eps
        Yb, rews, _, _, _ = sharded_reverse_once(ctx, _OneRank, 0, 1, N, T, Hn1, s0, Ybar, sigma, e, want_bars=False, rng=rng_key)
        Yb, rews = Yb.clone(), rews.clone()
        full = ctx.reverse_once_rng(s0, Ybar, sigma, *rng_key) if rng_key else ctx.reverse_once(s0, Ybar, sigma, eps)
        assert torch.equal(rews, full["rews"])
        w = _weights(ctx, N + 1)
        nodes = R.download(ctx, "Y0s", N + 1)
        ref, b_wsum = R.wsum_ref(w, nodes)
        eps_n = (ctx.rng_fill(*rng_key, 0, N) if rng_key else eps).cpu().numpy().reshape(N, -1)
        _, b_ybar = R.ybar_ref(w, eps_n, Ybar.cpu().numpy(), sigma.cpu().numpy(), model.nu)
        err = Yb.cpu().numpy().reshape(-1) - full["Ybar"].cpu().numpy().reshape(-1)
        assert np.all(np.abs(err) <= b_wsum + b_ybar), (example, rng_key, R.worst(err, b_wsum + b_ybar))
        worst = max(worst, R.worst(err, b_wsum + b_ybar))
    print(f"\n{example}: lean sharded vs fused mean action: worst {worst:.3g} of the bound")


# ------------------------------------------------------------------------------------------------------------- 5. shift
SHIFT_SHAPES = sorted({(16, 4), (20, 5), (25, 5), (20, 4), (24, 6),     # the example YAMLs' (Hsample, Hnode)
                       (16, 2), (35, 2),                                # the smallest Hnode a quadratic spline allows
                       (27, 9), (35, 5), (35, 9)})                      # Hnode + 1 = DIAL_MAX_NODE, Hsample + 1 = DIAL_MAX_T


@pytest.mark.parametrize("key", ["go2", "h1", "allegro"])
def test_shift_matches_fp64(key):
    """shift_kernel / dial_shift_batch (M = 3 distinct plans) against dial_core.py:160-166 in fp64 with the cfg's fp32 matrices, at every
    example's horizon and the capacity edges; Hnode = 1 has no quadratic spline and is refused at creation."""
    import torch
    from dial_mpc_amd import _lib
    example, _ = MODELS[key]
    rng = np.random.default_rng(5)
    worst = 0.0
    for Hs, Hn in SHIFT_SHAPES:
        dc, env, model, task, cfg = setup_case(example, 8, Hs, Hnode=Hn)
        ctx = _lib.Context(model, task, cfg)
        W, V = R.cfg_matrices(cfg)
        Y = rng.uniform(-1.5, 1.5, (3, Hn + 1, model.nu)).astype(np.float32)
        Y[1] *= 1e-3
        got = ctx.shift_batch(_dev(Y)).cpu().numpy()
        for g in range(3):
            ref, bound = R.shift_ref(W, V, Y[g])
            assert np.all(np.abs(got[g] - ref) <= bound), (key, Hs, Hn, g, R.worst(got[g] - ref, bound))
            worst = max(worst, R.worst(got[g] - ref, bound))
        assert torch.equal(ctx.shift(_dev(Y[2])).cpu(), torch.as_tensor(got[2]))
        del ctx
    dc, env, model, task, cfg = setup_case(example, 8, 16, Hnode=2)
    cfg.Hnode = 1
    with pytest.raises(_lib.DialHipError, match="out of range"):
        _lib.Context(model, task, cfg)
    print(f"\n{key}: shift: worst {worst:.3g} of the bound")


# ------------------------------------------------------------------------------------------------------------- reduce after a lean launch
def test_reduce_after_a_lean_launch_is_refused():
    """dial_shard_reduce* sum the rows the last rollout launch wrote: after a lean launch (DIAL_SHARD_LEAN, reverse_once[_batch] without
    bars) they refuse with DIAL_ERR_ARG until a full launch has written them; with_mean outside 0 .. 3 is refused."""
    import torch
    from dial_mpc_amd import _lib
    N, H = 64, 8
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", N, H)
    ctx = _lib.Context(model, task, cfg, options=dict(plan_cap=2))
    s0, _, _ = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(model.nv)))
    Hn1 = dc.Hnode + 1
    rng = np.random.default_rng(1)
    Ybar, sigma = _dev(0.2 * rng.uniform(-1, 1, (Hn1, model.nu))), _dev(np.full(Hn1, 0.3))
    eps = _dev(rng.standard_normal((N, Hn1, model.nu)))
    rews_local = torch.empty(N + 1, dtype=torch.float32, device="cuda")
    rews_all = _dev(rng.standard_normal(N + 1))
    packed = torch.empty(ctx.packed_size(), dtype=torch.float32, device="cuda")
    gathered = rews_all.clone()

    def reduce_ok():
        ctx.shard_reduce(rews_all, N, 0, N, True, packed)
        ctx.shard_reduce_gathered(gathered, 1, N, N, 0, N, True, torch.empty_like(rews_all), packed)

    def refused(what=""):
        for call in (lambda: ctx.shard_reduce(rews_all, N, 0, N, True, packed),
                     lambda: ctx.shard_reduce_gathered(gathered, 1, N, N, 0, N, True, torch.empty_like(rews_all), packed)):
            with pytest.raises(_lib.DialHipError, match=r"\(-1\).*stale.*" + what):
                call()

    reduce_ok()                                                            # a fresh context: rows uploaded by a caller are summed
    ctx.shard_rollout(s0, Ybar, sigma, eps, N, 3, rews_local)              # lean shard rollout
    refused("DIAL_SHARD_LEAN")
    ctx.shard_rollout_rng(s0, Ybar, sigma, 7, 1, 0, N, 1, rews_local)      # a full one writes the rows again
    reduce_ok()
    ctx.shard_rollout_rng(s0, Ybar, sigma, 7, 1, 0, N, 3, rews_local)
    refused("DIAL_SHARD_LEAN")
    ctx.reverse_once(s0, Ybar, sigma, eps)
    reduce_ok()
    ctx.reverse_once(s0, Ybar, sigma, eps, want_bars=False)
    refused("mean action only")
    ctx.shard_rollout(s0, Ybar, sigma, eps, N, 1, rews_local)
    reduce_ok()
    states = torch.stack([s0, s0]).contiguous()
    Y2, sg2, eps2 = torch.stack([Ybar, Ybar]).contiguous(), torch.stack([sigma, sigma]).contiguous(), torch.stack([eps, eps]).contiguous()
    ctx.reverse_once_batch(states, Y2, sg2, eps2, want_bars=False)
    refused("mean action only")
    ctx.reverse_once_batch(states, Y2, sg2, eps2)
    reduce_ok()
    for call in (lambda: ctx.shard_reduce(rews_all, N, 0, N, 4, packed),
                 lambda: ctx.shard_rollout(s0, Ybar, sigma, eps, N, 4, rews_local),
                 lambda: ctx.shard_rollout_rng(s0, Ybar, sigma, 7, 1, 0, N, -1, rews_local)):
        with pytest.raises(_lib.DialHipError, match=r"\(-1\).*with_mean"):
            call()
    reduce_ok()
    torch.cuda.synchronize()
    ctx.status()
