"""GPU tests of robust planning over a model ensemble: the robust iterations of a context with an ensemble bound by
dial_set_plan_ensemble (csrc/plan_ens_kernel.h and plan_ens_aggregate.hip in libdialplanens.so, and the rollout kernel of a task
plugin built with plan_ensemble=True).  The gate is bit identity, and the reference is never the new kernel: a context CREATED from
variant v running the parent's kernels with the same inputs (the raw rewards and hypothesis 0's scratch rows), the NumPy fp64
statement of the aggregation (tests/ensemble_ref.py), a context with the same models bound per plan by dial_set_plan_models (the tail
where the ensemble is degenerate), and the fp64 softmax / weighted sums with the bounds of tests/planner_ref.py (the tail on mixed
hypotheses).
Shapes of tests/plan_models_cases.py: N = 8 samples, H = 4, M = 3 plans, its four variants, start states, Ybars, scales and eps;
R = 3 hypotheses per plan, HYP = [[0, 1, 2], [3, 0, 1], [2, 2, 3]] (plan 2 repeats one)."""
import numpy as np
import pytest

import ensemble_ref as E
import plan_models_cases as C
import planner_ref as R
from dial_mpc_amd import _abi
from plan_models_cases import M, N
from plugin_cases import F, build_matrix, case_model_dict, load_case, probe_source

pytestmark = pytest.mark.gpu

ARG, UNSUP = _abi.MACROS["DIAL_ERR_ARG"], _abi.MACROS["DIAL_ERR_UNSUPPORTED"]
INST = {"unitree_go2_trot": 1, "unitree_h1_jog": 2, "unitree_h1_loco": 3, "allegro_reorient": 4, "unitree_go2_crate_climb": 5,
        "unitree_h1_push_crate": 6}
ALL_CASES = C.EXAMPLES + ["generic", "plugin"]
# contexts whose rollout wavefronts own an overflow area in global memory (one per wavefront of the largest grid the context was
# created for): the ensemble launch's R x M x (N + 1) wavefronts need plan_cap = M R there; everywhere else plan_cap = M is enough
OVERFLOW_CASES = ("generic", "unitree_go2_crate_climb", "unitree_h1_push_crate")
PROBE_PARAMS = [F["qvel"], 1]   # the probe reward of the plugin cases: the base's lateral velocity
BARS = ("rews", "Ybar", "qbar", "qdbar", "xbar")
SEGS = ("Y0s", "qss", "qdss", "xss")
NR = 3
HYP = [[0, 1, 2], [3, 0, 1], [2, 2, 3]]
PER_PLAN = [2, 0, 3]
RNG_KEY = (0x5EED_0000_0002, 3)
MODES = [("mean", 1.0), ("min", 1.0), ("cvar", 0.5), ("cvar", 0.1), ("cvar", 1.0)]   # cvar: k = 2, 1, R


def _dev(x, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda:0")


_made, _refs, _ref_out = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    _made.clear()
    _refs.clear()
    _ref_out.clear()


def _ens_plugin(**kw):
    from dial_mpc_amd.plugin import build_plugin
    return build_plugin(case_model_dict("go2"), probe_source(), plan_ensemble=True, **kw)


def _make(case):
    """A case, one per module run: dict(env, model, task, cfg, kw, ctx, structs, inst, inputs).  An example's name (its own
    instantiation; plan_cap = M, or M R for OVERFLOW_CASES), "generic" (the Go2 on the capacity-dimension kernel with plan_cap = M R;
    "generic-small": plan_cap = M), "plugin" (the Go2 probe plugin with the ensemble AND the per-model rollout kernel)
    and "plugin-plain" (the default probe plugin, which has neither)."""
    from dial_mpc_amd import _lib
    if case in _made:
        return _made[case]
    opts = dict(plan_cap=M)
    if case.startswith("plugin"):
        c = load_case("go2", N=N, H=C.H)
        env, md, example, dc = c["env"], c["md"], "unitree_go2_trot", c["dc"]
        model, task, cfg = c["model"], c["ptask"], c["cfg"]
        path = build_matrix(["go2"])["go2"] if case == "plugin-plain" else _ens_plugin(plan_models=True)
        kw = dict(plugin=path, user_params=PROBE_PARAMS, options=opts)
        inst = 7
    else:
        example = "unitree_go2_trot" if case.startswith("generic") else case
        dc, env, model, task, cfg, md = C.load(example)
        if case in OVERFLOW_CASES:   # (the crate scenes' own instantiations run capped workspaces with overflow areas too)
            opts["plan_cap"] = M * NR
        if case.startswith("generic"):
            opts["force_generic"] = 1
            opts["con_cap"] = 2   # four feet on the ground: every standing step runs on the wavefront's overflow area (tests/test_gpu_capacity_kernel.py)
        kw = dict(options=opts)
        inst = 0 if case.startswith("generic") else INST[example]
    ctx = _lib.Context(model, task, cfg, device=0, **kw)
    assert ctx.debug_last_launch()["inst"] == inst
    Hn1 = dc.Hnode + 1
    rng = np.random.default_rng(11)
    qpos, qvel = C.start(model, env)
    inputs = dict(states=ctx.env_reset_batch(_dev(qpos), _dev(qvel)),
                  Ybars=_dev(0.3 * rng.uniform(-1, 1, (M, Hn1, model.nu))),
                  scales=_dev(np.stack([np.full(Hn1, 0.2 + 0.1 * g) for g in range(M)])),
                  eps=_dev(rng.standard_normal((M, N, Hn1, model.nu))),
                  us=_dev(C.controls(model)))
    _made[case] = dict(env=env, model=model, task=task, cfg=cfg, kw=kw, ctx=ctx, structs=C.structs(model, md, example), inst=inst, inputs=inputs)
    return _made[case]


def _ref(case, v):
    """The reference of variant v: a context CREATED from that model, on which only the parent's kernels ever run."""
    from dial_mpc_amd import _lib
    if (case, v) not in _refs:
        c = _make(case)
        ctx = _lib.Context(c["structs"][v], c["task"], c["cfg"], device=0, **c["kw"])
        assert ctx.debug_last_launch()["inst"] == c["inst"]
        _refs[(case, v)] = ctx
    return _refs[(case, v)]


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items() if v is not None}


def _batch(ctx, i, rng_key=None, want_bars=True):
    if rng_key is not None:
        return _host(ctx.reverse_once_batch_rng(i["states"], i["Ybars"], i["scales"], *rng_key, want_bars=want_bars))
    return _host(ctx.reverse_once_batch(i["states"], i["Ybars"], i["scales"], i["eps"], want_bars=want_bars))


def _once(ctx, i):
    return _host(ctx.reverse_once(i["states"][0].contiguous(), i["Ybars"][0].contiguous(), i["scales"][0].contiguous(), i["eps"][0].contiguous()))


def _ref_batch(case, v, rng_key=None):
    """The grouped call on the reference context of variant v (computed once, shared, left unchanged) and its scratch rows."""
    key = (case, v, rng_key)
    if key not in _ref_out:
        ctx = _ref(case, v)
        out = _batch(ctx, _make(case)["inputs"], rng_key)
        out["scratch"] = {s: R.download(ctx, s, M * (N + 1)).reshape(M, N + 1, -1) for s in SEGS + ("rewss",)}
        _ref_out[key] = out
    return _ref_out[key]


def _raw(ctx, m=M):
    import torch
    raw = ctx.ensemble_rewards(m)
    torch.cuda.synchronize()
    return raw.cpu().numpy().copy()


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()   # (bit for bit, NaNs and signed zeros included)


@pytest.mark.parametrize("case", ALL_CASES)
def test_1_raw_rewards_are_each_models_rewards(case):
    """After a bound reverse_once_batch, ensemble_rewards(M)[r, g] equals, bit for bit, row g of rews of the same grouped call on the
    context created from variant HYP[g][r]; the same with in-kernel noise.  The three slabs are not all equal."""
    import torch
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        assert ctx.set_plan_ensemble(c["structs"], HYP).tolist() == HYP
        for rng_key in (None, RNG_KEY):
            _batch(ctx, i, rng_key)
            ll = ctx.debug_last_launch()
            assert (ll["inst"], ll["wpb"], ll["blocks"], ll["queue"], ll["relay"], ll["pair"]) == (c["inst"], 1, NR * M * (N + 1), 0, 0, 0)
            dev = ctx.ensemble_rewards(M)
            assert tuple(dev.shape) == (NR, M, N + 1)
            assert not (torch.equal(dev[0], dev[1]) and torch.equal(dev[1], dev[2])), "all slabs equal: the test would be vacuous"
            raw = _raw(ctx)
            assert np.isfinite(raw).all()
            for g in range(M):
                for r in range(NR):
                    assert _bits(raw[r, g], _ref_batch(case, HYP[g][r], rng_key)["rews"][g]), (case, rng_key, g, r)
            assert _bits(raw[0, 2], raw[1, 2]) and not _bits(raw[0, 0], raw[1, 0])   # plan 2 repeats a hypothesis, plan 0 does not
    finally:
        ctx.set_plan_ensemble(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_2_aggregate_is_the_stated_one(case):
    """mean, min, cvar with k = 2, k = 1 and k = R: the returned rews equals tests/ensemble_ref.py of the downloaded raw rewards bit for
    bit; cvar with k = 1 equals min bit for bit."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    got = {}
    try:
        for mode, alpha in MODES:
            ctx.set_plan_ensemble(c["structs"], HYP, mode, alpha)
            out = _batch(ctx, i, want_bars=False)
            raw = _raw(ctx)
            want = E.aggregate(raw, mode, alpha)
            assert _bits(out["rews"], want), (case, mode, alpha, np.abs(out["rews"] - want).max())
            got[(mode, alpha)] = out["rews"]
        assert [E.cvar_k(a, NR) for _, a in MODES[2:]] == [2, 1, NR]
        assert _bits(got[("cvar", 0.1)], got[("min", 1.0)])
        assert not _bits(got[("mean", 1.0)], got[("min", 1.0)]) and not _bits(got[("cvar", 0.5)], got[("min", 1.0)])
    finally:
        ctx.set_plan_ensemble(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_3_tail_exact_where_the_ensemble_is_degenerate(case):
    """R = 1 with hyp [[2], [0], [3]], and R = 3 with the same hypothesis three times per plan: in every aggregate mode rews, Ybar,
    qbar, qdbar and xbar equal the outputs of dial_set_plan_models per plan with [2, 0, 3] bit for bit (the fp64 sum of equal fp32
    values and its division by their number are exact); also for the lean call and for the one-plan reverse_once (row 0)."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        ctx.set_plan_models(c["structs"], PER_PLAN)
        want = dict(full=_batch(ctx, i), lean=_batch(ctx, i, want_bars=False), once=_once(ctx, i))
        ctx.set_plan_models(None)
        assert sorted(want["lean"]) == ["Ybar", "rews"] and all(np.isfinite(want["full"][k]).all() for k in BARS)
        for hyp in ([[v] for v in PER_PLAN], [[v] * 3 for v in PER_PLAN]):
            for mode, alpha in MODES[:3]:
                ctx.set_plan_ensemble(c["structs"], hyp, mode, alpha)
                got = dict(full=_batch(ctx, i), lean=_batch(ctx, i, want_bars=False), once=_once(ctx, i))
                assert ctx.debug_last_launch()["blocks"] == len(hyp[0]) * (N + 1)   # (the one-plan call: row 0's hypotheses)
                for call in want:
                    assert sorted(got[call]) == sorted(want[call])
                    for k in want[call]:
                        assert _bits(got[call][k], want[call][k]), (case, len(hyp[0]), mode, call, k)
    finally:
        ctx.set_plan_models(None)
        ctx.set_plan_ensemble(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_4_tail_on_mixed_hypotheses(case):
    """HYP with mean: the device's weights are the fp64 softmax of the aggregated rews, and Ybar, qbar, qdbar, xbar the fp64 weighted
    sums of hypothesis 0's rows in the scratch, within the bounds tests/test_gpu_planner_kernels.py applies to the same kernels; those
    rows equal the rows of the context created from variant HYP[g][0] bit for bit."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        ctx.set_plan_ensemble(c["structs"], HYP, "mean")
        out = _batch(ctx, i)
        rows = M * (N + 1)
        w = R.download(ctx, "weights", rows).reshape(M, N + 1)
        X = {s: R.download(ctx, s, rows).reshape(M, N + 1, -1) for s in SEGS + ("rewss",)}
        assert _bits(out["rews"], E.aggregate(_raw(ctx), "mean"))
        temp = c["cfg"].temp_sample
        worst = 0.0
        for g in range(M):
            ref_w, bound_w = R.softmax_ref(out["rews"][g], temp)[0], R.softmax_bound(out["rews"][g], temp)
            assert np.all(np.abs(w[g] - ref_w) <= bound_w), (case, g, R.worst(w[g] - ref_w, bound_w))
            for s, k in zip(SEGS, ("Ybar", "qbar", "qdbar", "xbar")):
                ref, bound = R.wsum_ref(w[g], X[s][g])
                err = out[k][g].reshape(-1) - ref
                assert R.isclose_to_bound(out[k][g].reshape(-1), ref, bound), (case, g, k, R.worst(err, bound))
                worst = max(worst, R.worst(err, bound))
            nominal = _ref_batch(case, HYP[g][0])["scratch"]
            for s in X:
                assert _bits(X[s][g], nominal[s][g]), (case, g, s)
        print(f"\n{case}: robust tail: worst {worst:.3g} of the bound")
    finally:
        ctx.set_plan_ensemble(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_5_other_entry_points_unbind_rebind_timing(case):
    """While bound, dial_rollout and env_step equal the unbound context's bit for bit.  After unbinding, reverse_once_batch equals the
    never-bound outputs and debug_last_launch reports the usual path.  Rebinding with other indices takes effect.  dial_set_timing
    records one launch per robust iteration."""
    import torch
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]

    def others():
        ro = [x.cpu().numpy().copy() for x in ctx.rollout(i["states"][1].contiguous(), i["us"])]
        act = i["us"][:M, 0].contiguous()
        st = [x.cpu().numpy().copy() for x in ctx.env_step_batch(i["states"], act)]
        one = [x.cpu().numpy().copy() for x in ctx.env_step(i["states"][1].contiguous(), act[1].contiguous())]
        torch.cuda.synchronize()
        return ro + st + one
    try:
        plain = _batch(ctx, i)
        ll_plain = ctx.debug_last_launch()
        plain_others = others()
        ctx.set_plan_ensemble(c["structs"], HYP, "min")
        first = _batch(ctx, i)
        raw_first = _raw(ctx)
        assert not _bits(first["rews"], plain["rews"])
        for a, b in zip(others(), plain_others):
            assert _bits(a, b), (case, "rollout / env_step while bound")
        assert _bits(_raw(ctx), raw_first)   # ... and they left the binding's raw rewards alone
        # rebinding with other indices takes effect
        other = [[1, 0], [1, 3], [0, 0]]
        assert ctx.set_plan_ensemble(c["structs"], other, "min").tolist() == other
        with pytest.raises(Exception, match="no robust iteration has run since"):
            ctx.ensemble_rewards(M)
        again = _batch(ctx, i)
        raw = _raw(ctx)
        assert raw.shape == (2, M, N + 1) and not _bits(again["rews"], first["rews"])
        for g in range(M):
            for r in range(2):
                assert _bits(raw[r, g], _ref_batch(case, other[g][r])["rews"][g]), (case, g, r)
        # timing: one launch per robust iteration
        ctx.set_timing(True)
        _batch(ctx, i)
        ms, launches = ctx.rollout_ms()
        assert launches == 1 and ms > 0
        ctx.set_timing(False)
        ctx.set_plan_ensemble(None)
        back = _batch(ctx, i)
        assert ctx.debug_last_launch() == ll_plain
        for k in BARS:
            assert _bits(back[k], plain[k]), (case, "unbound", k)
        ctx.set_plan_ensemble(None)   # (unbinding twice is fine)
    finally:
        ctx.set_timing(False)
        ctx.set_plan_ensemble(None)


def test_6_plugin_plan_params_apply_per_plan():
    """Per-plan task parameters bound together with an ensemble: plan g's rollouts under every hypothesis read row g.  set_user_params
    and set_user_table are refused while the ensemble is bound."""
    case = "plugin"
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    sel = np.array([[F["qpos"], 2], [F["qvel"], 0], [F["xpos"], 5]], np.float32)
    try:
        ctx.set_plan_ensemble(c["structs"], HYP)
        shared = _batch(ctx, i)
        ctx.set_plan_params(sel)
        _batch(ctx, i)
        raw = _raw(ctx)
        for v in sorted({v for row in HYP for v in row}):
            ref_ctx = _ref(case, v)
            try:
                ref_ctx.set_plan_params(sel)
                ref = _batch(ref_ctx, i)
            finally:
                ref_ctx.set_plan_params(None)
            for g in range(M):
                for r in range(NR):
                    if HYP[g][r] == v:
                        assert _bits(raw[r, g], ref["rews"][g]), (g, r)
        pv = np.asarray(PROBE_PARAMS, np.float32)
        assert ctx.lib.dial_set_user_params(ctx.h, pv.ctypes.data, len(pv)) == ARG
        err = ctx.lib.dial_last_error(ctx.h).decode()
        assert err.startswith("dial_set_user_params: a plan ensemble is bound") and "unbind first" in err
        tab = _dev(np.zeros((4, 2)))
        assert ctx.lib.dial_set_user_table(ctx.h, tab.data_ptr(), 4, 2, 0, 0) == ARG
        assert "dial_set_user_table: a plan ensemble is bound" in ctx.lib.dial_last_error(ctx.h).decode()
        ctx.set_plan_params(None)
        for k in BARS:
            assert _bits(_batch(ctx, i)[k], shared[k]), k
        ctx.set_plan_ensemble(None)
        assert ctx.lib.dial_set_user_params(ctx.h, pv.ctypes.data, len(pv)) == 0   # unbound: accepted again
    finally:
        ctx.set_plan_params(None)
        ctx.set_plan_ensemble(None)


def test_7_refusals(tmp_path):
    import shutil
    from dial_mpc_amd import _lib
    case = "unitree_go2_trot"
    c = _make(case)
    ctx, structs, lib, h, i = c["ctx"], c["structs"], c["ctx"].lib, c["ctx"].h, c["inputs"]
    copy = lambda m: type(m).from_buffer_copy(m)   # noqa: E731
    arr = (_abi.DialModel * 4)(*structs)
    hyp = np.array(HYP, np.int32)
    P = hyp.ctypes.data
    plain = _batch(ctx, i)
    # ---- DIAL_ERR_ARG at bind time, each with its message
    for args, msg in [((arr, 0, P, M, NR, 0, 1.0), "V = 0 is outside 1 .. DIAL_MAX_PLAN_MODELS"),
                      ((arr, 1025, P, M, NR, 0, 1.0), "V = 1025 is outside 1 .. DIAL_MAX_PLAN_MODELS"),
                      ((arr, 4, P, M, 0, 0, 1.0), "R = 0 is outside 1 .. DIAL_MAX_ENSEMBLE"),
                      ((arr, 4, P, M, 33, 0, 1.0), "R = 33 is outside 1 .. DIAL_MAX_ENSEMBLE"),
                      ((arr, 4, P, 0, NR, 0, 1.0), "rows = 0 is outside 1 .. the context's plan capacity 3"),
                      ((arr, 4, P, M + 1, 2, 0, 1.0), "rows = 4 is outside 1 .. the context's plan capacity 3"),
                      ((None, 4, P, M, NR, 0, 1.0), "a null pointer with V = 4, rows = 3, R = 3"),
                      ((arr, 4, None, M, NR, 0, 1.0), "a null pointer with V = 4, rows = 3, R = 3"),
                      ((arr, 4, P, M, NR, 3, 1.0), "unknown aggregate 3"),
                      ((arr, 4, P, M, NR, -1, 1.0), "unknown aggregate -1"),
                      ((arr, 4, P, M, NR, 2, 0.0), "is outside (0, 1]"),
                      ((arr, 4, P, M, NR, 2, 1.5), "is outside (0, 1]"),
                      ((arr, 4, P, M, NR, 2, -0.5), "is outside (0, 1]"),
                      ((arr, 4, P, M, NR, 2, float("nan")), "is outside (0, 1]"),
                      ((arr, 3, P, M, NR, 0, 1.0), "hyp[1][0] = 3 is outside 0 .. V - 1 = 2")]:
        assert lib.dial_set_plan_ensemble(h, *args) == ARG, msg
        err = lib.dial_last_error(h).decode()
        assert err.startswith("dial_set_plan_ensemble: ") and msg in err, err
    neg = np.array([[0, 1, 2], [0, 0, -1], [0, 0, 0]], np.int32)
    assert lib.dial_set_plan_ensemble(h, arr, 4, neg.ctypes.data, M, NR, 0, 1.0) == ARG and "hyp[1][2] = -1" in lib.dial_last_error(h).decode()
    assert lib.dial_set_plan_ensemble(None, arr, 4, P, M, NR, 0, 1.0) == ARG
    assert lib.dial_set_plan_ensemble(h, arr, 4, P, M, NR, 1, 7.0) == 0   # (alpha is read by cvar alone)
    ctx.set_plan_ensemble(None)
    out = _dev(np.zeros((NR, M, N + 1)))
    assert lib.dial_get_ensemble_rewards(h, out.data_ptr(), M, None) == ARG and "no plan ensemble is bound" in lib.dial_last_error(h).decode()

    def refused(models, index, match, code=ARG, cx=ctx, **kw):
        with pytest.raises(_lib.DialHipError, match=match) as e:
            cx.set_plan_ensemble(models, index, **kw)
        assert f"({code})" in str(e.value) and "dial_set_plan_ensemble: " in str(e.value)
    # rejected models: dial_set_plan_models's rule
    m = copy(structs[0])
    m.nu = 11
    refused([structs[0], m], [[0, 1]], r"model 1 is rejected: nu = 11, the context's model has 12")
    m2 = copy(structs[2])
    m2.timestep = 0.004
    refused([structs[0], structs[1], m2], [[0, 1, 2]], r"model 2 is rejected: its timestep 0.004\d* differs from the context's 0.02")
    # a sharded context, and one without a dial_cfg
    sctx = _lib.Context(c["model"], c["task"], c["cfg"], device=0, n_local_cap=N // 2)
    refused(structs, [[0]], "the context is sharded", ARG, sctx)
    nctx = _lib.Context(c["model"], c["task"], None, device=0)
    assert nctx.lib.dial_set_plan_ensemble(nctx.h, arr, 4, P, 1, NR, 0, 1.0) == ARG and "without a dial_cfg" in nctx.lib.dial_last_error(nctx.h).decode()
    for k in BARS:   # none of the refused calls bound anything
        assert _bits(_batch(ctx, i)[k], plain[k]), k
    try:
        # ---- mutual exclusion with dial_set_plan_models, in both orders
        ctx.set_plan_models(structs, PER_PLAN)
        refused(structs, HYP, "plan models are bound")
        ctx.set_plan_models(None)
        ctx.set_plan_ensemble(structs, HYP)
        with pytest.raises(_lib.DialHipError, match="dial_set_plan_models: a plan ensemble is bound") as e:
            ctx.set_plan_models(structs, PER_PLAN)
        assert f"({ARG})" in str(e.value)
        # ---- a refused bind leaves the previous binding working
        first = _batch(ctx, i)
        raw_first = _raw(ctx)
        assert not _bits(first["rews"], plain["rews"])
        refused([structs[0], m], [[0, 1]], "model 1 is rejected")
        assert lib.dial_set_plan_ensemble(h, arr, 4, P, M, NR, 9, 1.0) == ARG
        again = _batch(ctx, i)
        for k in BARS:
            assert _bits(again[k], first[k]), ("a refused bind keeps the previous binding", k)
        assert _bits(_raw(ctx), raw_first)
        # ---- at launch time
        assert lib.dial_get_ensemble_rewards(h, out.data_ptr(), M - 1, None) == ARG
        assert "M = 2, the last ensemble launch had 3 plans" in lib.dial_last_error(h).decode()
        ctx.set_plan_ensemble(structs, HYP[:2])
        with pytest.raises(_lib.DialHipError, match="M = 3 plans, but the bound plan ensemble has hypotheses for 2 plans") as e:
            _batch(ctx, i)
        assert f"({ARG})" in str(e.value) and ctx.debug_last_launch()["blocks"] == 0
        assert lib.dial_get_ensemble_rewards(h, out.data_ptr(), M, None) == ARG   # (no launch since this binding)
        # a state trace is bound: no TRACE instantiation of the new kernel; a refused launch records no time
        ctx.set_plan_ensemble(structs, HYP)
        ctx.set_timing(True)
        ctx.set_state_trace(M * (N + 1))
        with pytest.raises(_lib.DialHipError, match="state trace") as e:
            _batch(ctx, i)
        assert f"({UNSUP})" in str(e.value) and "rollout launch: " in str(e.value)
        assert ctx.rollout_ms()[1] == 0
    finally:
        ctx.set_timing(False)
        ctx.set_state_trace(None)
        ctx.set_plan_models(None)
        ctx.set_plan_ensemble(None)
    # ---- the capacity-dimension kernel with plan_cap = M: R x M x (N + 1) wavefronts exceed its overflow areas
    g = _make("generic-small")
    try:
        g["ctx"].set_plan_ensemble(g["structs"], HYP)
        with pytest.raises(_lib.DialHipError, match=r"rollout launch: .*overflow areas.*plan_cap >= M x R = 9 provides them") as e:
            _batch(g["ctx"], g["inputs"])
        assert f"({ARG})" in str(e.value) and g["ctx"].debug_last_launch()["blocks"] == 0
        g["ctx"].set_plan_ensemble(g["structs"], [[v] for v in PER_PLAN])   # R = 1 fits
        assert np.isfinite(_batch(g["ctx"], g["inputs"])["rews"]).all()
    finally:
        g["ctx"].set_plan_ensemble(None)
    # ---- DIAL_ERR_UNSUPPORTED
    p = _make("plugin-plain")   # a plugin without the table: binding is refused, its rollouts still run
    refused(p["structs"], HYP, "dial_plugin_plan_ens_v1", UNSUP, p["ctx"])
    assert np.isfinite(_batch(p["ctx"], p["inputs"])["rews"]).all()
    ictx = _lib.Context(c["model"], c["task"], c["cfg"], device=0, lib_path=_lib.IEEE_LIB_PATH, **c["kw"])
    refused(structs, HYP, "IEEE measurement build", UNSUP, ictx)
    lone = tmp_path / "libdialhip.so"
    shutil.copy(_lib.LIB_PATH, lone)
    lctx = _lib.Context(c["model"], c["task"], c["cfg"], device=0, lib_path=str(lone), **c["kw"])
    refused(structs, HYP, "libdialplanens.so", UNSUP, lctx)
    for k in BARS:
        assert _bits(_batch(lctx, i)[k], plain[k]), ("its unbound launches are what they were", k)


def test_mbdpi_ensemble_round_trip():
    """MBDPI(ensemble=dict(...)) on the Go2 env: the default hypotheses, the aggregated rewards of a robust iteration, set_ensemble(None)
    gives the nominal planner back, and every dict gets the env's timestep."""
    import torch
    from dial_mpc_amd.core.dial_core import MBDPI
    from dial_mpc_amd.mjcf import vary_model
    dc, env, model, task, cfg, md = C.load("unitree_go2_trot")
    heavy, slick = vary_model(md, mass_scale={"base": 1.4}), dict(vary_model(md, friction_scale=0.5), timestep=0.001)
    nominal = MBDPI(dc, env, n_plans=M)
    i = _make("unitree_go2_trot")["inputs"]
    states = i["states"]
    want = nominal.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    mb = MBDPI(dc, env, n_plans=M, ensemble=dict(models=[md, heavy, slick], aggregate="min"))
    assert mb.hyp.tolist() == [[0, 1, 2]] * M
    got = mb.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    raw = _raw(mb.ctx)
    assert np.isfinite(got).all() and _bits(raw[0], want) and _bits(got, E.aggregate(raw, "min")) and not _bits(got, want)
    assert mb.set_ensemble([md, heavy], hyp=[1, 0], aggregate="cvar", alpha=0.5).tolist() == [[1, 0]] * M
    got = mb.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    raw = _raw(mb.ctx)
    assert _bits(raw[1], want) and _bits(got, E.aggregate(raw, "cvar", 0.5))
    assert mb.set_ensemble(None) is None and mb.hyp is None
    got = mb.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    assert _bits(got, want)
    with pytest.raises(ValueError, match="ensemble is dict"):
        MBDPI(dc, env, n_plans=M, ensemble=dict(variants=[md]))
    torch.cuda.synchronize()
