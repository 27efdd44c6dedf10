"""GPU tests of planner model ensembles: the rollout launches of a context with models bound by dial_set_plan_models
(csrc/plan_var_kernel.h in libdialplanvar.so, and in a task plugin built with plan_models=True).  The gate is bit identity, and the
reference is never the new kernel: a context CREATED from variant v (dial_create builds its constants) running the parent's kernels
with the same inputs.
N = 8 samples, H = 4, M = 3 plans (plan_cap 3), V = 4 variants (tests/plant_models_cases.py's), per-plan index [2, 0, 3], per-sample
index [0, 1, 2, 3, 3, 2, 1, 0, 1]; the noise is passed as data.  That every non-identity variant changes a reward from these start
states and controls is checked on the CPU with the fp32 oracle (tests/test_plan_models_host.py) and asserted here on the device by the
first test."""
import numpy as np
import pytest

import plan_models_cases as C
import planner_ref as R
from dial_mpc_amd import _abi
from plan_models_cases import M, N, PER_PLAN, PER_SAMPLE
from plugin_cases import F, build_matrix, load_case

pytestmark = pytest.mark.gpu

ARG, UNSUP = _abi.MACROS["DIAL_ERR_ARG"], _abi.MACROS["DIAL_ERR_UNSUPPORTED"]
INST = {"unitree_go2_trot": 1, "unitree_h1_jog": 2, "unitree_h1_loco": 3, "allegro_reorient": 4, "unitree_go2_crate_climb": 5,
        "unitree_h1_push_crate": 6}
ALL_CASES = C.EXAMPLES + ["generic", "plugin"]
PROBE_PARAMS = [F["qvel"], 1]   # the probe reward of the plugin cases: the base's lateral velocity
BARS = ("rews", "Ybar", "qbar", "qdbar", "xbar")


def _dev(x, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda:0")


_made, _refs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_contexts():
    yield
    _made.clear()
    _refs.clear()


def _make(case):
    """A case, one per module run: dict(env, model, task, cfg, kw, ctx, structs, inst, inputs).  An example's name (its own
    instantiation), "generic" (the Go2 on the capacity-dimension kernel), "plugin" (the Go2 probe plugin with the per-model rollout
    kernel) and "plugin-plain" (the default probe plugin, which has none)."""
    from dial_mpc_amd import _lib
    if case in _made:
        return _made[case]
    opts = dict(plan_cap=M)
    if case.startswith("plugin"):
        c = load_case("go2", N=N, H=C.H)
        env, md, example, dc = c["env"], c["md"], "unitree_go2_trot", c["dc"]
        model, task, cfg = c["model"], c["ptask"], c["cfg"]
        path = build_matrix(["go2"])["go2"] if case == "plugin-plain" else C.build_plan_plugin("go2")
        kw = dict(plugin=path, user_params=PROBE_PARAMS, options=opts)
        inst = 7
    else:
        example = "unitree_go2_trot" if case == "generic" else case
        dc, env, model, task, cfg, md = C.load(example)
        if case == "generic":
            opts["force_generic"] = 1
        kw = dict(options=opts)
        inst = 0 if case == "generic" else INST[example]
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


def _batch(ctx, i, rng_key=None):
    if rng_key is not None:
        return _host(ctx.reverse_once_batch_rng(i["states"], i["Ybars"], i["scales"], *rng_key))
    return _host(ctx.reverse_once_batch(i["states"], i["Ybars"], i["scales"], i["eps"]))


def _rollout(ctx, i, B=N + 1):
    return [x.cpu().numpy().copy() for x in ctx.rollout(i["states"][1].contiguous(), i["us"][:B].contiguous())]


def _once(ctx, i):
    return _host(ctx.reverse_once(i["states"][1].contiguous(), i["Ybars"][1].contiguous(), i["scales"][1].contiguous(), i["eps"][1].contiguous()))


def _bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()   # (bit for bit, NaNs and signed zeros included)


@pytest.mark.parametrize("case", ALL_CASES)
def test_1_variants_matter(case):
    """dial_rollout with the same controls on the four reference contexts: every non-identity variant differs from variant 0 in the
    step rewards of at least one rollout.  Otherwise the rest of the file is vacuous."""
    c = _make(case)
    rewss = [_rollout(_ref(case, v), c["inputs"])[0] for v in range(4)]
    assert all(np.isfinite(r).all() for r in rewss)
    for v in (1, 2, 3):
        assert (rewss[v] != rewss[0]).any(axis=1).any(), (case, v)


@pytest.mark.parametrize("case", ALL_CASES)
def test_2_per_plan_each_plan_is_its_models_plan(case):
    """reverse_once_batch with models bound per plan: plan g's rews, Ybar, qbar, qdbar and xbar equal, bit for bit, plan g of the same
    grouped call on the reference context of variant model_of[g]; the same with in-kernel noise."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        assert ctx.set_plan_models(c["structs"], PER_PLAN).tolist() == PER_PLAN
        for rng_key in (None, (0x5EED_0000_0002, 3)):
            got = _batch(ctx, i, rng_key)
            ll = ctx.debug_last_launch()
            assert (ll["inst"], ll["wpb"], ll["blocks"], ll["queue"], ll["relay"], ll["pair"]) == (c["inst"], 1, M * (N + 1), 0, 0, 0)
            assert all(np.isfinite(got[k]).all() for k in BARS)
            for g in range(M):
                ref = _batch(_ref(case, PER_PLAN[g]), i, rng_key)
                for k in BARS:
                    assert _bits(got[k][g], ref[k][g]), (case, rng_key, g, k)
    finally:
        ctx.set_plan_models(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_3_per_sample_given_controls(case):
    """dial_rollout with B = 9 and models bound per sample: row n of rewss, qss, qdss and xposs equals row n of the same call on the
    reference context of variant model_of[n]."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        ctx.set_plan_models(c["structs"], PER_SAMPLE, per="sample")
        got = _rollout(ctx, i)
        refs = {v: _rollout(_ref(case, v), i) for v in sorted(set(PER_SAMPLE))}
        for n in range(N + 1):
            for k, name in enumerate(("rewss", "qss", "qdss", "xposs")):
                assert _bits(got[k][n], refs[PER_SAMPLE[n]][k][n]), (case, n, name)
    finally:
        ctx.set_plan_models(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_4_per_sample_planning(case):
    """reverse_once with models bound per sample: rews[n] equals rews[n] of the reference context of variant model_of[n] for every n,
    the mean trajectory included; the device's weights are the fp64 softmax of its own rews and Ybar the fp64 weighted sum of its own
    candidate nodes, within the bounds tests/test_gpu_planner_kernels.py uses (planner_ref.softmax_bound / wsum_ref)."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        ctx.set_plan_models(c["structs"], PER_SAMPLE, per="sample")
        got = _once(ctx, i)
        w = R.download(ctx, "weights", N + 1).reshape(-1)
        nodes = R.download(ctx, "Y0s", N + 1)
        refs = {v: _once(_ref(case, v), i) for v in sorted(set(PER_SAMPLE))}
        for n in range(N + 1):
            assert _bits(got["rews"][n], refs[PER_SAMPLE[n]]["rews"][n]), (case, n)
        assert len({refs[v]["rews"].tobytes() for v in refs}) == 4
        temp = c["cfg"].temp_sample
        ref_w, bound_w = R.softmax_ref(got["rews"], temp)[0], R.softmax_bound(got["rews"], temp)
        print(f"\n{case}: weights worst {R.worst(w - ref_w, bound_w):.3g} of the bound")
        assert np.all(np.abs(w - ref_w) <= bound_w), (case, R.worst(w - ref_w, bound_w))
        ref_y, bound_y = R.wsum_ref(w, nodes)
        err = got["Ybar"].reshape(-1) - ref_y
        print(f"{case}: Ybar worst {R.worst(err, bound_y):.3g} of the bound")
        assert np.all(np.abs(err) <= bound_y), (case, R.worst(err, bound_y))
    finally:
        ctx.set_plan_models(None)


@pytest.mark.parametrize("case", ALL_CASES)
def test_5_identity_and_unbind(case):
    """V = 1 with the context's own model bound per plan: the grouped, the one-plan and the given-controls launches equal the unbound
    launches of the same context bit for bit.  After set_plan_models(None) they equal them again and debug_last_launch reports the
    parent's path."""
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    try:
        plain = _batch(ctx, i)
        ll_plain = ctx.debug_last_launch()
        plain_one, plain_us = _once(ctx, i), _rollout(ctx, i)
        ctx.set_plan_models([c["model"]], [0] * M)
        bound = _batch(ctx, i)
        assert ctx.debug_last_launch()["wpb"] == 1 and ctx.debug_last_launch()["blocks"] == M * (N + 1)
        for k in BARS:
            assert _bits(bound[k], plain[k]), (case, k)
        one = _once(ctx, i)
        assert ctx.debug_last_launch()["blocks"] == N + 1 and ctx.debug_last_launch()["relay"] == 0
        for k in BARS:
            assert _bits(one[k], plain_one[k]), (case, "one plan", k)
        for a, b in zip(_rollout(ctx, i), plain_us):
            assert _bits(a, b), (case, "given controls")
        ctx.set_plan_models(None)
        again = _batch(ctx, i)
        assert ctx.debug_last_launch() == ll_plain
        for k in BARS:
            assert _bits(again[k], plain[k]), (case, "unbound", k)
        ctx.set_plan_models(None)   # (unbinding twice is fine)
    finally:
        ctx.set_plan_models(None)


def test_6_plugin_plan_params_and_plan_models_together():
    """Per-plan parameter rows bound together with per-plan models: plan g's reward reads row g AND its rollouts run model model_of[g]
    -- it equals the reference context of that variant with the same rows bound.  set_user_params is refused while models are bound,
    set_plan_params keeps working."""
    from dial_mpc_amd import _lib
    case = "plugin"
    c = _make(case)
    ctx, i = c["ctx"], c["inputs"]
    sel = np.array([[F["qpos"], 2], [F["qvel"], 0], [F["xpos"], 5]], np.float32)
    try:
        ctx.set_plan_models(c["structs"], PER_PLAN)
        shared = _batch(ctx, i)
        ctx.set_plan_params(sel)
        got = _batch(ctx, i)
        assert not _bits(got["rews"], shared["rews"])
        for g in range(M):
            ref_ctx = _ref(case, PER_PLAN[g])
            try:
                ref_ctx.set_plan_params(sel)
                ref = _batch(ref_ctx, i)
            finally:
                ref_ctx.set_plan_params(None)
            for k in BARS:
                assert _bits(got[k][g], ref[k][g]), (g, k)
        pv = np.asarray(PROBE_PARAMS, np.float32)
        assert ctx.lib.dial_set_user_params(ctx.h, pv.ctypes.data, len(pv)) == ARG
        err = ctx.lib.dial_last_error(ctx.h).decode()
        assert err.startswith("dial_set_user_params: plan models are bound") and "unbind first" in err
        tab = _dev(np.zeros((4, 2)))
        assert ctx.lib.dial_set_user_table(ctx.h, tab.data_ptr(), 4, 2, 0, 0) == ARG
        assert "dial_set_user_table: plan models are bound" in ctx.lib.dial_last_error(ctx.h).decode()
        ctx.set_plan_params(None)
        for k in BARS:
            assert _bits(_batch(ctx, i)[k], shared[k]), k
        ctx.set_plan_models(None)
        assert ctx.lib.dial_set_user_params(ctx.h, pv.ctypes.data, len(pv)) == 0   # unbound: accepted again
    finally:
        ctx.set_plan_params(None)
        ctx.set_plan_models(None)


def test_7_refusals(tmp_path):
    import shutil
    from dial_mpc_amd import _lib
    case = "unitree_go2_trot"
    c = _make(case)
    ctx, structs, lib, h, i = c["ctx"], c["structs"], c["ctx"].lib, c["ctx"].h, c["inputs"]
    copy = lambda m: type(m).from_buffer_copy(m)   # noqa: E731
    arr = (_abi.DialModel * 4)(*structs)
    plan = np.array(PER_PLAN, np.int32)
    samp = np.array(PER_SAMPLE, np.int32)
    P, S = plan.ctypes.data, samp.ctypes.data
    plain = _batch(ctx, i)
    # ---- DIAL_ERR_ARG at bind time, each with its message
    for args, msg in [((arr, 0, P, M, 0), "V = 0 is outside 1 .. DIAL_MAX_PLAN_MODELS"),
                      ((arr, 1025, P, M, 0), "V = 1025 is outside 1 .. DIAL_MAX_PLAN_MODELS"),
                      ((arr, 4, P, 0, 0), "rows = 0 must be >= 1"),
                      ((arr, 4, P, -1, 0), "rows = -1 must be >= 1"),
                      ((None, 4, P, M, 0), "a null pointer with V = 4, rows = 3"),
                      ((arr, 4, None, M, 0), "a null pointer with V = 4, rows = 3"),
                      ((arr, 4, P, M, 2), "unknown mode 2"),
                      ((arr, 4, P, M, -1), "unknown mode -1"),
                      ((arr, 4, S, M + 1, 0), "rows = 4 exceeds the context's plan capacity 3"),
                      ((arr, 4, S, N, 1), "rows = 8, DIAL_PLAN_MODELS_PER_SAMPLE needs Nsample + 1 = 9"),
                      ((arr, 4, S, N + 2, 1), "rows = 10, DIAL_PLAN_MODELS_PER_SAMPLE needs Nsample + 1 = 9"),
                      ((arr, 3, P, M, 0), "model_of[2] = 3 is outside 0 .. V - 1 = 2"),
                      ((arr, 3, S, N + 1, 1), "model_of[3] = 3 is outside 0 .. V - 1 = 2")]:
        assert lib.dial_set_plan_models(h, *args) == ARG, msg
        err = lib.dial_last_error(h).decode()
        assert err.startswith("dial_set_plan_models: ") and msg in err, err
    neg = np.array([0, -1, 0], np.int32)
    assert lib.dial_set_plan_models(h, arr, 4, neg.ctypes.data, M, 0) == ARG and "model_of[1] = -1" in lib.dial_last_error(h).decode()
    assert lib.dial_set_plan_models(None, arr, 4, P, M, 0) == ARG

    def refused(models, index, match, code=ARG, cx=ctx, per="plan"):
        with pytest.raises(_lib.DialHipError, match=match) as e:
            cx.set_plan_models(models, index, per)
        assert f"({code})" in str(e.value) and "dial_set_plan_models: " in str(e.value)
    # rejected models: dial_set_plant_models's rule, and the timestep must be the context's own
    m = copy(structs[0])
    m.nu = 11
    refused([structs[0], m], [0, 1, 0], r"model 1 is rejected: nu = 11, the context's model has 12")
    m = copy(structs[0])
    m.dof_parentid[9] = 6
    refused([m], [0], r"model 0 is rejected: .*(topology|would pick kernel instantiation 0 for it, the context runs instantiation 1)")
    m = copy(structs[2])
    m.timestep = 0.004
    refused([structs[0], structs[1], m], [0, 1, 2], r"model 2 is rejected: its timestep 0.004\d* differs from the context's 0.02")
    # a sharded context, and one without a dial_cfg
    sctx = _lib.Context(c["model"], c["task"], c["cfg"], device=0, n_local_cap=N // 2)
    refused(structs, [0], "the context is sharded", ARG, sctx)
    nctx = _lib.Context(c["model"], c["task"], None, device=0)
    assert nctx.lib.dial_set_plan_models(nctx.h, arr, 4, P, 1, 0) == ARG and "without a dial_cfg" in nctx.lib.dial_last_error(nctx.h).decode()
    for k in BARS:   # none of the refused calls bound anything
        assert _bits(_batch(ctx, i)[k], plain[k]), k
    # ---- at launch time; a refused bind leaves the previous binding working
    try:
        ctx.set_plan_models(structs, PER_PLAN[:2])
        with pytest.raises(_lib.DialHipError, match="M = 3 plans, but the bound plan models index 2 plans") as e:
            _batch(ctx, i)
        assert f"({ARG})" in str(e.value) and ctx.debug_last_launch()["blocks"] == 0
        ctx.set_plan_models(structs, PER_PLAN)
        first = _batch(ctx, i)
        assert not _bits(first["rews"], plain["rews"])
        refused([structs[0], m], [0, 1, 0], "model 1 is rejected")
        assert lib.dial_set_plan_models(h, arr, 4, P, M, 7) == ARG
        again = _batch(ctx, i)
        for k in BARS:
            assert _bits(again[k], first[k]), ("a refused bind keeps the previous binding", k)
        # timing keeps working while bound, and a refused launch records nothing
        ctx.set_timing(True)
        _batch(ctx, i)
        ms, launches = ctx.rollout_ms()
        assert launches == 1 and ms > 0
        # a state trace is bound: no TRACE instantiation of the new kernel
        ctx.set_state_trace(M * (N + 1))
        with pytest.raises(_lib.DialHipError, match="state trace") as e:
            _batch(ctx, i)
        assert f"({UNSUP})" in str(e.value)
        assert ctx.rollout_ms()[1] == 0
        ctx.set_timing(False)
        ctx.set_state_trace(None)
        ctx.set_plan_models(structs, PER_SAMPLE, per="sample")
        us = _dev(np.zeros((N + 2, C.H + 1, ctx.nu)))
        with pytest.raises(_lib.DialHipError, match="B = 10 rollouts, but the bound plan models index 9 samples") as e:
            ctx.rollout(i["states"][1].contiguous(), us)
        assert f"({ARG})" in str(e.value)
        assert np.isfinite(_rollout(ctx, i, B=4)[0]).all()   # fewer rollouts than rows: fine
    finally:
        ctx.set_timing(False)
        ctx.set_state_trace(None)
        ctx.set_plan_models(None)
    # ---- DIAL_ERR_UNSUPPORTED
    p = _make("plugin-plain")   # a plugin without the table: binding is refused, its rollouts still run
    refused(p["structs"], PER_PLAN, "dial_plugin_plan_var_v1", UNSUP, p["ctx"])
    assert np.isfinite(_batch(p["ctx"], p["inputs"])["rews"]).all()
    ictx = _lib.Context(c["model"], c["task"], c["cfg"], device=0, lib_path=_lib.IEEE_LIB_PATH, **c["kw"])
    refused(structs, PER_PLAN, "IEEE measurement build", UNSUP, ictx)
    lone = tmp_path / "libdialhip.so"
    shutil.copy(_lib.LIB_PATH, lone)
    lctx = _lib.Context(c["model"], c["task"], c["cfg"], device=0, lib_path=str(lone), **c["kw"])
    refused(structs, PER_PLAN, "libdialplanvar.so", UNSUP, lctx)
    for k in BARS:
        assert _bits(_batch(lctx, i)[k], plain[k]), ("its unbound launches are what they were", k)


def test_mbdpi_models_round_trip():
    """MBDPI(models=, model_of=, model_per=) on the Go2 env: the default indices, per plan and per sample, set_models(None) gives the
    nominal planner back, and every dict gets the env's timestep."""
    import torch
    from dial_mpc_amd.core.dial_core import MBDPI
    from dial_mpc_amd.mjcf import vary_model
    dc, env, model, task, cfg, md = C.load("unitree_go2_trot")
    heavy, slick = vary_model(md, mass_scale={"base": 1.4}), dict(vary_model(md, friction_scale=0.5), timestep=0.001)
    nominal = MBDPI(dc, env, n_plans=M)
    i = _make("unitree_go2_trot")["inputs"]
    states = i["states"]
    want = nominal.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    mb = MBDPI(dc, env, n_plans=M, models=[md, heavy, slick])
    assert mb.model_of.tolist() == [0, 1, 2]
    got = mb.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    assert np.isfinite(got).all() and _bits(got[0], want[0]) and not _bits(got[1], want[1]) and not _bits(got[2], want[2])
    assert mb.set_models([md, heavy], per="sample").tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    rews = mb.reverse_once(states[1], 0, i["Ybars"][1], i["scales"][1], eps=i["eps"][1])[2]["rews"]
    ref = nominal.reverse_once(states[1], 0, i["Ybars"][1], i["scales"][1], eps=i["eps"][1])[2]["rews"]
    same = (rews == ref).cpu().numpy()
    assert same[0::2].all() and not same[1::2].any()
    assert mb.set_models(None) is None and mb.model_of is None
    got = mb.reverse_once_batch(states, 0, i["Ybars"], i["scales"], eps=i["eps"])[2]["rews"].cpu().numpy()
    assert _bits(got, want)
    torch.cuda.synchronize()
