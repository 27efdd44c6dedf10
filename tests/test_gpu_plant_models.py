"""GPU tests of plant model mismatch: dial_plant_step with models bound by dial_set_plant_models (csrc/plant_var_kernel.h in
libdialplantvar.so, and in a task plugin built with plant_models=True).  The gate is bit identity everywhere, and the reference is
never the new kernel: plant b of a varied launch against the PLAIN plant kernel (with a disturbance bound: plant_dist_kernel) on a
context created from the variant model_of[b], run at M = 1 with plant b's rows.
M = 8 plants, K = 4 steps at sim_dt = 0.005, V = 4 variants, model_of = [0, 1, 2, 3, 3, 2, 1, 0]; shapes, rows, clocks and start
states are tests/plant_models_cases.py's (those of tests/test_gpu_plant_dist.py plus 0.3 m/s of lateral base velocity).  That every
non-identity variant moves its plant from these start states is checked on the CPU with the fp32 oracle
(tests/test_plant_models_host.py) and asserted here on the device before anything is compared."""
import uuid

import numpy as np
import pytest
import yaml

import plant_models_cases as C
from conftest import setup_case
from control_cases import params
from dial_mpc_amd import _abi
from plant_dist_cases import pack
from plant_models_cases import CTRL_DT, K, M, MODEL_OF, SIM_DT, T
from plant_plugin_cases import build_plant_plugin
from plugin_cases import load_case

pytestmark = pytest.mark.gpu

ARG, UNSUP = _abi.MACROS["DIAL_ERR_ARG"], _abi.MACROS["DIAL_ERR_UNSUPPORTED"]
GEN = dict(force_generic=1)   # dial_options: the capacity-dimension instantiation (DimsMax, kernel instantiation 0)
INST = {"unitree_go2_trot": 1, "unitree_h1_jog": 2, "unitree_h1_loco": 3, "allegro_reorient": 4, "unitree_go2_crate_climb": 5,
        "unitree_h1_push_crate": 6}
ALL_CASES = C.EXAMPLES + ["generic", "plugin", "plugin-law"]


def _dev(x, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype), device="cuda:0")


_made, _refs = {}, {}


def _make(case):
    """A case, one per module run: dict(env, md, model, task, kw, ctx, structs).  An example's name (its own instantiation),
    "generic" (the Go2 on the capacity-dimension kernel), "plugin" / "plugin-law" (the Go2 probe plugin with the per-plant-model AND
    the disturbed plant kernel, without / with the probe law) and "plugin-plant-only" (the plant=True sibling, which has neither).
    The model runs at sim_dt with one physics step per step, as env.make_plant builds it; structs are the V = 4 variants."""
    from dial_mpc_amd import _lib
    if case in _made:
        return _made[case]
    if case.startswith("plugin"):
        c = load_case("go2", N=8, H=4)
        env, md, example = c["env"], c["md"], "unitree_go2_trot"
        model, task = type(c["model"]).from_buffer_copy(c["model"]), type(c["ptask"]).from_buffer_copy(c["ptask"])
        law = "probe" if case == "plugin-law" else None
        path = build_plant_plugin("go2", None) if case == "plugin-plant-only" else C.build_var_plugin("go2", law, disturbance=True)
        kw = dict(plugin=path, user_params=params(0) if law else [])
        inst = 7
    else:
        example = "unitree_go2_trot" if case == "generic" else case
        _, env, model, task, _ = setup_case(example, 8, 4, per_rollout=True)
        md = env.sys.model
        kw = dict(options=GEN if case == "generic" else None)
        inst = 0 if case == "generic" else INST[example]
    model.timestep = SIM_DT
    task.n_frames, task.dt = 1, SIM_DT
    ctx = _lib.Context(model, task, None, device=0, **kw)
    assert ctx.debug_last_launch()["inst"] == inst
    structs = [C.variant_struct(model, v) for v in C.variants(md, example)]
    _made[case] = dict(env=env, md=md, model=model, task=task, kw=kw, ctx=ctx, structs=structs, inst=inst)
    return _made[case]


def _ref(case, v):
    """The reference of variant v: a context CREATED from that model (the parent's path: dial_create builds and uploads its constants),
    on which only the parent's plant kernels ever run."""
    from dial_mpc_amd import _lib
    if (case, v) not in _refs:
        c = _make(case)
        ctx = _lib.Context(c["structs"][v], c["task"], None, device=0, **c["kw"])
        assert ctx.debug_last_launch()["inst"] == c["inst"]
        _refs[(case, v)] = ctx
    return _refs[(case, v)]


def _start(c, seed):
    qpos, qvel = C.start_qpos_qvel(c["model"], c["env"], seed)
    return c["ctx"].env_reset_batch(_dev(qpos), _dev(qvel))


def _run(ctx, s0, t, plan_time, rows, flags, sel=slice(None)):
    """One launch of K steps from copies of (s0, t) -> (states, clocks, trace), device tensors."""
    st, tt = s0[sel].clone(), _dev(t[sel], np.float64)
    trace = _dev(np.zeros((st.shape[0], K, 1 + ctx.nq + ctx.nv + ctx.nu)))
    ctx.plant_step(st, tt, _dev(plan_time[sel]), rows[sel].contiguous(), CTRL_DT, SIM_DT, K, flags, trace)
    return st, tt, trace


def _modes(case, c):
    from dial_mpc_amd import _lib
    if case == "plugin-law":
        return [("LAW", _lib.PLANT_LAW)]
    return [("CTRL", _lib.PLANT_CTRL)] + ([] if C.positional(c["model"]) else [("PD", _lib.PLANT_PD)])


def _mode_rows(c, mode, seed):
    if mode == "LAW":
        return np.random.default_rng(seed).uniform(-0.8, 0.8, (M, T, c["model"].nu)).astype(np.float32)
    return C.rows(c["model"], c["env"], mode == "PD" or C.positional(c["model"]), seed)


def _same(a, b, sel, why):
    import torch
    for what, x, y in zip(("states", "clocks", "trace"), a, b):
        assert torch.equal(x[sel], y), (why, what)


@pytest.mark.parametrize("case", ALL_CASES)
def test_each_plant_is_its_models_plant(case):
    """Every instantiation, every control mode the case has: states, clocks and traces of plant b of ONE varied launch equal those of
    the plain plant kernel on the context created from model model_of[b], at M = 1 with plant b's rows.  First: every non-identity
    variant's plants differ from the identity context's plants in at least one state word (the Allegro's third variant is not the
    friction scale, which its start states do not feel: plant_models_cases.variant_args)."""
    import torch
    c = _make(case)
    ctx = c["ctx"]
    s0 = _start(c, seed=3)
    t, plan_time = C.clocks()
    try:
        for mode, flags in _modes(case, c):
            rows = _dev(_mode_rows(c, mode, seed=4))
            ctx.set_plant_models(c["structs"], MODEL_OF)
            got = _run(ctx, s0, t, plan_time, rows, flags)
            assert torch.isfinite(got[0]).all()
            ident = _run(_ref(case, 0), s0, t, plan_time, rows, flags)
            for b in range(M):
                assert torch.equal(got[0][b], ident[0][b]) == (MODEL_OF[b] == 0), (case, mode, b, MODEL_OF[b])
            for b in range(M):
                ref = _run(_ref(case, MODEL_OF[b]), s0, t, plan_time, rows, flags, sel=slice(b, b + 1))
                _same(got, ref, slice(b, b + 1), (case, mode, b))
    finally:
        ctx.set_plant_models(None)


@pytest.mark.parametrize("case", ["unitree_go2_trot", "allegro_reorient", "generic", "plugin"])
def test_one_model_is_the_plain_launch_and_a_permuted_index_permutes(case):
    """V = 1 with the context's own model equals the unbound launch at M = 8.  With every plant started from the same state, rows and
    clock, the result of plant b depends on model_of[b] alone: a permuted index permutes the results."""
    import torch
    from dial_mpc_amd import _lib
    c = _make(case)
    ctx = c["ctx"]
    s0 = _start(c, seed=5)
    rows = _dev(C.rows(c["model"], c["env"], C.positional(c["model"]), seed=6))
    t, plan_time = C.clocks()
    try:
        plain = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)
        ctx.set_plant_models([c["model"]], [0] * M)
        _same(_run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL), plain, slice(None), case)
        s1, r1 = s0[1:2].expand(M, -1).contiguous(), rows[1:2].expand(M, -1, -1).contiguous()
        t1, p1 = np.full(M, t[1]), np.full(M, plan_time[1], np.float32)
        ctx.set_plant_models(c["structs"], MODEL_OF)
        a = _run(ctx, s1, t1, p1, r1, _lib.PLANT_CTRL)
        perm = [3, 1, 4, 0, 7, 6, 2, 5]
        ctx.set_plant_models(c["structs"], [MODEL_OF[p] for p in perm])
        b = _run(ctx, s1, t1, p1, r1, _lib.PLANT_CTRL)
        assert len({a[0][i].cpu().numpy().tobytes() for i in range(M)}) == 4   # four models, four different plants
        for x, y in zip(a, b):
            assert torch.equal(x[perm], y), case
    finally:
        ctx.set_plant_models(None)


@pytest.mark.parametrize("case", ["unitree_go2_trot", "unitree_h1_push_crate", "generic", "plugin", "plugin-law"])
def test_with_a_disturbance_bound_each_plant_is_the_disturbed_plant_of_its_model(case):
    """tests/test_gpu_plant_dist.py's data (gains from {0.5, 0.75, 1.25}, biases on a 1/8 grid, one to three kicks per plant whose
    windows hold one step each) bound next to the models: plant b equals plant_dist_kernel on the context of model model_of[b] with
    plant b's row bound, at M = 1."""
    import torch
    c = _make(case)
    ctx = c["ctx"]
    nu, nv = ctx.nu, ctx.nv
    s0 = _start(c, seed=14)
    t, plan_time = C.clocks()
    rng = np.random.default_rng(16)
    gain, bias = rng.choice([0.5, 0.75, 1.25], (M, nu)), rng.integers(-16, 17, (M, nu)) / 8.0
    clk = np.array([[t[m] + k * SIM_DT for k in range(K)] for m in range(M)])
    win = lambda x: (float(np.float32(x - 0.5 * SIM_DT)), float(np.float32(x + 0.5 * SIM_DT)))   # noqa: E731
    events = [[(*win(clk[m, (m + j) % K]), rng.integers(-8, 9, nv) / 64.0) for j in range(1 + m % 3)] for m in range(M)]
    packed, E = pack(nu, nv, gain, bias, events)
    dist = _dev(packed)
    try:
        for mode, flags in _modes(case, c):
            rows = _dev(_mode_rows(c, mode, seed=15))
            ctx.set_plant_models(c["structs"], MODEL_OF)
            undisturbed = _run(ctx, s0, t, plan_time, rows, flags)
            ctx.set_plant_disturbance(dist, E)
            got = _run(ctx, s0, t, plan_time, rows, flags)
            assert torch.isfinite(got[0]).all() and not torch.equal(got[0], undisturbed[0])
            for b in range(M):
                ref_ctx = _ref(case, MODEL_OF[b])
                try:
                    ref_ctx.set_plant_disturbance(dist[b:b + 1].contiguous(), E)
                    ref = _run(ref_ctx, s0, t, plan_time, rows, flags, sel=slice(b, b + 1))
                finally:
                    ref_ctx.set_plant_disturbance(None)
                _same(got, ref, slice(b, b + 1), (case, mode, b))
            ctx.set_plant_disturbance(None)
    finally:
        ctx.set_plant_disturbance(None)
        ctx.set_plant_models(None)


def test_rebind_unbind_and_a_failed_bind():
    import torch
    from dial_mpc_amd import _lib
    case = "unitree_go2_trot"
    c = _make(case)
    ctx, structs = c["ctx"], c["structs"]
    s0 = _start(c, seed=18)
    rows = _dev(C.rows(c["model"], c["env"], False, seed=19))
    t, plan_time = C.clocks()
    run = lambda cx, sel=slice(None): _run(cx, s0, t, plan_time, rows, _lib.PLANT_CTRL, sel=sel)   # noqa: E731
    try:
        plain = run(ctx)
        ctx.set_plant_models(structs, MODEL_OF)
        first = run(ctx)
        other = [1, 1, 3, 2, 0, 0, 2, 3]
        ctx.set_plant_models([structs[3], structs[1], structs[2], structs[0]], other)   # another set, another order: the results follow
        second = run(ctx)
        order = [3, 1, 2, 0]
        for b in range(M):
            _same(second, run(_ref(case, order[other[b]]), slice(b, b + 1)), slice(b, b + 1), b)
        assert not torch.equal(first[0], second[0])
        bad = type(structs[1]).from_buffer_copy(structs[1])
        bad.timestep = 0.004
        with pytest.raises(_lib.DialHipError, match=r"model 1 is rejected: its timestep"):
            ctx.set_plant_models([structs[0], bad], [0, 1] * 4)
        idx = np.array([0, 1, 4, 3, 3, 2, 1, 0], np.int32)
        arr = (_abi.DialModel * 4)(*structs)
        assert ctx.lib.dial_set_plant_models(ctx.h, arr, 4, idx.ctypes.data, M) == ARG
        assert "model_of[2] = 4 is outside" in ctx.lib.dial_last_error(ctx.h).decode()
        _same(run(ctx), second, slice(None), "a failed bind keeps the previous binding")
        ctx.set_plant_models(None)
        _same(run(ctx), plain, slice(None), "unbound: the plain kernel's results")
        ctx.set_plant_models(None)   # (unbinding twice is fine)
        assert torch.equal(run(ctx, slice(0, 4))[0], plain[0][:4])   # ... for any M
    finally:
        ctx.set_plant_models(None)


def test_refusals(tmp_path):
    import shutil
    import torch
    from dial_mpc_amd import _lib
    case = "unitree_go2_trot"
    c = _make(case)
    ctx, structs, lib, h = c["ctx"], c["structs"], c["ctx"].lib, c["ctx"].h
    copy = lambda m: type(m).from_buffer_copy(m)   # noqa: E731
    s0 = _start(c, seed=20)
    rows = _dev(C.rows(c["model"], c["env"], False, seed=21))
    t, plan_time = C.clocks()

    def refused(models, index, match, code=ARG, cx=ctx):
        with pytest.raises(_lib.DialHipError, match=match) as e:
            cx.set_plant_models(models, index)
        assert f"({code})" in str(e.value) and "dial_set_plant_models: " in str(e.value)
    # another nu
    m = copy(structs[0])
    m.nu = 11
    refused([structs[0], m], [0, 1], r"model 1 is rejected: nu = 11, the context's model has 12")
    # another dof tree: the second leg hangs off the first one's hip
    m = copy(structs[0])
    m.dof_parentid[9] = 6
    refused([m], [0], r"model 0 is rejected: .*(topology|would pick kernel instantiation 0 for it, the context runs instantiation 1)")
    # another timestep
    m = copy(structs[2])
    m.timestep = 0.004
    refused([structs[0], structs[1], m], [0, 1, 2], r"model 2 is rejected: its timestep 0.004\d* differs from the context's 0.005")
    # nine distinct (solref, solimp) rows on a Go2 context: dial_create would run such a model on the capacity-dimension kernel
    md = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in c["md"].items()}
    md["con_solref"] = np.array(md["con_solref"], np.float64)
    md["jnt_solref"] = np.array(md["jnt_solref"], np.float64)
    lim = np.asarray(md["lim_jnt"]).astype(int)
    for i in range(4):
        md["con_solref"][i, 0] = 0.02 + 0.001 * (i + 1)
    for i in range(5):
        md["jnt_solref"][lim[i], 0] = 0.03 + 0.001 * (i + 1)
    from dial_mpc_amd.plugin import kbi_unique_rows
    assert kbi_unique_rows(md) >= 9
    refused([C.variant_struct(c["model"], md)], [0], r"model 0 is rejected: dial_create would pick kernel instantiation 0 for it, the context runs instantiation 1")
    # the index, the counts, null pointers
    idx = np.array([0, 1, 2, 4], np.int32)
    arr = (_abi.DialModel * 4)(*structs)
    assert lib.dial_set_plant_models(h, arr, 4, idx.ctypes.data, 4) == ARG and "model_of[3] = 4 is outside 0 .. V - 1 = 3" in lib.dial_last_error(h).decode()
    idx[3] = -1
    assert lib.dial_set_plant_models(h, arr, 4, idx.ctypes.data, 4) == ARG and "model_of[3] = -1" in lib.dial_last_error(h).decode()
    idx[3] = 3
    for args, msg in [((arr, 0, idx.ctypes.data, 4), "V = 0 is outside 1 .. DIAL_MAX_PLANT_MODELS"),
                      ((arr, 1025, idx.ctypes.data, 4), "V = 1025 is outside"),
                      ((arr, 4, idx.ctypes.data, 0), "M = 0 is outside 1 .. DIAL_MAX_PLANTS"),
                      ((arr, 4, idx.ctypes.data, _abi.MACROS["DIAL_MAX_PLANTS"] + 1), "is outside 1 .. DIAL_MAX_PLANTS"),
                      ((None, 4, idx.ctypes.data, 4), "a null pointer with V = 4, M = 4"),
                      ((arr, 4, None, 4), "a null pointer with V = 4, M = 4")]:
        assert lib.dial_set_plant_models(h, *args) == ARG, msg
        err = lib.dial_last_error(h).decode()
        assert err.startswith("dial_set_plant_models: ") and msg in err, err
    plain = _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)   # none of the refused calls bound anything
    try:
        ctx.set_plant_models(structs, MODEL_OF)
        assert not torch.equal(_run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL)[0], plain[0])
        with pytest.raises(_lib.DialHipError, match="bound plant models index 8 plants") as e:   # M mismatch at step time
            _run(ctx, s0, t, plan_time, rows, _lib.PLANT_CTRL, sel=slice(0, 4))
        assert f"({ARG})" in str(e.value) and "dial_plant_step: " in str(e.value)
    finally:
        ctx.set_plant_models(None)
    # a plugin without the table: binding is refused, its plant still steps
    p = _make("plugin-plant-only")
    refused(p["structs"], MODEL_OF, "dial_plugin_plant_var_v1", UNSUP, p["ctx"])
    assert torch.isfinite(_run(p["ctx"], _start(p, seed=20), t, plan_time, rows, _lib.PLANT_CTRL)[0]).all()
    # dial_set_user_params / dial_set_user_table while bound: unbind first
    q = _make("plugin-law")
    try:
        q["ctx"].set_plant_models(q["structs"], MODEL_OF)
        pv = np.asarray(params(0), np.float32)
        assert q["ctx"].lib.dial_set_user_params(q["ctx"].h, pv.ctypes.data, len(pv)) == ARG
        err = q["ctx"].lib.dial_last_error(q["ctx"].h).decode()
        assert err.startswith("dial_set_user_params: plant models are bound") and "unbind first" in err
        tab = _dev(np.zeros((4, 2)))
        assert q["ctx"].lib.dial_set_user_table(q["ctx"].h, tab.data_ptr(), 4, 2, 0, 0) == ARG
        assert "dial_set_user_table: plant models are bound" in q["ctx"].lib.dial_last_error(q["ctx"].h).decode()
        q["ctx"].set_plant_models(None)
        assert q["ctx"].lib.dial_set_user_params(q["ctx"].h, pv.ctypes.data, len(pv)) == 0   # unbound: accepted again
    finally:
        q["ctx"].set_plant_models(None)
    # the IEEE measurement build has no plant, and a library without libdialplantvar.so next to it cannot bind
    ictx = _lib.Context(c["model"], c["task"], None, device=0, lib_path=_lib.IEEE_LIB_PATH)
    refused(structs, MODEL_OF, "IEEE measurement build", UNSUP, ictx)
    lone = tmp_path / "libdialhip.so"
    shutil.copy(_lib.LIB_PATH, lone)
    shutil.copy(_lib.PLANT_LIB_PATH, tmp_path / "libdialplant.so")
    lctx = _lib.Context(c["model"], c["task"], None, device=0, lib_path=str(lone))
    refused(structs, MODEL_OF, "libdialplantvar.so", UNSUP, lctx)
    _same(_run(lctx, s0, t, plan_time, rows, _lib.PLANT_CTRL), plain, slice(None), "its plain plant is what it was")


def test_plant_class_round_trip():
    """Plant(models=..., model_of=...) on the Go2 env: plant b follows its model (heavier trunk, less friction), set_models(None)
    gives the plain plants back, a list of M models maps one to one, reset() keeps the binding."""
    from dial_mpc_amd.deploy.plant import Plant
    from dial_mpc_amd.mjcf import vary_model
    c = _make("unitree_go2_trot")
    env, md = c["env"], c["md"]
    heavy, slick = vary_model(md, mass_scale={1: 1.3}), vary_model(md, friction_scale=0.5, damping_scale=2.0)
    rows = np.zeros((T, c["model"].nu), np.float32)
    plain = Plant(env, SIM_DT, "torque", M=4)
    plain.step(rows, 0.0, K=8)
    want = plain.states.cpu().numpy()
    p = Plant(env, SIM_DT, "torque", M=4, models=[md, heavy, slick], model_of=[0, 1, 2, 0])
    assert p.model_of.tolist() == [0, 1, 2, 0]
    p.step(rows, 0.0, K=8)
    got = p.states.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])
    assert not np.array_equal(got[1], want[1]) and not np.array_equal(got[2], want[2]) and not np.array_equal(got[1], got[2])
    p.reset()
    p.step(rows, 0.0, K=8)
    assert np.array_equal(p.states.cpu().numpy(), got)            # reset() keeps the binding
    p.set_models([heavy, md, md, slick])                          # M models: one to one
    p.reset()
    p.step(rows, 0.0, K=8)
    again = p.states.cpu().numpy()
    assert np.array_equal(again[0], got[1]) and np.array_equal(again[3], got[2]) and np.array_equal(again[1], want[1])
    p.set_models(None)
    p.reset()
    p.step(rows, 0.0, K=8)
    assert np.array_equal(p.states.cpu().numpy(), want)


def _sim_loop(block, ticks):
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.deploy.dial_plan import MBDPublisher
    from dial_mpc_amd.deploy.dial_sim import DialSim, DialSimConfig
    from dial_mpc_amd.utils.io_utils import get_example_path, load_dataclass_from_dict
    d = yaml.safe_load(open(get_example_path("unitree_go2_trot_deploy.yaml")))
    d["sync_mode"] = True
    d["Nsample"] = 256
    if block is not None:
        d["sim_model"] = block
    dial_config, env_config, env = load_dial_and_env(d)
    prefix = "v" + uuid.uuid4().hex[:8] + "_"
    sim = DialSim(load_dataclass_from_dict(DialSimConfig, d), env_config, dial_config, env, shm_prefix=prefix)
    pub = MBDPublisher(env, env_config, dial_config, shm_prefix=prefix)
    qs = []

    def on_tick(k):
        assert sim.step_sync(poll=0) > 0
        qs.append(sim.plant.qpos_qvel().copy())
    try:
        pub.main_loop(max_ticks=ticks, on_tick=on_tick)
        pub.close()
    finally:
        sim.close()
    return np.array(qs), sim


def test_dial_mpc_sim_with_a_sim_model_block_in_process():
    """dial-mpc-sim (sync mode) and the planner in one process, 0.2 s of sim time: with a sim_model block the plant runs the varied
    model (V = 1), stays finite and upright, and moves differently from the plant without the block."""
    block = dict(mass_scale={"base": 1.3}, com_offset={"base": [0.03, 0.0, 0.0]}, friction_scale=0.6, damping_scale=1.5, armature_scale=1.0)
    q, sim = _sim_loop(block, 10)
    assert sim.plant.model_of.tolist() == [0] and 0.2 - 0.5 * SIM_DT <= sim.t < 0.25
    q0, sim0 = _sim_loop(None, 10)
    assert sim0.plant.model_of is None
    assert np.isfinite(q).all() and q[:, 2].min() > 0.15 and q.shape == q0.shape and not np.array_equal(q, q0)
