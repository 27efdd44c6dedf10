"""The device at ROUNDING LEVEL against the fp64 oracle in the regime where the answer is unique and smooth: a robot in the air
(tests/smooth_ref.py).  Only shipped entry points -- env_reset_batch, plant_step, rollout, reverse_once -- on the product build, the
capacity-dimension kernels, the Go2 pair kernels, the IEEE build and a task plugin.  Every block's tolerance is 8 x the fp32 oracle's
own distance from the fp64 oracle (smooth_ref.tolerance); no witnesses, no jitter, no case left out.  Each test prints, per block, its
worst error, tolerance and ratio (lines that start with SMOOTH).  The measured ratios are in DESIGN.md section 2."""
import os

import numpy as np
import pytest

import smooth_ref as S
from conftest import LS_IN_BRACKET, LS_SWAP, seeded_inputs, setup_case, with_solver
from test_gpu_plant import CTRL_DT, GEN, INST, SIM_DT, R, T as PLANT_T, _case as plant_case, _clocks, _dev, _rows

pytestmark = pytest.mark.gpu

GO2, JUMP, H1, LOCO, HAND, CRATE, PUSH = S.EXAMPLES
assert (GO2, H1, LOCO, HAND) == ("unitree_go2_trot", "unitree_h1_jog", "unitree_h1_loco", "allegro_reorient")


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _oracle_pair(model, task, cfg=None):
    import oracle as O
    return O.Oracle(model, task, cfg, np.float64), O.Oracle(model, task, cfg, np.float32)


# ------------------------------------------------------------------------------------------------------------------ reset
@pytest.mark.parametrize("example", S.EXAMPLES)
def test_reset_at_rounding_level(example):
    """env_reset_batch on 64 class-F states (and 64 class-L states of the pyramidal models): qvel and qpos come back bit for bit --
    but for the free joints' quaternions, which kinematics normalises in place --, and qacc_warmstart, i.e. qacc_smooth (class L:
    the solve over the active limit rows), matches the fp64 oracle's reset under the rule."""
    from dial_mpc_amd import _lib
    _, env, model, task, _ = S.case(example)
    o64, o32 = S.oracles(example)
    ctx = _lib.Context(model, task, None, device=0)
    for cls in ("F", "L") if example in S.PYRAMIDAL else ("F",):
        q, v, _ = S.smooth_states(env, model, cls, 64, seed=21)
        states, = _host(ctx.env_reset_batch(_dev(q), _dev(v)))
        gate = S.Gate(example, cls, "reset", "product")
        gate.reset_blocks(model, o64, o32, q, v, states)
        gate.check()


# ------------------------------------------------------------------------------------------------------------------ plant, one step
PLANT = [(ex, None) for ex in INST] + [(GO2, GEN), (LOCO, GEN)]


@pytest.mark.parametrize("example,options", PLANT, ids=[f"{ex}{'-generic' if o else ''}" for ex, o in PLANT])
def test_plant_step_at_rounding_level(example, options):
    """plant_step, K = 1 with a trace, M = 64 plants in test_gpu_plant's setting (dt 0.005, identity action map, dyadic rows), modes
    DIAL_PLANT_CTRL and DIAL_PLANT_PD, classes F and L: the state after the step against ONE fp64 oracle step from the same
    downloaded fp32 state, under the rule; the trace row holds the state before the step bit for bit."""
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import ctrl_row
    M = 64
    position = example == HAND     # position actuators: DIAL_PLANT_PD is refused
    for pd in (False,) if position else (False, True):
        env, model, task = plant_case(example, pd)
        o64, o32 = _oracle_pair(model, task)
        ctx = _lib.Context(model, task, None, device=0, options=options)
        assert ctx.debug_last_launch()["inst"] == (0 if options else INST[example])
        nq, nv = ctx.nq, ctx.nv
        for cls in ("F",) if position else ("F", "L"):
            q, v, _ = S.smooth_states(env, model, cls, M, seed=31)
            states = ctx.env_reset_batch(_dev(q), _dev(v))
            s0 = states.cpu().numpy().copy()
            rows = _rows(env, M, pd, seed=32)
            t, plan_time = _clocks(M)
            trace = _dev(np.zeros((M, 1, 1 + nq + nv + ctx.nu)))
            ctx.plant_step(states, _dev(t, np.float64), _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, 1, _lib.PLANT_PD if pd else _lib.PLANT_CTRL, trace)
            got, tr = _host(states, trace)
            assert np.array_equal(tr[:, 0, 1:1 + nq + nv], s0[:, :nq + nv]), "the trace row is not the pre-step state, bit for bit"
            us = np.array([rows[m, ctrl_row(t[m], plan_time[m], CTRL_DT, PLANT_T)] for m in range(M)]) / np.float32(R)
            if not pd:
                assert np.array_equal(tr[:, 0, 1 + nq + nv:], us * np.float32(R)), "DIAL_PLANT_CTRL: the trace's ctrl is the picked row"
            r64 = [o64.rollout(s0[m], us[m][None, None]) for m in range(M)]
            r32 = [o32.rollout(s0[m], us[m][None, None]) for m in range(M)]
            ref = lambda rs: (np.array([r[1][0, 0] for r in rs], np.float64), np.array([r[2][0, 0] for r in rs], np.float64))  # noqa: E731
            gate = S.Gate(example, cls, "plant-" + ("PD" if pd else "CTRL"), "generic" if options else "product")
            gate.state_blocks(model, "-", got[:, :nq], got[:, nq:nq + nv], ref(r64), ref(r32))
            gate.check()


# ------------------------------------------------------------------------------------------------------------------ rollouts
def _device_rollouts(example, model=None, options=None, lib_path=None, B=16, gate=True, build="product"):
    """Five env steps of B rollouts from each of the four class-F rollout cases on a context of `example`; gated unless gate=False.
    Returns the device's (rewss, qss, qdss, xss), stacked [4, B, T, ...]."""
    from dial_mpc_amd import _lib
    _, env, model0, task, cfg = S.case(example)
    model = model0 if model is None else model
    o64, o32 = _oracle_pair(model, task, cfg)
    ctx = _lib.Context(model, task, cfg, device=0, options=options, lib_path=lib_path)
    q, v, us = S.rollout_cases(example)
    us = np.ascontiguousarray(us[:, :B])
    resets, = _host(ctx.env_reset_batch(_dev(q), _dev(v)))
    states = S.with_steps(resets)
    got = [_host(*ctx.rollout(_dev(states[i]), _dev(us[i]))) for i in range(len(states))]
    ctx.status()
    got = tuple(np.stack([g[k] for g in got]) for k in range(4))
    if gate:
        for i in range(len(states)):   # from the device's own start state, every physics step of the fp64 trajectories is in class F
            S.assert_stays_free(model, task, o64, states[i], us[i])
        g = S.Gate(example, "F", "rollout", build)
        g.reset_blocks(model, o64, o32, q, v, resets)
        g.rollout_blocks(model, got, *S.rollout_refs(o64, o32, states, us))
        g.check()
    return got, ctx


@pytest.mark.parametrize("example", S.EXAMPLES)
def test_rollouts_at_rounding_level(example):
    """ctx.rollout, B = 16, H = 4 from four class-F states per example (two of them mid-episode: step counter 25), us uniform in
    +- 0.3: rewss, qss, qdss, xss against the fp64 oracle per step index under the rule."""
    _device_rollouts(example)


@pytest.mark.parametrize("pair_mode,B", [(1, 16), (2, 15)])
def test_go2_pair_modes_at_rounding_level(pair_mode, B):
    """The Go2 on the one-sample kernels at any batch (pair_mode = 1) and on the two-samples-per-wavefront kernels (pair_mode = 2)
    with an odd batch: the upper half of the last wavefront idles."""
    _, ctx = _device_rollouts(GO2, options=dict(pair_mode=pair_mode), B=B, build=f"pair_mode={pair_mode}")
    assert ctx.debug_last_launch()["pair"] == (pair_mode == 2)


@pytest.mark.parametrize("example", [GO2, LOCO])
def test_generic_kernel_rollouts_at_rounding_level(example):
    _, ctx = _device_rollouts(example, options=GEN, build="generic")
    assert ctx.debug_last_launch()["inst"] == 0


@pytest.mark.parametrize("example", [GO2, H1])
def test_ieee_build_rollouts_at_rounding_level(example):
    from dial_mpc_amd import _lib
    if not os.path.exists(_lib.IEEE_LIB_PATH):
        pytest.skip("libdialhip_ieee.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    _device_rollouts(example, lib_path=_lib.IEEE_LIB_PATH, build="IEEE")


@pytest.mark.parametrize("example", [GO2, H1])
def test_line_search_rule_does_not_matter_in_free_flight(example):
    """Class F has no active row: the Newton solver returns qacc_smooth before any line search, so DIAL_LS_SWAP and the shipped
    DIAL_LS_IN_BRACKET give the same bits on the device."""
    _, _, model, _, _ = S.case(example)
    assert model.ls_rule == LS_SWAP
    swap, _ = _device_rollouts(example, gate=False)
    shipped, _ = _device_rollouts(example, model=with_solver(model, ls_rule=LS_IN_BRACKET), build="product-in-bracket")
    for a, b in zip(swap, shipped):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ planner path
@pytest.mark.parametrize("example", S.LEGGED)
def test_planner_path_at_rounding_level(example):
    """reverse_once from one class-F state, N = 63, Hnode = Hsample = 2 (the shortest a config may have: three spline points), Ybar
    scale 0.2, noise as data at a quarter of the config's scale: the device's per-step rewards (debug_scratch) against the fp64 oracle's reverse_once under the rule --
    what reaches K2 and the control tables through nodes instead of us.  With Hnode = Hsample the nodes ARE the controls, so Y0s is
    gated against the oracle's us as well."""
    from dial_mpc_amd import _lib
    dc, env, model, task, cfg = setup_case(example, 63, 2, Hnode=2, per_rollout=True)
    o64, o32 = _oracle_pair(model, task, cfg)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=41, Ybar_scale=0.2)
    # a quarter of the config's noise scale: at full size (sigma ~ 1, us clipped to +- 1) some of the Go2's 64 rollouts reach a joint
    # limit within three steps from every candidate state, whatever its joint velocities (fp64 oracle)
    sigma = (0.25 * sigma).astype(np.float32)
    q, v, _ = S.smooth_states(env, model, "F", 8, seed=42)
    ctx = _lib.Context(model, task, cfg, device=0)
    resets, = _host(ctx.env_reset_batch(_dev(q), _dev(v)))
    chosen = None
    for i in range(len(resets)):   # the first state all of whose 64 fp64 trajectories stay in class F (the oracle alone decides)
        ref64 = o64.reverse_once(resets[i], Ybar, sigma, eps, full=True)
        try:
            S.assert_stays_free(model, task, o64, resets[i], ref64["us"].astype(np.float32))
        except AssertionError:
            continue
        chosen = i
        break
    assert chosen is not None, "no candidate state keeps the planner's 64 rollouts in class F"
    ref32 = o32.reverse_once(resets[chosen], Ybar, sigma, eps, full=True)
    ctx.reverse_once(_dev(resets[chosen]), _dev(Ybar), _dev(sigma), _dev(eps))
    ctx.status()
    sc = ctx.debug_scratch()
    gate = S.Gate(example, "F", "planner", "product")
    for t in range(cfg.Hsample + 1):
        gate.block("reward", t, sc["rewss"][:, t], ref64["rewss"][:, t], ref32["rewss"][:, t])
    assert sc["Y0s"].shape == ref64["us"].shape
    gate.block("Y0s", "-", sc["Y0s"], ref64["us"], ref32["us"])
    gate.check()


# ------------------------------------------------------------------------------------------------------------------ task plugin
def test_task_plugin_rollouts_at_rounding_level():
    """The default Go2 probe plugin of tests/plugin_cases.py: the rollout gate on qss / qdss / xss (the probe's reward is its own)."""
    from dial_mpc_amd import _lib
    from plugin_cases import build_matrix, load_case
    c = load_case("go2", N=15, H=4)
    model, cfg = c["model"], c["cfg"]
    o64, o32 = _oracle_pair(model, c["otask"], cfg)
    ctx = _lib.Context(model, c["ptask"], cfg, plugin=build_matrix(["go2"])["go2"], user_params=[0, 0])
    q, v, us = S.rollout_cases(GO2)
    resets, = _host(ctx.env_reset_batch(_dev(q), _dev(v)))
    states = S.with_steps(resets)
    for i in range(len(states)):
        S.assert_stays_free(model, c["otask"], o64, states[i], us[i])
    got = [_host(*ctx.rollout(_dev(states[i]), _dev(us[i]))) for i in range(len(states))]
    got = tuple(np.stack([g[k] for g in got]) for k in range(4))
    gate = S.Gate(GO2, "F", "rollout", "plugin")
    gate.reset_blocks(model, o64, o32, q, v, resets)
    gate.rollout_blocks(model, got, *S.rollout_refs(o64, o32, states, us), rewards=False)
    gate.check()
