"""The synthetic robots of tests/synthetic/ on the device (tests/synthetic_cases.py describes them): per model a task plugin with the
reward of tests/synthetic/zoo_reward.hip, under the rounding-level gate in the air (smooth_ref's rule, unchanged) and the per-transition
gate in contact (conftest.transition_parity from the device's own traced state, DIAL_LS_SWAP; no unwitnessed transition, witnessed
share <= 10 %, every rollout counted); the capacity-dimension kernel under the Go2 walk task for the two models with four sites; and
the capacity-dimension kernel's refusal of two_trees.  Each test prints its measured figures (lines starting with SMOOTH, CONTACT,
CHAIN); DESIGN.md section 2 records them."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import smooth_ref as S
import synthetic_cases as Z
from conftest import TOL, _within
from dial_mpc_amd import _abi

pytestmark = pytest.mark.gpu

K = _abi.MACROS
IREW, IUSER = K["DIAL_INFO_REWARD"], K["DIAL_INFO_USER"]


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.fixture(scope="module")
def plugins():
    """The plugin of every model, built once (or found in the cache), at most four compiler processes at a time."""
    from dial_mpc_amd.plugin import build_plugin
    with ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(lambda n: build_plugin(Z.load(n)["md"], Z.REWARD), Z.MODELS))
    return dict(zip(Z.MODELS, paths))


def _plugin_ctx(c, path):
    from dial_mpc_amd import _lib
    return _lib.Context(c["model"], c["ptask"], c["cfg"], device=0, plugin=path, user_params=list(Z.WEIGHTS))


def _walk_ctx(c):
    """The capacity-dimension kernel: no built-in instantiation has a synthetic model's dimensions."""
    from dial_mpc_amd import _lib
    assert Z.walk_task_reads_in_range(c["model"], c["otask"]) is None
    return _lib.Context(c["model"], c["otask"], c["cfg"], device=0)


def _step_chain(ctx, model, s0, acts, mirror):
    """env.step chained over `acts` from the packed state s0 -> (rewards, q, qd, x.pos) per step; mirror=True: each step's reward against
    zoo_reward.hip in NumPy on the device's own returned state, body frames, ctrl and action (tolerance of
    test_gpu_custom_env.test_rewards_match_numpy_mirror), and the reward's step counter in info_user."""
    nq, nv, nb = model.nq, model.nv, model.nbody
    ni = nq + 2 * nv
    st = _dev(s0)
    out = []
    for t, a in enumerate(acts):
        st, xpos, xquat, ctrl = ctx.env_step(st, _dev(a))
        s, xp, xq, cc = _host(st, xpos, xquat, ctrl)
        if mirror:
            want = Z.mirror_reward(model, s, xp.reshape(nb - 1, 3), xq.reshape(nb - 1, 4), cc, a)
            assert abs(s[ni + IREW] - want) <= 1e-4 * abs(want) + 1e-5, (t, float(s[ni + IREW]), want)
            assert s[ni + IUSER] == s0[ni + IUSER] + t + 1
        out.append((s[ni + IREW], s[:nq].copy(), s[nq:nq + nv].copy(), xp.reshape(-1).copy()))
    return tuple(np.array([o[k] for o in out]) for k in range(4))


def _in_the_air(c, ctx, build, rewards, mirror):
    """Gate c on one context: env_reset_batch of 16 class-F states; five env steps of ctx.rollout, 4 states x 16 rollouts (two states
    at step counter 25); env.step chained over rollout 0 of every state through the same blocks."""
    name, model = c["name"], c["model"]
    o64, o32 = Z.oracles(c)
    q16, v16, _ = S.smooth_states(c["env"], model, "F", 16, seed=21)
    gate = S.Gate(name, "F", "reset+rollout", build)
    gate.reset_blocks(model, o64, o32, q16, v16, _host(ctx.env_reset_batch(_dev(q16), _dev(v16)))[0])
    q, v, us = Z.smooth_cases(name, c["control"])
    resets, = _host(ctx.env_reset_batch(_dev(q), _dev(v)))
    states = S.with_steps(resets)
    for i in range(4):
        S.assert_stays_free(model, c["otask"], o64, states[i], us[i])
    got = [_host(*ctx.rollout(_dev(states[i]), _dev(us[i]))) for i in range(4)]
    ctx.status()
    got = tuple(np.stack([g[k] for g in got]) for k in range(4))
    r64, r32 = S.rollout_refs(o64, o32, states, us)
    gate.rollout_blocks(model, got, r64, r32, rewards=rewards)
    gate.check()
    chain = [_step_chain(ctx, model, states[i], us[i, 0], mirror) for i in range(4)]
    chain = tuple(np.stack([ch[k] for ch in chain])[:, None] for k in range(4))
    g2 = S.Gate(name, "F", "env_step chain", build)
    g2.rollout_blocks(model, chain, tuple(r[:, :1] for r in r64), tuple(r[:, :1] for r in r32), rewards=rewards)
    g2.check()
    # Bit for bit is NOT promised between env.step and a rollout: two kernels, compiled separately from the same body; what holds
    # is that both pass the gate.  Whether they happen to agree is printed.
    same = all(np.array_equal(chain[k][:, 0], got[k][:, 0]) for k in range(1, 4))
    print(f"CHAIN {name} {build}: env.step chain == rollout bit for bit: {same}; worst ratios rollout {gate.worst()[4]:.3f}, chain {g2.worst()[4]:.3f}")
    return got


AIR = [(n, "position") for n in Z.MODELS] + [("chain_mixed", "torque")]


@pytest.mark.parametrize("name,control", AIR, ids=[f"{n}-{k}" for n, k in AIR])
def test_plugin_in_the_air_at_rounding_level(plugins, name, control):
    c = Z.load(name, control)
    _in_the_air(c, _plugin_ctx(c, plugins[name]), f"plugin-{control}", rewards=False, mirror=True)


def _reset_in_contact(model, o32, q, v, s0):
    """env_reset_batch of a contact state against the fp32 oracle's reset: qpos / qvel bit for bit but for the normalised quaternions
    (conftest.TOL there), qacc_warmstart -- the solve over the contact rows -- within conftest.TOL["qd"] scaled by 1 / timestep (a
    velocity tolerance per step, as an acceleration), or from a <= 64 ulp jittered state (the gate's witness rule)."""
    nq, nv = model.nq, model.nv
    quat = S.quat_entries(model)
    assert np.array_equal(s0[nq:nq + nv], v) and np.array_equal(s0[:nq][~quat], q[~quat])
    assert _within(s0[:nq], o32.env_reset(q, v)[0][:nq], TOL["q"]).all()
    tol = dict(rtol=TOL["qd"]["rtol"], atol=TOL["qd"]["atol"] / float(model.timestep))
    w = slice(nq + nv, nq + 2 * nv)
    rng = np.random.default_rng(17)
    for k in range(65):
        qj, vj = q.copy(), v.copy()
        if k:
            mag = 2.0 ** ((k - 1) * 7 // 64)
            qj += (rng.integers(-1, 2, nq) * mag * np.spacing(np.abs(q))).astype(np.float32)
            vj += (rng.integers(-1, 2, nv) * mag * np.spacing(np.abs(v))).astype(np.float32)
        if _within(s0[w], o32.env_reset(qj, vj)[0][w], tol).all():
            return k
    raise AssertionError(("reset: qacc_warmstart outside the gate, no witness", float(np.abs(s0[w] - o32.env_reset(q, v)[0][w]).max())))


def _in_contact(c, ctx, q, v, us, build, physics_only, mirror):
    """Gate d on one context: per start state a rollout launch with the state trace, every transition of every rollout through
    conftest.transition_parity; then env.step chained for 8 steps against rollout 0 at conftest.TOL."""
    model = c["model"]
    _, o32 = Z.oracles(c)
    trace_dev = ctx.set_state_trace(us.shape[1])
    tot, worst, outs = [0, 0], 0.0, []
    for i in range(len(q)):
        s0, = _host(ctx.env_reset_batch(_dev(q[i:i + 1]), _dev(v[i:i + 1])))
        s0 = s0[0]
        _reset_in_contact(model, o32, q[i], v[i], s0)
        got = _host(*ctx.rollout(_dev(s0), _dev(us[i])))
        ctx.status()
        rep = Z.contact_gate(c, o32, s0, us[i], got, trace_dev.cpu().numpy(), physics_only)
        assert rep["transitions"] == us.shape[1] * us.shape[2] and not rep["unwitnessed"], rep
        tot[0] += rep["witnessed"]
        tot[1] += rep["transitions"]
        worst = max(worst, rep["direct_worst"])
        chain = _step_chain(ctx, model, s0, us[i, 0], mirror)
        for k, key in ((1, "q"), (2, "qd"), (3, "x")):
            assert _within(chain[k], got[k][0], TOL[key]).all(), (i, key, float(np.abs(chain[k] - got[k][0]).max()))
        outs.append(got)
    print(f"CONTACT {c['name']} {build}: witnessed {tot[0]} / {tot[1]}, worst direct transition {worst:.4f} x TOL")
    assert tot[0] <= Z.WITNESS_CAP * tot[1], tot
    return outs


# Measured on one MI355X (2026-10-21), witnessed / transitions and the worst direct transition in units of TOL: chain_mixed 0 / 256, 0.0014;
# fixed_arm 0 / 256, 0.0101; two_trees 0 / 256, 0.0009; wide_base 0 / 256, 0.0044; deep_chain 0 / 256, 0.0077.  Capacity-dimension kernel:
# chain_mixed 0 / 256, 0.0013; wide_base 0 / 256, 0.0035.  In the air, worst ratio rollout / env.step chain: 0.18 / 0.56, 0.19 / 0.45, 0.20 / 0.21,
# 0.21 / 0.23, 0.23 / 0.41 (same order), chain_mixed under torque control 0.21 / 0.44; the chain equalled the rollout bit for bit every time.
# reverse_once on the plugins 0.17, 0.27, 0.19, 0.29, 0.20 (same order), on the capacity-dimension kernel 0.32 / 0.25; plant_step CTRL 0.18 (chain_mixed),
# 0.17 (fixed_arm), PD 0.14 (chain_mixed, motors only).
@pytest.mark.parametrize("name", Z.MODELS)
def test_plugin_in_contact_per_transition(plugins, name):
    c, q, v, us = Z.contact_cases(name)
    _in_contact(c, _plugin_ctx(c, plugins[name]), q, v, us, "plugin", physics_only=True, mirror=True)


def test_two_trees_falling_case_on_the_device(plugins):
    """The named case of tests/test_synthetic_models.py (capsule-capsule candidates between the two trees inside their margin at the
    start, velocities in +- 1): the plugin's distance from the fp64 oracle is the fp32 oracle's own at every step (within a factor 2),
    and every transition passes conftest.TOL directly."""
    c = Z.load("two_trees", "position", N=Z.CONTACT_B - 1, H=Z.CONTACT_T - 1)
    o64, o32 = Z.oracles(c)
    q, v, us = Z.falling_case(c)
    ctx = _plugin_ctx(c, plugins["two_trees"])
    trace_dev = ctx.set_state_trace(us.shape[0])
    s0 = _host(ctx.env_reset_batch(_dev(q[None]), _dev(v[None])))[0][0]
    got = _host(*ctx.rollout(_dev(s0), _dev(us)))
    ctx.status()
    r64, r32 = o64.rollout(s0, us), o32.rollout(s0, us)
    for t in range(us.shape[1]):
        for k, what in ((1, "q"), (2, "qd")):
            e_dev, e_32 = np.abs(got[k][:, t] - r64[k][:, t]).max(), np.abs(r32[k][:, t] - r64[k][:, t]).max()
            print(f"FALLING step {t} {what}: device - fp64 {e_dev:.3e}, fp32 oracle - fp64 {e_32:.3e}")
            assert e_dev <= 2 * e_32 + 1e-6, (t, what, e_dev, e_32)
    rep = Z.contact_gate(c, o32, s0, us, got, trace_dev.cpu().numpy(), physics_only=True)
    assert rep["direct"] == rep["transitions"] == us.shape[0] * us.shape[1], rep


# ------------------------------------------------------------------------------------------------------------------ capacity-dimension kernel
@pytest.mark.parametrize("name", Z.WALK)
def test_capacity_kernel_under_the_walk_task(plugins, name):
    """The capacity-dimension kernel (DimsMax) on the two models with four sites, Go2 walk task with the feet mapped to them (checked
    to read nothing outside the model first): gates c and d WITH the rewards, and per rollout against the plugin of the same model."""
    c = Z.load(name)
    ctx = _walk_ctx(c)
    air = _in_the_air(c, ctx, "capacity-kernel", rewards=True, mirror=False)
    assert ctx.debug_last_launch()["inst"] == 0
    q, v, us = Z.smooth_cases(name)
    pctx = _plugin_ctx(c, plugins[name])
    for i in range(4):   # same start states (the reset's bits may differ between the kernels: each from its own reset)
        st = S.with_steps(_host(pctx.env_reset_batch(_dev(q), _dev(v)))[0])[i]
        pl = _host(*pctx.rollout(_dev(st), _dev(us[i])))
        for k, key in ((1, "q"), (2, "qd"), (3, "x")):
            assert _within(pl[k], air[k][i], TOL[key]).all(), (name, i, key)
    cc, qc, vc, usc = Z.contact_cases(name)
    wctx = _walk_ctx(cc)
    wal = _in_contact(cc, wctx, qc, vc, usc, "capacity-kernel", physics_only=False, mirror=False)
    pin = _in_contact(cc, _plugin_ctx(cc, plugins[name]), qc, vc, usc, "plugin", physics_only=True, mirror=False)
    for i in range(2):   # per rollout, the plugin against the capacity-dimension kernel; knife-edge rollouts: at most one per state
        ok = np.ones(usc.shape[1:3], bool)
        for k, key in ((1, "q"), (2, "qd"), (3, "x")):
            w = _within(pin[i][k], wal[i][k], TOL[key])
            ok &= w.reshape(*usc.shape[1:3], -1).all(-1)
        assert ok[:, 0].all() and (~ok.all(1)).sum() <= 1, (name, i, np.flatnonzero(~ok.all(1)).tolist())


def test_capacity_kernel_refuses_two_trees():
    """dial_create without a plugin: a pyramidal model with sphere-capsule / capsule-capsule candidates is refused with a message (the
    built-in pyramidal kernels have no such narrow phase)."""
    from dial_mpc_amd import _lib
    c = Z.load("two_trees")
    task = Z.walk_task(c["md"], c["ptask"], feet=False, home_z=0.3)
    task.nfeet = 4   # (dial_create's own check of the Go2 tasks; the sites are never read: no context comes to exist)
    with pytest.raises(_lib.DialHipError, match="task plugin only"):
        _lib.Context(c["model"], task, c["cfg"], device=0)


# ------------------------------------------------------------------------------------------------------------------ planner path
def _planner_case(name):
    """(case, fp64 / fp32 oracles, inputs, candidate reset inputs) of one reverse_once: N = 63, Hnode = Hsample = 2 (the nodes ARE the
    controls), Ybar scale 0.2, a quarter of the noise scale, eight class-F candidate states."""
    from conftest import seeded_inputs
    from dial_mpc_amd.core.dial_config import DialConfig
    c = Z.load(name, "position", N=63, H=2)
    eps, sigma, Ybar = seeded_inputs(DialConfig(Nsample=63, Hsample=2, Hnode=2), c["model"].nu, seed=41, Ybar_scale=0.2)
    q, v, _ = S.smooth_states(c["env"], c["model"], "F", 8, seed=42)
    return c, Z.oracles(c), (eps, (0.25 * sigma).astype(np.float32), Ybar), (q, v)


def _planner_gate(c, ctx, oracles, inputs, qv, build, rewards):
    """reverse_once from the first candidate state whose 64 fp64 trajectories stay in class F, through the planner block of the smooth
    gate: the nodes (Y0s) and, where the oracle's task is the context's (rewards=True), the per-step rewards."""
    model, task, cfg = c["model"], c["otask"], c["cfg"]
    (o64, o32), (eps, sigma, Ybar) = oracles, inputs
    resets, = _host(ctx.env_reset_batch(_dev(qv[0]), _dev(qv[1])))
    chosen = None
    for i in range(len(resets)):
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
    gate = S.Gate(c["name"], "F", "planner", build)
    if rewards:
        for t in range(cfg.Hsample + 1):
            gate.block("reward", t, sc["rewss"][:, t], ref64["rewss"][:, t], ref32["rewss"][:, t])
    gate.block("Y0s", "-", sc["Y0s"], ref64["us"], ref32["us"])
    # the rollouts' states against both oracles run on the DEVICE's own controls (Hnode = Hsample: its nodes, exact fp32 inputs)
    us_dev = np.ascontiguousarray(sc["Y0s"], np.float32)
    r64, r32 = (tuple(np.asarray(a, np.float64) for a in o.rollout(resets[chosen], us_dev)) for o in (o64, o32))
    gate.rollout_blocks(model, (sc["rewss"], sc["qss"], sc["qdss"], sc["xss"]), r64, r32, rewards=False)
    gate.check()
    print(f"PLANNER {c['name']} {build}: worst ratio {gate.worst()[4]:.3f}")
    return sc, resets[chosen]


@pytest.mark.parametrize("name", Z.MODELS)
def test_plugin_planner_path_in_the_air(plugins, name):
    """One reverse_once per model on its plugin: the nodes against the fp64 oracle's, and the rollouts' states (the scratch's qss / qdss /
    xss) against the two oracles run on the device's own nodes, through the gate.  The reward is the plugin's own and is not gated here
    (tests of env.step compare it with its NumPy restatement); it must be finite and differ between rollouts."""
    c, oracles, inputs, qv = _planner_case(name)
    sc, s0 = _planner_gate(c, _plugin_ctx(c, plugins[name]), oracles, inputs, qv, "plugin", rewards=False)
    assert np.isfinite(sc["rewss"]).all() and sc["rewss"].std() > 0


@pytest.mark.parametrize("name", Z.WALK)
def test_capacity_kernel_planner_path_in_the_air(name):
    """The same on the capacity-dimension kernel under the walk task, with the per-step rewards gated."""
    from dial_mpc_amd import _lib
    c, oracles, inputs, qv = _planner_case(name)
    _planner_gate(c, _lib.Context(c["model"], c["otask"], c["cfg"], device=0), oracles, inputs, qv, "capacity-kernel", rewards=True)


# ------------------------------------------------------------------------------------------------------------------ plant
PLANT_MODELS = ("chain_mixed", "fixed_arm")


@pytest.fixture(scope="module")
def plant_plugins():
    from dial_mpc_amd.plugin import build_plugin
    with ThreadPoolExecutor(max_workers=2) as ex:
        paths = list(ex.map(lambda n: build_plugin(Z.load(n)["md"], Z.REWARD, plant=True), PLANT_MODELS))
    return dict(zip(PLANT_MODELS, paths))


def _plant_case(name, pd, motors_only=False):
    """The model at sim rate (one physics step of 0.005 s per step) with the action map made the identity up to the factor R, as
    tests/test_gpu_plant.py does: (case, plugin task, oracle task).  motors_only: the same model with every actuator a motor (the
    compiled struct's act_isposition cleared; dimensions, and so the plugin, stay) -- what DIAL_PLANT_PD accepts."""
    from test_gpu_plant import R, SIM_DT
    c = dict(Z.load(name, "position"))
    assert abs(c["model"].timestep - SIM_DT) < 1e-9
    if motors_only:
        c["model"] = type(c["model"]).from_buffer_copy(c["model"])
        for a in range(c["model"].nu):
            c["model"].act_isposition[a] = 0
    tasks = []
    for key in ("ptask", "otask"):
        t = type(c[key]).from_buffer_copy(c[key])
        t.n_frames, t.dt, t.position_control, t.action_scale = 1, SIM_DT, 0 if pd else 1, 1.0
        for a in range(c["model"].nu):
            t.joint_offset[a] = 0.0
            t.joint_range[a][0], t.joint_range[a][1] = -R, R
            t.phys_range[a][0], t.phys_range[a][1] = -R, R
        tasks.append(t)
    return c, tasks[0], tasks[1]


PLANT = [("chain_mixed", False), ("fixed_arm", False), ("chain_mixed", True)]


@pytest.mark.parametrize("name,pd", PLANT, ids=[f"{n}-{'PD' if p else 'CTRL'}" for n, p in PLANT])
def test_plugin_plant_step_in_the_air(plant_plugins, name, pd):
    """One plant_step (K = 1, with a trace) of 64 class-F plants at dt 0.005 on the plant kernel of the model's plugin, dyadic rows in
    +- 0.25 picked by the host's clock rule: the state after the step against ONE fp64 oracle step from the same downloaded state under
    smooth_ref's rule; the trace row holds the state before the step bit for bit, and under DIAL_PLANT_CTRL the picked row.
    DIAL_PLANT_PD refuses a model with a position actuator (test_plant_pd_refusals), which chain_mixed has: its PD case runs the same
    model with the wrist servo as a motor (the same plugin; the oracle runs that model too)."""
    import oracle as O
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import ctrl_row
    from test_gpu_plant import CTRL_DT, SIM_DT, R, T, _clocks
    M = 64
    c, ptask, otask = _plant_case(name, pd, motors_only=pd)
    model = c["model"]
    nq, nv, nu = model.nq, model.nv, model.nu
    o64, o32 = O.Oracle(model, otask, None, np.float64), O.Oracle(model, otask, None, np.float32)
    ctx = _lib.Context(model, ptask, None, device=0, plugin=plant_plugins[name], user_params=list(Z.WEIGHTS))
    q, v, _ = S.smooth_states(c["env"], model, "F", M, seed=31)
    states = ctx.env_reset_batch(_dev(q), _dev(v))
    s0 = states.cpu().numpy().copy()
    rows = (np.random.default_rng(32).integers(-64, 65, (M, T, nu)) / 256).astype(np.float32)
    t, plan_time = _clocks(M)
    import torch
    trace = _dev(np.zeros((M, 1, 1 + nq + nv + nu)))
    ctx.plant_step(states, torch.as_tensor(t, dtype=torch.float64, device="cuda"), _dev(plan_time), _dev(rows), CTRL_DT, SIM_DT, 1,
                   _lib.PLANT_PD if pd else _lib.PLANT_CTRL, trace)
    got, tr = _host(states, trace)
    assert np.array_equal(tr[:, 0, 1:1 + nq + nv], s0[:, :nq + nv]), "the trace row is not the pre-step state, bit for bit"
    us = np.array([rows[m, ctrl_row(t[m], plan_time[m], CTRL_DT, T)] for m in range(M)]) / np.float32(R)
    if not pd:
        assert np.array_equal(tr[:, 0, 1 + nq + nv:], us * np.float32(R)), "DIAL_PLANT_CTRL: the trace's ctrl is the picked row"
    r64 = [o64.rollout(s0[m], us[m][None, None]) for m in range(M)]
    r32 = [o32.rollout(s0[m], us[m][None, None]) for m in range(M)]
    ref = lambda rs: (np.array([r[1][0, 0] for r in rs], np.float64), np.array([r[2][0, 0] for r in rs], np.float64))  # noqa: E731
    gate = S.Gate(name, "F", "plant-" + ("PD" if pd else "CTRL"), "plugin")
    gate.state_blocks(model, "-", got[:, :nq], got[:, nq:nq + nv], ref(r64), ref(r32))
    gate.check()
    print(f"PLANT {name} {'PD' if pd else 'CTRL'}: worst ratio {gate.worst()[4]:.3f}")


def test_plant_pd_refusals(plant_plugins):
    """DIAL_PLANT_PD hands the row to a PD law that reads actuator a's joint at qpos[7 + a] / qvel[6 + a] and applies a torque.  Both
    models have position actuators and are refused for that, before anything else; with every actuator a motor chain_mixed is accepted
    (test_plugin_plant_step_in_the_air) and fixed_arm, which has no free joint, is refused by the 7 + a check."""
    import torch
    from dial_mpc_amd import _lib
    from test_gpu_plant import CTRL_DT, SIM_DT, T
    for name, motors_only, match in (("chain_mixed", False, "position actuators"), ("fixed_arm", False, "position actuators"),
                                     ("fixed_arm", True, r"qpos\[7 \+ a\]")):
        c, ptask, _ = _plant_case(name, True, motors_only)
        ctx = _lib.Context(c["model"], ptask, None, device=0, plugin=plant_plugins[name], user_params=list(Z.WEIGHTS))
        st = ctx.env_reset_batch(_dev(np.asarray(c["env"]._init_q)[None]), _dev(np.zeros((1, c["model"].nv))))
        with pytest.raises(_lib.DialHipError, match=match) as e:
            ctx.plant_step(st, torch.zeros(1, dtype=torch.float64, device="cuda"), _dev([0.0]), _dev(np.zeros((1, T, c["model"].nu))), CTRL_DT,
                           SIM_DT, 1, _lib.PLANT_PD)
        assert f"({K['DIAL_ERR_ARG']})" in str(e.value), str(e.value)


def test_plugin_context_refuses_implicit_damping(plugins):
    """dial_create_plugin on a pyramidal model with eulerdamp = 1 (check_model bypassed: the struct is edited after the plugin was
    built): refused with DIAL_ERR_UNSUPPORTED and dial_create's message, which both entry points share."""
    from dial_mpc_amd import _lib
    c = Z.load("chain_mixed")
    m2 = type(c["model"]).from_buffer_copy(c["model"])
    m2.eulerdamp = 1
    with pytest.raises(_lib.DialHipError, match="eulerdamp is only supported on the elliptic-cone instantiations") as e:
        _lib.Context(m2, c["ptask"], c["cfg"], device=0, plugin=plugins["chain_mixed"], user_params=list(Z.WEIGHTS))
    assert f"({K['DIAL_ERR_UNSUPPORTED']})" in str(e.value)
