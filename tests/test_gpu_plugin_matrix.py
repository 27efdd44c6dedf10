"""Task plugins across models, reward inputs and launch paths (GPU).  Every model of tests/plugin_cases.py carries the probe reward of
tests/plugin_probe.hip, which returns one element of the reward's inputs (csrc/user_reward.h) chosen at run time: a plugin per model
reads every input, and each one is compared with the fp32 oracle of the robot's built-in task (physics does not depend on the reward)
or with the device's own outputs where the contract makes them identical.  Launch paths a plugin context takes (relay, rollout queue,
state trace, contact overflow, grouped plans) are held to bit identity with the plain launch."""
import numpy as np
import pytest

from conftest import TOL, _within, perturbed_state, seeded_inputs
from dial_mpc_amd import _abi
from plugin_cases import CASES, CRATES, F, PROBE_BAD, build_matrix, load_case
from test_gpu_custom_env import _physics_gate

pytestmark = pytest.mark.gpu

ALL = list(CASES)
H = 12
IU, IREW, ISTEP = _abi.MACROS["DIAL_INFO_USER"], _abi.MACROS["DIAL_INFO_REWARD"], _abi.MACROS["DIAL_INFO_STEP"]

# Tolerances of the pre-integration forward quantities against Oracle.forward_dump (fp32 both sides).
# n_frames == 1: the reference is computed from the SAME fp32 state, so only the evaluation differs: forward kinematics chains at most
# 12 rotations / translations of O(1 m) (each a few fp32 roundings, 2^-24 relative), so positions and quaternions agree to ~1e-6;
# 2e-5 leaves a 10x margin.  Contact distance / position add one narrow phase on top (box routines: a few dozen operations on O(1 m)
# coordinates), 5e-5.
# n_frames > 1: the reference state itself comes from n_frames - 1 oracle sub-steps from the same start state, so it carries the
# solver's fp32 rounding of those sub-steps (the suite's per-step gate on q is 3e-4, conftest.TOL): 1e-3 on everything.
TOL_KIN, TOL_CON, TOL_SUB = 2e-5, 5e-5, 1e-3


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


@pytest.fixture(scope="module")
def plugins():
    return build_matrix()


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = load_case(name, N=16, H=H)
    return _cases[name]


def _ctx(c, path, params=(0, 0), cfg=True, **opts):
    from dial_mpc_amd import _lib
    return _lib.Context(c["model"], c["ptask"], c["cfg"] if cfg else None, plugin=path, user_params=list(params), options=opts)


def _oracle(c, model=None, frames=None):
    import oracle as O
    t = c["otask"]
    if frames is not None:   # the same task with fewer physics sub-steps per control step (test_physics_pins does the same)
        t = type(t).from_buffer_copy(t)
        t.n_frames, t.dt = frames, float(np.float32(c["model"].timestep) * frames)
    return O.Oracle(c["model"] if model is None else model, t, c["cfg"], np.float32)


def _starts(c, o64=None):
    """The keyframe, three perturbed states and, for the crate scenes, touching poses (those of their own tests)."""
    import oracle as O
    env, nv = c["env"], c["model"].nv
    out = [(np.array(env._init_q, np.float64), np.zeros(nv))] + [perturbed_state(env, s) for s in range(3)]
    if c["name"] in CRATES:
        o64 = O.Oracle(c["model"], c["otask"], c["cfg"], np.float64)
        if c["name"] == "go2_crate":
            from test_crate_climb import touching_state
            out += [touching_state(env, o64, s) for s in range(2)]
        else:
            from test_push_crate import pushing_state
            out += [pushing_state(env, o64, s) for s in range(2)]
    return out


def _pre_state(c, o32, state, action):
    """The state whose forward() the reward's pre-integration inputs come from: the start state when n_frames == 1, else the state
    before the LAST physics sub-step (an oracle env.step of n_frames - 1 sub-steps from the same start)."""
    nf = c["otask"].n_frames
    if nf == 1:
        return state
    s1, _, _, _ = _oracle(c, frames=nf - 1).env_step(state, action)
    return s1


def _fwd_ref(c, o32, pre):
    nq, nv = c["model"].nq, c["model"].nv
    d = o32.forward_dump(pre[:nq], pre[nq:nq + nv], None, pre[nq + nv:nq + 2 * nv])
    return dict(xpos=d["xpos"].ravel(), xquat=d["xquat"].ravel(), spos=d["site_xpos"].ravel(), cdist=d["con_dist"].ravel(),
                cpos=d["con_pos"].ravel())


@pytest.mark.parametrize("name", ALL)
def test_env_reset_and_step_match_oracle(plugins, name):
    """a. env.reset / env.step on the plugin == the fp32 oracle, from the keyframe, perturbed states and (crates) touching poses, at
    the tolerances of test_gpu_parity.test_env_reset_and_step_match_oracle."""
    c = _case(name)
    model, nv, nq = c["model"], c["model"].nv, c["model"].nq
    ctx, o32 = _ctx(c, plugins[name], cfg=False), _oracle(c)
    rng = np.random.default_rng(2)
    for q, qd in _starts(c):
        s_o, xp_o, xq_o = o32.env_reset(q, qd)
        s_g, xp_g, xq_g = ctx.env_reset(_dev(q), _dev(qd))
        nqv = nq + nv
        atol = np.full(s_o.shape, 5e-4)
        atol[nqv:nqv + nv] = 5e-4 * max(1.0, float(np.abs(s_o[nqv:nqv + nv]).max()) * 1e-2)
        err = np.abs(s_g.cpu().numpy() - s_o)
        assert np.all(err <= atol + 2e-4 * np.abs(s_o)), float(err.max())
        assert np.allclose(xp_g.cpu().numpy(), xp_o, atol=1e-6) and np.allclose(xq_g.cpu().numpy(), xq_o, atol=1e-6)
        for _ in range(10):
            a = rng.uniform(-0.5, 0.5, model.nu).astype(np.float32)
            s_o, xp_o, xq_o, c_o = o32.env_step(s_o, a)
            s_g, xp_g, xq_g, c_g = ctx.env_step(s_g, _dev(a))
        sg = s_g.cpu().numpy()
        assert np.allclose(sg[:nq], s_o[:nq], atol=1e-3), float(np.abs(sg[:nq] - s_o[:nq]).max())
        assert np.allclose(c_g.cpu().numpy(), c_o, rtol=1e-3, atol=2e-2)
        assert sg[nq + 2 * nv + ISTEP] == 10.0
        assert sg[nq + 2 * nv + IU + 2] == 10.0          # the probe's step counter persisted across the ten env.steps


def _rows(c):
    """(field name, index) of every element of every reward input of the case's model."""
    m = c["model"]
    n = dict(qpos=m.nq, qvel=m.nv, xpos=3 * m.nbody, xquat=4 * m.nbody, spos=3 * m.nsite, cdist=m.ncon, cpos=3 * m.ncon,
             ctrl=m.nu, act=m.nu)
    rows = [(f, i) for f, k in n.items() for i in range(k)]
    rows += [(f, 0) for f in ("step", "dt", "nq", "nv", "nu", "nbody", "nsite", "ncon", "counter")]
    rows += [("xpos", 3 * m.nbody), ("cdist", m.ncon)]   # one past the end: the probe's guard, not a read out of bounds
    return rows


@pytest.mark.parametrize("name", ALL)
def test_reward_inputs_through_env_step(plugins, name):
    """b. Every element of every reward input, one env_step_batch per start state (one row per (field, index), the selector in the
    row's info_user[0:2]).  Against: the returned state (qpos, qvel: bit-equal), ctrl_out (bit-equal) and the oracle's ctrl, the
    action (bit-equal), the step counter / dt / dimensions (exact), the pre-integration forward quantities of Oracle.forward_dump
    (TOL_KIN / TOL_CON / TOL_SUB above; body 0 is the world: origin, identity rotation).  All rows run the same physics: their
    states are bit-identical apart from the selector."""
    c = _case(name)
    m = c["model"]
    nq, nv, nu, nb = m.nq, m.nv, m.nu, m.nbody
    info = nq + 2 * nv
    ctx, o32 = _ctx(c, plugins[name], cfg=False), _oracle(c)
    rows = _rows(c)
    R = len(rows)
    dt32 = np.float32(c["ptask"].dt)
    assert dt32 == np.float32(np.float32(m.timestep) * c["ptask"].n_frames)
    worst = {}
    rng = np.random.default_rng(11)
    for q, qd in _starts(c):
        s0, _, _ = ctx.env_reset(_dev(q), _dev(qd))
        s0 = s0.cpu().numpy()
        s0[info + ISTEP] = 5.0
        s0[info + IU + 2] = 3.0                                   # the probe's counter: 3 steps taken (it adds one)
        act = rng.uniform(-0.8, 0.8, nu).astype(np.float32)
        S = np.repeat(s0[None], R, 0)
        S[:, info + IU] = [F[f] for f, _ in rows]
        S[:, info + IU + 1] = [i for _, i in rows]
        out, xpos, xquat, ctrl = [t.cpu().numpy() for t in ctx.env_step_batch(_dev(S), _dev(np.repeat(act[None], R, 0)))]
        rew = out[:, info + IREW]
        # the selector persists, the counter advanced, slot 3 holds the value returned
        assert np.array_equal(out[:, info + IU:info + IU + 2], S[:, info + IU:info + IU + 2])
        assert np.all(out[:, info + IU + 2] == 4.0) and np.array_equal(out[:, info + IU + 3], rew)
        assert np.all(out[:, info + ISTEP] == 6.0)
        # same physics in every row
        assert np.array_equal(out[:, :info], np.repeat(out[:1, :info], R, 0))
        assert np.array_equal(xpos, np.repeat(xpos[:1], R, 0)) and np.array_equal(ctrl, np.repeat(ctrl[:1], R, 0))
        st, ct = out[0], ctrl[0]
        _, _, _, c_o = o32.env_step(s0, act)
        pre = _pre_state(c, o32, s0, act)
        ref = _fwd_ref(c, o32, pre)
        nf1 = c["otask"].n_frames == 1
        got = {}
        for r, (f, i) in enumerate(rows):
            got.setdefault(f, {})[i] = rew[r]
        arr = lambda f, n: np.array([got[f][i] for i in range(n)], np.float32)   # noqa: E731
        assert np.array_equal(arr("qpos", nq), st[:nq]) and np.array_equal(arr("qvel", nv), st[nq:nq + nv])
        assert np.array_equal(arr("ctrl", nu), ct) and np.array_equal(arr("act", nu), act)
        assert np.allclose(arr("ctrl", nu), c_o, rtol=1e-4, atol=1e-4), float(np.abs(arr("ctrl", nu) - c_o).max())
        worst["ctrl"] = max(worst.get("ctrl", 0.0), float(np.abs(arr("ctrl", nu) - c_o).max()))
        assert got["step"][0] == 5.0 and got["dt"][0] == dt32 and got["counter"][0] == 4.0
        for f, v in (("nq", nq), ("nv", nv), ("nu", nu), ("nbody", nb), ("nsite", m.nsite), ("ncon", m.ncon)):
            assert got[f][0] == v, f
        assert got["xpos"][3 * nb] == PROBE_BAD and got["cdist"][m.ncon] == PROBE_BAD
        xp, xq = arr("xpos", 3 * nb).reshape(nb, 3), arr("xquat", 4 * nb).reshape(nb, 4)
        assert np.all(xp[0] == 0.0) and np.array_equal(xq[0], np.float32([1, 0, 0, 0])), "body 0 is the world"
        # env.step's own xpos / xquat outputs (bodies 1 ..) are the same pre-integration quantities, bit for bit
        assert np.array_equal(xp[1:], xpos[0]) and np.array_equal(xq[1:], xquat[0])
        _check_parked(c, arr("cdist", m.ncon), arr("cpos", 3 * m.ncon).reshape(-1, 3), ref, TOL_CON if nf1 else TOL_SUB, worst)
        for f, n, tol in (("xpos", 3 * nb, TOL_KIN), ("xquat", 4 * nb, TOL_KIN), ("spos", 3 * m.nsite, TOL_KIN)):
            tol = tol if nf1 else TOL_SUB
            g = arr(f, n)
            if f == "xquat":   # (q and -q are the same rotation; both sides normalise the same way, but compare up to sign)
                g4, r4 = g.reshape(-1, 4), ref[f].reshape(-1, 4)
                sgn = np.where(np.sum(g4 * r4, 1) < 0, -1.0, 1.0)[:, None]
                e = np.abs(g4 - sgn * r4).ravel()
            else:
                e = np.abs(g.astype(np.float64) - ref[f])
            worst[f] = max(worst.get(f, 0.0), float(e.max()) if e.size else 0.0)
            assert e.size == 0 or e.max() <= tol, (f, int(np.argmax(e)), float(e.max()))
    if name in CRATES:   # (the trunk / torso over the floor: its plane-box slots are parked in these poses)
        assert worst.get("parked plane-box", 0) > 0 and worst["parked slots"] > worst["parked plane-box"], worst
    print(f"{name}: worst |reward input - oracle| " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def _park_dist():
    import os
    import re
    from dial_mpc_amd._lib import _CSRC
    return float(re.search(r"#define\s+DIAL_BOX_PARK_DIST\s+([0-9.]+)f", open(os.path.join(_CSRC, "box_collide.h")).read()).group(1))


PARK = _park_dist()   # box_collide.h: DIAL_BOX_PARK_DIST (1 cm)


def _rotate(q, v):
    w, x, y, z = q
    u = np.array([x, y, z])
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def _geom_centres(c, ref):
    """World centre of every geom from the oracle's body frames: xpos[b] + R(xquat[b]) geom_pos[g]."""
    md = c["md"]
    xp, xq = ref["xpos"].reshape(-1, 3).astype(np.float64), ref["xquat"].reshape(-1, 4).astype(np.float64)
    bid, gp = np.asarray(md["geom_bodyid"]).ravel(), np.asarray(md["geom_pos"], np.float64).reshape(-1, 3)
    return np.array([xp[b] + _rotate(xq[b], gp[g]) for g, b in enumerate(bid)])


def _check_parked(c, cdist, cpos, ref, tol, worst):
    """cdist / cpos per contact slot against the oracle, with the documented convention of the box narrow phases (user_reward.h):
    a plane-box, capsule-box or box-box candidate whose broad phase puts it more than DIAL_BOX_PARK_DIST (1 cm) from touching is
    PARKED -- cdist is above 1 cm and either a lower bound of the distance (the broad phase's gap) or 1.0; cpos is the box's centre
    (plane-box) or the midpoint of the two geoms' centres (capsule-box, box-box), checked against the oracle's geom frames.
    Every other slot (sphere / capsule candidates, box candidates within 1 cm) equals the oracle's narrow phase within `tol`; a box
    slot farther than 1 cm either equals it too (its broad phase did not park it) or follows the parked rule."""
    from dial_mpc_amd import _abi
    K = _abi.MACROS
    md = c["md"]
    kind = np.asarray(md["con_kind"]).ravel()
    g1, g2 = np.asarray(md["con_geom1"]).ravel(), np.asarray(md["con_geom2"]).ravel()
    rd, rp = ref["cdist"], ref["cpos"].reshape(-1, 3)
    gc = _geom_centres(c, ref) if len(kind) else None
    boxy = np.isin(kind, [K["DIAL_CON_PLANE_BOX"], K["DIAL_CON_CAPSULE_BOX"], K["DIAL_CON_BOX_BOX"]])
    exact = ~boxy | (rd <= PARK)
    parked = 0
    for i in np.flatnonzero(~exact):   # (oracle: more than 1 cm apart)
        if abs(cdist[i] - rd[i]) <= tol and np.abs(cpos[i] - rp[i]).max() <= tol:
            continue                   # the narrow phase ran
        parked += 1
        if kind[i] == K["DIAL_CON_PLANE_BOX"]:
            worst["parked plane-box"] = worst.get("parked plane-box", 0) + 1
        assert cdist[i] > PARK, ("parked slot reads as touching", i, float(cdist[i]), float(rd[i]))
        assert cdist[i] == 1.0 or cdist[i] <= rd[i] + tol, ("parked cdist", i, float(cdist[i]), float(rd[i]))
        want = gc[g2[i]] if kind[i] == K["DIAL_CON_PLANE_BOX"] else 0.5 * (gc[g1[i]] + gc[g2[i]])
        e = float(np.abs(cpos[i] - want).max())
        worst["parked cpos"] = max(worst.get("parked cpos", 0.0), e)
        assert e <= tol, ("parked cpos", i, int(kind[i]), cpos[i].tolist(), want.tolist())
    worst["parked slots"] = worst.get("parked slots", 0) + parked
    ed = np.abs(cdist[exact].astype(np.float64) - rd[exact])
    ep = np.abs(cpos[exact].astype(np.float64) - rp[exact])
    worst["cdist"] = max(worst.get("cdist", 0.0), float(ed.max()) if ed.size else 0.0)
    worst["cpos"] = max(worst.get("cpos", 0.0), float(ep.max()) if ep.size else 0.0)
    assert ed.size == 0 or ed.max() <= tol, ("cdist", int(np.flatnonzero(exact)[np.argmax(ed)]), float(ed.max()))
    assert ep.size == 0 or ep.max() <= tol, ("cpos", float(ep.max()))
    return parked


SELECTIONS = ("qvel0", "trunk_z", "cdist", "ctrl0", "step", "counter")


def _selection(c, what):
    m = c["model"]
    if what == "qvel0":
        return F["qvel"], 0
    if what == "trunk_z":
        return F["xpos"], 3 * 1 + 2
    if what == "cdist":
        return (F["cdist"], 0) if m.ncon else (F["ncon"], 0)
    if what == "ctrl0":
        return F["ctrl"], 0
    return F[what], 0


@pytest.mark.parametrize("name", ALL)
def test_reward_inputs_through_rollouts_and_physics(plugins, name):
    """c. ctx.rollout (16 rollouts, H = 12) with the probe selecting in turn qvel[0], the trunk's height, a cdist slot, ctrl[0], the
    step and the info_user counter: every per-step reward against the rollout's own per-step outputs (post-integration: bit-equal),
    Oracle.forward_dump of the pre-integration state (taken from the state trace of the same launch: TOL_KIN / TOL_CON / TOL_SUB),
    an oracle env.step restarted at that state (ctrl) and t (step) / t + 1 (counter).  The post-integration, step and counter checks
    cover all 16 rollouts; the references rebuilt on the CPU (trunk height, cdist, ctrl) cover every step of every third rollout
    (0, 3, ..., 15: 6 of 16), which keeps the oracle's share of the test's time small.  The state trace equals qss / qdss bit for bit,
    and the probe's selection leaves the physics bit-identical.
    e. Physics against the fp32 oracle per rollout (DIAL_LS_SWAP, test_gpu_custom_env._physics_gate: q / qd / x at every step)."""
    c = _case(name)
    m, cfg = c["model"], c["cfg"]
    nq, nv, nu = m.nq, m.nv, m.nu
    info = nq + 2 * nv
    T = cfg.Hsample + 1
    o32 = _oracle(c)
    ctx, ctxt = _ctx(c, plugins[name]), _ctx(c, plugins[name])
    trace = ctxt.set_state_trace(16)
    q, qd = perturbed_state(c["env"], 5)
    s0, _, _ = o32.env_reset(q, qd)
    us = np.random.default_rng(9).uniform(-0.8, 0.8, (16, T, nu)).astype(np.float32)
    ref = o32.rollout(s0, us)
    nf1 = c["otask"].n_frames == 1
    first = None
    worst = {}
    for what in SELECTIONS:
        ctx.set_user_params(_selection(c, what))
        got = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
        rewss, qss, qdss, xss = got
        if first is None:   # the state-trace launch: the same rollouts, and its trace rows are their states
            ctxt.set_user_params(_selection(c, what))
            for a, b in zip(got, [t.cpu().numpy() for t in ctxt.rollout(_dev(s0), _dev(us))]):
                assert np.array_equal(a, b)
            tr = trace.cpu().numpy()
            assert np.array_equal(tr[:, :, :nq], qss) and np.array_equal(tr[:, :, nq:nq + nv], qdss)
            first = got
            _physics_gate(got[1:], ref[1:], 16, T, max_diverged=1)
        else:
            for a, b in zip(first[1:], got[1:]):
                assert np.array_equal(a, b), what
        if what == "qvel0":
            assert np.array_equal(rewss, qdss[:, :, 0])
        elif what == "step":
            assert np.array_equal(rewss, np.broadcast_to(np.arange(T, dtype=np.float32), (16, T)))
        elif what == "counter":
            assert np.array_equal(rewss, np.broadcast_to(np.arange(1, T + 1, dtype=np.float32), (16, T)))
            assert np.all(tr[:, :, info + IU + 2] == np.arange(1, T + 1))
        elif what == "cdist" and not m.ncon:
            assert np.all(rewss == 0.0)
        else:
            e = 0.0
            field, idx = _selection(c, what)
            for n in range(0, 16, 3):
                for t in range(T):
                    start = s0 if t == 0 else tr[n, t - 1]
                    if what == "ctrl0":
                        want = o32.env_step(start, us[n, t])[3][0]
                        tol = 1e-4 + 1e-4 * abs(want)
                    else:
                        r = _fwd_ref(c, o32, _pre_state(c, o32, start, us[n, t]))
                        want = (r["xpos"] if field == F["xpos"] else r["cdist"])[idx]
                        tol = (TOL_KIN if field == F["xpos"] else TOL_CON) if nf1 else TOL_SUB
                    e = max(e, abs(float(rewss[n, t]) - float(want)))
                    assert abs(float(rewss[n, t]) - float(want)) <= tol, (what, n, t, float(rewss[n, t]), float(want))
            worst[what] = e
    print(f"{name}: worst |rollout reward - reference| " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("name", ALL)
def test_reverse_once_softmax(plugins, name):
    """d (per model). reverse_once: weights and Ybar against an fp64 host softmax of the device's own rewards (probe: qvel[0])."""
    import torch
    c = _case(name)
    dc, cfg = c["dc"], c["cfg"]
    nu = c["model"].nu
    ctx = _ctx(c, plugins[name], params=(F["qvel"], 0))
    s0, _, _ = ctx.env_reset(_dev(c["env"]._init_q), _dev(np.zeros(c["model"].nv)))
    eps, sigma, Ybar = seeded_inputs(dc, nu, seed=1, Ybar_scale=0.2)
    out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
    torch.cuda.synchronize()
    sc = ctx.debug_scratch()
    rews = out["rews"].cpu().numpy().astype(np.float64)
    assert np.allclose(sc["rewss"].astype(np.float64).mean(1), rews, rtol=1e-5, atol=1e-6)
    logp = (rews - rews[-1]) / rews.std() / cfg.temp_sample
    w = np.exp(logp - logp.max())
    w /= w.sum()
    assert np.allclose(sc["weights"][: len(w)], w, rtol=1e-3, atol=1e-6)
    Yw = np.einsum("n,nij->ij", w, sc["Y0s"].astype(np.float64)[: len(w)])
    assert np.allclose(out["Ybar"].cpu().numpy(), Yw, rtol=1e-4, atol=1e-5)


def _plan(ctx, s0, ins, iters=1):
    """`iters` consecutive reverse_once calls (Ybar fed back): per iteration the outputs and the scratch the contract compares."""
    import torch
    eps, sigma, Ybar = ins
    res = []
    for _ in range(iters):
        out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
        torch.cuda.synchronize()
        ctx.status()
        sc = ctx.debug_scratch()
        r = {k: out[k].cpu().numpy().copy() for k in ("Ybar", "rews", "qbar", "qdbar", "xbar")}
        r.update({k: np.array(sc[k]) for k in ("rewss", "qss", "qdss", "xss", "Y0s", "weights")})
        res.append(r)
        Ybar = r["Ybar"]
    return res


def _same(a, b, what):
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k], y[k], equal_nan=True), (what, k)   # (the counter probe: equal rewards, NaN weights)


# (probe, consecutive iterations): the counter gives every sample the same reward, so its softmax weights and Ybar are NaN (equal_nan
# in _same) -- one iteration compares its rewards and states; a second would plan from NaN controls
PROBES = (("cdist", 0, 3), ("counter", 0, 1))


def _start(c, ctx):
    s0, _, _ = ctx.env_reset(_dev(c["env"]._init_q), _dev(np.zeros(c["model"].nv)))
    return s0


@pytest.mark.parametrize("name", ["go2_crate", "h1_push_crate"])
def test_launch_paths_relay_and_con_cap(plugins, name):
    """d. Mean-trajectory relay (relay_always=1) vs no_relay=1, and con_cap=1 (every touching step on the overflow area) vs the
    default cap, with the probe reading a cdist slot (3 consecutive iterations) and the info_user counter (one iteration, see
    PROBES): bit-identical rewards, qss, qdss, xss, Ybar and weights."""
    c = load_case(name, N=64, H=H)
    ins = seeded_inputs(c["dc"], c["model"].nu, seed=4, Ybar_scale=0.2)
    for field, idx, iters in PROBES:
        p = (F[field], idx)
        ref = _plan(_ctx(c, plugins[name], params=p, no_relay=1), _start(c, _ctx(c, plugins[name])), ins, iters=iters)
        ctx = _ctx(c, plugins[name], params=p, relay_always=1)
        _same(_plan(ctx, _start(c, ctx), ins, iters=iters), ref, ("relay", field))
        ctx = _ctx(c, plugins[name], params=p, con_cap=1)
        _same(_plan(ctx, _start(c, ctx), ins, iters=iters), ref, ("con_cap", field))


def test_launch_paths_overflow_under_the_relay(plugins):
    """d. Go2 crate climb plugin at a relay-sized N = 1024 (relay_always: the grid holds N + pieces wavefronts, each with an overflow
    area): con_cap = 1 == the default cap, bit for bit."""
    N = 1024
    c = load_case("go2_crate", N=N, H=H)
    ins = seeded_inputs(c["dc"], c["model"].nu, seed=5, Ybar_scale=0.2)
    p = (F["cdist"], 20)
    outs = []
    for cap in (0, 1):
        ctx = _ctx(c, plugins["go2_crate"], params=p, con_cap=cap, relay_always=1)
        assert ctx.lib.dial_debug_resident_rollouts(ctx.h, N + 1) >= N + 1 + H + 1      # everything resident: the relay runs
        outs.append(_plan(ctx, _start(c, ctx), ins))
        del ctx
    assert np.all(np.isfinite(outs[0][0]["rews"]))
    _same(outs[0], outs[1], "con_cap at N=1024")


def test_launch_paths_queue_and_trace(plugins):
    """d. The rollout queue (N beyond the resident rollouts) vs no_queue=1, and the state trace against qss / qdss, on the Go2 plugin."""
    from dial_mpc_amd import _lib
    c0 = load_case("go2", N=64, H=H)
    probe = _lib.Context(c0["model"], c0["ptask"], c0["cfg"], plugin=plugins["go2"])
    slots = probe.lib.dial_debug_resident_rollouts(probe.h, 10 ** 6)
    del probe
    N = slots + slots // 2
    c = load_case("go2", N=N, H=H)
    ins = seeded_inputs(c["dc"], c["model"].nu, seed=6, Ybar_scale=0.2)
    for field, idx, _ in PROBES:
        p = (F[field], idx) if field != "cdist" else (F["cdist"], 1)
        ctx = _ctx(c, plugins["go2"], params=p)
        assert 0 < ctx.lib.dial_debug_resident_rollouts(ctx.h, N + 1) < N + 1
        q = _plan(ctx, _start(c, ctx), ins)
        ctx1 = _ctx(c, plugins["go2"], params=p, no_queue=1)
        assert ctx1.lib.dial_debug_resident_rollouts(ctx1.h, N + 1) == 0
        _same(q, _plan(ctx1, _start(c, ctx1), ins), ("queue", field))
        trace = ctx.set_state_trace(N + 1)   # (a traced launch takes neither the queue nor the spread grid)
        qt = _plan(ctx, _start(c, ctx), ins)
        _same(q, qt, ("trace", field))
        tr = trace.cpu().numpy()
        nq, nv = c["model"].nq, c["model"].nv
        assert np.array_equal(tr[:, :, :nq], qt[0]["qss"]) and np.array_equal(tr[:, :, nq:nq + nv], qt[0]["qdss"])


def _scratch_rows(ctx, rows):
    """Host copies of the rollout scratch of the last launch with `rows` rollouts (grouped launches: plan g's rows [g B, (g + 1) B))."""
    import ctypes
    import torch
    ptrs = [ctypes.c_void_p() for _ in range(6)]
    assert ctx.lib.dial_debug_scratch(ctx.h, *[ctypes.byref(p) for p in ptrs]) == 0
    T = ctx.cfg.Hsample + 1
    shapes = dict(rewss=(rows, T), qss=(rows, T, ctx.nq), qdss=(rows, T, ctx.nv), xss=(rows, T, ctx.nx), weights=(rows,))
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    out = {}
    for (k, shp), p in zip(shapes.items(), ptrs[1:]):
        host = np.empty(shp, np.float32)
        assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), p, ctypes.c_size_t(host.nbytes), ctypes.c_int(2)) == 0, k
        out[k] = host
    return out


def test_grouped_plans_on_push_crate(plugins):
    """d. M = 3 grouped plans (reverse_once_batch) from three different start states (keyframe, two perturbed states) on the H1
    push-crate plugin == three single plans, bit for bit: rewards, per-step rewards, qss, qdss, xss, weights, Ybar and the mean
    trajectory's states."""
    import torch
    N, M = 64, 3
    c = load_case("h1_push_crate", N=N, H=H)
    nu, nv = c["model"].nu, c["model"].nv
    starts = [(c["env"]._init_q, np.zeros(nv))] + [perturbed_state(c["env"], s) for s in range(M - 1)]
    outs = ("Ybar", "rews", "qbar", "qdbar", "xbar")
    for field, idx, _ in PROBES:
        ctx = _ctx(c, plugins["h1_push_crate"], params=(F[field], idx), plan_cap=M)
        S = [ctx.env_reset(_dev(q), _dev(qd))[0] for q, qd in starts]
        ins = [seeded_inputs(c["dc"], nu, seed=k, Ybar_scale=0.2) for k in range(M)]
        singles = []
        for s0, (eps, sigma, Ybar) in zip(S, ins):
            out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
            torch.cuda.synchronize()
            one = {k: out[k].cpu().numpy().copy() for k in outs}
            one.update(_scratch_rows(ctx, N + 1))
            singles.append(one)
        assert not np.array_equal(singles[0]["qss"], singles[1]["qss"])   # (the plans really start apart)
        outb = ctx.reverse_once_batch(torch.stack(S).contiguous(), _dev(np.stack([i[2] for i in ins])),
                                      _dev(np.stack([i[1] for i in ins])), _dev(np.stack([i[0] for i in ins])))
        torch.cuda.synchronize()
        sc = _scratch_rows(ctx, M * (N + 1))
        for g in range(M):
            for k in outs:
                assert np.array_equal(outb[k][g].cpu().numpy(), singles[g][k], equal_nan=True), (field, g, k)
            for k, v in sc.items():
                assert np.array_equal(v[g * (N + 1):(g + 1) * (N + 1)], singles[g][k], equal_nan=True), (field, g, k)


@pytest.mark.parametrize("name", ["go2", "h1_push_crate"])
def test_physics_gate_catches_a_one_percent_mass_error(plugins, name):
    """e. Power check of the physics gate: the plugin context gets the model with body 1's mass 1 % off (same dimensions, same
    plugin), the oracle keeps the original.  The gate of the plugin tests (at most 1 of 16 rollouts outside conftest.TOL) must fail."""
    c = _case(name)
    m, cfg = c["model"], c["cfg"]
    bad = type(m).from_buffer_copy(m)
    bad.body_mass[1] = m.body_mass[1] * 1.01
    from dial_mpc_amd import _lib
    ctx = _lib.Context(bad, c["ptask"], cfg, plugin=plugins[name], user_params=[F["qvel"], 0])
    o32 = _oracle(c)
    T = cfg.Hsample + 1
    s0, _, _ = o32.env_reset(*perturbed_state(c["env"], 5))
    us = np.random.default_rng(9).uniform(-0.8, 0.8, (16, T, m.nu)).astype(np.float32)
    got = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
    ref = o32.rollout(s0, us)
    ok = np.ones((16, T), bool)
    for k, g, r in zip(("q", "qd", "x"), got[1:], ref[1:]):
        w = _within(g, r, TOL[k])
        ok &= w if w.ndim == 2 else w.reshape(16, T, -1).all(-1)
    print(f"{name}: 1 % mass error -> {int((~ok.all(1)).sum())} of 16 rollouts outside the gate, first at step "
          f"{int(np.argmax(~ok.all(0))) if (~ok).any() else -1}")
    with pytest.raises(AssertionError):
        _physics_gate(got[1:], ref[1:], 16, T, max_diverged=1)
