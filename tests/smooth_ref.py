"""Contact-free states, fp64 / fp32 references and THE tolerance rule of the rounding-level gates (tests/test_smooth_ref.py,
tests/test_smooth_emu.py on the CPU, tests/test_gpu_smooth.py on the device).

The regime: a robot in the air.  No contact inside its margin, so the solve is qacc = qacc_smooth (class F), or only limit rows
active under DIAL_LS_SWAP (class L): one step is a smooth function of the state, the rewards read smooth forward quantities, and
the answer is unique.  No witnesses, no jitter, no case left out: a block's tolerance is 8 x what the fp32 oracle itself differs
from the fp64 oracle on the same fp32 inputs (`tolerance` below, the only place a tolerance comes from).
"""
import functools

import numpy as np

import oracle as O
from conftest import setup_case
from dial_mpc_amd import _abi

EXAMPLES = ("unitree_go2_trot", "unitree_go2_seq_jump", "unitree_h1_jog", "unitree_h1_loco", "allegro_reorient",
            "unitree_go2_crate_climb", "unitree_h1_push_crate")
PYRAMIDAL = tuple(e for e in EXAMPLES if e != "allegro_reorient")       # class L: pyramidal models only
LEGGED = PYRAMIDAL
FREE, SLIDE, HINGE = (_abi.MACROS[k] for k in ("DIAL_JNT_FREE", "DIAL_JNT_SLIDE", "DIAL_JNT_HINGE"))
CLEAR = 0.01          # a candidate contact stays this far outside its margin, an unpushed limited joint this far inside its range
INTERIOR = 0.15       # limited joints are drawn inside [lo + 0.15 w, hi - 0.15 w]
FACTOR = 8.0          # the margin of tests/lane_ref.py, for the same reasons: the product build contracts, uses -freciprocal-math and v_sin_f32 / v_cos_f32
FLOOR_ULP = 4.0
US_SCALE = 0.3        # rollouts: us uniform in +- 0.3


@functools.lru_cache(maxsize=None)
def case(example, N=15, H=4):
    """(dial_config, env, model under DIAL_LS_SWAP where pyramidal, task, cfg), cached: N + 1 = 16 rollouts of H + 1 = 5 env steps."""
    return setup_case(example, N, H, per_rollout=True)


@functools.lru_cache(maxsize=None)
def oracles(example):
    _, _, model, task, cfg = case(example)
    return O.Oracle(model, task, cfg, np.float64), O.Oracle(model, task, cfg, np.float32)


def joints(model):
    """[(type, qpos address, dof address, limited, lo, hi)] of the model's joints."""
    return [(int(model.jnt_type[j]), int(model.jnt_qposadr[j]), int(model.jnt_dofadr[j]), bool(model.jnt_limited[j]),
             float(model.jnt_range[j][0]), float(model.jnt_range[j][1])) for j in range(model.njnt)]


def base_dofs(model):
    """Mask [nv]: dofs of free joints (the 'base qvel' quantity); the others are 'joint qvel'."""
    mask = np.zeros(model.nv, bool)
    for typ, _, da, _, _, _ in joints(model):
        if typ == FREE:
            mask[da:da + 6] = True
    return mask


def quat_entries(model):
    """Mask [nq]: the quaternions of free joints.  Kinematics normalises them in place (the oracle and the kernels do, as MJX does), so
    they are the only entries of qpos that a reset or a plant's trace may return changed, by an ulp or two."""
    mask = np.zeros(model.nq, bool)
    for typ, qa, _, _, _, _ in joints(model):
        if typ == FREE:
            mask[qa + 3:qa + 7] = True
    return mask


def _keyframe_pose(model):
    """The Allegro hand (elliptic cones) and the push crate (the model with a dry-friction row) perturb the keyframe's joint angles:
    arbitrary finger poses self-collide (62 of 64 draws), and the H1 next to the crate has to stay clear of it."""
    return model.cone == _abi.MACROS["DIAL_CONE_ELLIPTIC"] or model.nfri > 0


def classify(model, o64, qpos, qvel, ctrl=None, warm=None, pushed=()):
    """The fp64 oracle's verdict on one state: None when it is in the class (F when `pushed` is empty, else L with exactly the joints
    `pushed` beyond a limit), otherwise the reason as text."""
    d = o64.forward_dump(qpos, qvel, ctrl, warm)
    margin = _abi.as_numpy(model, "con_margin")[:model.ncon].astype(np.float64)
    if model.ncon and not np.all(d["con_dist"] > margin + CLEAR):
        c = int(np.argmin(d["con_dist"] - margin))
        return f"contact {c}: dist {d['con_dist'][c]:.4f} within margin {margin[c]:.4f} + {CLEAR}"
    q = np.asarray(qpos, np.float64)
    for r in range(model.nlim):
        j = int(model.lim_jnt[r])
        inside = min(q[model.jnt_qposadr[j]] - model.jnt_range[j][0], model.jnt_range[j][1] - q[model.jnt_qposadr[j]]) - model.jnt_margin[j]
        if j in pushed:
            if d["efc_force"][r] == 0:
                return f"pushed joint {j}: its limit row carries no force"
        elif d["efc_force"][r] != 0 or inside < CLEAR:
            return f"joint {j}: {inside:.4f} inside its range, limit-row force {d['efc_force'][r]:.3g}"
    return None


def smooth_states(env, model, cls, count, seed):
    """`count` states (qpos [count, nq], qvel [count, nv], float32) of class "F" (free flight) or "L" (free flight with limited
    actuated joints 0.02 - 0.1 rad beyond a limit), drawn deterministically from `seed` and selected with the fp64 oracle alone,
    from at most 4 x count draws (asserted).  Also returns, per state, the set of pushed joints (empty in class F)."""
    assert cls in ("F", "L")
    assert cls == "F" or model.cone == _abi.MACROS["DIAL_CONE_PYRAMIDAL"], "class L: pyramidal models only"
    rng = np.random.default_rng(seed)
    o64 = O.Oracle(model, env.make_task(), None, np.float64)
    q0 = np.asarray(env._init_q, np.float64)
    keyframe, hand = _keyframe_pose(model), model.cone == _abi.MACROS["DIAL_CONE_ELLIPTIC"]
    jn = joints(model)
    by_qadr = {qa: j for j, (_, qa, _, _, _, _) in enumerate(jn)}
    qs, vs, pushes, draws, reasons = [], [], [], 0, []
    while len(qs) < count:
        assert draws < 4 * count, f"{count} class-{cls} states need more than {4 * count} draws; rejected: {reasons[-5:]}"
        draws += 1
        q, v, k_free = q0.copy(), np.zeros(model.nv), 0
        for typ, qa, da, limited, lo, hi in jn:
            if typ == FREE:
                q[qa + 2] += 1.0 + 2.0 * k_free          # the k-th free joint is lifted by 1 + 2 k m
                k_free += 1
                quat = rng.standard_normal(4)
                q[qa + 3:qa + 7] = quat / np.linalg.norm(quat)
                v[da:da + 3] = rng.uniform(-1, 1, 3) * (3.0 if hand else 1.0)
                v[da + 3:da + 6] = rng.uniform(-1, 1, 3) * 3.0
            elif typ in (SLIDE, HINGE):
                if limited:
                    a, b = lo + INTERIOR * (hi - lo), hi - INTERIOR * (hi - lo)
                    q[qa] = np.clip(q0[qa] + rng.uniform(-0.15, 0.15), a, b) if keyframe else rng.uniform(a, b)
                v[da] = rng.uniform(-1, 1) * (3.0 if hand else 5.0)
        pushed = set()
        if cls == "L":
            for a in range(model.nu):
                typ, qa, da, limited, lo, hi = jn[by_qadr[int(model.act_qposadr[a])]]
                push, side, depth = rng.random() < 0.4, rng.integers(2), rng.uniform(0.02, 0.1)
                if limited and push:
                    q[qa] = lo - depth if side == 0 else hi + depth
                    # A pushed joint keeps moving OUTWARD (its drawn speed, the sign of the push).  Moving inward, the damping term of
                    # the row's reference acceleration outweighs the position term above ~25 |pos| rad/s and the row carries no force:
                    # measured, fp64 oracle: only 15 - 47 % of such rows carry force (Go2, H1 jog; time steps 0.005 and 0.02), so that a
                    # state with its ~5 pushed joints would be accepted in under 5 % of the draws and the bound of 4 x count draws
                    # could not hold.  Moving outward: 98 - 100 %.
                    v[da] = -abs(v[da]) if side == 0 else abs(v[da])
                    pushed.add(by_qadr[qa])
        q32, v32 = q.astype(np.float32), v.astype(np.float32)
        why = classify(model, o64, q32, v32, pushed=pushed)
        if why is None:
            qs.append(q32), vs.append(v32), pushes.append(pushed)
        else:
            reasons.append(why)
    return np.array(qs), np.array(vs), pushes


def rollout_us(model, count, B, T, seed, scale=US_SCALE):
    """[count, B, T, nu] float32 controls, uniform in +- scale."""
    return np.random.default_rng(seed).uniform(-scale, scale, (count, B, T, model.nu)).astype(np.float32)


def hold_action(model, task, qpos):
    """The action whose act2joint target is the state's own actuated joint angles, [..., nu]."""
    nu = model.nu
    lo, hi = (np.array([task.joint_range[a][k] for a in range(nu)], np.float64) for k in (0, 1))
    off = np.array([task.joint_offset[a] for a in range(nu)], np.float64)
    adr = [int(model.act_qposadr[a]) for a in range(nu)]
    return (np.asarray(qpos, np.float64)[..., adr] - off - (lo + hi) / 2) / ((hi - lo) / 2) / task.action_scale


@functools.lru_cache(maxsize=None)
def rollout_cases(example, count=4, B=16, seed=11):
    """`count` class-F start states (qpos, qvel) of `example` with controls us [count, B, T, nu] whose B fp64 trajectories each stay
    in class F at every physics step: the first `count` such among 4 x count states of `smooth_states`, selected with the fp64
    oracle alone (asserted to suffice).  us is uniform in +- 0.3; for the Allegro hand, whose keyframe leaves ~1 cm between neighbouring
    finger geoms, +- 0.1 around the action that holds the start pose (a position actuator pulled towards mid-range closes those gaps
    within two control steps whatever the noise)."""
    _, env, model, task, cfg = case(example)
    o64, _ = oracles(example)
    return rollout_cases_for(example, env, model, task, cfg, o64, count, B, seed)


def rollout_cases_for(example, env, model, task, cfg, o64, count=4, B=16, seed=11):
    """rollout_cases for any (env, model, task, cfg) with its fp64 oracle -- a model that is no shipped example (`example` only
    names it in messages)."""
    T = cfg.Hsample + 1
    q, v, _ = smooth_states(env, model, "F", 4 * count, seed)
    hand = model.cone == _abi.MACROS["DIAL_CONE_ELLIPTIC"]
    us = rollout_us(model, 4 * count, B, T, seed + 1, scale=0.1 if hand else US_SCALE)
    if hand:
        us = (hold_action(model, task, q)[:, None, None, :] + us).astype(np.float32)
    keep = []
    for i in range(4 * count):
        try:
            assert_stays_free(model, task, o64, o64.env_reset(q[i], v[i])[0], us[i])
        except AssertionError:
            continue
        keep.append(i)
        if len(keep) == count:
            break
    assert len(keep) == count, f"{example}: {len(keep)} of {4 * count} states keep all {B} rollouts in class F; {count} are needed"
    return q[keep], v[keep], us[keep]


def substep_oracle(model, task):
    """An fp64 oracle that advances ONE physics step with a given ctrl (position_control with the identity action map up to the
    factor R): what walks through the physics sub-steps inside one env.step."""
    R = 4096.0
    t = type(task).from_buffer_copy(task)
    t.n_frames, t.dt, t.position_control, t.action_scale = 1, model.timestep, 1, 1.0
    for a in range(model.nu):
        t.joint_offset[a] = 0.0
        t.joint_range[a][0], t.joint_range[a][1] = -R, R
        t.phys_range[a][0], t.phys_range[a][1] = -R, R
    return O.Oracle(model, t, None, np.float64), R


def assert_stays_free(model, task, o64, state, us):
    """Every physics step of the fp64 trajectories of `us` [B, T, nu] from the packed `state` starts in class F, and so does the
    state each of them ends in."""
    nq, nv = model.nq, model.nv
    osub, R = substep_oracle(model, task)
    for b in range(us.shape[0]):
        st = np.asarray(state, np.float64)
        for t in range(us.shape[1]):
            st2, _, _, ctrl = o64.env_step(st, us[b, t])
            sub = st.copy()
            for f in range(task.n_frames):
                why = classify(model, o64, sub[:nq], sub[nq:nq + nv], ctrl, sub[nq + nv:nq + 2 * nv])
                assert why is None, f"rollout {b}, step {t}, sub-step {f} leaves class F: {why}"
                sub = osub.env_step(sub, ctrl / R)[0]
            assert np.allclose(sub[:nq + nv], st2[:nq + nv], rtol=0, atol=1e-9), (b, t)
            st = st2
        why = classify(model, o64, st[:nq], st[nq:nq + nv])
        assert why is None, f"rollout {b} ends outside class F: {why}"


# ------------------------------------------------------------------------------------------------------------------ the tolerance rule
def tolerance(ref64, ref32, qpos=False, extra=0.0):
    """The tolerance of one block -- one (example, class, gate, quantity, step index) with all its cases:
    max(8 x worst |fp32 oracle - fp64 oracle|, 4 ulp (fp32) of the largest reference magnitude; qpos: of max(1, |q|)) + extra.
    `extra` is an additive term of a documented approximation of the product build (none is in use: see DESIGN.md section 2)."""
    ref64, ref32 = np.asarray(ref64, np.float64), np.asarray(ref32, np.float64)
    mag = float(np.max(np.abs(ref64)))
    if qpos:
        mag = max(1.0, mag)
    floor = FLOOR_ULP * float(np.spacing(np.float32(mag)))
    return max(FACTOR * float(np.max(np.abs(ref32 - ref64))), floor) + extra


class Gate:
    """The blocks of one test: `block` prints worst error, tolerance and ratio, `check` asserts that no block is above 1."""

    def __init__(self, example, cls, gate, build):
        self.key, self.rows = (example, cls, gate, build), []

    def block(self, quantity, step, got, ref64, ref32, qpos=False, extra=0.0):
        got = np.asarray(got, np.float64)
        assert got.shape == np.asarray(ref64).shape == np.asarray(ref32).shape, (quantity, got.shape, np.shape(ref64), np.shape(ref32))
        tol = tolerance(ref64, ref32, qpos=qpos, extra=extra)
        err = float(np.max(np.abs(got - np.asarray(ref64, np.float64))))
        ratio = err / tol if np.isfinite(err) else float("inf")
        self.rows.append((quantity, step, err, tol, ratio))
        print("SMOOTH %s %s %s %s | %-10s step %s | err %.3e tol %.3e ratio %.3f" % (*self.key, quantity, step, err, tol, ratio))
        return ratio

    def state_blocks(self, model, step, q, qd, ref64, ref32):
        """qpos / base qvel / joint qvel blocks of [cases, nq] and [cases, nv] arrays; ref = (q, qd)."""
        base = base_dofs(model)
        self.block("qpos", step, q, ref64[0], ref32[0], qpos=True)
        assert bool(base.any()) == any(int(model.jnt_type[j]) == FREE for j in range(model.njnt)), "base_dofs missed a free joint"
        if base.any():   # (a model without a free joint has no base block)
            self.block("base_qvel", step, qd[..., base], ref64[1][..., base], ref32[1][..., base])
        if (~base).any():
            self.block("joint_qvel", step, qd[..., ~base], ref64[1][..., ~base], ref32[1][..., ~base])

    def reset_blocks(self, model, o64, o32, qpos, qvel, states):
        """The reset gate on packed `states` [n, nstate] returned for (qpos, qvel): qvel and qpos bit-equal to the inputs but for the
        free joints' quaternions, which are normalised in place; those (in the qpos block) and qacc_warmstart -- qacc_smooth, here --
        against the fp64 oracle's reset under the rule."""
        nq, nv, quat = model.nq, model.nv, quat_entries(model)
        states = np.asarray(states)
        assert np.array_equal(states[:, nq:nq + nv], qvel), "reset: qvel is not the input, bit for bit"
        assert np.array_equal(states[:, :nq][:, ~quat], np.asarray(qpos)[:, ~quat]), "reset: qpos is not the input, bit for bit"
        s64 = np.array([o64.env_reset(a, b)[0] for a, b in zip(qpos, qvel)])
        s32 = np.array([o32.env_reset(a, b)[0] for a, b in zip(qpos, qvel)])
        w = slice(nq + nv, nq + 2 * nv)
        self.block("qpos", "-", states[:, :nq], s64[:, :nq], s32[:, :nq], qpos=True)
        self.block("qacc_warmstart", "-", states[:, w], s64[:, w], s32[:, w])

    def rollout_blocks(self, model, got, ref64, ref32, rewards=True):
        """Per step index: reward, qpos, base qvel, joint qvel, x.pos of (rewss, qss, qdss, xss) arrays [..., T, *]."""
        for t in range(np.asarray(got[1]).shape[-2]):
            if rewards:
                self.block("reward", t, np.asarray(got[0])[..., t], ref64[0][..., t], ref32[0][..., t])
            self.state_blocks(model, t, np.asarray(got[1])[..., t, :], np.asarray(got[2])[..., t, :],
                              (ref64[1][..., t, :], ref64[2][..., t, :]), (ref32[1][..., t, :], ref32[2][..., t, :]))
            self.block("x.pos", t, np.asarray(got[3])[..., t, :], ref64[3][..., t, :], ref32[3][..., t, :])

    def worst(self):
        return max(self.rows, key=lambda r: r[4])

    def check(self):
        bad = [r for r in self.rows if not r[4] <= 1.0]
        assert not bad, (self.key, bad)
        return self


def rollout_refs(o64, o32, states, us):
    """The two oracles' rollouts from packed fp32 `states` [S, nstate] with `us` [S, B, T, nu], stacked to [S, B, T, ...]."""
    r64 = [o64.rollout(s, u) for s, u in zip(states, us)]
    r32 = [o32.rollout(s, u) for s, u in zip(states, us)]
    stack = lambda rs: tuple(np.stack([r[k] for r in rs]).astype(np.float64) for k in range(4))  # noqa: E731
    return stack(r64), stack(r32)


START_STEPS = (0, 0, 25, 25)   # info.step of the four rollout start states


def with_steps(states, steps=START_STEPS):
    """Copy of packed reset states [S, nstate] with the step counter of state i set to steps[i]: the second half of the rollout
    cases starts mid-episode (0.5 s: inside the command ramp, half a gait period on), where the gait clock, the ramped targets and the
    moving yaw / position targets are not at their trivial start values.  The physics does not read the counter."""
    states = np.array(states, np.float32)
    ni = states.shape[1] - _abi.MACROS["DIAL_INFO_N"]
    states[:, ni + _abi.MACROS["DIAL_INFO_STEP"]] = np.asarray(steps, np.float32)[:states.shape[0]]
    return states


def reset_states(o32, qpos, qvel):
    """Packed fp32 states of the fp32 oracle's env.reset (CPU tests; the GPU tests start from the device's own reset)."""
    return np.array([o32.env_reset(q, v)[0] for q, v in zip(qpos, qvel)], np.float32)
