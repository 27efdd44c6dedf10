"""The box zoo: three synthetic models of tests/synthetic/ whose box geoms are everything the two crates are not (a crate is ONE large
box whose geom frame is the frame of its free body).  Next to tests/synthetic_cases.py, whose helpers it reuses; shared by
tests/test_box_zoo.py (CPU) and tests/test_gpu_box_zoo.py.

  box_limbs  box geoms offset and rotated in their body frames: on the free base, on a shin two joints deep (tilted, next to a capsule
             rod), on a SECOND free body (with a sphere); plane-box from three bodies, capsule-box, sphere-box, sphere-capsule (so it
             needs a plugin), plane-sphere, plane-capsule; no box-box
  box_pair   ONE box-box pair (a tray on a jointed limb body against a plank on a second free body) on dimensions whose dead velocity
             temporaries hold the four clipping polygons EXACTLY (6 nv + 12 nbody = 240 = 4 x 60 words); four sites (the Go2 walk task
             is valid) and no sphere- / capsule-capsule pair (the capacity-dimension kernel runs it too).  box_pair_short: one welded
             body fewer, 12 words short -- refused
  box_self   one tree whose own geoms collide: a box on limb a's last body against a capsule and a sphere on limb b's last body

Every model's plugin carries the PROBE reward of tests/plugin_probe.hip (one plugin per model reads every cdist / cpos word); physics
is gated with physics_only=True and without the reward mirror, which the five robots of synthetic_cases.py cover."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

import synthetic_cases as Z
from dial_mpc_amd import _abi
from dial_mpc_amd.envs.custom_env import CustomEnv
from plugin_cases import PROBE

MODELS = ("box_limbs", "box_pair", "box_self")
WALK = ("box_pair",)
M = _abi.MACROS
PLANE_BOX, SPHERE_BOX, CAPSULE_BOX, BOX_BOX = (M["DIAL_CON_" + k] for k in ("PLANE_BOX", "SPHERE_BOX", "CAPSULE_BOX", "BOX_BOX"))
BOX_KINDS = (PLANE_BOX, SPHERE_BOX, CAPSULE_BOX, BOX_BOX)
KIND_NAME = {0: "plane-sphere", 1: "plane-capsule+", 2: "plane-capsule-", 3: "sphere-capsule", 4: "capsule-capsule", PLANE_BOX: "plane-box",
             SPHERE_BOX: "sphere-box", CAPSULE_BOX: "capsule-box", BOX_BOX: "box-box"}
NEAR = 0.01   # the slots of the geometry checks: within 1 cm of touching (DIAL_BOX_PARK_DIST: beyond it a box slot may be parked)


def box_pair_short(tmp_dir):
    """box_pair without its fifth pod (nbody 11): 6 * 16 + 12 * 11 = 228 words for polygons of 240, written to tmp_dir -> its path."""
    text = open(Z.xml_path("box_pair")).read()
    start = text.index("<!-- fifth pod -->")
    end = text.index("</body>", start) + len("</body>")
    assert text[start:end].count("<body") == 1
    path = os.path.join(str(tmp_dir), "box_pair_short.xml")
    with open(path, "w") as f:
        f.write(text[:start] + text[end:])
    return path


@dataclass
class BoxConfig(Z.ZooConfig):
    probe_field: float = 1.0    # the probe's selector for rollouts (plugin_probe.hip: params[0], params[1]): qpos[0]
    probe_index: float = 0.0


def env_class(path):
    name = os.path.splitext(os.path.basename(path))[0]
    return type("BoxZoo_" + name, (CustomEnv,), dict(model_path=path, reward_hip=PROBE, user_params=("probe_field", "probe_index")))


PARAMS = (1.0, 0.0)


@functools.lru_cache(maxsize=None)
def load(name, N=15, H=4, frames=4):
    """The case of one model, as synthetic_cases.load makes it, with the probe reward.  frames=1: both tasks with ONE physics step per
    control step (dt = the timestep) -- the reward's pre-integration inputs then belong to the start state itself."""
    from conftest import LS_SWAP, with_solver
    from dial_mpc_amd.core.dial_config import DialConfig
    from dial_mpc_amd.core.dial_core import make_cfg
    env = env_class(Z.xml_path(name))(BoxConfig(dt=0.005 * frames))
    md = env.sys.model
    model = with_solver(env.make_model(), ls_rule=LS_SWAP)
    ptask = env.make_task()
    assert ptask.kind == M["DIAL_TASK_USER"] and ptask.n_frames == frames
    otask = Z.walk_task(md, ptask, feet=name in WALK, home_z=float(env._init_q[2]))
    cfg = make_cfg(DialConfig(Nsample=N, Hsample=H, Hnode=min(4, H)))
    return dict(name=name, control="position", env=env, md=md, model=model, ptask=ptask, otask=otask, cfg=cfg, walk=name in WALK)


@functools.lru_cache(maxsize=None)
def smooth_cases(name):
    import smooth_ref as S
    c = load(name)
    o64, _ = Z.oracles(c)
    return S.rollout_cases_for(name, c["env"], c["model"], c["otask"], c["cfg"], o64)


# ------------------------------------------------------------------------------------------------------------------ geometry in NumPy
def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def quat_mat(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def geom_constants(model):
    """(geom_pos, geom_quat, geom_size) as the model struct holds them (fp32), in fp64."""
    return tuple(_abi.as_numpy(model, k)[:model.ngeom].astype(np.float64) for k in ("geom_pos", "geom_quat", "geom_size"))


def geom_world(md, xpos, xquat, model=None):
    """World pose of every collision geom from body frames [nbody, 3] / [nbody, 4] (body 0 the world), in NumPy fp64 and with nothing
    of the oracle's or the kernel's: centre xpos + R(xquat) geom_pos, rotation matrix of xquat * geom_quat.  model: take the
    constants from the struct (fp32) instead of the compiled dict."""
    gpos, gquat = (md["geom_pos"], md["geom_quat"]) if model is None else geom_constants(model)[:2]
    out = []
    for g in range(int(md["ngeom"])):
        b = int(md["geom_bodyid"][g])
        out.append((np.asarray(xpos[b], np.float64) + quat_mat(xquat[b]) @ np.asarray(gpos[g], np.float64),
                    quat_mat(quat_mul(_unit(xquat[b]), np.asarray(gquat[g], np.float64)))))
    return out


def pose_slack(model, g1, g2):
    """What the fp32 model constants leave open in a distance between geoms g1 and g2, in metres.  A geom_quat rounded to fp32 is a unit
    quaternion only to |q|^2 - 1 = e ~ 1e-8; whether a reader normalises it (as geom_world does) or expands it as it stands (the
    homogeneous matrix form scales the geom's axes by 1 + e) is a convention, worth e x the geom's extent.  Bound: 2 (|e1| + |e2|) x (the
    two geoms' circumradii + 1 cm) -- 1e-9 .. 1e-8 m here, six orders below a wrong pose composition."""
    _, gquat, gsize = geom_constants(model)
    e = [abs(float(gquat[g] @ gquat[g]) - 1.0) for g in (g1, g2)]
    return 2.0 * (e[0] + e[1]) * (float(np.linalg.norm(gsize[g1])) + float(np.linalg.norm(gsize[g2])) + 0.01)


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def body_frames(dump):
    """[nbody, 3], [nbody, 4] with the world as body 0, from Oracle.forward_dump (which lists either nbody or nbody - 1 bodies)."""
    xp, xq = np.asarray(dump["xpos"], np.float64).reshape(-1, 3), np.asarray(dump["xquat"], np.float64).reshape(-1, 4)
    return xp, xq


# ------------------------------------------------------------------------------------------------------------------ in contact
def _settle(c, o64, q0, hold, seconds=(3.0, 12.0)):
    model = c["model"]
    nq, nv = model.nq, model.nv
    st = o64.env_reset(q0, np.zeros(nv))[0]
    for k in range(int(seconds[1] / 0.02)):
        st = o64.env_step(st, hold)[0]
        if k >= int(seconds[0] / 0.02) - 1 and np.abs(st[nq:nq + nv]).max() < 0.02:
            break
    return st[:nq].copy(), st[nq:nq + nv].copy()


def _hold(c, pose):
    import smooth_ref as S
    return np.clip(S.hold_action(c["model"], c["otask"], np.asarray(pose, np.float64)), -1, 1)


def _drop(model, q, height=0.03, speed=0.3):
    """Every free body `height` higher, moving down at `speed`."""
    q, v = np.array(q, np.float64), np.zeros(model.nv)
    for qa, da in Z._free_joints(model):
        q[qa + 2] += height
        v[da + 2] = -speed
    return q, v


def _axis_quat(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def _place_cargo(c, q, geom, centre, world_quat):
    """qpos with the second free body placed so that its geom `geom` has the world centre and orientation given."""
    md = c["md"]
    qa = Z._free_joints(c["model"])[1][0]
    gq, gp = np.asarray(md["geom_quat"][geom], np.float64), np.asarray(md["geom_pos"][geom], np.float64)
    bq = quat_mul(np.asarray(world_quat, np.float64), gq * [1, -1, -1, -1])
    bq /= np.linalg.norm(bq)
    q = np.array(q, np.float64)
    q[qa + 3:qa + 7] = bq
    q[qa:qa + 3] = np.asarray(centre, np.float64) - quat_mat(bq) @ gp
    return q


@functools.lru_cache(maxsize=None)
def contact_cases(name):
    """(case, qpos [S, nq], qvel [S, nv], us [S, 16, 8, nu], labels) of the in-contact gate, float32.  State 0 of every model RESTS on
    its contacts (the fp64 oracle holds the keyframe's joint targets from the keyframe until the model is at rest); the others start
    3 cm above their contacts, moving down at 0.3 m/s.
      box_limbs  0: the sprawled robot on the floor (trunk slab and foot pad: plane-box), the cargo block along the shin's rod (both
                    capsule-box candidates) with its ball on the trunk slab (sphere-box)
                 1: the same 3 cm up: the tilted boxes land corner first on the floor, then the cargo on the robot
      box_pair   0: the plank LEANS, one end on the floor, its underside on the tray's upper edge -- an edge on a face.  (Lying flat
                    on the tray it would be a flush face on a face, a clipping knife edge; the lean is the tilt.)
                 1: the plank 3 cm above the tray with a CORNER down over the tray's top face
                 2: the plank 3 cm above the tray with a long EDGE down, crossing the tray's upper edge at an angle (edge across edge)
      box_self   0: the servos press limb a's bar flat against limb b's rod (capsule-box)
                 1: other joint targets (hips -+ 0.25, knees straight: the limbs meet in a V), the bar's end pressed on limb b's tip
                    (sphere-box); at rest under those targets, then 3 cm up
    us = the action that holds the state's resting pose + uniform noise in +- 0.3, clipped to +- 1."""
    c = load(name, N=Z.CONTACT_B - 1, H=Z.CONTACT_T - 1)
    model, md = c["model"], c["md"]
    o64, _ = Z.oracles(c)
    nv = model.nv
    q0 = np.asarray(c["env"]._init_q, np.float64).copy()
    rest_q, rest_v = _settle(c, o64, q0, _hold(c, q0))
    assert np.abs(rest_v).max() < 0.05, f"{name}: not at rest ({np.abs(rest_v).max():.3g})"
    states, labels, holds = [(rest_q, rest_v)], ["resting"], [_hold(c, rest_q)]
    if name == "box_limbs":
        states.append(_drop(model, rest_q))
        labels.append("dropped 3 cm")
    elif name == "box_self":
        q1 = q0.copy()
        q1[7:11] = [-0.25, 0.0, 0.25, 0.0]
        tip_q, _ = _settle(c, o64, q1, _hold(c, q1))
        states.append(_drop(model, tip_q))
        labels.append("bar on the tip, dropped 3 cm")
        holds.append(_hold(c, q1))
    else:
        names = md["names"]["geom"]
        tray, plank = names.index("tray_slab"), names.index("cargo_plank")
        d = o64.forward_dump(rest_q, np.zeros(nv))
        centre, R = geom_world(md, *body_frames(d))[tray]
        top = centre + R @ np.array([0.0, 0.0, float(md["geom_size"][tray][2])])
        h = np.asarray(md["geom_size"][plank], np.float64)
        # corner down: the plank's diagonal (-1, -1, -1) h turned onto -z, then a yaw; its lowest corner 3 cm above the tray's top
        diag = -h / np.linalg.norm(h)
        axis = np.cross(diag, [0, 0, -1.0])
        ang = np.arccos(np.clip(diag @ [0, 0, -1.0], -1, 1))
        wq = quat_mul(_axis_quat([0, 0, 1], 0.4), _axis_quat(axis, ang))
        q = _place_cargo(c, rest_q, plank, top + [0.0, 0.0, 0.03 + np.linalg.norm(h)], wq)
        states.append((q, _drop(model, q, 0.0)[1]))
        labels.append("plank corner over the tray's face")
        # edge down: rolled 45 deg + 5 deg about its long axis (the edge along x lowest), yawed 35 deg against the tray, centred over
        # the tray's +x upper edge
        wq = quat_mul(_axis_quat([0, 0, 1], 0.6), _axis_quat([1, 0, 0], np.pi / 4 + 0.09))
        edge = centre + R @ np.array([float(md["geom_size"][tray][0]), 0.0, float(md["geom_size"][tray][2])])
        low = np.abs(quat_mat(wq).T @ [0, 0, 1.0]) @ h   # the plank's extent below its centre
        q = _place_cargo(c, rest_q, plank, edge + [0.0, 0.0, 0.03 + low], wq)
        states.append((q, _drop(model, q, 0.0)[1]))
        labels.append("plank edge across the tray's edge")
    q = np.array([s[0] for s in states], np.float32)
    v = np.array([s[1] for s in states], np.float32)
    holds += [holds[0]] * (len(states) - len(holds))
    us = np.array(holds)[:, None, None, :] + np.random.default_rng(29).uniform(-0.3, 0.3, (len(states), Z.CONTACT_B, Z.CONTACT_T, model.nu))
    return c, q, v, np.clip(us, -1, 1).astype(np.float32), labels


def touching_kinds(c, q, v):
    """{kind: slots with con_dist < 0} per start state, by the fp64 oracle."""
    o64, _ = Z.oracles(c)
    kind = np.asarray(c["md"]["con_kind"]).ravel()
    out = []
    for qi, vi in zip(q, v):
        d = o64.forward_dump(qi.astype(np.float64), vi.astype(np.float64))
        out.append({int(k): int(((kind == k) & (d["con_dist"] < 0)).sum()) for k in np.unique(kind)})
    return out


# ------------------------------------------------------------------------------------------------------------------ contact geometry
GEOM_STATES = 32


def _scatter(c, rest_q, rng):
    """The resting pose scattered: joints +- 0.4 rad inside their ranges, the base up to 2 cm up or down and tilted by up to 0.2 rad,
    a second free body moved by up to 15 cm / 4 cm (xy / z) and turned by up to 0.6 rad.  A pose for ONE forward pass, not a state a
    trajectory reaches: geoms may overlap by centimetres."""
    import smooth_ref as S
    model = c["model"]
    q = np.array(rest_q, np.float64)
    for typ, qa, _, limited, lo, hi in S.joints(model):
        if typ != S.FREE:
            q[qa] = np.clip(q[qa] + rng.uniform(-0.4, 0.4), lo, hi) if limited else q[qa] + rng.uniform(-0.4, 0.4)
    for k, (qa, _) in enumerate(Z._free_joints(model)):
        reach, turn = ((0.0, 0.02), 0.2) if k == 0 else ((0.15, 0.04), 0.6)
        q[qa:qa + 2] += rng.uniform(-1, 1, 2) * reach[0]
        q[qa + 2] += rng.uniform(-1, 1) * reach[1]
        rot = quat_mul(_axis_quat(rng.standard_normal(3), rng.uniform(0, turn)), q[qa + 3:qa + 7])
        q[qa + 3:qa + 7] = rot / np.linalg.norm(rot)
    return q


@functools.lru_cache(maxsize=None)
def geometry_states(name):
    """32 fp32 states (qpos, qvel) per model for the contact-geometry checks, chosen with the fp64 oracle alone.  The first 16 lie on
    short fp64 rollouts from the contact cases' start states under random controls (after control steps 0, 2, 4, 6).  The other 16 are
    the resting pose scattered (_scatter), taken in the order drawn whenever a pose adds a slot within 1 cm to a contact kind that
    still has fewer than 8, or lacks a touching or a clear one; a pose on a knife edge (_stable: an fp64 slot that moves by more than 1e-5
    under 4 ulp of jitter) is passed over.  Every contact kind of the model ends with at least 8 slot instances
    within 1 cm, touching and not (asserted)."""
    c, q, v, us, _ = contact_cases(name)
    model = c["model"]
    nq, nv = model.nq, model.nv
    o64, _ = Z.oracles(c)
    rng = np.random.default_rng(37)
    kind = np.asarray(c["md"]["con_kind"]).ravel()
    kinds = [int(k) for k in np.unique(kind)]
    half = GEOM_STATES // 2
    per = -(-half // len(q))
    qs, vs = [], []
    for i in range(len(q)):
        for b in range(-(-per // 4)):
            st = o64.env_reset(q[i].astype(np.float64), v[i].astype(np.float64))[0]
            for t in range(7):
                if t % 2 == 0 and len(qs) < min(half, (i + 1) * per):
                    qs.append(st[:nq].astype(np.float32)), vs.append(st[nq:nq + nv].astype(np.float32))
                st = o64.env_step(st, np.clip(us[i, b, t] + rng.uniform(-0.2, 0.2, model.nu), -1, 1))[0]
    assert len(qs) == half, len(qs)

    def near_of(a, b):
        d = o64.forward_dump(a.astype(np.float64), b.astype(np.float64))["con_dist"]
        return {k: d[(kind == k) & (d < NEAR)] for k in kinds}
    have = {k: np.zeros(0) for k in kinds}
    for a, b in zip(qs, vs):
        for k, d in near_of(a, b).items():
            have[k] = np.concatenate([have[k], d])
    short = lambda k, d: len(d) < 8 or not (d < 0).any() or not (d >= 0).any()   # noqa: E731
    for draw in range(4000):
        if len(qs) == GEOM_STATES:
            break
        a, b = _scatter(c, q[0], rng).astype(np.float32), rng.uniform(-0.5, 0.5, nv).astype(np.float32)
        if not _stable(o64, kind, a, rng):
            continue
        new = near_of(a, b)
        useful = [k for k in kinds if short(k, have[k]) and len(new[k])
                  and (len(have[k]) < 8 or ((new[k] < 0).any() and not (have[k] < 0).any()) or ((new[k] >= 0).any() and not (have[k] >= 0).any()))]
        if useful or not any(short(k, have[k]) for k in kinds):
            qs.append(a), vs.append(b)
            for k in kinds:
                have[k] = np.concatenate([have[k], new[k]])
    assert len(qs) == GEOM_STATES, (name, len(qs), {KIND_NAME[k]: len(d) for k, d in have.items()})
    for k in kinds:
        assert not short(k, have[k]), (name, KIND_NAME[k], len(have[k]), int((have[k] < 0).sum()))
    return c, np.array(qs), np.array(vs)


def _stable(o64, kind, a, rng, tries=3, ulps=4, bound=1e-5):
    """No live slot of the fp64 oracle moves by more than `bound` when qpos is jittered by <= 4 ulp: the pose sits on no knife edge
    (a box-box candidate order about to swap, a sphere centre crossing a box's mid-plane)."""
    base = o64.forward_dump(a.astype(np.float64), np.zeros(o64.nv))
    live = base["con_dist"] < NEAR
    for _ in range(tries):
        j = (a + rng.integers(-ulps, ulps + 1, a.shape) * np.spacing(np.abs(a))).astype(np.float32)
        d = o64.forward_dump(j.astype(np.float64), np.zeros(o64.nv))
        if np.abs(d["con_dist"] - base["con_dist"])[live].max(initial=0.0) > bound or np.abs(d["con_pos"] - base["con_pos"])[live].max(initial=0.0) > bound:
            return False
    return True


def geometry_reference(name):
    """(case, qpos, qvel, fp64 dumps, fp32 dumps) of the geometry states: Oracle.forward_dump of the SAME fp32 state in both precisions."""
    c, qs, vs = geometry_states(name)
    o64, o32 = Z.oracles(c)
    r64 = [o64.forward_dump(a.astype(np.float64), b.astype(np.float64)) for a, b in zip(qs, vs)]
    r32 = [o32.forward_dump(a, b) for a, b in zip(qs, vs)]
    return c, qs, vs, r64, r32


def _exact_mask(kind, dist64):
    """The slots whose narrow phase must have run (test_gpu_plugin_matrix._check_parked): every sphere / capsule / sphere-box slot, and a
    plane-box, capsule-box or box-box slot the fp64 oracle puts within DIAL_BOX_PARK_DIST."""
    from test_gpu_plugin_matrix import PARK
    boxy = np.isin(kind, [PLANE_BOX, CAPSULE_BOX, BOX_BOX])
    return ~boxy | (dist64 <= PARK)


def geometry_tolerances(c, r64, r32):
    """{kind: (tolerance, the fp32 oracle's worst error)}: 8 x the fp32 oracle's worst |fp32 - fp64| of cdist and cpos over the live slots
    of that kind in the geometry states, floor 1e-6 -- the rule of lane_ref.reference_tolerance, computed at run time."""
    from lane_ref import TOL_FLOOR
    kind = np.asarray(c["md"]["con_kind"]).ravel()
    out = {}
    for k in np.unique(kind):
        worst = 0.0
        for a, b in zip(r64, r32):
            m = _exact_mask(kind, a["con_dist"]) & (kind == k)
            if m.any():
                worst = max(worst, float(np.abs(b["con_dist"][m] - a["con_dist"][m]).max()),
                            float(np.abs(np.asarray(b["con_pos"]).reshape(-1, 3)[m] - np.asarray(a["con_pos"]).reshape(-1, 3)[m]).max()))
        out[int(k)] = (max(TOL_FLOOR, 8.0 * worst), worst)
    return out


def geometry_gate(name, cdist, cpos, what):
    """cdist [32, ncon] / cpos [32, ncon, 3] of a build under test against the fp64 oracle's forward_dump of the same fp32 states.
    Live slots (_exact_mask) at the per-kind tolerance; one outside it needs a WITNESS: the fp64 oracle from qpos jittered by <= 4 ulp
    agrees with the build within the tolerance (32 draws).  Parked slots follow test_gpu_plugin_matrix._check_parked, which is
    called with the live slots set to the reference.  -> report dict(live, witnessed, unwitnessed, ratio {kind: worst err / tol}, tol)."""
    from test_gpu_plugin_matrix import _check_parked
    c, qs, vs, r64, r32 = geometry_reference(name)
    o64, _ = Z.oracles(c)
    kind = np.asarray(c["md"]["con_kind"]).ravel()
    tols = geometry_tolerances(c, r64, r32)
    tol = np.array([tols[int(k)][0] for k in kind])
    rep = dict(live=0, witnessed=0, unwitnessed=[], parked=0, ratio={int(k): 0.0 for k in np.unique(kind)}, tol=tols)
    rng = np.random.default_rng(43)
    for s in range(len(qs)):
        rd, rp = r64[s]["con_dist"], np.asarray(r64[s]["con_pos"]).reshape(-1, 3)
        live = _exact_mask(kind, rd)
        err = np.maximum(np.abs(cdist[s].astype(np.float64) - rd), np.abs(cpos[s].astype(np.float64) - rp).max(-1))
        rep["live"] += int(live.sum())
        for k in np.unique(kind):
            m = live & (kind == k) & (err <= tol)
            if m.any():
                rep["ratio"][int(k)] = max(rep["ratio"][int(k)], float((err[m] / tol[m]).max()))
        bad = np.flatnonzero(live & (err > tol))
        left = set(bad.tolist())
        for _ in range(32 if len(bad) else 0):
            j = (qs[s] + rng.integers(-4, 5, qs[s].shape) * np.spacing(np.abs(qs[s]))).astype(np.float32)
            d = o64.forward_dump(j.astype(np.float64), vs[s].astype(np.float64))
            jp = np.asarray(d["con_pos"]).reshape(-1, 3)
            for i in list(left):
                if abs(float(cdist[s, i]) - d["con_dist"][i]) <= tol[i] and np.abs(cpos[s, i].astype(np.float64) - jp[i]).max() <= tol[i]:
                    left.discard(i)
            if not left:
                break
        rep["witnessed"] += len(bad) - len(left)
        rep["unwitnessed"] += [(s, int(i), KIND_NAME[int(kind[i])], float(err[i]), float(tol[i])) for i in sorted(left)]
        # the parked slots: _check_parked with the live slots taken out of its own comparison
        cd, cp = np.where(live, rd, cdist[s]).astype(np.float64), np.where(live[:, None], rp, cpos[s]).astype(np.float64)
        ref = dict(xpos=np.asarray(r64[s]["xpos"]).ravel(), xquat=np.asarray(r64[s]["xquat"]).ravel(), cdist=rd, cpos=rp.ravel())
        rep["parked"] += _check_parked(c, cd, cp, ref, float(tol.max()), {})
    print(f"GEOMETRY {name} {what}: live {rep['live']}, witnessed {rep['witnessed']}, parked {rep['parked']}, per kind tol / worst ratio: "
          + ", ".join(f"{KIND_NAME[k]} {tols[k][0]:.2e} / {r:.2f}" for k, r in rep["ratio"].items()))
    return rep


def assert_geometry(rep):
    assert not rep["unwitnessed"], rep["unwitnessed"][:5]
    assert rep["witnessed"] <= 0.01 * rep["live"], (rep["witnessed"], rep["live"])
