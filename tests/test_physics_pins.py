"""First-principles pins of the oracle's physics that need neither MuJoCo/MJX nor the oracle's own machinery.

The JAX reference cannot run here and ships no vectors ("parity unpinned").  What CAN be done
is to check the oracle against independent derivations of the same quantities:

  * mass matrix         <- second derivative of the kinetic energy  sum_b 1/2 (m |v_com|^2 + w^T I w), with body
                           velocities obtained by finite differences of plain forward kinematics (no cdof / CRB);
  * bias forces         <- Lagrange's equations  d/dt(dT/dv) - dT/dq + dV/dq  on the hinge coordinates (no RNE);
  * contact Jacobians   <- finite-difference velocity of the material contact point;
  * impedance / aref    <- MuJoCo's documented solref / solimp formulas, restated vectorised (MJX code shape);
  * Newton solver       <- SciPy minimisation of the documented primal cost
                           1/2 (a - a0)^T M (a - a0) + sum_r 1/2 D_r min(0, J_r a - aref_r)^2 .
Conventions checked on the way: free joint = world-frame linear velocity + BODY-frame angular velocity, semi-implicit
Euler with quaternion exponential, [ang; lin] spatial vectors."""
import numpy as np
import pytest

import oracle as O
from conftest import perturbed_state, setup_case
from dial_mpc_amd import mjcf

ROBOTS = [("unitree_go2_trot", 8), ("unitree_h1_jog", 8), ("unitree_h1_loco", 8)]


def _integrate(m, q, v, eps):
    """mj_integratePos: q (+) eps * v."""
    q2 = np.array(q, dtype=np.float64)
    for j in range(m["njnt"]):
        qa, da = int(m["jnt_qposadr"][j]), int(m["jnt_dofadr"][j])
        if m["jnt_type"][j] == mjcf.JNT_FREE:
            q2[qa:qa + 3] += eps * v[da:da + 3]
            w = eps * np.asarray(v[da + 3:da + 6])
            ang = np.linalg.norm(w)
            dq = np.array([1.0, 0, 0, 0]) if ang == 0 else np.concatenate([[np.cos(ang / 2)], w / ang * np.sin(ang / 2)])
            q2[qa + 3:qa + 7] = mjcf.quat_mul(q2[qa + 3:qa + 7], dq)         # body-frame angular velocity
        else:
            q2[qa] += eps * v[da]
    return q2


def _body_velocities(m, q, v, eps=1e-6):
    kp, km = mjcf.host_kinematics(m, _integrate(m, q, v, eps)), mjcf.host_kinematics(m, _integrate(m, q, v, -eps))
    vcom = (kp["xipos"] - km["xipos"]) / (2 * eps)
    omega = np.zeros_like(vcom)
    for b in range(m["nbody"]):
        dR = kp["xmat"][b] @ km["xmat"][b].T                                  # ~ I + 2 eps [w]x
        omega[b] = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / (4 * eps)
    return vcom, omega


def _kinetic_bilinear(m, q, v1, v2):
    k0 = mjcf.host_kinematics(m, q)
    vc1, w1 = _body_velocities(m, q, v1)
    vc2, w2 = _body_velocities(m, q, v2)
    t = 0.0
    for b in range(1, m["nbody"]):
        I = k0["ximat"][b] @ np.diag(m["body_inertia"][b]) @ k0["ximat"][b].T
        t += m["body_mass"][b] * vc1[b] @ vc2[b] + w1[b] @ I @ w2[b]
    return t


def _case(example, seed):
    dc, env, model, task, cfg = setup_case(example, 8, 8)
    md = env.sys.model
    q, qd = perturbed_state(env, seed)
    return env, md, model, task, cfg, np.asarray(q, np.float64), np.asarray(qd, np.float64)


def check_mass_matrix(md, M, q, what=""):
    """M against the kinetic energy's bilinear form (+ armature) on random velocity pairs and on every diagonal entry; any tree."""
    nv = md["nv"]
    rng = np.random.default_rng(0)
    # full bilinear form on random velocity pairs + every diagonal entry
    for _ in range(6):
        a, b = rng.normal(size=nv), rng.normal(size=nv)
        ref = _kinetic_bilinear(md, q, a, b) + a @ (np.asarray(md["dof_armature"]) * b)
        assert abs(a @ M @ b - ref) < 1e-6 * max(1.0, abs(ref)), (what, a @ M @ b, ref)
    for i in range(nv):
        e = np.zeros(nv)
        e[i] = 1.0
        ref = _kinetic_bilinear(md, q, e, e) + md["dof_armature"][i]
        assert abs(M[i, i] - ref) < 1e-6 * max(1.0, abs(ref)), (what, i)


@pytest.mark.parametrize("example,_n", ROBOTS)
def test_mass_matrix_is_the_hessian_of_the_kinetic_energy(example, _n):
    env, md, model, task, cfg, q, qd = _case(example, 3)
    o64 = O.Oracle(model, task, cfg, np.float64)
    M = o64.forward_dump(q, np.zeros(md["nv"]))["qM"]
    check_mass_matrix(md, M, q, example)


def joint_coordinates(md):
    """(dof indices, qpos addresses) of the slide / hinge joints -- the ordinary coordinates; the rest are free-joint dofs."""
    dofs, qadr = [], []
    for j in range(md["njnt"]):
        if md["jnt_type"][j] != mjcf.JNT_FREE:
            dofs.append(int(md["jnt_dofadr"][j]))
            qadr.append(int(md["jnt_qposadr"][j]))
    return np.array(dofs, int), np.array(qadr, int)


def check_lagrange_bias(md, o64, q, qd, what=""):
    """Every free base at rest: on the slide / hinge coordinates c = sum_k dM/dq_k qd_k qd - 1/2 d(qd^T M qd)/dq + dV/dq.  Any number
    of free joints, anywhere in the dof order (none: a fixed-base model)."""
    nv, nq = md["nv"], md["nq"]
    dofs, qadr = joint_coordinates(md)
    v = np.zeros(nv)
    v[dofs] = np.asarray(qd)[dofs]
    bias = o64.forward_dump(q, v)["qfrc_bias"]
    g = np.asarray(md["gravity"], np.float64)

    def Mh(qq):
        return o64.forward_dump(qq, np.zeros(nv))["qM"][np.ix_(dofs, dofs)]

    def V(qq):
        k = mjcf.host_kinematics(md, qq)
        return -sum(md["body_mass"][b] * g @ k["xipos"][b] for b in range(1, md["nbody"]))

    h, nh = 1e-5, len(dofs)
    th = v[dofs]
    dM = np.zeros((nh, nh, nh))       # dM[k] = dM/dtheta_k
    dV = np.zeros(nh)
    for k in range(nh):
        e = np.zeros(nq)
        e[qadr[k]] = h
        dM[k] = (Mh(q + e) - Mh(q - e)) / (2 * h)
        dV[k] = (V(q + e) - V(q - e)) / (2 * h)
    Mdot = np.einsum("kij,k->ij", dM, th)
    c = Mdot @ th - 0.5 * np.einsum("kij,i,j->k", dM, th, th) + dV
    assert np.allclose(bias[dofs], c, rtol=1e-5, atol=2e-5), (what, np.abs(bias[dofs] - c).max())


@pytest.mark.parametrize("example,_n", ROBOTS)
def test_bias_forces_satisfy_lagranges_equations_on_the_hinges(example, _n):
    """Base at rest: on the hinge coordinates c = sum_k dM/dq_k qd_k qd - 1/2 d(qd^T M qd)/dq + dV/dq."""
    env, md, model, task, cfg, q, qd = _case(example, 5)
    o64 = O.Oracle(model, task, cfg, np.float64)
    dofs, qadr = joint_coordinates(md)
    assert np.array_equal(dofs, np.arange(6, md["nv"])) and np.array_equal(qadr, np.arange(7, md["nq"]))
    check_lagrange_bias(md, o64, q, qd, example)


@pytest.mark.parametrize("example,_n", ROBOTS)
def test_bias_forces_satisfy_the_hamel_equations_on_every_dof(example, _n):
    """ALL dofs, moving base included.  The free joint's velocity is a quasi-velocity (world-frame linear, BODY-frame
    angular), so Lagrange's equations take Hamel's form: with p = M v, D_k the derivative along generator k (a step of
    mj_integratePos along the unit velocity e_k) and the so(3) structure constants of the body-frame rates,
        c_k = (d/dt M) v |_k  -  D_k (1/2 v^T M v)  +  D_k V  +  [w x p_rot]_k   (last term: rotational base dofs only).
    M is taken as the Hessian of the kinetic energy of plain forward kinematics (no cdof / CRB / RNE anywhere)."""
    env, md, model, task, cfg, q, qd = _case(example, 7)
    o64 = O.Oracle(model, task, cfg, np.float64)
    nv = md["nv"]
    v = np.array(qd)
    bias = o64.forward_dump(q, v)["qfrc_bias"]
    g = np.asarray(md["gravity"], np.float64)
    arm = np.asarray(md["dof_armature"], np.float64)
    E = np.eye(nv)

    def Mv(qq):          # M(qq) v from the kinetic energy's bilinear form (body velocities by finite differences)
        return np.array([_kinetic_bilinear(md, qq, E[i], v) for i in range(nv)]) + arm * v

    def T(qq):
        return 0.5 * (_kinetic_bilinear(md, qq, v, v) + v @ (arm * v))

    def V(qq):
        k = mjcf.host_kinematics(md, qq)
        return -sum(md["body_mass"][b] * g @ k["xipos"][b] for b in range(1, md["nbody"]))

    h = 2e-4
    Mdot_v = (Mv(_integrate(md, q, v, h)) - Mv(_integrate(md, q, v, -h))) / (2 * h)
    c = np.array(Mdot_v)
    for k in range(nv):
        qp, qm = _integrate(md, q, E[k], h), _integrate(md, q, E[k], -h)
        c[k] += -(T(qp) - T(qm)) / (2 * h) + (V(qp) - V(qm)) / (2 * h)
    p = Mv(q)
    c[3:6] += np.cross(v[3:6], p[3:6])
    scale = max(1.0, float(np.abs(bias).max()))
    assert np.allclose(bias, c, rtol=0, atol=2e-4 * scale), (example, np.abs(bias - c).max(), scale)


@pytest.mark.parametrize("example,_n", ROBOTS + [("allegro_reorient", 8)])
def test_invweight0_and_meaninertia_follow_their_definitions(example, _n):
    """What MuJoCo's mj_setConst derives at qpos0, checked from the DEFINITIONS with independent ingredients -- M as the
    Hessian of the kinetic energy, body Jacobians as finite differences of forward kinematics:
    meaninertia = mean diag M;  dof_invweight0 = diag M^-1 (free joint: mean over its 3 translational / 3 rotational dofs);
    body_invweight0 = (tr(Jp M^-1 Jp^T) / 3, tr(Jr M^-1 Jr^T) / 3) at the body's centre of mass."""
    dc, env, model, task, cfg = setup_case(example, 8, 8)
    md = env.sys.model
    nv, nb = md["nv"], md["nbody"]
    q0 = np.asarray(md["qpos0"], np.float64)
    E = np.eye(nv)
    M = np.array([[_kinetic_bilinear(md, q0, E[i], E[j]) for j in range(nv)] for i in range(nv)]) + np.diag(md["dof_armature"])
    Minv = np.linalg.inv(M)
    assert abs(md["meaninertia"] - np.mean(np.diag(M))) < 1e-6 * np.mean(np.diag(M))
    diw = np.diag(Minv).copy()
    for j in range(md["njnt"]):
        if md["jnt_type"][j] == mjcf.JNT_FREE:
            da = int(md["jnt_dofadr"][j])
            diw[da:da + 3], diw[da + 3:da + 6] = diw[da:da + 3].mean(), diw[da + 3:da + 6].mean()
    assert np.allclose(md["dof_invweight0"], diw, rtol=2e-5), np.abs(np.asarray(md["dof_invweight0"]) / diw - 1).max()
    vc, om = zip(*[_body_velocities(md, q0, E[i]) for i in range(nv)])       # columns of Jp (at the COM) and Jr
    for b in range(1, nb):
        Jp, Jr = np.stack([vc[i][b] for i in range(nv)], 1), np.stack([om[i][b] for i in range(nv)], 1)
        ref = np.array([np.trace(Jp @ Minv @ Jp.T) / 3, np.trace(Jr @ Minv @ Jr.T) / 3])
        assert np.allclose(md["body_invweight0"][b], ref, rtol=2e-5, atol=1e-9), (example, b, md["body_invweight0"][b], ref)


def check_floor_contact_jacobians(md, d, q, contacts, what=""):
    """The pyramid rows of the contacts `contacts` (geom1 a plane with normal +z on the world body) against the finite-difference
    velocity of the material contact point on body2.  Any tree."""
    nv = md["nv"]
    k0 = mjcf.host_kinematics(md, q)
    nl = md["nlim"] + md.get("nfri", 0)
    rng = np.random.default_rng(1)
    eps = 1e-6
    for c in contacts:
        assert int(md["con_body1"][c]) == 0, (what, c)
        b2 = int(md["con_body2"][c])
        p = d["con_pos"][c]
        ploc = k0["xmat"][b2].T @ (p - k0["xpos"][b2])
        rows = d["efc_J"][nl + 4 * c: nl + 4 * c + 4]
        mu = md["con_friction"][c][0]
        Jn, Jt1, Jt2 = (rows[0] + rows[1]) / 2, (rows[0] - rows[1]) / (2 * mu), (rows[2] - rows[3]) / (2 * mu)
        # contact frame: normal = plane normal (0,0,1); tangents from the oracle's rows are checked for orthonormality
        for _ in range(3):
            v = rng.normal(size=nv)
            kp, km = mjcf.host_kinematics(md, _integrate(md, q, v, eps)), mjcf.host_kinematics(md, _integrate(md, q, v, -eps))
            vel = ((kp["xpos"][b2] + kp["xmat"][b2] @ ploc) - (km["xpos"][b2] + km["xmat"][b2] @ ploc)) / (2 * eps)
            comp = np.array([Jn @ v, Jt1 @ v, Jt2 @ v])
            assert abs(comp[0] - vel[2]) < 1e-6 * max(1, abs(vel[2])), (what, c)                  # normal = +z
            assert abs(np.linalg.norm(comp) - np.linalg.norm(vel)) < 1e-6 * max(1, np.linalg.norm(vel)), (what, c)   # orthonormal frame


@pytest.mark.parametrize("example,_n", ROBOTS[:2])
def test_contact_jacobian_is_the_velocity_of_the_material_contact_point(example, _n):
    env, md, model, task, cfg, _, _ = _case(example, 0)
    q = np.array(env._init_q, np.float64)                     # home pose: every foot contact is active
    o64 = O.Oracle(model, task, cfg, np.float64)
    d = o64.forward_dump(q, np.zeros(md["nv"]))
    assert np.all(d["con_dist"] < 0)
    check_floor_contact_jacobians(md, d, q, range(md["ncon"]), example)


def _impedance_rows(md, q, v, d):
    """constraint.make_constraint's (D, aref) restated vectorised from the documented solref / solimp formulas:
    rows = limits then 4 pyramid edges per contact."""
    nl, nc, nv = md["nlim"], md["ncon"], md["nv"]
    dt = float(md["timestep"])
    ji = np.asarray(md["lim_jnt"][:nl], int)
    qa, da = np.asarray(md["jnt_qposadr"])[ji], np.asarray(md["jnt_dofadr"])[ji]
    rng_ = np.asarray(md["jnt_range"])[ji]
    dmin_, dmax_ = q[qa] - rng_[:, 0], rng_[:, 1] - q[qa]
    pos_l = np.minimum(dmin_, dmax_) - np.asarray(md["jnt_margin"])[ji]
    sgn = np.where(dmin_ < dmax_, 1.0, -1.0)
    vel_l = sgn * v[da]
    invw_l = np.asarray(md["dof_invweight0"])[da]
    pos_c = np.repeat(d["con_dist"][:nc] - np.asarray(md["con_margin"])[:nc], 4)
    biw = np.asarray(md["body_invweight0"])[:, 0]
    t = biw[np.asarray(md["con_body1"][:nc], int)] + biw[np.asarray(md["con_body2"][:nc], int)]
    mu = np.asarray(md["con_friction"])[:nc, 0]
    invw_c = np.repeat((t + mu * mu * t) * 2 * mu * mu / float(md["impratio"]), 4)
    vel_c = d["efc_J"][nl:] @ v
    pos = np.concatenate([pos_l, pos_c])
    vel = np.concatenate([vel_l, vel_c])
    invw = np.concatenate([invw_l, invw_c])
    solref = np.concatenate([np.asarray(md["jnt_solref"])[ji], np.repeat(np.asarray(md["con_solref"])[:nc], 4, 0)])
    solimp = np.concatenate([np.asarray(md["jnt_solimp"])[ji], np.repeat(np.asarray(md["con_solimp"])[:nc], 4, 0)])
    tc = np.maximum(solref[:, 0], 2 * dt)
    dr = solref[:, 1]
    d0, dm, width, mid, power = (np.clip(solimp[:, 0], 1e-4, 0.9999), np.clip(solimp[:, 1], 1e-4, 0.9999),
                                 np.maximum(solimp[:, 2], 1e-15), np.clip(solimp[:, 3], 1e-4, 0.9999),
                                 np.maximum(solimp[:, 4], 1))
    k = 1 / (dm * dm * tc * tc * dr * dr)
    b = 2 / (dm * tc)
    x = np.abs(pos) / width
    y = np.where(x < mid, x ** power / mid ** (power - 1), 1 - (1 - x) ** power / (1 - mid) ** (power - 1))
    imp = np.where(x > 1, dm, np.clip(d0 + y * (dm - d0), d0, dm))
    active = pos < 0
    R = np.maximum(invw * (1 - imp) / imp, 1e-15)
    return np.where(active, 1 / R, 0.0), np.where(active, -b * vel - k * imp * pos, 0.0)


@pytest.mark.parametrize("example,_n", ROBOTS)
def test_constraint_rows_match_the_documented_impedance_formulas(example, _n):
    env, md, model, task, cfg, q, qd = _case(example, 2)
    o64 = O.Oracle(model, task, cfg, np.float64)
    for qq, vv in ((np.array(env._init_q, np.float64), np.zeros(md["nv"])), (q, qd)):
        if example == "unitree_go2_trot":
            qq = qq.copy()
            qq[9] = -0.84          # a calf joint past its upper limit (-0.85...): a limit row becomes active
        d = o64.forward_dump(qq, vv)
        D, aref = _impedance_rows(md, qq, vv, d)
        assert np.allclose(d["efc_D"], D, rtol=1e-5, atol=0), (example, np.abs(d["efc_D"] - D).max())
        assert np.allclose(d["efc_aref"], aref, rtol=1e-5, atol=1e-7 * (1 + np.abs(aref).max()))
        assert (D > 0).sum() > 0


@pytest.mark.parametrize("example,_n", ROBOTS)
def test_converged_newton_solution_minimises_the_primal_cost(example, _n):
    """Run the oracle's solver to convergence (iterations = 100) and compare qacc with SciPy's minimiser of the
    primal cost built from the oracle's own (M, a0, J, D, aref) -- checks the solver, its line search and the
    active-set logic independently of how they are coded."""
    from scipy.optimize import minimize
    env, md, model, task, cfg, q, qd = _case(example, 4)
    m2 = type(model).from_buffer_copy(model)
    m2.iterations, m2.ls_iterations = 100, 50
    o64 = O.Oracle(m2, task, cfg, np.float64)
    nv = md["nv"]
    for qq, vv in ((np.array(env._init_q, np.float64), np.zeros(nv)), (q, 0.2 * qd)):
        d = o64.forward_dump(qq, vv, ctrl=np.zeros(md["nu"]))
        M, a0, J, D, aref = d["qM"], d["qacc_smooth"], d["efc_J"], d["efc_D"], d["efc_aref"]

        def cost(a):
            r = J @ a - aref
            ra = np.minimum(r, 0)
            return 0.5 * (a - a0) @ M @ (a - a0) + 0.5 * np.sum(D * ra * ra)

        def grad(a):
            r = J @ a - aref
            return M @ (a - a0) + J.T @ (D * np.minimum(r, 0))

        def hess(a):
            act = (J @ a - aref) < 0
            return M + (J.T * (D * act)) @ J

        res = minimize(cost, a0, jac=grad, hess=hess, method="trust-exact", options=dict(gtol=1e-10, maxiter=500))
        assert np.linalg.norm(grad(res.x)) < 1e-6 * (1 + np.linalg.norm(M @ a0))
        scale = 1 + np.abs(res.x).max()
        assert np.abs(d["qacc"] - res.x).max() < 1e-5 * scale, (example, np.abs(d["qacc"] - res.x).max(), d["niter"])
        assert cost(d["qacc"]) <= cost(res.x) * (1 + 1e-9) + 1e-9
        # the truncated solve the envs use (2 iterations) is a descent from both start points, never worse than them
        o_trunc = O.Oracle(model, task, cfg, np.float64)
        dt = o_trunc.forward_dump(qq, vv, ctrl=np.zeros(md["nu"]))
        assert cost(dt["qacc"]) <= cost(a0) + 1e-9 and cost(dt["qacc"]) >= cost(res.x) - 1e-7 * (1 + abs(cost(res.x)))


def test_free_joint_integration_uses_the_quaternion_exponential_of_the_body_rate():
    """Torque-free, gravity-free, contact-free: after one step qpos' = integrate(qpos, qvel', dt) (semi-implicit)."""
    from scipy.spatial.transform import Rotation as R
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", 8, 8)
    m2, t2 = type(model).from_buffer_copy(model), type(task).from_buffer_copy(task)
    for k in range(3):
        m2.gravity[k] = 0.0
    for a in range(12):
        t2.kp[a] = t2.kd[a] = 0.0
    o64 = O.Oracle(m2, t2, cfg, np.float64)
    q = np.array(env._init_q, np.float64)
    q[2] = 3.0
    qd = np.random.default_rng(3).normal(0, 1.0, 18)
    s0, _, _ = o64.env_reset(q, qd)
    s1, _, _, _ = o64.env_step(s0, np.zeros(12))
    v1 = s1[19:37]
    dt = float(m2.timestep)
    assert np.allclose(s1[:3], s0[:3] + dt * v1[:3], atol=1e-12)
    r0 = R.from_quat(np.roll(s0[3:7], -1))
    r1 = r0 * R.from_rotvec(dt * v1[3:6])                     # right-multiplication = body-frame rate
    q1 = np.roll(r1.as_quat(), 1)
    q1 *= np.sign(q1[0]) * np.sign(s1[3])
    assert np.allclose(s1[3:7], q1, atol=1e-9)
    assert np.allclose(s1[7:19], s0[7:19] + dt * v1[6:], atol=1e-12)


# ------------------------------------------------------------------ Allegro: elliptic cones, condim 6, Euler damping
def _allegro_resting_state(o64, env, steps=60):
    """Hold (approximately) the keyframe pose: the ball comes to rest on three fingertips."""
    jr = env.joint_range
    act = 2 * (-jr[:, 0] / (jr[:, 1] - jr[:, 0])) - 1
    st, _, _ = o64.env_reset(env._init_q, np.zeros(22))
    for _ in range(steps):
        st, xp, _, ctrl = o64.env_step(st, act)
    return st, xp, ctrl, act


def _elliptic_cost(md, M, a0, J, D, aref, a):
    """The documented primal cost with elliptic cones: per contact, top zone 0, bottom zone 1/2 sum D r^2, middle zone
    1/2 Dm (N - mu T)^2 with U = (mu r_0, f_j r_j), Dm = D_0 / (mu^2 (1 + mu^2)), mu = friction_0 / sqrt(impratio)."""
    nl, dims, fr, impratio = md["nlim"], md["con_dim"], np.asarray(md["con_friction"]), float(md["impratio"])
    r = J @ a - aref
    c = 0.5 * (a - a0) @ M @ (a - a0)
    rl = np.minimum(r[:nl], 0)
    c += 0.5 * np.sum(D[:nl] * rl * rl)
    r0 = nl
    for k, dim in enumerate(dims):
        mu = fr[k, 0] / np.sqrt(impratio)
        U = np.concatenate([[r[r0] * mu], r[r0 + 1:r0 + dim] * fr[k, :dim - 1]])
        N, T = U[0], np.sqrt(np.sum(U[1:] ** 2))
        if N >= mu * T or (T <= 0 and N >= 0):
            pass
        elif mu * N + T <= 0 or (T <= 0 and N < 0):
            c += 0.5 * np.sum(D[r0:r0 + dim] * r[r0:r0 + dim] ** 2)
        else:
            c += 0.5 * D[r0] / (mu * mu * (1 + mu * mu)) * (N - mu * T) ** 2
        r0 += dim
    return c


def test_allegro_ball_rests_in_the_hand_and_forces_balance_gravity():
    dc, env, model, task, cfg = setup_case("allegro_reorient", 8, 8)
    md = env.sys.model
    o64 = O.Oracle(model, task, cfg, np.float64)
    st, xp, ctrl, act = _allegro_resting_state(o64, env, 100)
    # at the task's target height, (nearly) at rest
    assert abs(xp[0][2] - 0.13) < 2e-3 and np.abs(st[23:26]).max() < 5e-3 and np.abs(st[26:29]).max() < 5e-2
    d = o64.forward_dump(st[:23], st[23:45], ctrl, st[45:67])
    assert np.abs(d["qacc"][:6]).max() < 0.2
    # net contact force on the ball = - gravity force (object dofs 0..2 are world-frame translations)
    f_ball = (d["efc_J"].T @ d["efc_force"])[:3]
    assert np.allclose(f_ball, [0, 0, 0.01 * 9.81], atol=2e-3), f_ball
    active = [c for c in range(19) if d["con_dist"][c] < 0]
    assert set(active) <= {15, 16, 17, 18} and len(active) >= 3                    # sphere-capsule contacts only


def test_allegro_converged_solve_minimises_the_elliptic_primal_cost():
    from scipy.optimize import minimize
    dc, env, model, task, cfg = setup_case("allegro_reorient", 8, 8)
    md = env.sys.model
    t1 = type(task).from_buffer_copy(task)
    t1.n_frames, t1.dt = 1, 0.005                                 # one physics sub-step per call: states mid-impact
    o64 = O.Oracle(model, t1, cfg, np.float64)
    jr = env.joint_range
    act = 2 * (-jr[:, 0] / (jr[:, 1] - jr[:, 0])) - 1
    st, _, _ = o64.env_reset(env._init_q, np.zeros(22))
    checked = 0
    for k in range(200):
        st, _, _, ctrl = o64.env_step(st, act + 0.3 * np.sin(0.07 * k + np.arange(16)))
        if k % 7:
            continue
        d = o64.forward_dump(st[:23], st[23:45], ctrl, st[45:67])
        if not (d["con_dist"] < 0).any():
            continue
        M, a0, J, D, aref = d["qM"], d["qacc_smooth"], d["efc_J"], d["efc_D"], d["efc_aref"]
        cost = lambda a: _elliptic_cost(md, M, a0, J, D, aref, a)   # noqa: E731
        res = minimize(cost, d["qacc"], method="BFGS", options=dict(gtol=1e-11, maxiter=4000))
        res2 = minimize(cost, a0, method="BFGS", options=dict(gtol=1e-11, maxiter=4000))
        best = min(res.fun, res2.fun)
        assert cost(d["qacc"]) <= best * (1 + 1e-7) + 1e-9, (k, cost(d["qacc"]), best, d["niter"])
        checked += 1
    assert checked >= 5


def test_allegro_contact_rows_are_relative_point_and_angular_velocities():
    """condim-6 sphere-capsule contact: rows 0-2 = relative velocity of the two material contact points in the contact
    frame, rows 3-5 = relative angular velocity (body2 - body1), by finite differences of plain forward kinematics."""
    dc, env, model, task, cfg = setup_case("allegro_reorient", 8, 8)
    md = env.sys.model
    o64 = O.Oracle(model, task, cfg, np.float64)
    st, xp, ctrl, act = _allegro_resting_state(o64, env, 30)
    q = st[:23].astype(np.float64)
    d = o64.forward_dump(q, np.zeros(22))
    k0 = mjcf.host_kinematics(md, q)
    nl, eps = md["nlim"], 1e-6
    adr = nl + np.concatenate([[0], np.cumsum(md["con_dim"])[:-1]])
    rng = np.random.default_rng(2)
    tested = 0
    for c in range(14, 19):
        if d["con_dist"][c] >= 0:
            continue
        b1, b2, p = int(md["con_body1"][c]), int(md["con_body2"][c]), d["con_pos"][c]
        rows = d["efc_J"][adr[c]:adr[c] + 6]
        loc = [k0["xmat"][b].T @ (p - k0["xpos"][b]) for b in (b1, b2)]
        for _ in range(3):
            v = rng.normal(size=22)
            kp, km = mjcf.host_kinematics(md, _integrate(md, q, v, eps)), mjcf.host_kinematics(md, _integrate(md, q, v, -eps))
            vel, om = [], []
            for b, l in zip((b1, b2), loc):
                vel.append(((kp["xpos"][b] + kp["xmat"][b] @ l) - (km["xpos"][b] + km["xmat"][b] @ l)) / (2 * eps))
                dR = kp["xmat"][b] @ km["xmat"][b].T
                om.append(np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / (4 * eps))
            rel_v, rel_w = vel[1] - vel[0], om[1] - om[0]
            lin, ang = rows[:3] @ v, rows[3:] @ v
            # the frame is orthonormal with the normal along (capsule point - sphere centre)
            assert abs(np.linalg.norm(lin) - np.linalg.norm(rel_v)) < 1e-5 * max(1, np.linalg.norm(rel_v))
            assert abs(np.linalg.norm(ang) - np.linalg.norm(rel_w)) < 1e-5 * max(1, np.linalg.norm(rel_w))
            n = p - k0["xpos"][b1]
            n /= np.linalg.norm(n)
            assert abs(lin[0] - n @ rel_v) < 1e-5 * max(1, abs(n @ rel_v)) and abs(ang[0] - n @ rel_w) < 1e-5 * max(1, abs(n @ rel_w))
        tested += 1
    assert tested >= 2


def test_allegro_euler_damping_is_the_implicit_update():
    """eulerdamp: qvel' = qvel + dt (M + dt B)^-1 (qfrc_smooth + qfrc_constraint); for the undamped free ball it is the
    plain update, for the damped finger joints it differs from qacc by the documented amount."""
    dc, env, model, task, cfg = setup_case("allegro_reorient", 8, 8)
    t1 = type(task).from_buffer_copy(task)
    t1.n_frames, t1.dt = 1, 0.005
    o64 = O.Oracle(model, t1, cfg, np.float64)
    st, _, _ = o64.env_reset(env._init_q, np.zeros(22))
    rng = np.random.default_rng(0)
    st[23:45] = rng.normal(0, 0.3, 22)
    ctrl = np.clip(rng.normal(0.5, 0.3, 16), 0.3, 1.0)
    d = o64.forward_dump(st[:23], st[23:45], ctrl, st[45:67])
    jr = env.joint_range
    # reproduce env.step's ctrl with an action, then compare the velocity update
    act = 2 * ((ctrl - jr[:, 0] - env._init_q[7:]) / (jr[:, 1] - jr[:, 0])) - 1
    st1, _, _, c1 = o64.env_step(st, act)
    d = o64.forward_dump(st[:23], st[23:45], c1, st[45:67])
    dt, B = 0.005, np.diag(np.asarray(env.sys.model["dof_damping"], np.float64))
    M = d["qM"]
    qfrc = M @ d["qacc"]                       # = qfrc_smooth + qfrc_constraint at the solver's solution
    qacc_damped = np.linalg.solve(M + dt * B, qfrc)
    assert np.allclose(st1[23:45], st[23:45] + dt * qacc_damped, rtol=1e-6, atol=1e-8)
    assert np.allclose(qacc_damped[:6], d["qacc"][:6], atol=1e-9) and np.abs(qacc_damped[6:] - d["qacc"][6:]).max() > 1e-3


# ---------------------------------------------------------------- a whole control step from first principles
def _first_principles_step(md, q, v, ctrl):
    """One physics step of the Go2 built ONLY from: plain forward kinematics (mjcf.host_kinematics), the kinetic and potential
    energy, the documented impedance formulas, the geometry of a sphere on a plane, SciPy's minimiser and the quaternion
    exponential.  Nothing of the oracle is called: no cdof, CRB, RNE, support.jac, Newton solver or line search.

      M        = Hessian of T(q, v) = sum_b 1/2 (m |v_com|^2 + w^T I w)  (+ armature), body velocities by finite differences
      bias     = Hamel's form of Lagrange's equations (world-frame linear / body-frame angular quasi-velocities of the base)
      tau      = clipped motor torque - damping * v
      contacts = foot spheres (Go2) / the end spheres of the foot capsules (H1) on the floor: dist = z_centre - r, point below
                 the centre, frame (n, y, n x y) resp. (n, projected capsule axis, ...); Jacobian rows = finite-difference
                 velocity of the material contact point, 4 pyramid edges Jn +- mu Jt
      qacc     = argmin 1/2 (a - a0)^T M (a - a0) + sum_r 1/2 D_r min(0, J_r a - aref_r)^2
      v' = v + dt qacc,  q' = q (+) dt v'  (semi-implicit Euler, quaternion exponential of the body rate)"""
    from scipy.optimize import minimize
    nv, nq, nl, nc = md["nv"], md["nq"], md["nlim"], md["ncon"]
    dt = float(md["timestep"])
    g = np.asarray(md["gravity"], np.float64)
    arm = np.asarray(md["dof_armature"], np.float64)
    E = np.eye(nv)
    # ---- M
    M = np.zeros((nv, nv))
    for i in range(nv):
        for j in range(i + 1):
            M[i, j] = M[j, i] = _kinetic_bilinear(md, q, E[i], E[j])
    M += np.diag(arm)

    # ---- bias (the derivation of test_bias_forces_satisfy_the_hamel_equations_on_every_dof)
    def Mv(qq):
        return np.array([_kinetic_bilinear(md, qq, E[i], v) for i in range(nv)]) + arm * v

    def T(qq):
        return 0.5 * (_kinetic_bilinear(md, qq, v, v) + v @ (arm * v))

    def V(qq):
        k = mjcf.host_kinematics(md, qq)
        return -sum(md["body_mass"][b] * g @ k["xipos"][b] for b in range(1, md["nbody"]))

    h = 2e-4
    bias = (Mv(_integrate(md, q, v, h)) - Mv(_integrate(md, q, v, -h))) / (2 * h)
    for k in range(nv):
        qp, qm = _integrate(md, q, E[k], h), _integrate(md, q, E[k], -h)
        bias[k] += -(T(qp) - T(qm)) / (2 * h) + (V(qp) - V(qm)) / (2 * h)
    bias[3:6] += np.cross(v[3:6], Mv(q)[3:6])
    # ---- applied forces
    tau = np.zeros(nv)
    cr = np.asarray(md["act_ctrlrange"], np.float64)
    for a in range(md["nu"]):
        c = np.clip(ctrl[a], cr[a, 0], cr[a, 1]) if md["act_ctrllimited"][a] else ctrl[a]
        tau[int(md["act_dofadr"][a])] += float(md["act_gear"][a]) * c
    qfrc_smooth = tau - np.asarray(md["dof_damping"], np.float64) * v - bias
    a0 = np.linalg.solve(M, qfrc_smooth)
    # ---- contacts: foot spheres on the floor
    k0 = mjcf.host_kinematics(md, q)
    n = np.array([0.0, 0.0, 1.0])
    J = np.zeros((nl + 4 * nc, nv))
    dist = np.zeros(nc)
    eps = 1e-6
    for c in range(nc):
        g2, b2 = int(md["con_geom2"][c]), int(md["con_body2"][c])
        r = float(md["geom_size"][g2][0])
        ctr = k0["xpos"][b2] + k0["xmat"][b2] @ np.asarray(md["geom_pos"][g2], np.float64)
        kind = int(md["con_kind"][c])
        frame = np.array([n, [0.0, 1.0, 0.0], np.cross(n, [0.0, 1.0, 0.0])])
        if kind in (1, 2):
            # a capsule on the floor touches with the sphere at one of its ends; MJX's plane_capsule takes the first tangent
            # along the capsule's axis projected into the plane (a CONVENTION: it orients the friction pyramid)
            axis = (k0["xmat"][b2] @ mjcf.quat_to_mat(np.asarray(md["geom_quat"][g2], np.float64)))[:, 2]
            ctr = ctr + (1.0 if kind == 1 else -1.0) * axis * float(md["geom_size"][g2][1])
            b = axis - n * (n @ axis)
            if np.linalg.norm(b) >= 0.5:
                b = b / np.linalg.norm(b)
                frame = np.array([n, b, np.cross(n, b)])
        else:
            assert kind == 0
        dist[c] = ctr[2] - r
        p = ctr - n * (r + 0.5 * dist[c])
        ploc = k0["xmat"][b2].T @ (p - k0["xpos"][b2])
        Jp = np.zeros((3, nv))
        for i in range(nv):
            kp, km = mjcf.host_kinematics(md, _integrate(md, q, E[i], eps)), mjcf.host_kinematics(md, _integrate(md, q, E[i], -eps))
            Jp[:, i] = ((kp["xpos"][b2] + kp["xmat"][b2] @ ploc) - (km["xpos"][b2] + km["xmat"][b2] @ ploc)) / (2 * eps)
        Jc = frame @ Jp
        mu = float(md["con_friction"][c][0])
        J[nl + 4 * c:nl + 4 * c + 4] = [Jc[0] + mu * Jc[1], Jc[0] - mu * Jc[1], Jc[0] + mu * Jc[2], Jc[0] - mu * Jc[2]]
    ji = np.asarray(md["lim_jnt"][:nl], int)
    qa, da = np.asarray(md["jnt_qposadr"])[ji], np.asarray(md["jnt_dofadr"])[ji]
    rng_ = np.asarray(md["jnt_range"])[ji]
    J[np.arange(nl), da] = np.where(q[qa] - rng_[:, 0] < rng_[:, 1] - q[qa], 1.0, -1.0)
    D, aref = _impedance_rows(md, q, v, dict(con_dist=dist, efc_J=J))

    def cost(a):
        ra = np.minimum(J @ a - aref, 0)
        return 0.5 * (a - a0) @ M @ (a - a0) + 0.5 * np.sum(D * ra * ra)

    def grad(a):
        return M @ (a - a0) + J.T @ (D * np.minimum(J @ a - aref, 0))

    def hess(a):
        return M + (J.T * (D * ((J @ a - aref) < 0))) @ J

    res = minimize(cost, a0, jac=grad, hess=hess, method="trust-exact", options=dict(gtol=1e-11, maxiter=1000))
    v2 = v + dt * res.x
    return _integrate(md, q, v2, dt), v2, dict(M=M, bias=bias, a0=a0, qacc=res.x, dist=dist)


def test_a_whole_physics_step_from_first_principles_matches_the_oracle():
    """The composition, not just the parts: state -> next state of the Go2 standing on its feet, driven by motor torques,
    from the first-principles step above vs the oracle's `env.step` physics (solver run to convergence; the envs' 2-iteration
    truncation is pinned separately).  Finite-difference ingredients limit the agreement to ~1e-5."""
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", 8, 8)
    md = env.sys.model
    m2 = type(model).from_buffer_copy(model)
    m2.iterations, m2.ls_iterations = 100, 50
    o64 = O.Oracle(m2, task, cfg, np.float64)
    nv, nq = md["nv"], md["nq"]
    rng = np.random.default_rng(3)
    q = np.array(env._init_q, np.float64)
    q[7:] += rng.uniform(-0.05, 0.05, nv - 6)
    q[2] -= 0.004                                              # feet pressed 4 mm into the floor: all four contacts carry load
    v = rng.normal(0, 0.3, nv)
    ctrl = rng.uniform(-8, 8, md["nu"])
    q2, v2, parts = _first_principles_step(md, q, v, ctrl)
    assert np.all(parts["dist"] < 0)
    d = o64.forward_dump(q, v, ctrl=ctrl)
    # the parts, once more, in this very state
    # (measured: M 2.7e-7 of 16, bias 4.8e-6 of 159, qacc_smooth 4.8e-6 of 266, qacc 2.1e-5 of 234 -- relative 1e-7 .. 1e-8,
    #  the accuracy of the finite differences; the gates sit at 1e-6 relative)
    assert np.allclose(d["qM"], parts["M"], atol=1e-6 * np.abs(parts["M"]).max())
    assert np.allclose(d["qfrc_bias"], parts["bias"], atol=1e-6 * max(1.0, np.abs(parts["bias"]).max()))
    assert np.allclose(d["qacc_smooth"], parts["a0"], atol=1e-6 * max(1.0, np.abs(parts["a0"]).max()))
    scale = 1 + np.abs(parts["qacc"]).max()
    assert np.abs(d["qacc"] - parts["qacc"]).max() < 1e-6 * scale, np.abs(d["qacc"] - parts["qacc"]).max()
    # the step: the oracle integrates its own qacc; compare the next state
    dt = float(md["timestep"])
    v_o = v + dt * d["qacc"]
    q_o = _integrate(md, q, v_o, dt)
    assert np.abs(v2 - v_o).max() < 1e-6 * scale * dt + 1e-12
    assert np.abs(q2 - q_o).max() < 1e-6 * scale * dt * dt + 1e-12
    # and the oracle's own integrator agrees with that formula (env.step = one physics step for this config)
    s0, _, _ = o64.env_reset(q, v)
    # (an action whose PD torque equals `ctrl` is awkward to construct: the integrator is checked on the oracle's own step)
    s1, _, _, ctrl_used = o64.env_step(s0, np.zeros(md["nu"]))
    d1 = o64.forward_dump(q, v, ctrl=ctrl_used)
    v1 = v + dt * d1["qacc"]
    assert np.allclose(s1[nq:nq + nv], v1, atol=1e-9) and np.allclose(s1[:nq], _integrate(md, q, v1, dt), atol=1e-9)


@pytest.mark.parametrize("example,nstates", [("unitree_go2_trot", 6), ("unitree_h1_jog", 3)])
def test_first_principles_step_on_random_states(example, nstates):
    """The same composition over several random states of the Go2 and the H1 (capsule feet): perturbed joints, base height
    varied so that between one and all of the contacts are closed, random velocities and motor torques.  Gate: 1e-6 relative on
    qacc and on the next state (finite-difference accuracy)."""
    dc, env, model, task, cfg = setup_case(example, 8, 8)
    md = env.sys.model
    m2 = type(model).from_buffer_copy(model)
    m2.iterations, m2.ls_iterations = 200, 50
    o64 = O.Oracle(m2, task, cfg, np.float64)
    nv = md["nv"]
    rng = np.random.default_rng(11)
    dt = float(md["timestep"])
    closed = []
    for k in range(nstates):
        q = np.array(env._init_q, np.float64)
        q[7:] += rng.uniform(-0.08, 0.08, nv - 6)
        q[3:7] = mjcf.quat_mul(q[3:7], np.array([1.0, *rng.normal(0, 0.02, 3)]))
        q[3:7] /= np.linalg.norm(q[3:7])
        q[2] += rng.uniform(-0.006, 0.004)
        v = rng.normal(0, 0.3, nv)
        ctrl = rng.uniform(-10, 10, md["nu"])
        q2, v2, parts = _first_principles_step(md, q, v, ctrl)
        closed.append(int((parts["dist"] < 0).sum()))
        d = o64.forward_dump(q, v, ctrl=ctrl)
        scale = 1 + np.abs(parts["qacc"]).max()
        assert np.allclose(d["con_dist"], parts["dist"], atol=1e-7)       # (the oracle reads the model constants as fp32)
        assert np.abs(d["qacc"] - parts["qacc"]).max() < 1e-6 * scale, (example, k, np.abs(d["qacc"] - parts["qacc"]).max(), scale)
        v_o = v + dt * d["qacc"]
        assert np.abs(v2 - v_o).max() < 1e-6 * scale * dt + 1e-12
        assert np.abs(q2 - _integrate(md, q, v_o, dt)).max() < 1e-6 * scale * dt * dt + 1e-12
    assert max(closed) >= 2 and len(set(closed)) >= 1, closed
