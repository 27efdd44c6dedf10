"""The synthetic robots of tests/synthetic/ without a GPU: what mjcf.compile_mjcf makes of them, the oracle's physics on them from
first principles, the derived tables, the host wave emulator (the capacity-dimension instantiation, and a task plugin's instantiation
at the model's own dimensions) under the rounding-level gate in the air and the per-transition gate in contact, and the refusals a user
of a model like these can run into.  tests/synthetic_cases.py describes the models and the two tasks every case carries.

Measured (CPU, emulator; the device's figures are in DESIGN.md section 2), worst error / tolerance per model -- class-F gate, then the
in-contact gate's worst direct transition.  Witnessed shares of the in-contact gate (caps 10 % and 5 %): emulator 0 of 256 transitions for
every model; the fp32 oracle against itself under 1 ulp of jitter 1 of 256 (chain_mixed), 0 of 256 (the others).
  chain_mixed  position 0.14, torque 0.14 | contact 0.002      fixed_arm 0.15 | contact 0.002      wide_base 0.25 | contact 0.003
  deep_chain   0.17 | contact 0.008      two_trees 0.17 | contact 0.001, falling case 0.011
Every model runs on the capacity dimensions (two_trees excepted: that instantiation refuses it) and on its plugin instantiation; the two
give the same figures.
Resolving power (fp32 oracle with one constant of chain_mixed changed), worst class-F ratio: slide axis tilted by 1e-3 rad 412, body_quat
rotated by 1e-3 rad 58, joint anchor + 1e-4 m 256, gear x (1 + 1e-3) under torque control 15.9."""
import os

import numpy as np
import pytest

import emu_lib
import oracle as O
import smooth_ref as S
import synthetic_cases as Z
from dial_mpc_amd import _abi, mjcf
from emu_lib import Emu
from plugin_cases import keep_contacts
from test_physics_pins import check_floor_contact_jacobians, check_lagrange_bias, check_mass_matrix

K = _abi.MACROS
UNSUPPORTED = K["DIAL_ERR_UNSUPPORTED"]

# name -> (nq, nv, nu, nbody, njnt, ngeom, nsite, ncon, nlim, nfri, nefc), con_kind
TABLE = {
    "chain_mixed": ((10, 9, 3, 5, 4, 5, 4, 6, 3, 0, 27), [0, 0, 1, 2, 1, 2]),
    "fixed_arm": ((6, 6, 6, 7, 6, 2, 0, 1, 6, 0, 10), [0]),
    "two_trees": ((18, 16, 4, 7, 6, 8, 0, 22, 4, 0, 92), [0, 0] + [1, 2] * 5 + [3] * 4 + [4] * 6),
    "wide_base": ((22, 21, 15, 17, 16, 8, 4, 12, 15, 0, 63), [0, 0] + [1, 2] * 5),
    "deep_chain": ((13, 12, 6, 8, 7, 5, 0, 6, 6, 0, 30), [0, 0, 1, 2, 1, 2]),
}
PLUGIN_EMU = Z.MODELS   # every model also runs on its plugin instantiation (emu_lib.user_variant: one emulator build per model)


# ------------------------------------------------------------------------------------------------------------------ the compiler
@pytest.mark.parametrize("name", Z.MODELS)
def test_compiled_dimensions_and_contact_list(name):
    md = mjcf.compile_mjcf(Z.xml_path(name))
    dims = tuple(int(md[k]) for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "nsite", "ncon", "nlim", "nfri", "nefc"))
    assert dims == TABLE[name][0]
    assert np.asarray(md["con_kind"]).tolist() == TABLE[name][1]
    assert md["cone"] == 0 and md["eulerdamp"] == 0 and md["iterations"] == 2 and md["ls_iterations"] == 5 and "home" in md["keyframes"]
    # inside the capacities of include/dial_mpc.h
    assert md["nbody"] <= 24 and md["nv"] <= 28 and md["nu"] <= 20 and md["ngeom"] <= 20 and md["nsite"] <= 8 and md["ncon"] <= 56 and md["nlim"] <= 24
    _abi.make_model(md)   # (raises when a field exceeds its capacity)


def test_what_each_model_is_for():
    md = {n: Z.load(n)["md"] for n in Z.MODELS}
    c = md["chain_mixed"]
    assert c["jnt_type"].tolist() == [mjcf.JNT_FREE, mjcf.JNT_SLIDE, mjcf.JNT_HINGE, mjcf.JNT_HINGE]
    assert c["body_jntnum"].tolist() == [0, 1, 2, 0, 1]                       # two joints on one body, none on the next
    assert not np.allclose(c["body_quat"][1:], [1, 0, 0, 0]) and np.abs(c["jnt_pos"][1:]).max() > 0
    assert not np.allclose(c["body_iquat"][1], [1, 0, 0, 0]) and np.abs(c["body_ipos"][1]).max() > 0
    assert c["act_qposadr"].tolist() == [7, 8, 9] and c["act_gear"].tolist() == [2, 1, 1] and c["act_isposition"].tolist() == [0, 0, 1]
    f = md["fixed_arm"]
    assert mjcf.JNT_FREE not in f["jnt_type"].tolist() and f["jnt_type"].tolist() == [mjcf.JNT_HINGE] * 5 + [mjcf.JNT_SLIDE]
    assert sorted(f["act_isposition"].tolist()) == [0, 1, 1, 1, 1, 1] and 1.5 in f["act_gear"].tolist()
    t = md["two_trees"]
    assert t["jnt_type"].tolist().count(mjcf.JNT_FREE) == 2 and t["body_rootid"].tolist() == [0, 1, 1, 1, 1, 1, 6]
    between = [(int(a), int(b)) for a, b in zip(t["con_body1"], t["con_body2"]) if a != 0]
    assert len(between) == 10 and all(b == 6 for _, b in between)              # robot bodies against the second tree
    w = md["wide_base"]
    limbs = [sum(1 for n in w["names"]["body"] if n[0] == limb and n[1:].isdigit()) for limb in "abcdef"]
    assert limbs == [4, 3, 3, 2, 2, 1] and w["nv"] == 21 and w["ncon"] >= 9
    d = md["deep_chain"]
    assert d["body_depth"].tolist() == list(range(8)) and d["nv"] == 12


def test_custom_env_takes_each_actuators_own_joint_range():
    """A model whose first joint is not free (fixed_arm) or that has a second free joint (two_trees): the env's sampling and clipping
    ranges are those of the joints the actuators drive, not `jnt_range[1:]`."""
    for name in Z.MODELS:
        c = Z.load(name)
        md, env = c["md"], c["env"]
        want = np.array([md["jnt_range"][md["jnt_qposadr"].tolist().index(int(a))] for a in md["act_qposadr"]])
        assert np.array_equal(env.joint_range, want) and env.joint_range.shape == (md["nu"], 2), name
        for a in range(md["nu"]):
            assert tuple(c["ptask"].phys_range[a]) == tuple(np.float32(want[a])), (name, a)


# ------------------------------------------------------------------------------------------------------------------ first principles
def _pin_state(c, seed):
    """A random state for the pins: joints inside their ranges, free bodies rotated, in the air."""
    q, v, _ = S.smooth_states(c["env"], c["model"], "F", 1, seed)
    return q[0].astype(np.float64), v[0].astype(np.float64)


@pytest.mark.parametrize("name", Z.MODELS)
def test_mass_matrix_and_bias_forces_from_first_principles(name):
    c = Z.load(name)
    o64, _ = Z.oracles(c)
    q, v = _pin_state(c, 3)
    check_mass_matrix(c["md"], o64.forward_dump(q, np.zeros(c["md"]["nv"]))["qM"], q, name)
    check_lagrange_bias(c["md"], o64, q, v, name)


@pytest.mark.parametrize("name", Z.MODELS)
def test_floor_contact_jacobians_from_first_principles(name):
    c, q, v, _ = Z.contact_cases(name)
    o64, _ = Z.oracles(c)
    q = q[0].astype(np.float64)
    d = o64.forward_dump(q, np.zeros(c["md"]["nv"]))
    touching = [k for k in range(c["md"]["ncon"]) if d["con_dist"][k] < 0 and c["md"]["con_body1"][k] == 0]
    assert touching, name
    check_floor_contact_jacobians(c["md"], d, q, touching, name)


# ------------------------------------------------------------------------------------------------------------------ derived tables
@pytest.mark.parametrize("name", Z.MODELS)
def test_derived_levels_and_ancestor_masks(name):
    c = Z.load(name)
    md = c["md"]
    d = Emu(c["model"], c["otask"], c["cfg"], path=1).derived()
    assert d["rc"] == 0
    depth, parent = md["body_depth"].tolist(), md["body_parent"].tolist()
    assert d["nlevel"] == max(depth)
    for lvl in range(1, d["nlevel"] + 1):
        assert d["lvl_body"][d["lvl_start"][lvl - 1]:d["lvl_start"][lvl]] == [b for b in range(1, md["nbody"]) if depth[b] == lvl]
    dof_body = md["dof_bodyid"].tolist()
    for b in range(md["nbody"]):
        chain, bb = set(), b
        while bb > 0:
            chain.add(bb)
            bb = parent[bb]
        assert d["body_ancmask"][b] == sum(1 << i for i in range(md["nv"]) if dof_body[i] in chain), (name, b)
    for i in range(md["nv"]):   # dofs of ancestor bodies, and the earlier dofs of the own body
        b = dof_body[i]
        want = d["body_ancmask"][parent[b]] | sum(1 << j for j in range(i + 1) if dof_body[j] == b)
        assert d["dof_ancmask"][i] == want, (name, i)


def test_wide_base_work_list_groups():
    """The H work list of dial_build_derived (the square layouts' table).  With the model's twelve floor contacts there is NONE: the
    list exists for at most eight contacts, and neither the capacity-dimension kernel nor a plugin reads it.  With the eight contacts
    of limbs a (four), b and c (two each) the base dofs are touched by 8 = 4 chunks of 2 (P = 4), limb a's first two dofs by 4 (P = 2)
    and every other touched dof by 2 (P = 1); groups never straddle a quad and come in the order 4, 2, 1."""
    c = Z.load("wide_base")
    md = c["md"]
    assert Emu(c["model"], c["otask"], c["cfg"], path=1).derived()["hitem"] == []
    on = [k for k in range(12) if int(md["con_body2"][k]) in (3, 5, 8, 11)]
    assert len(on) == 8
    m8 = _abi.make_model(keep_contacts(md, on))
    items = Emu(m8, c["otask"], c["cfg"], path=1).derived()["hitem"]
    assert items
    touched = {i: sum(1 for k in on if (1 << i) & _mask(md, int(md["con_body2"][k]))) for i in range(21)}
    assert [touched[i] for i in range(10)] == [8] * 6 + [4, 4, 2, 2]
    sizes = [P for (_, _, P, writer, _, _) in items if writer]
    assert sizes == sorted(sizes, reverse=True) and set(sizes) == {4, 2, 1}
    pos = 0
    for (i, j, P, writer, n, cons) in items:
        if writer:
            assert pos % P == 0, "a group straddles a quad"
            assert P == {8: 4, 4: 2, 2: 1, 0: 1}[touched[i]], (i, j, P)
            group = items[pos:pos + P]
            assert all(g[:3] == (i, j, P) for g in group) and [g[3] for g in group] == [1] + [0] * (P - 1)
            assert sorted(k for g in group for k in g[5]) == [x for x in range(8) if (1 << i) & _mask(md, int(md["con_body2"][on[x]]))]
        pos += 1
    entries = {(i, j) for (i, j, _, w, _, _) in items if w}
    assert entries == {(i, j) for i in range(21) for j in range(i + 1) if (md_anc(md, i) >> j) & 1}


def _mask(md, body):
    m, b = 0, body
    while b > 0:
        m |= sum(1 << i for i in range(md["nv"]) if md["dof_bodyid"][i] == b)
        b = int(md["body_parent"][b])
    return m


def md_anc(md, i):
    m, j = 0, i
    while j >= 0:
        m |= 1 << j
        j = int(md["dof_parentid"][j])
    return m


# ------------------------------------------------------------------------------------------------------------------ emulator, in the air
def _emu(c, plugin):
    """The capacity-dimension instantiation under the walk task, or the model's plugin instantiation under its own task."""
    if not plugin:
        return Emu(c["model"], c["otask"], c["cfg"], path=1)
    defines, tag = emu_lib.user_variant(c["md"], Z.REWARD)
    e = Emu(c["model"], c["ptask"], c["cfg"], path=0, defines=defines, tag=tag)
    e.set_user_params(Z.WEIGHTS)
    return e


AIR = [(n, "position", False) for n in Z.MODELS if n != "two_trees"] + [("chain_mixed", "torque", False)] + [(n, "position", True) for n in PLUGIN_EMU]


@pytest.mark.parametrize("name,control,plugin", AIR, ids=[f"{n}-{k}-{'plugin' if p else 'generic'}" for n, k, p in AIR])
def test_emulator_in_the_air_at_rounding_level(name, control, plugin):
    """Gate c: env_reset of 16 class-F states and five env steps of 4 states x 16 rollouts (|us| <= 0.3, two states at step counter
    25) against the fp64 oracle under smooth_ref's rule, unchanged.  The race check runs on the first case.  Rewards are gated where
    the walk task is valid for the model (chain_mixed, wide_base on the generic path); a plugin's reward against its NumPy mirror."""
    c = Z.load(name, control)
    model = c["model"]
    o64, o32 = Z.oracles(c)
    emu = _emu(c, plugin)
    q16, v16, _ = S.smooth_states(c["env"], model, "F", 16, seed=21)
    gate = S.Gate(name, "F", "reset+rollout", f"emulator-{control}-{'plugin' if plugin else 'generic'}")
    gate.reset_blocks(model, o64, o32, q16, v16, np.array([emu.env_reset(a, b, check_races=False)[0] for a, b in zip(q16, v16)]))
    q, v, us = Z.smooth_cases(name, control)
    resets = np.array([emu.env_reset(q[i], v[i], check_races=(i == 0))[0] for i in range(4)])
    states = S.with_steps(resets)
    for i in range(4):
        S.assert_stays_free(model, c["otask"], o64, states[i], us[i])
    got = [emu.rollout(states[i], us[i], check_races=(i == 0)) for i in range(4)]
    got = tuple(np.stack([g[k] for g in got]) for k in range(4))
    gate.rollout_blocks(model, got, *S.rollout_refs(o64, o32, states, us), rewards=c["walk"] and not plugin)
    gate.check()
    print(f"WORST {name} {control} plugin={plugin}: {gate.worst()}")
    if plugin:   # the reward of tests/synthetic/zoo_reward.hip on the emulator's own outputs, three chained env.steps
        ni, st = model.nq + 2 * model.nv, states[0]
        for t in range(3):
            st, xp, xq, ctrl = emu.env_step(st, us[0, 0, t], check_races=(t == 0))
            want = Z.mirror_reward(model, st, xp, xq, ctrl, us[0, 0, t])
            assert abs(st[ni + K["DIAL_INFO_REWARD"]] - want) <= 1e-4 * abs(want) + 1e-5, (t, st[ni + K["DIAL_INFO_REWARD"]], want)
            assert st[ni + K["DIAL_INFO_USER"]] == t + 1


def test_capacity_dimension_kernel_refuses_two_trees():
    """A pyramidal model with sphere-capsule or capsule-capsule candidates: those narrow phases exist in the elliptic instantiations and
    in a task plugin's; the capacity-dimension instantiation read such a slot as a plane contact (in the air: qacc_warmstart off by
    1.9e4, 3.8e6 x the class-F tolerance) and now refuses the model, as dial_create does."""
    c = Z.load("two_trees")
    q = c["env"]._init_q
    with pytest.raises(AssertionError, match=f"rc={UNSUPPORTED}"):
        Emu(c["model"], c["otask"], c["cfg"], path=1).env_reset(q, np.zeros(c["model"].nv))
    floor_only = _abi.make_model(keep_contacts(c["md"], [k for k in range(22) if c["md"]["con_kind"][k] < 3]))
    Emu(floor_only, c["otask"], c["cfg"], path=1).env_reset(q, np.zeros(c["model"].nv))


# ------------------------------------------------------------------------------------------------------------------ emulator, in contact
def _share(rep):
    return rep["witnessed"] / rep["transitions"]


CONTACT = [(n, False) for n in Z.MODELS if n != "two_trees"] + [(n, True) for n in PLUGIN_EMU]


@pytest.mark.parametrize("name,plugin", CONTACT, ids=[f"{n}-{'plugin' if p else 'generic'}" for n, p in CONTACT])
def test_emulator_in_contact_per_transition(name, plugin):
    """Gate d: 2 start states (resting; 3 cm above its contacts, moving down) x 16 rollouts x 8 control steps under DIAL_LS_SWAP.
    Every transition of every rollout from the emulator's own traced state against the fp32 oracle at conftest.TOL; no transition
    without a <= 64 ulp witness, witnessed share <= 10 %.  First the inputs: the fp32 oracle from 1-ulp jittered states through the
    same gate needs witnesses for <= 5 % of the transitions.  Every model on its plugin instantiation, and all but two_trees on the
    capacity dimensions too."""
    c, q, v, us = Z.contact_cases(name)
    model = c["model"]
    ni = model.nq + 2 * model.nv
    _, o32 = Z.oracles(c)
    emu = _emu(c, plugin)
    tot = dict(ref=[0, 0], emu=[0, 0])
    worst = 0.0
    for i in range(2):
        s0 = o32.env_reset(q[i], v[i])[0]
        ref = Z.contact_gate(c, o32, s0, us[i], *Z.jittered_oracle_run(o32, s0, us[i], ni, seed=5 + i), physics_only=False)
        out = emu.rollout(s0, us[i], check_races=(i == 0), trace=True)
        rep = Z.contact_gate(c, o32, s0, us[i], out[:4], out[5], physics_only=plugin or not c["walk"])
        assert ref["transitions"] == rep["transitions"] == 16 * 8
        assert not ref["unwitnessed"] and not rep["unwitnessed"], (ref["unwitnessed"], rep["unwitnessed"])
        for key, r in (("ref", ref), ("emu", rep)):
            tot[key][0] += r["witnessed"]
            tot[key][1] += r["transitions"]
        worst = max(worst, rep["direct_worst"])
    print(f"CONTACT {name} plugin={plugin}: witnessed emulator {tot['emu'][0]} / {tot['emu'][1]}, fp32 oracle under 1 ulp {tot['ref'][0]} / {tot['ref'][1]}, "
          f"worst direct {worst:.4f}")
    assert tot["ref"][0] <= Z.REFERENCE_CAP * tot["ref"][1], tot
    assert tot["emu"][0] <= Z.WITNESS_CAP * tot["emu"][1], tot


def test_two_trees_falling_case():
    """The case behind the divergence that prompted these tests (emulator, capacity-dimension path, against fp64: q 4.2e-4, qd 8.4e-2
    where the fp32 oracle has 5.4e-7, 5.8e-5).  Its cause was no solver knife edge: that path evaluated the capsule-capsule slots between
    the two trees with the plane-capsule formula, from the first step in which one came inside its margin.  On the plugin instantiation,
    which has the narrow phases: the emulator's distance from the fp64 oracle is the fp32 oracle's own at every step (within a factor 2),
    and every transition passes conftest.TOL directly -- no witness."""
    c = Z.load("two_trees", "position", N=Z.CONTACT_B - 1, H=Z.CONTACT_T - 1)
    model = c["model"]
    o64, o32 = Z.oracles(c)
    q, v, us = Z.falling_case(c)
    d = o64.forward_dump(q, v)
    assert (d["con_dist"][c["md"]["con_kind"] == 4] < 0).sum() >= 1, "no capsule-capsule candidate touches at the start"
    s0 = o32.env_reset(q, v)[0]
    out = _emu(c, True).rollout(s0, us, check_races=True, trace=True)
    r64, r32 = o64.rollout(s0, us), o32.rollout(s0, us)
    for t in range(Z.CONTACT_T):
        for k, what in ((1, "q"), (2, "qd")):
            e_emu, e_32 = np.abs(out[k][:, t] - r64[k][:, t]).max(), np.abs(r32[k][:, t] - r64[k][:, t]).max()
            print(f"FALLING step {t} {what}: emulator - fp64 {e_emu:.3e}, fp32 oracle - fp64 {e_32:.3e}")
            assert e_emu <= 2 * e_32 + 1e-6, (t, what, e_emu, e_32)
    rep = Z.contact_gate(c, o32, s0, us, out[:4], out[5], physics_only=True)
    assert rep["direct"] == rep["transitions"] == 128, rep


# ------------------------------------------------------------------------------------------------------------------ refusals
def _with(name, old, new, tmp_path, count=1):
    text = open(Z.xml_path(name)).read()
    assert text.count(old) == count, (old, text.count(old))
    path = tmp_path / (name + "_variant.xml")
    path.write_text(text.replace(old, new))
    return str(path)


def test_implicit_damping_is_refused_before_any_context(tmp_path):
    """damping > 0 without <flag eulerdamp="disable"/> compiles with eulerdamp = 1, which the pyramidal kernels do not integrate:
    check_model, build_plugin and CustomEnv.__init__ say so, naming the flag; the emulator answers DIAL_ERR_UNSUPPORTED as dial_create
    (whose own message stays) and dial_create_plugin (the same function body) do."""
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import build_plugin, check_model
    path = _with("chain_mixed", '<flag eulerdamp="disable"/>', "", tmp_path)
    md = mjcf.compile_mjcf(path)
    assert md["eulerdamp"] == 1
    for refuse in (lambda: check_model(md), lambda: build_plugin(md, Z.REWARD), lambda: Z.env_class(path)(Z.ZooConfig())):
        with pytest.raises(DialHipError, match=r'eulerdamp="disable"'):
            refuse()
    c = Z.load("chain_mixed")
    with pytest.raises(AssertionError, match=f"rc={UNSUPPORTED}"):
        Emu(_abi.make_model(md), c["otask"], c["cfg"], path=1).env_reset(c["env"]._init_q, np.zeros(9))
    from dial_mpc_amd._lib import _CSRC
    text = open(os.path.join(_CSRC, "dial_hip.hip")).read()
    assert "dial_create: eulerdamp is only supported on the elliptic-cone instantiations" in text


def test_thirteen_dof_path_is_refused(tmp_path):
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import check_model
    md = mjcf.compile_mjcf(Z.deep_chain_7(tmp_path))
    assert md["nv"] == 13
    with pytest.raises(DialHipError, match=r"body 'l7' is moved by 13 dofs.*hold 12"):
        check_model(md)
    c = Z.load("deep_chain")
    assert Emu(_abi.make_model(md), c["otask"], c["cfg"], path=1).derived()["rc"] == UNSUPPORTED
    assert Emu(c["model"], c["otask"], c["cfg"], path=1).derived()["rc"] == 0   # twelve: the limit itself


def test_two_actuators_on_one_dof_are_refused(tmp_path):
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import check_model
    path = _with("chain_mixed", '<motor name="swing_motor" joint="swing"', '<motor name="swing_motor" joint="rail"', tmp_path)
    md = mjcf.compile_mjcf(path)
    with pytest.raises(DialHipError, match=r"actuators 'rail_motor' and 'swing_motor' both drive dof 6.*one actuator per dof"):
        check_model(md)
    c = Z.load("chain_mixed")
    assert Emu(_abi.make_model(md), c["otask"], c["cfg"], path=1).derived()["rc"] == UNSUPPORTED


def test_contact_pair_element_is_not_dropped_silently(tmp_path):
    """compile_mjcf used to ignore <contact><pair>: no entry in the contact list, no message."""
    path = _with("chain_mixed", "<actuator>", '<contact><pair geom1="floor" geom2="tip_ball" condim="3"/></contact>\n  <actuator>', tmp_path)
    with pytest.raises(NotImplementedError, match=r"<contact><pair>"):
        mjcf.compile_mjcf(path)


def test_fixed_arm_under_torque_control_needs_a_law():
    with pytest.raises(ValueError, match=r"joint 0 is not a free base joint"):
        Z.env_class(Z.xml_path("fixed_arm"))(Z.ZooConfig(leg_control="torque"))
    Z.env_class(Z.xml_path("chain_mixed"))(Z.ZooConfig(leg_control="torque"))   # actuators on qpos 7, 8, 9: the 7 + a convention


def test_walk_task_validity():
    """The Go2 walk task (the capacity-dimension kernel's built-in kind) reads nothing outside the model for the two models with four
    sites, and is no valid task for the others."""
    for name in Z.MODELS:
        c = Z.load(name)
        why = Z.walk_task_reads_in_range(c["model"], c["otask"])
        assert (why is None) == (name in Z.WALK), (name, why)


# ------------------------------------------------------------------------------------------------------------------ resolving power
def _tilt_slide_axis(model, task):
    ax = np.array([float(x) for x in model.jnt_axis[1]])
    assert model.jnt_type[1] == K["DIAL_JNT_SLIDE"]
    n = np.cross(ax, [0.0, 1.0, 0.0])
    n /= np.linalg.norm(n)
    new = np.cos(1e-3) * ax + np.sin(1e-3) * n
    for k in range(3):
        model.jnt_axis[1][k] = new[k]


def _rotate_body_quat(model, task):
    q = np.array([float(x) for x in model.body_quat[4]])
    r = np.array([np.cos(5e-4), 0.0, 0.0, np.sin(5e-4)])   # 1e-3 rad about z
    new = mjcf.quat_mul(q, r)
    for k in range(4):
        model.body_quat[4][k] = new[k]


def _move_anchor(model, task):
    model.jnt_pos[2][0] = model.jnt_pos[2][0] + 1e-4


def _gear(model, task):
    assert model.act_gear[0] == 2.0
    model.act_gear[0] = model.act_gear[0] * (1 + 1e-3)


CHANGES = {"slide axis tilted by 1e-3 rad": _tilt_slide_axis, "body_quat[4] rotated by 1e-3 rad": _rotate_body_quat,
           "jnt_pos[2][0] + 1e-4 m": _move_anchor, "act_gear[0] x (1 + 1e-3)": _gear}


@pytest.mark.parametrize("change", list(CHANGES))
def test_resolving_power(change):
    """The fp32 oracle of chain_mixed with ONE constant changed, through the class-F gate against the unchanged pair: it must leave
    the gate by a ratio well above 1 (asserted: > 4, i.e. 32 x the fp32 oracle's own distance from fp64).  Measured worst ratios: slide
    axis 412, body_quat 58, anchor 256, gear under torque control (default gains kp 30, kd 1) 15.9."""
    control = "torque" if "gear" in change else "position"   # (under position control the motor's force is a small joint angle)
    c = Z.load("chain_mixed", control)
    model, task, cfg = c["model"], c["otask"], c["cfg"]
    o64, o32 = Z.oracles(c)
    m2, t2 = type(model).from_buffer_copy(model), type(task).from_buffer_copy(task)
    CHANGES[change](m2, t2)
    bad = O.Oracle(m2, t2, cfg, np.float32)
    q, v, us = Z.smooth_cases("chain_mixed", control)
    st = S.with_steps(S.reset_states(o32, q, v))
    r64, r32 = S.rollout_refs(o64, o32, st, us)
    got = tuple(np.stack([bad.rollout(s, u)[k] for s, u in zip(st, us)]).astype(np.float64) for k in range(4))
    gate = S.Gate("chain_mixed", "F", "resolving", change)
    gate.rollout_blocks(model, got, r64, r32)
    quantity, step, err, tol, ratio = gate.worst()
    print(f"RESOLVING {change}: worst block {quantity} step {step}: err {err:.3e} / tol {tol:.3e} = {ratio:.1f}")
    assert ratio > 4.0, f"{change}: worst ratio {ratio:.3f}"
