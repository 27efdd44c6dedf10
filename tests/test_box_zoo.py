"""The box zoo of tests/box_zoo_cases.py without a GPU: what mjcf.compile_mjcf makes of box geoms that are offset and rotated in their
body frames, the oracle's box geometry on whole models against an independent NumPy pose composition and brute force, the host wave
emulator on each model's plugin instantiation (in the air under smooth_ref's rule, in contact per transition with the race check, the
contact geometry through the probe reward), and the refusals: a model one body short of the box-box polygon scratch, and a box margin
that reaches the parking distance -- both from the emulator, and from check_model / build_plugin / CustomEnv.__init__ before any compile.

Box margins: a resting box hovers INSIDE its margin (the contact force starts at dist < margin; measured 1.9 mm at margin 2 mm), so a
slot with con_dist < 0 at rest needs margin 0.  Only box_limbs' foot pad carries one (1 mm)."""
import numpy as np
import pytest

import box_zoo_cases as B
import emu_lib
import smooth_ref as S
import synthetic_cases as Z
from dial_mpc_amd import _abi, mjcf
from emu_lib import Emu
from plugin_cases import F
from test_box_collisions import _max_separation, _segment_box_distance, _support_sep, box_closest

K = _abi.MACROS
UNSUPPORTED = K["DIAL_ERR_UNSUPPORTED"]
IU, IREW = K["DIAL_INFO_USER"], K["DIAL_INFO_REWARD"]


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


# ------------------------------------------------------------------------------------------------------------------ the compiler
# name -> dims (nq, nv, nu, nbody, njnt, ngeom, nsite, ncon, nlim, nfri, nefc), geom names in compiled order, body names,
#         boxes {geom: (body, half sizes, geom_pos, geom_quat as written in the MJCF)}, contact list [(kind, sub, geom1, geom2)], margins
PB, SB, CB, BB = 5, 6, 7, 8
TABLE = {
    "box_limbs": dict(
        dims=(18, 16, 4, 7, 6, 7, 0, 22, 4, 0, 92),
        geoms=["floor", "trunk_slab", "shin_l_rod", "foot_l_pad", "foot_r", "cargo_block", "cargo_ball"],
        bodies=["world", "trunk", "thigh_l", "shin_l", "thigh_r", "shin_r", "cargo"],
        boxes={"trunk_slab": ("trunk", (0.14, 0.07, 0.04), (0.01, 0.005, 0.002), (0.9840, 0.0262, 0.0046, 0.1735)),
               "foot_l_pad": ("shin_l", (0.03, 0.035, 0.025), (0.165, 0.0, -0.01), (0.9848, 0.0868, 0.1302, 0.0751)),
               "cargo_block": ("cargo", (0.06, 0.03, 0.02), (0.0437, 0.0263, -0.021), (0.9659258, 0.1830127, 0.1830127, 0.0))},
        contacts=[(0, 0, "floor", "foot_r"), (0, 0, "floor", "cargo_ball"), (1, 0, "floor", "shin_l_rod"), (2, 0, "floor", "shin_l_rod")]
        + [(PB, k, "floor", g) for g in ("trunk_slab", "foot_l_pad", "cargo_block") for k in range(4)]
        + [(3, 0, "cargo_ball", "shin_l_rod"), (SB, 0, "cargo_ball", "trunk_slab"), (SB, 0, "cargo_ball", "foot_l_pad"),
           (SB, 0, "foot_r", "cargo_block"), (CB, 0, "shin_l_rod", "cargo_block"), (CB, 1, "shin_l_rod", "cargo_block")],
        margin={"foot_l_pad": 0.001}),
    "box_pair": dict(
        dims=(18, 16, 4, 12, 6, 5, 4, 15, 4, 0, 64),
        geoms=["floor", "base_bar", "tray_slab", "foot_ball", "cargo_plank"],
        bodies=["world", "base", "pod_a", "pod_b", "arm", "tray", "pod_c", "leg", "foot", "pod_d", "cargo", "pod_e"],
        boxes={"tray_slab": ("tray", (0.08, 0.07, 0.03), (0.10, 0.01, -0.015), (0.9751, 0.0212, 0.0436, 0.2162)),
               "cargo_plank": ("cargo", (0.10, 0.04, 0.02), (0.02, -0.01, 0.01), (0.9396926, 0.0, 0.2418448, 0.2418448))},
        contacts=[(0, 0, "floor", "foot_ball"), (1, 0, "floor", "base_bar"), (2, 0, "floor", "base_bar")]
        + [(PB, k, "floor", g) for g in ("tray_slab", "cargo_plank") for k in range(4)] + [(BB, k, "tray_slab", "cargo_plank") for k in range(4)],
        margin={}),
    "box_self": dict(
        dims=(11, 10, 4, 6, 5, 7, 0, 18, 4, 0, 76),
        geoms=["floor", "base_slab", "a1_rod", "a2_bar", "b1_rod", "b2_rod", "b2_tip"],
        bodies=["world", "base", "a1", "a2", "b1", "b2"],
        boxes={"base_slab": ("base", (0.10, 0.08, 0.03), (-0.01, 0.004, 0.001), (0.9914, 0.0152, 0.0087, 0.1299)),
               "a2_bar": ("a2", (0.06, 0.015, 0.02), (0.075, 0.002, 0.0), (0.9950, 0.0868, 0.0076, 0.0436))},
        contacts=[(0, 0, "floor", "b2_tip")] + [(k, 0, "floor", g) for g in ("a1_rod", "b1_rod", "b2_rod") for k in (1, 2)]
        + [(PB, k, "floor", g) for g in ("base_slab", "a2_bar") for k in range(4)]
        + [(SB, 0, "b2_tip", "a2_bar"), (CB, 0, "b2_rod", "a2_bar"), (CB, 1, "b2_rod", "a2_bar")],
        margin={}),
}


@pytest.mark.parametrize("name", B.MODELS)
def test_compiled_box_tables_and_contact_list(name):
    md = mjcf.compile_mjcf(Z.xml_path(name))
    t = TABLE[name]
    assert tuple(int(md[k]) for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "nsite", "ncon", "nlim", "nfri", "nefc")) == t["dims"]
    assert md["names"]["geom"] == t["geoms"] and md["names"]["body"] == t["bodies"]
    assert md["cone"] == 0 and md["eulerdamp"] == 0 and abs(md["timestep"] - 0.005) < 1e-12 and md["act_isposition"].tolist() == [1] * 4
    boxes = [g for g in range(md["ngeom"]) if md["geom_type"][g] == mjcf.GEOM_BOX]
    assert [t["geoms"][g] for g in boxes] == list(t["boxes"])
    for g in boxes:
        body, half, pos, quat = t["boxes"][t["geoms"][g]]
        assert t["bodies"][int(md["geom_bodyid"][g])] == body
        assert np.array_equal(md["geom_size"][g], half) and np.array_equal(md["geom_pos"][g], pos)
        assert np.allclose(md["geom_quat"][g], _unit(quat), rtol=0, atol=1e-15)
        assert not np.allclose(_unit(quat), [1, 0, 0, 0], atol=1e-2) and np.abs(pos).max() > 0, "the geom frame is the body frame"
    got = [(int(k), int(s), t["geoms"][int(a)], t["geoms"][int(b)]) for k, s, a, b in zip(md["con_kind"], md["con_sub"], md["con_geom1"], md["con_geom2"])]
    assert got == t["contacts"]
    for c, (_, _, a, b) in enumerate(got):
        assert md["con_margin"][c] == max(t["margin"].get(a, 0.0), t["margin"].get(b, 0.0))
        assert t["bodies"][int(md["con_body1"][c])] == (t["boxes"][a][0] if a in t["boxes"] else t["bodies"][int(md["geom_bodyid"][t["geoms"].index(a)])])
    assert md["ncon"] <= 56 and md["nefc"] <= K["DIAL_MAX_EFC"]
    _abi.make_model(md)


def test_what_each_box_model_is_for():
    md = {n: B.load(n)["md"] for n in B.MODELS}
    lim, pair, slf = md["box_limbs"], md["box_pair"], md["box_self"]
    kinds = lambda m: sorted(set(np.asarray(m["con_kind"]).tolist()))   # noqa: E731
    assert kinds(lim) == [0, 1, 2, 3, PB, SB, CB] and kinds(pair) == [0, 1, 2, PB, BB] and kinds(slf) == [0, 1, 2, PB, SB, CB]
    # box_limbs: plane-box from three bodies, one of them two joints deep; a second free body
    assert sorted({int(b) for k, b in zip(lim["con_kind"], lim["con_body2"]) if k == PB}) == [1, 3, 6]
    assert lim["body_depth"][3] == 3 and lim["jnt_type"].tolist().count(mjcf.JNT_FREE) == 2
    # box_pair: the polygon scratch fits exactly; the pair joins a jointed limb body and the second free body; walk task valid
    nbb = int((np.asarray(pair["con_kind"]) == BB).sum())
    assert nbb == 4 and 6 * pair["nv"] + 12 * pair["nbody"] == 60 * nbb == 240
    bb = [(int(a), int(b)) for k, a, b in zip(pair["con_kind"], pair["con_body1"], pair["con_body2"]) if k == BB]
    assert bb == [(5, 10)] * 4 and pair["body_jntnum"][5] == 1 and pair["body_depth"][5] == 3 and pair["body_rootid"][10] == 10
    assert pair["body_jntnum"].tolist().count(0) == 6   # the world and five welded pods
    c = B.load("box_pair")
    assert Z.walk_task_reads_in_range(c["model"], c["otask"]) is None
    for n in ("box_limbs", "box_self"):
        assert Z.walk_task_reads_in_range(B.load(n)["model"], B.load(n)["otask"]) is not None
    # box_self: one tree; both self-contacts join bodies with shared ancestors that are neither parent nor child
    assert slf["body_rootid"].tolist() == [0, 1, 1, 1, 1, 1]
    own = [(int(a), int(b)) for a, b in zip(slf["con_body1"], slf["con_body2"]) if a != 0]
    assert own == [(5, 3)] * 3 and slf["body_parent"][5] == 4 and slf["body_parent"][3] == 2 and slf["body_parent"][4] == slf["body_parent"][2] == 1


def test_excluded_pairs_are_absent(tmp_path):
    """box_self: the parent-child rule drops (a1_rod, a2_bar), <contact><exclude> drops (base_slab, a2_bar) -- both pass the contype /
    conaffinity filter, and the second appears (as the model's only box-box pair) once the exclude element is taken out."""
    md = B.load("box_self")["md"]
    names = md["names"]["geom"]
    pairs = {(names[int(a)], names[int(b)]) for a, b in zip(md["con_geom1"], md["con_geom2"])}
    assert ("a1_rod", "a2_bar") not in pairs and ("base_slab", "a2_bar") not in pairs and BB not in md["con_kind"].tolist()
    text = open(Z.xml_path("box_self")).read()
    assert text.count('<exclude body1="base" body2="a2"/>') == 1
    p = tmp_path / "box_self_all.xml"
    p.write_text(text.replace('<exclude body1="base" body2="a2"/>', ""))
    m2 = mjcf.compile_mjcf(str(p))
    got = [(int(k), names[int(a)], names[int(b)]) for k, a, b in zip(m2["con_kind"], m2["con_geom1"], m2["con_geom2"]) if k == BB]
    assert got == [(BB, "base_slab", "a2_bar")] * 4 and m2["ncon"] == md["ncon"] + 4
    assert ("a1_rod", "a2_bar") not in {(names[int(a)], names[int(b)]) for a, b in zip(m2["con_geom1"], m2["con_geom2"])}


# ------------------------------------------------------------------------------------------------------------------ oracle geometry
def _sphere_box(c, R, h, s, r):
    q, inside = box_closest(c, R, h, s)
    if not inside:
        return np.linalg.norm(q - s) - r
    return -(np.min(h - np.abs(R.T @ (s - c))) + r)


def _verts(c, R, h):
    return np.array([c + R @ (np.array([(i & 1) * 2 - 1, ((i >> 1) & 1) * 2 - 1, ((i >> 2) & 1) * 2 - 1]) * h) for i in range(8)])


@pytest.mark.parametrize("name", B.MODELS)
def test_oracle_box_geometry_against_brute_force(name):
    """Every box slot the fp64 oracle's forward_dump puts within 1 cm, in the 32 geometry states (those of the GPU test): con_dist against
    the brute-force signed distance of tests/test_box_collisions.py at ITS tolerances, on geom poses composed here in NumPy fp64 --
    xpos + R(xquat) geom_pos, xquat * geom_quat -- from the dump's body frames and the model struct's fp32 constants; each tolerance is the file's plus box_zoo_cases.pose_slack (~1e-9 m: fp32 geom_quats are not exactly unit).  plane-box: the sub-th lowest vertex (1e-12); sphere-box:
    the clamp (1e-12); capsule-box: the minimised segment distance for sub 0 (2e-6), an end sphere for sub 1 (1e-9); box-box: the
    oracle's narrow phase on the NumPy poses reproduces the slot (1e-9: the pose composition), its normal's support separation is within
    5 % + 2e-5 of the sampled maximum, the first candidate is not deeper than that slab, and every live point lies between the two
    surfaces (1e-6)."""
    c, qs, vs, r64, _ = B.geometry_reference(name)
    md = c["md"]
    o64, _ = Z.oracles(c)
    kind, sub = np.asarray(md["con_kind"]).ravel(), np.asarray(md["con_sub"]).ravel()
    g1, g2 = np.asarray(md["con_geom1"]).ravel(), np.asarray(md["con_geom2"]).ravel()
    size = B.geom_constants(c["model"])[2]
    rng = np.random.default_rng(3)
    seen = {k: 0 for k in B.BOX_KINDS}
    for s in range(len(qs)):
        d = r64[s]
        gw = B.geom_world(md, *B.body_frames(d), model=c["model"])
        dist, pos = d["con_dist"], np.asarray(d["con_pos"]).reshape(-1, 3)
        for i in np.flatnonzero(np.isin(kind, B.BOX_KINDS) & (dist < B.NEAR)):
            (ca, Ra), (cb, Rb), ha, hb = gw[g1[i]], gw[g2[i]], size[g1[i]], size[g2[i]]
            k = int(kind[i])
            seen[k] += 1
            where = (name, s, int(i), B.KIND_NAME[k], int(sub[i]))
            slack = B.pose_slack(c["model"], int(g1[i]), int(g2[i]))
            if k == B.PLANE_BOX:
                heights = np.sort((_verts(cb, Rb, hb) - ca) @ Ra[:, 2])
                assert np.isclose(dist[i], heights[sub[i]], rtol=0, atol=1e-12 + slack), (where, dist[i], heights[sub[i]])
            elif k == B.SPHERE_BOX:
                assert np.isclose(dist[i], _sphere_box(cb, Rb, hb, ca, ha[0]), rtol=0, atol=1e-12 + slack), where
            elif k == B.CAPSULE_BOX:
                r, hl = ha[0], ha[1]
                e0, e1 = ca - Ra[:, 2] * hl, ca + Ra[:, 2] * hl
                pts = e0 + np.linspace(0, 1, 2001)[:, None] * (e1 - e0)
                inside = np.all(np.abs((pts - cb) @ Rb) <= hb, axis=1)
                through = inside.any()
                if inside.all():      # (the whole axis inside the box: plain end spheres; test_box_collisions passes over it too)
                    continue
                if sub[i] == 0:
                    want = -r if through else _segment_box_distance(cb, Rb, hb, e0, e1) - r
                    assert np.isclose(dist[i], want, rtol=0, atol=2e-6 + slack), (where, dist[i], want)
                elif not through:
                    ends = [_sphere_box(cb, Rb, hb, e, r) for e in (e0, e1)]
                    assert min(abs(dist[i] - ends[0]), abs(dist[i] - ends[1])) < 1e-9 + slack, (where, dist[i], ends)
            else:
                d_np, p_np, f_np = o64.box_contact(B.BOX_BOX, int(sub[i]), (ca, Ra, ha), (cb, Rb, hb))
                assert abs(d_np - dist[i]) <= 1e-9 + slack and np.abs(p_np - pos[i]).max() <= 1e-9 + slack, (where, d_np, dist[i])
                n = f_np[0]
                for (c_, R_, h_, sg) in ((ca, Ra, ha, +1.0), (cb, Rb, hb, -1.0)):
                    l = R_.T @ (pos[i] - sg * n * dist[i] * 0.5 - c_)
                    assert np.max(np.abs(l) - h_) < 1e-6, (where, float(np.max(np.abs(l) - h_)))
                if sub[i] == 0:
                    smax, sep_n = _max_separation(ca, Ra, ha, cb, Rb, hb, rng), _support_sep(ca, Ra, ha, cb, Rb, hb, n)
                    assert sep_n >= smax - 0.05 * abs(smax) - 2e-5 and sep_n <= smax + 1e-9, (where, sep_n, smax)
                    assert np.isclose(dist[i], sep_n, atol=1e-9) or dist[i] >= sep_n - 1e-9, (where, dist[i], sep_n)
    for k in B.BOX_KINDS:
        assert (seen[k] >= 8) == (k in kind.tolist()), (name, B.KIND_NAME[k], seen[k])


@pytest.mark.parametrize("name", B.MODELS)
def test_geometry_states_need_no_witness_from_the_fp32_oracle(name):
    """The inputs of the geometry gate: the fp32 oracle's own cdist / cpos pass it without a single witness (the states sit on no knife
    edge), and no per-kind tolerance is looser than 1e-5 (a state on a discontinuity would inflate the tolerance of its kind)."""
    c, qs, vs, r64, r32 = B.geometry_reference(name)
    cd = np.array([r["con_dist"] for r in r32])
    cp = np.array([np.asarray(r["con_pos"]).reshape(-1, 3) for r in r32])
    rep = B.geometry_gate(name, cd, cp, "fp32 oracle")
    assert rep["witnessed"] == 0 and not rep["unwitnessed"]
    assert max(t for t, _ in rep["tol"].values()) <= 1e-5, rep["tol"]


def test_every_box_kind_touches_in_a_start_state():
    for name in B.MODELS:
        c, q, v, us, labels = B.contact_cases(name)
        touch = B.touching_kinds(c, q, v)
        for k in B.BOX_KINDS:
            if k in np.asarray(c["md"]["con_kind"]).tolist():
                assert any(t[k] > 0 for t in touch), (name, B.KIND_NAME[k], touch)
        assert touch[0][B.PLANE_BOX] > 0, "state 0: a box resting on the floor"
    assert B.touching_kinds(*B.contact_cases("box_pair")[:3])[0][B.BOX_BOX] > 0, "the plank lies on the tray"


# ------------------------------------------------------------------------------------------------------------------ emulator
def _emu(c, plugin=True):
    if not plugin:
        return Emu(c["model"], c["otask"], c["cfg"], path=1)
    defines, tag = emu_lib.user_variant(c["md"], B.PROBE)
    e = Emu(c["model"], c["ptask"], c["cfg"], path=0, defines=defines, tag=tag)
    e.set_user_params(B.PARAMS)
    return e


BUILDS = [(n, True) for n in B.MODELS] + [("box_pair", False)]
IDS = [f"{n}-{'plugin' if p else 'capacity'}" for n, p in BUILDS]


@pytest.mark.parametrize("name,plugin", BUILDS, ids=IDS)
def test_emulator_in_the_air_at_rounding_level(name, plugin):
    """Class F under smooth_ref's rule, unchanged and with no additive term: env_reset of 16 states, five env steps of 4 states x 16
    rollouts against the fp64 oracle; the race check on the first case.  box_pair also on the capacity dimensions (path 1) with the walk
    task's rewards."""
    c = B.load(name)
    model = c["model"]
    o64, o32 = Z.oracles(c)
    emu = _emu(c, plugin)
    q16, v16, _ = S.smooth_states(c["env"], model, "F", 16, seed=21)
    gate = S.Gate(name, "F", "reset+rollout", f"emulator-{'plugin' if plugin else 'capacity'}")
    gate.reset_blocks(model, o64, o32, q16, v16, np.array([emu.env_reset(a, b, check_races=False)[0] for a, b in zip(q16, v16)]))
    q, v, us = B.smooth_cases(name)
    states = S.with_steps(np.array([emu.env_reset(q[i], v[i], check_races=(i == 0))[0] for i in range(4)]))
    for i in range(4):
        S.assert_stays_free(model, c["otask"], o64, states[i], us[i])
    got = [emu.rollout(states[i], us[i], check_races=(i == 0)) for i in range(4)]
    got = tuple(np.stack([g[k] for g in got]) for k in range(4))
    gate.rollout_blocks(model, got, *S.rollout_refs(o64, o32, states, us), rewards=c["walk"] and not plugin)
    gate.check()
    print(f"WORST {name} plugin={plugin}: {gate.worst()}")


@pytest.mark.parametrize("name,plugin", BUILDS, ids=IDS)
def test_emulator_in_contact_per_transition(name, plugin):
    """Per start state of box_zoo_cases.contact_cases: 16 rollouts x 8 control steps, every transition from the emulator's own traced
    state against the fp32 oracle at conftest.TOL (transition_parity); no transition without a witness, witnessed share <= 10 %; the
    race check on the first rollout launch of each state.  First the reference: the fp32 oracle against itself under 1 ulp of jitter needs
    witnesses for <= 5 % (this is also the check that keeps box_pair's leaning plank: no flush face on a face)."""
    c, q, v, us, labels = B.contact_cases(name)
    model = c["model"]
    ni = model.nq + 2 * model.nv
    _, o32 = Z.oracles(c)
    emu = _emu(c, plugin)
    tot, worst = dict(ref=[0, 0], emu=[0, 0]), 0.0
    for i in range(len(q)):
        s0 = o32.env_reset(q[i], v[i])[0]
        ref = Z.contact_gate(c, o32, s0, us[i], *Z.jittered_oracle_run(o32, s0, us[i], ni, seed=5 + i), physics_only=False)
        out = emu.rollout(s0, us[i], check_races=True, trace=True)
        rep = Z.contact_gate(c, o32, s0, us[i], out[:4], out[5], physics_only=plugin or not c["walk"])
        assert ref["transitions"] == rep["transitions"] == 16 * 8
        assert not ref["unwitnessed"] and not rep["unwitnessed"], (labels[i], ref["unwitnessed"], rep["unwitnessed"])
        for key, r in (("ref", ref), ("emu", rep)):
            tot[key][0] += r["witnessed"]
            tot[key][1] += r["transitions"]
        worst = max(worst, rep["direct_worst"])
        print(f"CONTACT {name} plugin={plugin} state {i} ({labels[i]}): witnessed emulator {rep['witnessed']}, reference {ref['witnessed']} of 128")
    print(f"CONTACT {name} plugin={plugin}: witnessed emulator {tot['emu'][0]} / {tot['emu'][1]}, fp32 oracle under 1 ulp {tot['ref'][0]} / {tot['ref'][1]}, "
          f"worst direct {worst:.4f}")
    assert tot["ref"][0] <= Z.REFERENCE_CAP * tot["ref"][1], tot
    assert tot["emu"][0] <= Z.WITNESS_CAP * tot["emu"][1], tot


def _emu_geometry(name, change=None):
    """cdist [32, ncon] / cpos [32, ncon, 3] of the emulator's plugin instantiation in the geometry states: per state one env.step (one
    physics step per control step) per probed word, the probe's selector in info_user[0:2].  change(model): edit a copy of the struct."""
    c1 = dict(B.load(name, frames=1))
    if change is not None:
        c1["model"] = type(c1["model"]).from_buffer_copy(c1["model"])
        change(c1["model"])
    c, qs, vs = B.geometry_states(name)
    model = c1["model"]
    ni, ncon = model.nq + 2 * model.nv, model.ncon
    emu = _emu(c1)
    cdist, cpos = np.zeros((len(qs), ncon), np.float32), np.zeros((len(qs), ncon, 3), np.float32)
    act = np.zeros(model.nu, np.float32)
    for s in range(len(qs)):
        s0 = emu.env_reset(qs[s], vs[s], check_races=False)[0]
        assert np.array_equal(s0[model.nq:model.nq + model.nv], vs[s])
        s0[:model.nq] = qs[s]   # (env.reset normalises the quaternions; the probed state is the fp32 state itself)
        for field, n, dst in ((F["cdist"], ncon, cdist[s]), (F["cpos"], 3 * ncon, cpos[s].reshape(-1))):
            for i in range(n):
                st = s0.copy()
                st[ni + IU], st[ni + IU + 1] = field, i
                dst[i] = emu.env_step(st, act, check_races=(s == 0 and i == 0))[0][ni + IREW]
    return cdist, cpos


@pytest.mark.parametrize("name", B.MODELS)
def test_emulator_contact_geometry_through_the_probe(name):
    """The GPU test's geometry gate (box_zoo_cases.geometry_gate) on the emulator's plugin instantiation."""
    B.assert_geometry(B.geometry_gate(name, *_emu_geometry(name), "emulator"))


def test_geometry_gate_resolves_a_milliradian_in_a_geom_frame():
    """Power of the gate: box_limbs with the foot pad's geom_quat turned by 1e-3 rad about x in the struct the emulator gets (the
    oracle keeps the model).  30 um at the pad's corners against tolerances of 1e-6: live slots without a witness."""
    def turn(model):
        g = B.load("box_limbs")["md"]["names"]["geom"].index("foot_l_pad")
        q = B.quat_mul(np.array([float(x) for x in model.geom_quat[g]]), [np.cos(5e-4), np.sin(5e-4), 0.0, 0.0])
        for k in range(4):
            model.geom_quat[g][k] = q[k]
    got = _emu_geometry("box_limbs", turn)
    B.assert_geometry(B.geometry_gate("box_limbs", *_emu_geometry("box_limbs"), "emulator"))
    with pytest.raises(AssertionError):   # (a live slot without a witness, or a parked slot above the true separation)
        B.assert_geometry(B.geometry_gate("box_limbs", *got, "emulator, foot pad turned by 1e-3 rad"))


# ------------------------------------------------------------------------------------------------------------------ refusals
def _variant(name, old, new, tmp_path):
    text = open(Z.xml_path(name)).read()
    assert text.count(old) == 1, (old, text.count(old))
    path = tmp_path / (name + "_variant.xml")
    path.write_text(text.replace(old, new))
    return str(path)


def _refusers(md, path):
    from dial_mpc_amd.plugin import build_plugin, check_model
    return (lambda: check_model(md), lambda: build_plugin(md, B.PROBE), lambda: B.env_class(path)(B.BoxConfig()))


def test_one_body_short_of_the_polygon_scratch_is_refused(tmp_path, monkeypatch):
    """box_pair_short: four box-box candidates need 240 words, 6 * 16 + 12 * 11 = 228 are there.  The emulator answers
    DIAL_ERR_UNSUPPORTED on both dispatch paths (as dial_create: the count is the MODEL's, whatever the
    instantiation's arrays hold); check_model, build_plugin and CustomEnv.__init__ raise before any compile (no hipcc call), naming the
    candidates, the words needed and the words the model has.  box_pair, the exact fit, passes all of these."""
    import subprocess
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import check_model
    path = B.box_pair_short(tmp_path)
    md = mjcf.compile_mjcf(path)
    assert (md["nv"], md["nbody"], md["ncon"]) == (16, 11, 15)
    c = B.load("box_pair")
    q0 = c["env"]._init_q
    # (path 0 and path 1 of the default emulator build: the condition stands in front of every pyramidal instantiation's dispatch, a
    # plugin's included, so no emulator is built at the short model's dimensions to see it)
    for emu in (Emu(_abi.make_model(md), c["otask"], c["cfg"], path=1), Emu(_abi.make_model(md), c["otask"], c["cfg"], path=0)):
        with pytest.raises(AssertionError, match=f"rc={UNSUPPORTED}"):
            emu.env_reset(q0, np.zeros(16))
        with pytest.raises(AssertionError, match=f"rc={UNSUPPORTED}"):
            emu.rollout(np.zeros(emu.state_size, np.float32), np.zeros((1, 1, 4), np.float32))

    def no_compile(*a, **k):
        raise AssertionError(f"a subprocess was started before the refusal: {a[0]}")
    with monkeypatch.context() as mp:
        mp.setattr(subprocess, "run", no_compile)
        for refuse in _refusers(md, path):
            with pytest.raises(DialHipError, match=r"4 box-box candidate contacts.*need 240 words.*model has 228"):
                refuse()
    check_model(c["md"])
    B.env_class(Z.xml_path("box_pair"))(B.BoxConfig())
    _emu(c, True).env_reset(q0, np.zeros(16))
    _emu(c, False).env_reset(q0, np.zeros(16))
    from dial_mpc_amd._lib import _CSRC
    import os
    assert "dial_create: too many box-box candidate contacts for the polygon scratch" in open(os.path.join(_CSRC, "dial_hip.hip")).read()


def test_box_margin_at_the_parking_distance_is_refused(tmp_path, monkeypatch):
    """A box contact whose margin reaches DIAL_BOX_PARK_DIST (1 cm) would be activated with a parked candidate's placeholder values:
    refused like the scratch, naming the two geoms.  9 mm passes."""
    import subprocess
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import check_model
    c = B.load("box_limbs")
    path = _variant("box_limbs", 'margin="0.001"', 'margin="0.01"', tmp_path)
    md = mjcf.compile_mjcf(path)
    with pytest.raises(AssertionError, match=f"rc={UNSUPPORTED}"):
        Emu(_abi.make_model(md), c["ptask"], c["cfg"], path=0, **dict(zip(("defines", "tag"), emu_lib.user_variant(md, B.PROBE)))).env_reset(
            c["env"]._init_q, np.zeros(16))
    with monkeypatch.context() as mp:
        mp.setattr(subprocess, "run", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a subprocess was started before the refusal")))
        for refuse in _refusers(md, path):
            with pytest.raises(DialHipError, match=r"geoms 'floor' and 'foot_l_pad' has margin 0\.01 m.*margin < 0\.01 m"):
                refuse()
    ok = mjcf.compile_mjcf(_variant("box_limbs", 'margin="0.001"', 'margin="0.009"', tmp_path))
    check_model(ok)
    check_model(c["md"])
