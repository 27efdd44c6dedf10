"""Inputs and gates of the lane-local pins (tests/lane_cases): written ONCE as functions of (input rows, output words), applied to the
emulator build by tests/test_lane_emu.py and to the two device builds by tests/test_gpu_lane_cases.py.  Geometry is gated against
the fp64 oracle in generic position (G1) and against plain fp64 geometry in degenerate position (G2); the brute-force helpers are
those of tests/test_box_collisions.py, imported, not copied."""
import functools
import itertools
import json
import os

import numpy as np

import oracle as O
from conftest import setup_case
from test_box_collisions import (KIND_BOX_BOX, KIND_CAPSULE_BOX, KIND_PLANE_BOX, KIND_SPHERE_BOX, _max_separation, _q2m, _rand_quat,
                                 _segment_box_distance, _support_sep, box_closest, rand_rot)
from test_ls_bracket import _fkey, _reference

import lane_lib as L

KINDS = {"plane_box": (KIND_PLANE_BOX, 4), "sphere_box": (KIND_SPHERE_BOX, 1), "capsule_box": (KIND_CAPSULE_BOX, 2), "box_box": (KIND_BOX_BOX, 4)}
PARK = float(np.float32(0.01))       # DIAL_BOX_PARK_DIST
TOL_FLOOR = 1e-6                     # 8 ulp at 1 m
WITNESS_CAP = 0.01
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ rows and words
def q2m(q):
    """dm::quat_to_mat in fp64, [..., 4] -> [..., 3, 3] (the quaternion is NOT renormalised: both sides see the same matrix)."""
    q = np.asarray(q, np.float64)
    w, x, y, z = (q[..., k] for k in range(4))
    m = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def geom_rows(kind, nsub, pairs):
    """pairs of ((c1, q1, size1), (c2, q2, h2)) -> [len * nsub, 22] float32 rows, the subs of one pair next to each other."""
    rows = []
    for g1, g2 in pairs:
        body = np.concatenate([np.asarray(x, np.float64).ravel() for x in (*g1, *g2)])
        for sub in range(nsub):
            rows.append(np.concatenate([[kind, sub], body]))
    return np.array(rows).astype(F32)


def row_geoms(row):
    """(c1, q1, R1, s1), (c2, q2, R2, h2) of one row, fp64 values of the fp32 inputs."""
    r = np.asarray(row, np.float64)
    return (r[2:5], r[5:9], q2m(r[5:9]), r[9:12]), (r[12:15], r[15:19], q2m(r[15:19]), r[19:22])


def decode(out):
    """[n, 13] words -> dist [n], pos [n, 3], frame [n, 3, 3] as fp64."""
    f = np.ascontiguousarray(out).view(F32).astype(np.float64)
    return f[:, 0], f[:, 1:4], f[:, 4:13].reshape(-1, 3, 3)


@functools.lru_cache(maxsize=None)
def oracle(dtype_name):
    _dc, _env, model, task, cfg = setup_case("unitree_go2_trot", 8, 4)
    return O.Oracle(model, task, cfg, np.dtype(dtype_name).type)


def oracle_rows(rows, dtype_name="float64"):
    """The oracle on the same (fp32-rounded) inputs, as words-free arrays: dist, pos, frame."""
    orc = oracle(dtype_name)
    n = len(rows)
    d, p, f = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3, 3))
    r64 = np.asarray(rows, np.float64)
    m1, m2 = q2m(r64[:, 5:9]), q2m(r64[:, 15:19])
    for i in range(n):
        r = r64[i]
        d[i], p[i], f[i] = orc.box_contact(int(r[0]), int(r[1]), (r[2:5], m1[i], r[9:12]), (r[12:15], m2[i], r[19:22]))
    return d, p, f


# ------------------------------------------------------------------------------------------------------------------ G1 inputs
def g1_pairs(kind, n=1000):
    """The generator of test_box_collisions.test_kernel_narrow_phase_matches_the_oracle (seed 10 + kind)."""
    rng = np.random.default_rng(10 + kind)
    pairs = []
    for _ in range(n):
        c2, q2, h2 = rng.normal(size=3) * 0.2, _rand_quat(rng), rng.uniform(0.05, 0.5, 3)
        q1 = _rand_quat(rng)
        R2 = _q2m(q2)
        if kind == KIND_PLANE_BOX:
            c1, size1 = c2 - _q2m(q1)[:, 2] * rng.uniform(0.0, 0.6), np.array([0, 0, 0.05])
        elif kind == KIND_SPHERE_BOX:
            c1, size1 = c2 + R2 @ (rng.normal(size=3) * h2 * 1.2), np.array([rng.uniform(0.01, 0.1), 0, 0])
        elif kind == KIND_CAPSULE_BOX:
            c1, size1 = c2 + R2 @ (rng.normal(size=3) * h2 * 1.3), np.array([rng.uniform(0.01, 0.03), rng.uniform(0.03, 0.2), 0])
        else:
            size1 = rng.uniform(0.04, 0.3, 3)
            c1 = c2 + _q2m(_rand_quat(rng))[:, 0] * rng.uniform(0.05, 0.7)
        pairs.append(((c1, q1, size1), (c2, q2, h2)))
    return pairs


def m2q(R):
    """rotation matrix -> unit quaternion (w, x, y, z), fp64 (Shepperd's branches)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def edge_pairs(n=300, seed=77):
    """Box-box pairs whose closest features are two EDGES crossing at 30-90 degrees with a gap of -3 mm .. +3 mm along their common
    perpendicular: an edge of A (axis i, at a random corner of the other two axes), and the (+, +) edge along B's axis 0, whose outward
    diagonal looks back at A's."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        cA, RA, hA = rng.normal(size=3) * 0.1, rand_rot(rng), rng.uniform(0.05, 0.3, 3)
        hB = rng.uniform(0.05, 0.3, 3)
        i = int(rng.integers(3))
        j, k = (i + 1) % 3, (i + 2) % 3
        sj, sk = rng.choice([-1.0, 1.0], 2)
        u = RA[:, i]
        nrm = (sj * RA[:, j] + sk * RA[:, k]) / np.sqrt(2.0)            # outward diagonal of A's edge, perpendicular to u
        th = np.deg2rad(rng.uniform(30, 90)) * rng.choice([-1.0, 1.0])
        dB = np.cos(th) * u + np.sin(th) * np.cross(nrm, u)
        m = np.cross(dB, nrm)
        RB = np.stack([dB, (-nrm + m) / np.sqrt(2.0), (-nrm - m) / np.sqrt(2.0)], 1)
        pA = cA + sj * hA[j] * RA[:, j] + sk * hA[k] * RA[:, k]
        a, b = rng.uniform(-0.6, 0.6) * hA[i], rng.uniform(-0.6, 0.6) * hB[0]
        gap = rng.uniform(-0.003, 0.003)
        cB = pA + a * u + gap * nrm - b * dB - RB @ np.array([0.0, hB[1], hB[2]])
        pairs.append(((cA, m2q(RA), hA), (cB, m2q(RB), hB)))
    return pairs


def is_edge_contact(rows, d64, f64):
    """Per PAIR of box-box rows (4 subs): the fp64 oracle found one live candidate whose normal is no face normal of either box
    (the classification of test_box_box_depth_normal_and_points)."""
    res = []
    for p in range(0, len(rows), 4):
        (_, _, RA, _), (_, _, RB, _) = row_geoms(rows[p])
        n = f64[p, 0]
        live = int((d64[p:p + 4] < 0.5).sum())
        res.append(live == 1 and d64[p] < PARK and np.min(np.abs(np.abs(RA.T @ n) - 1)) > 1e-6 and np.min(np.abs(np.abs(RB.T @ n) - 1)) > 1e-6)
    return np.array(res)


@functools.lru_cache(maxsize=None)
def g1_cases(name):
    """rows, fp64 oracle (d, p, f), fp32 oracle (d, p, f), tolerance of one kind -- computed once per process and shared."""
    kind, nsub = KINDS[name]
    rows = geom_rows(kind, nsub, g1_pairs(kind))
    if kind == KIND_BOX_BOX:
        rows = np.concatenate([rows, geom_rows(kind, nsub, edge_pairs())])
    ref64, ref32 = oracle_rows(rows, "float64"), oracle_rows(rows, "float32")
    for a in (rows, *ref64, *ref32):
        a.setflags(write=False)
    return rows, ref64, ref32, reference_tolerance(kind, ref32, ref64)


# ------------------------------------------------------------------------------------------------------------------ G1 gates
def candidate_errors(kind, got, ref):
    """Per case: error of dist, of pos (live reference candidates only: ref dist <= 0.5), of frame[0], of frame rows 1-2 (only where
    the reference normal is off make_frame's switch at |n_y| = 0.5), and whether BOTH sides are parked (> 1 cm; never sphere-box)."""
    (d, p, f), (dr, pr, fr) = got, ref
    e_d = np.abs(d - dr)
    e_p = np.where(dr > 0.5, 0.0, np.abs(p - pr).max(1))
    e_n = np.abs(f[:, 0] - fr[:, 0]).max(1)
    ny = np.abs(fr[:, 0, 1])
    e_f = np.where(np.abs(ny - 0.5) <= 1e-3, 0.0, np.abs(f[:, 1:] - fr[:, 1:]).max((1, 2)))
    parked = (d > PARK) & (dr > PARK) if kind != KIND_SPHERE_BOX else np.zeros(len(d), bool)
    return e_d, e_p, e_n, e_f, parked


def reference_tolerance(kind, ref32, ref64):
    """8 x the worst error (dist, pos of live candidates) of the fp32 ORACLE against the fp64 oracle on the same cases, floor 1e-6.
    A case where the fp32 oracle itself takes another discrete choice (error beyond the suite's older 2e-5) would make the figure
    meaningless: there must be none on the chosen inputs."""
    e_d, e_p, _e_n, _e_f, parked = candidate_errors(kind, ref32, ref64)
    err = np.where(parked, 0.0, np.maximum(e_d, e_p))
    assert (err > 2e-5).sum() == 0, ("the fp32 oracle leaves the fp64 oracle on the chosen inputs", kind, int((err > 2e-5).sum()))
    return max(TOL_FLOOR, 8.0 * float(err.max())), float(err.max())


def close_to(kind, got, ref, tol):
    e_d, e_p, e_n, e_f, parked = candidate_errors(kind, got, ref)
    return parked | ((e_d <= tol) & (e_p <= tol) & (e_n <= 10 * tol) & (e_f <= 10 * tol))


def check_frames(f, tol, what):
    """orthonormal and right-handed in EVERY case"""
    g = np.abs(f @ f.transpose(0, 2, 1) - np.eye(3)).max((1, 2))
    assert np.all(g <= 10 * tol), (what, "frame not orthonormal", float(g.max()), int(np.argmax(g)))
    assert np.all(np.linalg.det(f) > 0.99), (what, "frame not right-handed")


def jittered(row, rng, copies=32, ulps=4):
    """copies of one row with every non-zero geometry word moved by <= ulps units in the last place"""
    x = np.repeat(np.asarray(row, F32)[None], copies, 0)
    bits = x.view(np.int32)
    delta = rng.integers(-ulps, ulps + 1, size=(copies, 20)).astype(np.int32)
    bits[:, 2:] += np.where(bits[:, 2:] != 0, delta, 0)
    return x


def face_sbest64(gA, gB):
    """the separation on the best of the six FACE axes and the bounding-sphere gap, fp64 (box_box's two broad phases)"""
    (cA, _, RA, hA), (cB, _, RB, hB) = gA, gB
    tw = cB - cA
    t, C = RA.T @ tw, RA.T @ RB
    sA = np.abs(t) - (hA + np.abs(C) @ hB)
    sB = np.abs(C.T @ t) - (hB + np.abs(C).T @ hA)
    return max(sA.max(), sB.max()), np.linalg.norm(tw) - np.linalg.norm(hA) - np.linalg.norm(hB)


def segment_box_distance64(gC, gB):
    """exact distance of the capsule's axis from the box: the squared distance is convex in t -- ternary search in fp64"""
    (ctr, _, Rc, size), (c, _, R, h) = gC, gB
    e0, e1 = ctr - Rc[:, 2] * size[1], ctr + Rc[:, 2] * size[1]
    l0, l1 = R.T @ (e0 - c), R.T @ (e1 - c)
    f = lambda t: np.linalg.norm(np.maximum(np.abs(l0 + t * (l1 - l0)) - h, 0.0))
    lo, hi = 0.0, 1.0
    for _ in range(200):
        a, b = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        if f(a) <= f(b):
            hi = b
        else:
            lo = a
    return f(0.5 * (lo + hi))


def capsule_parks64(gC, gB):
    """fp64 values of capsule_box's two broad phases: bounding-sphere gap and best slab separation"""
    (ctr, _, Rc, size), (c, _, R, h) = gC, gB
    r, hl = size[0], size[1]
    e0, e1 = ctr - Rc[:, 2] * hl, ctr + Rc[:, 2] * hl
    l0, l1 = R.T @ (e0 - c), R.T @ (e1 - c)
    lo, hi = np.minimum(l0, l1) - r, np.maximum(l0, l1) + r
    return np.linalg.norm(c - ctr) - (hl + r) - np.linalg.norm(h), max(-1.0, float(np.max(np.maximum(lo - h, -h - hi))))


def plane_lowest64(gP, gB):
    (pp, _, Rp, _), (c, _, R, h) = gP, gB
    n = Rp[:, 2]
    return (c - pp) @ n - np.abs(R.T @ n) @ h


_SEP_CACHE = {}
BRUTE_EVERY = 8


def true_separation_box_box(row, index):
    """A value that is AT MOST the true fp64 separation of two disjoint boxes: the best of the 15 separating axes (support-function
    separation along the six face normals and the nine edge-edge directions).  The true separation -- the maximum over ALL directions,
    which _max_separation searches by brute force at ~0.13 s a pair -- is never smaller, so a parked dist below this value + tol is
    below the true one + tol.  Every BRUTE_EVERY-th judged pair is run through _max_separation as well, which must not come out
    below the 15-axis value.  Cached per input row: the device builds and the emulator share the inputs."""
    key = np.asarray(row[2:], F32).tobytes()
    if key not in _SEP_CACHE:
        (cA, _, RA, hA), (cB, _, RB, hB) = row_geoms(row)
        axes = [RA[:, k] for k in range(3)] + [RB[:, k] for k in range(3)]
        axes += [np.cross(RA[:, i], RB[:, j]) for i in range(3) for j in range(3)]
        sep = max(_support_sep(cA, RA, hA, cB, RB, hB, s * a / np.linalg.norm(a)) for a in axes if np.linalg.norm(a) > 1e-9 for s in (1.0, -1.0))
        if index % BRUTE_EVERY == 0:
            brute = _max_separation(cA, RA, hA, cB, RB, hB, np.random.default_rng(1))
            assert brute >= sep - 1e-9, ("_max_separation below the 15-axis separation", brute, sep)
        _SEP_CACHE[key] = sep
    return _SEP_CACHE[key]


def parked_contract(kind, rows, got, tol, margin=1e-4):
    """The header comment of box_collide.h for candidates the kernel parks (dist beyond DIAL_BOX_PARK_DIST, pair not touching): a parked dist
    is > DIAL_BOX_PARK_DIST and at most the true fp64 separation + tol; where the fp64 value of a broad-phase quantity is clear of the
    threshold by `margin`, candidates sub >= 1 of capsule-box and box-box are exactly 1.f.  Returns the indices it judged."""
    d = got[0]
    judged = []
    if kind == KIND_SPHERE_BOX:
        return judged
    for i in np.nonzero(d > PARK)[0]:
        g1, g2 = row_geoms(rows[i])
        sub = int(rows[i][1])
        if kind == KIND_PLANE_BOX:
            low = plane_lowest64(g1, g2)
            if low <= PARK - margin:
                continue                                    # not parked: a vertex more than 1 cm above a plane the box touches
            assert PARK < d[i] <= low + tol, ("plane-box parked", i, d[i], low)
        elif kind == KIND_CAPSULE_BOX:
            gap, sep = capsule_parks64(g1, g2)
            if max(gap, sep) <= PARK - margin:
                continue
            if sub == 0:
                true = segment_box_distance64(g1, g2) - g1[3][0]
                assert PARK < d[i] <= true + tol, ("capsule-box parked", i, d[i], true)
            elif max(gap, sep) > PARK + margin:
                assert got[0][i] == 1.0, ("capsule-box parked, sub 1", i, d[i])
        else:
            sface, gap = face_sbest64(g1, g2)
            if max(sface, gap) <= PARK - margin:
                continue
            if sub == 0:
                true = true_separation_box_box(rows[i], int(i) // 4)
                assert PARK < d[i] <= true + tol, ("box-box parked", i, d[i], true)
            elif max(sface, gap) > PARK + margin:
                assert d[i] == 1.0, ("box-box parked, sub >= 1", i, d[i])
        judged.append(int(i))
    return judged


def gate_g1(name, out, what):
    """G1 on one build's output words of g1_cases(name).  Returns a dict of measured figures."""
    kind, _nsub = KINDS[name]
    rows, ref64, _ref32, (tol, ref_err) = g1_cases(name)
    got = decode(out)
    check_frames(got[2], tol, (what, name))
    ok = close_to(kind, got, ref64, tol)
    e_d, e_p, _e_n, _e_f, parked = candidate_errors(kind, got, ref64)
    agree = ok & ~parked
    worst = float(np.maximum(e_d, e_p)[agree].max()) if agree.any() else 0.0
    rng = np.random.default_rng(2024)
    witnessed, unwitnessed = [], []
    for i in np.nonzero(~ok)[0]:
        jr = jittered(rows[i], rng)
        jref = oracle_rows(jr, "float64")
        one = tuple(np.repeat(a[i:i + 1], len(jr), 0) for a in got)
        (witnessed if close_to(kind, one, jref, tol).any() else unwitnessed).append(int(i))
    judged = parked_contract(kind, rows, got, tol)
    fig = dict(kind=name, build=what, cases=len(rows), tol=tol, fp32_oracle_err=ref_err, worst=worst, ratio=worst / tol,
               witnessed=len(witnessed), unwitnessed=len(unwitnessed), parked=int(parked.sum()), parked_judged=len(judged))
    print("\nG1", json.dumps(fig))
    assert not unwitnessed, (what, name, "unwitnessed cases", unwitnessed[:8], [rows[i].tolist() for i in unwitnessed[:2]])
    assert len(witnessed) <= WITNESS_CAP * len(rows), (what, name, "witnessed cases over the cap", len(witnessed))
    return fig


# ------------------------------------------------------------------------------------------------------------------ G2 inputs
def yaw_quat(a):
    return np.array([np.cos(0.5 * a), 0.0, 0.0, np.sin(0.5 * a)])


def flat_on_plane_pairs(n=200, seed=31):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(n):
        h = rng.uniform(0.05, 0.5, 3)
        yaw = 0.0 if k % 2 == 0 else rng.uniform(-np.pi, np.pi)
        cxy = rng.normal(size=2) * 0.3
        pairs.append(((np.zeros(3), yaw_quat(0.0), np.array([0, 0, 0.05])), (np.array([cxy[0], cxy[1], h[2] - rng.uniform(0, 0.003)]), yaw_quat(yaw), h)))
    return pairs


def stacked_pairs(n, seed, equal_yaw):
    """B lying on A's top face with an overlap in x and y, penetration 0-3 mm; relative yaw 0 or 20-70 degrees"""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        hA, hB = rng.uniform(0.1, 0.4, 3), rng.uniform(0.05, 0.3, 3)
        ya = rng.uniform(-np.pi, np.pi)
        yb = ya if equal_yaw else ya + np.deg2rad(rng.uniform(20, 70)) * rng.choice([-1.0, 1.0])
        cA = rng.normal(size=3) * 0.1
        off = q2m(yaw_quat(ya))[:, :2] @ (rng.uniform(-0.7, 0.7, 2) * hA[:2])
        cB = cA + np.array([off[0], off[1], hA[2] + hB[2] - rng.uniform(0, 0.003)])
        pairs.append(((cA, yaw_quat(ya), hA), (cB, yaw_quat(yb), hB)))
    return pairs


def clip_polygon64(poly, a, b):
    """Sutherland-Hodgman step: the part of `poly` (list of 2-vectors) with a . x <= b"""
    res = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        fp, fq = a @ p - b, a @ q - b
        if fp <= 0:
            res.append(p)
        if (fp <= 0) != (fq <= 0):
            res.append(p + (q - p) * (fp / (fp - fq)))
    return res


def face_intersection64(gA, gB):
    """vertices (world xy) of the intersection of A's and B's horizontal face rectangles, fp64"""
    (cA, _, RA, hA), (cB, _, RB, hB) = gA, gB
    poly = [cB[:2] + RB[:2, 0] * sx * hB[0] + RB[:2, 1] * sy * hB[1] for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
    for ax, hh in ((RA[:2, 0], hA[0]), (RA[:2, 1], hA[1])):
        for sg in (1.0, -1.0):
            poly = clip_polygon64(poly, sg * ax, hh + sg * (ax @ cA[:2]))
            if not poly:
                return np.zeros((0, 2))
    return np.array(poly)


def same_sets(kind, got, ref, tol, lo, hi):
    """the live candidates of rows lo..hi as SETS: every one of either side has a partner within tol on the other side"""
    live_g = [i for i in range(lo, hi) if got[0][i] < 0.5]
    live_r = [i for i in range(lo, hi) if ref[0][i] < 0.5]
    if len(live_g) != len(live_r):
        return False
    near = lambda a, i, b, j: (abs(a[0][i] - b[0][j]) <= tol and np.abs(a[1][i] - b[1][j]).max() <= tol
                               and np.abs(a[2][i][0] - b[2][j][0]).max() <= 10 * tol)
    return all(any(near(got, i, ref, j) for j in live_r) for i in live_g) and all(any(near(got, i, ref, j) for i in live_g) for j in live_r)


# ------------------------------------------------------------------------------------------------------------------ G2 gates
def box_box_tol():
    return g1_cases("box_box")[3][0]


def gate_flat_on_plane(run, what):
    rows = geom_rows(KIND_PLANE_BOX, 4, flat_on_plane_pairs())
    tol = g1_cases("plane_box")[3][0]
    got, ref = decode(run(rows)), oracle_rows(rows)
    check_frames(got[2], tol, what)
    ok = close_to(KIND_PLANE_BOX, got, ref, tol) & (got[0] <= PARK)
    assert ok.all(), (what, "flat on a plane: candidates differ from the oracle's, in order", np.nonzero(~ok)[0][:8].tolist())
    assert np.all(got[0] <= tol) and np.all(got[0] >= -0.003 - tol)


def gate_stacked_equal_yaw(run, what):
    rows = geom_rows(KIND_BOX_BOX, 4, stacked_pairs(200, 32, True))
    tol = box_box_tol()
    got, ref = decode(run(rows)), oracle_rows(rows)
    check_frames(got[2], tol, what)
    bad = [p // 4 for p in range(0, len(rows), 4) if not same_sets(KIND_BOX_BOX, got, ref, tol, p, p + 4)]
    assert not bad, (what, "stacked at equal yaw: candidate sets differ from the fp64 oracle's", bad[:8])


def gate_stacked_different_yaw(run, what):
    """Returns (pairs whose candidate SET differs from the fp64 oracle's, pairs): a recorded property, not a failure."""
    pairs = stacked_pairs(400, 33, False)
    rows = geom_rows(KIND_BOX_BOX, 4, pairs)
    tol = box_box_tol()
    got, ref = decode(run(rows)), oracle_rows(rows)
    check_frames(got[2], tol, what)
    d, p, f = got
    ndiff = 0
    for k in range(len(pairs)):
        lo = 4 * k
        gA, gB = row_geoms(rows[lo])
        pen = (gA[0][2] + gA[3][2]) - (gB[0][2] - gB[3][2])               # top of A minus bottom of B
        poly = face_intersection64(gA, gB)
        live = [i for i in range(lo, lo + 4) if d[i] < 0.5]
        assert len(live) == min(4, len(poly)) and len(live) >= 3, (what, k, "live candidates", len(live), "polygon vertices", len(poly))
        for i in live:
            assert abs(d[i] + pen) <= tol, (what, k, "dist is not minus the penetration", d[i], -pen)
            assert np.abs(f[i, 0] - [0, 0, 1]).max() <= 10 * tol, (what, k, "normal is not A's face normal towards B", f[i, 0])
            assert np.linalg.norm(poly - p[i, :2], axis=1).min() <= tol, (what, k, "candidate off the intersection polygon's vertices",
                                                                          float(np.linalg.norm(poly - p[i, :2], axis=1).min()))
            assert abs(p[i, 2] - (gA[0][2] + gA[3][2] - 0.5 * pen)) <= tol, (what, k, "pos is not midway between the faces")
        ds = [d[i] for i in range(lo, lo + 4)]
        assert ds == sorted(ds), (what, k, "candidates do not come deepest first", ds)
        ndiff += 0 if same_sets(KIND_BOX_BOX, got, ref, tol, lo, lo + 4) else 1
    print(f"\nG2 {what}: stacked boxes at different yaw, candidate set differs from the fp64 oracle's in {ndiff} of {len(pairs)} pairs")
    return ndiff, len(pairs)


def gate_fixed_scenes(run, what):
    """test_capsule_lying_on_a_face_touches_with_both_ends and test_trunk_box_resting_on_the_crate_edge_gets_face_contacts on the kernel"""
    c, h = np.array([0.0, 0, 0.3]), np.array([0.31, 0.46, 0.3])
    qc = m2q(np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]))               # capsule axis along world x
    ctr, hl, r = np.array([0.05, 0.1, 0.6 + 0.013 - 0.002]), 0.06, 0.013
    rows = geom_rows(KIND_CAPSULE_BOX, 2, [((ctr, qc, [r, hl, 0]), (c, yaw_quat(0), h))])
    d, p, f = decode(run(rows))
    assert np.isclose(d[0], -0.002) and np.isclose(d[1], -0.002), (what, d)
    assert np.allclose(f[0, 0], [0, 0, -1]) and np.allclose(f[1, 0], [0, 0, -1]), (what, f[:, 0])
    assert np.isclose(abs(p[0, 0] - p[1, 0]), 2 * hl), (what, p)
    cB, hB = np.array([1.3, 0, 0.3]), np.array([0.31, 0.46, 0.3])
    pitch = -0.5
    RA = np.array([[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]])
    hA = np.array([0.1881, 0.04675, 0.057])
    cA = np.array([0.99, 0.0, 0.6]) + RA @ np.array([0.0, 0.0, hA[2] - 0.003])
    rows = geom_rows(KIND_BOX_BOX, 4, [((cA, m2q(RA), hA), (cB, yaw_quat(0), hB))])
    d, p, f = decode(run(rows))
    live = [i for i in range(4) if d[i] < 0.001]
    assert len(live) >= 2, (what, d)
    ys = sorted(p[i, 1] for i in live)
    assert ys[-1] - ys[0] > 1.5 * hA[1], (what, ys)
    for i in live:
        assert -0.004 < d[i] < 0.001 and abs(p[i, 0] - 0.99) < 0.01 and abs(p[i, 2] - 0.6) < 0.01, (what, d[i], p[i])


def gate_sphere_placement(run, what):
    """centre inside the box (also exactly at the centre of a cube: any nearest face is valid), exactly on a face, an edge, a vertex"""
    tol = g1_cases("sphere_box")[3][0]
    rng = np.random.default_rng(34)
    c, h, r = np.array([0.25, -0.5, 0.125]), np.array([0.5, 0.25, 0.125]), 0.0625        # exact in fp32, identity orientation
    pairs, where = [], []
    for l in ([0.5, 0.0625, 0.03125], [0.5, -0.25, 0.0], [0.25, 0.25, 0.125], [-0.5, 0.25, 0.125], [0.5, 0.25, -0.125], [0.0, 0.0, -0.125]):
        pairs.append(((c + np.array(l), yaw_quat(0), [r, 0, 0]), (c, yaw_quat(0), h)))
        where.append("surface")
    pairs.append(((np.array([1.0, 2.0, -0.5]), yaw_quat(0), [r, 0, 0]), (np.array([1.0, 2.0, -0.5]), _rand_quat(rng), np.array([0.25, 0.25, 0.25]))))
    where.append("cube centre")
    for _ in range(200):
        cc, q, hh = rng.normal(size=3) * 0.2, _rand_quat(rng), rng.uniform(0.05, 0.5, 3)
        pairs.append(((cc + _q2m(q) @ (rng.uniform(-0.98, 0.98, 3) * hh), yaw_quat(0), [rng.uniform(0.01, 0.1), 0, 0]), (cc, q, hh)))
        where.append("inside")
    rows = geom_rows(KIND_SPHERE_BOX, 1, pairs)
    d, p, f = decode(run(rows))
    check_frames(f, tol, what)
    for i, row in enumerate(rows):
        (s, _, _, size), (cb, _, R, hb) = row_geoms(row)
        l = R.T @ (s - cb)
        depth = np.min(hb - np.abs(l))
        assert depth >= -1e-7, (what, where[i], "generator")
        assert abs(d[i] + max(depth, 0.0) + size[0]) <= tol, (what, where[i], i, "dist", d[i], -depth - size[0])
        nl = R.T @ f[i, 0]
        k = int(np.argmax(np.abs(nl)))
        assert np.abs(np.abs(nl) - np.eye(3)[k]).max() <= 10 * tol, (what, where[i], i, "the normal is no face normal", nl)
        assert hb[k] - abs(l[k]) <= depth + tol, (what, where[i], i, "not through a nearest face")
        if abs(l[k]) > tol:
            assert nl[k] * l[k] < 0, (what, where[i], i, "the normal does not point into the box")
        assert np.abs(p[i] - (s + f[i, 0] * (size[0] + 0.5 * d[i]))).max() <= tol, (what, where[i], i, "pos")


def gate_capsule_through(run, what):
    """the `through` branch of test_capsule_box_first_candidate_is_the_closest_point_of_the_segment, on the kernel's output"""
    tol = g1_cases("capsule_box")[3][0]
    rng = np.random.default_rng(2)
    pairs = []
    for _ in range(240):
        c, q, h = rng.normal(size=3), _rand_quat(rng), rng.uniform(0.05, 0.6, 3)
        qc, hl, r = _rand_quat(rng), rng.uniform(0.03, 0.4), rng.uniform(0.01, 0.05)
        pairs.append(((c + _q2m(q) @ (rng.normal(size=3) * h * 1.3), qc, [r, hl, 0]), (c, q, h)))
    rows = geom_rows(KIND_CAPSULE_BOX, 2, pairs)
    d, p, f = decode(run(rows))
    check_frames(f, tol, what)
    n_through = 0
    ts = np.linspace(0, 1, 2001)
    for k in range(len(pairs)):
        (ctr, _, Rc, size), (c, _, R, h) = row_geoms(rows[2 * k])
        r, hl = size[0], size[1]
        e0, e1 = ctr - Rc[:, 2] * hl, ctr + Rc[:, 2] * hl
        pts = e0 + ts[:, None] * (e1 - e0)
        margin = np.abs((pts - c) @ R) - h
        inside = np.all(margin <= 0, axis=1)
        if not inside.any() or inside.all() or np.abs(margin[[0, -1]]).min() < 1e-4 or np.all(margin <= 0, axis=1).sum() < 3:
            continue                                     # not through, wholly inside, or within rounding of either
        n_through += 1
        d0, p0, f0 = d[2 * k], p[2 * k], f[2 * k]
        assert abs(d0 + r) <= tol, (what, k, "dist is not minus the radius", d0, r)
        surf = p0 - f0[0] * (r * 0.5)
        loc = R.T @ (surf - c)
        assert np.max(np.abs(loc) - h) < 4 * tol and np.min(np.abs(np.abs(loc) - h)) < 4 * tol, (what, k, "not on the surface", loc, h)
        kf = int(np.argmin(np.abs(np.abs(loc) - h)))
        assert np.allclose(R.T @ f0[0], -np.sign(loc[kf]) * np.eye(3)[kf], atol=10 * tol), (what, k, "not into the box through that face")
        first = int(np.argmax(inside)) if not inside[0] else int(len(ts) - 1 - np.argmax(inside[::-1]))
        assert np.linalg.norm(pts[first] - surf) < 2.0 * np.linalg.norm(e1 - e0) / 2000 + 4 * tol, (what, k, "not where the axis crosses")
    assert n_through > 20, n_through


def axis_aligned_pairs(n=200, seed=35):
    """both boxes at multiples of 90 degrees about z (every edge axis has len < 1e-4 and is skipped), faces 3 mm apart to 3 mm deep"""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        hA, hB = rng.uniform(0.1, 0.4, 3), rng.uniform(0.05, 0.3, 3)
        qa, qb = yaw_quat(0.5 * np.pi * rng.integers(4)), yaw_quat(0.5 * np.pi * rng.integers(4))
        eA, eB = np.abs(q2m(qa)) @ hA, np.abs(q2m(qb)) @ hB            # world extents
        ax = int(rng.integers(3))
        cA = rng.normal(size=3) * 0.1
        off = rng.uniform(-0.7, 0.7, 3) * eA
        off[ax] = rng.choice([-1.0, 1.0]) * (eA[ax] + eB[ax] + rng.uniform(-0.003, 0.003))
        pairs.append(((cA, qa, hA), (cA + off, qb, hB)))
    # FLUSH faces (numbers exact in fp32, identity orientation): the incident face's vertices lie exactly ON the clip planes (fp == 0 counts
    # as inside) -- the same footprint on top of each other, and a smaller box whose +x and -y sides are flush with the larger one's
    for k in range(8):
        hA = np.array([0.25, 0.125 * (1 + k % 3), 0.25])
        cA = np.array([0.5, -0.25, 0.125 * k])
        pen = 2.0 ** -9 if k % 2 else -2.0 ** -9
        pairs.append(((cA, yaw_quat(0), hA), (cA + [0, 0, 0.5 - pen], yaw_quat(0), hA)))
        hB = np.array([0.125, 0.0625, 0.25])
        pairs.append(((cA, yaw_quat(0), hA), (cA + [hA[0] - hB[0], -(hA[1] - hB[1]), 0.5 - pen], yaw_quat(0), hB)))
    return pairs


def gate_axis_aligned(run, what):
    rows = geom_rows(KIND_BOX_BOX, 4, axis_aligned_pairs())
    tol = box_box_tol()
    got, ref = decode(run(rows)), oracle_rows(rows)
    check_frames(got[2], tol, what)
    bad = [p // 4 for p in range(0, len(rows), 4) if not same_sets(KIND_BOX_BOX, got, ref, tol, p, p + 4)]
    assert not bad, (what, "axis-aligned boxes: candidate sets differ from the fp64 oracle's", bad[:8])
    assert (got[0] < 0.5).sum() >= 3 * len(rows) // 4 - 8
    assert np.all(got[0][-64:] < 0.5), (what, "flush faces: a vertex ON a clip plane was dropped", got[0][-64:].reshape(-1, 4))


def park_threshold_pairs(n=200, seed=36):
    """box-box pairs whose best face separation lies within 1e-4 of DIAL_BOX_PARK_DIST: B over A's top face, slightly tilted"""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n):
        hA, hB = rng.uniform(0.1, 0.4, 3), rng.uniform(0.05, 0.3, 3)
        qa = yaw_quat(rng.uniform(-np.pi, np.pi))
        qb = _rand_quat(rng) * np.array([1, 0.02, 0.02, 1]) + np.array([2.0, 0, 0, 0])
        qb /= np.linalg.norm(qb)
        RB = q2m(qb)
        cA = rng.normal(size=3) * 0.1
        off = q2m(qa)[:, :2] @ (rng.uniform(-0.5, 0.5, 2) * hA[:2])
        low = np.abs(RB[2]) @ hB                                          # B's extent below its centre
        target = PARK + rng.uniform(-0.9e-4, 0.9e-4)
        cB = cA + np.array([off[0], off[1], hA[2] + low + target])
        for _it in range(3):                                               # (a face of the tilted B may separate better than A's top face)
            cB[2] -= face_sbest64((cA, qa, q2m(qa), hA), (cB, qb, RB, hB))[0] - target
        pairs.append(((cA, qa, hA), (cB, qb, hB)))
    return pairs


def gate_park_threshold(run, what):
    """either side of the park decision is valid: what comes out satisfies the parked contract or G1's comparison"""
    rows = geom_rows(KIND_BOX_BOX, 4, park_threshold_pairs())
    tol = box_box_tol()
    sb = np.array([face_sbest64(*row_geoms(r))[0] for r in rows[::4]])
    assert np.all(np.abs(sb - PARK) <= 1.0001e-4), ("generator", float(np.abs(sb - PARK).max()))
    got, ref = decode(run(rows)), oracle_rows(rows)
    check_frames(got[2], tol, what)
    ok = close_to(KIND_BOX_BOX, got, ref, tol)
    judged = set(parked_contract(KIND_BOX_BOX, rows, got, tol))
    for i in np.nonzero(~ok)[0]:
        assert i in judged and got[0][i] > PARK, (what, "neither parked nor the oracle's candidate", int(i), got[0][i], ref[0][i])
    n_parked = int((got[0][::4] > PARK).sum())
    print(f"\nG2 {what}: {n_parked} of {len(rows) // 4} threshold pairs parked")
    assert 0 < n_parked < len(rows) // 4


G2_GATES = {"flat_on_plane": gate_flat_on_plane, "stacked_equal_yaw": gate_stacked_equal_yaw, "stacked_different_yaw": gate_stacked_different_yaw,
            "fixed_scenes": gate_fixed_scenes, "sphere_placement": gate_sphere_placement, "capsule_through": gate_capsule_through,
            "axis_aligned": gate_axis_aligned, "park_threshold": gate_park_threshold}


# ------------------------------------------------------------------------------------------------------------------ G5: segments
SEG_MODES = ("generic", "parallel", "collinear", "one of zero length", "crossing", "both of zero length")


def seg_rows(seed=41):
    """(op, 12 floats): generic, parallel, collinear, zero-length and crossing segments; make_frame at lengths 1e-6 .. 1e3"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(400):
        a, b, pt = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        rows.append([L.S_POINT, *a, *b, *pt, 0, 0, 0])
    for _ in range(20):
        a, pt = rng.normal(size=3), rng.normal(size=3)
        rows.append([L.S_POINT, *a, *a, *pt, 0, 0, 0])                                    # zero length
        rows.append([L.S_POINT, *a, *(a + rng.normal(size=3)), *a, 0, 0, 0])              # the point is an end
    for k in range(600):
        a0, da = rng.normal(size=3) * 0.3, rng.normal(size=3) * rng.uniform(0.05, 0.5)
        mode = k % 6
        if mode == 0:
            b0, db = rng.normal(size=3) * 0.3, rng.normal(size=3) * rng.uniform(0.05, 0.5)
        elif mode == 1:                                                                   # parallel
            b0, db = a0 + rng.normal(size=3) * 0.2, da * rng.uniform(-2, 2)
        elif mode == 2:                                                                   # collinear
            b0, db = a0 + da * rng.uniform(-2, 2), da * rng.uniform(0.2, 2)
        elif mode == 3:                                                                   # one of zero length
            b0, db = rng.normal(size=3) * 0.3, np.zeros(3)
        elif mode == 4:                                                                   # crossing (they meet in a point)
            db = rng.normal(size=3) * 0.3
            b0 = a0 + da * rng.uniform(0.1, 0.9) - db * rng.uniform(0.1, 0.9)
        else:                                                                             # both of zero length
            da, b0, db = np.zeros(3), rng.normal(size=3) * 0.3, np.zeros(3)
        rows.append([L.S_SEGSEG, *a0, *(a0 + da), *b0, *(b0 + db)])
    for e in np.linspace(-6, 3, 37):
        for _ in range(8):
            v = rng.normal(size=3)
            rows.append([L.S_FRAME, *(v / np.linalg.norm(v) * 10.0 ** e), *([0] * 9)])
    for v in ([0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1], [0.6, 0.8, 0], [0.8, 0.6, 0]):
        rows.append([L.S_FRAME, *v, *([0] * 9)])
    return np.array(rows, np.float64).astype(F32)


def _csp(a, b, pt, dt):
    ab, pa = b - a, pt - a
    t = np.clip((pa * ab).sum(-1, dtype=dt) / ((ab * ab).sum(-1, dtype=dt) + dt(1e-6)), dt(0), dt(1))
    return a + t[..., None] * ab


def _cs2s(a0, a1, b0, b1, dt):
    """mujoco.mjx._src.math.closest_segment_to_segment_points, restated in NumPy at precision dt"""
    da, db = a1 - a0, b1 - b0
    la, lb = np.sqrt((da * da).sum(-1, dtype=dt)), np.sqrt((db * db).sum(-1, dtype=dt))
    with np.errstate(invalid="ignore", divide="ignore"):
        da = np.where(la[:, None] > 0, da / la[:, None], dt(0))
        db = np.where(lb[:, None] > 0, db / lb[:, None], dt(0))
    ha, hb = la * dt(0.5), lb * dt(0.5)
    am, bm = a0 + da * ha[:, None], b0 + db * hb[:, None]
    tr = am - bm
    dadb, dat, dbt = (da * db).sum(-1, dtype=dt), (da * tr).sum(-1, dtype=dt), (db * tr).sum(-1, dtype=dt)
    ota = (-dat + dadb * dbt) / ((dt(1) - dadb * dadb) + dt(1e-6))
    otb = dbt + ota * dadb
    ta, tb = np.clip(ota, -ha, ha), np.clip(otb, -hb, hb)
    ba, bb = am + da * ta[:, None], bm + db * tb[:, None]
    na, nb = _csp(a0, a1, bb, dt), _csp(b0, b1, ba, dt)
    d1, d2 = ((na - bb) ** 2).sum(-1, dtype=dt), ((nb - ba) ** 2).sum(-1, dtype=dt)
    return np.where((d1 < d2)[:, None], na, ba), np.where((d1 < d2)[:, None], bb, nb), d1, d2


def gate_segments(out, what):
    """G5.  closest_segment_point / closest_segment_to_segment against the fp64 restatement (tolerance: 8 x the error of the SAME restatement
    evaluated in fp32, floor 1e-6); where the final `d1 < d2` choice is within rounding of a tie (parallel, collinear, crossing: both
    candidates are closest pairs) either pair is accepted.  make_frame: orthonormal, right-handed, row 0 along the input."""
    rows = seg_rows()
    w = np.ascontiguousarray(out).view(F32).astype(np.float64)
    op = rows[:, 0].astype(int)
    x64, x32 = rows[:, 1:].astype(np.float64), rows[:, 1:]
    fig = {}
    m = op == L.S_POINT
    r64 = _csp(x64[m, 0:3], x64[m, 3:6], x64[m, 6:9], np.float64)
    r32 = _csp(x32[m, 0:3], x32[m, 3:6], x32[m, 6:9], F32).astype(np.float64)
    tol = max(TOL_FLOOR, 8 * float(np.abs(r32 - r64).max()))
    err = np.abs(w[m, :3] - r64).max()
    fig["point"] = (float(err), tol)
    assert err <= tol, (what, "closest_segment_point", float(err), tol)
    m = op == L.S_SEGSEG
    seg = lambda x, dt: _cs2s(x[m, 0:3], x[m, 3:6], x[m, 6:9], x[m, 9:12], dt)
    a64, b64, d1, d2 = seg(x64, np.float64)
    a32, b32, e1, e2 = seg(x32, F32)
    ga, gb = w[m, 0:3], w[m, 3:6]
    dist = lambda a, b: np.linalg.norm(a - b, axis=1)
    e32_p = np.maximum(np.abs(a32 - a64).max(1), np.abs(b32 - b64).max(1))
    e32_d = np.abs(dist(a32.astype(np.float64), b32.astype(np.float64)) - dist(a64, b64))
    e_p = np.maximum(np.abs(ga - a64).max(1), np.abs(gb - b64).max(1))
    e_d = np.abs(dist(ga, gb) - dist(a64, b64))
    mode = np.arange(m.sum()) % 6
    for k, mname in enumerate(SEG_MODES):
        s = mode == k
        # the POINTS are ill-conditioned where the segments are parallel or collinear (MJX divides by 1 - (da . db)^2 + 1e-6): there the
        # restatement's own fp32 error is large and the gate on the points says little; the DISTANCE between them stays well-conditioned
        tol_p, tol_d = max(TOL_FLOOR, 8 * float(e32_p[s].max())), max(TOL_FLOOR, 8 * float(e32_d[s].max()))
        fig["segseg " + mname] = (float(e_p[s].max()), tol_p, float(e_d[s].max()), tol_d)
        assert e_p[s].max() <= tol_p and e_d[s].max() <= tol_d, (what, "closest_segment_to_segment", mname, fig["segseg " + mname])
    m = op == L.S_FRAME
    fr, v = w[m].reshape(-1, 3, 3), x64[m, 0:3]
    g = np.abs(fr @ fr.transpose(0, 2, 1) - np.eye(3)).max()
    along = np.abs(fr[:, 0] - v / np.linalg.norm(v, axis=1, keepdims=True)).max()
    fig["frame"] = (float(g), float(along))
    assert g <= 1e-6 and along <= 1e-6 and np.all(np.linalg.det(fr) > 0.99), (what, "make_frame", float(g), float(along))
    print("\nG5", what, json.dumps(fig))
    return fig


# ------------------------------------------------------------------------------------------------------------------ G6: keys
def np_fkey(x):
    """test_ls_bracket._fkey on an array"""
    b = (np.asarray(x, F32) + F32(0)).view(np.int32)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def fkey_inputs():
    tiny, big_den, fmin = F32(1e-45), np.array(0x007FFFFF, np.int32).view(F32), F32(1.17549435e-38)
    one_up, one_dn = np.nextafter(F32(1), F32(2)), np.nextafter(F32(1), F32(0))
    edge = [0.0, tiny, big_den, fmin, 1.0, one_up, one_dn, 3e38, np.inf]
    rng = np.random.default_rng(51)
    rnd = rng.standard_normal(4096).astype(F32) * F32(10.0) ** rng.integers(-44, 38, 4096).astype(F32)
    rnd[:256] = rng.integers(1, 0x00800000, 256).astype(np.int32).view(F32) * rng.choice([-1, 1], 256).astype(F32)   # denormals
    with np.errstate(over="ignore"):
        x = np.concatenate([np.array(edge, F32), -np.array(edge, F32), rnd]).astype(F32)
    return x[np.isfinite(x) | np.isinf(x)]


def gate_fkey(out, what):
    x = fkey_inputs()
    want = np_fkey(x)
    assert all(int(want[i]) == _fkey(x[i]) for i in range(0, len(x), 97)), "np_fkey is not test_ls_bracket._fkey"
    got = np.ascontiguousarray(out[:, 0]).view(np.int32)
    bad = np.nonzero((got != want) | (out[:, 1].view(np.int32) != want))[0]
    assert bad.size == 0, (what, "fkey / fkeyf", x[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert got[0] == 0 and got[9] == 0 and x[9] == 0 and np.signbit(x[9]), (what, "the two zeros do not share key 0")
    order = np.argsort(x.astype(np.float64), kind="stable")
    xs, ks = x[order].astype(np.float64), got[order].astype(np.int64)
    assert np.all((np.diff(xs) > 0) == (np.diff(ks) > 0)) and np.all(np.diff(ks) >= 0), (what, "order not preserved")
    den = (np.abs(x) > 0) & (np.abs(x) < F32(1.17549435e-38))
    assert den.sum() >= 260 and np.all(got[den] != 0), (what, "denormals flushed")


def pack_inputs():
    rng = np.random.default_rng(52)
    n = 8192
    alpha = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(F32)
    cost = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32)
    d0 = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(F32)
    d1 = (np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-4, 6, n) + 1e-8).astype(F32)
    alpha[:64] = 0
    d0[64:128] = 0
    return np.stack([alpha, cost, d0, d1], 1)


def gate_pack(out, emu_out, ieee_like, what):
    """alpha, cost, d0 words bit-exact; nalpha bit-exact with IEEE arithmetic (emulator, IEEE build), within 2.5 ulp of |d0 / d1| + 0.5 ulp of
    the result on the product build (1-ulp v_rcp_f32, one multiply, one subtraction), against fp64.  Returns the worst error / that bound."""
    x = pack_inputs()
    want = np.stack([x[:, 0].view(np.uint32), (x[:, 0] - x[:, 2] / x[:, 3]).astype(F32).view(np.uint32),
                     np_fkey(x[:, 1]).view(np.uint32), np_fkey(x[:, 2]).view(np.uint32)], 1)
    for k, name in ((0, "alpha"), (2, "cost"), (3, "d0")):
        assert np.array_equal(out[:, k], want[:, k]), (what, "ls_pack", name)
    if ieee_like:
        assert np.array_equal(out[:, 1], want[:, 1]), (what, "ls_pack nalpha differs from the correctly rounded alpha - d0 / d1")
        assert emu_out is None or np.array_equal(out[:, :4], emu_out[:, :4])
    x64 = x.astype(np.float64)
    q = x64[:, 2] / x64[:, 3]
    exact = x64[:, 0] - q
    got = out[:, 1].view(F32).astype(np.float64)
    ulp_q, ulp_r = np.spacing(np.abs(q).astype(F32)).astype(np.float64), np.spacing(np.abs(got).astype(F32)).astype(np.float64)
    bound = 2.5 * ulp_q + 0.5 * ulp_r
    ratio = float((np.abs(got - exact) / bound).max())
    in_q = float(((np.abs(got - exact) - 0.5 * ulp_r) / ulp_q).max())      # what the quotient contributes, in its own ulps (bound: 2.5)
    print(f"\nG6 {what}: ls_pack nalpha, worst error {ratio:.3g} of its bound; beyond the result's half ulp: {in_q:.3g} ulp of d0 / d1")
    assert ratio <= 1.0, (what, "ls_pack nalpha", ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def update_keys():
    """the case set of test_ls_bracket.test_bracket_update_takes_the_reference_decisions"""
    edge = [_fkey(v) for v in (0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 1.0000001, -1.0000001, 3e38, -3e38, np.inf, -np.inf)]
    cases = np.array(list(itertools.product(edge, repeat=5)), np.int64)
    rng = np.random.default_rng(5)
    small = rng.integers(-4, 5, size=(200000, 5))
    wide = rng.standard_normal((200000, 5)).astype(F32) * F32(10.0) ** rng.integers(-30, 30, size=(200000, 1))
    arr = np.concatenate([cases, small, np_fkey(wide).astype(np.int64)]).astype(np.int32)
    arr.setflags(write=False)
    return arr


@functools.lru_cache(maxsize=None)
def update_reference(rule_swap):
    r = _reference(rule_swap, update_keys())
    r.setflags(write=False)
    return r


def points_of(sel, own, width=4):
    """the words (0x100 id + word) an end carries after the update: sel -1 keeps its own point (id `own`), 0 / 1 / 2 = lo_next / hi_next / mid"""
    ident = np.where(sel < 0, own, sel + 3)
    return (0x100 * ident)[:, None] + np.arange(width)[None]


def gate_update(side, what):
    """ls_update (both rules) and ls_update_lazy<true> / <false> per lane, on the full case set, against _reference"""
    arr = update_keys()
    for rule in (0, 1):
        ref = update_reference(bool(rule))
        out = side.key(L.K_UPDATE, arr, rule).view(np.int32)
        want = np.concatenate([points_of(ref[:, 2], 1, 3), ref[:, 0:1], points_of(ref[:, 3], 2, 3), ref[:, 1:2], ref[:, 4:5]], 1)
        bad = np.nonzero((out[:, :9] != want).any(1))[0]
        assert bad.size == 0, (what, "ls_update rule", rule, arr[bad[:3]], out[bad[:3]], want[bad[:3]])
    for par in (0, 1, 2):
        ref = update_reference(par == 1)
        out = side.key(L.K_LAZY, arr, par).view(np.int32)
        bad = np.nonzero((out[:, :5] != ref).any(1))[0]
        assert bad.size == 0, (what, "ls_update_lazy par", par, arr[bad[:3]], out[bad[:3]], ref[bad[:3]])
        lo_new, hi_new = ref[:, 2] >= 0, ref[:, 3] >= 0
        for col, new, sel, init in ((5, lo_new, ref[:, 2], 11), (6, lo_new, ref[:, 2], 12), (7, lo_new, ref[:, 2], 13),
                                    (8, hi_new, ref[:, 3], 14), (9, hi_new, ref[:, 3], 15)):
            assert np.array_equal(out[:, col], np.where(new, 1000 + sel, init)), (what, "ls_update_lazy fetched word", par, col)


def gate_inputs():
    """the case set of test_ls_bracket.test_range_compare_form_of_the_done_test"""
    edge = [_fkey(v) for v in (0.0, 1e-45, -1e-45, 1e-12, -1e-12, 1.0, -1.0, np.inf, -np.inf)] + [1, -1, 2, -2, 2 ** 31 - 1, -2 ** 31 + 1]
    gt = [0.0, 1e-45, 1e-12, 3e-7, 1.0, 3e38]
    cases = [(a, b, _fkey(g), _fkey(-g)) for a in edge for b in edge for g in gt]
    rng = np.random.default_rng(9)
    for _ in range(20000):
        g = float(F32(10.0 ** rng.uniform(-40, 3)))
        x = (rng.standard_normal(2).astype(F32) * F32(10.0 ** rng.uniform(-42, 4))).tolist()
        cases.append((_fkey(x[0]), _fkey(x[1]), _fkey(g), _fkey(-g)))
    return np.array(cases, np.int64).astype(np.int32)


def gate_done_test(out, what):
    arr = gate_inputs().astype(np.int64)
    lo, hi, kg, kng = arr.T
    c_lo, c_hi = (lo < 0) & (lo > kng), (hi > 0) & (hi < kg)
    o = out.view(np.int32)
    assert np.array_equal(o[:, 1], c_lo.astype(np.int32)), (what, "ls_converged_lo", arr[o[:, 1] != c_lo][:5])
    assert np.array_equal(o[:, 2], c_hi.astype(np.int32)), (what, "ls_converged_hi", arr[o[:, 2] != c_hi][:5])
    assert np.array_equal(o[:, 0], 3 * (c_lo | c_hi).astype(np.int32)), (what, "ls_converged against the range-compare form")
    assert (o[:, 0] == 3).sum() > 100 and (o[:, 0] == 0).sum() > 100


@functools.lru_cache(maxsize=None)
def uniform_keys():
    edge = [_fkey(v) for v in (0.0, 1e-45, -1e-45, 1.0, -1.0)]
    rng = np.random.default_rng(53)
    wide = rng.standard_normal((4096, 5)).astype(F32) * F32(10.0) ** rng.integers(-30, 30, size=(4096, 1))
    arr = np.concatenate([np.array(list(itertools.product(edge, repeat=5)), np.int64), np_fkey(wide).astype(np.int64)]).astype(np.int32)
    arr.setflags(write=False)
    return arr


def gate_uniform(side, what):
    """the wave-uniform variant: the per-lane variant's decisions (= _reference), the words of the chosen group's FIRST lane"""
    arr = uniform_keys()
    for rule in (0, 1):
        ref = _reference(bool(rule), arr)
        lane = side.key(L.K_LAZY, arr, rule).view(np.int32)
        assert np.array_equal(lane[:, :5], ref), (what, "per-lane variant", rule)
        for minmax in (True, False):
            out = side.key_uniform(arr, rule, minmax).view(np.int32)
            for base, sel, own, d0 in ((0, ref[:, 2], 1, ref[:, 0]), (4, ref[:, 3], 2, ref[:, 1])):
                group = np.where(sel == 0, 0, np.where(sel == 1, 16, 32))                 # first lane of lo_next / hi_next / mid
                for k in range(3):
                    want = np.where(sel < 0, 0x100 * own + k, 0x3F800000 + 0x1000 * k + group)
                    assert np.array_equal(out[:, base + k], want), (what, "wave-uniform: fetched word", rule, minmax, base, k)
                assert np.array_equal(out[:, base + 3], d0), (what, "wave-uniform: slope key", rule, minmax, base)
            assert np.array_equal(out[:, 8], ref[:, 4]), (what, "wave-uniform: any", rule, minmax)


def open_result_inputs():
    rng = np.random.default_rng(54)
    v = (rng.standard_normal((4096, 8)) * 10.0 ** rng.integers(-6, 6, (4096, 8))).astype(F32)
    v[:512, 7] = v[:512, 3]                                                              # ties
    v[512:1024, 6] = v[512:1024, 2]
    v[1024:1100, 3] = 0
    v[1100:1200, 7] = -0.0
    return v


def gate_open_result(side, what):
    """ls_open and ls_result against plain float comparisons on the decoded values"""
    v = open_result_inputs()
    p = v.view(np.int32).copy()
    for col in (2, 3, 6, 7):
        p[:, col] = np_fkey(v[:, col])
    out = side.key(L.K_OPEN, p).view(np.int32)
    lesser = v[:, 7] < v[:, 3]
    want = np.where(lesser[:, None], np.concatenate([p[:, 4:8], p[:, 0:4]], 1), np.concatenate([p[:, 0:4], p[:, 4:8]], 1))
    assert np.array_equal(out[:, :8], want), (what, "ls_open")
    r = np.stack([p[:, 2], p[:, 0], p[:, 6], p[:, 4], np_fkey(v[:, 5])], 1)              # p0.cost, lo.alpha, lo.cost, hi.alpha, hi.cost
    out = side.key(L.K_RESULT, r).view(np.int32)
    c0, cl, ch = v[:, 2], v[:, 6], v[:, 5]
    assert np.array_equal(out[:, 0], np.where(cl < ch, p[:, 0], p[:, 4])), (what, "ls_result alpha")
    assert np.array_equal(out[:, 1], ((cl < c0) | (ch < c0)).astype(np.int32)), (what, "ls_result improved")


# ------------------------------------------------------------------------------------------------------------------ G7: trig
SINCOS_TOL = 1.2e-6      # dmath.h's documented 1e-6 + 2e-7 for rounding x / 2 pi at |r| <= 0.5


def hinge_half_ranges():
    """half the range limits of every hinge of the shipped models (the arguments fast_sincos sees are joint HALF angles)"""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dial_mpc_amd", "models")
    vals = set()
    for dirpath, _d, files in os.walk(root):
        for f in files:
            if f.endswith(".json"):
                with open(os.path.join(dirpath, f)) as fh:
                    m = json.load(fh)
                for typ, rng in zip(m["jnt_type"], m["jnt_range"]):
                    if typ == 3:                                   # mjJNT_HINGE
                        vals.update(0.5 * float(t) for t in rng)
    assert len(vals) > 10 and max(abs(v) for v in vals) <= np.pi
    return np.array(sorted(vals), np.float64)


def trig_rows():
    rng = np.random.default_rng(61)
    ang = np.concatenate([np.linspace(-np.pi, np.pi, 65536), np.linspace(-1e-3, 1e-3, 4096), hinge_half_ranges()]).astype(F32)
    ang = np.clip(ang, -F32(np.pi), F32(np.pi))
    ax = rng.normal(size=(len(ang), 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    return np.concatenate([ax, ang[:, None].astype(np.float64)], 1).astype(F32)


def gate_trig(out, what):
    """G7.  Returns the worst absolute errors of fast_sincos and of |q| - 1."""
    rows = trig_rows()
    w = np.ascontiguousarray(out).view(F32).astype(np.float64)
    x = rows[:, 3].astype(np.float64)
    e_s, e_c = np.abs(w[:, 0] - np.sin(x)), np.abs(w[:, 1] - np.cos(x))
    q = w[:, 2:6]
    ax = rows[:, :3].astype(np.float64)
    want = np.concatenate([np.cos(0.5 * x)[:, None], ax * np.sin(0.5 * x)[:, None]], 1)
    e_q, e_unit = np.abs(q - want).max(), np.abs(np.linalg.norm(q, axis=1) - 1).max()
    print(f"\nG7 {what}: fast_sincos worst |error| sin {e_s.max():.3g} cos {e_c.max():.3g} on {len(x)} points; "
          f"axis_angle_to_quat | |q| - 1 | {e_unit:.3g}, worst component error {e_q:.3g}")
    assert max(e_s.max(), e_c.max()) <= SINCOS_TOL, (what, "fast_sincos", float(e_s.max()), float(e_c.max()), float(x[np.argmax(np.maximum(e_s, e_c))]))
    assert e_unit <= 3e-6 and e_q <= 3e-6, (what, "axis_angle_to_quat", float(e_unit), float(e_q))
    return float(max(e_s.max(), e_c.max())), float(e_unit)
