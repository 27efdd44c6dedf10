"""The lane-local code of the kernels on the device, one case per lane: the box narrow phases of csrc/box_collide.h, the MJX segment
helpers and make_frame of rollout_body.h, the integer-key bracket bookkeeping of ls_bracket.h, dm::fast_sincos.  The cases of
tests/lane_cases/lane_cases.h are compiled for gfx950 twice -- product flags (contraction, -freciprocal-math, -fapprox-func,
-fno-honor-nans) and IEEE flags -- and for the host emulator; tests/test_lane_emu.py runs the gates of tests/lane_ref.py on the
emulator build, this file runs the SAME functions on the two device builds:

  G1  generic position against the fp64 oracle; tolerance per kind = 8 x the fp32 oracle's own worst error, floor 1e-6, frame[0] 10 x;
      a case outside it must be witnessed by the fp64 oracle on inputs jittered by <= 4 ulp (capped at 1 %), else the test fails;
      parked candidates keep the contract of box_collide.h's header;
  G2  degenerate position by geometry (box flat on a plane, stacked boxes, the two fixed scenes, sphere placements, capsule axis
      through the box, axis-aligned pairs, pairs at the park threshold);
  G3  layout independence, bit for bit: kinds per wavefront / interleaved lane by lane, partial last wavefront, polygon slices
      pre-filled with 0 / NaN;
  G4  the IEEE build against the emulator build, bit for bit (geom, seg, key);
  G5  segment helpers against an fp64 restatement of the MJX formulas;  G6  bracket keys;  G7  fast_sincos against fp64.

MEASURED on an MI355X, 2026-10-19 (the same table stands in DESIGN.md section 2):
  G1 worst error of agreeing live candidates / tolerance (ratio), product build | IEEE build (= the emulator build, bit for bit):
      plane-box   (4000 cases)  1.15e-7 / 1.00e-6 (0.12) | 1.46e-7 (0.15)        sphere-box (1000)  2.07e-7 / 1.41e-6 (0.15) | 2.58e-7 (0.18)
      capsule-box (2000)        1.79e-7 / 2.14e-6 (0.08) | 1.34e-7 (0.06)        box-box    (5200)  8.17e-7 / 1.43e-6 (0.57) | 4.51e-7 (0.31)
      no witnessed and no unwitnessed case on either build; the tolerances are 8 x the fp32 oracle's 1.11e-7, 1.76e-7, 2.68e-7, 1.79e-7.
  G2 boxes stacked at different yaw: the candidate SET differs from the fp64 oracle's in 144 (product) / 143 (IEEE, emulator) of 400 pairs.
  G4 one finding, see zero_sign_only: 5410 frame words differ from the emulator's in the sign of a zero, no other bit of any word.
  G6 ls_pack's nalpha on the product build: the quotient contributes 1.18 ulp of d0 / d1 at worst (bound 2.5); IEEE build 0.496 (bit-exact).
  G7 fast_sincos worst |error| 2.66e-7 (sin), 2.39e-7 (cos) on 69678 points, both builds; axis_angle_to_quat | |q| - 1 | <= 1.54e-7.
"""
import numpy as np
import pytest

import lane_lib as L
import lane_ref as R

pytestmark = pytest.mark.gpu

BUILDS = ["product", "ieee"]
_DEV = {}


def _dev(name):
    if name not in _DEV:
        _DEV[name] = L.Dev(ieee=name == "ieee")
    return _DEV[name]


@pytest.fixture(scope="module")
def emu():
    return L.Emu()


@pytest.fixture(scope="module", params=BUILDS)
def dev(request):
    return _dev(request.param)


def name_of(dev):
    return "ieee" if dev.ieee else "product"


def assert_same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "case, word", bad[0].tolist(), hex(got[tuple(bad[0])]), hex(want[tuple(bad[0])]), len(bad), "words differ in",
                           len(set(bad[:, 0].tolist())), "cases")


# ------------------------------------------------------------------------------------------------------------- G1, G2
@pytest.mark.parametrize("name", list(R.KINDS))
def test_generic_position_matches_the_fp64_oracle(dev, name):
    R.gate_g1(name, dev.geom(R.g1_cases(name)[0]), name_of(dev))


@pytest.mark.parametrize("gate", list(R.G2_GATES))
def test_degenerate_position_by_geometry(dev, gate):
    R.G2_GATES[gate](dev.geom, name_of(dev))


# ------------------------------------------------------------------------------------------------------------- G3
def mixed_rows(npairs=48):
    """the contact phase's layout: the kinds interleaved pair by pair, the subs of one pair in adjacent lanes (4 + 1 + 2 + 4 lanes a round)"""
    per = {name: (R.g1_cases(name)[0], nsub) for name, (_k, nsub) in R.KINDS.items()}
    edge = R.g1_cases("box_box")[0][4000:]
    rows = []
    for p in range(npairs):
        for name, (r, nsub) in per.items():
            rows.append(r[p * nsub:(p + 1) * nsub])
        rows.append(edge[4 * p:4 * p + 4])
    stacked = R.geom_rows(R.KIND_BOX_BOX, 4, R.stacked_pairs(npairs, 33, False))       # face contacts: the polygon in LDS is used
    return np.concatenate(rows + [stacked])


def test_layout_independence_bit_for_bit(dev):
    rows = mixed_rows()
    n = len(rows)
    base = dev.geom(rows)                                                               # (b) interleaved lane by lane
    assert not np.any(base == L.SENTINEL)
    # (a) one kind per wavefront: sorted by kind, every kind's block padded to a multiple of 64 with copies of its first row
    blocks, where = [], np.zeros(n, int)
    at = 0
    for kind in sorted(set(rows[:, 0].tolist())):
        idx = np.nonzero(rows[:, 0] == kind)[0]
        where[idx] = at + np.arange(len(idx))
        pad = (-len(idx)) % 64
        blocks += [rows[idx], np.repeat(rows[idx[:1]], pad, 0)]
        at += len(idx) + pad
    assert_same(dev.geom(np.concatenate(blocks))[where], base, "one kind per wavefront against interleaved")
    # (c) a partial last wavefront
    for m in (1, 63, 65):
        assert_same(dev.geom(rows[:m]), base[:m], ("n", m))
        assert_same(dev.geom(rows[n - m:]), base[n - m:], ("the last n", m))
    # (d) the polygon slices pre-filled with NaN
    assert_same(dev.geom(rows, fill=1), base, "slices pre-filled with NaN against zeros")
    big = R.g1_cases("box_box")[0]
    assert_same(dev.geom(big, fill=1), dev.geom(big, fill=0), "slices pre-filled with NaN against zeros, box-box")


# ------------------------------------------------------------------------------------------------------------- G4
def zero_sign_only(got, want, cols):
    """FINDING (MI355X, 2026-10-19), the one operation of this code that is not IEEE on the IEEE build: make_frame's Gram-Schmidt step
    `bb[k] -= a[k] * ab` for the component of bb that is the constant 0.f.  AMDGPU instruction selection folds `fsub 0.0, x` into the
    NEG source modifier of x's consumers whatever the fast-math flags (the ISA of make_frame holds v_mul_f32 v8, v2, v7 and then
    -v8 as operand of v_mul / v_div_scale / v_div_fixup, no v_sub), so 0.f - (+0.f) comes out as -0.f where IEEE gives +0.f.  It shows
    exactly where a[k] * ab is +0: an axis-aligned normal, e.g. boxes stacked on a face.  The words it reaches are frame rows 1-2, and
    only as the SIGN OF A ZERO: in those words a device -0 / emulator +0 pair (either way round) is accepted, every other bit of every
    word is compared.  Returns the number of such words."""
    diff = got != want
    zeros = ((got | want) & 0x7FFFFFFF) == 0
    allowed = np.zeros(got.shape, bool)
    allowed[:, cols] = True
    diff_ok = diff & zeros & allowed
    return np.where(diff_ok, want, got), int(diff_ok.sum())


def test_ieee_build_is_the_emulator_bit_for_bit(emu):
    """+ - x / sqrt and compares only: with the IEEE flags every one is correctly rounded on both sides.  A differing word is a finding;
    the one found is described, and admitted as narrowly as it can be, in zero_sign_only above."""
    dev = _dev("ieee")
    geom = [R.g1_cases(name)[0] for name in R.KINDS] + [mixed_rows()]
    geom += [R.geom_rows(R.KIND_PLANE_BOX, 4, R.flat_on_plane_pairs()), R.geom_rows(R.KIND_BOX_BOX, 4, R.stacked_pairs(200, 32, True)),
             R.geom_rows(R.KIND_BOX_BOX, 4, R.axis_aligned_pairs()), R.geom_rows(R.KIND_BOX_BOX, 4, R.park_threshold_pairs())]
    nzero = 0
    for k, rows in enumerate(geom):
        want = emu.geom(rows)
        got, nz = zero_sign_only(dev.geom(rows), want, slice(7, 13))
        assert_same(got, want, ("geom", k))
        nzero += nz
    seg = R.seg_rows()
    want = emu.seg(seg)
    raw = dev.seg(seg)
    got, nz = zero_sign_only(raw, want, slice(3, 9))
    got[seg[:, 0] != L.S_FRAME] = raw[seg[:, 0] != L.S_FRAME]                           # (the exception is make_frame's alone)
    assert_same(got, want, "seg")
    print(f"\nG4: {nzero + nz} frame words differ from the emulator's in the sign of a zero")
    x = R.fkey_inputs()[:, None].view(np.int32)
    assert_same(dev.key(L.K_FKEY, x), emu.key(L.K_FKEY, x), "fkey")
    p = R.pack_inputs().view(np.int32)
    assert_same(dev.key(L.K_PACK, p), emu.key(L.K_PACK, p), "ls_pack")
    arr = R.update_keys()
    for op, pars in ((L.K_UPDATE, (0, 1)), (L.K_LAZY, (0, 1, 2))):
        for par in pars:
            assert_same(dev.key(op, arr, par), emu.key(op, arr, par), ("key op", op, par))
    g = R.gate_inputs()
    assert_same(dev.key(L.K_GATE, g), emu.key(L.K_GATE, g), "done test")
    for rule in (0, 1):
        for minmax in (True, False):
            assert_same(dev.key_uniform(R.uniform_keys(), rule, minmax), emu.key_uniform(R.uniform_keys(), rule, minmax), ("uniform", rule, minmax))


# ------------------------------------------------------------------------------------------------------------- G5
def test_segment_helpers_and_make_frame(dev):
    R.gate_segments(dev.seg(R.seg_rows()), name_of(dev))


# ------------------------------------------------------------------------------------------------------------- G6
def test_keys_are_the_numpy_keys(dev):
    """+-0, +-denormals, +-DM_FLT_MIN, +-1 and its neighbours, +-3e38, +-inf, 4096 random floats: fkey and fkeyf bit-identical to
    test_ls_bracket._fkey; both zeros share key 0, order preserved, denormals not flushed"""
    R.gate_fkey(dev.key(L.K_FKEY, R.fkey_inputs()[:, None].view(np.int32)), name_of(dev))


def test_ls_pack(dev, emu):
    p = R.pack_inputs().view(np.int32)
    R.gate_pack(dev.key(L.K_PACK, p), emu.key(L.K_PACK, p), dev.ieee, name_of(dev))


def test_bracket_update_per_lane(dev):
    """the case set of test_ls_bracket (0.65 M rows): ls_update (both rules), ls_update_lazy<true> (both rules) and <false>, one case a lane"""
    R.gate_update(dev, name_of(dev))


def test_done_test_forms(dev):
    R.gate_done_test(dev.key(L.K_GATE, R.gate_inputs()), name_of(dev))


def test_bracket_update_wave_uniform(dev):
    R.gate_uniform(dev, name_of(dev))


def test_open_and_result(dev):
    R.gate_open_result(dev, name_of(dev))


# ------------------------------------------------------------------------------------------------------------- G7
def test_fast_sincos_and_axis_angle_to_quat(dev):
    """65536 points on [-pi, pi], 4096 on [-1e-3, 1e-3], the half-ranges of every hinge of the shipped models: |error| <= 1.2e-6
    (dmath.h's 1e-6 + 2e-7 for rounding x / 2 pi); axis_angle_to_quat a unit quaternion within 3e-6"""
    R.gate_trig(dev.trig(R.trig_rows()), name_of(dev))
