"""Every primitive of dial_mpc_amd/csrc/wave.h on the device against its definition.  The cases of tests/wave_prims/prim_cases.h are
compiled for gfx950 twice -- product flags (-DDIAL_FUSED_DPP, contraction, fast math) and IEEE flags -- and for the host emulator;
tests/test_wave_prims_emu.py pins the emulator to NumPy statements of wave.h's comments, this file pins the device to the emulator:

  1. data movement (DPP shifts and broadcasts, v_permlane16/32_swap, ds_bpermute gathers and reversals): bit-identical, on inputs
     that include +-0, +-inf, denormals and NaNs with distinct payloads -- a move must not touch a bit, a filled lane holds +0;
  2. ballots, lane predicates and stream compaction;
  3. sums: (a) bit-identical to the device's documented association stated on the host, (b) within d 2^-24 sum|v| of the fp64 sum
     (d = depth of that association, not a measurement), (c) replicated results agree in every lane of their group;
  4. the contraction regression (wave.h: WaveH::opaque): a product formed next to the reduction must not be fused into it;
  5. the fused DPP arithmetic of the product build (hand-written v_fmac_f32_dpp / v_mul_f32_dpp / v_rcp_f32_dpp) against std::fmaf;
  6. every WaveH case again with only one half executing it, and with the two halves in the two arms of one branch.

Measured once on an MI355X, 2026-10-18, the same on the product and on the IEEE build: worst sum error 0.588 of its bound (register
sums, Wave and WaveH), 0.146 (Wave) / 0.180 (WaveH) for the item sums; worst rcp_pick error 0.711 ulp."""
import numpy as np
import pytest

import prim_lib as PL
import prim_ref as R

pytestmark = pytest.mark.gpu

BUILDS = ["product", "ieee"]
HALF_CASES = [c for c in range(len(R.CASE_NAMES)) if c != PL.C_COMPACT]
_DEV = {}


@pytest.fixture(scope="module")
def emu():
    return PL.Emu()


@pytest.fixture(scope="module", params=BUILDS)
def dev(request):
    if request.param not in _DEV:
        _DEV[request.param] = PL.Dev(ieee=request.param == "ieee")
    return _DEV[request.param]


def assert_same(got, want, what):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "set, slot, lane", bad[0].tolist(), hex(got[tuple(bad[0])]), hex(want[tuple(bad[0])]), len(bad), "words differ")


def run(side, case, x, par, half2):
    return side.half(case, x, par) if half2 else side.wave(case, x, par)


# ------------------------------------------------------------------------------------------------------------- 1, 2. moves, ballots
@pytest.mark.parametrize("half2", [False, True], ids=["Wave", "WaveH"])
@pytest.mark.parametrize("case", [PL.C_ROW, PL.C_PICK, PL.C_BCAST, PL.C_PERM, PL.C_MASK, PL.C_COMPACT],
                         ids=lambda c: R.CASE_NAMES[c])
def test_moves_and_ballots_are_bit_identical_to_the_emulator(emu, dev, case, half2):
    """Shifts N in 1..4 (every N the kernels use, and 3), row_bcast K in 0..15, pick / WaveH::bc K in 0..31, Wave::bc K in {0, 15, 16,
    31, 32, 63}, rowbc, dup_rows, dup_halves, grp8_bcast3, gather64 / gather, lane_reverse n in {1, 18, 22, 26, 32 (, 64)}; mask with
    different predicates in the two halves, lane_gt / eq / lt, compact at counts {0, 1, 31, 32, 33, 64} (ascending lanes, words past
    the count untouched).  Every result word, and every word no case writes (the sentinel), must match the emulator."""
    for x, par in R.launches(emu, case, half2):
        what = (R.CASE_NAMES[case], "WaveH" if half2 else "Wave", "par", par)
        got = run(dev, case, x, par, half2)
        assert_same(got, run(emu, case, x, par, half2), what)
        R.check_slots(got, R.ref_case(case, x, half2, par), what)       # (and the NumPy statement, directly)


# ------------------------------------------------------------------------------------------------------------- 3. sums
DEPTH = {64: 6, 32: 5, 16: 4, 8: 3}


def group_check(got, v, g, extra, what):
    """(b), (c) for one result slot: got [nset, 64] float32 holds, in every lane, the sum of its aligned group of g lanes of v.
    Returns the worst error as a fraction of the bound (depth(g) + extra) 2^-24 sum|v|."""
    n = len(v)
    gb = R.u32(got).reshape(n, 64 // g, g)
    assert np.all(gb == gb[:, :, :1]), (what, "lanes of one group hold different bits")
    v64 = v.astype(np.float64).reshape(n, 64 // g, g)
    err = np.abs(got.reshape(n, 64 // g, g)[:, :, 0].astype(np.float64) - v64.sum(-1))
    bound = (DEPTH[g] + extra) * R.EPS * np.abs(v64).sum(-1)
    assert np.all(err <= bound), (what, "error over bound", float((err / np.maximum(bound, 1e-300)).max()))
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


def row16_expected(emu, v):
    return np.array([[emu.row_tree(s[16 * g:16 * g + 16]) for g in range(4) for _ in range(16)] for s in v], np.float32)


@pytest.mark.parametrize("half2", [False, True], ids=["Wave", "WaveH"])
def test_register_sums(emu, dev, half2):
    """vsum, vsumN<3>, row16_sum, row16_sum3, row16_sumN<2>, seg8_sumN<2>.  (a): vsum / vsumN equal emu_tree64 (Wave) / emu_tree32
    (WaveH) and seg8_sumN equals the emulator's.  For the row16_* family the expected value is emu_row_tree of the group -- the
    DEVICE's association (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) -- NOT the emulator's row16_sum, which adds the 16 lanes
    one after the other and is only compared at a tolerance elsewhere."""
    (x, par), = R.launches(emu, PL.C_VSUMS, half2)
    got = run(dev, PL.C_VSUMS, x, par, half2)
    e = run(emu, PL.C_VSUMS, x, par, half2)
    a, b, c = x[:, 0], x[:, 1], x[:, 2]
    LW = 32 if half2 else 64
    tree = emu.tree32 if half2 else emu.tree64
    for slot, v in ((0, a), (1, a), (2, b), (3, c)):
        want = np.array([[tree(s[h:h + LW]) for h in range(0, 64, LW) for _ in range(LW)] for s in v], np.float32)
        assert_same(got[:, slot], R.u32(want), ("vsum", slot))
    for slot, v in ((4, a), (5, a), (6, b), (7, c), (8, b), (9, c)):
        assert_same(got[:, slot], R.u32(row16_expected(emu, v)), ("row16", slot))
    assert_same(got[:, 10:12], e[:, 10:12], "seg8_sumN")
    assert_same(got[:, :4], e[:, :4], "vsum vs emulator")
    assert np.all(got[:, 12:] == PL.SENTINEL)
    R.check_slots(got, R.ref_case(PL.C_VSUMS, x, half2, par, row16_tree=True), "vsums vs NumPy")
    worst = 0.0
    f = got.view(np.float32)
    for slot, v, g in ((0, a, LW), (1, a, LW), (2, b, LW), (3, c, LW), (4, a, 16), (5, a, 16), (6, b, 16), (7, c, 16), (8, b, 16),
                       (9, c, 16), (10, a, 8), (11, c, 8)):
        worst = max(worst, group_check(f[:, slot], v, g, 0, ("vsums slot", slot)))
    print(f"\n{'WaveH' if half2 else 'Wave'} ({'ieee' if dev.ieee else 'product'}): register sums, worst error {worst:.3g} of its bound")


@pytest.mark.parametrize("half2", [False, True], ids=["Wave", "WaveH"])
def test_item_sums_and_max(emu, dev, half2):
    """sum, sum3 at counts {0, 1, 17, 64, 65, 220} (Wave) / {0, 1, 17, 32, 33, 72} (WaveH): bit-identical to the emulator with
    tree_sums (lane-strided partial sums, then the tree) and within (d + ceil(count / stride) - 1) 2^-24 sum|v| of fp64.  maxv (Wave):
    bit-identical to the maximum -- an all-negative set, ties, count 0 (-inf), counts on both sides of the lane stride; no NaNs (the
    product build is -fno-honor-nans)."""
    LW = 32 if half2 else 64
    worst = 0.0
    for x, count in R.launches(emu, PL.C_FSUMS, half2):
        got = run(dev, PL.C_FSUMS, x, count, half2)
        assert_same(got, run(emu, PL.C_FSUMS, x, count, half2), ("fsums", count))
        R.check_slots(got, R.ref_case(PL.C_FSUMS, x, half2, count), ("fsums vs NumPy", count))
        f = got.view(np.float32)
        extra = max(-(-count // LW) - 1, 0)
        for slot, sign in ((0, 1.0), (1, 1.0), (2, 1.0), (3, -1.0)):
            for h in range(0, 64, LW):
                it = np.array([[x[k, i // LW, h + i % LW] for i in range(count)] for k in range(len(x))], np.float64).reshape(len(x), count)
                res = f[:, slot, h:h + LW]
                assert np.all(R.u32(res) == R.u32(res[:, :1])), ("fsums", count, "lanes disagree")
                err = np.abs(res[:, 0].astype(np.float64) - sign * it.sum(1))
                bound = (DEPTH[LW] + extra) * R.EPS * np.abs(it).sum(1)
                assert np.all(err <= bound), ("fsums", count, slot, float((err / np.maximum(bound, 1e-300)).max()))
                if np.any(bound > 0):
                    worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        if not half2:
            it = x.reshape(len(x), -1)[:, :count]
            want = it.max(1) if count else np.full(len(x), -np.inf, np.float32)
            assert_same(got[:, 4], R.u32(np.repeat(want[:, None], 64, 1)), ("maxv", count))
    print(f"\n{'WaveH' if half2 else 'Wave'} ({'ieee' if dev.ieee else 'product'}): item sums, worst error {worst:.3g} of its bound")


# ------------------------------------------------------------------------------------------------------------- 4. contraction
def test_a_product_is_not_contracted_into_the_butterfly(emu, dev):
    """WaveH: the summand a[l] * b[l] is formed in the case body and fed straight into vsum, row16_sum and sum.  On inputs where
    fma(a_l, b_l, round(a_l' b_l')) differs from round(a_l b_l) + round(a_l' b_l') in at least a quarter of the lanes (asserted by
    prim_ref.contraction_inputs with std::fmaf), all 32 lanes of a half must agree bit for bit and hold the tree sum of the
    SEPARATELY rounded products.  This is what WaveH::opaque is for; without it the lanes of a half disagree in the last bit on the
    product build."""
    (x, par), = R.launches(emu, PL.C_CONTRACT, True)
    got = dev.half(PL.C_CONTRACT, x, par)
    for slot, g in ((0, 32), (1, 16), (2, 32)):
        gb = got[:, slot].reshape(len(x), 64 // g, g)
        assert np.all(gb == gb[:, :, :1]), ("the lanes of a group disagree", slot, int((gb != gb[:, :, :1]).sum()))
    p = emu.mulf(x[:, 0], x[:, 1])
    want = {0: R.half_rep(R.tree64, p, True), 1: row16_expected(emu, p), 2: R.half_rep(R.tree64, p, True)}
    R.check_slots(got, {s: R.u32(v) for s, v in want.items()}, "contraction")


# ------------------------------------------------------------------------------------------------------------- 5. fused DPP arithmetic
@pytest.mark.parametrize("half2", [False, True], ids=["Wave", "WaveH"])
def test_fused_dpp_arithmetic(emu, dev, half2):
    """fma_pick / fnma_pick / mul_pick for every K in 0..31 on the X | Y of dup_rows, normal numbers only; with the first consumer
    immediately after dup_rows in source order (the s_nop 1 in dup_rows) and with three dependent VALU results the consumer needs
    written in between (source order does not bind the scheduler: two instruction streams, not a guaranteed distance).  Product build: fma / fnma
    are std::fmaf(other, +-pick, acc), ONE rounding (computed in C: prims_emu.cpp).  IEEE build: the emulator's two roundings.  Both:
    mul_pick is the product."""
    half = R.P & 32
    for case in (PL.C_FMA, PL.C_FNMA, PL.C_MUL):
        for x, par in R.launches(emu, case, half2):
            got = run(dev, case, x, par, half2)
            e = run(emu, case, x, par, half2)
            if case != PL.C_MUL and not dev.ieee:
                v, other, acc = x[:, 0], x[:, 1], x[:, 2]
                for k in range(32):
                    pk = v[:, half | k]
                    e[:, k] = R.u32(emu.fmaf(other, pk if case == PL.C_FMA else -pk, acc))
            assert_same(got, e, (R.CASE_NAMES[case], "near" if par == 0 else "far"))


@pytest.mark.parametrize("half2", [False, True], ids=["Wave", "WaveH"])
def test_rcp_pick(emu, dev, half2):
    """rcp_pick<K>, K in 0..31: bit-identical to fast_rcp of the same lane's broadcast in the same kernel, and within 1 ulp of the
    fp64 reciprocal of THAT lane (the accuracy the CDNA ISA documents for V_RCP_F32); no word outside its slots is written."""
    worst = 0.0
    for x, par in R.launches(emu, PL.C_RCP, half2):
        got = run(dev, PL.C_RCP, x, par, half2)
        assert_same(got[:, :32], got[:, 32:64], ("rcp_pick vs fast_rcp", par))
        live = R.ref_case(PL.C_RCP, x, half2, par)                        # the far variant's live chain, and nothing else written
        R.check_slots(got[:, 64:], {s - 64: e for s, e in live.items() if s >= 64}, ("rcp: slots past its own", par))
        v = x[:, 0]
        for k in range(32):
            exact = 1.0 / v[:, (R.P & 32) | k].astype(np.float64)
            ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
            err = np.abs(got[:, k].view(np.float32).astype(np.float64) - exact) / ulp
            worst = max(worst, float(err.max()))
    print(f"\n{'WaveH' if half2 else 'Wave'} ({'ieee' if dev.ieee else 'product'}): rcp_pick, worst error {worst:.3g} ulp")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------- 6. divergent halves
@pytest.mark.parametrize("case", HALF_CASES, ids=lambda c: R.CASE_NAMES[c])
def test_divergent_halves(emu, dev, case):
    """Every WaveH case with only half 0 executing it, only half 1, and half 0 executing it in the `if` while half 1 executes ANOTHER
    case in the `else`: the active half's words are bit-identical to the convergent run, the inactive half's still hold the sentinel."""
    other = HALF_CASES[(HALF_CASES.index(case) + 5) % len(HALF_CASES)]
    opar = R.launches(emu, other, True)[-1][1]
    for x, par in R.launches(emu, case, True):
        conv = dev.half(case, x, par)
        oconv = dev.half(other, x, opar)
        lo, hi = slice(0, 32), slice(32, 64)
        for mode, act, idle in ((1, lo, hi), (2, hi, lo)):
            got = dev.half(case, x, par, mode=mode)
            assert_same(got[:, :, act], conv[:, :, act], (R.CASE_NAMES[case], "mode", mode))
            assert np.all(got[:, :, idle] == PL.SENTINEL), (R.CASE_NAMES[case], "mode", mode, "the idle half wrote")
        got = dev.half(case, x, par, mode=3, case1=other, par1=opar)
        assert_same(got[:, :, lo], conv[:, :, lo], (R.CASE_NAMES[case], "if-arm"))
        assert_same(got[:, :, hi], oconv[:, :, hi], (R.CASE_NAMES[other], "else-arm next to", R.CASE_NAMES[case]))
