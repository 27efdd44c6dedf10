"""The CPU leg of the wave.h / register L D L^T pins (tests/test_gpu_wave_prims.py and tests/test_gpu_reg_chol.py compare the DEVICE
with the emulator; this file is what their results stand on):
  * every case of tests/wave_prims/prim_cases.h on the emulator, bit for bit against a NumPy statement of the comment above the
    primitive in wave.h (tests/prim_ref.py) -- the definitions are pinned independently of the C++;
  * the device side of the same cases cross-compiles for gfx950 with the product and with the IEEE flags;
  * the emulator's register L D L^T: the v_readlane form, the DPP form and the half-wave form agree bit for bit, a REUSE solve is
    bit for bit the fresh solve, the LDS copy of the factor is an exact +0 off the pattern, and the error against fp64 in units of
    kappa_2(A) 2^-24 (printed per instantiation; between 0.0845 for the H1 and 0.518 for the dense 26 x 26 of the push crate when
    this was written) is what the device's gate is derived from."""
import os

import numpy as np
import pytest

import prim_lib as PL
import prim_ref as R


@pytest.fixture(scope="module")
def emu():
    return PL.Emu()


@pytest.mark.parametrize("half2", [False, True], ids=["Wave", "WaveH"])
@pytest.mark.parametrize("case", range(len(R.CASE_NAMES)), ids=R.CASE_NAMES)
def test_emulator_matches_the_definition(emu, case, half2):
    for x, par in R.launches(emu, case, half2):
        got = emu.half(case, x, par) if half2 else emu.wave(case, x, par)
        R.check_slots(got, R.ref_case(case, x, half2, par), (R.CASE_NAMES[case], "WaveH" if half2 else "Wave", "par", par))


def test_emulator_trees_match_their_numpy_statement(emu):
    """emu_row_tree / emu_tree64 / emu_tree32 (the associations the device's sums are held to) against tests/prim_ref.py"""
    for v in R.num_sets(1)[0]:
        assert R.u32(emu.tree64(v)) == R.u32(R.tree64(v)) and R.u32(emu.tree32(v)) == R.u32(R.tree32(v))
        assert R.u32(emu.row_tree(v[:16])) == R.u32(R.tree_row(v[:16]))


def test_input_sets_have_their_properties(emu):
    mv = R.move_sets().view(np.uint32)
    assert all(len(set(s.tolist())) >= 4 for s in mv) and len(set(mv[5].tolist())) == 64 and np.all(np.isnan(mv[5:7].view(np.float32)))
    a, b = R.contraction_inputs(emu)          # (asserts the part-4 property itself)
    assert a.shape == b.shape == (8, 64)
    for s in R.num_sets(4).reshape(-1, 64):
        assert np.any(s[:32] != s[32:]) and np.all(np.isfinite(s)) and np.all(np.abs(s) >= 2.0 ** -126)


@pytest.mark.parametrize("ieee", [False, True], ids=["product", "ieee"])
def test_device_library_cross_compiles(ieee):
    so = PL.build_dev(ieee)
    assert os.path.getsize(so) > 0


# ------------------------------------------------------------------------------------------------------------------ L D L^T
@pytest.mark.parametrize("name", list(PL.INST))
def test_emulator_reg_chol(emu, name):
    A, b = R.all_systems(name)
    N = PL.INST[name][1]
    res, C, worst = R.emu_chol(emu, name)
    for f, r in res.items():
        for key in ("x", "dinv", "scratch"):
            assert np.array_equal(R.u32(r[key]), R.u32(res[0][key])), (name, "form", f, key, "differs from the v_readlane form")
        assert np.array_equal(R.u32(r["x_reuse"]), R.u32(r["x"])), (name, "form", f, "REUSE differs from the fresh solve")
        assert np.all(np.isfinite(r["x"]))
    off = ~np.tril(R.anc_mask(name), -1)
    scr = R.u32(res[0]["scratch"])
    assert np.all(scr[:, :, :N][:, off] == 0) and np.all(scr[:, :, N:] == 0), "the LDS factor off the pattern / in the pad columns"
    nans = np.full_like(res[0]["scratch"], np.nan)       # NaN in every word a solve may write (the pad columns are never written)
    nans[:, :, N:] = 0.0
    dirty = np.roll(res[0]["scratch"], 2, 0).copy()      # another system's factor in scratch, NaN in its pad columns
    dirty[:, :, N:] = np.nan
    for f in res:
        for kw in (dict(scr0=nans), dict(scr0=dirty), dict(alias=1)):          # ... and scratch = the storage of A itself
            again = emu.chol(name, f, A, b, **kw)
            assert all(np.array_equal(R.u32(again[k]), R.u32(res[f][k])) for k in ("x", "dinv", "x_reuse")), (name, f, list(kw))
            assert np.array_equal(R.u32(again["scratch"][:, :, :N]), scr[:, :, :N]), (name, f, list(kw), "stale words in the factor")
        got = R.u32(emu.chol(name, f, A, b, scr0=nans)["scratch"])
        assert np.all(got[:, :, :N][:, off] == 0) and np.all(got[:, :, N:] == 0), (name, f, "NaN-filled scratch: off the pattern")
    print(f"\n{name}: emulator L D L^T vs fp64 on {len(A)} systems: worst {worst:.3g} kappa eps")
    assert worst < 1.0      # (backward-stable elimination: far inside kappa eps; the device's gate is 4 x this figure)
