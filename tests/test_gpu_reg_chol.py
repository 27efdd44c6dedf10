"""The register L D L^T of dial_mpc_amd/csrc/solver_reg.h (reg_chol_solve_v, reg_chol_solve2, their REUSE path) on the device against
fp64, for every square instantiation with the topologies rollout_body.h passes for it: Go2, H1, H1 loco and the Allegro on their dof
trees (M, M + dt B, the pyramidal H), the Allegro with TopoDense (the cone solver's H), and the generic path's DimsPadV squares
(solve_spd_reg / solve_sq_reg): 18 on the Go2's tree (crate climb, M and H), 26 on the H1's tree plus the crate's own root (push crate,
M), 26 dense (push crate, H: Dims::h_dense) and the capacity dimension 28 dense; reg_chol_solve2 also on WaveH for the Go2, a different
system in each half.  Inputs (tests/prim_ref.py): SPD matrices exactly on the pattern, sigma in {1, 1e-2, 1e-4} x 20 seeds
(kappa 2e1 .. 5e5), the same with rows scaled by 1e-3 .. 1e3, and the real M and M + J^T D J of every model at its initial pose from
the fp64 oracle; right-hand-side lanes >= N hold NaN.

Gates, on the product build and on the IEEE build:
  1. ||x - x64||_inf / ||x64||_inf <= C kappa_2(A) 2^-24 against np.linalg.solve on the fp32-rounded system, C = 4 x the worst ratio
     the EMULATOR reaches on the same inputs (computed at run time; the 4 covers the device's 1-ulp v_rcp_f32 and the product build's
     contraction against the emulator's correctly rounded arithmetic);
  2. IEEE build: the v_readlane form, the DPP form and each half of the half-wave form are bit-identical;
  3. REUSE is bit-identical to the fresh solve -- IEEE build: both forms; product build: the DPP form (both paths spell the same
     instructions); reg_chol_solve_v on the product build is held to gate 1 and the test reports whether the bits agree;
  4. after a fresh solve every word of `scratch` off the pattern and in the pad columns is +0 -- also when all N x N words the solve
     may write held NaN before (the pad columns are never written: they keep the zeros init_square gave them) -- the words on the
     pattern are the unit-lower factor of the fp64 L D L^T in the same elimination direction and the reciprocals are 1 / d_k, both
     within the bound of gate 1;
  5. a fresh solve into a NaN-filled scratch, into one that holds another system's factor (NaN in its pad columns), or into the
     storage of A itself, gives the same bits as into a zeroed scratch.

Worst ratio of gate 1 over all forms, fresh and REUSE, in units of kappa 2^-24 -- measured once on an MI355X, 2026-10-18, 122 systems
per instantiation (device product build / device IEEE build / emulator; the gate is 4 x the emulator's figure):
    go2            0.116  / 0.170  / 0.170        h1             0.0912 / 0.0987 / 0.0845        h1loco   0.111 / 0.169 / 0.139
    allegro        0.304  / 0.429  / 0.429        allegro_dense  0.280  / 0.465  / 0.334
On the product build reg_chol_solve_v's REUSE solve was bit-identical to its fresh solve for these five as well.
The four DimsPadV instantiations (crate_climb, push_crate, push_crate_dense, capacity_dense) were added after that run and HAVE NOT
BEEN MEASURED ON A DEVICE: no device ratio is recorded for them.  Their emulator ratios on the same 122 systems are 0.170, 0.0986,
0.518 and 0.392; the test prints the device's next to them when it runs."""
import numpy as np
import pytest

import prim_lib as PL
import prim_ref as R

pytestmark = pytest.mark.gpu

FORM_NAMES = {0: "reg_chol_solve_v", 1: "reg_chol_solve2", 2: "reg_chol_solve2 / WaveH"}
_DEV = {}


@pytest.fixture(scope="module")
def emu():
    return PL.Emu()


@pytest.fixture(scope="module", params=["product", "ieee"])
def dev(request):
    if request.param not in _DEV:
        _DEV[request.param] = PL.Dev(ieee=request.param == "ieee")
    return _DEV[request.param]


def same(a, b):
    return np.array_equal(R.u32(a), R.u32(b))


def rel(got, want):
    """per system: ||got - want||_max / ||want||_max"""
    n = len(got)
    return np.abs(got.astype(np.float64) - want).reshape(n, -1).max(1) / np.abs(want).reshape(n, -1).max(1)


@pytest.mark.parametrize("name", list(PL.INST))
def test_reg_chol_against_fp64(emu, dev, name):
    A, b = R.all_systems(name)
    N = PL.INST[name][1]
    _, C, emu_worst = R.emu_chol(emu, name)
    assert emu_worst < 1.0, "the emulator itself is outside kappa eps: the gate derived from it would mean nothing"
    forms = (0, 1, 2) if name == "go2" else (0, 1)
    res = {f: dev.chol(name, f, A, b) for f in forms}
    kappa = np.array([np.linalg.cond(a.astype(np.float64)) for a in A])
    fac = [R.ldlt64(a) for a in A]
    Lf, dinv64 = np.stack([f[0] for f in fac]), np.stack([1.0 / f[1] for f in fac])
    on = np.tril(R.anc_mask(name), -1)
    worst, build = 0.0, "ieee" if dev.ieee else "product"
    for f, r in res.items():
        what = (name, build, FORM_NAMES[f])
        assert np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["x_reuse"])), (what, "a NaN of the idle lanes reached the result")
        # gate 1
        for key in ("x", "x_reuse"):
            ratio = R.chol_ratio(A, b, r[key])
            worst = max(worst, ratio.max())
            print(f"\n{name} ({build}) {FORM_NAMES[f]} {key}: worst {ratio.max():.3g} kappa eps (gate {C:.3g}, emulator {emu_worst:.3g})", end="")
            assert ratio.max() <= C, (what, key, "system", int(ratio.argmax()), float(ratio.max()), "gate", C)
        # gate 3
        agree = same(r["x_reuse"], r["x"])
        if dev.ieee or f != 0:
            assert agree, (what, "REUSE differs from the fresh solve in", int((R.u32(r["x_reuse"]) != R.u32(r["x"])).sum()), "words")
        else:
            print(f"\n{name} ({build}) {FORM_NAMES[f]}: REUSE {'is' if agree else 'is NOT'} bit-identical to the fresh solve", end="")
        # gate 4
        scr = R.u32(r["scratch"])
        assert np.all(scr[:, :, :N][:, ~on] == 0) and np.all(scr[:, :, N:] == 0), (what, "scratch off the pattern is not +0")
        bound = C * kappa * R.EPS
        eL = rel(r["scratch"][:, :, :N], Lf)
        eD = rel(r["dinv"], dinv64)
        assert np.all(eL <= bound), (what, "factor", int((eL / bound).argmax()), float((eL / bound).max()))
        assert np.all(eD <= bound), (what, "pivot reciprocals", int((eD / bound).argmax()), float((eD / bound).max()))
    # gate 2
    if dev.ieee:
        for f in forms[1:]:
            for key in ("x", "dinv", "scratch", "x_reuse"):
                assert same(res[f][key], res[0][key]), (name, FORM_NAMES[f], key, "differs from reg_chol_solve_v")
    # gates 4 and 5 on scratches that do not start as zeros: NaN in every word a solve may write (the kernel stores columns 0 .. N-1
    # only; the pad columns are never written and stay what they were: 0 here, as init_square leaves them), the previous system's
    # factor with NaN in the pad columns, and scratch = the storage of A
    for f in forms:
        nans = np.full_like(res[f]["scratch"], np.nan)
        nans[:, :, N:] = 0.0
        dirty = np.roll(res[f]["scratch"], 2, 0).copy()
        dirty[:, :, N:] = np.nan
        for tag, kw in (("NaN-filled", dict(scr0=nans)), ("another factor", dict(scr0=dirty)), ("alias", dict(alias=1))):
            again = dev.chol(name, f, A, b, **kw)
            what = (name, build, FORM_NAMES[f], tag)
            for key in ("x", "dinv", "x_reuse"):
                assert same(again[key], res[f][key]), (what, key, "depends on what scratch held")
            assert same(again["scratch"][:, :, :N], res[f]["scratch"][:, :, :N]), (what, "stale words in the factor")
            if tag == "NaN-filled":
                scr = R.u32(again["scratch"])
                assert np.all(scr[:, :, :N][:, ~on] == 0) and np.all(scr[:, :, N:] == 0), (what, "scratch off the pattern is not +0")
    print(f"\n{name} ({build}): worst device ratio {worst:.3g}, emulator {emu_worst:.3g}, gate {C:.3g}")
