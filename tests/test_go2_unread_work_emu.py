"""The Go2 walk's deferring wave without the work no output reads (csrc/wave.h: WaveD::solver_cap_exit, WaveD::lean_tail_cut), on
the host wave emulator, no GPU needed.

rollout_sample on a WaveD -- the Newton loop ends when the iteration cap is reached, and the last control step of a rollout that
stores neither q nor qd ends behind the position stage, without a solve -- must give the bits of rollout_sample on a Wave, which runs
every pass and every phase: both changes only remove operations.  Full rollouts (every per-step output) and lean ones (qss, qdss and
xss null), with the race detector off (ascending lane order) and on (both lane orders, the descending one's image kept).

The harness (tests/reward_defer/unread_emu.cpp) also counts how the solves end; the inputs must produce both kinds of exit -- by
tolerance (the state in the air: no active row, niter = 0) and at the cap (feet on the floor) -- or the comparison would not see the
changed exit at work."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import go2_unread_cases as C
import oracle as O
from conftest import seeded_inputs, with_solver
from dial_mpc_amd import _abi

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reward_defer")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dial_mpc_amd", "csrc")
_SO = os.path.join(_HERE, "libunread_emu.so")
FULL = ("Y0s", "rewss", "rews", "qss", "qdss", "xss")
LEAN = ("Y0s", "rewss", "rews")
N = 8
# (H, iteration caps): H = 6 -> T = 7 and H = 1 -> T = 2, the smallest rollout the stash allows; cap 1 is the solver's `max_iter == 1`
# branch, 2 the shipped cap, 3 a cap above it
CASES = [(16, (2,)), (6, (1, 3)), (1, (1, 2, 3))]


def _build():
    src = os.path.join(_HERE, "unread_emu.cpp")
    deps = [src, _abi.HEADER] + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")]
    if os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(f) for f in deps):
        return _SO
    tmp = f"{_SO}.{os.getpid()}.tmp"   # atomic: parallel test workers may all find the library stale at once
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fno-strict-aliasing", "-ffp-contract=off", "-DDIAL_EMU",
                           "-o", tmp, src])
    os.replace(tmp, _SO)
    return _SO


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(_build())


def _rollout(lib, model, task, cfg, state, Ybar, sigma, eps, defer, check_races, lean):
    Hn1, T, B = cfg.Hnode + 1, cfg.Hsample + 1, cfg.Nsample + 1
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))  # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    state, Ybar, eps, ns = f32(state), f32(Ybar), f32(eps), f32(sigma).reshape(-1)
    out = dict(Y0s=np.zeros((B, Hn1, model.nu), np.float32), rewss=np.zeros((B, T), np.float32), rews=np.zeros(B, np.float32),
               qss=np.zeros((B, T, model.nq), np.float32), qdss=np.zeros((B, T, model.nv), np.float32),
               xss=np.zeros((B, T, (model.nbody - 1) * 3), np.float32))
    exits = (ctypes.c_int * 2)()
    rc = lib.unread_emu_rollout(ctypes.byref(model), ctypes.byref(task), ctypes.byref(cfg), p(state), p(eps), p(Ybar), p(ns), int(ns.size),
                                cfg.Nsample, B, T, Hn1, *(None if lean and k in ("qss", "qdss", "xss") else p(out[k]) for k in FULL),
                                int(check_races), int(defer), exits)
    assert rc == 0, f"unread_emu_rollout: rc = {rc} (> 0: phases that depend on the lane order, < 0: error)"
    return out, (exits[0], exits[1])


@pytest.fixture(scope="module", params=CASES, ids=[f"H{h}" for h, _ in CASES])
def case(request, lib):
    """N = 8 noisy rollouts + the mean trajectory from the rest pose, a perturbed state and a state in the air (class F, selected with
    the fp64 oracle), at every iteration cap of the case; every variant once: (wave, lane orders, lean)."""
    H, caps = request.param
    dc, env, model, task, cfg = C.setup(N, H)
    states = C.start_states(env, model, O.Oracle(model, task, cfg, np.float32))
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=3, Ybar_scale=0.3)
    runs = {}
    for cap in caps:
        m = with_solver(model, iterations=cap)
        for sname, s0 in states.items():
            for d in (0, 1):
                for r in (0, 1):
                    for lean in (False, True):
                        runs[(cap, sname, d, r, lean)] = _rollout(lib, m, task, cfg, s0, Ybar, sigma, eps, d, r, lean)
    return runs, caps, tuple(states)


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("races", [0, 1], ids=["ascending", "both-orders"])
def test_removed_work_changes_no_bit(case, races, lean):
    runs, caps, states = case
    for cap in caps:
        for sname in states:
            ref, _ = runs[(cap, sname, 0, races, lean)]
            got, _ = runs[(cap, sname, 1, races, lean)]
            assert np.all(np.isfinite(ref["rewss"])) and ref["rewss"].std() > 0
            for k in (LEAN if lean else FULL):
                assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (cap, sname, k)


def test_lean_equals_full(case):
    """the cut step stores the same last step reward: a lean rollout's rewards are the full rollout's"""
    runs, caps, states = case
    for cap in caps:
        for sname in states:
            for k in LEAN:
                assert np.array_equal(runs[(cap, sname, 1, 0, True)][0][k].view(np.uint32), runs[(cap, sname, 1, 0, False)][0][k].view(np.uint32))


def test_inputs_leave_the_solver_both_ways(case):
    """per iteration cap: solves that end by tolerance AND solves that end at the cap, on both waves; the state in the air ends
    its first solve by tolerance, the rest pose reaches the cap"""
    runs, caps, states = case
    for cap in caps:
        for d in (0, 1):
            tol = sum(runs[(cap, s, d, 0, False)][1][0] for s in states)
            at_cap = sum(runs[(cap, s, d, 0, False)][1][1] for s in states)
            print(f"cap {cap}, {'WaveD' if d else 'Wave'}: {tol} solves end by tolerance, {at_cap} at the cap")
            # (cap 1: the solver's `max_iter == 1` branch tests no tolerance -- every solve runs its one iteration)
            assert at_cap > 0 and (tol > 0) == (cap != 1), (cap, d, tol, at_cap)
        assert (runs[(cap, "air", 1, 0, False)][1][0] > 0 or cap == 1) and runs[(cap, "rest", 1, 0, False)][1][1] > 0
        # both waves take the same exits in full rollouts; a lean WaveD rollout skips the solve of its last step
        assert runs[(cap, "rest", 1, 0, False)][1] == runs[(cap, "rest", 0, 0, False)][1]
        B = N + 1
        assert sum(runs[(cap, "rest", 1, 0, True)][1]) == sum(runs[(cap, "rest", 1, 0, False)][1]) - B
