"""Deferred step rewards of the Go2 walk (csrc/wave.h: WaveD) on the host wave emulator, no GPU needed.

rollout_sample with a stash -- every step stores what its reward reads, the step rewards are evaluated once per rollout, control
step t in lane t -- must give the bits of rollout_sample without one (the reward lane of every step): same term code on the same
input words, compiled without contraction, added to the fp64 sum in the same order.  Both with the race detector off (phases run
in ascending lane order) and on (every phase run in both lane orders from one LDS snapshot, the descending one's image kept; no
phase may depend on the order)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from conftest import perturbed_state, seeded_inputs, setup_case
from dial_mpc_amd import _abi

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reward_defer")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dial_mpc_amd", "csrc")
_SO = os.path.join(_HERE, "libdefer_emu.so")
KEYS = ("Y0s", "rewss", "rews", "qss", "qdss", "xss")


def _build():
    src = os.path.join(_HERE, "defer_emu.cpp")
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


def _rollout(lib, model, task, cfg, state, Ybar, sigma, eps, defer, check_races):
    N, Hn1, T, B = cfg.Nsample, cfg.Hnode + 1, cfg.Hsample + 1, cfg.Nsample + 1
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))  # noqa: E731
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    state, Ybar, eps, ns = f32(state), f32(Ybar), f32(eps), f32(sigma).reshape(-1)
    out = dict(Y0s=np.zeros((B, Hn1, model.nu), np.float32), rewss=np.zeros((B, T), np.float32), rews=np.zeros(B, np.float32),
               qss=np.zeros((B, T, model.nq), np.float32), qdss=np.zeros((B, T, model.nv), np.float32),
               xss=np.zeros((B, T, (model.nbody - 1) * 3), np.float32))
    rc = lib.defer_emu_rollout(ctypes.byref(model), ctypes.byref(task), ctypes.byref(cfg), p(state), p(eps), p(Ybar), p(ns), int(ns.size),
                               N, B, T, Hn1, *(p(out[k]) for k in KEYS), int(check_races), int(defer))
    assert rc == 0, f"defer_emu_rollout: rc = {rc} (> 0: phases that depend on the lane order, < 0: error)"
    return out


@pytest.fixture(scope="module", params=[16, 5], ids=["H16", "H5"])
def case(request, lib):
    """N = 8 noisy rollouts + the mean trajectory from a perturbed state (feet in and out of contact), every variant once."""
    dc, env, model, task, cfg = setup_case("unitree_go2_trot", 8, request.param)
    o32 = O.Oracle(model, task, cfg, np.float32)
    q, qd = perturbed_state(env, 1)
    s0, _, _ = o32.env_reset(q, qd)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=3, Ybar_scale=0.3)
    runs = {(d, r): _rollout(lib, model, task, cfg, s0, Ybar, sigma, eps, d, r) for d in (0, 1) for r in (0, 1)}
    return runs, cfg


@pytest.mark.parametrize("races", [0, 1], ids=["ascending", "both-orders"])
def test_deferred_rewards_are_bit_identical(case, races):
    runs, cfg = case
    step, defer = runs[(0, races)], runs[(1, races)]
    assert np.all(np.isfinite(step["rewss"])) and step["rewss"].std() > 0 and np.unique(step["rewss"]).size > cfg.Nsample
    for k in KEYS:
        assert np.array_equal(defer[k].view(np.uint32), step[k].view(np.uint32)), k


def test_lane_order_changes_nothing(case):
    runs, _ = case
    for k in KEYS:
        assert np.array_equal(runs[(1, 0)][k].view(np.uint32), runs[(1, 1)][k].view(np.uint32)), k


def test_mean_reward_is_the_ordered_fp64_sum(case):
    """rews = the fp64 sum of the T step rewards in ascending step order, divided by T, rounded once."""
    runs, cfg = case
    d = runs[(1, 0)]
    T = cfg.Hsample + 1
    acc = np.zeros(d["rewss"].shape[0], np.float64)
    for t in range(T):
        acc += d["rewss"][:, t].astype(np.float64)
    assert np.array_equal((acc / T).astype(np.float32).view(np.uint32), d["rews"].view(np.uint32))
