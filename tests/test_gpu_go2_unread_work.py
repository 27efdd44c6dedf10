"""Work no output reads, removed from the Go2 walk's deferring kernel (csrc/wave.h: WaveD::solver_cap_exit, WaveD::lean_tail_cut).

The default context launches rollout_defer_kernel<DimsGo2>, whose Newton loop ends as soon as the iteration cap is reached and whose
last control step, in a launch that stores neither q nor qd (want_bars=False), ends behind the position stage (no solve).  A
context with no_defer_reward = 1 launches the untouched per-step kernel: every pass of the solver, every phase of every step.  Both
changes only remove operations, so on libdialhip_ieee.so AND on the product library everything either launch emits is compared bit
for bit.  Every comparison asserts through debug_last_launch which kernel ran on each side.

Cases: (N, H) = (64, 16), (63, 5), (100, 6) -- T = 7, the last relay piece is one step, the cut one -- and (8, 1), T = 2, the
smallest rollout the stash allows; the mean trajectory as relay pieces (from T = 4: shorter ones are never cut into pieces, which
the test asserts) and as one wavefront; the rest pose (contacts active, the cap
is reached), a perturbed state, and a state in the air (tests/smooth_ref.py class F: no active row, the solver stops by tolerance
with niter = 0); the model's iteration cap at 1 (the `max_iter == 1` branch), 2 (shipped) and 3; noise as data and drawn in the kernel."""
import os

import numpy as np
import pytest
import torch

import go2_unread_cases as C
import oracle as O
from conftest import seeded_inputs, with_solver
from dial_mpc_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(64, 16), (63, 5), (100, 6), (8, 1)]
LAUNCH = {"relay": dict(relay_always=1), "one-wavefront": dict(no_relay=1)}
LIBS = {"ieee": _lib.IEEE_LIB_PATH, "product": None}
ITERATIONS = (1, 2, 3)
FULL = ("rewss", "rews", "Ybar", "qss", "qdss", "xss", "Y0s", "weights", "qbar", "qdbar", "xbar")
LEAN = ("rews", "Ybar", "weights", "rewss", "Y0s")   # (a lean launch still stores its step rewards and nodes)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda:0")


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _run(ctx, s0, Ybar, sigma, eps, rng, want_bars):
    if rng:
        out = ctx.reverse_once_rng(dev(s0), dev(Ybar), dev(sigma), 1234, 7, want_bars=want_bars)
    else:
        out = ctx.reverse_once(dev(s0), dev(Ybar), dev(sigma), dev(eps), want_bars=want_bars)
    torch.cuda.synchronize()
    ctx.status()
    res = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    res.update(ctx.debug_scratch())
    return res, ctx.debug_last_launch()


def _case(N, H):
    dc, env, model, task, cfg = C.setup(N, H)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=5, Ybar_scale=0.3)
    return model, task, cfg, C.start_states(env, model, O.Oracle(model, task, cfg, np.float32)), (Ybar, sigma, eps)


def _pair(model, task, cfg, lib_path, options, iterations):
    m = with_solver(model, iterations=iterations)
    return (_lib.Context(m, task, cfg, device=0, lib_path=lib_path, options=dict(options)),
            _lib.Context(m, task, cfg, device=0, lib_path=lib_path, options=dict(options, no_defer_reward=1)))


def _assert_launches(ll, ll_ref, launch, T):
    assert ll["defer_reward"] == 1 and ll_ref["defer_reward"] == 0, (ll, ll_ref)
    relay = launch == "relay" and T >= 4   # (dial_hip.hip: a mean trajectory of fewer than four steps is never cut into pieces)
    assert ll["inst"] == 1 and ll["relay"] == ll_ref["relay"] == relay and ll["blocks"] == ll_ref["blocks"]


@pytest.mark.parametrize("build", list(LIBS))
@pytest.mark.parametrize("launch", list(LAUNCH))
@pytest.mark.parametrize("N,H", SHAPES)
def test_equals_the_per_step_kernel(N, H, launch, build):
    """Lean first, then full, on the context under test (the full call after a cut one); full first on the reference."""
    assert LIBS[build] is None or os.path.exists(LIBS[build])
    model, task, cfg, states, (Ybar, sigma, eps) = _case(N, H)
    for iterations in ITERATIONS:
        ctx, ref = _pair(model, task, cfg, LIBS[build], LAUNCH[launch], iterations)
        for sname, s0 in states.items():
            for rng in (False, True):
                lean, ll_lean = _run(ctx, s0, Ybar, sigma, eps, rng, False)
                full, ll_full = _run(ctx, s0, Ybar, sigma, eps, rng, True)
                full_ref, ll_full_ref = _run(ref, s0, Ybar, sigma, eps, rng, True)
                lean_ref, ll_lean_ref = _run(ref, s0, Ybar, sigma, eps, rng, False)
                _assert_launches(ll_lean, ll_lean_ref, launch, H + 1)
                _assert_launches(ll_full, ll_full_ref, launch, H + 1)
                assert np.all(np.isfinite(full_ref["rewss"])) and full_ref["rewss"].std() > 0
                where = (build, launch, N, H, iterations, sname, rng)
                for got, exp, keys, kind in ((full, full_ref, FULL, "full"), (lean, lean_ref, LEAN, "lean")):
                    for k in keys:
                        if not _bits(got[k], exp[k]):
                            d = np.abs(got[k].astype(np.float64) - exp[k].astype(np.float64))
                            print(f"{where} {kind} {k}: max |diff| {d.max():.3g} at {np.unravel_index(d.argmax(), d.shape)}, "
                                  f"{int((d > 0).sum())} of {d.size} entries")
                    for k in keys:
                        assert _bits(got[k], exp[k]), (where, kind, k)


@pytest.mark.parametrize("build", list(LIBS))
@pytest.mark.parametrize("launch", list(LAUNCH))
def test_cut_step_leaves_nothing_behind(launch, build):
    """deferring kernel on both sides: a full call after a lean one equals the first full call of a fresh context"""
    model, task, cfg, states, (Ybar, sigma, eps) = _case(100, 6)
    for sname, s0 in states.items():
        alone = _lib.Context(model, task, cfg, device=0, lib_path=LIBS[build], options=dict(LAUNCH[launch]))
        after = _lib.Context(model, task, cfg, device=0, lib_path=LIBS[build], options=dict(LAUNCH[launch]))
        exp, ll_exp = _run(alone, s0, Ybar, sigma, eps, False, True)
        _, ll_lean = _run(after, s0, Ybar, sigma, eps, False, False)
        got, ll_got = _run(after, s0, Ybar, sigma, eps, False, True)
        assert ll_exp["defer_reward"] == ll_lean["defer_reward"] == ll_got["defer_reward"] == 1
        for k in FULL:
            assert _bits(got[k], exp[k]), (build, launch, sname, k)
