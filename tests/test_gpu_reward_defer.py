"""Deferred step rewards of the Go2 walk on the device (csrc/reward_defer_kernel.h; dial_options.no_defer_reward).

The default context launches the kernel that evaluates the step rewards once per rollout, control step t in lane t; a context
with no_defer_reward = 1 launches the kernel with the reward lane in every step (what every launch ran before).  Every test
asserts through debug_last_launch which of the two ran -- a silently disabled path would pass every comparison.

On libdialhip_ieee.so (no contraction) everything a reverse_once emits is bit-identical between the two: the same term code on
the same input bits and the same ordered fp64 sum.  On the product library the same equality is asserted: the physics does not see
the reward, and both kernels inline the one reward phase of env_step."""
import os

import numpy as np
import pytest
import torch

import oracle as O
from conftest import perturbed_state, seeded_inputs, setup_case
from dial_mpc_amd import _lib

pytestmark = pytest.mark.gpu

EX = "unitree_go2_trot"
SHAPES = [(64, 16), (63, 5), (100, 7)]
LAUNCH = {"relay": dict(relay_always=1), "one-wavefront": dict(no_relay=1)}
LIBS = {"ieee": _lib.IEEE_LIB_PATH, "product": None}
SCRATCH = ("Y0s", "rewss", "qss", "qdss", "xss", "weights")
OUT = ("Ybar", "rews", "qbar", "qdbar", "xbar")


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda:0")


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _states(env, model, o32):
    """the rest pose and a perturbed state (feet in and out of contact)"""
    rest, _, _ = o32.env_reset(env._init_q, np.zeros(model.nv))
    q, qd = perturbed_state(env, 1)
    pert, _, _ = o32.env_reset(q, qd)
    return dict(rest=rest, perturbed=pert)


def _run(ctx, s0, Ybar, sigma, eps, rng, want_bars=True):
    """one reverse_once (noise as data, or drawn in the kernel) -> everything it emits, as host arrays"""
    if rng:
        out = ctx.reverse_once_rng(dev(s0), dev(Ybar), dev(sigma), 1234, 7, want_bars=want_bars)
    else:
        out = ctx.reverse_once(dev(s0), dev(Ybar), dev(sigma), dev(eps), want_bars=want_bars)
    torch.cuda.synchronize()
    ctx.status()
    res = {k: out[k].cpu().numpy() for k in OUT if out[k] is not None}
    res.update(ctx.debug_scratch())
    return res, ctx.debug_last_launch()


def _pair(example, N, H, lib_path, options):
    """(default context, no_defer_reward context, inputs)"""
    dc, env, model, task, cfg = setup_case(example, N, H)
    o32 = O.Oracle(model, task, cfg, np.float32)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=5, Ybar_scale=0.3)
    a = _lib.Context(model, task, cfg, device=0, lib_path=lib_path, options=dict(options))
    b = _lib.Context(model, task, cfg, device=0, lib_path=lib_path, options=dict(options, no_defer_reward=1))
    return a, b, _states(env, model, o32), (Ybar, sigma, eps), model


@pytest.mark.parametrize("build", list(LIBS))
@pytest.mark.parametrize("launch", list(LAUNCH))
@pytest.mark.parametrize("N,H", SHAPES)
def test_deferred_equals_per_step(N, H, launch, build):
    assert LIBS[build] is None or os.path.exists(LIBS[build])
    ctx, ref, states, (Ybar, sigma, eps), _ = _pair(EX, N, H, LIBS[build], LAUNCH[launch])
    for sname, s0 in states.items():
        for rng in (False, True):
            got, ll = _run(ctx, s0, Ybar, sigma, eps, rng)
            exp, ll_ref = _run(ref, s0, Ybar, sigma, eps, rng)
            assert ll["defer_reward"] == 1 and ll_ref["defer_reward"] == 0, (ll, ll_ref)
            assert ll["inst"] == 1 and ll["relay"] == ll_ref["relay"] == (launch == "relay") and ll["blocks"] == ll_ref["blocks"]
            assert np.all(np.isfinite(exp["rewss"])) and exp["rewss"].std() > 0
            for k in SCRATCH + OUT:
                if not _bits(got[k], exp[k]):
                    d = np.abs(got[k].astype(np.float64) - exp[k].astype(np.float64))
                    print(f"{build} {launch} N={N} H={H} {sname} rng={rng} {k}: max |diff| {d.max():.3g} at {np.unravel_index(d.argmax(), d.shape)}, "
                          f"{int((d > 0).sum())} of {d.size} entries, largest in ulp of the per-step value "
                          f"{float((d / np.spacing(np.abs(exp[k]).astype(np.float32)).astype(np.float64)).max()):.3g}")
            for k in SCRATCH + OUT:
                assert _bits(got[k], exp[k]), (build, launch, sname, rng, k)


@pytest.mark.parametrize("build", list(LIBS))
def test_lean_iteration_equals_full(build):
    """without bars (the rollouts store no per-step states) the deferred kernel emits the same Ybar and mean rewards"""
    ctx, _, states, (Ybar, sigma, eps), _ = _pair(EX, 64, 16, LIBS[build], LAUNCH["relay"])
    for s0 in states.values():
        full, ll = _run(ctx, s0, Ybar, sigma, eps, False)
        lean, ll_lean = _run(ctx, s0, Ybar, sigma, eps, False, want_bars=False)
        assert ll["defer_reward"] == 1 and ll_lean["defer_reward"] == 1
        assert _bits(lean["Ybar"], full["Ybar"]) and _bits(lean["rews"], full["rews"])


@pytest.mark.parametrize("build", list(LIBS))
def test_given_controls_defer_too(build):
    """dial_rollout (controls given, no nodes): deferred as well, same step rewards and states"""
    ctx, ref, states, _, model = _pair(EX, 64, 16, LIBS[build], {})
    us = np.random.default_rng(2).uniform(-1, 1, (37, 17, model.nu)).astype(np.float32)
    for s0 in states.values():
        got = [t.cpu().numpy() for t in ctx.rollout(dev(s0), dev(us))]
        ll = ctx.debug_last_launch()
        exp = [t.cpu().numpy() for t in ref.rollout(dev(s0), dev(us))]
        assert ll["defer_reward"] == 1 and ll["blocks"] == 37 and ref.debug_last_launch()["defer_reward"] == 0
        for a, b, k in zip(got, exp, ("rewss", "qss", "qdss", "xss")):
            assert _bits(a, b), k


@pytest.mark.parametrize("example,N,H", [(EX, 64, 18), ("unitree_go2_seq_jump", 48, 16)], ids=["T19-stash-too-large", "seq-jump"])
def test_launches_that_must_not_defer(example, N, H):
    """T = 19: the stash (1 824 B) no longer fits nine workgroups per CU; seq-jump: another task kind.  Both run the per-step kernel."""
    for launch in LAUNCH.values():
        ctx, ref, states, (Ybar, sigma, eps), _ = _pair(example, N, H, None, launch)
        for s0 in states.values():
            got, ll = _run(ctx, s0, Ybar, sigma, eps, False)
            exp, ll_ref = _run(ref, s0, Ybar, sigma, eps, False)
            assert ll["defer_reward"] == 0 and ll == ll_ref and ll["inst"] == 1
            for k in SCRATCH + OUT:
                assert _bits(got[k], exp[k]), k


def test_relay_pieces_equal_one_wavefront_three_launches():
    """Deferred on both sides, product build: the mean trajectory as relay pieces (every piece evaluates its own steps and hands
    the running sum on; the turn flag re-arms) equals the mean trajectory as one wavefront, launch after launch."""
    dc, env, model, task, cfg = setup_case(EX, 64, 16)
    o32 = O.Oracle(model, task, cfg, np.float32)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=5, Ybar_scale=0.3)
    relay = _lib.Context(model, task, cfg, device=0, options=LAUNCH["relay"])
    one = _lib.Context(model, task, cfg, device=0, options=LAUNCH["one-wavefront"])
    s0 = _states(env, model, o32)["perturbed"]
    for it in range(3):
        got, ll = _run(relay, s0, Ybar, sigma, eps, False)
        exp, ll_one = _run(one, s0, Ybar, sigma, eps, False)
        assert ll["defer_reward"] == 1 and ll["relay"] == 1 and ll_one["defer_reward"] == 1 and ll_one["relay"] == 0
        for k in SCRATCH + OUT:
            assert _bits(got[k], exp[k]), (it, k)
        Ybar = got["Ybar"]   # (the next launch plans from this one's result)
