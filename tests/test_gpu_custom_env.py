"""Custom environments on the GPU: a task plugin (user reward compiled for one model, dial_create_plugin) against the fp32 oracle,
a numpy restatement of the example reward, the built-in instantiations and the closed-loop driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import LS_SWAP, TOL, _within, seeded_inputs, with_solver

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX_DIR = os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env")
EX_MOD = "dial_mpc_amd.examples.custom_env.go2_height_walk"
EX_YAML = os.path.join(EX_DIR, "go2_height_walk.yaml")


@pytest.fixture(scope="module", autouse=True)
def _registry():
    """The example registers itself in the env registry; this module's tests leave the registry as they found it."""
    import importlib
    import dial_mpc_amd.envs as dial_envs
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    mod = sys.modules.get(EX_MOD)
    if mod is None:
        importlib.import_module(EX_MOD)
    else:
        importlib.reload(mod)   # (registered again: an earlier module's teardown removed it)
    yield
    dial_envs._envs.clear()
    dial_envs._envs.update(saved[0])
    dial_envs._configs.clear()
    dial_envs._configs.update(saved[1])


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")


def _case(N=64, H=16):
    import importlib
    importlib.import_module(EX_MOD)
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    d = yaml.safe_load(open(EX_YAML))
    d["Nsample"], d["Hsample"] = N, H
    dc, ec, env = load_dial_and_env(d)
    return dc, env, make_cfg(dc)


@pytest.fixture(scope="module")
def ex():
    dc, env, cfg = _case()
    return dict(dc=dc, env=env, cfg=cfg, plugin=env.plugin_path(), params=env.user_param_vector())


def _go2_walk_task():
    from dial_mpc_amd.envs.unitree_go2_env import UnitreeGo2Env, UnitreeGo2EnvConfig
    return UnitreeGo2Env(UnitreeGo2EnvConfig()).make_task()


def _physics_gate(got, ref, B, T, max_diverged):
    """Per-rollout gate of the rollout parity tests (conftest.TOL on q / qd / x at every step): every rollout within it, up to
    `max_diverged` knife-edge rollouts (the witness search of test_gpu_parity compares rewards too, which differ here by design)."""
    ok = np.ones((B, T), bool)
    for name, g, r in zip(("q", "qd", "x"), got, ref):
        w = _within(g, r, TOL[name])
        ok &= w if w.ndim == 2 else w.reshape(B, T, -1).all(-1)
    bad = np.flatnonzero(~ok.all(1))
    assert ok[:, 0].all(), "first step differs"
    assert len(bad) <= max_diverged, f"rollouts outside the gate: {bad.tolist()}"
    return len(bad)


def _mirror_reward(p, qvel, xpos_trunk, xquat_trunk, ctrl):
    """numpy (fp64) restatement of go2_height_walk.hip."""
    w, x, y, z = [float(v) for v in xquat_trunk]
    zx, zy, zz = 2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)
    return (-p[2] * (qvel[0] - p[0]) ** 2 - p[3] * (xpos_trunk[2] - p[1]) ** 2 - p[4] * (zx * zx + zy * zy + (zz - 1) ** 2)
            - p[5] * float(np.sum(np.asarray(ctrl, np.float64) ** 2)))


def test_plugin_physics_matches_oracle(ex):
    """1. Go2 + the example reward (DIAL_LS_SWAP): each rollout's q / qd / x equal the fp32 oracle's (built-in walk task: physics
    does not depend on the reward)."""
    import oracle as O
    from dial_mpc_amd import _lib
    env, cfg = ex["env"], ex["cfg"]
    model = with_solver(env.make_model(), ls_rule=LS_SWAP)
    ctx = _lib.Context(model, env.make_task(), cfg, plugin=ex["plugin"], user_params=ex["params"])
    o32 = O.Oracle(model, _go2_walk_task(), cfg, np.float32)
    s0, _, _ = o32.env_reset(env._init_q, np.zeros(model.nv))
    us = np.random.default_rng(4).uniform(-0.8, 0.8, (16, cfg.Hsample + 1, model.nu)).astype(np.float32)
    got = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
    ref = o32.rollout(s0, us)
    _physics_gate(got[1:], ref[1:], 16, cfg.Hsample + 1, max_diverged=1)


def _go2_fewer_contacts(model_dict, drop=3):
    """The Go2 without the contact candidate of one foot: 3 contacts, 24 constraint rows -- dimensions no built-in kernel has."""
    m = dict(model_dict)
    n = int(m["ncon"])
    keep = [c for c in range(n) if c != drop]
    for k in list(m):
        if k.startswith("con_") and np.asarray(m[k]).shape[:1] == (n,):
            m[k] = np.asarray(m[k])[keep]
    m["ncon"] = n - 1
    m["nefc"] = int(m["nefc"]) - 4
    return m


def test_plugin_on_a_model_no_instantiation_matches(ex):
    """2. A derived model (Go2 with three contact candidates): plugin == oracle, and == the capacity-dimension kernel's run."""
    import oracle as O
    from dial_mpc_amd import _abi, _lib
    from dial_mpc_amd.plugin import build_plugin
    env, cfg = ex["env"], ex["cfg"]
    md = _go2_fewer_contacts(env.sys.model)
    model = with_solver(_abi.make_model(md), ls_rule=LS_SWAP)
    path = build_plugin(md, env.reward_source())
    ctx = _lib.Context(model, env.make_task(), cfg, plugin=path, user_params=ex["params"])
    o32 = O.Oracle(model, _go2_walk_task(), cfg, np.float32)
    s0, _, _ = o32.env_reset(env._init_q, np.zeros(model.nv))
    us = np.random.default_rng(5).uniform(-0.8, 0.8, (16, cfg.Hsample + 1, model.nu)).astype(np.float32)
    got = [t.cpu().numpy() for t in ctx.rollout(_dev(s0), _dev(us))]
    _physics_gate(got[1:], o32.rollout(s0, us)[1:], 16, cfg.Hsample + 1, max_diverged=1)
    gen = _lib.Context(model, _go2_walk_task(), cfg)   # (falls through to DimsMax: no built-in instantiation has 3 contacts)
    ref = [t.cpu().numpy() for t in gen.rollout(_dev(s0), _dev(us))]
    _physics_gate(got[1:], ref[1:], 16, cfg.Hsample + 1, max_diverged=1)


def _env_steps(ex, n_steps=12, ctx=None):
    """n env.steps of the example from its keyframe with fixed actions: per step (reward, info, qvel, xpos, xquat, ctrl)."""
    import torch
    from dial_mpc_amd import _lib
    env = ex["env"]
    if ctx is None:
        ctx = _lib.Context(env.make_model(), env.make_task(), None, plugin=ex["plugin"], user_params=ex["params"])
    M = _lib._abi.MACROS
    nq, nv, nb = ctx.nq, ctx.nv, ctx.nbody
    state, _, _ = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(nv)))
    acts = np.random.default_rng(7).uniform(-0.5, 0.5, (n_steps, ctx.nu)).astype(np.float32)
    out = []
    for t in range(n_steps):
        state, xpos, xquat, ctrl = ctx.env_step(state, _dev(acts[t]))
        torch.cuda.synchronize()
        s = state.cpu().numpy()
        info = s[nq + 2 * nv:]
        out.append(dict(rew=float(info[M["DIAL_INFO_REWARD"]]), info=info.copy(), qvel=s[nq:nq + nv].copy(),
                        xpos=xpos.cpu().numpy().reshape(nb - 1, 3), xquat=xquat.cpu().numpy().reshape(nb - 1, 4),
                        ctrl=ctrl.cpu().numpy()))
    return out


def test_rewards_match_numpy_mirror(ex):
    """3. The device's per-step rewards equal go2_height_walk.hip restated in numpy on the device's own returned states.
    Tolerance: the reward is a handful of fp32 products / sums of O(1..100) terms; 1e-4 relative + 1e-5 absolute covers the
    fp32 rounding of ~20 operations (each <= 2^-24 relative) with a wide margin -- the measured difference is printed."""
    M = __import__("dial_mpc_amd._abi", fromlist=["MACROS"]).MACROS
    p = ex["params"]
    worst = 0.0
    for t, st in enumerate(_env_steps(ex)):
        # xpos / xquat from env.step are the PRE-integration forward quantities, qvel is post-integration (user_reward.h)
        want = _mirror_reward(p, st["qvel"], st["xpos"][0], st["xquat"][0], st["ctrl"])
        worst = max(worst, abs(st["rew"] - want))
        assert abs(st["rew"] - want) <= 1e-4 * abs(want) + 1e-5, (t, st["rew"], want)
        u = M["DIAL_INFO_USER"]
        assert st["info"][u] == np.float32(st["qvel"][0]) and st["info"][u + 1] == t + 1   # info_user persists across env.step
        assert st["info"][M["DIAL_INFO_STEP"]] == t + 1
    print(f"max |reward - numpy mirror| = {worst:.3g}")


def test_set_user_params_changes_rewards(ex):
    """6. dial_set_user_params: new parameters, same plugin, rewards as the mirror predicts."""
    from dial_mpc_amd import _lib
    env = ex["env"]
    p2 = list(ex["params"])
    p2[0], p2[1], p2[3] = 0.0, 0.4, 3.0
    ctx = _lib.Context(env.make_model(), env.make_task(), None, plugin=ex["plugin"], user_params=ex["params"])
    ctx.set_user_params(p2)
    moved = 0
    for st in _env_steps(ex, n_steps=4, ctx=ctx):
        args = (st["qvel"], st["xpos"][0], st["xquat"][0], st["ctrl"])
        want, old = _mirror_reward(p2, *args), _mirror_reward(ex["params"], *args)
        assert abs(st["rew"] - want) <= 1e-4 * abs(want) + 1e-5, (st["rew"], want, old)
        moved += abs(want - old) > 1e-3
    assert moved == 4


def test_reverse_once_on_plugin_context(ex):
    """4. reverse_once: Ybar and the weights against an fp64 host softmax of the device's own rewards; 5. M = 4 grouped plans
    bit-identical to four single plans."""
    import torch
    from dial_mpc_amd import _lib
    env, cfg, dc = ex["env"], ex["cfg"], ex["dc"]
    ctx = _lib.Context(env.make_model(), env.make_task(), cfg, plugin=ex["plugin"], user_params=ex["params"], options=dict(plan_cap=4))
    s0, _, _ = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(ctx.nv)))
    singles = []
    ins = [seeded_inputs(dc, ctx.nu, seed=k, Ybar_scale=0.2) for k in range(4)]
    for eps, sigma, Ybar in ins:
        out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
        torch.cuda.synchronize()
        singles.append({k: out[k].cpu().numpy().copy() for k in ("Ybar", "rews")})
    sc = ctx.debug_scratch()
    r = sc["rewss"].astype(np.float64).mean(1) if "rewss" in sc else None
    rews = singles[-1]["rews"].astype(np.float64)
    if r is not None:
        assert np.allclose(r, rews, rtol=1e-5, atol=1e-6)
    logp = (rews - rews[-1]) / rews.std() / cfg.temp_sample
    w = np.exp(logp - logp.max())
    w /= w.sum()
    assert np.allclose(sc["weights"][: len(w)], w, rtol=1e-3, atol=1e-6)
    Y0s = sc["Y0s"].astype(np.float64)[: len(w)]
    Ybar = np.einsum("n,nij->ij", w, Y0s)
    assert np.allclose(singles[-1]["Ybar"], Ybar, rtol=1e-4, atol=1e-5)
    S = torch.stack([s0] * 4).contiguous()
    Yb = _dev(np.stack([i[2] for i in ins]))
    sg = _dev(np.stack([i[1] for i in ins]))
    ep = _dev(np.stack([i[0] for i in ins]))
    outb = ctx.reverse_once_batch(S, Yb, sg, ep)
    torch.cuda.synchronize()
    for g in range(4):
        assert np.array_equal(outb["Ybar"][g].cpu().numpy(), singles[g]["Ybar"])
        assert np.array_equal(outb["rews"][g].cpu().numpy(), singles[g]["rews"])


def test_shipped_context_unaffected_by_plugin(ex):
    """7. A shipped Go2 context gives the same results, bit for bit, before and after a plugin context exists in the process."""
    import torch
    from conftest import setup_case
    from dial_mpc_amd import _lib

    dc, env, model, task, cfg = setup_case("unitree_go2_trot", 64, 16)
    eps, sigma, Ybar = seeded_inputs(dc, model.nu, seed=1, Ybar_scale=0.2)

    def plan():
        ctx = _lib.Context(model, task, cfg)
        s0, _, _ = ctx.env_reset(_dev(env._init_q), _dev(np.zeros(model.nv)))
        out = ctx.reverse_once(s0, _dev(Ybar), _dev(sigma), _dev(eps))
        torch.cuda.synchronize()
        return out["Ybar"].cpu().numpy(), out["rews"].cpu().numpy()
    before = plan()
    pe = ex["env"]
    pctx = _lib.Context(pe.make_model(), pe.make_task(), ex["cfg"], plugin=ex["plugin"], user_params=ex["params"])
    s1, _, _ = pctx.env_reset(_dev(pe._init_q), _dev(np.zeros(pctx.nv)))
    pctx.reverse_once(s1, _dev(np.zeros((ex["cfg"].Hnode + 1, pctx.nu))), _dev(np.full(ex["cfg"].Hnode + 1, 0.1)),
                      _dev(np.random.default_rng(0).standard_normal((ex["cfg"].Nsample, ex["cfg"].Hnode + 1, pctx.nu))))
    torch.cuda.synchronize()
    after = plan()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_closed_loop_driver(ex, tmp_path):
    """8. dial-mpc --custom-env <example> --config <example yaml> --n-steps 5 as a fresh child process."""
    cfg = yaml.safe_load(open(EX_YAML))
    cfg["output_dir"] = str(tmp_path / "out")
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "dial_mpc_amd.core.dial_core", "--custom-env", EX_MOD, "--config", str(p), "--n-steps", "5"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "mean reward" in r.stdout and "nan" not in r.stdout.split("mean reward")[1].split("\n")[0].lower(), r.stdout[-2000:]
    files = [f for f in os.listdir(tmp_path / "out")]
    assert any("states" in f for f in files), files
