#!/usr/bin/env python3
"""Custom environments: ms per reverse_once at Go2 N=2048 H=16 for (a) the example task plugin (go2_height_walk), (b) the Go2 walk
task forced onto the capacity-dimension kernel (DimsMax, dial_options.force_generic), (c) the shipped DimsGo2 kernel; the plugin's
cold compile time (empty cache) and its kernels' resource line (tools/isa/disasm_lib.py).  Writes a markdown report.
--plan-params: instead, grouped reverse_once_batch_rng of the example plugin at M plans (--plans, default 4 and 32), the shared task
parameters against bound per-plan rows (dial_set_plan_params), alternating.
--control-law: instead, reverse_once of the example reward's plugin WITHOUT a control law against the same plugin WITH BaseEnv's
torque law restated as a user law (examples/custom_env/base_pd_law.hip), alternating; the difference next to the spread of the
no-law plugin's own rounds, and both plugins' kernel resource lines.

usage: bench_custom_env.py <out.md> [--iters 200] [--rounds 3] [--plan-params [--plans 4 32]] [--control-law]"""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ms_per_call(ctx, s0, dc, iters):
    import torch
    rng = np.random.default_rng(0)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device="cuda")   # noqa: E731
    eps = dev(rng.standard_normal((dc.Nsample, dc.Hnode + 1, ctx.nu)))
    Ybar = dev(np.zeros((dc.Hnode + 1, ctx.nu)))
    sig = dev(np.full(dc.Hnode + 1, 0.3))
    for _ in range(20):
        ctx.reverse_once(s0, Ybar, sig, eps, want_bars=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ctx.reverse_once(s0, Ybar, sig, eps, want_bars=False)
    e1.record()
    torch.cuda.synchronize()
    ctx.status()
    return e0.elapsed_time(e1) / iters


def _ms_per_batch(ctx, states, dc, iters, rows):
    """ms per grouped reverse_once_batch_rng (lean) of len(states) plans; rows: per-plan parameters bound for the calls, or None."""
    import torch
    M = int(states.shape[0])
    Ybar = torch.zeros((M, dc.Hnode + 1, ctx.nu), device="cuda")
    sig = torch.full((M, dc.Hnode + 1), 0.3, device="cuda")
    ctx.set_plan_params(rows)
    for _ in range(10):
        ctx.reverse_once_batch_rng(states, Ybar, sig, 0, 0, want_bars=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        ctx.reverse_once_batch_rng(states, Ybar, sig, 0, i, want_bars=False)
    e1.record()
    torch.cuda.synchronize()
    ctx.set_plan_params(None)
    ctx.status()
    return e0.elapsed_time(e1) / iters


def plan_params_report(a, env, dc, cfg):
    import torch
    from dial_mpc_amd import _lib
    lines = ["# Per-plan task parameters: grouped plans of the example plugin, shared against bound rows", "",
             f"reverse_once_batch_rng (lean: mean actions only), go2_height_walk plugin, N = {dc.Nsample}, H = {dc.Hsample}, "
             f"Hnode = {dc.Hnode}; {a.iters} calls per measurement, {a.rounds} alternating rounds (median; all rounds listed).  "
             "`shared`: every plan reads the context's one parameter vector; `rows`: dial_set_plan_params binds M rows (per-plan vx and "
             "height), plan g's reward reads row g.", "",
             "| M | parameters | ms per call (median) | ms per plan | rounds |", "|---|---|---|---|---|"]
    for M in a.plans:
        ctx = _lib.Context(env.make_model(), env.make_task(), cfg, options=dict(plan_cap=M), **env.context_kwargs())
        q = torch.as_tensor(np.tile(env._init_q, (M, 1)), dtype=torch.float32, device="cuda")
        states = ctx.env_reset_batch(q, torch.zeros((M, ctx.nv), device="cuda"))
        rows = env.plan_params(vx=list(np.linspace(0.2, 1.2, M)), height=list(np.linspace(0.25, 0.35, M)))
        res = {"shared": [], "rows": []}
        for _ in range(a.rounds):   # alternating
            res["shared"].append(_ms_per_batch(ctx, states, dc, a.iters, None))
            res["rows"].append(_ms_per_batch(ctx, states, dc, a.iters, rows))
        for k, v in res.items():
            lines.append(f"| {M} | {k} | {np.median(v):.3f} | {np.median(v) / M:.4f} | {', '.join(f'{x:.3f}' for x in v)} |")
        del ctx
    isa = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "disasm_lib.py"), env.plugin_path(),
                          os.path.join(tempfile.gettempdir(), "isa_plugin"), "--notes-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True).stdout.replace(ROOT + os.sep, "")   # (the plugin's path relative to the repository)
    lines += ["", "Plugin kernels (tools/isa/disasm_lib.py --notes-only):", "", "```", isa.strip(), "```"]
    return lines


def _isa_notes(path, tag):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "disasm_lib.py"), path, os.path.join(tempfile.gettempdir(), tag),
                           "--notes-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout.replace(ROOT + os.sep, "").strip()


def control_law_report(a, env, dc, cfg):
    import torch
    from dial_mpc_amd import _lib, plugin
    law = os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "base_pd_law.hip")
    paths = {"no law (built-in control)": env.plugin_path(),
             "restated PD law (base_pd_law.hip)": plugin.build_plugin(env.sys.model, env.reward_source(), control_src=law)}
    ctxs = {k: _lib.Context(env.make_model(), env.make_task(), cfg, plugin=p, user_params=env.user_param_vector()) for k, p in paths.items()}
    res = {k: [] for k in ctxs}
    for _ in range(a.rounds):   # alternating, so that clock / power drift hits both alike
        for k, ctx in ctxs.items():
            s0, _, _ = ctx.env_reset(torch.as_tensor(env._init_q, dtype=torch.float32, device="cuda"), torch.zeros(ctx.nv, device="cuda"))
            res[k].append(_ms_per_call(ctx, s0, dc, a.iters))
    base, with_law = (np.asarray(v) for v in res.values())
    lines = ["# User control laws: the plugin with a restated PD law against the plugin without a law", "",
             f"reverse_once (lean: mean action only), go2_height_walk reward, Go2 model, N = {dc.Nsample}, H = {dc.Hsample}, Hnode = {dc.Hnode}; "
             f"{a.iters} calls per measurement, {a.rounds} alternating rounds (median; all rounds listed).  The baseline is the no-law plugin "
             "of the same run.", "",
             "| plugin | ms per reverse_once (median) | min | max | rounds |", "|---|---|---|---|---|"]
    for k, v in res.items():
        lines.append(f"| {k} | {np.median(v):.4f} | {min(v):.4f} | {max(v):.4f} | {', '.join(f'{x:.4f}' for x in v)} |")
    diff, spread = float(np.median(with_law) - np.median(base)), float(base.max() - base.min())
    lines += ["", f"Difference of the medians (law - no law): {diff * 1e3:+.2f} us ({100 * diff / np.median(base):+.2f} %); spread (max - min) of "
              f"the no-law plugin's own rounds: {spread * 1e3:.2f} us; per-round differences: "
              f"{', '.join(f'{1e3 * (x - y):+.2f}' for x, y in zip(with_law, base))} us.", ""]
    for k, p in paths.items():
        lines += [f"Kernels of the plugin, {k} (tools/isa/disasm_lib.py --notes-only):", "", "```", _isa_notes(p, "isa_" + ("law" if "restated" in k else "nolaw")), "```", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plan-params", action="store_true", help="measure shared against per-plan task parameters instead")
    ap.add_argument("--plans", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--control-law", action="store_true", help="measure the plugin without a control law against one with the restated PD law instead")
    a = ap.parse_args()
    import torch
    from dial_mpc_amd import _lib, plugin
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    importlib.import_module("dial_mpc_amd.examples.custom_env.go2_height_walk")
    d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk.yaml")))
    d["Nsample"], d["Hsample"] = 2048, 16
    dc, _, env = load_dial_and_env(d)
    if a.plan_params or a.control_law:
        lines = (plan_params_report if a.plan_params else control_law_report)(a, env, dc, make_cfg(dc))
        open(a.out, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    t = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "unitree_go2_trot.yaml")))
    t["Nsample"], t["Hsample"] = 2048, 16
    dct, _, go2 = load_dial_and_env(t)
    cfg = make_cfg(dc)
    with tempfile.TemporaryDirectory() as tmp:   # cold compile: an empty cache
        os.environ["DIAL_PLUGIN_CACHE"] = tmp
        t0 = time.time()
        plugin.build_plugin(env.sys.model, env.reward_source())
        cold_s = time.time() - t0
        t0 = time.time()
        plugin.build_plugin(env.sys.model, env.reward_source())
        warm_s = time.time() - t0
        del os.environ["DIAL_PLUGIN_CACHE"]
    path = env.plugin_path()
    isa = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "disasm_lib.py"), path, os.path.join(tempfile.gettempdir(), "isa_plugin"),
                          "--notes-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    ctxs = {
        "(a) plugin, example reward (DimsUser)": _lib.Context(env.make_model(), env.make_task(), cfg, **env.context_kwargs()),
        "(b) Go2 walk on DimsMax (force_generic)": _lib.Context(go2.make_model(), go2.make_task(), make_cfg(dct), options=dict(force_generic=1)),
        "(c) Go2 walk on DimsGo2 (shipped)": _lib.Context(go2.make_model(), go2.make_task(), make_cfg(dct)),
    }
    res = {k: [] for k in ctxs}
    for _ in range(a.rounds):   # alternating, so that clock / power drift hits all three alike
        for k, ctx in ctxs.items():
            s0, _, _ = ctx.env_reset(torch.as_tensor(env._init_q, dtype=torch.float32, device="cuda"), torch.zeros(ctx.nv, device="cuda"))
            res[k].append(_ms_per_call(ctx, s0, dc, a.iters))
    lines = ["# Custom environments: task-plugin timing", "",
             f"reverse_once (lean: mean action only), Go2 model, N = {dc.Nsample}, H = {dc.Hsample}, Hnode = {dc.Hnode}; "
             f"{a.iters} calls per measurement, {a.rounds} alternating rounds (median; all rounds listed).", "",
             "| setup | ms per reverse_once (median) | rounds |", "|---|---|---|"]
    for k, v in res.items():
        lines.append(f"| {k} | {np.median(v):.3f} | {', '.join(f'{x:.3f}' for x in v)} |")
    lines += ["", f"Plugin compile, cold (empty cache, one translation unit + link): {cold_s:.1f} s; cached lookup: {warm_s * 1e3:.0f} ms "
              f"(host: {os.cpu_count()} CPUs).", "", "Plugin kernels (tools/isa/disasm_lib.py --notes-only):", "", "```", isa.strip(), "```", ""]
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
