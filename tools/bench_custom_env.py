#!/usr/bin/env python3
"""Custom environments: ms per reverse_once at Go2 N=2048 H=16 for (a) the example task plugin (go2_height_walk), (b) the Go2 walk
task forced onto the capacity-dimension kernel (DimsMax, dial_options.force_generic), (c) the shipped DimsGo2 kernel; the plugin's
cold compile time (empty cache) and its kernels' resource line (tools/isa/disasm_lib.py).  Writes a markdown report.

usage: bench_custom_env.py <out.md> [--iters 200] [--rounds 3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    from dial_mpc_amd import _lib, plugin
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    importlib.import_module("dial_mpc_amd.examples.custom_env.go2_height_walk")
    d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk.yaml")))
    d["Nsample"], d["Hsample"] = 2048, 16
    dc, _, env = load_dial_and_env(d)
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
