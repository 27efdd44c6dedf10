#!/usr/bin/env python3
"""Reference tables of custom environments: what a table costs a planner step.  ms per reverse_once at Go2 N=2048 H=16, by device
events, for
  (a) the parent commit's library and its go2_height_walk plugin (given with --parent-lib / --parent-plugin: a build of the commit
      before the reference table, made outside this tree),
  (b) this tree, the same env, no table bound,
  (c) go2_track_clip, whose reward reads its row through in.row (the two-row ring in LDS),
  (d) the same reward reading in.table[in.row_index * in.table_cols + j]: a global load on the reward lane, after the physics,
all in ONE process, alternating, --rounds rounds each.  The condition on (b): median(b) <= median(a) + 2 x (max - min of a's
rounds) -- a custom env that binds no table pays nothing beyond the parent's own run-to-run spread.  Writes a markdown report.

usage: bench_user_table.py <out.md> [--parent-lib libdialhip.so --parent-plugin libdialplugin.so] [--iters 200] [--rounds 5]"""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EX = os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env")


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


def _env(name):
    from dial_mpc_amd.core.dial_core import load_dial_and_env, make_cfg
    importlib.import_module("dial_mpc_amd.examples.custom_env." + name)
    d = yaml.safe_load(open(os.path.join(EX, name + ".yaml")))
    d["Nsample"], d["Hsample"] = 2048, 16
    dc, _, env = load_dial_and_env(d)
    return dc, env, make_cfg(dc)


def _isa_notes(path, tag):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "disasm_lib.py"), path, os.path.join(tempfile.gettempdir(), tag),
                           "--notes-only"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout.replace(ROOT + os.sep, "").strip()


def global_read_source(src: str) -> str:
    """The clip reward with every read of its row turned into a read of the whole table in global memory (variant d)."""
    assert "in.row[" in src
    return src.replace("in.row[", "in.table[in.row_index * in.table_cols + ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--parent-lib", default=None, help="libdialhip.so of the parent commit (variant a)")
    ap.add_argument("--parent-plugin", default=None, help="the parent commit's go2_height_walk plugin (variant a)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if (a.parent_lib is None) != (a.parent_plugin is None):
        ap.error("--parent-lib and --parent-plugin go together")
    import torch
    from dial_mpc_amd import _lib, plugin
    dc, walk, cfg = _env("go2_height_walk")
    dcc, clip, cfgc = _env("go2_track_clip")
    table = clip.make_table()
    paths = {"b": walk.plugin_path(), "c": clip.plugin_path(),
             "d": plugin.build_plugin(clip.sys.model, global_read_source(clip.reward_source()))}
    ctxs = {}
    if a.parent_lib:
        ctxs["(a) parent commit, go2_height_walk"] = _lib.Context(walk.make_model(), walk.make_task(), cfg, lib_path=a.parent_lib,
                                                                  plugin=a.parent_plugin, user_params=walk.user_param_vector())
    ctxs["(b) this commit, go2_height_walk, no table"] = _lib.Context(walk.make_model(), walk.make_task(), cfg, **walk.context_kwargs())
    ctxs["(c) go2_track_clip, in.row (LDS ring)"] = _lib.Context(clip.make_model(), clip.make_task(), cfgc, **clip.context_kwargs())
    ctxs["(d) go2_track_clip, in.table (global load)"] = _lib.Context(clip.make_model(), clip.make_task(), cfgc,
                                                                       **dict(clip.context_kwargs(), plugin=paths["d"]))
    res = {k: [] for k in ctxs}
    for _ in range(a.rounds):   # alternating, so that clock / power drift and the neighbours' load hit every variant alike
        for k, ctx in ctxs.items():
            s0, _, _ = ctx.env_reset(torch.as_tensor(walk._init_q, dtype=torch.float32, device="cuda"), torch.zeros(ctx.nv, device="cuda"))
            res[k].append(_ms_per_call(ctx, s0, dc, a.iters))
    lines = ["# Reference tables of custom environments: cost per planner step", "",
             f"reverse_once (lean: mean action only) by device events, Go2 model, N = {dc.Nsample}, H = {dc.Hsample}, Hnode = {dc.Hnode}; "
             f"{a.iters} calls per measurement after 20 warm-up calls, {a.rounds} alternating rounds in one process (median; all rounds "
             f"listed).  The clip's table is [{table.shape[0]}, {table.shape[1]}], wrap mode.", "",
             "| variant | ms per reverse_once (median) | min | max | max - min | rounds |", "|---|---|---|---|---|---|"]
    for k, v in res.items():
        lines.append(f"| {k} | {np.median(v):.4f} | {min(v):.4f} | {max(v):.4f} | {max(v) - min(v):.4f} | {', '.join(f'{x:.4f}' for x in v)} |")
    med = {k[1]: float(np.median(v)) for k, v in res.items()}
    lines.append("")
    if "a" in med:
        va = res[next(k for k in res if k[1] == "a")]
        spread = max(va) - min(va)
        ok = med["b"] <= med["a"] + 2 * spread
        lines += [f"Condition on (b): median(b) = {med['b']:.4f} ms against median(a) + 2 x (max - min of a) = {med['a']:.4f} + 2 x {spread:.4f} = "
                  f"{med['a'] + 2 * spread:.4f} ms: {'MET' if ok else 'NOT MET'} (b - a = {1e3 * (med['b'] - med['a']):+.2f} us, "
                  f"{100 * (med['b'] - med['a']) / med['a']:+.2f} %).", ""]
    else:
        lines += ["Variant (a) was not measured (no --parent-lib / --parent-plugin): the condition on (b) is not evaluated here.", ""]
    d = med["c"] - med["d"]
    lines += [f"Ring against global load: (c) - (d) = {1e3 * d:+.2f} us ({100 * d / med['d']:+.2f} %): "
              + ("the ring is faster than the reward lane's global load." if d < 0 else
                 "the ring is NOT faster than the reward lane's global load at this size; it stays for the control law's sake, which reads "
                 "its row at the top of the step, where nothing hides a load."), ""]
    for key, tag in (("b", "no table"), ("c", "in.row"), ("d", "in.table")):
        lines += [f"Kernels of plugin ({key}), {tag} (tools/isa/disasm_lib.py --notes-only):", "", "```", _isa_notes(paths[key], "isa_table_" + key), "```", ""]
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
