"""What the update rules cost and how the closed loops fare under them; writes profiles/update_rule.md.

  timing       reverse_once (M = 1) / reverse_once_batch of the Go2 trot example, in-kernel noise, with bars, at N = 2048, H = 16 with
               M = 1, 4 and 32 plans and at N = 65536 on one GPU, under "mppi", "cem" (elite_frac 0.1) and "ps" -- one context per
               rule in ONE process, interleaved call by call.  --parent-lib names a libdialhip.so built from the parent commit (its
               sibling libraries next to it): a fourth context runs it under mppi in the same interleaving, so that the unchanged path
               is compared with the parent on the same box in the same session.  Device events around each call; the median over
               --iters calls per variant, and the spread of the medians of --rounds repetitions.
  kernels      --kernel-csv names the kernel trace of a `rocprofv3 --kernel-trace --output-format csv -- python
               tools/bench_update_rule.py --trace-run` run (no counters): per shape TRACE_CALLS calls under each rule in a fixed
               order, from which the durations of weights_kernel and elite_weights_kernel are read shape by shape.
  closed loop  Go2 trot and H1 jog, --ticks control steps of dial_core's synchronous loop at the example's sizes under each rule:
               mean reward, lowest trunk height, plan latency p50.  A record; nothing is gated.

Usage: python tools/bench_update_rule.py [--parent-lib PATH] [--parent-label REV] [--kernel-csv CSV] [--iters 30] [--rounds 5]
                                         [--ticks 150] [--session TEXT] [--out profiles/update_rule.md]
       python tools/bench_update_rule.py --trace-run        (under rocprofv3 --kernel-trace)
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2048, 1), (2048, 4), (2048, 32), (65536, 1))   # (Nsample, plans)
RULES = ("mppi", "cem", "ps")
ELITE_FRAC = 0.1
TRACE_CALLS, TRACE_SKIP = 40, 10


def _load(example, **over):
    import yaml
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    d.update(over)
    return load_dial_and_env(d)


def _contexts(N, M, variants, parent_lib):
    """{variant: (ctx, inputs, out)} for the Go2 trot at Nsample = N, H = 16, M plans; "parent" runs parent_lib under mppi."""
    import torch
    from dial_mpc_amd import _lib
    from dial_mpc_amd.core.dial_core import make_cfg
    dc, ec, env = _load("unitree_go2_trot", Nsample=N, Hsample=16)
    model, task, cfg = env.make_model(), env.make_task(), make_cfg(dc)
    Hn1 = dc.Hnode + 1
    made = {}
    for name in variants:
        ctx = _lib.Context(model, task, cfg, device=0, options=dict(plan_cap=M), lib_path=parent_lib if name == "parent" else None)
        if name in ("cem", "ps"):
            ctx.set_update_rule("elite", _lib.elite_count(name, N, ELITE_FRAC, 0))
        dev = ctx.torch_device
        q0 = np.tile(np.asarray(env._init_q, np.float32), (M, 1))
        ins = (ctx.env_reset_batch(torch.as_tensor(q0, device=dev), torch.zeros((M, ctx.nv), dtype=torch.float32, device=dev)),
               torch.zeros((M, Hn1, ctx.nu), dtype=torch.float32, device=dev), torch.full((M, Hn1), 0.5, dtype=torch.float32, device=dev))
        made[name] = (ctx, ins, ctx._out_batch(M, True))
    return made


def _call(entry, counter):
    ctx, ins, out = entry
    ctx.reverse_once_batch_rng(*ins, 1234, counter, out=out, want_bars=True)   # (M = 1 runs exactly reverse_once_rng)


def bench_timing(iters, rounds, parent_lib):
    import torch
    variants = (("parent",) if parent_lib else ()) + RULES
    rows = []
    for N, M in SHAPES:
        made = _contexts(N, M, variants, parent_lib)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        count = [0]

        def call(name):
            count[0] += 1
            start.record()
            _call(made[name], count[0])
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)   # milliseconds
        for name in variants * 8:   # warm-up: every code object loaded, the clocks up
            call(name)
        medians = {name: [] for name in variants}
        for _ in range(rounds):
            samples = {name: [] for name in variants}
            for _ in range(iters):
                for name in variants:   # interleaved: neighbours in time see the same machine
                    samples[name].append(call(name))
            for name in variants:
                medians[name].append(float(np.median(samples[name])))
        for name in variants:
            made[name][0].status()
            assert torch.isfinite(made[name][2]["Ybar"]).all(), name
        if parent_lib:   # the unchanged path computes what the parent computes: one more call each on the same noise key
            for name in ("parent", "mppi"):
                _call(made[name], 0)
            torch.cuda.synchronize()
            for k in ("rews", "Ybar", "qbar", "qdbar", "xbar"):
                assert torch.equal(made["parent"][2][k], made["mppi"][2][k]), (N, M, k)
        rows.append((N, M, {name: (float(np.median(v)), min(v), max(v)) for name, v in medians.items()}))
        del made
    return rows


def trace_run():
    """Under rocprofv3 --kernel-trace: per shape, TRACE_CALLS calls under mppi, then cem, then ps (the order read_kernel_csv assumes)."""
    import torch
    n = 0
    for N, M in SHAPES:
        made = _contexts(N, M, RULES, None)
        for name in RULES:
            for _ in range(TRACE_CALLS):
                n += 1
                _call(made[name], n)
            torch.cuda.synchronize()
        del made


def read_kernel_csv(path):
    """{(N, M): {rule: (median us, min, max)}} of the K4a kernel's own duration from trace_run's kernel trace."""
    rows = list(csv.DictReader(open(path)))
    name_key = next(k for k in rows[0] if k.lower().replace("_", "") == "kernelname")
    t0 = next(k for k in rows[0] if k.lower().startswith("start"))
    t1 = next(k for k in rows[0] if k.lower().startswith("end"))
    rows.sort(key=lambda r: int(r[t0]))
    dur = {"weights_kernel": [], "elite_weights_kernel": []}
    for r in rows:
        base = r[name_key].split("(")[0].replace(".kd", "").strip()
        if base in dur:
            dur[base].append((int(r[t1]) - int(r[t0])) / 1e3)
    assert len(dur["weights_kernel"]) == len(SHAPES) * TRACE_CALLS and len(dur["elite_weights_kernel"]) == 2 * len(SHAPES) * TRACE_CALLS, \
        {k: len(v) for k, v in dur.items()}
    out = {}
    for i, shape in enumerate(SHAPES):
        w = dur["weights_kernel"][i * TRACE_CALLS:(i + 1) * TRACE_CALLS][TRACE_SKIP:]
        e = dur["elite_weights_kernel"][2 * i * TRACE_CALLS:2 * (i + 1) * TRACE_CALLS]
        cells = {"mppi": w, "cem": e[:TRACE_CALLS][TRACE_SKIP:], "ps": e[TRACE_CALLS:][TRACE_SKIP:]}
        out[shape] = {k: (float(np.median(v)), min(v), max(v)) for k, v in cells.items()}
    return out


def closed_loop(example, rule, ticks):
    import torch
    from dial_mpc_amd.core.dial_core import MBDPI, _generator
    dc, ec, env = _load(example, update_method=rule, elite_frac=ELITE_FRAC)
    mbdpi = MBDPI(dc, env, kernel_rng=True)
    rng = _generator(dc.seed, mbdpi.device)
    state = env.reset(rng)
    Y0 = torch.zeros((dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=mbdpi.device)
    rews, height, plan_ms = [], [], []
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for t in range(ticks):
        state = env.step(state, Y0[0])
        rews.append(float(state.reward))
        height.append(float(state.pipeline_state.qpos[2]))
        start.record()
        Y0 = mbdpi.shift(Y0)
        n_diffuse = dc.Ndiffuse_init if t == 0 else dc.Ndiffuse
        factors = mbdpi.sigma_control[None, :] * (dc.traj_diffuse_factor ** torch.arange(n_diffuse, device=mbdpi.device))[:, None]
        for i in range(n_diffuse):
            rng, Y0, info = mbdpi.reverse_once(state, rng, Y0, factors[i], want_bars=(i == n_diffuse - 1))
        stop.record()
        stop.synchronize()
        mbdpi.ctx.status()
        plan_ms.append(start.elapsed_time(stop))
    return dict(N=dc.Nsample, H=dc.Hsample, Ndiffuse=dc.Ndiffuse, K=mbdpi.n_elite, reward=float(np.mean(rews)), h_min=float(np.min(height)),
                p50=float(np.percentile(plan_ms[1:], 50)), finite=bool(np.isfinite(rews).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-label", default="the parent commit")
    ap.add_argument("--kernel-csv", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=150)
    ap.add_argument("--session", default="", help="free text naming the box and session of the run (goes into the file)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_rule.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_update_rule: no GPU visible; these are GPU measurements")
    if a.trace_run:
        return trace_run()
    import socket
    import time
    props = torch.cuda.get_device_properties(0)
    cell = lambda v: f"{v[0]:.4f} ({v[1]:.4f} .. {v[2]:.4f})"   # noqa: E731
    lines = [f"# Update rules (mppi / cem / ps) on {torch.cuda.get_device_name(0)} (tools/bench_update_rule.py)", "",
             f"Device: {props.name}, {props.multi_processor_count} CUs, {props.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, "
             f"HIP {torch.version.hip}.  Box `{socket.gethostname()}`, session of {time.strftime('%Y-%m-%d %H:%M', time.gmtime())} UTC"
             f"{'; ' + a.session if a.session else ''}: every table below comes from this one box and session.", "",
             "## Time of one reverse_once[_batch] (Go2 trot, H = 16, in-kernel noise, with bars), ms", "",
             f"Device events around each call; one context per column in one process, interleaved call by call after 8 warm-up calls each; "
             f"per cell the median over {a.rounds} rounds of the median of {a.iters} calls and the lowest .. highest round median (the "
             f"run-to-run spread).  cem: elite_frac {ELITE_FRAC} (K = 205 at N = 2048, 6554 at N = 65536); ps: K = 1.  "
             + (f"parent: libdialhip.so built from {a.parent_label}, loaded next to this build, under its only rule." if a.parent_lib else
                "No parent build was given."), "",
             "| N | M | parent mppi | mppi | cem | ps | mppi / parent | cem / mppi | ps / mppi |", "|---|---|---|---|---|---|---|---|---|"]
    if a.kernel_csv:
        k = read_kernel_csv(a.kernel_csv)   # (before the long part: a trace of another run fails here)
    timing = bench_timing(a.iters, a.rounds, a.parent_lib)
    for N, M, r in timing:
        par = r.get("parent")
        lines.append(f"| {N} | {M} | {cell(par) if par else '-'} | {cell(r['mppi'])} | {cell(r['cem'])} | {cell(r['ps'])} | "
                     f"{'x %.4f' % (r['mppi'][0] / par[0]) if par else '-'} | x {r['cem'][0] / r['mppi'][0]:.4f} | x {r['ps'][0] / r['mppi'][0]:.4f} |")
    lines.append("")
    if a.kernel_csv:
        lines += ["## The K4a kernel alone, us (one `rocprofv3 --kernel-trace` run of `--trace-run`, no counters)", "",
                  f"Per shape {TRACE_CALLS} calls under each rule, the first {TRACE_SKIP} dropped; median (lowest .. highest) of the kernel's own "
                  f"duration.  mppi: `weights_kernel`; cem and ps: `elite_weights_kernel`.", "",
                  "| N | M | weights_kernel (mppi) | elite_weights_kernel (cem) | elite_weights_kernel (ps) | cem / mppi | ps / mppi |",
                  "|---|---|---|---|---|---|---|"]
        for (N, M), r in k.items():
            c3 = lambda v: f"{v[0]:.2f} ({v[1]:.2f} .. {v[2]:.2f})"   # noqa: E731
            lines.append(f"| {N} | {M} | {c3(r['mppi'])} | {c3(r['cem'])} | {c3(r['ps'])} | x {r['cem'][0] / r['mppi'][0]:.2f} | x {r['ps'][0] / r['mppi'][0]:.2f} |")
        lines.append("")
    lines += [f"## Closed loop: {a.ticks} control steps ({a.ticks * 0.02:.1f} s) of the synchronous driver's loop at the example's sizes", "",
              "In-kernel noise, seed of the example.  Recorded, not gated.  The sampling noise follows DIAL's annealing schedule under every "
              "rule (no adaptation from the elites).", "",
              "| example | rule | N | H | K | mean reward | lowest trunk height, m | plan p50, ms |", "|---|---|---|---|---|---|---|---|"]
    for example in ("unitree_go2_trot", "unitree_h1_jog"):
        for rule in RULES:
            c = closed_loop(example, rule, a.ticks)
            lines.append(f"| {example} | {rule} | {c['N']} | {c['H']} | {c['K'] or '-'} | {c['reward']:.4f}{'' if c['finite'] else ' (not finite)'} | "
                         f"{c['h_min']:.3f} | {c['p50']:.3f} |")
    lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
