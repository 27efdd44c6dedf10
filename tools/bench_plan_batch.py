#!/usr/bin/env python3
"""M-scaling of grouped planning (dial_reverse_once_batch): M independent plans from M states in one launch, against the same M plans
run one after the other through dial_reverse_once.  One JSON line per (example, N, H, M) case:

  ms_per_iter_full / _lean     one batched reverse_once of all M plans (full: every output; lean: mean action only)
  rollout_kernel_ms_full       the rollout launch of a full batched iteration alone (hipEvents, Context.set_timing)
  rollouts_per_s               M (N + 1) / ms_per_iter_full
  seq_ms_per_iter_full         the same M plans as M single-plan reverse_once calls back to back
  tick_p50_ms / tick_p95_ms    one batched control tick (env.step of M states + shift of M plans + Ndiffuse iterations, the last
                               full), over --ticks ticks; seq_tick_*: the same tick as M single-plan ticks
  speedup_full / speedup_tick  sequential / batched

Inputs as bench.py: 256 synthetic states (home + perturbed, tools: dial_mpc_amd/utils/synthetic.py) made by one env.reset_batch,
cycled; noise from the in-kernel RNG (the production setting).  Every shape is warmed up before it is timed.  Needs a GPU.

usage: python tools/bench_plan_batch.py [--steps 50] [--warmup 5] [--ticks 200] [--case go2|h1|allegro ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"go2": ("unitree_go2_trot", 2048, 16, (1, 2, 4, 8, 16, 32)),
         "h1": ("unitree_h1_jog", 2048, 16, (1, 4, 8)),
         "allegro": ("allegro_reorient", 4096, 24, (1, 2))}


def run_case(example, N, H, Ms, args):
    import torch
    import yaml
    from dial_mpc_amd.core.dial_core import MBDPI, load_dial_and_env
    from dial_mpc_amd.utils.io_utils import get_example_path
    from dial_mpc_amd.utils.synthetic import perturbed_state
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    d["Nsample"], d["Hsample"] = N, H
    dc, _, env = load_dial_and_env(d)
    pl = MBDPI(dc, env, kernel_rng=True, n_plans=max(Ms))
    dev = pl.device
    Hn1, nu = dc.Hnode + 1, pl.nu
    qs, qds = [np.array(env._init_q, dtype=np.float64)], [np.zeros(env.sys.nv)]
    for seed in range(255):
        q, qd = perturbed_state(env, seed)
        qs.append(q)
        qds.append(qd)
    pool = pl.ctx.env_reset_batch(torch.as_tensor(np.stack(qs), dtype=torch.float32, device=dev).contiguous(),
                                  torch.as_tensor(np.stack(qds), dtype=torch.float32, device=dev).contiguous())
    sigma = pl.sigma_control
    sync = torch.cuda.synchronize
    for M in Ms:
        batches = [pool[[(v * M + g) % 256 for g in range(M)]].contiguous() for v in range(4)]
        Y = torch.zeros((M, Hn1, nu), dtype=torch.float32, device=dev)

        def batched(steps, want_bars):
            nonlocal Y
            for i in range(steps):
                _, Y, _ = pl.reverse_once_batch(batches[i % 4], None, Y, sigma, want_bars=want_bars)

        def sequential(steps):
            for i in range(steps):
                for g in range(M):
                    pl.reverse_once(batches[i % 4][g], None, Y[g], sigma, want_bars=True)

        def timed(fn, *a):
            fn(args.warmup, *a)      # warm this shape
            sync()
            t0 = time.perf_counter()
            fn(args.steps, *a)
            sync()
            return (time.perf_counter() - t0) / args.steps * 1e3

        ms_full = timed(batched, True)
        pl.ctx.set_timing(True)
        batched(args.steps, True)
        sync()
        k_ms, n_launch = pl.ctx.rollout_ms()
        pl.ctx.set_timing(False)
        ms_lean = timed(batched, False)
        seq_full = timed(sequential)

        # control ticks: batched (env.step of M states, shift of M plans, Ndiffuse iterations) and the same as M single-plan ticks
        sts = [env.reset() for _ in range(M)]
        Yb = torch.zeros((M, Hn1, nu), dtype=torch.float32, device=dev)
        Ys = [torch.zeros((Hn1, nu), dtype=torch.float32, device=dev) for _ in range(M)]
        lat_b, lat_s = [], []
        for tick in range(args.ticks + 2):
            sync()
            a = time.perf_counter()
            sb = env.step_batch(sts, Yb[:, 0])
            Yb = pl.shift_batch(Yb)
            for i in range(dc.Ndiffuse):
                _, Yb, _ = pl.reverse_once_batch(sb, None, Yb, sigma * dc.traj_diffuse_factor ** i, want_bars=i == dc.Ndiffuse - 1)
            sync()
            b = time.perf_counter()
            for g in range(M):
                s1 = env.step(sts[g], Ys[g][0])
                Ys[g] = pl.shift(Ys[g])
                for i in range(dc.Ndiffuse):
                    _, Ys[g], _ = pl.reverse_once(s1, None, Ys[g], sigma * dc.traj_diffuse_factor ** i, want_bars=i == dc.Ndiffuse - 1)
            sync()
            c = time.perf_counter()
            if tick >= 2:   # (the first two: warm-up of the tick's shapes)
                lat_b.append((b - a) * 1e3)
                lat_s.append((c - b) * 1e3)
        pl.ctx.status()
        out = dict(example=example, N=N, H=H, M=M, ms_per_iter_full=round(ms_full, 4), ms_per_iter_lean=round(ms_lean, 4),
                   rollout_kernel_ms_full=round(k_ms / max(n_launch, 1), 4),
                   rollouts_per_s=round(M * (N + 1) / ms_full * 1e3), seq_ms_per_iter_full=round(seq_full, 4),
                   speedup_full=round(seq_full / ms_full, 3),
                   tick_p50_ms=round(float(np.percentile(lat_b, 50)), 3), tick_p95_ms=round(float(np.percentile(lat_b, 95)), 3),
                   seq_tick_p50_ms=round(float(np.percentile(lat_s, 50)), 3), seq_tick_p95_ms=round(float(np.percentile(lat_s, 95)), 3),
                   speedup_tick=round(float(np.percentile(lat_s, 50) / np.percentile(lat_b, 50)), 3),
                   ticks=len(lat_b), steps=args.steps, warmup=args.warmup, Ndiffuse=dc.Ndiffuse, noise="in-kernel Philox")
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--case", action="append", choices=sorted(CASES), default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_plan_batch.py: no GPU visible -- the grouped planner runs on the GPU only (no CPU fallback)")
    for name in args.case or ["go2", "h1", "allegro"]:
        run_case(*CASES[name], args)


if __name__ == "__main__":
    main()
