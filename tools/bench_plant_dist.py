"""What plant disturbances cost, and a record of a planner recovering from a shove; writes profiles/plant_dist.md.

  kernels      dial_plant_step, K = 16 steps per launch from the same start state, at M = 1 and M = 256, on the Go2's own
               instantiation and on the capacity-dimension kernel (force_generic), three variants measured in ONE process and
               interleaved launch by launch:
                 undisturbed   nothing bound (plant_kernel, libdialplant.so)
                 identity      gain 1, bias 0, no event slot (plant_dist_kernel, libdialplantdist.so)
                 16 events     16 event slots whose windows hold every step, dv = 0: every slot fires at every step -- the worst case,
                               16 x nv LDS additions per step -- and the physics stays the undisturbed run's, step for step
               Device events around each launch; the median over --iters launches per variant, and the spread of the medians of
               --rounds repetitions.  There is no threshold: the numbers are a record.
  closed loop  M = 8 Go2 trot plants (sim_dt 5 ms, PD at the plant rate) under the grouped planner (one reverse_once_batch launch per
               annealing iteration for all 8 plans), sync schedule; plants 4 .. 7 are shoved sideways once (Plant.shove).  Base height
               and lateral velocity over time, shoved against unshoved.  A record, not a gate.

Usage: python tools/bench_plant_dist.py [--iters 200] [--rounds 5] [--ticks 150] [--out profiles/plant_dist.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIM_DT, K_BENCH = 0.005, 16


def _load(example):
    import yaml
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    return d, load_dial_and_env(d)


def bench_kernels(iters, rounds):
    import torch
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import disturbance_row
    _, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    T = dc.Hsample + 1
    out = []
    for label, options in (("Go2 (its own instantiation)", None), ("Go2 on the capacity-dimension kernel", dict(force_generic=1))):
        model, task = env.make_model(), env.make_task()
        model.timestep = SIM_DT
        task.n_frames, task.dt = 1, SIM_DT
        ctx = _lib.Context(model, task, None, device=0, options=options)
        dev = ctx.torch_device
        for M in (1, 256):
            q0 = np.tile(np.asarray(env._init_q, np.float32), (M, 1))
            s0 = ctx.env_reset_batch(torch.as_tensor(q0, device=dev), torch.zeros((M, ctx.nv), dtype=torch.float32, device=dev))
            rows = torch.zeros((M, T, ctx.nu), dtype=torch.float32, device=dev)
            pt = torch.zeros(M, dtype=torch.float32, device=dev)
            st, tt = s0.clone(), torch.zeros(M, dtype=torch.float64, device=dev)
            ident = torch.as_tensor(np.tile(disturbance_row(ctx.nu, ctx.nv), (M, 1)), device=dev)
            live = [(-1.0, 1.0e6, np.zeros(ctx.nv))] * _lib.PLANT_MAX_EVENTS
            busy = torch.as_tensor(np.tile(disturbance_row(ctx.nu, ctx.nv, None, None, live), (M, 1)), device=dev)
            variants = [("undisturbed", None, 0), ("identity", ident, 0), ("16 events", busy, _lib.PLANT_MAX_EVENTS)]
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def launch(dist, E):
                ctx.set_plant_disturbance(dist, E)
                st.copy_(s0)
                tt.zero_()
                start.record()
                ctx.plant_step(st, tt, pt, rows, 0.02, SIM_DT, K_BENCH, _lib.PLANT_CTRL)
                stop.record()
                stop.synchronize()
                return start.elapsed_time(stop) * 1e3   # microseconds
            for _, dist, E in variants * 10:   # warm-up: every variant's code object loaded, every shape seen
                launch(dist, E)
            medians = {name: [] for name, _, _ in variants}
            for _ in range(rounds):
                samples = {name: [] for name, _, _ in variants}
                for _ in range(iters):
                    for name, dist, E in variants:   # interleaved: neighbours in time see the same machine
                        samples[name].append(launch(dist, E))
                for name in samples:
                    medians[name].append(float(np.median(samples[name])))
            ctx.set_plant_disturbance(None)
            assert torch.isfinite(st).all()
            out.append((label, M, {name: (float(np.median(v)), min(v), max(v)) for name, v in medians.items()}))
    return out


def closed_loop(ticks, shove_t=1.0, shove_s=0.1, shove_dv=1.0):
    import torch
    from dial_mpc_amd import _abi
    from dial_mpc_amd.core.dial_core import MBDPI, _generator
    from dial_mpc_amd.deploy.plant import Plant
    _, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    M, K = 8, int(round(ec.dt / SIM_DT))
    mbdpi = MBDPI(dc, env, n_plans=M)
    dev = mbdpi.device
    plant = Plant(env, SIM_DT, "position", M=M, device=mbdpi.ctx.device, disturbance=True)
    shoved = list(range(M // 2, M))
    for m in shoved:
        plant.shove(shove_t, shove_s, [0.0, shove_dv, 0.0, 0.0, 0.0, 0.0], plant=m)
    nq, nv = plant.nq, plant.nv
    packed = torch.stack([env.reset().packed for _ in range(M)]).contiguous()
    step_slot = nq + 2 * nv + _abi.MACROS["DIAL_INFO_STEP"]
    rng = _generator(dc.seed, dev)
    Y = torch.zeros((M, dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=dev)
    rec = []
    for tick in range(ticks):
        packed[:, :nq + nv] = plant.states[:, :nq + nv]
        packed[:, step_slot] = float(tick)
        Y = mbdpi.shift_batch(Y)
        for i in range(dc.Ndiffuse_init if tick == 0 else dc.Ndiffuse):
            rng, Y, _ = mbdpi.reverse_once_batch(packed, rng, Y, np.array([dc.traj_diffuse_factor ** i], np.float32), want_bars=False)
        mbdpi.ctx.status()
        us = mbdpi.node2u_vvmap(Y).cpu().numpy()
        targets = np.stack([[env.act2joint(u) for u in us[m]] for m in range(M)]).astype(np.float32)
        plant.step(targets, plant.t, K=K, hold_first=True)
        s = plant.states[:, :nq + nv].cpu().numpy()
        rec.append((plant.t, s[:, 2].copy(), s[:, nq + 1].copy(), s[:, 0].copy()))
    return dict(M=M, shoved=shoved, shove=(shove_t, shove_s, shove_dv), rec=rec, Nsample=dc.Nsample, Ndiffuse=dc.Ndiffuse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_dist.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plant_dist: no GPU visible; these are GPU measurements")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# Plant disturbances on {torch.cuda.get_device_name(0)} (tools/bench_plant_dist.py)", "",
             f"Device: {props.name}, {props.multi_processor_count} CUs, {props.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, "
             f"HIP {torch.version.hip}.", "",
             f"## Kernel cost: one launch of K = {K_BENCH} sim steps (Go2 trot scene, sim_dt 5 ms, DIAL_PLANT_CTRL, zero rows, from the home pose)", "",
             f"Device events around each launch; the three variants interleaved launch by launch in one process; per cell the median over "
             f"{a.rounds} rounds of the median of {a.iters} launches, and the lowest .. highest round median.", "",
             "| kernel | M | undisturbed | identity data (disturbed kernel) | 16 events firing at every step (dv = 0) |", "|---|---|---|---|---|"]
    for label, M, r in bench_kernels(a.iters, a.rounds):
        base = r["undisturbed"][0]
        cell = lambda v: f"{v[0]:.1f} us ({v[1]:.1f} .. {v[2]:.1f}; {100.0 * (v[0] / base - 1.0):+.1f} %)"   # noqa: E731
        lines.append(f"| {label} | {M} | {r['undisturbed'][0]:.1f} us ({r['undisturbed'][1]:.1f} .. {r['undisturbed'][2]:.1f}) | "
                     f"{cell(r['identity'])} | {cell(r['16 events'])} |")
    lines += ["", "Percentages are against the undisturbed kernel of the same row.  No threshold applies: this is a record.", ""]
    c = closed_loop(a.ticks)
    t, s, dv = c["shove"]
    lines += [f"## Closed loop: {c['M']} Go2 trot plants under the grouped planner, plants {c['shoved'][0]} .. {c['shoved'][-1]} shoved", "",
              f"Sync schedule, Nsample {c['Nsample']}, Ndiffuse {c['Ndiffuse']}, PD at the plant rate (sim_leg_control: position).  The shove: "
              f"{dv} m/s sideways (+y, world frame) spread over {s} s from t = {t} s.  Mean (min .. max) over the four plants of each group.", "",
              "| t [s] | base height, unshoved [m] | base height, shoved [m] | lateral velocity, unshoved [m/s] | lateral velocity, shoved [m/s] |",
              "|---|---|---|---|---|"]
    sh = np.array(c["shoved"])
    un = np.array([m for m in range(c["M"]) if m not in c["shoved"]])
    fmt = lambda v, p: f"{v.mean():.{p}f} ({v.min():.{p}f} .. {v.max():.{p}f})"   # noqa: E731
    for k, (tk, h, vy, _) in enumerate(c["rec"]):
        if (k + 1) % 5 == 0:
            lines.append(f"| {tk:.2f} | {fmt(h[un], 3)} | {fmt(h[sh], 3)} | {fmt(vy[un], 2)} | {fmt(vy[sh], 2)} |")
    hs = np.array([r[1] for r in c["rec"]])
    lines += ["", f"Lowest base height over the run: unshoved {hs[:, un].min():.3f} m, shoved {hs[:, sh].min():.3f} m.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
