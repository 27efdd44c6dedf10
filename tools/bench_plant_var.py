"""What per-plant model constants cost, and a record of one planner model driving sixteen mismatched plants; writes
profiles/plant_var.md.

  kernels      dial_plant_step, K = 16 steps per launch from the same start state, at M = 1 and M = 256, on the Go2's own
               instantiation and on the capacity-dimension kernel (force_generic), five variants measured in ONE process and
               interleaved launch by launch:
                 undisturbed        nothing bound (plant_kernel, libdialplant.so)
                 identity dist      gain 1, bias 0, no event slot (plant_dist_kernel, libdialplantdist.so)
                 V = 1              one block of constants, the context's own model, every plant indexes it (plant_var_kernel)
                 V = M              M distinct models (trunk density 1 + b / 1000), plant b stages block b: M different staging reads
                                    instead of one L2-hot block
                 V = M + dist       the same with the identity disturbance bound next to it
               Device events around each launch; the median over --iters launches per variant, and the spread of the medians of
               --rounds repetitions.  The ratios are against the parent's kernels; there is no threshold: the numbers are a record.
  closed loop  sixteen Go2 trot plants (sim_dt 5 ms, PD at the plant rate) under the grouped planner, which plans with the ONE nominal
               model, for 3 s: trunk mass_scale in {0.8, 1.0, 1.2, 1.4} x friction_scale in {1.0, 0.7, 0.5, 0.35}.  Per plant: mean
               base height, mean forward-velocity error after the ramp-up, and whether it fell.  A record, not a gate.

Usage: python tools/bench_plant_var.py [--iters 200] [--rounds 5] [--ticks 150] [--out profiles/plant_var.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIM_DT, K_BENCH = 0.005, 16
NAMES = ("undisturbed", "identity dist", "V = 1", "V = M", "V = M + dist")


def _load(example):
    import yaml
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    return d, load_dial_and_env(d)


def _struct(md):
    from dial_mpc_amd import _abi
    st = _abi.make_model(md)
    st.timestep = SIM_DT
    return st


def bench_kernels(iters, rounds):
    import torch
    from dial_mpc_amd import _lib
    from dial_mpc_amd.deploy.plant import disturbance_row
    from dial_mpc_amd.mjcf import vary_model
    _, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    T = dc.Hsample + 1
    distinct = [_struct(vary_model(env.sys.model, mass_scale={1: 1.0 + b / 1000.0})) for b in range(256)]
    out = []
    for label, options in (("Go2 (its own instantiation)", None), ("Go2 on the capacity-dimension kernel", dict(force_generic=1))):
        model, task = env.make_model(), env.make_task()
        model.timestep = SIM_DT
        task.n_frames, task.dt = 1, SIM_DT
        # one context per variant, bound once: binding V = 256 models builds and uploads 256 blocks, far too slow to repeat per launch
        ctxs = {name: _lib.Context(model, task, None, device=0, options=options) for name in NAMES}
        ctx = ctxs["undisturbed"]
        dev = ctx.torch_device
        for M in (1, 256):
            q0 = np.tile(np.asarray(env._init_q, np.float32), (M, 1))
            s0 = ctx.env_reset_batch(torch.as_tensor(q0, device=dev), torch.zeros((M, ctx.nv), dtype=torch.float32, device=dev))
            rows = torch.zeros((M, T, ctx.nu), dtype=torch.float32, device=dev)
            pt = torch.zeros(M, dtype=torch.float32, device=dev)
            st, tt = s0.clone(), torch.zeros(M, dtype=torch.float64, device=dev)
            ident = torch.as_tensor(np.tile(disturbance_row(ctx.nu, ctx.nv), (M, 1)), device=dev)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctxs["identity dist"].set_plant_disturbance(ident, 0)
            ctxs["V = 1"].set_plant_models([model], [0] * M)
            ctxs["V = M"].set_plant_models(distinct[:M])
            ctxs["V = M + dist"].set_plant_models(distinct[:M])
            ctxs["V = M + dist"].set_plant_disturbance(ident, 0)

            def launch(cx):
                st.copy_(s0)
                tt.zero_()
                start.record()
                cx.plant_step(st, tt, pt, rows, 0.02, SIM_DT, K_BENCH, _lib.PLANT_CTRL)
                stop.record()
                stop.synchronize()
                return start.elapsed_time(stop) * 1e3   # microseconds
            for name in NAMES * 10:   # warm-up: every variant's code object loaded, every shape seen
                launch(ctxs[name])
            medians = {name: [] for name in NAMES}
            for _ in range(rounds):
                samples = {name: [] for name in NAMES}
                for _ in range(iters):
                    for name in NAMES:   # interleaved: neighbours in time see the same machine
                        samples[name].append(launch(ctxs[name]))
                for name in samples:
                    medians[name].append(float(np.median(samples[name])))
            for cx in ctxs.values():
                cx.set_plant_models(None)
                cx.set_plant_disturbance(None)
            assert torch.isfinite(st).all()
            out.append((label, M, {name: (float(np.median(v)), min(v), max(v)) for name, v in medians.items()}))
    return out


MASS, FRICTION = (0.8, 1.0, 1.2, 1.4), (1.0, 0.7, 0.5, 0.35)


def closed_loop(ticks):
    import torch
    from dial_mpc_amd import _abi
    from dial_mpc_amd.core.dial_core import MBDPI, _generator
    from dial_mpc_amd.deploy.plant import Plant
    from dial_mpc_amd.mjcf import vary_model
    d, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    grid = [(ms, fs) for ms in MASS for fs in FRICTION]
    M, K = len(grid), int(round(ec.dt / SIM_DT))
    mbdpi = MBDPI(dc, env, n_plans=M)
    dev = mbdpi.device
    models = [vary_model(env.sys.model, mass_scale={1: ms}, friction_scale=fs) for ms, fs in grid]
    plant = Plant(env, SIM_DT, "position", M=M, device=mbdpi.ctx.device, models=models)
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
        quat = s[:, 3:7]
        up = 1.0 - 2.0 * (quat[:, 1] ** 2 + quat[:, 2] ** 2)
        rec.append((plant.t, s[:, 2].copy(), s[:, nq].copy(), up))
    return dict(grid=grid, rec=rec, vx=float(d.get("default_vx", 0.0)), ramp=float(d.get("ramp_up_time", 0.0)), Nsample=dc.Nsample,
                Ndiffuse=dc.Ndiffuse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_var.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plant_var: no GPU visible; these are GPU measurements")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# Per-plant model constants on {torch.cuda.get_device_name(0)} (tools/bench_plant_var.py)", "",
             f"Device: {props.name}, {props.multi_processor_count} CUs, {props.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, "
             f"HIP {torch.version.hip}.", "",
             f"## Kernel cost: one launch of K = {K_BENCH} sim steps (Go2 trot scene, sim_dt 5 ms, DIAL_PLANT_CTRL, zero rows, from the home pose)", "",
             f"Device events around each launch; the five variants interleaved launch by launch in one process (one context per variant, bound once); per cell the median over {a.rounds} rounds of the median of {a.iters} launches, and the lowest .. highest round median.  "
             f"V = M: plant b stages its own block of constants (M distinct models, trunk density 1 + b / 1000); at M = 1 that is V = 1 with "
             f"another model.", "",
             "| kernel | M | undisturbed (plant_kernel) | identity disturbance (plant_dist_kernel) | V = 1 | V = M distinct models | V = M + identity disturbance |",
             "|---|---|---|---|---|---|---|"]
    for label, M, r in bench_kernels(a.iters, a.rounds):
        base, dbase = r["undisturbed"][0], r["identity dist"][0]
        plain = lambda v: f"{v[0]:.1f} us ({v[1]:.1f} .. {v[2]:.1f})"   # noqa: E731
        cell = lambda v, b: f"{v[0]:.1f} us ({v[1]:.1f} .. {v[2]:.1f}; x {v[0] / b:.3f})"   # noqa: E731
        lines.append(f"| {label} | {M} | {plain(r['undisturbed'])} | {plain(r['identity dist'])} | {cell(r['V = 1'], base)} | "
                     f"{cell(r['V = M'], base)} | {cell(r['V = M + dist'], dbase)} |")
    lines += ["", "Ratios: V = 1 and V = M against the undisturbed kernel of the same row, V = M + disturbance against the disturbed kernel of "
              "the same row (the parent's kernels).  No threshold applies: this is a record.", ""]
    c = closed_loop(a.ticks)
    ts = np.array([r[0] for r in c["rec"]])
    h = np.array([r[1] for r in c["rec"]])
    vx = np.array([r[2] for r in c["rec"]])
    up = np.array([r[3] for r in c["rec"]])
    after = ts > c["ramp"]
    lines += [f"## Closed loop: sixteen Go2 trot plants under the grouped planner for {ts[-1]:.2f} s, one nominal planner model", "",
              f"Sync schedule, Nsample {c['Nsample']}, Ndiffuse {c['Ndiffuse']}, PD at the plant rate (sim_leg_control: position), commanded "
              f"forward velocity {c['vx']} m/s after a {c['ramp']} s ramp.  Plant b runs trunk mass_scale x friction_scale of its row "
              f"(mjcf.vary_model; one launch of plant_var_kernel per control tick for all sixteen).  Mean base height over the run; forward-"
              f"velocity error = mean over t > {c['ramp']} s of (vx - {c['vx']}); fell = base height below 0.15 m or the trunk's up axis below "
              f"0.5 at any tick.", "",
              "| plant | trunk mass_scale | friction_scale | mean base height [m] | lowest base height [m] | mean forward-velocity error [m/s] | fell |",
              "|---|---|---|---|---|---|---|"]
    for b, (ms, fs) in enumerate(c["grid"]):
        fell = bool((h[:, b] < 0.15).any() or (up[:, b] < 0.5).any() or not np.isfinite(h[:, b]).all())
        lines.append(f"| {b} | {ms} | {fs} | {h[:, b].mean():.3f} | {h[:, b].min():.3f} | {(vx[after, b] - c['vx']).mean():+.3f} | {'yes' if fell else 'no'} |")
    lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
