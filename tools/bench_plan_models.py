"""What planner model ensembles cost, and a record of sixteen mismatched plants under three planners; writes profiles/plan_models.md.

  launches     reverse_once_batch of the Go2 trot example (N = 2048, H = 16, in-kernel noise, lean: no bars) at M = 1, 4 and 32 plans,
               four variants measured in ONE process and interleaved call by call:
                 (a) unbound         nothing bound: the parent's launch paths (M = 1 the one-sample kernel with the mean-trajectory
                                     relay, M >= 2 the pair kernel's queue)
                 (b) V = 1           one block of constants, the context's own model, bound per plan (rollout_var_kernel)
                 (c) per plan V = M  M distinct models (trunk density 1 + g / 1000), plan g plans with block g
                 (d) per sample V=16 sixteen distinct models, rollout n of every plan stages block n % 16
               Device events around each call (rollouts + softmax + weighted sum); the median over --iters calls per variant, and the
               spread of the medians of --rounds repetitions.  There is no threshold: the numbers are a record.
  closed loop  sixteen Go2 trot plants (sim_dt 5 ms, PD at the plant rate) with the trunk at 1.0 / 1.2 / 1.4 x mass for 3 s, planned
               three ways: the nominal grouped planner, per-plan models matching each plant, per-sample randomisation over the three
               models.  Per way: how many plants stand at the end.  A record, not a gate.

Usage: python tools/bench_plan_models.py [--iters 40] [--rounds 5] [--ticks 150] [--out profiles/plan_models.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIM_DT = 0.005
NAMES = ("unbound", "V = 1", "per plan V = M", "per sample V = 16")
PLANS = (1, 4, 32)


def _load(example, **over):
    import yaml
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    d.update(over)
    return d, load_dial_and_env(d)


def bench_launches(iters, rounds):
    import torch
    from dial_mpc_amd import _lib
    from dial_mpc_amd.core.dial_core import make_cfg
    from dial_mpc_amd.mjcf import vary_model
    _, (dc, ec, env) = _load("unitree_go2_trot", Nsample=2048, Hsample=16)
    model, task, cfg = env.make_model(), env.make_task(), make_cfg(dc)
    distinct = [vary_model(env.sys.model, mass_scale={1: 1.0 + g / 1000.0}) for g in range(max(PLANS))]
    out = []
    for M in PLANS:
        # one context per variant, bound once
        ctxs = {name: _lib.Context(model, task, cfg, device=0, options=dict(plan_cap=M)) for name in NAMES}
        ctx = ctxs["unbound"]
        dev = ctx.torch_device
        Hn1 = dc.Hnode + 1
        q0 = np.tile(np.asarray(env._init_q, np.float32), (M, 1))
        states = ctx.env_reset_batch(torch.as_tensor(q0, device=dev), torch.zeros((M, ctx.nv), dtype=torch.float32, device=dev))
        Ybars = torch.zeros((M, Hn1, ctx.nu), dtype=torch.float32, device=dev)
        scales = torch.full((M, Hn1), 0.5, dtype=torch.float32, device=dev)
        ctxs["V = 1"].set_plan_models([model], [0] * M)
        ctxs["per plan V = M"].set_plan_models(distinct[:M], list(range(M)))
        ctxs["per sample V = 16"].set_plan_models(distinct[:16], None, per="sample")
        outs = {name: cx._out_batch(M, False) for name, cx in ctxs.items()}
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        count = [0]

        def call(name):
            count[0] += 1
            start.record()
            ctxs[name].reverse_once_batch_rng(states, Ybars, scales, 1234, count[0], out=outs[name], want_bars=False)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)   # milliseconds
        for name in NAMES * 5:   # warm-up: every variant's code object loaded
            call(name)
        paths = {name: ctxs[name].debug_last_launch() for name in NAMES}
        medians = {name: [] for name in NAMES}
        for _ in range(rounds):
            samples = {name: [] for name in NAMES}
            for _ in range(iters):
                for name in NAMES:   # interleaved: neighbours in time see the same machine
                    samples[name].append(call(name))
            for name in samples:
                medians[name].append(float(np.median(samples[name])))
        for name in NAMES:
            assert torch.isfinite(outs[name]["rews"]).all(), name
            ctxs[name].set_plan_models(None)
        out.append((M, {name: (float(np.median(v)), min(v), max(v)) for name, v in medians.items()}, paths))
        del ctxs
    return out


MASS = (1.0, 1.2, 1.4)
WAYS = ("nominal planner", "per-plan models matching each plant", "per-sample randomisation over {1.0, 1.2, 1.4}")


def closed_loop(ticks, way):
    import torch
    from dial_mpc_amd import _abi
    from dial_mpc_amd.core.dial_core import MBDPI, _generator
    from dial_mpc_amd.deploy.plant import Plant
    from dial_mpc_amd.mjcf import vary_model
    d, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    M = 16
    mass_of = [b % len(MASS) for b in range(M)]
    variants = [vary_model(env.sys.model, mass_scale={1: ms}) for ms in MASS]
    K = int(round(ec.dt / SIM_DT))
    kw = {}
    if way == 1:
        kw = dict(models=variants, model_of=mass_of, model_per="plan")
    elif way == 2:
        kw = dict(models=variants, model_of=None, model_per="sample")
    mbdpi = MBDPI(dc, env, n_plans=M, **kw)
    dev = mbdpi.device
    plant = Plant(env, SIM_DT, "position", M=M, device=mbdpi.ctx.device, models=variants, model_of=mass_of)
    nq, nv = plant.nq, plant.nv
    packed = torch.stack([env.reset().packed for _ in range(M)]).contiguous()
    step_slot = nq + 2 * nv + _abi.MACROS["DIAL_INFO_STEP"]
    rng = _generator(dc.seed, dev)
    Y = torch.zeros((M, dc.Hnode + 1, mbdpi.nu), dtype=torch.float32, device=dev)
    h, up = [], []
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
        h.append(s[:, 2].copy())
        up.append(1.0 - 2.0 * (s[:, 4] ** 2 + s[:, 5] ** 2))
    h, up = np.array(h), np.array(up)
    fell = [bool((h[:, b] < 0.15).any() or (up[:, b] < 0.5).any() or not np.isfinite(h[:, b]).all()) for b in range(M)]
    return dict(t=plant.t, mass=[MASS[k] for k in mass_of], fell=fell, h_end=h[-1], Nsample=dc.Nsample, Ndiffuse=dc.Ndiffuse,
                model_of=None if mbdpi.model_of is None else mbdpi.model_of.tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_models.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_models: no GPU visible; these are GPU measurements")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# Planner model ensembles on {torch.cuda.get_device_name(0)} (tools/bench_plan_models.py)", "",
             f"Device: {props.name}, {props.multi_processor_count} CUs, {props.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, "
             f"HIP {torch.version.hip}.", "",
             "## Cost: one reverse_once_batch of M plans (Go2 trot, N = 2048, H = 16, in-kernel noise, no bars)", "",
             f"Device events around each call (rollout launch + softmax + weighted sum); the four variants interleaved call by call in one "
             f"process (one context per variant, bound once); per cell the median over {a.rounds} rounds of the median of {a.iters} calls, and "
             f"the lowest .. highest round median; the ratio is against (a) of the same row.  (c): plan g stages its own block (trunk density "
             f"1 + g / 1000; at M = 1 that is V = 1 with another model).  (d): rollout n of every plan stages block n % 16.", "",
             "| M | (a) unbound | (b) bound, V = 1 | (c) per plan, V = M | (d) per sample, V = 16 | unbound launch path |",
             "|---|---|---|---|---|---|"]
    for M, r, paths in bench_launches(a.iters, a.rounds):
        base = r["unbound"][0]
        plain = lambda v: f"{v[0]:.3f} ms ({v[1]:.3f} .. {v[2]:.3f})"   # noqa: E731
        cell = lambda v: f"{v[0]:.3f} ms ({v[1]:.3f} .. {v[2]:.3f}; x {v[0] / base:.3f})"   # noqa: E731
        p = paths["unbound"]
        path = ("pair kernel" if p["pair"] else "one-sample kernel") + (", queue" if p["queue"] else "") + (", relay" if p["relay"] else "") + \
            f", {p['blocks']} workgroups of {p['wpb']}"
        b = paths["V = 1"]
        assert b["wpb"] == 1 and b["blocks"] == M * 2049 and not b["pair"] and not b["queue"], b
        lines.append(f"| {M} | {plain(r['unbound'])} | {cell(r['V = 1'])} | {cell(r['per plan V = M'])} | {cell(r['per sample V = 16'])} | {path} |")
    lines += ["", "The bound launches are a plain grid of M x 2049 one-wavefront workgroups of rollout_var_kernel.  No threshold applies: this "
              "is a record.", ""]
    res = [closed_loop(a.ticks, w) for w in range(3)]
    c = res[0]
    lines += [f"## Closed loop: sixteen Go2 trot plants for {c['t']:.2f} s, trunk at 1.0 / 1.2 / 1.4 x mass, three planners", "",
              f"Sync schedule, Nsample {c['Nsample']}, Ndiffuse {c['Ndiffuse']}, PD at the plant rate (sim_leg_control: position), nominal friction.  "
              f"Plant b runs trunk mass_scale {list(MASS)}[b % 3] (dial_set_plant_models).  The planner is the grouped one (sixteen plans per "
              f"launch): nominal (nothing bound), per plan (plan b plans with plant b's model), per sample (rollout n of every plan under "
              f"model n % 3, the mean trajectory under the nominal one).  fell = base height below 0.15 m or the trunk's up axis below 0.5 at "
              f"any tick; standing = not fell.", "",
              "| planner | standing of 16 | standing at 1.0 x (6 plants) | at 1.2 x (5) | at 1.4 x (5) | plants that fell |",
              "|---|---|---|---|---|---|"]
    for w, r in enumerate(res):
        stand = [not f for f in r["fell"]]
        per = {ms: sum(s for s, m in zip(stand, r["mass"]) if m == ms) for ms in MASS}
        lines.append(f"| {WAYS[w]} | {sum(stand)} | {per[1.0]} | {per[1.2]} | {per[1.4]} | {[b for b, f in enumerate(r['fell']) if f]} |")
    lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
