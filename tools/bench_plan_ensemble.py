"""What robust planning over a model ensemble costs, and a record of sixteen mismatched plants under it; writes profiles/plan_ensemble.md.

  launches     reverse_once_batch of the Go2 trot example (N = 2048, H = 16, in-kernel noise, lean: no bars) at M = 1 and 4 plans with
               R = 1, 3 and 8 hypotheses per plan, three variants measured in ONE process and interleaved call by call:
                 (a) unbound   nothing bound: M plans on the parent's launch paths (one model, one rollout per candidate)
                 (e) ensemble  dial_set_plan_ensemble with R distinct models per plan, aggregate mean: one launch of R x M x 2049
                               wavefronts, the aggregation, ONE softmax and weighted sum per plan
                 (b) grouped   the parent's way to run the same rollouts: a context with plan_cap = M R, dial_set_plan_models per
                               plan, M R grouped plans (plan g R + r plans with model r from plan g's state) -- M R softmaxes and
                               weighted sums that a caller would throw away, R times the scratch, and (with in-kernel noise) not even
                               the same noise per hypothesis
               Device events around each call; the median over --iters calls per variant, and the spread of the medians of --rounds
               repetitions.  The variants alternate call by call, after a warm-up that loads every code object and lets the clocks
               settle, so that neighbours in time see the same machine.  There is no threshold: the numbers are a record.
  closed loop  sixteen Go2 trot plants (sim_dt 5 ms, PD at the plant rate) with the trunk at 1.0 / 1.2 / 1.4 x mass for 3 s, planned
               under the ensemble {1.0, 1.2, 1.4} with aggregate mean and with aggregate min.  Per way: how many plants stand at the
               end, next to the recorded 9 / 16 (nominal planner) and 16 / 16 (per-sample randomisation) of profiles/plan_models.md.

Usage: python tools/bench_plan_ensemble.py [--iters 30] [--rounds 5] [--ticks 150] [--out profiles/plan_ensemble.md]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIM_DT = 0.005
NAMES = ("unbound", "ensemble", "grouped")
PLANS = (1, 4)
HYPS = (1, 3, 8)


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
    distinct = [vary_model(env.sys.model, mass_scale={1: 1.0 + r / 20.0}) for r in range(max(HYPS))]
    Hn1 = dc.Hnode + 1
    out = []
    for M in PLANS:
        for Rn in HYPS:
            caps = {"unbound": M, "ensemble": M, "grouped": M * Rn}
            ctxs = {name: _lib.Context(model, task, cfg, device=0, options=dict(plan_cap=caps[name])) for name in NAMES}
            dev = ctxs["unbound"].torch_device
            nv, nu = ctxs["unbound"].nv, ctxs["unbound"].nu
            ins = {}
            for name in NAMES:
                P = caps[name]
                q0 = np.tile(np.asarray(env._init_q, np.float32), (P, 1))
                ins[name] = (ctxs[name].env_reset_batch(torch.as_tensor(q0, device=dev), torch.zeros((P, nv), dtype=torch.float32, device=dev)),
                             torch.zeros((P, Hn1, nu), dtype=torch.float32, device=dev),
                             torch.full((P, Hn1), 0.5, dtype=torch.float32, device=dev))
            ctxs["ensemble"].set_plan_ensemble(distinct[:Rn], [list(range(Rn))] * M, "mean")
            ctxs["grouped"].set_plan_models(distinct[:Rn], [p % Rn for p in range(M * Rn)])
            outs = {name: cx._out_batch(caps[name], False) for name, cx in ctxs.items()}
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            count = [0]

            def call(name):
                count[0] += 1
                start.record()
                ctxs[name].reverse_once_batch_rng(*ins[name], 1234, count[0], out=outs[name], want_bars=False)
                stop.record()
                stop.synchronize()
                return start.elapsed_time(stop)   # milliseconds
            for name in NAMES * 8:   # warm-up: every variant's code object loaded, the clocks up
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
            e, g = paths["ensemble"], paths["grouped"]
            assert e["wpb"] == 1 and e["blocks"] == Rn * M * 2049 and g["wpb"] == 1 and g["blocks"] == Rn * M * 2049, (e, g)
            ctxs["ensemble"].set_plan_ensemble(None)
            ctxs["grouped"].set_plan_models(None)
            out.append((M, Rn, {name: (float(np.median(v)), min(v), max(v)) for name, v in medians.items()}, paths))
            del ctxs
    return out


MASS = (1.0, 1.2, 1.4)
WAYS = ("ensemble {1.0, 1.2, 1.4}, aggregate mean", "ensemble {1.0, 1.2, 1.4}, aggregate min")
AGGREGATES = ("mean", "min")


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
    mbdpi = MBDPI(dc, env, n_plans=M, ensemble=dict(models=variants, aggregate=AGGREGATES[way]))
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
                hyp=mbdpi.hyp[0].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_ensemble.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_ensemble: no GPU visible; these are GPU measurements")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# Robust planning over a model ensemble on {torch.cuda.get_device_name(0)} (tools/bench_plan_ensemble.py)", "",
             f"Device: {props.name}, {props.multi_processor_count} CUs, {props.total_memory / 2**30:.0f} GiB; torch {torch.__version__}, "
             f"HIP {torch.version.hip}.", "",
             "## Cost: one reverse_once_batch of M plans with R hypotheses per plan (Go2 trot, N = 2048, H = 16, in-kernel noise, no bars)", "",
             f"Device events around each call; the three variants interleaved call by call in one process (one context per variant, bound "
             f"once, 8 warm-up calls each); per cell the median over {a.rounds} rounds of the median of {a.iters} calls, and the lowest .. "
             f"highest round median.  (a): nothing bound, M plans, one model.  (e): dial_set_plan_ensemble, R distinct models (trunk mass "
             f"x 1 + r / 20), aggregate mean: R x M x 2049 wavefronts in one launch, the aggregation, one softmax and weighted sum per "
             f"plan.  (b): the same rollouts the parent's way -- plan_cap = M R, dial_set_plan_models per plan over M R grouped plans, M R "
             f"softmaxes and weighted sums.", "",
             "| M | R | (a) unbound | (e) ensemble | (b) M R grouped plans, per-plan models | (e) / (a) | (e) / (b) |",
             "|---|---|---|---|---|---|---|"]
    for M, Rn, r, paths in bench_launches(a.iters, a.rounds):
        cell = lambda v: f"{v[0]:.3f} ms ({v[1]:.3f} .. {v[2]:.3f})"   # noqa: E731
        lines.append(f"| {M} | {Rn} | {cell(r['unbound'])} | {cell(r['ensemble'])} | {cell(r['grouped'])} | x {r['ensemble'][0] / r['unbound'][0]:.3f} | "
                     f"x {r['ensemble'][0] / r['grouped'][0]:.3f} |")
    lines += ["", "Both bound variants are a plain grid of R x M x 2049 one-wavefront workgroups.  No threshold applies: this is a record.", ""]
    res = [closed_loop(a.ticks, w) for w in range(len(WAYS))]
    c = res[0]
    lines += [f"## Closed loop: sixteen Go2 trot plants for {c['t']:.2f} s, trunk at 1.0 / 1.2 / 1.4 x mass, planned under the ensemble", "",
              f"Sync schedule, Nsample {c['Nsample']}, Ndiffuse {c['Ndiffuse']}, PD at the plant rate (sim_leg_control: position), nominal friction.  "
              f"Plant b runs trunk mass_scale {list(MASS)}[b % 3] (dial_set_plant_models).  The planner is the grouped one (sixteen plans per "
              f"launch); every plan rolls every candidate out under the three models (hypotheses {c['hyp']}, hypothesis 0 the nominal one) "
              f"and weights it by the aggregate.  fell = base height below 0.15 m or the trunk's up axis below 0.5 at any tick; standing = "
              f"not fell.  Recorded in profiles/plan_models.md for the same plants: 9 stand under the nominal planner, 16 under per-sample "
              f"randomisation over the three models.", "",
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
