"""Latency and throughput of the plant simulator (deploy/plant.py, dial_plant_step) on one GPU; writes profiles/plant.md.

  async step   one sim step of one plant (M = 1, K = 1), including the [qpos, qvel] copy to the host: what dial-mpc-sim pays per 5 ms
  sync tick    one control tick of the sync loop (K = 4, row 0), including the copy
  batch        M = 256 plants x K = 4 steps per launch, in plant steps per second
  planner      MBDPublisher's plan latency (p50 over --ticks ticks, Go2 trot deploy example) with a dial-mpc-sim process running
               beside it, against the same loop with the in-process FakePlant test double (tests/fake_plant.py)

Usage: python tools/bench_plant.py [--iters 500] [--ticks 100] [--out profiles/plant.md]
"""
import argparse
import os
import subprocess
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _load(example):
    import yaml
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.utils.io_utils import get_example_path
    d = yaml.safe_load(open(get_example_path(example + ".yaml")))
    return d, load_dial_and_env(d)


def _pct(xs):
    a = np.asarray(xs) * 1e3
    return float(np.percentile(a, 50)), float(np.percentile(a, 95))


def bench_plant(iters):
    import torch
    from dial_mpc_amd.deploy.plant import Plant
    _, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    T = dc.Hsample + 1
    rows = np.zeros((T, env.sys.nu), np.float32)
    out = {}
    p = Plant(env, 0.005, "torque", M=1)
    for name, K, hold in (("async step (M = 1, K = 1)", 1, False), ("sync tick (M = 1, K = 4)", 4, True)):
        p.reset()
        lat = []
        for i in range(iters + 20):
            t0 = time.perf_counter()
            p.step(rows, np.float32(p.t), K=K, hold_first=hold)
            p.qpos_qvel()
            if i >= 20:
                lat.append(time.perf_counter() - t0)
        out[name] = _pct(lat)
    pb = Plant(env, 0.005, "torque", M=256)
    for _ in range(5):
        pb.step(rows, 0.0, K=4)
    torch.cuda.synchronize()
    n = max(20, iters // 10)
    t0 = time.perf_counter()
    for _ in range(n):
        pb.step(rows, 0.0, K=4)
    torch.cuda.synchronize()
    out["batch (M = 256, K = 4)"] = 256 * 4 * n / (time.perf_counter() - t0)
    return out


def bench_planner(ticks):
    from dial_mpc_amd.deploy.dial_plan import MBDPublisher
    from fake_plant import FakePlant
    d, (dc, ec, env) = _load("unitree_go2_trot_deploy")
    prefix = "b" + uuid.uuid4().hex[:8] + "_"
    plant = FakePlant(env, dc, shm_prefix=prefix)
    try:
        pub = MBDPublisher(env, ec, dc, shm_prefix=prefix)
        lat_fake = pub.main_loop(max_ticks=ticks, on_tick=lambda k: plant.step_with_action(pub.Y[0]))
        pub.close()
    finally:
        plant.close()
    prefix = "b" + uuid.uuid4().hex[:8] + "_"
    sim = subprocess.Popen([sys.executable, "-m", "dial_mpc_amd.deploy.dial_sim", "--example", "unitree_go2_trot_deploy",
                            "--shm-prefix", prefix], cwd=ROOT, stdout=subprocess.DEVNULL)
    try:
        while not os.path.exists(f"/dev/shm/{prefix}tau_shm"):
            if sim.poll() is not None:
                raise RuntimeError("dial_sim exited early")
            time.sleep(0.05)
        pub = MBDPublisher(env, ec, dc, shm_prefix=prefix)
        lat_sim = pub.main_loop(max_ticks=ticks, sleep_when_idle=0.0)
        pub.close()
    finally:
        sim.send_signal(2)
        sim.wait(60)
    return _pct(lat_fake[1:]), _pct(lat_sim[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant.md"))
    a = ap.parse_args()
    import torch
    res = bench_plant(a.iters)
    fake, sim = bench_planner(a.ticks)
    lines = [f"# Plant simulator on {torch.cuda.get_device_name(0)} (tools/bench_plant.py, Go2 trot deploy example, sim_dt 5 ms)", "",
             "| measurement | p50 | p95 |", "|---|---|---|"]
    for k, v in res.items():
        if isinstance(v, tuple):
            lines.append(f"| {k}, incl. state copy to host | {v[0]:.3f} ms | {v[1]:.3f} ms |")
    lines += ["", f"Batch: M = 256 plants, K = 4 steps per launch: {res['batch (M = 256, K = 4)'] / 1e6:.3f} M plant steps/s.", "",
              "| MBDPublisher plan latency | p50 | p95 |", "|---|---|---|",
              f"| against FakePlant (in process) | {fake[0]:.2f} ms | {fake[1]:.2f} ms |",
              f"| with a dial-mpc-sim process running | {sim[0]:.2f} ms | {sim[1]:.2f} ms |", ""]
    async_p95 = res["async step (M = 1, K = 1)"][1]
    lines.append(f"The async step's p95 is {async_p95:.3f} ms of the 5 ms sim step"
                 + (" -- it fits comfortably." if async_p95 < 2.5 else " -- it does NOT fit comfortably inside 5 ms."))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
