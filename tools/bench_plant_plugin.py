"""Latency and throughput of the plant simulator of a custom environment (csrc/plant_kernel.h: plant_kernel at the model's dimensions in the env's
task plugin) next to the built-in plant kernels, on one GPU; writes profiles/plant_plugin.md.  Modelled on tools/bench_plant.py.

  async step   one sim step of one plant (M = 1, K = 1), including the [qpos, qvel] copy to the host
  batch        M = 256 plants x K = 4 steps per launch, in plant steps per second

for four paths, measured in ONE process, alternating from round to round, after a warm-up, the device synchronised before every
clock read:
  plugin CTRL   go2_stance_residual's plant-enabled plugin, rows applied as the actuators' ctrl
  plugin LAW    the same plugin, its control law evaluated at every sim step (DIAL_PLANT_LAW)
  Go2 kernel    the Go2 trot deploy example on the Go2's own plant kernel (plant_kernel<DimsGo2>)
  capacity      the same example on the capacity-dimension plant kernel (dial_options.force_generic)

and the new kernel's registers, spills and scratch for the Go2 and the H1 push-crate scene (tests/plugin_cases.py) from hipcc's
-Rpass-analysis=kernel-resource-usage (cross-compiles: --resources-only needs no GPU and writes --resources-json, which a later run
can read instead of compiling again).

Usage: python tools/bench_plant_plugin.py [--iters 300] [--rounds 5] [--out profiles/plant_plugin.md]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATHS = ("plugin CTRL", "plugin LAW", "Go2 kernel", "capacity")


def kernel_resources(model_name):
    """{field: value} of plant_kernel<DimsUser...> in the plant-enabled probe plugin (with the probe law) of a model of tests/plugin_cases.py."""
    from control_cases import control_source
    from dial_mpc_amd import plugin
    from dial_mpc_amd._lib import _COMMON, _CSRC, _FAST
    from plugin_cases import case_model_dict, probe_source
    with tempfile.TemporaryDirectory() as work:
        open(os.path.join(work, "dial_plugin_dims.h"), "w").write(plugin.dims_header(case_model_dict(model_name)))
        open(os.path.join(work, "dial_user_reward.hip"), "w").write(probe_source())
        open(os.path.join(work, "dial_user_control.hip"), "w").write(control_source())
        cmd = [plugin._hipcc()] + list(_COMMON + _FAST) + ["-DDIAL_PLUGIN_USER_CTRL=1", "-DDIAL_PLUGIN_PLANT=1", "-Rpass-analysis=kernel-resource-usage",
                                                       "-I", work, "-c", "-o", os.path.join(work, "plugin.o"), os.path.join(_CSRC, "plugin.hip")]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-4000:])
    out, cur = {}, None
    for line in r.stdout.splitlines():
        line = re.sub(r"\s*\[-Rpass[^\]]*\]\s*$", "", line)
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\S+)$", line)
        if m and cur and "plant_kernel" in cur:
            out[m.group(1).strip()] = m.group(2)
    if not out:
        raise RuntimeError("no kernel-resource-usage remark names plant_kernel:\n" + r.stdout[-2000:])
    return out


def resources():
    names = ("go2", "h1_push_crate")
    with ThreadPoolExecutor(max_workers=2) as ex:
        return dict(zip(names, ex.map(kernel_resources, names)))


def _plants(M):
    import importlib
    import yaml
    from dial_mpc_amd import _lib
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    from dial_mpc_amd.deploy.plant import Plant
    from dial_mpc_amd.utils.io_utils import get_example_path
    importlib.import_module("dial_mpc_amd.examples.custom_env.go2_stance_residual")
    d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_stance_residual_deploy.yaml")))
    dc, _, cenv = load_dial_and_env(d)
    _, _, benv = load_dial_and_env(yaml.safe_load(open(get_example_path("unitree_go2_trot_deploy.yaml"))))
    T = dc.Hsample + 1
    plants = {"plugin CTRL": Plant(cenv, 0.005, "torque", M=M), "plugin LAW": Plant(cenv, 0.005, "law", M=M),
              "Go2 kernel": Plant(benv, 0.005, "torque", M=M), "capacity": Plant(benv, 0.005, "torque", M=M)}
    cap = plants["capacity"]
    model, task = benv.make_model(), benv.make_task()
    model.timestep = 0.005
    task.n_frames, task.dt = 1, 0.005
    cap.ctx = _lib.Context(model, task, None, cap.ctx.device, options=dict(force_generic=1))
    cap.reset()
    assert cap.ctx.debug_last_launch()["inst"] == 0 and plants["Go2 kernel"].ctx.debug_last_launch()["inst"] == 1
    assert plants["plugin LAW"].ctx.debug_last_launch()["inst"] == 7
    return plants, np.zeros((T, benv.sys.nu), np.float32)


def measure(iters, rounds):
    import torch
    out = {k: {} for k in PATHS}
    plants, rows = _plants(1)
    lat = {k: [] for k in PATHS}
    for rnd in range(rounds + 1):   # (round 0 is the warm-up)
        for k in PATHS:
            p = plants[k]
            p.reset()
            torch.cuda.synchronize()
            for _ in range(iters):
                t0 = time.perf_counter()
                p.step(rows, np.float32(p.t), K=1)
                p.qpos_qvel()            # (the copy to the host synchronises)
                if rnd:
                    lat[k].append(time.perf_counter() - t0)
    for k in PATHS:
        a = np.asarray(lat[k]) * 1e3
        out[k]["p50"], out[k]["p95"] = float(np.percentile(a, 50)), float(np.percentile(a, 95))
    plants, rows = _plants(256)
    n = max(20, iters // 10)
    rate = {k: [] for k in PATHS}
    for rnd in range(rounds + 1):
        for k in PATHS:
            p = plants[k]
            p.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                p.step(rows, 0.0, K=4)
            torch.cuda.synchronize()
            if rnd:
                rate[k].append(256 * 4 * n / (time.perf_counter() - t0))
    for k in PATHS:
        out[k]["steps_per_s"] = float(np.median(rate[k]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_plugin.md"))
    ap.add_argument("--resources-json", default=None, help="read the kernel's resources from this file if it exists, else write them there")
    ap.add_argument("--resources-only", action="store_true", help="compile and record the resources, measure nothing (no GPU needed)")
    a = ap.parse_args()
    if a.resources_json and os.path.exists(a.resources_json) and not a.resources_only:
        res = json.load(open(a.resources_json))
    else:
        res = resources()
        if a.resources_json:
            json.dump(res, open(a.resources_json, "w"), indent=1)
    if a.resources_only:
        print(json.dumps(res, indent=1))
        return
    import torch
    m = measure(a.iters, a.rounds)
    lines = [f"# Plant simulator of a custom environment on {torch.cuda.get_device_name(0)} (tools/bench_plant_plugin.py, sim_dt 5 ms)", "",
             f"Four paths in one process, alternating over {a.rounds} rounds after a warm-up round, {a.iters} async steps per round and path;",
             "the device is synchronised before every clock read.  Plugin: go2_stance_residual's; built-in: the Go2 trot deploy example.", "",
             "| path | async step p50 (M = 1, K = 1, incl. state copy) | p95 | batch (M = 256, K = 4) |", "|---|---|---|---|"]
    for k in PATHS:
        lines.append(f"| {k} | {m[k]['p50']:.3f} ms | {m[k]['p95']:.3f} ms | {m[k]['steps_per_s'] / 1e6:.3f} M plant steps/s |")
    lo, hi = sorted((m["Go2 kernel"]["steps_per_s"], m["capacity"]["steps_per_s"]))
    lines.append("")
    for k in PATHS[:2]:
        r = m[k]["steps_per_s"]
        where = "between the Go2's own kernel and the capacity-dimension kernel, as expected" if lo <= r <= hi else (
            "NOT between the two built-in kernels: it is " + ("slower than both" if r < lo else "faster than both"))
        lines.append(f"Batch throughput of {k}: {where}.")
    lines += ["", "## plant_kernel<DimsUser...>: registers, spills, scratch (-Rpass-analysis=kernel-resource-usage, plugin with the probe law)", ""]
    fields = [f for f in ("VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize", "Occupancy", "LDS Size") if
              all(f in res[n] for n in res)]
    lines += ["| model | " + " | ".join(fields) + " |", "|---" * (len(fields) + 1) + "|"]
    for n in res:
        lines.append(f"| {n} | " + " | ".join(str(res[n][f]) for f in fields) + " |")
    scratch = {n: int(res[n].get("ScratchSize", 0)) for n in res}
    lines += ["", "The kernel uses no scratch memory." if not any(scratch.values()) else
              "The kernel HAS scratch memory: " + ", ".join(f"{n} {v} bytes per lane" for n, v in scratch.items() if v) + "."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
