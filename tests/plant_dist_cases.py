"""Shared pieces of the plant-disturbance tests (tests/test_plant_dist_host.py on the CPU, tests/test_gpu_plant_dist.py on the GPU):
the Go2 probe plugin of tests/plugin_cases.py built WITH the disturbed plant kernel (build_plugin(plant_disturbance=True):
csrc/plant_dist_kernel.h behind the fifth table), without a law and with the probe law of tests/control_probe.hip, and the packing of
one buffer of disturbance rows."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from plant_plugin_cases import law_source
from plugin_cases import case_model_dict, probe_source

DIST_SYMBOL = "dial_plugin_plant_dist_v1"
VARIANTS = [("go2", None), ("go2", "probe")]


def build_dist_plugin(model="go2", law=None):
    """The probe plugin of a model of plugin_cases.CASES with the disturbed plant kernel (found in the cache after the first build)."""
    from dial_mpc_amd.plugin import build_plugin
    return build_plugin(case_model_dict(model), probe_source(), control_src=law_source(law), plant_disturbance=True)


def build_dist_plugins(variants=VARIANTS):
    variants = list(variants)
    with ThreadPoolExecutor(max_workers=2) as ex:
        paths = list(ex.map(lambda v: build_dist_plugin(*v), variants))
    return dict(zip(variants, paths))


def pack(nu, nv, gains, biases, events):
    """[M, 2 nu + E (2 + nv)] float32 from per-plant gains [M, nu], biases [M, nu] and event lists (t0, t1, dv[nv]), each list padded
    to the longest with the all-zero slot -> (rows, E)."""
    from dial_mpc_amd.deploy.plant import disturbance_row
    E = max(len(e) for e in events)
    pad = (0.0, 0.0, np.zeros(nv))
    rows = np.stack([disturbance_row(nu, nv, gains[m], biases[m], list(events[m]) + [pad] * (E - len(events[m]))) for m in range(len(events))])
    return rows, E
