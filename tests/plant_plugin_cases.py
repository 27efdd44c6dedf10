"""Shared pieces of the plant-plugin tests (tests/test_plant_plugin.py on the CPU, tests/test_gpu_plant_plugin.py on the GPU): task
plugins built WITH the plant simulator's kernel (build_plugin(plant=True): csrc/plant_kernel.h's plant_kernel behind
csrc/plant_plugin.h's table) for two models of
tests/plugin_cases.py -- the Go2 and the H1 push-crate scene (nu = 19, a dry-friction row, the generic feature set) -- each without a
law and with the probe law of tests/control_probe.hip, next to the probe reward of tests/plugin_probe.hip; the Go2 also with the
table probe of tests/plant_law_probe.hip and as a plugin whose plant table reports another version."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

from control_cases import control_source
from plugin_cases import HERE, case_model_dict, probe_source

MODELS = ("go2", "h1_push_crate")
TABLE_LAW = os.path.join(HERE, "plant_law_probe.hip")
PLPROBE_BAD = -12345.0
# (model, law): law None -- no control law; "probe" -- control_probe.hip; "table" -- plant_law_probe.hip
VARIANTS = [(m, law) for m in MODELS for law in (None, "probe")] + [("go2", "table")]


def law_source(law):
    return None if law is None else (control_source() if law == "probe" else open(TABLE_LAW).read())


def build_plant_plugin(model, law=None, version=None):
    """The plant-enabled probe plugin of a model of plugin_cases.CASES (found in the cache after the first build).  version: the value
    its plant table reports instead of DIAL_PLUGIN_PLANT_VERSION (a stand-in for a plugin built from other sources)."""
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin
    flags = None if version is None else list(_COMMON + _FAST) + [f"-DDIAL_PLUGIN_PLANT_VERSION={int(version)}"]
    return build_plugin(case_model_dict(model), probe_source(), flags=flags, control_src=law_source(law), plant=True)


def build_plant_plugins(variants=VARIANTS, jobs=4):
    """Build (or find in the cache) the plant-enabled plugins -> {(model, law): path}, at most `jobs` hipcc processes at once."""
    variants = list(variants)
    with ThreadPoolExecutor(max_workers=min(jobs, 4)) as ex:
        paths = list(ex.map(lambda v: build_plant_plugin(*v), variants))
    return dict(zip(variants, paths))


def law_step_loop(t, ctrl_dt):
    """deploy.plant.law_step restated as a search: the largest integer n in [0, 2^24] with n <= t / ctrl_dt (the fp64 quotient), 0
    when there is none (negative clocks, NaN)."""
    q = float(t) / float(ctrl_dt)
    if q != q or q < 0.0:
        return 0
    lo, hi = 0, 1 << 24          # invariant: lo <= q; the answer is in [lo, hi]
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if float(mid) <= q:
            lo = mid
        else:
            hi = mid - 1
    return lo
