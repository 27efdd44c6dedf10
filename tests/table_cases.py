"""Shared pieces of the reference-table tests (tests/test_user_table.py on the CPU, tests/test_gpu_user_table.py on the GPU): the probe
reward of tests/table_probe.hip built into the plugins of two models of tests/plugin_cases.py, the same reward next to the probe law
of tests/table_law_probe.hip on the Go2, and the host rule in a brute-force form."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from plugin_cases import HERE, case_model_dict

PROBE = os.path.join(HERE, "table_probe.hip")
LAW = os.path.join(HERE, "table_law_probe.hip")
MODELS = ("go2", "go2_crate")               # go2_crate: the capped workspace with its global overflow area
TF = dict(row=1, table=2, row_index=3, table_rows=4, table_cols=5)   # field codes of table_probe.hip
TPROBE_NONE, TPROBE_BAD = -777.0, -12345.0


def build_table_plugins(jobs=3):
    """Build (or find in the cache) the probe plugins -> {"go2", "go2_crate": reward only; "go2_law": reward and law}."""
    from dial_mpc_amd.plugin import build_plugin
    rew, law = open(PROBE).read(), open(LAW).read()
    jobs_ = [(n, dict(model=case_model_dict(n), reward_src=rew)) for n in MODELS]
    jobs_.append(("go2_law", dict(model=case_model_dict("go2"), reward_src=rew, control_src=law)))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        paths = list(ex.map(lambda j: build_plugin(j[1]["model"], j[1]["reward_src"], control_src=j[1].get("control_src")), jobs_))
    return dict(zip([j[0] for j in jobs_], paths))


def build_stale_plugins():
    """The Go2 probe plugin as sources before the table would build it, through two switches of the plugin's translation unit ->
    {"no_table": no dial_plugin_table_v1 export, "version": an export that reports another table version}."""
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import build_plugin
    rew, md = open(PROBE).read(), case_model_dict("go2")
    flags = {"no_table": ["-DDIAL_PLUGIN_NO_TABLE"], "version": ["-DDIAL_PLUGIN_TABLE_VERSION=99"]}
    with ThreadPoolExecutor(max_workers=2) as ex:
        paths = list(ex.map(lambda f: build_plugin(md, rew, flags=_COMMON + _FAST + f), flags.values()))
    return dict(zip(flags, paths))


def brute_row(step, row0, rows, mode):
    """The rule of csrc/user_reward.h by walking: start at row 0 and move one row per unit of step + row0, forwards or backwards,
    stopping at the ends ("clamp") or going round ("wrap")."""
    r = step + row0
    if mode == "clamp":
        return 0 if r < 0 else (rows - 1 if r > rows - 1 else r)
    i = 0
    for _ in range(abs(r)):
        i += 1 if r > 0 else -1
        if i == rows:
            i = 0
        if i < 0:
            i = rows - 1
    return i


def dyadic_table(rows, cols, seed=0):
    """[rows, cols] float32 of DISTINCT dyadic values k / 64: exact in fp32, and equality with a host element identifies it."""
    k = np.random.default_rng(seed).permutation(4 * rows * cols)[:rows * cols] - 2 * rows * cols
    return (k.astype(np.float32) / 64.0).reshape(rows, cols)
