"""Loader and thin wrappers of libdialhip.so -- the HIP product path.

There is deliberately NO fallback: if the shared library is missing, or no HIP device is present, the
calls below raise.  Tensors are PyTorch-ROCm tensors used purely as HBM allocations; the kernels get
raw device pointers and the current torch stream through the C ABI of include/dial_mpc.h.
"""
from __future__ import annotations

import ctypes
import glob
import os
import subprocess
from typing import Optional

import numpy as np

from dial_mpc_amd import _abi

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("DIAL_HIP_LIB", os.path.join(_CSRC, "libdialhip.so"))  # override: profiling builds
_lib = None


class DialHipError(RuntimeError):
    pass


IEEE_LIB_PATH = os.path.join(_CSRC, "libdialhip_ieee.so")


N_FAMILIES = 8     # robot families of csrc/kernel_list.h (7: the Go2's two-samples-per-wavefront kernels), one translation unit each (kern_family.hip -DDIAL_FAMILY=k)
# device fast-math flags of the product build (the IEEE measurement variant drops them):
# -fno-hip-fp32-correctly-rounded-divide-sqrt: fp32 divide / sqrt via v_rcp / v_sqrt sequences (<= 2.5 ulp)
# instead of the IEEE fix-up chains; well inside the fp32 parity tolerance.
# device only: -freciprocal-math (a/b -> a * v_rcp(b), no frexp/ldexp range scaling) and -fapprox-func
# (native v_sqrt / v_rsq / v_exp / v_log without denormal fix-ups); finite-math is NOT assumed (+-inf
# control ranges are compared against).  -fno-honor-nans: min / max / clip become single v_min / v_max instead of
# compare + select chains.
# -DDIAL_FUSED_DPP: the pair kernel's broadcast-multiply-adds as single v_fmac_f32_dpp instructions (csrc/wave.h: WaveH::fma_pick);
# product build only -- the fused form IS a contraction.
_FAST = ["-DDIAL_FUSED_DPP", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-Xarch_device", "-freciprocal-math", "-Xarch_device", "-fapprox-func",
         "-Xarch_device", "-fno-honor-nans"]
# -fno-slp-vectorize (both variants): the SLP pass packs pairs of scalar fp32 ops into v_pk_* and pays for it in v_mov
# shuffles -- measured 5-6% slower on this issue-bound kernel.
# the IEEE measurement variant: none of the fast-math flags and NO fused multiply-add contraction either -- every fp32 operation
# rounded on its own, as the CPU oracle computes.  Which a * b + c pairs the compiler fuses depends on the basic-block structure around
# them, i.e. differs between two kernels that run the same arithmetic on different lane layouts: this variant is where the Go2's
# two-samples-per-wavefront kernel is compared BIT FOR BIT with the one-sample kernel (tests/test_gpu_parity.py).
# (-DDIAL_IEEE_BUILD, host code only: this variant carries no plant simulator -- dial_plant_step fails with DIAL_ERR_UNSUPPORTED)
_IEEE = ["-Xarch_device", "-ffp-contract=off", "-DDIAL_IEEE_BUILD"]
_COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Xarch_device", "-fno-slp-vectorize"]
# per robot family (kern_family.hip -DDIAL_FAMILY=k): LLVM's "max-ilp" machine-scheduling strategy for the Allegro's kernels -- their
# launch lasts as long as ONE lone wavefront's dependence chain, which the strategy shortens: A/B on one box
# (profiles/r05_ab_sched_max_ilp.txt) Allegro example 6.67 -> 6.51 ms (-2.5 %); the Go2 (+2 %), the push crate (+2 %) and the H1 (+-0)
# keep the default strategy.
# Family 4 (the capacity-dimension kernels, DimsMax): SimplifyCFG's common-code sinking is OFF.  A wavefront whose touching contacts
# exceed the capped LDS workspace runs a second inlined copy of the constraint code on an overflow area in GLOBAL memory
# (csrc/rollout_body.h: forward_tail); the sinking pass merges instructions of the two copies into one block behind pointer PHIs that
# mix the LDS and the global address space, and instruction selection then dies with "Illegal instruction detected: V_CMP_NE_U32 0,
# $src_shared_base" -- rounds 4-5 met this as "the translation unit trips an LLVM bug whenever <some loop> changes shape" and
# kept old code shapes alive for it; round 6 bisected the pass (tools/isa/llvm_sink_bug.md).
_FAMILY_FLAGS = {3: ["-mllvm", "-amdgpu-sched-strategy=max-ilp"], 4: ["-mllvm", "-simplifycfg-sink-common=false"]}


def build(force: bool = False, verbose: bool = False, ieee: bool = False) -> str:
    """Compile the library for gfx950 in-tree (hipcc cross-compiles without a GPU): csrc/dial_hip.hip (host side, K4 / K5
    kernels) and csrc/kern_family.hip once per robot family, the translation units IN PARALLEL, then one link.

    ieee=True builds the MEASUREMENT variant libdialhip_ieee.so: the same sources without the device fast-math flags
    (correctly rounded divide / sqrt, no reciprocal-math, no approximate functions, NaNs honoured) and without fused
    multiply-add contraction (_IEEE above).  It is never the product
    path; the GPU suite loads it next to the product library to show how much of the knife-edge witness traffic is the
    fast-math rounding (tests/test_gpu_parity.py: test_ieee_build_needs_no_more_witnesses)."""
    if not ieee:   # the plant simulator's kernels: a library of their own next to the product library (build_plant)
        build_plant(force=force, verbose=verbose)
        build_plant_dist(force=force, verbose=verbose)
        build_plant_var(force=force, verbose=verbose)
        build_plan_var(force=force, verbose=verbose)
        build_plan_ens(force=force, verbose=verbose)
        build_reward_defer(force=force, verbose=verbose)
        build_update_rule(force=force, verbose=verbose)
    # (the IEEE measurement variant links the deferred-reward kernel's and the elite rule's units itself: libdialhip_ieee.so's code
    #  objects are pinned by nothing)
    return _build_lib(IEEE_LIB_PATH if ieee else LIB_PATH, [(os.path.join(_CSRC, "dial_hip.hip"), [], "dial_hip.o")] +
                      ([(os.path.join(_CSRC, "reward_defer.hip"), [], "reward_defer.o"),
                        (os.path.join(_CSRC, "update_rule.hip"), [], "update_rule.o")] if ieee else []) +
                      [(os.path.join(_CSRC, "kern_family.hip"), [f"-DDIAL_FAMILY={k}"] + _FAMILY_FLAGS.get(k, []), f"kern_family_{k}.o")
                       for k in range(N_FAMILIES)], force, verbose, ieee)


PLANT_LIB_PATH = os.path.join(_CSRC, "libdialplant.so")
N_PLANT_FAMILIES = 7   # kernel_list.h's families 0 .. 6 (7, the Go2's pair kernels, has no env.step and no plant)


def build_plant(force: bool = False, verbose: bool = False) -> str:
    """libdialplant.so: the plant kernel (csrc/plant_kernel.h) once per robot family (plant_family.hip -DDIAL_FAMILY=k, the product
    flags and _FAMILY_FLAGS), kept out of libdialhip.so so that its code objects stay as shipped.  libdialhip.so's dial_plant_step
    loads it from its own directory on first use.  Same staleness check, lock and parallel compile as `build`."""
    return _build_lib(PLANT_LIB_PATH, [(os.path.join(_CSRC, "plant_family.hip"), [f"-DDIAL_FAMILY={k}"] + _FAMILY_FLAGS.get(k, []),
                                        f"plant_family_{k}.o") for k in range(N_PLANT_FAMILIES)], force, verbose, False)


PLANT_DIST_LIB_PATH = os.path.join(_CSRC, "libdialplantdist.so")


def build_plant_dist(force: bool = False, verbose: bool = False) -> str:
    """libdialplantdist.so: the disturbed plant kernel (csrc/plant_dist_kernel.h: velocity kicks and actuator errors,
    dial_set_plant_disturbance) once per robot family (plant_dist_family.hip -DDIAL_FAMILY=k, build_plant's flags), a library of its
    own so that libdialplant.so's and libdialhip.so's code objects stay as shipped.  libdialhip.so's dial_plant_step loads it from
    its own directory the first time a launch has a disturbance bound."""
    return _build_lib(PLANT_DIST_LIB_PATH, [(os.path.join(_CSRC, "plant_dist_family.hip"), [f"-DDIAL_FAMILY={k}"] + _FAMILY_FLAGS.get(k, []),
                                             f"plant_dist_family_{k}.o") for k in range(N_PLANT_FAMILIES)], force, verbose, False)


PLANT_VAR_LIB_PATH = os.path.join(_CSRC, "libdialplantvar.so")


def build_plant_var(force: bool = False, verbose: bool = False) -> str:
    """libdialplantvar.so: the plant kernel with per-plant model constants (csrc/plant_var_kernel.h: dial_set_plant_models) once per
    robot family (plant_var_family.hip -DDIAL_FAMILY=k, build_plant's flags), a library of its own so that the code objects of
    libdialplant.so, libdialplantdist.so and libdialhip.so stay as shipped.  libdialhip.so loads it from its own directory the first
    time plant models are bound."""
    return _build_lib(PLANT_VAR_LIB_PATH, [(os.path.join(_CSRC, "plant_var_family.hip"), [f"-DDIAL_FAMILY={k}"] + _FAMILY_FLAGS.get(k, []),
                                            f"plant_var_family_{k}.o") for k in range(N_PLANT_FAMILIES)], force, verbose, False)


PLAN_VAR_LIB_PATH = os.path.join(_CSRC, "libdialplanvar.so")


def build_plan_var(force: bool = False, verbose: bool = False) -> str:
    """libdialplanvar.so: the rollout kernel with per-plan / per-sample model constants (csrc/plan_var_kernel.h: dial_set_plan_models)
    once per robot family (plan_var_family.hip -DDIAL_FAMILY=k, build_plant's flags), a library of its own so that the code objects of
    libdialhip.so and the plant libraries stay as shipped.  libdialhip.so loads it from its own directory the first time planner
    models are bound."""
    return _build_lib(PLAN_VAR_LIB_PATH, [(os.path.join(_CSRC, "plan_var_family.hip"), [f"-DDIAL_FAMILY={k}"] + _FAMILY_FLAGS.get(k, []),
                                           f"plan_var_family_{k}.o") for k in range(N_PLANT_FAMILIES)], force, verbose, False)


REWARD_DEFER_LIB_PATH = os.path.join(_CSRC, "libdialdefer.so")


def build_reward_defer(force: bool = False, verbose: bool = False) -> str:
    """libdialdefer.so: the Go2's plain-grid rollout kernel that evaluates the walking task's step rewards once per rollout
    (csrc/reward_defer_kernel.h, one unit: reward_defer.hip, the product flags), a library of its own so that the code objects of
    libdialhip.so stay as shipped.  libdialhip.so loads it from its own directory when a context that can use it is created; without
    it such a context runs the per-step kernel (Context.debug_last_launch()["defer_reward"] says which)."""
    return _build_lib(REWARD_DEFER_LIB_PATH, [(os.path.join(_CSRC, "reward_defer.hip"), [], "reward_defer.o")], force, verbose, False)


UPDATE_RULE_LIB_PATH = os.path.join(_CSRC, "libdialupdate.so")


def build_update_rule(force: bool = False, verbose: bool = False) -> str:
    """libdialupdate.so: the K4a kernel of the elite update rule (csrc/update_rule.h: elite_weights_kernel; one unit, update_rule.hip,
    the product flags) and its launcher, a library of its own so that the code objects of libdialhip.so stay as shipped.  libdialhip.so
    loads it from its own directory the first time the elite rule is bound (dial_set_update_rule); without it that call fails."""
    return _build_lib(UPDATE_RULE_LIB_PATH, [(os.path.join(_CSRC, "update_rule.hip"), [], "update_rule.o")], force, verbose, False)


PLAN_ENS_LIB_PATH = os.path.join(_CSRC, "libdialplanens.so")


def build_plan_ens(force: bool = False, verbose: bool = False) -> str:
    """libdialplanens.so: the ensemble rollout kernel (csrc/plan_ens_kernel.h: dial_set_plan_ensemble) once per robot family
    (plan_ens_family.hip -DDIAL_FAMILY=k, build_plant's flags) and the aggregation kernel in a unit of its own
    (plan_ens_aggregate.hip), a library of its own so that the code objects of every other library stay as shipped.  libdialhip.so
    loads it from its own directory the first time an ensemble is bound."""
    return _build_lib(PLAN_ENS_LIB_PATH, [(os.path.join(_CSRC, "plan_ens_family.hip"), [f"-DDIAL_FAMILY={k}"] + _FAMILY_FLAGS.get(k, []),
                                           f"plan_ens_family_{k}.o") for k in range(N_PLANT_FAMILIES)] +
                      [(os.path.join(_CSRC, "plan_ens_aggregate.hip"), [], "plan_ens_aggregate.o")], force, verbose, False)


def _build_lib(out: str, units, force: bool, verbose: bool, ieee: bool) -> str:
    from concurrent.futures import ThreadPoolExecutor
    # every source of the library takes part in the staleness check (a stale .so must never ship silently)
    srcs = sorted(glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(_CSRC, "*.hip"))) + [_abi.HEADER, os.path.abspath(__file__)]   # (this file: the flags)
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = _COMMON + (_IEEE if ieee else _FAST) + ([] if ieee else os.environ.get("DIAL_HIPCC_EXTRA", "").split())
    # ONE builder at a time per output file (ranks of a multi-process launch, pytest-xdist workers that all find a stale tree): an
    # exclusive flock on build/<library>.lock, staleness re-checked once the lock is held -- the others find a fresh library.
    # Objects go to a directory of THIS call (flags hashed into its name, pid-suffixed), the library is linked next to its final place
    # and moved there atomically; the directory and the temporary are removed whether the build succeeds or not.
    import fcntl
    import hashlib
    import shutil
    build_root = os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "build")
    os.makedirs(build_root, exist_ok=True)
    tag = hashlib.sha1(" ".join(flags).encode()).hexdigest()[:8]
    objdir = os.path.join(build_root, f"obj_{os.path.basename(out)}_{tag}_{os.getpid()}")
    tmp_out = f"{out}.{os.getpid()}.tmp"
    with open(os.path.join(build_root, os.path.basename(out) + ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
                return out
            os.makedirs(objdir, exist_ok=True)
            units = [(src, defs, os.path.join(objdir, obj)) for src, defs, obj in units]

            def compile_unit(u):
                src, defs, obj = u
                cmd = [hipcc] + flags + defs + ["-c", "-o", obj, src]
                if verbose:
                    print(" ".join(cmd))
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if r.returncode != 0:   # (the compiler's own words, not just the exit status: a failed unit must be impossible to overlook)
                    raise DialHipError(f"hipcc failed ({r.returncode}) on {os.path.basename(src)} {' '.join(defs)}:\n{r.stdout[-4000:]}")
                return obj
            with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 1, 16)) as pool:
                objs = list(pool.map(compile_unit, units))
            cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp_out] + objs
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(tmp_out, out)
            return out
        finally:
            shutil.rmtree(objdir, ignore_errors=True)
            if os.path.exists(tmp_out):
                os.remove(tmp_out)
            fcntl.flock(lock, fcntl.LOCK_UN)


def load(path: Optional[str] = None):
    """The product library (cached), or -- path given -- another build of it (measurement variants; not cached)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib_path = LIB_PATH if path is None else path
    if not os.path.exists(lib_path):
        raise DialHipError(f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP extension is the only compute path; there is no CPU fallback)")
    lib = ctypes.CDLL(lib_path)
    vp, ci, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
    lib.dial_create.argtypes = [ctypes.POINTER(vp), vp, vp, vp, ci]
    lib.dial_create_sharded.argtypes = [ctypes.POINTER(vp), vp, vp, vp, ci, ci]
    lib.dial_create_ex.argtypes = [ctypes.POINTER(vp), vp, vp, vp, ci, ci, vp]
    lib.dial_set_state_trace.argtypes = [vp, fp, ci]
    lib.dial_destroy.argtypes = [vp]
    lib.dial_destroy.restype = None
    lib.dial_last_error.argtypes = [vp]
    lib.dial_last_error.restype = ctypes.c_char_p
    lib.dial_rollout.argtypes = [vp, fp, fp, ci, fp, fp, fp, fp, vp]
    lib.dial_reverse_once.argtypes = [vp, fp, fp, fp, ci, fp, fp, fp, fp, fp, fp, vp]
    lib.dial_shard_rollout.argtypes = [vp, fp, fp, fp, ci, fp, ci, ci, fp, vp]
    lib.dial_shard_reduce.argtypes = [vp, fp, ci, ci, ci, ci, fp, vp]
    lib.dial_shard_ybar.argtypes = [vp, fp, ci, fp, fp, fp, ci, fp, vp]
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    lib.dial_reverse_once_rng.argtypes = [vp, fp, fp, fp, ci, u64, u32, fp, fp, fp, fp, fp, vp]
    lib.dial_shard_rollout_rng.argtypes = [vp, fp, fp, fp, ci, u64, u32, ci, ci, ci, fp, vp]
    lib.dial_rng_fill.argtypes = [vp, u64, u32, ci, ci, fp, vp]
    lib.dial_shard_ybar_rng.argtypes = [vp, fp, ci, u64, u32, fp, fp, ci, fp, vp]
    lib.dial_shard_pack_rewards.argtypes = [vp, fp, ci, ci, ci, fp, vp]
    try:
        lib.dial_shard_ybar_gathered.argtypes = [vp, fp, ci, ci, ci, fp, fp, fp, ci, fp, fp, vp]
        lib.dial_shard_ybar_gathered_rng.argtypes = [vp, fp, ci, ci, ci, u64, u32, fp, fp, ci, fp, fp, vp]
        lib.dial_shard_reduce_gathered.argtypes = [vp, fp, ci, ci, ci, ci, ci, ci, fp, fp, vp]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (an A/B build of an earlier round may lack them; the product library may not)
            raise
    lib.dial_shift.argtypes = [vp, fp, vp]
    lib.dial_env_step.argtypes = [vp, fp, fp, fp, fp, fp, vp]
    try:
        lib.dial_reverse_once_batch.argtypes = [vp, fp, fp, fp, ci, fp, ci, fp, fp, fp, fp, fp, vp]
        lib.dial_reverse_once_batch_rng.argtypes = [vp, fp, fp, fp, ci, u64, u32, ci, fp, fp, fp, fp, fp, vp]
        lib.dial_shift_batch.argtypes = [vp, fp, ci, vp]
        lib.dial_env_step_batch.argtypes = [vp, fp, fp, fp, fp, fp, ci, vp]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack the grouped entry points)
            raise
    try:
        lib.dial_create_plugin.argtypes = [ctypes.POINTER(vp), vp, vp, vp, ci, vp, ctypes.c_char_p, vp, ci]
        lib.dial_set_user_params.argtypes = [vp, vp, ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack the task-plugin entry points)
            raise
    try:
        lib.dial_set_plan_params.argtypes = [vp, fp, ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack per-plan task parameters)
            raise
    try:
        lib.dial_user_control.argtypes = [vp, fp, fp, ci, fp, vp]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack user control laws)
            raise
    try:
        lib.dial_set_user_table.argtypes = [vp, fp, ci, ci, ci, ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack the reference table)
            raise
    try:
        lib.dial_plant_step.argtypes = [vp, fp, fp, fp, fp, ci, ctypes.c_double, ctypes.c_double, ci, ci, fp, ci, vp]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack the plant simulator)
            raise
    try:
        lib.dial_set_plant_disturbance.argtypes = [vp, fp, ci, ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack plant disturbances)
            raise
    try:
        lib.dial_set_plant_models.argtypes = [vp, vp, ci, vp, ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack per-plant models)
            raise
    try:
        lib.dial_set_plan_models.argtypes = [vp, vp, ci, vp, ci, ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack planner models)
            raise
    try:
        lib.dial_set_plan_ensemble.argtypes = [vp, vp, ci, vp, ci, ci, ci, ctypes.c_float]
        lib.dial_get_ensemble_rewards.argtypes = [vp, fp, ci, vp]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack plan ensembles)
            raise
    try:
        lib.dial_set_update_rule.argtypes = [vp, ci, ci]
        lib.dial_get_weights.argtypes = [vp, fp, ci, vp]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack the update rules)
            raise
    lib.dial_env_reset.argtypes = [vp, fp, fp, fp, fp, fp, vp]
    lib.dial_env_reset_batch.argtypes = [vp, fp, fp, fp, fp, fp, ci, vp]
    lib.dial_status.argtypes = [vp]
    lib.dial_set_timing.argtypes = [vp, ci]
    lib.dial_get_rollout_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ci)]
    lib.dial_abi_sizes.argtypes = [ctypes.POINTER(ci)] * 3
    lib.dial_selftest.argtypes = [ctypes.POINTER(ctypes.c_float)]
    lib.dial_debug_scratch.argtypes = [vp] + [ctypes.POINTER(vp)] * 6
    lib.dial_lds_bytes.argtypes = [vp]
    lib.dial_debug_resident_rollouts.argtypes = [vp, ctypes.c_int]
    try:
        lib.dial_debug_last_launch.argtypes = [vp, ctypes.POINTER(ci), ci]
    except AttributeError:
        if path is None and "DIAL_HIP_LIB" not in os.environ:   # (A/B builds of earlier commits lack the launch record)
            raise
    if path is None:
        _lib = lib
    return lib


EXPORTED = ("dial_create", "dial_create_sharded", "dial_create_ex", "dial_set_state_trace", "dial_destroy", "dial_last_error", "dial_rollout", "dial_reverse_once",
            "dial_shard_rollout", "dial_shard_reduce", "dial_shard_ybar", "dial_reverse_once_rng",
            "dial_shard_rollout_rng", "dial_rng_fill", "dial_shard_ybar_rng", "dial_shard_pack_rewards",
            "dial_shard_ybar_gathered", "dial_shard_ybar_gathered_rng", "dial_shard_reduce_gathered", "dial_shift", "dial_env_step", "dial_env_reset", "dial_env_reset_batch",
            "dial_status", "dial_set_timing", "dial_get_rollout_ms", "dial_abi_sizes",
            "dial_reverse_once_batch", "dial_reverse_once_batch_rng", "dial_shift_batch", "dial_env_step_batch",
            "dial_create_plugin", "dial_set_user_params", "dial_set_plan_params", "dial_plant_step", "dial_user_control",
            "dial_set_user_table", "dial_set_plant_disturbance", "dial_set_plant_models",
            "dial_set_plan_models", "dial_set_plan_ensemble", "dial_get_ensemble_rewards",
            "dial_set_update_rule", "dial_get_weights")

# dial_plant_step flags (include/dial_mpc.h)
PLANT_CTRL, PLANT_PD, PLANT_HOLD_FIRST = (_abi.MACROS[k] for k in ("DIAL_PLANT_CTRL", "DIAL_PLANT_PD", "DIAL_PLANT_HOLD_FIRST"))
PLANT_LAW = _abi.MACROS["DIAL_PLANT_LAW"]   # a task plugin built with a plant and a control law: the rows are normalised actions
PLANT_MAX_EVENTS = _abi.MACROS["DIAL_PLANT_MAX_EVENTS"]   # event slots of a plant's disturbance row (dial_set_plant_disturbance)


def plant_dist_row(nu: int, nv: int, n_events: int) -> int:
    """Floats of one plant's disturbance row, gain[nu] | bias[nu] | E x { t0, t1, dv[nv] } (DIAL_PLANT_DIST_ROW of include/dial_mpc.h)."""
    return 2 * int(nu) + int(n_events) * (2 + int(nv))


MAX_PLANT_MODELS = _abi.MACROS["DIAL_MAX_PLANT_MODELS"]   # distinct plant models of one binding (dial_set_plant_models)
MAX_PLANTS = _abi.MACROS["DIAL_MAX_PLANTS"]


def plant_model_index(model_of, V: int, M: Optional[int] = None) -> np.ndarray:
    """The index dial_set_plant_models takes: contiguous int32 [M] with 0 <= model_of[b] < V.  model_of None: M must be V (or None),
    and plant b runs model b.  Raises ValueError on another shape, a non-integer or an index out of range."""
    V = int(V)
    if not 1 <= V <= MAX_PLANT_MODELS:
        raise ValueError(f"plant models: {V} models; 1 .. DIAL_MAX_PLANT_MODELS = {MAX_PLANT_MODELS} are allowed")
    if model_of is None:
        if M is not None and int(M) != V:
            raise ValueError(f"plant models: {V} models for M = {M} plants need a model_of (without one, plant b runs model b)")
        return np.arange(V, dtype=np.int32)
    a = np.asarray(model_of)
    if a.ndim != 1 or a.size < 1 or a.size > MAX_PLANTS or not np.issubdtype(a.dtype, np.integer) or (M is not None and a.size != int(M)):
        raise ValueError(f"plant models: model_of is an integer list of one index per plant{'' if M is None else f' (M = {M})'}; got "
                         f"shape {a.shape}, dtype {a.dtype}")
    if a.min() < 0 or a.max() >= V:
        raise ValueError(f"plant models: model_of holds indices outside 0 .. V - 1 = {V - 1}")
    return np.ascontiguousarray(a, dtype=np.int32)


MAX_PLAN_MODELS = _abi.MACROS["DIAL_MAX_PLAN_MODELS"]   # distinct planner models of one binding (dial_set_plan_models)
PLAN_MODEL_MODES = {"plan": _abi.MACROS["DIAL_PLAN_MODELS_PER_PLAN"], "sample": _abi.MACROS["DIAL_PLAN_MODELS_PER_SAMPLE"]}


def plan_model_index(model_of, V: int, rows: int, per: str = "plan") -> np.ndarray:
    """The index dial_set_plan_models takes: contiguous int32 [rows] with 0 <= model_of[r] < V.  per="plan": one row per plan (rows =
    the plans the binding serves, at most the context's plan capacity), default row g = g % V.  per="sample": rows = Nsample + 1, one
    row per noisy sample and the mean trajectory's last; default n % V for the noisy samples and 0 for the mean trajectory.  Raises
    ValueError on an unknown `per`, another shape, a non-integer or an index out of range."""
    if per not in PLAN_MODEL_MODES:
        raise ValueError(f"plan models: per = {per!r}; 'plan' or 'sample' are allowed")
    V, rows = int(V), int(rows)
    if not 1 <= V <= MAX_PLAN_MODELS:
        raise ValueError(f"plan models: {V} models; 1 .. DIAL_MAX_PLAN_MODELS = {MAX_PLAN_MODELS} are allowed")
    if rows < 1 or (per == "plan" and rows > _abi.MACROS["DIAL_MAX_PLANS"]) or (per == "sample" and rows < 2):
        raise ValueError(f"plan models: {rows} rows; per plan 1 .. DIAL_MAX_PLANS = {_abi.MACROS['DIAL_MAX_PLANS']}, per sample Nsample + 1 >= 2")
    if model_of is None:
        a = np.arange(rows, dtype=np.int32) % V
        if per == "sample":
            a[rows - 1] = 0   # the mean trajectory: the first model
        return a
    a = np.asarray(model_of)
    if a.ndim != 1 or a.size != rows or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"plan models: model_of is an integer list of {rows} entries (per {per}: "
                         f"{'one per plan' if per == 'plan' else 'Nsample + 1, the mean trajectory last'}); got shape {a.shape}, dtype {a.dtype}")
    if a.min() < 0 or a.max() >= V:
        raise ValueError(f"plan models: model_of holds indices outside 0 .. V - 1 = {V - 1}")
    return np.ascontiguousarray(a, dtype=np.int32)


MAX_ENSEMBLE = _abi.MACROS["DIAL_MAX_ENSEMBLE"]   # hypotheses per plan of one ensemble (dial_set_plan_ensemble)
ENSEMBLE_AGGREGATES = {"mean": _abi.MACROS["DIAL_ENSEMBLE_MEAN"], "min": _abi.MACROS["DIAL_ENSEMBLE_MIN"], "cvar": _abi.MACROS["DIAL_ENSEMBLE_CVAR"]}


def plan_ensemble_index(hyp, V: int, rows: int, R: Optional[int] = None) -> np.ndarray:
    """The hypotheses dial_set_plan_ensemble takes: contiguous int32 [rows, R] with 0 <= hyp[g, r] < V -- plan g rolls every
    candidate out under models[hyp[g, 0 .. R-1]], hypothesis 0 its nominal model.  hyp None: every plan gets all V models in order
    (R = V).  A flat list of R indices is shared by all plans.  Raises ValueError on another shape, a non-integer, an index out of
    range, R outside 1 .. DIAL_MAX_ENSEMBLE or rows outside 1 .. DIAL_MAX_PLANS."""
    V, rows = int(V), int(rows)
    if not 1 <= V <= MAX_PLAN_MODELS:
        raise ValueError(f"plan ensemble: {V} models; 1 .. DIAL_MAX_PLAN_MODELS = {MAX_PLAN_MODELS} are allowed")
    if not 1 <= rows <= _abi.MACROS["DIAL_MAX_PLANS"]:
        raise ValueError(f"plan ensemble: {rows} rows; 1 .. DIAL_MAX_PLANS = {_abi.MACROS['DIAL_MAX_PLANS']} are allowed (one per plan)")
    if hyp is None:
        if R is not None and int(R) != V:
            raise ValueError(f"plan ensemble: R = {R} without hypotheses; the default is all V = {V} models in order (R = V)")
        a = np.tile(np.arange(V, dtype=np.int32), (rows, 1))
    else:
        a = np.asarray(hyp)
        if a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"plan ensemble: hyp is a non-empty integer list [R] or [rows][R]; got shape {a.shape}, dtype {a.dtype}")
        if a.ndim == 1:
            a = np.tile(a, (rows, 1))
        if a.ndim != 2 or a.shape[0] != rows or (R is not None and a.shape[1] != int(R)):
            raise ValueError(f"plan ensemble: hyp is [R] or [rows = {rows}][R{'' if R is None else f' = {int(R)}'}]; got shape {a.shape}")
        if a.min() < 0 or a.max() >= V:
            raise ValueError(f"plan ensemble: hyp holds indices outside 0 .. V - 1 = {V - 1}")
    if not 1 <= a.shape[1] <= MAX_ENSEMBLE:
        raise ValueError(f"plan ensemble: R = {a.shape[1]} hypotheses per plan; 1 .. DIAL_MAX_ENSEMBLE = {MAX_ENSEMBLE} are allowed")
    return np.ascontiguousarray(a, dtype=np.int32)


# update rules (dial_set_update_rule): how a plan's rewards become the weights of its candidates
UPDATE_RULES = {"mppi": _abi.MACROS["DIAL_UPDATE_MPPI"], "elite": _abi.MACROS["DIAL_UPDATE_ELITE"]}
UPDATE_METHODS = {"mppi": "mppi", "cem": "elite", "ps": "elite"}   # DialConfig.update_method -> the rule that serves it


def elite_count(method: str, Nsample: int, elite_frac: float = 0.1, n_elite: int = 0) -> int:
    """The elite count K of DialConfig.update_method `method` over Nsample noisy samples and the mean trajectory: "ps" (best sample)
    -> 1; "cem" (elite mean) -> n_elite when it is above 0, else ceil(round(elite_frac * Nsample, 9)), at least 1 (the rounding keeps
    0.1 * 2000-style products that land one ulp above an integer from gaining an elite).  Raises KeyError for another method ("mppi"
    has no elite count), ValueError for elite_frac outside (0, 1], a negative n_elite or a count above Nsample + 1."""
    import math
    if method == "ps":
        return 1
    if method != "cem":
        raise KeyError(method)
    Nsample, n_elite = int(Nsample), int(n_elite)
    if n_elite < 0:
        raise ValueError(f"elite count: n_elite = {n_elite} is negative (0: derive it from elite_frac)")
    if n_elite > 0:
        K = n_elite
    else:
        frac = float(elite_frac)
        if not 0.0 < frac <= 1.0:   # (a NaN fails both comparisons)
            raise ValueError(f"elite count: elite_frac = {elite_frac!r} is outside (0, 1]")
        K = max(1, math.ceil(round(frac * Nsample, 9)))
    if K > Nsample + 1:
        raise ValueError(f"elite count: K = {K} exceeds the Nsample + 1 = {Nsample + 1} candidates of a plan")
    return K


def plan_param_rows(rows) -> np.ndarray:
    """Per-plan task parameters as dial_set_plan_params takes them: `rows` [M, n] (array, nested list or tensor; n <= DIAL_USER_PARAMS)
    -> float32 [M, DIAL_USER_PARAMS], each row padded with zeros.  Raises ValueError on another shape."""
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    a = np.asarray(rows, dtype=np.float32)
    cap, max_plans = _abi.MACROS["DIAL_USER_PARAMS"], _abi.MACROS["DIAL_MAX_PLANS"]
    if a.ndim != 2 or a.shape[1] > cap:
        raise ValueError(f"per-plan task parameters are [M, n] rows with n <= DIAL_USER_PARAMS = {cap}; got shape {a.shape}")
    if not 1 <= a.shape[0] <= max_plans:
        raise ValueError(f"per-plan task parameters: {a.shape[0]} rows; 1 .. DIAL_MAX_PLANS = {max_plans} are allowed")
    out = np.zeros((a.shape[0], cap), np.float32)
    out[:, :a.shape[1]] = a
    return out


TABLE_MODES = {"clamp": _abi.MACROS["DIAL_TABLE_CLAMP"], "wrap": _abi.MACROS["DIAL_TABLE_WRAP"]}
TABLE_MAX_ROWS = 1 << 24


def table_mode(mode) -> int:
    """"clamp" / "wrap" (or the DIAL_TABLE_* value) -> the mode dial_set_user_table takes.  Raises ValueError on anything else."""
    if isinstance(mode, str) and mode in TABLE_MODES:
        return TABLE_MODES[mode]
    if not isinstance(mode, (str, bool)) and mode in TABLE_MODES.values():
        return int(mode)
    raise ValueError(f"reference table mode {mode!r}; one of {sorted(TABLE_MODES)}")


def check_user_table(shape, dtype=None) -> None:
    """Raise ValueError unless `shape` (and `dtype`, where given) is a reference table's: [rows, cols] float32 with
    1 <= rows <= 1 << 24 and 1 <= cols <= DIAL_USER_TABLE_COLS."""
    cap = _abi.MACROS["DIAL_USER_TABLE_COLS"]
    shape = tuple(int(n) for n in shape)
    if len(shape) != 2:
        raise ValueError(f"a reference table is [rows, cols]; got shape {shape}")
    if not 1 <= shape[0] <= TABLE_MAX_ROWS:
        raise ValueError(f"a reference table has 1 .. {TABLE_MAX_ROWS} rows; got shape {shape}")
    if not 1 <= shape[1] <= cap:
        raise ValueError(f"a reference table has 1 .. DIAL_USER_TABLE_COLS = {cap} columns; got shape {shape}")
    if dtype is not None and str(dtype) != "torch.float32" and (str(dtype).startswith("torch.") or np.dtype(dtype) != np.float32):
        raise ValueError(f"a reference table is float32; got {dtype}")


def user_table_array(table) -> np.ndarray:
    """A host table (array or nested list) as dial_set_user_table takes it: float32 [rows, cols], C-contiguous.  Floating-point and
    integer input is converted; anything else, another rank or size raises ValueError."""
    a = np.asarray(table)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"a reference table holds floats; got dtype {a.dtype}")
    check_user_table(a.shape)
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float32", "need contiguous float32 device tensors"
    return t.data_ptr()


def _stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


class Context:
    """One dial_ctx: (device, model, task, cfg).  Not thread-safe (C ABI contract)."""

    def __init__(self, model: "_abi.DialModel", task: "_abi.DialTask", cfg: Optional["_abi.DialCfg"],
                 device: Optional[int] = None, n_local_cap: Optional[int] = None, lib_path: Optional[str] = None,
                 options: Optional[dict] = None, plugin: Optional[str] = None, user_params=None,
                 user_table=None, table_row0: int = 0, table_mode: str = "clamp"):
        """n_local_cap: size the rollout scratch for that many local samples (one rank of a sharded run).
        lib_path: another build of the library (measurement variants, e.g. libdialhip_ieee.so).
        options: fields of `dial_options` (include/dial_mpc.h) -- launch-shape / measurement switches, e.g.
        dict(no_queue=1); none of them changes a result bit.  The library itself reads no environment variables.
        plugin: path of a task plugin (dial_mpc_amd/plugin.py: build_plugin) whose kernels serve this context (task.kind =
        DIAL_TASK_USER; dial_create_plugin), user_params its float task parameters (<= DIAL_USER_PARAMS; set_user_params),
        user_table / table_row0 / table_mode its reference table (set_user_table)."""
        import torch
        self.lib = load(lib_path)
        if not torch.cuda.is_available():
            raise DialHipError("no HIP device visible to PyTorch: the DIAL-MPC kernels only run on a GPU")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.torch_device = torch.device("cuda", self.device)
        self.model, self.task, self.cfg = model, task, cfg
        self.nq, self.nv, self.nu, self.nbody = model.nq, model.nv, model.nu, model.nbody
        self.nx = (model.nbody - 1) * 3
        self.state_size = _abi.state_size(model.nq, model.nv)
        h = ctypes.c_void_p()
        self.options = dict(options or {})
        self.plan_cap = max(1, int(self.options.get("plan_cap", 0)))   # plans of one grouped call (reverse_once_batch)
        unknown = set(self.options) - set(_abi.DialOptions._meta)
        if unknown:
            raise ValueError(f"unknown dial_options fields: {sorted(unknown)}")
        opts = _abi.fill(_abi.DialOptions(), self.options)
        self.plugin = plugin
        self._user_table = None
        if user_table is not None and plugin is None:
            raise DialHipError("user_table: the reference table is a task plugin's (plugin=)")
        if user_table is not None and not hasattr(user_table, "is_cuda"):
            user_table = user_table_array(user_table)   # (refuse a bad table before anything is created)
        if plugin is not None:
            if n_local_cap is not None:
                raise DialHipError("task-plugin contexts cannot be sharded (n_local_cap)")
            vals = [] if user_params is None else list(user_params)
            p = self._params(vals)
            rc = self.lib.dial_create_plugin(ctypes.byref(h), ctypes.addressof(model), ctypes.addressof(task),
                                             ctypes.addressof(cfg) if cfg is not None else None, self.device, ctypes.addressof(opts),
                                             os.fsencode(plugin), ctypes.addressof(p), len(vals))
            if rc != 0:
                raise DialHipError(f"dial_create_plugin failed ({rc}): {self.lib.dial_last_error(None).decode()}")
            self.h = h
            if user_table is not None:
                self.set_user_table(user_table, table_row0, table_mode)
            return
        rc = self.lib.dial_create_ex(ctypes.byref(h), ctypes.addressof(model), ctypes.addressof(task),
                                     ctypes.addressof(cfg) if cfg is not None else None, self.device,
                                     -1 if (n_local_cap is None or cfg is None) else int(n_local_cap), ctypes.addressof(opts))
        if rc != 0:
            raise DialHipError(f"dial_create failed ({rc}): {self.lib.dial_last_error(None).decode()}")
        self.h = h

    @staticmethod
    def _params(values):
        v = [] if values is None else [float(x) for x in values]
        cap = _abi.MACROS["DIAL_USER_PARAMS"]
        if len(v) > cap:
            raise ValueError(f"{len(v)} user parameters; a task plugin takes at most DIAL_USER_PARAMS = {cap}")
        return (ctypes.c_float * max(1, len(v)))(*v) if v else (ctypes.c_float * 1)()

    def set_user_params(self, values):
        """New float task parameters of a task-plugin context (no rebuild; synchronises the device)."""
        vals = [] if values is None else list(values)
        p = self._params(vals)
        n = len(vals)
        self._check(self.lib.dial_set_user_params(self.h, ctypes.addressof(p), n), "dial_set_user_params")

    def set_plan_params(self, rows):
        """Per-plan task parameters of a task-plugin context (dial_set_plan_params): `rows` [M, n] (n <= DIAL_USER_PARAMS; host array
        or tensor, padded with zeros) -- plan g of a grouped launch / state g of env_step_batch reads row g, single-plan launches row 0.
        The device copy stays alive while bound.  None unbinds: the shared parameters (set_user_params) apply again."""
        import torch
        if rows is None:
            self._check(self.lib.dial_set_plan_params(self.h, None, 0), "dial_set_plan_params")
            self._plan_params = None
            return None
        cap = _abi.MACROS["DIAL_USER_PARAMS"]
        if (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] == cap
                and rows.is_contiguous() and rows.device == self.torch_device):
            dev = rows   # (already in the binding's layout: no copy)
        else:
            dev = torch.as_tensor(plan_param_rows(rows), device=self.torch_device)
        self._check(self.lib.dial_set_plan_params(self.h, dev.data_ptr(), int(dev.shape[0])), "dial_set_plan_params")
        self._plan_params = dev
        return dev

    def set_user_table(self, table, row0: int = 0, mode="clamp"):
        """The reference table of a task-plugin context (dial_set_user_table): `table` [rows, cols <= DIAL_USER_TABLE_COLS], a host
        array (copied to the device) or a contiguous float32 device tensor (bound as it is).  Every control step hands the reward
        and the control law row clamp-or-wrap(step counter + row0).  Returns the bound device tensor: it stays alive while bound and
        may be rewritten in place between launches without a new call.  None unbinds.  Synchronises the device."""
        import torch
        m = table_mode(mode)
        if table is None:
            self._check(self.lib.dial_set_user_table(self.h, None, 0, 0, 0, m), "dial_set_user_table")
            self._user_table = None
            return None
        if isinstance(table, torch.Tensor) and table.is_cuda:
            check_user_table(table.shape, table.dtype)
            if table.device != self.torch_device or not table.is_contiguous():
                raise ValueError("a device reference table must be contiguous and on the context's device")
            dev = table
        else:
            if isinstance(table, torch.Tensor):
                table = table.detach().numpy()
            dev = torch.as_tensor(user_table_array(table), device=self.torch_device)
        self._check(self.lib.dial_set_user_table(self.h, dev.data_ptr(), int(dev.shape[0]), int(dev.shape[1]), int(row0), m),
                    "dial_set_user_table")
        self._user_table = dev
        return dev

    def user_control(self, states, actions):
        """The user control law of a task-plugin context (dial_user_control) for n rows in one launch: states [n, state_size] packed,
        actions [n, nu] -> ctrl [n, nu], what env_step would hand the actuators from row g's state with row g's action.  With per-plan
        parameters bound, row g reads parameter row g.  Raises DialHipError on a context without a law."""
        import torch
        n = int(states.shape[0])
        assert tuple(states.shape) == (n, self.state_size) and tuple(actions.shape) == (n, self.nu)
        ctrl = torch.empty((n, self.nu), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_user_control(self.h, _ptr(states), _ptr(actions), n, _ptr(ctrl), _stream()), "dial_user_control")
        return ctrl

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.dial_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise DialHipError(f"{what} failed ({rc}): {self.lib.dial_last_error(self.h).decode()}")

    # ---- K6
    def env_reset(self, qpos, qvel):
        import torch
        state = torch.zeros(self.state_size, dtype=torch.float32, device=self.torch_device)
        xpos = torch.zeros((self.nbody - 1, 3), dtype=torch.float32, device=self.torch_device)
        xquat = torch.zeros((self.nbody - 1, 4), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_env_reset(self.h, _ptr(qpos), _ptr(qvel), _ptr(state), _ptr(xpos), _ptr(xquat),
                                            _stream()), "dial_env_reset")
        return state, xpos, xquat

    def env_reset_batch(self, qpos, qvel):
        """n states in one launch: qpos [n, nq], qvel [n, nv] -> packed states [n, state_size]."""
        import torch
        n = int(qpos.shape[0])
        states = torch.zeros((n, self.state_size), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_env_reset_batch(self.h, _ptr(qpos), _ptr(qvel), _ptr(states), None, None, n, _stream()),
                    "dial_env_reset_batch")
        return states

    def env_step_batch(self, states, actions):
        """M states in one launch: states [M, state_size], actions [M, nu] -> (states, xpos [M, nbody-1, 3], xquat, ctrl [M, nu])."""
        import torch
        M = int(states.shape[0])
        assert tuple(states.shape) == (M, self.state_size) and tuple(actions.shape) == (M, self.nu)
        states = states.clone()
        f32 = dict(dtype=torch.float32, device=self.torch_device)
        xpos = torch.zeros((M, self.nbody - 1, 3), **f32)
        xquat = torch.zeros((M, self.nbody - 1, 4), **f32)
        ctrl = torch.zeros((M, self.nu), **f32)
        self._check(self.lib.dial_env_step_batch(self.h, _ptr(states), _ptr(actions), _ptr(xpos), _ptr(xquat), _ptr(ctrl), M,
                                                 _stream()), "dial_env_step_batch")
        return states, xpos, xquat, ctrl

    def env_step(self, state, action):
        import torch
        state = state.clone()
        xpos = torch.zeros((self.nbody - 1, 3), dtype=torch.float32, device=self.torch_device)
        xquat = torch.zeros((self.nbody - 1, 4), dtype=torch.float32, device=self.torch_device)
        ctrl = torch.zeros(self.nu, dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_env_step(self.h, _ptr(state), _ptr(action), _ptr(xpos), _ptr(xquat), _ptr(ctrl),
                                           _stream()), "dial_env_step")
        return state, xpos, xquat, ctrl

    # ---- plant simulator (dial_plant_step; deploy/plant.py)
    def plant_step(self, states, t, plan_time, ctrl, ctrl_dt: float, sim_dt: float, K: int, flags: int, trace=None):
        """K physics steps of M plants in one launch, all in place: states [M, state_size] float32, t [M] float64 clocks,
        plan_time [M] float32, ctrl [M, T, nu] float32 (the published rows), trace [M, K, 1 + nq + nv + nu] float32 or None.
        The context's model must have timestep = sim_dt (Plant / env.make_plant build one).  A task-plugin context needs a plugin
        built with a plant (build_plugin(plant=True)); PLANT_LAW, its law at every sim step, needs one with a control law too."""
        import torch
        M = int(states.shape[0])
        assert states.dim() == 2 and states.shape[1] == self.state_size, "states: [M, state_size]"
        assert ctrl.dim() == 3 and ctrl.shape[0] == M and ctrl.shape[2] == self.nu, "ctrl: [M, T, nu]"
        assert tuple(t.shape) == (M,) and t.dtype == torch.float64 and t.is_cuda and t.is_contiguous(), "t: [M] float64 device tensor"
        assert tuple(plan_time.shape) == (M,), "plan_time: [M]"
        if trace is not None:
            assert tuple(trace.shape) == (M, int(K), 1 + self.nq + self.nv + self.nu), "trace: [M, K, 1 + nq + nv + nu]"
        self._check(self.lib.dial_plant_step(self.h, _ptr(states), t.data_ptr(), _ptr(plan_time), _ptr(ctrl), int(ctrl.shape[1]),
                                             float(ctrl_dt), float(sim_dt), int(K), int(flags), _ptr(trace), M, _stream()),
                    "dial_plant_step")

    def set_plant_disturbance(self, dist, n_events: int = 0):
        """Bind plant disturbances (dial_set_plant_disturbance): `dist` a contiguous float32 device tensor [M, plant_dist_row(nu, nv,
        n_events)] -- row m = gain[nu] | bias[nu] | n_events x { t0, t1, dv[nv] } of plant m (deploy/plant.py: disturbance_row packs
        one) -- bound as it is: the context keeps a reference, and the tensor may be rewritten in place between launches.  While bound,
        plant_step needs M == dist.shape[0] and runs the disturbed kernel.  None unbinds."""
        if dist is None:
            self._check(self.lib.dial_set_plant_disturbance(self.h, None, 0, 0), "dial_set_plant_disturbance")
            self._plant_dist = None
            return None
        n_events = int(n_events)
        row = plant_dist_row(self.nu, self.nv, n_events)
        if 0 <= n_events <= PLANT_MAX_EVENTS and (dist.dim() != 2 or int(dist.shape[1]) != row):   # (a bad n_events: the library's message)
            raise ValueError(f"plant disturbance: rows of {row} floats (2 nu + n_events (2 + nv)) are needed; got shape {tuple(dist.shape)}")
        if dist.device != self.torch_device:
            raise ValueError("plant disturbance: the tensor must be on the context's device")
        self._check(self.lib.dial_set_plant_disturbance(self.h, _ptr(dist), int(dist.shape[0]), n_events), "dial_set_plant_disturbance")
        self._plant_dist = dist
        return dist

    def set_plant_models(self, models, model_of=None):
        """Bind per-plant model constants (dial_set_plant_models): `models` a list of V compiled model dicts or DialModel structs --
        variants of this context's model with the same structure and timestep (mjcf.vary_model makes them) --, `model_of` an integer
        list [M], plant b runs models[model_of[b]] (None: V == M, one to one).  The library copies both.  While bound, plant_step
        needs M == len(model_of) and runs the per-plant-model kernel.  models None unbinds."""
        if models is None:
            self._check(self.lib.dial_set_plant_models(self.h, None, 0, None, 0), "dial_set_plant_models")
            return None
        models = list(models)
        index = plant_model_index(model_of, len(models))
        arr = (_abi.DialModel * len(models))()
        for v, m in enumerate(models):
            struct = m if isinstance(m, _abi.DialModel) else _abi.make_model(m)   # (kept alive across the copy)
            ctypes.memmove(ctypes.addressof(arr[v]), ctypes.addressof(struct), ctypes.sizeof(_abi.DialModel))
        self._check(self.lib.dial_set_plant_models(self.h, ctypes.addressof(arr), len(models), index.ctypes.data, int(index.size)),
                    "dial_set_plant_models")
        return index

    def set_plan_models(self, models, model_of=None, per: str = "plan"):
        """Bind planner models (dial_set_plan_models): `models` a list of V compiled model dicts or DialModel structs -- variants of
        this context's model with the same structure and timestep (mjcf.vary_model makes them).  per="plan": `model_of` [rows <=
        plan_cap], every rollout of plan g of a grouped launch runs models[model_of[g]] (None: one row per plan of the context's plan
        capacity, g % V); one-plan launches read row 0.  per="sample": `model_of` [Nsample + 1], rollout n of every plan runs
        models[model_of[n]], the last row is the mean trajectory's (None: n % V, the mean trajectory model 0).  The library copies
        both.  While bound, rollout / reverse_once* / reverse_once_batch* run the per-model rollout kernel; env_step*, env_reset* and
        plant_step ignore the binding.  models None unbinds.  Returns the index."""
        if models is None:
            self._check(self.lib.dial_set_plan_models(self.h, None, 0, None, 0, 0), "dial_set_plan_models")
            return None
        models = list(models)
        if per not in PLAN_MODEL_MODES:
            raise ValueError(f"plan models: per = {per!r}; 'plan' or 'sample' are allowed")
        if self.cfg is None:
            raise ValueError("plan models: the context was created without a dial_cfg (it launches no rollouts)")
        rows = self.cfg.Nsample + 1 if per == "sample" else (len(model_of) if model_of is not None else self.plan_cap)
        index = plan_model_index(model_of, len(models), rows, per)
        arr = (_abi.DialModel * len(models))()
        for v, m in enumerate(models):
            struct = m if isinstance(m, _abi.DialModel) else _abi.make_model(m)   # (kept alive across the copy)
            ctypes.memmove(ctypes.addressof(arr[v]), ctypes.addressof(struct), ctypes.sizeof(_abi.DialModel))
        self._check(self.lib.dial_set_plan_models(self.h, ctypes.addressof(arr), len(models), index.ctypes.data, int(index.size),
                                                  PLAN_MODEL_MODES[per]), "dial_set_plan_models")
        return index

    def set_plan_ensemble(self, models, hyp=None, aggregate: str = "mean", alpha: float = 1.0):
        """Bind a model ensemble (dial_set_plan_ensemble): `models` a list of V compiled model dicts or DialModel structs (variants of
        this context's model, as set_plan_models takes them), `hyp` [rows <= plan_cap][R] indices into it (a flat [R] list: shared by
        every plan of the context's plan capacity; None: all V models in order for every plan).  While bound, reverse_once* (row 0)
        and reverse_once_batch* (M <= rows plans) roll every candidate out under all R hypotheses of its plan and run the softmax
        on the per-candidate aggregate: "mean", "min" or "cvar" (the mean of the ceil(alpha R) worst; alpha in (0, 1]).  qbar / qdbar /
        xbar are the weighted means of the trajectories under hypothesis 0, the plan's nominal model.  rollout, env_step*, env_reset*
        and plant_step ignore the binding.  models None unbinds.  Returns the hypotheses bound."""
        if models is None:
            self._check(self.lib.dial_set_plan_ensemble(self.h, None, 0, None, 0, 0, 0, 0.0), "dial_set_plan_ensemble")
            self._ens_R = 0
            return None
        models = list(models)
        if aggregate not in ENSEMBLE_AGGREGATES:
            raise ValueError(f"plan ensemble: aggregate = {aggregate!r}; {sorted(ENSEMBLE_AGGREGATES)} are allowed")
        if self.cfg is None:
            raise ValueError("plan ensemble: the context was created without a dial_cfg (it launches no rollouts)")
        a = None if hyp is None else np.asarray(hyp)
        rows = a.shape[0] if a is not None and a.ndim == 2 else self.plan_cap
        index = plan_ensemble_index(hyp, len(models), rows)
        arr = (_abi.DialModel * len(models))()
        for v, m in enumerate(models):
            struct = m if isinstance(m, _abi.DialModel) else _abi.make_model(m)   # (kept alive across the copy)
            ctypes.memmove(ctypes.addressof(arr[v]), ctypes.addressof(struct), ctypes.sizeof(_abi.DialModel))
        self._check(self.lib.dial_set_plan_ensemble(self.h, ctypes.addressof(arr), len(models), index.ctypes.data, int(index.shape[0]),
                                                    int(index.shape[1]), ENSEMBLE_AGGREGATES[aggregate], float(alpha)), "dial_set_plan_ensemble")
        self._ens_R = int(index.shape[1])
        return index

    def ensemble_rewards(self, M: int):
        """The raw per-hypothesis rewards [R, M, Nsample + 1] of the last robust iteration (dial_get_ensemble_rewards): row [r, g] holds
        plan g's candidates under its hypothesis r, the mean trajectory's last."""
        import torch
        R = getattr(self, "_ens_R", 0)
        out = torch.empty((max(R, 1), int(M), self.cfg.Nsample + 1), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_get_ensemble_rewards(self.h, _ptr(out), int(M), _stream()), "dial_get_ensemble_rewards")
        return out

    def set_update_rule(self, rule, n_elite: int = 0):
        """The rule that turns a plan's rewards into weights (dial_set_update_rule): "mppi" (the softmax, the default) or "elite" with
        the elite count n_elite in 1 .. Nsample + 1 -- uniform weights on the n_elite best candidates (ties by ascending index, NaN
        last), zero on the rest; the DIAL_UPDATE_* values are taken too.  No synchronisation: launches issued afterwards use it."""
        if isinstance(rule, str):
            if rule not in UPDATE_RULES:
                raise ValueError(f"update rule {rule!r}; one of {sorted(UPDATE_RULES)}")
            rule = UPDATE_RULES[rule]
        self._check(self.lib.dial_set_update_rule(self.h, int(rule), int(n_elite)), "dial_set_update_rule")

    def weights(self, M: int = 1):
        """The weights the last iteration formed (dial_get_weights; the softmax weights under "mppi" too): [M, Nsample + 1], M the
        plans of that launch.  On a sharded context M = 1 and the first n_total + 1 entries are that launch's."""
        import torch
        out = torch.zeros((int(M), self.cfg.Nsample + 1), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_get_weights(self.h, _ptr(out), int(M), _stream()), "dial_get_weights")
        return out

    # ---- K3
    def rollout(self, state, us, want_states: bool = True):
        import torch
        B, T = us.shape[0], us.shape[1]
        assert T == self.cfg.Hsample + 1 and us.shape[2] == self.nu
        dev = self.torch_device
        rewss = torch.empty((B, T), dtype=torch.float32, device=dev)
        qss = torch.empty((B, T, self.nq), dtype=torch.float32, device=dev) if want_states else None
        qdss = torch.empty((B, T, self.nv), dtype=torch.float32, device=dev) if want_states else None
        xss = torch.empty((B, T, self.nx), dtype=torch.float32, device=dev) if want_states else None
        self._check(self.lib.dial_rollout(self.h, _ptr(state), _ptr(us), B, _ptr(rewss), _ptr(qss), _ptr(qdss),
                                          _ptr(xss), _stream()), "dial_rollout")
        return rewss, qss, qdss, xss

    # ---- K1..K4
    def _out(self, want_bars: bool):
        import torch
        cfg, dev = self.cfg, self.torch_device
        N, Hn1, T = cfg.Nsample, cfg.Hnode + 1, cfg.Hsample + 1
        f32 = dict(dtype=torch.float32, device=dev)
        return dict(Ybar=torch.empty((Hn1, self.nu), **f32), rews=torch.empty(N + 1, **f32),
                    qbar=torch.empty((T, self.nq), **f32) if want_bars else None,
                    qdbar=torch.empty((T, self.nv), **f32) if want_bars else None,
                    xbar=torch.empty((T, self.nx), **f32) if want_bars else None)

    def reverse_once(self, state, Ybar, noise_scale, eps, out=None, want_bars: bool = True):
        """want_bars=False: qbar / qdbar / xbar are None and the rollouts do not write their per-step states."""
        cfg = self.cfg
        N, Hn1 = cfg.Nsample, cfg.Hnode + 1
        assert tuple(eps.shape) == (N, Hn1, self.nu) and tuple(Ybar.shape) == (Hn1, self.nu)
        ns = int(noise_scale.numel())
        if out is None:
            out = self._out(want_bars)
        self._check(self.lib.dial_reverse_once(self.h, _ptr(state), _ptr(Ybar), _ptr(noise_scale), ns, _ptr(eps),
                                               _ptr(out["Ybar"]), _ptr(out["rews"]), _ptr(out["qbar"]),
                                               _ptr(out["qdbar"]), _ptr(out["xbar"]), _stream()), "dial_reverse_once")
        return out

    def reverse_once_rng(self, state, Ybar, noise_scale, seed: int, counter: int, out=None, want_bars: bool = True):
        """reverse_once with the noise generated inside the rollout kernel (Philox keyed by seed / counter)."""
        if out is None:
            out = self._out(want_bars)
        self._check(self.lib.dial_reverse_once_rng(self.h, _ptr(state), _ptr(Ybar), _ptr(noise_scale),
                                                   int(noise_scale.numel()), int(seed), int(counter), _ptr(out["Ybar"]),
                                                   _ptr(out["rews"]), _ptr(out["qbar"]), _ptr(out["qdbar"]),
                                                   _ptr(out["xbar"]), _stream()), "dial_reverse_once_rng")
        return out

    # ---- grouped planning: M plans in one launch (dial_reverse_once_batch; plan g = row g of every argument)
    def _out_batch(self, M: int, want_bars: bool):
        import torch
        cfg = self.cfg
        N, Hn1, T = cfg.Nsample, cfg.Hnode + 1, cfg.Hsample + 1
        f32 = dict(dtype=torch.float32, device=self.torch_device)
        return dict(Ybar=torch.empty((M, Hn1, self.nu), **f32), rews=torch.empty((M, N + 1), **f32),
                    qbar=torch.empty((M, T, self.nq), **f32) if want_bars else None,
                    qdbar=torch.empty((M, T, self.nv), **f32) if want_bars else None,
                    xbar=torch.empty((M, T, self.nx), **f32) if want_bars else None)

    def reverse_once_batch(self, states, Ybars, noise_scales, eps, out=None, want_bars: bool = True):
        """states [M, state_size], Ybars [M, Hn1, nu], noise_scales [M, ns], eps [M, N, Hn1, nu] -> dict of [M, ...] outputs."""
        M = int(states.shape[0])
        N, Hn1 = self.cfg.Nsample, self.cfg.Hnode + 1
        assert tuple(eps.shape) == (M, N, Hn1, self.nu) and tuple(Ybars.shape) == (M, Hn1, self.nu)
        if out is None:
            out = self._out_batch(M, want_bars)
        self._check(self.lib.dial_reverse_once_batch(self.h, _ptr(states), _ptr(Ybars), _ptr(noise_scales),
                                                     int(noise_scales.shape[-1]), _ptr(eps), M, _ptr(out["Ybar"]), _ptr(out["rews"]),
                                                     _ptr(out["qbar"]), _ptr(out["qdbar"]), _ptr(out["xbar"]), _stream()),
                    "dial_reverse_once_batch")
        return out

    def reverse_once_batch_rng(self, states, Ybars, noise_scales, seed: int, counter: int, out=None, want_bars: bool = True):
        """reverse_once_batch with in-kernel noise: plan g draws rows [g N, (g + 1) N) of rng_fill(seed, counter, 0, M N)."""
        M = int(states.shape[0])
        if out is None:
            out = self._out_batch(M, want_bars)
        self._check(self.lib.dial_reverse_once_batch_rng(self.h, _ptr(states), _ptr(Ybars), _ptr(noise_scales),
                                                         int(noise_scales.shape[-1]), int(seed), int(counter), M, _ptr(out["Ybar"]),
                                                         _ptr(out["rews"]), _ptr(out["qbar"]), _ptr(out["qdbar"]), _ptr(out["xbar"]),
                                                         _stream()), "dial_reverse_once_batch_rng")
        return out

    def shift_batch(self, Y):
        """Y [M, Hn1, nu] -> shifted copy (one launch)."""
        Y = Y.clone()
        self._check(self.lib.dial_shift_batch(self.h, _ptr(Y), int(Y.shape[0]), _stream()), "dial_shift_batch")
        return Y

    def rng_fill(self, seed: int, counter: int, n_begin: int, n_count: int):
        import torch
        eps = torch.empty((n_count, self.cfg.Hnode + 1, self.nu), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_rng_fill(self.h, int(seed), int(counter), n_begin, n_count, _ptr(eps), _stream()),
                    "dial_rng_fill")
        return eps

    def shard_rollout_rng(self, state, Ybar, noise_scale, seed, counter, n_begin, n_local, with_mean, rews_local):
        self._check(self.lib.dial_shard_rollout_rng(self.h, _ptr(state), _ptr(Ybar), _ptr(noise_scale),
                                                    int(noise_scale.numel()), int(seed), int(counter), n_begin, n_local,
                                                    int(with_mean), _ptr(rews_local), _stream()), "dial_shard_rollout_rng")

    def shard_rollout(self, state, Ybar, noise_scale, eps_local, n_local: int, with_mean: bool, rews_local):
        ns = int(noise_scale.numel())
        self._check(self.lib.dial_shard_rollout(self.h, _ptr(state), _ptr(Ybar), _ptr(noise_scale), ns,
                                                _ptr(eps_local) if n_local > 0 else None, n_local, int(with_mean),
                                                _ptr(rews_local), _stream()), "dial_shard_rollout")

    def shard_reduce(self, rews_all, n_total: int, n_begin: int, n_local: int, include_mean: bool, packed_out):
        self._check(self.lib.dial_shard_reduce(self.h, _ptr(rews_all), n_total, n_begin, n_local, int(include_mean),
                                               _ptr(packed_out), _stream()), "dial_shard_reduce")

    def shard_ybar(self, rews_all, n_total: int, eps_all, Ybar, noise_scale, Ybar_out):
        ns = int(noise_scale.numel())
        self._check(self.lib.dial_shard_ybar(self.h, _ptr(rews_all), n_total, _ptr(eps_all), _ptr(Ybar), _ptr(noise_scale),
                                             ns, _ptr(Ybar_out), _stream()), "dial_shard_ybar")

    def shard_ybar_rng(self, rews_all, n_total: int, seed: int, counter: int, Ybar, noise_scale, Ybar_out):
        self._check(self.lib.dial_shard_ybar_rng(self.h, _ptr(rews_all), n_total, int(seed), int(counter), _ptr(Ybar),
                                                 _ptr(noise_scale), int(noise_scale.numel()), _ptr(Ybar_out), _stream()),
                    "dial_shard_ybar_rng")

    def shard_pack_rewards(self, gathered, world: int, per: int, n_total: int, rews_all):
        self._check(self.lib.dial_shard_pack_rewards(self.h, _ptr(gathered), world, per, n_total, _ptr(rews_all), _stream()),
                    "dial_shard_pack_rewards")

    # phase B straight from the all-gather's receive buffer (the packing step runs inside the weights kernel; rews_all receives the
    # packed rewards): two launches per iteration instead of four
    def shard_ybar_gathered(self, gathered, world: int, per: int, n_total: int, eps_all, Ybar, noise_scale, rews_all, Ybar_out):
        self._check(self.lib.dial_shard_ybar_gathered(self.h, _ptr(gathered), world, per, n_total, _ptr(eps_all), _ptr(Ybar), _ptr(noise_scale),
                                                      int(noise_scale.numel()), _ptr(rews_all), _ptr(Ybar_out), _stream()), "dial_shard_ybar_gathered")

    def shard_ybar_gathered_rng(self, gathered, world: int, per: int, n_total: int, seed: int, counter: int, Ybar, noise_scale, rews_all, Ybar_out):
        self._check(self.lib.dial_shard_ybar_gathered_rng(self.h, _ptr(gathered), world, per, n_total, int(seed), int(counter), _ptr(Ybar),
                                                          _ptr(noise_scale), int(noise_scale.numel()), _ptr(rews_all), _ptr(Ybar_out), _stream()),
                    "dial_shard_ybar_gathered_rng")

    def shard_reduce_gathered(self, gathered, world: int, per: int, n_total: int, n_begin: int, n_local: int, include_mean: bool, rews_all, packed_out):
        self._check(self.lib.dial_shard_reduce_gathered(self.h, _ptr(gathered), world, per, n_total, n_begin, n_local, int(include_mean),
                                                        _ptr(rews_all), _ptr(packed_out), _stream()), "dial_shard_reduce_gathered")

    def packed_size(self) -> int:
        T, Hn1 = self.cfg.Hsample + 1, self.cfg.Hnode + 1
        return Hn1 * self.nu + T * (self.nq + self.nv + self.nx)

    # ---- K5
    def shift(self, Y):
        Y = Y.clone()
        self._check(self.lib.dial_shift(self.h, _ptr(Y), _stream()), "dial_shift")
        return Y

    def status(self):
        """Raise if an earlier asynchronous launch gave up (sticky; costs no synchronisation)."""
        self._check(self.lib.dial_status(self.h), "dial_status")

    # ---- measurement
    def set_timing(self, enable: bool):
        self._check(self.lib.dial_set_timing(self.h, int(enable)), "dial_set_timing")

    def rollout_ms(self):
        tot, n = ctypes.c_double(0), ctypes.c_int(0)
        self._check(self.lib.dial_get_rollout_ms(self.h, ctypes.byref(tot), ctypes.byref(n)), "dial_get_rollout_ms")
        return tot.value, n.value

    def set_state_trace(self, rows: Optional[int]):
        """Diagnostics (parity tests): allocate a [rows, T, state_size] tensor into which every following rollout launch
        writes the packed state after each env.step; rows=None switches the trace off.  Returns the tensor."""
        import torch
        if rows is None:
            self._check(self.lib.dial_set_state_trace(self.h, None, 0), "dial_set_state_trace")
            self._trace = None
            return None
        self._trace = torch.zeros((int(rows), self.cfg.Hsample + 1, self.state_size), dtype=torch.float32, device=self.torch_device)
        self._check(self.lib.dial_set_state_trace(self.h, _ptr(self._trace), int(rows)), "dial_set_state_trace")
        return self._trace

    LAUNCH_FIELDS = ("inst", "wpb", "blocks", "queue", "relay", "mean_inline", "slice_pieces", "split", "pair", "trace", "con_cap", "rollouts",
                     "defer_reward")

    def debug_last_launch(self) -> dict:
        """What this context's most recent rollout launch did (dial_debug_last_launch; tests assert the path they target): kernel
        instantiation `inst` (0 = the capacity-dimension kernel, DimsMax), wavefronts per workgroup, grid workgroups (0: the call returned
        before launching), and 0 / 1 or counts for the rollout queue, the mean-trajectory relay, the interleaved mean trajectory, the
        time-slice pieces, the split launch, the Go2 pair kernel, the state-trace instantiation; `con_cap` the overflow cap in effect
        (0: no overflow areas), `rollouts` the batch, `defer_reward` 1 when the Go2 walk's kernel that evaluates the step rewards once per
        rollout ran (dial_options.no_defer_reward)."""
        buf = (ctypes.c_int * len(self.LAUNCH_FIELDS))()
        n = self.lib.dial_debug_last_launch(self.h, buf, len(buf))
        if n != len(self.LAUNCH_FIELDS):
            raise DialHipError(f"dial_debug_last_launch: {n} fields, this wrapper knows {len(self.LAUNCH_FIELDS)}")
        return dict(zip(self.LAUNCH_FIELDS, buf))

    def debug_scratch(self):
        """Host copies of the scratch tensors of the last reverse_once (tests only)."""
        import numpy as np
        import torch
        ptrs = [ctypes.c_void_p() for _ in range(6)]
        self._check(self.lib.dial_debug_scratch(self.h, *[ctypes.byref(p) for p in ptrs]), "dial_debug_scratch")
        cfg = self.cfg
        B, T, Hn1 = cfg.Nsample + 1, cfg.Hsample + 1, cfg.Hnode + 1
        shapes = [(B, Hn1, self.nu), (B, T), (B, T, self.nq), (B, T, self.nv), (B, T, self.nx), (B,)]
        names = ["Y0s", "rewss", "qss", "qdss", "xss", "weights"]
        torch.cuda.synchronize()
        hip = ctypes.CDLL("libamdhip64.so")
        out = {}
        for name, p, shp in zip(names, ptrs, shapes):
            host = np.empty(shp, np.float32)
            rc = hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), p, ctypes.c_size_t(host.nbytes), ctypes.c_int(2))
            if rc != 0:
                raise DialHipError(f"hipMemcpy of scratch {name} failed ({rc})")
            out[name] = host
        return out
