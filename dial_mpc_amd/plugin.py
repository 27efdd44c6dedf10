"""Task plugins: a user reward -- and optionally a user control law -- compiled, for one model, into the rollout / env.step /
env.reset kernels (HIP, gfx950).

``build_plugin(model, reward_src)`` writes the model's dimensions and the reward source next to ``csrc/plugin.hip``'s object,
compiles that one translation unit with the product flags (``_lib._COMMON + _FAST``) and links a shared library that
``libdialhip.so`` loads (``dial_create_plugin``; ``_lib.Context(..., plugin=path)``).  The reward's contract is in
``csrc/user_reward.h``.  ``control_src`` adds a control law (contract: ``csrc/user_control.h``) in place of BaseEnv's act2joint /
PD law; such a plugin carries one more kernel (``user_control_kernel``) and exports a second symbol (``CTRL_SYMBOL``).  Every plugin
exports ``TABLE_SYMBOL``, the host function behind the reference table (``dial_set_user_table``; no kernel of its own).
``plant=True`` adds the plant simulator's kernel at the model's dimensions (``plant_kernel`` of ``csrc/plant_kernel.h``,
the built-in families' kernel, behind the table of ``csrc/plant_plugin.h``;
``dial_plant_step`` on the plugin's contexts) and a fourth symbol (``PLANT_SYMBOL``); a plugin built without it is unchanged.
``plant_disturbance=True`` (implies ``plant=True``) adds the disturbed plant kernel (``plant_dist_kernel`` of
``csrc/plant_dist_kernel.h``; ``dial_set_plant_disturbance``) and a fifth symbol (``PLANT_DIST_SYMBOL``).
``plant_models=True`` (implies ``plant=True``) adds the plant kernel with per-plant model constants (``plant_var_kernel`` of
``csrc/plant_var_kernel.h``; ``dial_set_plant_models``) and a sixth symbol (``PLANT_VAR_SYMBOL``).
``plan_models=True`` adds the rollout kernel with per-plan / per-sample model constants (``rollout_var_kernel`` of
``csrc/plan_var_kernel.h``; ``dial_set_plan_models``) and a seventh symbol (``PLAN_VAR_SYMBOL``).
``plan_ensemble=True`` adds the ensemble rollout kernel (``rollout_ens_kernel`` of ``csrc/plan_ens_kernel.h``;
``dial_set_plan_ensemble``) and an eighth symbol (``PLAN_ENS_SYMBOL``).  Results are cached under ``build/plugins/<key>/`` (``DIAL_PLUGIN_CACHE`` overrides the root); the key
hashes every csrc source, ``include/dial_mpc.h``, the reward, the control law (when there is one), the dimensions, the flags and ``hipcc --version``.  hipcc
cross-compiles, so building needs no GPU.
"""
from __future__ import annotations

import glob
import hashlib
import os
import re
import shutil
import subprocess
from typing import Any, Dict, Optional, Sequence, Union

import numpy as np

from dial_mpc_amd import _abi
from dial_mpc_amd._lib import _COMMON, _CSRC, _FAST, DialHipError

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "dial_plugin_ops_v1"
CTRL_SYMBOL = "dial_plugin_ctrl_v1"   # exported only by a plugin built with a control law
TABLE_SYMBOL = "dial_plugin_table_v1"  # exported by every plugin: the reference table's host function (dial_set_user_table)
PLANT_SYMBOL = "dial_plugin_plant_v1"  # exported only by a plugin built with plant=True: the plant kernel's table (dial_plant_step)
PLANT_DIST_SYMBOL = "dial_plugin_plant_dist_v1"  # only with plant_disturbance=True: the disturbed plant kernel's table (dial_set_plant_disturbance)
PLANT_VAR_SYMBOL = "dial_plugin_plant_var_v1"  # only with plant_models=True: the per-plant-model plant kernel's table (dial_set_plant_models)
PLAN_VAR_SYMBOL = "dial_plugin_plan_var_v1"  # only with plan_models=True: the per-model rollout kernel's table (dial_set_plan_models)
PLAN_ENS_SYMBOL = "dial_plugin_plan_ens_v1"  # only with plan_ensemble=True: the ensemble rollout kernel's table (dial_set_plan_ensemble)
DIM_NAMES = ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "nsite", "ncon", "nlim", "nfri")
_DIM_MACROS = ("NQ", "NV", "NU", "NB", "NJ", "NG", "NS", "NC", "NL", "NFRI")


def _kbi_rows_capacity() -> int:
    m = re.search(r"#define\s+DIAL_KBI_ROWS\s+(\d+)", open(os.path.join(_CSRC, "cmodel.h")).read())
    return int(m.group(1))


def _model_dict(model: Union[Dict[str, Any], "_abi.DialModel"]) -> Dict[str, Any]:
    if isinstance(model, dict):
        return model
    return {k: (_abi.as_numpy(model, k) if _abi.DialModel._meta[k][0] else getattr(model, k)) for k in _abi.DialModel._meta}


def plugin_dims(model) -> Dict[str, int]:
    """The compile-time dimensions a plugin for `model` (a compiled model dict or a DialModel) is instantiated with."""
    d = _model_dict(model)
    return {k: int(np.asarray(d.get(k, 0))) for k in DIM_NAMES}


def kbi_unique_rows(model) -> int:
    """Distinct (solref, solimp) rows among the limit rows, contacts and dry-friction rows (csrc/derived.h: kbi_unique_rows)."""
    d = _model_dict(model)
    rows = set()
    f32 = lambda a: tuple(np.asarray(a, dtype=np.float32).ravel().tolist())   # noqa: E731

    def add(ref, imp):
        rows.add(f32(ref)[:2] + f32(imp)[:5])
    for l in range(int(d["nlim"])):
        j = int(np.asarray(d["lim_jnt"])[l])
        add(np.asarray(d["jnt_solref"])[j], np.asarray(d["jnt_solimp"])[j])
    for c in range(int(d["ncon"])):
        add(np.asarray(d["con_solref"])[c], np.asarray(d["con_solimp"])[c])
    for q in range(int(d.get("nfri", 0))):
        add(np.asarray(d["fri_solref"])[q], np.asarray(d["fri_solimp"])[q])
    return len(rows)


def check_topology(model) -> None:
    """Raise DialHipError for the tree shapes dial_create answers with DIAL_ERR_UNSUPPORTED (csrc/derived.h: dial_build_derived),
    with the body or the actuators it is about: a root-to-body path of more than 12 dofs, two actuators on one dof."""
    d = _model_dict(model)
    nb, nu = int(d["nbody"]), int(d["nu"])
    parent, dofnum = np.asarray(d["body_parent"]).ravel(), np.asarray(d["body_dofnum"]).ravel()
    names = d.get("names", {}) if isinstance(d, dict) else {}
    for b in range(1, nb):
        n, bb = 0, b
        while bb > 0:
            n += int(dofnum[bb])
            bb = int(parent[bb])
        if n > 12:
            who = repr(names["body"][b]) if names.get("body") else str(b)
            raise DialHipError(f"body {who} is moved by {n} dofs between the world and itself; the kernels' ancestor lists hold 12 "
                               "(a free joint counts 6): shorten the chain or weld a joint")
    seen: Dict[int, int] = {}
    for a in range(nu):
        dof = int(np.asarray(d["act_dofadr"]).ravel()[a])
        if dof in seen:
            who = [repr(names["actuator"][k]) if names.get("actuator") else str(k) for k in (seen[dof], a)]
            raise DialHipError(f"actuators {who[0]} and {who[1]} both drive dof {dof}; the kernels take one actuator per dof: merge "
                               "them into one actuator")
        seen[dof] = a


def _box_constants() -> tuple:
    """(DIAL_BOX_POLY_WORDS, DIAL_BOX_PARK_DIST) of csrc/box_collide.h."""
    text = open(os.path.join(_CSRC, "box_collide.h")).read()
    words = re.search(r"#define\s+DIAL_BOX_POLY_WORDS\s+(\d+)", text)
    park = re.search(r"#define\s+DIAL_BOX_PARK_DIST\s+([0-9.eE+-]+)f", text)
    return int(words.group(1)), float(np.float32(park.group(1)))


def check_box_contacts(model) -> None:
    """Raise DialHipError for the two box conditions dial_create answers with DIAL_ERR_UNSUPPORTED: more box-box candidates than the
    polygon scratch holds (their clipping polygons live in the dead velocity temporaries, 6 nv + 12 nbody words), and a box contact
    whose margin reaches the distance beyond which the box narrow phases park a candidate."""
    d = _model_dict(model)
    ncon = int(d["ncon"])
    if not ncon:
        return
    kind = np.asarray(d["con_kind"]).ravel()[:ncon]
    words, park = _box_constants()
    nbb = int((kind == _abi.MACROS["DIAL_CON_BOX_BOX"]).sum())
    have = 6 * int(d["nv"]) + 12 * int(d["nbody"])
    if nbb * words > have:
        raise DialHipError(f"the model has {nbb} box-box candidate contacts (four per pair of box geoms); their clipping polygons need "
                           f"{nbb * words} words of the kernels' polygon scratch ({words} each) and the model has {have} "
                           "(6 nv + 12 nbody): exclude a box pair (<contact><exclude>, contype / conaffinity) -- dial_create refuses "
                           "the model (too many box-box candidate contacts for the polygon scratch)")
    margin = np.asarray(d["con_margin"]).ravel()[:ncon]
    names = d.get("names", {}) if isinstance(d, dict) else {}
    for c in range(ncon):
        if kind[c] >= _abi.MACROS["DIAL_CON_PLANE_BOX"] and not np.float32(margin[c]) < np.float32(park):
            g = [int(np.asarray(d[k]).ravel()[c]) for k in ("con_geom1", "con_geom2")]
            who = [repr(names["geom"][k]) if names.get("geom") and k < len(names["geom"]) else str(k) for k in g]
            raise DialHipError(f"the contact of geoms {who[0]} and {who[1]} has margin {float(margin[c]):g} m; box contacts need margin "
                               f"< {park:g} m (DIAL_BOX_PARK_DIST: the box narrow phases park candidates that are further apart)")


def check_model(model) -> None:
    """Raise DialHipError when a task plugin cannot serve `model` (csrc/plugin_ops.h: PluginOps::check)."""
    d = _model_dict(model)
    if int(d.get("cone", 0)) != _abi.MACROS["DIAL_CONE_PYRAMIDAL"]:
        raise DialHipError("task plugins support pyramidal friction cones only: the model uses elliptic cones")
    if int(d.get("eulerdamp", 0)):
        raise DialHipError("the model integrates joint damping implicitly (MuJoCo's default whenever a joint has damping > 0); the "
                           "pyramidal kernels integrate it explicitly: add <option><flag eulerdamp=\"disable\"/></option> to the MJCF "
                           "(dial_create refuses eulerdamp on every pyramidal model)")
    check_topology(d)
    check_box_contacts(d)
    n, cap = kbi_unique_rows(d), _kbi_rows_capacity()
    if n > cap:
        raise DialHipError(f"the model has {n} distinct (solref, solimp) sets; the impedance table of a plugin holds "
                           f"DIAL_KBI_ROWS = {cap}")


def dims_header(model) -> str:
    dims = plugin_dims(model)
    return "".join(f"#define DIAL_PLUGIN_{m} {dims[k]}\n" for k, m in zip(DIM_NAMES, _DIM_MACROS))


def _read_reward(reward_src: str) -> str:
    if "\n" not in reward_src and reward_src.endswith(".hip") and os.path.isfile(reward_src):
        return open(reward_src).read()
    return reward_src


def _hipcc() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def cache_root() -> str:
    return os.environ.get("DIAL_PLUGIN_CACHE", os.path.join(_ROOT, "build", "plugins"))


def plugin_key(model, reward_src: str, flags: Sequence[str], control_src: Optional[str] = None) -> str:
    h = hashlib.sha256()
    for p in sorted(glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(_CSRC, "*.hip"))) + [_abi.HEADER]:
        h.update(os.path.basename(p).encode() + b"\0" + open(p, "rb").read() + b"\0")
    h.update(_read_reward(reward_src).encode() + b"\0")
    if control_src is not None:
        h.update(b"control\0" + _read_reward(control_src).encode() + b"\0")
    h.update(dims_header(model).encode() + b"\0")
    h.update(" ".join(flags).encode() + b"\0")
    h.update(subprocess.run([_hipcc(), "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout.encode())
    return h.hexdigest()


def build_plugin(model, reward_src: str, flags: Optional[Sequence[str]] = None, verbose: bool = False,
                 control_src: Optional[str] = None, plant: bool = False, plant_disturbance: bool = False,
                 plant_models: bool = False, plan_models: bool = False, plan_ensemble: bool = False) -> str:
    """Compile (or find in the cache) the task plugin of `model` with the reward `reward_src` (HIP source text, or the path of a
    .hip file) and, optionally, the control law `control_src` (the same two forms) -> path of the shared library.  plant=True:
    the plugin also carries the plant simulator's kernel (-DDIAL_PLUGIN_PLANT=1; the define is one of the flags the cache key
    hashes, so it is another library than the plugin without it).  plant_disturbance=True implies plant=True and adds the disturbed
    plant kernel (-DDIAL_PLUGIN_PLANT_DIST=1 after it: csrc/plant_dist_kernel.h, one kernel and one symbol more, again another library;
    the plugins built with plant=True or with neither keep their flags and keys).  plant_models=True implies plant=True too and adds
    the plant kernel with per-plant model constants (-DDIAL_PLUGIN_PLANT_VAR=1, last: csrc/plant_var_kernel.h, one kernel and one symbol
    more; it combines with plant_disturbance=True, and the plugins built without it keep their flags and keys).  plan_models=True adds the
    rollout kernel with per-plan / per-sample model constants (-DDIAL_PLUGIN_PLAN_VAR=1, after every other define:
    csrc/plan_var_kernel.h, dial_set_plan_models; one kernel and one symbol more).  It implies nothing and combines with plant=,
    plant_disturbance= and plant_models=; the plugins built without it keep their flags and keys.  plan_ensemble=True adds the ensemble
    rollout kernel (-DDIAL_PLUGIN_PLAN_ENS=1, after every other define: csrc/plan_ens_kernel.h, dial_set_plan_ensemble; one kernel and
    one symbol more) in the same way: it implies nothing, combines with the others and leaves their flags and keys alone.  A compile error in either source raises DialHipError with
    hipcc's own message."""
    import fcntl
    check_model(model)
    flags = list(_COMMON + _FAST if flags is None else flags)
    if plant or plant_disturbance or plant_models:
        flags.append("-DDIAL_PLUGIN_PLANT=1")
    if plant_disturbance:
        flags.append("-DDIAL_PLUGIN_PLANT_DIST=1")
    if plant_models:
        flags.append("-DDIAL_PLUGIN_PLANT_VAR=1")
    if plan_models:
        flags.append("-DDIAL_PLUGIN_PLAN_VAR=1")
    if plan_ensemble:
        flags.append("-DDIAL_PLUGIN_PLAN_ENS=1")
    reward = _read_reward(reward_src)
    control = None if control_src is None else _read_reward(control_src)
    key = plugin_key(model, reward, flags, control)[:24]
    root = cache_root()
    out_dir = os.path.join(root, key)
    out = os.path.join(out_dir, "libdialplugin.so")
    if os.path.exists(out):
        return out
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, key + ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)   # one builder per key (processes that race find the finished library)
        try:
            if os.path.exists(out):
                return out
            work = os.path.join(root, f"tmp_{key}_{os.getpid()}")
            os.makedirs(work, exist_ok=True)
            try:
                with open(os.path.join(work, "dial_plugin_dims.h"), "w") as f:
                    f.write("// generated by dial_mpc_amd/plugin.py: the model's compile-time dimensions\n" + dims_header(model))
                with open(os.path.join(work, "dial_user_reward.hip"), "w") as f:
                    f.write(reward)
                generated = ["dial_plugin_dims.h", "dial_user_reward.hip"]
                defs = []
                if control is not None:
                    with open(os.path.join(work, "dial_user_control.hip"), "w") as f:
                        f.write(control)
                    generated.append("dial_user_control.hip")
                    defs = ["-DDIAL_PLUGIN_USER_CTRL=1"]
                obj = os.path.join(work, "plugin.o")
                cmd = [_hipcc()] + flags + defs + ["-I", work, "-c", "-o", obj, os.path.join(_CSRC, "plugin.hip")]
                if verbose:
                    print(" ".join(cmd))
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if r.returncode != 0:
                    raise DialHipError(f"hipcc failed ({r.returncode}) on the task plugin:\n{r.stdout[-6000:]}")
                so = os.path.join(work, "libdialplugin.so")
                r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj],
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                if r.returncode != 0:
                    raise DialHipError(f"linking the task plugin failed ({r.returncode}):\n{r.stdout[-4000:]}")
                os.makedirs(out_dir, exist_ok=True)
                for name in generated:   # (kept beside the library: what it was built from)
                    shutil.copy(os.path.join(work, name), os.path.join(out_dir, name))
                os.replace(so, out)
                return out
            finally:
                shutil.rmtree(work, ignore_errors=True)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
