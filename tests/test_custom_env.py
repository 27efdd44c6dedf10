"""Custom environments without a GPU: building task plugins (hipcc cross-compiles), their cache, their refusals, the C ABI
surface and the planner's loud failure on a GPU-less host."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX_MOD = "dial_mpc_amd.examples.custom_env.go2_height_walk"
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module", autouse=True)
def _registry():
    """The example registers itself in the env registry; this module's tests leave the registry as they found it."""
    import importlib
    import dial_mpc_amd.envs as dial_envs
    saved = dict(dial_envs._envs), dict(dial_envs._configs)
    mod = sys.modules.get(EX_MOD)
    if mod is None:
        importlib.import_module(EX_MOD)
    else:
        importlib.reload(mod)   # (registered again: an earlier module's teardown removed it)
    yield
    dial_envs._envs.clear()
    dial_envs._envs.update(saved[0])
    dial_envs._configs.clear()
    dial_envs._configs.update(saved[1])


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("plugins"))
    old = os.environ.get("DIAL_PLUGIN_CACHE")
    os.environ["DIAL_PLUGIN_CACHE"] = d
    yield d
    if old is None:
        os.environ.pop("DIAL_PLUGIN_CACHE", None)
    else:
        os.environ["DIAL_PLUGIN_CACHE"] = old


@pytest.fixture(scope="module")
def env():
    import importlib
    import yaml
    importlib.import_module(EX_MOD)
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk.yaml")))
    return load_dial_and_env(d)[2]


@pytest.fixture(scope="module")
def built(cache, env):
    from dial_mpc_amd.plugin import build_plugin
    return build_plugin(env.sys.model, env.reward_source())


def _kernels(so, outdir):
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    import disasm_lib
    cos = disasm_lib.code_objects(so, outdir)
    names = []
    for co in cos:
        names += re.findall(r"<(_Z\w+)>:", open(_disasm(co)).read())
    return cos, names


def _disasm(co):
    s = co[:-2] + ".s"
    with open(s, "w") as f:
        subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], stdout=f)
    return s


def test_build_plugin_produces_a_gfx950_plugin(built, tmp_path):
    assert os.path.exists(built)
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", built], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+dial_plugin_ops_v1$", syms, flags=re.M), syms
    cos, names = _kernels(built, str(tmp_path))
    assert len(cos) == 1
    joined = "\n".join(names)
    for k in ("rollout_kernel", "env_step_kernel", "env_reset_kernel"):
        assert re.search(k + r"I8DimsUser", joined), (k, names)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), _disasm(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_cache_reuse_and_new_key(built, env):
    from dial_mpc_amd.plugin import build_plugin
    st = os.stat(built)
    again = build_plugin(env.sys.model, env.reward_source())
    assert again == built and os.stat(again).st_mtime_ns == st.st_mtime_ns and os.stat(again).st_ino == st.st_ino
    changed = build_plugin(env.sys.model, env.reward_source() + "\n// another reward\n")
    assert changed != built and os.path.exists(changed)


def test_reward_syntax_error_carries_hipcc_message(cache, env):
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import build_plugin
    bad = "DIAL_DEV float dial_user_reward(const DialRewardIn& in, const float* p, float* u) { return in.qvel[0] +; }\n"
    with pytest.raises(DialHipError, match=r"hipcc failed[\s\S]*error:"):
        build_plugin(env.sys.model, bad)


def test_refuses_elliptic_cones_and_full_impedance_table(cache, env):
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.envs.base_env import load_model
    from dial_mpc_amd.plugin import build_plugin
    with pytest.raises(DialHipError, match="cones"):
        build_plugin(load_model("wonik_allegro", "scene_left.xml"), env.reward_source())
    m = dict(env.sys.model)
    ref = np.array(m["con_solref"], dtype=np.float64).copy()
    jr = np.array(m["jnt_solref"], dtype=np.float64).copy()
    for c in range(ref.shape[0]):
        ref[c, 0] = 0.02 + 0.001 * c
    for j in range(jr.shape[0]):
        jr[j, 0] = 0.03 + 0.001 * j
    m["con_solref"], m["jnt_solref"] = ref, jr
    with pytest.raises(DialHipError, match="impedance table"):
        build_plugin(m, env.reward_source())


def test_generated_dims_match_the_model(env):
    from dial_mpc_amd import _abi
    from dial_mpc_amd.plugin import dims_header, plugin_dims
    model = env.make_model()
    dims = plugin_dims(env.sys.model)
    assert dims == plugin_dims(model)
    for k, v in dims.items():
        assert getattr(model, k) == v
    hdr = dims_header(env.sys.model)
    assert f"#define DIAL_PLUGIN_NQ {model.nq}\n" in hdr and f"#define DIAL_PLUGIN_NC {model.ncon}\n" in hdr
    assert _abi.MACROS["DIAL_TASK_USER"] == 7 and env.make_task().kind == 7


def test_c_abi_surface():
    from dial_mpc_amd import _abi, _lib
    text = open(_abi.HEADER).read()
    assert re.search(r"int dial_create_plugin\(dial_ctx\*\* out,", text) and re.search(r"int dial_set_user_params\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dial_create_plugin") and hasattr(lib, "dial_set_user_params")
    M = _abi.MACROS
    assert M["DIAL_INFO_LAST_CTRL"] + M["DIAL_MAX_U"] <= M["DIAL_INFO_USER"]
    assert M["DIAL_INFO_USER"] + M["DIAL_INFO_USER_N"] <= M["DIAL_INFO_N"]


def test_planner_without_gpu_fails_loudly(cache, env):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import yaml
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.core.dial_core import MBDPI, load_dial_and_env
    d = yaml.safe_load(open(os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk.yaml")))
    dc, _, e = load_dial_and_env(d)
    with pytest.raises(DialHipError):
        MBDPI(dc, e)
