"""Per-plan task parameters without a GPU: the C ABI surface, the plugin ABI version of a plugin built from the current sources, the
Python-side validation (rows, field names, the closed-loop driver's --env-param) and cross-compiled plugins."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX_MOD = "dial_mpc_amd.examples.custom_env.go2_height_walk"
EX_YAML = os.path.join(ROOT, "dial_mpc_amd", "examples", "custom_env", "go2_height_walk.yaml")


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
        importlib.reload(mod)
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
    from dial_mpc_amd.core.dial_core import load_dial_and_env
    return load_dial_and_env(yaml.safe_load(open(EX_YAML)))[2]


def _abi_version():
    m = re.search(r"#define\s+DIAL_PLUGIN_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "dial_mpc_amd", "csrc", "plugin_ops.h")).read())
    return int(m.group(1))


def test_c_abi_surface():
    from dial_mpc_amd import _abi, _lib
    text = open(_abi.HEADER).read()
    assert re.search(r"int dial_set_plan_params\(dial_ctx\* ctx, const float\* params, int rows\);", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "dial_set_plan_params") and "dial_set_plan_params" in _lib.EXPORTED
    sizes = [ctypes.c_int() for _ in range(3)]
    assert lib.dial_abi_sizes(*[ctypes.byref(s) for s in sizes]) == 0
    assert [s.value for s in sizes] == [ctypes.sizeof(_abi.DialModel), ctypes.sizeof(_abi.DialTask), ctypes.sizeof(_abi.DialCfg)]


def test_plugin_reports_the_new_abi_version(cache, env):
    """A plugin built from the current sources carries DIAL_PLUGIN_ABI_VERSION (2: per-plan parameters), which the library checks."""
    from dial_mpc_amd.plugin import SYMBOL, build_plugin
    assert _abi_version() == 2
    so = build_plugin(env.sys.model, env.reward_source())
    h = ctypes.CDLL(so, mode=ctypes.RTLD_LOCAL)
    entry = getattr(h, SYMBOL)
    entry.restype = ctypes.POINTER(ctypes.c_int)
    assert entry()[0] == 2   # (abi_version: the table's first field)


def test_plugins_cross_compile(cache, env):
    """hipcc builds the Go2 example's plugin and the probe plugin of the plugin tests; the env.step kernel takes the rows' pointer."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import disasm_lib
    from plugin_cases import build_matrix
    from dial_mpc_amd.plugin import build_plugin
    paths = [build_plugin(env.sys.model, env.reward_source()), build_matrix(["go2"], jobs=1)["go2"]]
    for so in paths:
        names = []
        for co in disasm_lib.code_objects(so, os.path.join(cache, "isa_" + os.path.basename(os.path.dirname(so)))):
            names += [k["name"] for k in disasm_lib.kernel_notes(co)]
        step = [_demangle(n) for n in names if "env_step_kernel" in n]
        assert len(step) == 1, step
        params = _params(step[0])   # (gm, tg, state, action, xpos_out, xquat_out, ctrl_out, plan_params)
        assert len(params) == 8 and params[-1] == "float const*", step
        assert sum("rollout_kernel" in n for n in names) == 3


def _params(sig):
    """Parameter types of a demangled function signature (commas inside template arguments do not split)."""
    depth, start, out = 0, None, []
    for i, ch in enumerate(sig):
        if ch in "<(":
            if ch == "(" and depth == 0:
                start = i + 1
            depth += 1
        elif ch in ">)":
            depth -= 1
            if ch == ")" and depth == 0:
                out.append(sig[start:i].strip())
        elif ch == "," and depth == 1 and start is not None:
            out.append(sig[start:i].strip())
            start = i + 1
    return out


def _demangle(name):
    """The C++ runtime's own demangler (abi::__cxa_demangle of libstdc++)."""
    lib = ctypes.CDLL("libstdc++.so.6")
    fn = lib.__cxa_demangle
    fn.restype = ctypes.c_void_p
    fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    status = ctypes.c_int(-1)
    p = fn(name.encode(), None, None, ctypes.byref(status))
    assert status.value == 0 and p, (name, status.value)
    out = ctypes.string_at(p).decode()
    ctypes.CDLL(None).free(ctypes.c_void_p(p))
    return out


def _resource_rows(path):
    """[(code object, kernel name: first 60 characters, VGPRs, spilled VGPRs, spilled SGPRs, scratch bytes)] of a library, in order."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "isa"))
    import disasm_lib
    import tempfile
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for co in disasm_lib.code_objects(path, d):
            for k in disasm_lib.kernel_notes(co):
                rows.append((os.path.basename(co), k["name"][:60], k["vgpr_count"], k["vgpr_spill_count"], k["sgpr_spill_count"],
                             k["private_segment_fixed_size"]))
    return rows


def test_shipped_kernel_resources_unchanged():
    """The nine shipped code objects keep the recorded per-kernel VGPR, spill and scratch table (tests/golden/shipped_kernel_resources.txt):
    the RolloutIO field and the env.step argument of per-plan parameters are read by the task-plugin instantiation only."""
    from dial_mpc_amd import _lib
    want = [tuple(line.split()) for line in open(os.path.join(ROOT, "tests", "golden", "shipped_kernel_resources.txt"))
            if line.strip() and not line.startswith("#")]
    got = _resource_rows(_lib.LIB_PATH)
    assert len({r[0] for r in got}) == 9
    assert got == want


def test_plan_param_rows_validation():
    from dial_mpc_amd import _abi, _lib
    P = _abi.MACROS["DIAL_USER_PARAMS"]
    rows = _lib.plan_param_rows([[1, 2], [3, 4], [5, 6]])
    assert rows.shape == (3, P) and rows.dtype == np.float32
    assert np.array_equal(rows[:, :2], [[1, 2], [3, 4], [5, 6]]) and not rows[:, 2:].any()
    for bad in (np.zeros((2, P + 1)), np.zeros(4), np.zeros((2, 2, 2)), np.zeros((0, 3)),
                np.zeros((_abi.MACROS["DIAL_MAX_PLANS"] + 1, 1))):
        with pytest.raises(ValueError):
            _lib.plan_param_rows(bad)


def test_custom_env_plan_params(env):
    rows = env.plan_params(vx=[0.3, 0.6, 0.9], height=[0.25, 0.3, 0.35])
    base = env.user_param_vector()
    assert rows.shape == (3, len(env.user_params)) and rows.dtype == np.float32
    assert np.array_equal(rows[:, 0], np.float32([0.3, 0.6, 0.9])) and np.array_equal(rows[:, 1], np.float32([0.25, 0.3, 0.35]))
    assert np.array_equal(rows[:, 2:], np.tile(np.float32(base[2:]), (3, 1)))   # fields not given: the config's values
    with pytest.raises(KeyError):
        env.plan_params(vx=[0.1, 0.2], speed=[1.0, 2.0])
    with pytest.raises(ValueError):
        env.plan_params(vx=[0.1, 0.2], height=[0.3])
    with pytest.raises(ValueError):
        env.plan_params()


def test_rows_on_a_built_in_env_are_refused():
    from dial_mpc_amd.envs.unitree_go2_env import UnitreeGo2Env, UnitreeGo2EnvConfig
    e = UnitreeGo2Env(UnitreeGo2EnvConfig())
    with pytest.raises(ValueError, match="custom environment"):
        e.step_batch([None, None], np.zeros((2, 12)), user_params=np.zeros((2, 1)))


def _main(argv, capsys):
    from dial_mpc_amd.core.dial_core import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


@pytest.mark.parametrize("argv,words", [
    (["--example", "unitree_go2_trot", "--n-envs", "4", "--env-param", "vx=0.1,0.2,0.3,0.4"], "built-in environment"),
    (["--custom-env", EX_MOD, "--config", EX_YAML, "--n-envs", "4", "--env-param", "vx=0.3,0.6"], "2 values for --n-envs 4"),
    (["--custom-env", EX_MOD, "--config", EX_YAML, "--env-param", "vx=0.3"], "--n-envs M with M > 1"),
    (["--custom-env", EX_MOD, "--config", EX_YAML, "--n-envs", "2", "--env-param", "speed=0.3,0.6"], "not one of the task parameters"),
    (["--custom-env", EX_MOD, "--config", EX_YAML, "--n-envs", "2", "--env-param", "vx"], "expected NAME=V1"),
    (["--custom-env", EX_MOD, "--config", EX_YAML, "--n-envs", "2", "--env-param", "vx=a,b"], "expected NAME=V1"),
])
def test_env_param_flag_is_checked_before_anything_runs(argv, words, capsys):
    assert words in _main(argv, capsys)
