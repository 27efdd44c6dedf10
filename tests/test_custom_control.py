"""User control laws without a GPU: a task plugin with the probe law of tests/control_probe.hip cross-compiles next to the probe reward,
exports the second table and carries user_control_kernel; a plugin without a law stays as it was; the cache tells laws apart; a
syntax error surfaces hipcc's message; an env with a law is free of the torque joint convention; the C ABI has dial_user_control."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from control_cases import build_control_plugins, control_source, permuted_go2_env
from plugin_cases import build_matrix, case_model_dict, probe_source
from test_custom_env import LLVM, ROOT, _disasm, _kernels


@pytest.fixture(scope="module")
def with_law():
    return build_control_plugins()   # (two builds, in parallel; the GPU suite finds them in the cache)


def _dyn_syms(so):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], stdout=subprocess.PIPE, text=True).stdout


def _exports(syms, name):
    return re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+" + name + "$", syms, flags=re.M) is not None


@pytest.mark.parametrize("name", ["go2", "h1_push_crate"])
def test_plugin_with_a_law_has_both_tables_and_the_control_kernel(with_law, name, tmp_path):
    so = with_law[name]
    syms = _dyn_syms(so)
    assert _exports(syms, "dial_plugin_ops_v1") and _exports(syms, "dial_plugin_ctrl_v1"), syms
    cos, names = _kernels(so, str(tmp_path))
    assert len(cos) == 1
    joined = "\n".join(names)
    for k in ("rollout_kernel", "env_step_kernel", "env_reset_kernel", "user_control_kernel"):
        assert re.search(k + r"I8DimsUser", joined), (k, names)
    assert len(set(names)) == 6, names   # three rollout variants, env.step, env.reset, the law's kernel
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), _disasm(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    for f in ("dial_plugin_dims.h", "dial_user_reward.hip", "dial_user_control.hip"):   # what it was built from, beside the library
        assert os.path.exists(os.path.join(os.path.dirname(so), f)), f
    assert open(os.path.join(os.path.dirname(so), "dial_user_control.hip")).read() == control_source()


def test_plugin_without_a_law_is_unchanged(with_law, tmp_path):
    so = build_matrix(["go2"])["go2"]
    assert so != with_law["go2"]
    syms = _dyn_syms(so)
    assert _exports(syms, "dial_plugin_ops_v1") and "dial_plugin_ctrl_v1" not in syms
    cos, names = _kernels(so, str(tmp_path))
    assert len(cos) == 1 and len(set(names)) == 5 and "user_control_kernel" not in "\n".join(names), names
    assert not os.path.exists(os.path.join(os.path.dirname(so), "dial_user_control.hip"))
    from dial_mpc_amd import plugin
    assert plugin.CTRL_SYMBOL == "dial_plugin_ctrl_v1" and plugin.SYMBOL == "dial_plugin_ops_v1"


def test_cache_key_tells_laws_apart():
    from dial_mpc_amd._lib import _COMMON, _FAST
    from dial_mpc_amd.plugin import plugin_key
    md, rew, flags = case_model_dict("go2"), probe_source(), _COMMON + _FAST
    none = plugin_key(md, rew, flags)
    law = plugin_key(md, rew, flags, control_source())
    other = plugin_key(md, rew, flags, control_source() + "\n// another law\n")
    assert len({none, law, other}) == 3
    assert plugin_key(md, rew, flags, None) == none and plugin_key(md, rew, flags, control_source()) == law


def test_law_syntax_error_carries_hipcc_message(tmp_path, monkeypatch):
    from dial_mpc_amd._lib import DialHipError
    from dial_mpc_amd.plugin import build_plugin
    monkeypatch.setenv("DIAL_PLUGIN_CACHE", str(tmp_path))
    bad = "DIAL_DEV float dial_user_control(const DialControlIn& in, int a, const float* p, const float* u) { return in.act[a] +; }\n"
    with pytest.raises(DialHipError, match=r"hipcc failed[\s\S]*dial_user_control\.hip[\s\S]*error:"):
        build_plugin(case_model_dict("go2"), probe_source(), control_src=bad)


def test_a_law_lifts_the_torque_joint_convention():
    """The permuted-actuator Go2 (tests/test_plugin_matrix.py) is refused under torque control without a law -- as before -- and
    accepted with one: the law indexes its own joints (act_qposadr / act_dofadr)."""
    import numpy as np
    with pytest.raises(ValueError, match=r"qpos\[7 \+ a\] / qvel\[6 \+ a\]"):
        permuted_go2_env("torque", with_law=False)
    env = permuted_go2_env("torque")
    assert list(np.asarray(env.sys.model["act_qposadr"])[:3]) == [10, 11, 12]
    assert env.control_source() == control_source() and env.make_task().position_control == 0


def test_c_abi_has_dial_user_control():
    from dial_mpc_amd import _abi, _lib
    text = open(_abi.HEADER).read()
    assert re.search(r"int dial_user_control\(dial_ctx\* ctx, const float\* states, const float\* actions, int n, float\* ctrl_out, void\* stream\);", text)
    assert "dial_user_control" in _lib.EXPORTED
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dial_user_control")
    assert hasattr(_lib.Context, "user_control")
