"""Reference tables of custom environments without a GPU: the C ABI declares and exports dial_set_user_table; probe plugins built from
the current sources export the third table, without and with a control law, and keep their kernel counts; the host restatement of the
index rule against a brute-force walk; shape and dtype validation of Context.set_user_table / CustomEnv.make_table; the example's
table."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from table_cases import brute_row, build_stale_plugins, build_table_plugins
from test_custom_env import LLVM, ROOT, _disasm, _kernels


@pytest.fixture(scope="module")
def plugins():
    return build_table_plugins()   # (three builds, in parallel; the GPU suite finds them in the cache)


def _dyn_syms(so):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", so], stdout=subprocess.PIPE, text=True).stdout


def _exports(syms, name):
    return re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+" + name + "$", syms, flags=re.M) is not None


def test_header_declares_the_entry_point_and_the_macros():
    from dial_mpc_amd import _abi
    text = open(_abi.HEADER).read()
    assert re.search(r"int dial_set_user_table\(dial_ctx\* ctx, const float\* table, int rows, int cols, int row0, int mode\);", text)
    assert _abi.MACROS["DIAL_USER_TABLE_COLS"] == 64 and _abi.MACROS["DIAL_TABLE_CLAMP"] == 0 and _abi.MACROS["DIAL_TABLE_WRAP"] == 1
    for h, struct in (("user_reward.h", "DialRewardIn"), ("user_control.h", "DialControlIn")):   # appended, in this order
        src = open(os.path.join(ROOT, "dial_mpc_amd", "csrc", h)).read()
        body = re.search(r"struct " + struct + r" \{(.*?)\n\};", src, flags=re.S).group(1)
        body = re.sub(r"//[^\n]*", "", body)
        tail = re.sub(r"\s+", " ", body).strip()
        assert tail.endswith("const float* row; int row_index; const float* table; int table_rows, table_cols;"), tail[-200:]


def test_library_exports_the_entry_point():
    from dial_mpc_amd import _lib
    assert "dial_set_user_table" in _lib.EXPORTED
    so = os.path.join(ROOT, "dial_mpc_amd", "csrc", "libdialhip.so")
    if not os.path.exists(so):
        _lib.build()
    assert _exports(_dyn_syms(so), "dial_set_user_table")
    assert _lib.TABLE_MODES == {"clamp": 0, "wrap": 1}


@pytest.mark.parametrize("name,kernels", [("go2", 5), ("go2_law", 6)])
def test_plugins_export_the_table_symbol_and_keep_their_kernels(plugins, name, kernels, tmp_path):
    from dial_mpc_amd import plugin
    assert plugin.TABLE_SYMBOL == "dial_plugin_table_v1"
    so = plugins[name]
    syms = _dyn_syms(so)
    assert _exports(syms, "dial_plugin_ops_v1") and _exports(syms, plugin.TABLE_SYMBOL), syms
    assert _exports(syms, "dial_plugin_ctrl_v1") == (kernels == 6)
    cos, names = _kernels(so, str(tmp_path))
    assert len(cos) == 1 and len(set(names)) == kernels, names
    assert ("user_control_kernel" in "\n".join(names)) == (kernels == 6)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa", "check_dpp_hazards.py"), _disasm(cos[0])],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_stand_ins_for_older_plugins(tmp_path):
    """The two plugins the GPU test of dial_set_user_table's refusals loads (built here, found in the cache there): one without the
    table symbol -- otherwise the same five kernels -- and one that exports it."""
    stale = build_stale_plugins()
    syms = _dyn_syms(stale["no_table"])
    assert _exports(syms, "dial_plugin_ops_v1") and "dial_plugin_table_v1" not in syms
    _, names = _kernels(stale["no_table"], str(tmp_path))
    assert len(set(names)) == 5, names
    assert _exports(_dyn_syms(stale["version"]), "dial_plugin_table_v1")


@pytest.mark.parametrize("mode", ["clamp", "wrap"])
@pytest.mark.parametrize("row0", [-9, 0, 4])
@pytest.mark.parametrize("rows", [1, 2, 7])
def test_table_row_matches_a_brute_force_walk(rows, row0, mode):
    from dial_mpc_amd import _lib
    from dial_mpc_amd.envs.custom_env import table_row
    for step in range(-5, 3 * rows + 1):
        want = brute_row(step, row0, rows, mode)
        assert 0 <= want < rows
        assert table_row(step, row0, rows, mode) == want, (step, row0, rows, mode)
        assert table_row(step, row0, rows, _lib.TABLE_MODES[mode]) == want
    with pytest.raises(ValueError):
        table_row(0, 0, 0, mode)
    with pytest.raises(ValueError):
        table_row(0, 0, rows, "mirror")


BAD_TABLES = [np.zeros(5, np.float32),                  # wrong rank
              np.zeros((2, 3, 4), np.float32),
              np.zeros((0, 5), np.float32),             # 0 rows
              np.zeros((3, 0), np.float32),
              np.zeros((3, 65), np.float32),            # cols > DIAL_USER_TABLE_COLS
              np.array([["a", "b"]])]                   # not numbers


@pytest.mark.parametrize("bad", BAD_TABLES, ids=lambda a: "x".join(map(str, a.shape)) + str(a.dtype))
def test_table_validation(bad):
    """A bad table is refused on the host, before any library call: by the conversion itself, by Context.set_user_table (called on an
    object without a context: the check comes first) and by a CustomEnv whose make_table returns it."""
    from dial_mpc_amd import _lib
    from dial_mpc_amd.examples.custom_env.go2_track_clip import Go2TrackClipConfig, Go2TrackClipEnv
    with pytest.raises(ValueError):
        _lib.user_table_array(bad)
    with pytest.raises(ValueError):
        _lib.Context.set_user_table(object.__new__(_lib.Context), bad)

    env = Go2TrackClipEnv(Go2TrackClipConfig())
    env.make_table = lambda: bad
    env._plugin = "unused.so"   # (context_kwargs would build the plugin: not what this test is about)
    with pytest.raises(ValueError):
        env.context_kwargs()
    with pytest.raises(ValueError):
        env.set_table(bad)
    with pytest.raises(ValueError):
        _lib.Context.set_user_table(object.__new__(_lib.Context), np.zeros((2, 2), np.float32), mode="mirror")


def test_table_conversion():
    from dial_mpc_amd import _lib
    a = _lib.user_table_array([[1, 2], [3, 4]])
    assert a.dtype == np.float32 and a.shape == (2, 2) and a.flags["C_CONTIGUOUS"]
    b = _lib.user_table_array(np.arange(12, dtype=np.float64).reshape(3, 4).T)
    assert b.dtype == np.float32 and b.flags["C_CONTIGUOUS"] and np.array_equal(b, np.arange(12).reshape(3, 4).T)
    assert _lib.user_table_array(np.zeros((1, 64))).shape == (1, 64)
    _lib.check_user_table((5, 3), np.float32)
    with pytest.raises(ValueError):
        _lib.check_user_table((5, 3), np.float64)


def test_custom_env_defaults_and_context_kwargs():
    """An env without a table passes none (the kwargs of before); the example passes its table, offset and mode; set_table overrides."""
    from dial_mpc_amd.envs.custom_env import CustomEnv
    from dial_mpc_amd.examples.custom_env.go2_height_walk import Go2HeightWalkConfig, Go2HeightWalkEnv
    from dial_mpc_amd.examples.custom_env.go2_track_clip import Go2TrackClipConfig, Go2TrackClipEnv
    assert CustomEnv.table_mode == "clamp" and CustomEnv.table_row0 == 0
    plain = Go2HeightWalkEnv(Go2HeightWalkConfig())
    assert plain.make_table() is None and plain._table() is None
    plain._plugin = "unused.so"   # (context_kwargs would build the plugin: not what this test is about)
    assert set(plain.context_kwargs()) == {"plugin", "user_params"}
    env = Go2TrackClipEnv(Go2TrackClipConfig())
    env._plugin = "unused.so"
    kw = env.context_kwargs()
    assert kw["table_mode"] == 1 and kw["table_row0"] == 0 and np.array_equal(kw["user_table"], env.make_table())
    assert env.set_table(np.ones((4, 13))) is None      # (no context yet: nothing to rebind)
    assert env.context_kwargs()["user_table"].shape == (4, 13)
    env.set_table(None)
    assert env.context_kwargs()["user_table"].shape == (100, 13)


def test_example_table_is_a_periodic_clip():
    from dial_mpc_amd.examples.custom_env.go2_track_clip import Go2TrackClipConfig, Go2TrackClipEnv
    env = Go2TrackClipEnv(Go2TrackClipConfig())
    t = env.make_table()
    assert t.shape == (100, 13) and t.dtype == np.float32 and np.all(np.isfinite(t)) and env.table_mode == "wrap"
    # periodic: the row after the last one is the first -- its step from row 99 is as small as any other step of the clip, and the
    # half-period shift negates the legs' swing about the home pose and leaves the trunk's height (two bobs per period) as it is
    steps = np.abs(np.diff(np.vstack([t, t[:1]]).astype(np.float64), axis=0)).max(axis=1)
    assert steps[-1] <= 1.0001 * steps[:-1].max() and steps.min() > 0
    home = np.asarray(env._init_q)[7:19]
    assert np.allclose((t[:50, :12] - home) + (t[50:, :12] - home), 0.0, atol=1e-6)
    assert np.allclose(t[:50, 12], t[50:, 12], atol=1e-6)
    lo, hi = env.joint_range[:, 0], env.joint_range[:, 1]
    assert np.all(t[:, :12] >= lo - 1e-6) and np.all(t[:, :12] <= hi + 1e-6)   # targets inside the sampling range
    src = env.reward_source()
    code = re.sub(r"//[^\n]*", "", src)
    assert "in.row[" in code and "/" not in code and "sqrt" not in code   # + - * only
