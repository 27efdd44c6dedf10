"""Grouped planning (M plans in one launch) -- the parts that need no GPU: the C ABI as _abi parses it, the symbols of the built
library, and the --n-envs handling of the closed-loop driver."""
import os
import re

import pytest

from dial_mpc_amd import _abi, _lib

NEW_ENTRY_POINTS = ("dial_reverse_once_batch", "dial_reverse_once_batch_rng", "dial_shift_batch", "dial_env_step_batch")


def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    return {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip()
            for m in re.finditer(r"^int\s+(dial_\w+)\s*\((.*?)\);", text, flags=re.M | re.S)}


def test_options_carry_the_plan_capacity():
    assert list(_abi.DialOptions._meta)[-1] == "plan_cap"           # appended: earlier fields keep their offsets
    assert _abi.DialOptions._meta["plan_cap"][0] == ()
    assert _abi.MACROS["DIAL_MAX_PLANS"] >= 32
    opts = _abi.fill(_abi.DialOptions(), dict(plan_cap=8))
    assert opts.plan_cap == 8 and opts.pair_mode == 0
    assert _abi.DialOptions().plan_cap == 0                           # default: one plan, today's allocation


def test_header_declares_the_grouped_entry_points():
    protos = _prototypes()
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
    assert protos["dial_reverse_once_batch"] == (
        "dial_ctx* ctx, const float* states, const float* Ybar_in, const float* noise_scale, int ns, const float* eps, int M, "
        "float* Ybar_out, float* rews, float* qbar, float* qdbar, float* xbar, void* stream")
    assert "uint64_t seed, uint32_t counter, int M" in protos["dial_reverse_once_batch_rng"]
    assert protos["dial_shift_batch"] == "dial_ctx* ctx, float* Y, int M, void* stream"
    assert protos["dial_env_step_batch"].endswith("float* ctrl_out, int M, void* stream")


def test_library_exports_the_grouped_entry_points():
    _lib.build()
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert name in _lib.EXPORTED
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_context_wrappers_exist():
    for name in ("reverse_once_batch", "reverse_once_batch_rng", "shift_batch", "env_step_batch"):
        assert callable(getattr(_lib.Context, name)), name
    from dial_mpc_amd.core.dial_core import MBDPI
    from dial_mpc_amd.envs.base_env import BaseEnv
    assert callable(MBDPI.reverse_once_batch) and callable(MBDPI.shift_batch) and callable(BaseEnv.step_batch)


def test_driver_n_envs_dispatch(monkeypatch):
    from dial_mpc_amd.core import dial_core
    seen = {}

    def fake_batched(dial_config, env, n_envs):
        seen.update(n_envs=n_envs, n_steps=dial_config.n_steps, env=env)
    monkeypatch.setattr(dial_core, "main_batched", fake_batched)
    monkeypatch.setattr(dial_core, "load_dial_and_env", lambda d: (dial_core.DialConfig(), None, "ENV"))
    dial_core.main(["--example", "unitree_go2_trot", "--n-envs", "3", "--n-steps", "5"])
    assert seen == dict(n_envs=3, n_steps=5, env="ENV")


def test_driver_n_envs_default_is_the_single_loop(monkeypatch):
    from dial_mpc_amd.core import dial_core

    class Stop(Exception):
        pass

    def fake_mbdpi(*a, **kw):
        raise Stop(kw)
    monkeypatch.setattr(dial_core, "main_batched", lambda *a: pytest.fail("--n-envs 1 must run the single loop"))
    monkeypatch.setattr(dial_core, "load_dial_and_env", lambda d: (dial_core.DialConfig(), None, "ENV"))
    monkeypatch.setattr(dial_core, "MBDPI", fake_mbdpi)
    with pytest.raises(Stop) as e:
        dial_core.main(["--example", "unitree_go2_trot"])
    assert e.value.args[0] == {}                                      # MBDPI(dial_config, env): no n_plans


@pytest.mark.parametrize("bad", ["0", "-2", "two"])
def test_driver_n_envs_rejects_bad_values(bad, capsys):
    from dial_mpc_amd.core import dial_core
    with pytest.raises(SystemExit):
        dial_core.main(["--example", "unitree_go2_trot", "--n-envs", bad])
    assert "--n-envs" in capsys.readouterr().err


def test_driver_list_examples_accepts_n_envs(capsys):
    from dial_mpc_amd.core import dial_core
    dial_core.main(["--list-examples", "--n-envs", "4"])
    assert "unitree_go2_trot" in capsys.readouterr().out


def test_bench_tool_is_present():
    assert os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_plan_batch.py"))
