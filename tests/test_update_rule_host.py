"""Update rules on the host: the NumPy reference of the elite rule against a brute-force rank count, the key map and the elite
arithmetic of csrc/update_rule.h compiled with g++, elite_count, DialConfig loading and the driver's overrides.  No GPU."""
import ctypes
import glob
import itertools
import os
import subprocess

import numpy as np
import pytest
import yaml

from dial_mpc_amd import _abi, _lib
from update_rule_ref import elite_order_ref, elite_weights_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "dial_mpc_amd", "csrc", "update_rule.h")
SPECIALS = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], np.float32)


def ranks_above(r):
    """Brute force, O(B^2), on floats: rank[.., i] = how many candidates stand before i -- j stands before i when it is a number and
    i a NaN, when r[j] > r[i], or when neither is above the other and j < i."""
    r = np.asarray(r, np.float32)
    a, b = r[..., :, None], r[..., None, :]                  # a = r[i], b = r[j]
    with np.errstate(invalid="ignore"):
        j_above = (~np.isnan(b) & np.isnan(a)) | (b > a)
        i_above = (~np.isnan(a) & np.isnan(b)) | (a > b)
    idx = np.arange(r.shape[-1])
    tie_before = ~j_above & ~i_above & (idx[None, :] < idx[:, None])
    return (j_above | tie_before).sum(-1)


@pytest.mark.parametrize("B", [2, 3, 4, 5, 6])
def test_reference_order_is_the_rank_count_exhaustively(B):
    rows = np.array(list(itertools.product(SPECIALS, repeat=B)), np.float32)
    rank = ranks_above(rows)
    assert (np.sort(rank, axis=1) == np.arange(B)).all()       # a total order: the ranks are a permutation
    for r, rk in zip(rows, rank):
        assert (rk[elite_order_ref(r)] == np.arange(B)).all(), r
    for r, rk in zip(rows[:: max(1, len(rows) // 200)], rank[:: max(1, len(rows) // 200)]):
        for K in range(1, B + 1):
            w = elite_weights_ref(r, K)
            assert w.dtype == np.float32 and ((w != 0) == (rk < K)).all(), (r, K)
            assert (w[rk < K].view(np.uint32) == (np.float32(1) / np.float32(K)).view(np.uint32)).all()
            assert (w[rk >= K].view(np.uint32) == 0).all()      # +0.0f, not -0


@pytest.mark.parametrize("B", [65, 1025])
def test_reference_on_random_draws(B):
    rng = np.random.default_rng(B)
    for trial in range(6):
        r = rng.standard_normal(B).astype(np.float32)
        if trial >= 2:   # ties and specials
            r = np.round(r * 2).astype(np.float32) / 2
            r[rng.integers(0, B, 5)] = rng.choice(SPECIALS, 5)
        rk = ranks_above(r)
        assert (rk[elite_order_ref(r)] == np.arange(B)).all()
        for K in (1, 2, -(-B // 10), B - 1, B):
            w = elite_weights_ref(r, K)
            assert int((w != 0).sum()) == K and ((w != 0) == (rk < K)).all()


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    assert os.path.exists(HEADER), "csrc/update_rule.h is missing"
    d = tmp_path_factory.mktemp("update_rule")
    src = d / "ur.cpp"
    src.write_text('#include "update_rule.h"\n'
                   'extern "C" void ur_keys(const uint32_t* bits, uint32_t* keys, int n) { for (int i = 0; i < n; i++) keys[i] = dial_update::reward_key(bits[i]); }\n'
                   'extern "C" uint32_t ur_weight_bits(int K) { return dial_update::elite_weight_bits(K); }\n'
                   'extern "C" int ur_ties(int K, int above) { return dial_update::elite_ties_taken(K, above); }\n'
                   'extern "C" int ur_bin(uint32_t above, uint32_t in_bin, uint32_t remaining) { return dial_update::elite_bin_holds(above, in_bin, remaining); }\n')
    out = d / "libur.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(out), str(src)])
    lib = ctypes.CDLL(str(out))
    lib.ur_keys.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.ur_keys.restype = None
    lib.ur_weight_bits.restype = ctypes.c_uint32
    lib.ur_bin.argtypes = [ctypes.c_uint32] * 3
    return lib


def _keys(lib, bits):
    bits = np.ascontiguousarray(bits, np.uint32)
    keys = np.empty_like(bits)
    lib.ur_keys(bits.ctypes.data, keys.ctypes.data, bits.size)
    return keys


SPECIAL_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x3f800000,
                         0xbf800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7f800001, 0xff800001, 0x7fc00000, 0xffc00000,
                         0x7fffffff, 0xffffffff], np.uint32)


def test_key_map_orders_like_the_contract(hostlib):
    rng = np.random.default_rng(7)
    bits = np.concatenate([SPECIAL_BITS, rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32)])
    keys = _keys(hostlib, bits)
    vals = bits.view(np.float32)
    nan = np.isnan(vals)
    assert nan.sum() >= 6
    assert (keys[nan] == 0).all()                      # every NaN pattern, both signs: the lowest key
    assert (keys[~nan] > 0).all()                      # ... strictly below every number, -inf included
    assert keys[0] == keys[1]                          # +0 and -0
    # key(a) > key(b) exactly when a ranks above b: every special against everything, and random pairs
    a_idx = np.concatenate([np.repeat(np.arange(len(SPECIAL_BITS)), bits.size), rng.integers(0, bits.size, 200000)])
    b_idx = np.concatenate([np.tile(np.arange(bits.size), len(SPECIAL_BITS)), rng.integers(0, bits.size, 200000)])
    a, b = vals[a_idx], vals[b_idx]
    with np.errstate(invalid="ignore"):
        above = (~np.isnan(a) & np.isnan(b)) | (a > b)
    assert ((keys[a_idx] > keys[b_idx]) == above).all()
    # and the order it induces is the reference's
    sample = vals[:4096]
    assert (np.argsort(-keys[:4096].astype(np.int64), kind="stable") == elite_order_ref(sample)).all()


def test_elite_arithmetic_of_the_header(hostlib):
    Ks = np.concatenate([np.arange(1, 70000), [(1 << 24) - 1, (1 << 23) + 1, 1 << 23]])
    want = (np.float32(1) / Ks.astype(np.float32)).view(np.uint32)
    got = np.array([hostlib.ur_weight_bits(int(K)) for K in Ks], np.uint32)
    assert (got == want).all(), Ks[got != want][:10]
    assert hostlib.ur_weight_bits(1) == 0x3f800000      # exactly 1.0f
    assert hostlib.ur_ties(205, 200) == 5 and hostlib.ur_ties(1, 0) == 1
    # a histogram bin holds the K'-th largest exactly when above < K' <= above + in_bin
    assert hostlib.ur_bin(0, 3, 1) and hostlib.ur_bin(0, 3, 3) and not hostlib.ur_bin(0, 3, 4)
    assert hostlib.ur_bin(4, 1, 5) and not hostlib.ur_bin(4, 1, 4) and not hostlib.ur_bin(4, 0, 5)


def test_elite_count():
    assert _lib.elite_count("cem", 2048, 0.1, 0) == 205          # ceil(204.8)
    assert _lib.elite_count("cem", 2000, 0.05, 0) == 100         # 0.05 * 2000 = 100.00000000000001 in binary: not 101
    assert _lib.elite_count("cem", 2048, 0.1, 7) == 7            # an explicit count wins
    assert _lib.elite_count("cem", 5, 0.01, 0) == 1              # at least one
    assert _lib.elite_count("cem", 63, 1.0, 0) == 63
    assert _lib.elite_count("cem", 63, 0.5, 64) == 64            # the mean trajectory is a candidate too
    assert _lib.elite_count("ps", 2048, 0.1, 0) == 1
    assert _lib.elite_count("ps", 2048, 7.0, -3) == 1            # ps reads neither
    for frac in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="elite_frac"):
            _lib.elite_count("cem", 2048, frac, 0)
    with pytest.raises(ValueError, match="negative"):
        _lib.elite_count("cem", 2048, 0.1, -1)
    with pytest.raises(ValueError, match="exceeds"):
        _lib.elite_count("cem", 63, 0.1, 65)
    with pytest.raises(KeyError):
        _lib.elite_count("mppi", 2048, 0.1, 0)
    assert _lib.UPDATE_RULES == {"mppi": 0, "elite": 1}
    assert _abi.MACROS["DIAL_UPDATE_MPPI"] == 0 and _abi.MACROS["DIAL_UPDATE_ELITE"] == 1
    for name in ("dial_set_update_rule", "dial_get_weights"):
        assert name in _lib.EXPORTED
    assert callable(_lib.Context.set_update_rule) and callable(_lib.Context.weights)


def test_dial_config_loads_the_new_fields_and_every_example_unchanged():
    from dial_mpc_amd.core.dial_config import DialConfig
    from dial_mpc_amd.utils.io_utils import load_dataclass_from_dict
    dc = load_dataclass_from_dict(DialConfig, dict(update_method="cem", elite_frac=0.25, Nsample=64, unknown_key=1))
    assert (dc.update_method, dc.elite_frac, dc.n_elite) == ("cem", 0.25, 0)
    assert (DialConfig().update_method, DialConfig().elite_frac, DialConfig().n_elite) == ("mppi", 0.1, 0)
    paths = sorted(glob.glob(os.path.join(ROOT, "dial_mpc_amd", "examples", "**", "*.yaml"), recursive=True))
    assert len(paths) >= 15
    for p in paths:
        dc = load_dataclass_from_dict(DialConfig, yaml.safe_load(open(p)))
        assert (dc.update_method, dc.elite_frac, dc.n_elite) == ("mppi", 0.1, 0), p


def test_planner_surface():
    from dial_mpc_amd.core import dial_core
    assert set(dial_core.UPDATE_FNS) == {"mppi", "cem", "ps"}
    assert dial_core.UPDATE_FNS["mppi"] is dial_core.softmax_update and dial_core.UPDATE_FNS["cem"] is dial_core.elite_update
    assert callable(dial_core.MBDPI.set_update) and callable(dial_core.MBDPI.weights)
    env = type("Env", (), dict(action_size=12))()
    with pytest.raises(KeyError):                      # as before: any other method is a KeyError, before anything is created
        dial_core.MBDPI(dial_core.DialConfig(update_method="nope"), env)
    with pytest.raises(ValueError, match="elite_frac"):
        dial_core.MBDPI(dial_core.DialConfig(update_method="cem", elite_frac=0.0), env)


class _Stop(Exception):
    pass


def _run_driver(monkeypatch, argv, batched=False):
    from dial_mpc_amd.core import dial_core
    seen = {}

    def fake_mbdpi(dial_config, env, **kw):
        seen["cfg"] = dial_config
        raise _Stop()

    def fake_batched(dial_config, env, n_envs, **kw):
        seen["cfg"] = dial_config
    monkeypatch.setattr(dial_core, "load_dial_and_env", lambda d: (dial_core.DialConfig(), None, "ENV"))
    monkeypatch.setattr(dial_core, "MBDPI", fake_mbdpi)
    monkeypatch.setattr(dial_core, "main_batched", fake_batched)
    if batched:
        dial_core.main(argv)
    else:
        with pytest.raises(_Stop):
            dial_core.main(argv)
    return seen["cfg"]


def test_driver_overrides(monkeypatch):
    base = ["--example", "unitree_go2_trot"]
    c = _run_driver(monkeypatch, base)
    assert (c.update_method, c.elite_frac, c.n_elite) == ("mppi", 0.1, 0)
    c = _run_driver(monkeypatch, base + ["--update-method", "cem", "--elite-frac", "0.25"])
    assert (c.update_method, c.elite_frac, c.n_elite) == ("cem", 0.25, 0)
    c = _run_driver(monkeypatch, base + ["--update-method", "ps"])
    assert (c.update_method, c.elite_frac) == ("ps", 0.1)
    c = _run_driver(monkeypatch, base + ["--n-envs", "3", "--update-method", "cem", "--elite-frac", "0.5"], batched=True)
    assert (c.update_method, c.elite_frac) == ("cem", 0.5)
    with pytest.raises(SystemExit):
        _run_driver(monkeypatch, base + ["--update-method", "softmax"])
