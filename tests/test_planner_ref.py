"""The fp64 restatements the GPU tests of the planner's kernels compare against (tests/philox_ref.py, tests/planner_ref.py), on the CPU:
Philox4x32-10 against the published Random123 known-answer vectors, the Box-Muller edge u1 = 1, the tools' use of the one restatement,
the cfg's spline matrices, and the error bounds against an fp32 emulation of the kernels' own summation orders."""
import importlib
import os
import sys

import numpy as np
import pytest

import philox_ref as P
import planner_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answers(ctr, key, out):
    """Random123's kat_vectors for philox4x32, 10 rounds (counter, key -> output)."""
    assert tuple(int(x) for x in P.philox4x32_10(*ctr, *key)) == out


def test_words_are_keyed_by_sample_quad_iteration_and_seed():
    seed = 0xFEDC_BA98_7654_3210
    w = P.words(np.array([3, 3]), np.array([1, 2]), 9, seed)
    assert w.shape == (2, 4) and not np.array_equal(w[0], w[1])
    assert tuple(w[0]) == tuple(int(x) for x in P.philox4x32_10(3, 1, 9, 0, 0x76543210, 0xFEDCBA98))


def test_uniforms_reach_one_and_the_normal_is_then_exactly_zero():
    u1, u2 = P.uniforms(np.array([0xFFFFFFFF, 0, 0x000000FF, 0x80000000], np.uint32))
    assert u1[0] == 1.0 and u1[1] == np.float32(0.5 / 16777216) and u2[0] == np.float32(0.5 / 16777216) and u2[1] == 0.5 / 16777216 + 0.5
    # the key the GPU test uses: word 0 = 0xffffff73 -> u1 = 1 -> the first pair of sample 5359985, quad 0 is exactly 0
    w = P.words(5359985, 0, 5, 0x9E37_79B9_7F4A_7C15)
    assert w[0] == 0xffffff73
    z, r, _, _ = P.box_muller(*P.uniforms(w))
    assert r[0] == 0 and z[0] == 0 and z[1] == 0 and z[2] != 0
    eps = P.philox_normal(0x9E37_79B9_7F4A_7C15, 5, 1, 114, n_begin=5359985)
    assert eps.shape == (1, 114) and eps.dtype == np.float32 and eps[0, 0] == 0 and eps[0, 1] == 0


def test_normals_are_standard_and_tail_quads_are_cut():
    z, r, t, L = P.normals(17, 2, 100, 4096, 114)
    assert z.shape == r.shape == t.shape == L.shape == (4096, 114)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    z120 = P.normals(17, 2, 100, 4096, 120)[0]
    assert np.array_equal(z120[:, :114], z)                       # C = 114: the last quad's first two draws


@pytest.mark.parametrize("tool", ["allegro_closed_loop_study", "allegro_drop_autopsy", "allegro_stall_rate"])
def test_tools_use_the_one_restatement(tool):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        mod = importlib.import_module(tool)
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    if tool == "allegro_drop_autopsy":    # (imports it where it is used)
        src = open(mod.__file__).read()
        assert "from philox_ref import philox_normal" in src and "def philox_normal" not in src
    else:
        assert mod.philox_normal is P.philox_normal


SHIFT_SHAPES = [(16, 4), (20, 5), (25, 5), (20, 4), (24, 6), (16, 2), (35, 2), (27, 9), (35, 5), (35, 9)]


@pytest.mark.parametrize("Hs,Hn", SHIFT_SHAPES)
def test_cfg_spline_matrices_are_the_fp64_ones_rounded(Hs, Hn):
    from dial_mpc_amd.core import spline
    from dial_mpc_amd.core.dial_config import DialConfig
    from dial_mpc_amd.core.dial_core import make_cfg
    dc = DialConfig(Nsample=8, Hsample=Hs, Hnode=Hn)
    W32, V32 = R.cfg_matrices(make_cfg(dc))
    W, V = spline.node2u_matrix(Hs, Hn), spline.u2node_matrix(Hs, Hn)
    assert np.array_equal(W32, W.astype(np.float32)) and np.array_equal(V32, V.astype(np.float32))


def test_shift_restatement_is_the_reference_formula():
    from dial_mpc_amd.core import spline
    W, V = spline.node2u_matrix(16, 4), spline.u2node_matrix(16, 4)
    Y = np.random.default_rng(0).uniform(-1, 1, (5, 12))
    got, bound = R.shift_ref(W, V, Y)
    u = W @ Y
    assert np.allclose(got, V @ np.concatenate([u[1:], np.zeros((1, 12))]), rtol=0, atol=1e-15)
    assert np.all(bound > 0) and np.all(bound < 1e-5)


def _softmax_fp32(r, temp):
    """weights_kernel's fp32 arithmetic in its own order (per-thread strided sums, a 64-lane butterfly, 16 partials in order)."""
    f = np.float32
    B = r.size

    def block_sum(v):
        acc = np.zeros(1024, f)
        for k in range(0, B, 1024):
            part = np.zeros(1024, f)
            part[:min(1024, B - k)] = v[k:k + 1024]
            acc = (acc + part).astype(f)
        acc = acc.reshape(16, 64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc[:, :o] + acc[:, o:2 * o]).astype(f)
        s = f(0)
        for x in acc[:, 0]:
            s = f(s + x)
        return s
    mean = f(block_sum(r) / f(B))
    std = f(np.sqrt(f(block_sum(((r - mean) ** 2).astype(f)) / f(B))))
    l = ((r - r[-1]).astype(f) / std / f(temp)).astype(f)
    mx = f(f(r.max() - r[-1]) / std / f(temp))
    e = np.exp((l - mx).astype(f)).astype(f)
    return (e / block_sum(e)).astype(f)


@pytest.mark.parametrize("B", [2, 65, 1025, 4097])
def test_softmax_bound_covers_fp32_rounding(B):
    rng = np.random.default_rng(B)
    for i, r in enumerate((rng.standard_normal(B), -1e3 + rng.uniform(-1e-2, 1e-2, B), rng.uniform(-3, 1, B))):
        r = r.astype(np.float32)
        w = _softmax_fp32(r, 0.05)
        ref, _, _ = R.softmax_ref(r, 0.05)
        assert np.all(np.abs(w - ref) <= R.softmax_bound(r, 0.05))
        # the mutation "sample std instead of population std" leaves the bound at small B (where the mean is not a cancellation)
        r64 = r.astype(np.float64)
        wrong = np.exp((r64 - r64[-1]) / r64.std(ddof=1) / 0.05 - ((r64.max() - r64[-1]) / r64.std(ddof=1) / 0.05))
        if B <= 65 and i != 1:
            assert not np.all(np.abs(wrong / wrong.sum() - ref) <= R.softmax_bound(r, 0.05))


@pytest.mark.parametrize("n_rows", [1, 64, 65, 128, 4097])
def test_wsum_bound_covers_fp32_rounding_and_not_a_missing_chunk(n_rows):
    f = np.float32
    rng = np.random.default_rng(n_rows)
    w = rng.uniform(0, 1, n_rows).astype(f)
    X = (rng.standard_normal((n_rows, 7)) * 10.0 ** rng.uniform(-3, 3, (n_rows, 1))).astype(f)
    per = -(-n_rows // 64)
    chunks = []
    for ch in range(64):
        part = np.zeros((4, 7), f)
        for r in range(ch * per, min(ch * per + per, n_rows)):
            part[(r - ch * per) % 4] = (part[(r - ch * per) % 4] + w[r] * X[r]).astype(f)
        chunks.append((((part[0] + part[1]).astype(f) + part[2]).astype(f) + part[3]).astype(f))
    got = np.zeros(7, f)
    for c in chunks:
        got = (got + c).astype(f)
    ref, bound = R.wsum_ref(w, X)
    assert np.all(np.abs(got - ref) <= bound)
    if 63 * per < n_rows:   # rows reach chunk 63: a final pass over 63 chunks leaves the bound
        short = np.sum(np.array(chunks[:63], np.float64), 0)
        assert not np.all(np.abs(short - ref) <= bound)
