"""NumPy statements of what the comments in dial_mpc_amd/csrc/wave.h say every primitive does, the input sets of the wave.h pins, and
the fp64 side of the register L D L^T pins (tests/test_wave_prims_emu.py, tests/test_gpu_wave_prims.py, tests/test_gpu_reg_chol.py).
Lanes are PHYSICAL lanes 0..63 throughout; for WaveH the half is p & 32 and the logical lane p & 31.  Moves are stated on the raw
uint32 words (a move must not touch a bit), arithmetic in np.float32 (one correctly rounded operation per NumPy operation)."""
import numpy as np

import prim_lib as PL

P = np.arange(64)
F32 = np.float32
EPS = 2.0 ** -24


def u32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ input sets
def move_sets():
    """8 sets of 64 words for the data movement cases: ramp, random, cancellation, and one set per special pattern."""
    rng = np.random.default_rng(11)
    s = np.zeros((8, 64), np.uint32)
    s[0] = u32(P + 0.5)
    s[1] = u32(_mixed(rng, 64))
    s[2] = u32(cancellation(rng, 64))
    s[3] = np.where(P & 1, 0x80000000, 0) + np.where(P & 2, 0x7F800000, 0)            # +0, -0, +inf, -inf
    s[4] = (P * 0x00020001 + 1) | np.where(P & 1, 0x80000000, 0)                       # denormals of both signs, all distinct
    s[5] = 0x7FC00000 + 0x101 * P + 1                                                  # quiet NaNs, distinct payloads
    s[6] = (0x7F800001 + 0x10001 * P) | np.where(P & 4, 0x80000000, 0)                 # signalling NaNs of both signs
    s[7] = np.where(P % 3 == 0, s[5], np.where(P % 3 == 1, s[1], s[3]))                # a mixture
    return s.view(F32)


def _mixed(rng, n):
    """distinct values of mixed sign, magnitudes spread over 1e-3 .. 1e3"""
    v = (10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    assert len(set(v.tolist())) == n
    return v


def cancellation(rng, n):
    """a set whose true sum is about 1e-6 of the sum of magnitudes"""
    a = np.abs(_mixed(rng, n // 2)).astype(np.float64)
    v = np.concatenate([a, -(a * (1 - 2e-6))]).astype(F32)
    v = v[rng.permutation(n)]
    r = abs(v.astype(np.float64).sum()) / np.abs(v.astype(np.float64)).sum()
    assert 2e-7 < r < 5e-6, r
    return v


def num_sets(k=1):
    """8 finite sets (x k independent inputs -> [k, 8, 64]) for the arithmetic cases: ramp, three random, two cancellation,
    all negative, ties.  The halves of every set differ."""
    out = []
    for q in range(k):
        rng = np.random.default_rng(100 + q)
        s = np.zeros((8, 64), F32)
        s[0] = P + 0.5 + q
        for i in (1, 2, 3):
            s[i] = _mixed(rng, 64)
        s[4], s[5] = cancellation(rng, 64), cancellation(rng, 64)
        s[6] = -np.abs(_mixed(rng, 64))
        s[7] = rng.choice(np.array([-2.5, 0.75, 3.0, 1e-3], F32), 64)
        s[7, 32:] += F32(0.125)
        out.append(s)
    return np.stack(out)


def pred_sets():
    """predicate patterns (negative = set): none, all, alternating, one lane, random, and only lanes >= count for each count"""
    s = [np.ones(64), -np.ones(64), np.where(P & 1, -1.0, 1.0), np.where(P == 37, -1.0, 1.0), np.where(P == 5, -1.0, 1.0),
         np.where(np.random.default_rng(5).random(64) < 0.4, -1.0, 1.0)]
    s += [np.where(P >= c, -1.0, 1.0) for c in (0, 1, 31, 32, 33)]
    return np.array(s, F32)


# ------------------------------------------------------------------------------------------------------------------ definitions
def tree_row(v):
    """wave.h: one row of 16 lanes -- quad_perm xor 1, xor 2, row_half_mirror, row_mirror.  v [..., 16] float32 -> [...]"""
    l = np.arange(16)
    s1 = v + v[..., l ^ 1]
    s2 = s1 + s1[..., l ^ 2]
    s3 = s2 + s2[..., (l & 8) | (7 - (l & 7))]
    return s3[..., 15] + s3[..., 0]


def tree64(v):
    r = [tree_row(v[..., 16 * g:16 * g + 16]) for g in range(4)]
    return (r[3] + r[2]) + (r[1] + r[0])


def tree32(v):
    return tree_row(v[..., :16]) + tree_row(v[..., 16:32])


def seg8(v):
    l = np.arange(64)
    s1 = v + v[..., l ^ 1]
    s2 = s1 + s1[..., l ^ 2]
    return s2 + s2[..., (l & ~7) | (7 - (l & 7))]


def seq16(v):
    """the EMULATOR's row16_sum: lanes of the group added one after the other"""
    out = np.zeros_like(v)
    for g in range(4):
        t = np.zeros(v.shape[:-1], F32)
        for l in range(16):
            t = t + v[..., 16 * g + l]
        out[..., 16 * g:16 * g + 16] = t[..., None]
    return out


def row16(v, tree):
    if not tree:
        return seq16(v)
    return np.repeat(np.stack([tree_row(v[..., 16 * g:16 * g + 16]) for g in range(4)], -1), 16, -1)


def half_rep(f, v, half2):
    """a wave-uniform (Wave) or half-uniform (WaveH) scalar, replicated into the lanes that hold it"""
    if not half2:
        return np.repeat(f(v)[..., None], 64, -1)
    g = tree32 if f is tree64 else f
    return np.concatenate([np.repeat(g(v[..., h:h + 32])[..., None], 32, -1) for h in (0, 32)], -1)


def strided(x, count, half2):
    """lane-strided partial sums of items 0 .. count-1 (item i = word i % LW of input i // LW), then nothing: [nset, 64]"""
    LW = 32 if half2 else 64
    v = np.zeros((len(x), 64), F32)
    for h in ((0, 32) if half2 else (0,)):
        for l in range(LW):
            for n, i in enumerate(range(l, count, LW)):
                t = x[:, i // LW, h + i % LW]
                v[:, h + l] = t if n == 0 else v[:, h + l] + t
    return v


def ref_case(case, x, half2, par=0, row16_tree=False):
    """{slot: expected [nset, 64]} (uint32 for moves, float32 for arithmetic) of one case of tests/wave_prims/prim_cases.h.
    row16_tree: the row16_* family in the DEVICE's association (tree_row) instead of the emulator's sequential sum."""
    xu = x.view(np.uint32)
    v, r, lo = xu[:, 0], {}, (P & 31) if half2 else P
    half = P & 32
    mv = lambda cond, idx: np.where(cond, v[:, np.clip(idx, 0, 63)], np.uint32(0))
    if case == PL.C_ROW:
        r[0], r[1] = v[:, P ^ 1], v[:, P ^ 2]
        for n in (1, 2, 3, 4):
            r[1 + n] = mv((P & 15) >= n, P - n)                          # lane N below inside the row of 16, 0 where the row ends
            r[5 + n] = mv((P & 15) + n <= 15, P + n)
            r[9 + n] = mv(((P & 15) < 8) & ((P & 15) >= n), P - n)       # lanes 0..7 of every row receive, lanes 8..15 read 0
            r[13 + n] = mv((P & 15) < 8, P + n)
        for k in range(16):
            r[18 + k] = v[:, (P & ~15) + k]
        if half2:
            r[34] = v[:, (P & ~7) | 3]
    elif case == PL.C_PICK:
        r[0], r[1] = v[:, half | (P & 15)], v[:, half | 16 | (P & 15)]
        for k in range(32):
            r[2 + k] = v[:, half | k]
    elif case == PL.C_BCAST:
        if half2:
            for k in range(32):
                r[k] = v[:, half | k]
        else:
            for s, k in enumerate((0, 15, 16, 31, 32, 63)):
                r[s] = v[:, np.full(64, k)]
            r[6], r[7] = v[:, P & 31], v[:, 32 | (P & 31)]
        for k in range(16):
            r[32 + k] = xu[:, 1][:, (half | k) if half2 else np.full(64, k)]
    elif case == PL.C_PERM:
        src = x[:, 1].astype(np.int64)
        r[0] = np.take_along_axis(v, (half | (src & 31)) if half2 else (src & 63), 1)
        for s, n in enumerate((1, 18, 22, 26, 32) + (() if half2 else (64,))):
            r[1 + s] = mv(lo < n, half + n - 1 - lo) if half2 else mv(P < n, n - 1 - P)
    elif case == PL.C_MASK:
        neg = (x[:, 0] < 0).astype(np.uint64)
        if half2:
            r[0] = np.concatenate([np.repeat((neg[:, h:h + 32] << np.arange(32, dtype=np.uint64)).sum(1)[:, None], 32, 1)
                                   for h in (0, 32)], 1).astype(np.uint32)
            r[1] = np.zeros_like(r[0])
        else:
            b = (neg << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
            r[0] = np.repeat((b & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None], 64, 1)
            r[1] = np.repeat((b >> np.uint64(32)).astype(np.uint32)[:, None], 64, 1)
        for q, k in enumerate((0, 17, 31, 30 if half2 else 63)):
            for s, c in enumerate((lo > k, lo == k, lo < k)):
                r[2 + 3 * q + s] = np.broadcast_to(u32(c.astype(F32)), v.shape)
    elif case == PL.C_COMPACT and not half2:
        r[0] = np.zeros(v.shape, np.uint32)
        r[1] = np.full(v.shape, PL.SENTINEL, np.uint32)
        for k in range(len(x)):
            lanes = [l for l in range(min(par, 64)) if x[k, 0, l] < 0]
            r[0][k] = len(lanes)
            r[1][k, :len(lanes)] = u32(np.array(lanes, F32))
    elif case == PL.C_VSUMS:
        a, b, c = x[:, 0], x[:, 1], x[:, 2]
        r[0] = half_rep(tree64, a, half2)
        r[1], r[2], r[3] = (half_rep(tree64, t, half2) for t in (a, b, c))
        r[4] = row16(a, row16_tree)
        r[5], r[6], r[7] = (row16(t, row16_tree) for t in (a, b, c))
        r[8], r[9] = row16(b, row16_tree), row16(c, row16_tree)
        r[10], r[11] = seg8(a), seg8(c)
    elif case == PL.C_FSUMS:
        LW = 32 if half2 else 64
        rev = x.copy()                                                   # item count-1-i in the place of item i
        for h in ((0, 32) if half2 else (0,)):
            for i in range(par):
                j = par - 1 - i
                rev[:, i // LW, h + i % LW] = x[:, j // LW, h + j % LW]
        r[0] = half_rep(tree64, strided(x, par, half2), half2)
        r[1] = r[0]
        r[2] = half_rep(tree64, strided(rev, par, half2), half2)
        r[3] = half_rep(tree64, strided(-x, par, half2), half2)
        if not half2:
            items = x.reshape(len(x), -1)[:, :par]
            r[4] = np.repeat((items.max(1) if par else np.full(len(x), -np.inf, F32))[:, None], 64, 1)
    elif case == PL.C_CONTRACT:
        p = x[:, 0] * x[:, 1]                                            # separately rounded products
        r[0] = half_rep(tree64, p, half2)
        r[1] = row16(p, row16_tree)
        r[2] = r[0]
    elif case in (PL.C_FMA, PL.C_FNMA, PL.C_MUL, PL.C_RCP):
        vf, other, acc = x[:, 0], x[:, 1], x[:, 2]
        for k in range(32):
            pk = vf[:, half | k]
            if case == PL.C_RCP:
                r[k] = r[32 + k] = F32(1) / pk
                if par:                                                  # the far variant's live chain on X: x 2, x 2, x 0.25
                    r[64] = ((vf[:, half | (P & 15)] * F32(2)) * F32(2)) * F32(0.25)
            else:                                                        # the emulator / IEEE build: two roundings
                r[k] = other * pk if case == PL.C_MUL else (acc + other * pk if case == PL.C_FMA else acc - other * pk)
    return {s: (e if e.dtype == np.uint32 else u32(e)) for s, e in r.items()}


def check_slots(got, want, what):
    """got [nset, NOUT, 64] uint32 against {slot: [nset, 64]}; every slot the definition does not name still holds the sentinel"""
    for s, e in want.items():
        bad = np.argwhere(got[:, s] != e)
        assert len(bad) == 0, (what, "slot", s, "set, lane", bad[0].tolist(), hex(got[:, s][tuple(bad[0])]), hex(e[tuple(bad[0])]))
    rest = [s for s in range(got.shape[1]) if s not in want]
    assert np.all(got[:, rest] == PL.SENTINEL), (what, "a slot outside the definition was written")


# ------------------------------------------------------------------------------------------------------------------ L D L^T
def anc_mask(name):
    """pattern[i, j]: dof j is an ancestor-or-self of dof i, or the other way round (the fill pattern of A and of the LDS factor)"""
    N, tree = PL.INST[name][1], PL.INST[name][2]
    if tree is None:
        return np.ones((N, N), bool)
    par, m = PL.PARENTS[tree], np.zeros((N, N), bool)
    for i in range(N):
        j = i
        while j >= 0:
            m[i, j] = m[j, i] = True
            j = par[j]
    return m


def chains(name):
    """for every dof, its ancestor chain (self included)"""
    m = anc_mask(name)
    return [np.nonzero(m[i, :i + 1])[0] for i in range(len(m))]


def spd_on_pattern(name, sigma, seed, scaled=False):
    """A = sum_i v_i v_i^T + sigma I with v_i random on the ancestor chain of dof i (exactly on the pattern); scaled: rows and
    columns scaled by 1e-3 .. 1e3 (mixed units).  Returns the fp32-rounded A and a random b."""
    rng = np.random.default_rng(seed)
    N = PL.INST[name][1]
    A = sigma * np.eye(N)
    for c in chains(name):
        v = np.zeros(N)
        v[c] = rng.standard_normal(len(c))
        A += np.outer(v, v)
    if scaled:
        d = 10.0 ** rng.uniform(-3, 3, N)
        A = A * np.outer(d, d)
    A = np.where(anc_mask(name), A, 0.0).astype(F32)          # (symmetric: rounding is elementwise)
    return A, rng.standard_normal(N).astype(F32)


def ldlt64(A):
    """fp64 L^T D L in the kernel's elimination direction (leaves first = the highest dof first; any leaves-first order gives the
    same factor): A = U^T D U with U unit LOWER in the reversed order.  Returns (Lfac, d): Lfac[k, i] = what scratch[k * S + i] holds
    -- the multiplier of dof k's column at its ancestor i < k -- and d the pivots."""
    A = np.array(A, np.float64)
    N = len(A)
    Lf, d = np.zeros((N, N)), np.zeros(N)
    for k in range(N - 1, -1, -1):
        d[k] = A[k, k]
        Lf[k, :k] = A[k, :k] / d[k]
        A[:k, :k] -= np.outer(Lf[k, :k], Lf[k, :k]) * d[k]
    return Lf, d


def chol_systems(name):
    """the synthetic systems of one instantiation: sigma in {1, 1e-2, 1e-4} x 20 seeds, plain and row-scaled -> A [120, N, N], b [120, N]"""
    sys_ = [spd_on_pattern(name, sigma, 1000 * q + seed, scaled) for scaled in (False, True)
            for q, sigma in enumerate((1.0, 1e-2, 1e-4)) for seed in range(20)]
    return np.stack([s[0] for s in sys_]), np.stack([s[1] for s in sys_])


def chol_ratio(A, b, x):
    """gate 1: ||x - x64||_inf / ||x64||_inf in units of kappa_2(A) 2^-24, per system (x64 from the fp32-rounded A, b)"""
    out = np.zeros(len(A))
    for k in range(len(A)):
        A64, b64 = A[k].astype(np.float64), b[k].astype(np.float64)
        x64 = np.linalg.solve(A64, b64)
        out[k] = np.abs(x[k] - x64).max() / np.abs(x64).max() / (np.linalg.cond(A64) * EPS)
    return out


# ------------------------------------------------------------------------------------------------------------------ launches
WAVE_COUNTS, HALF_COUNTS = (0, 1, 17, 64, 65, 220), (0, 1, 17, 32, 33, 72)
COMPACT_COUNTS = (0, 1, 31, 32, 33, 64)


def contraction_inputs(emu):
    """Part 4: a, b [8, 64] such that fusing the multiply into the first butterfly add -- fma(a_l, b_l, round(a_l' b_l')), l' = l ^ 1,
    instead of round(a_l b_l) + round(a_l' b_l') -- changes the last bit in at least a quarter of the lanes of every set."""
    rng = np.random.default_rng(77)
    a = (rng.uniform(0.5, 2.0, (8, 64)) * rng.choice([-1.0, 1.0], (8, 64))).astype(F32)
    b = (rng.uniform(0.5, 2.0, (8, 64)) * rng.choice([-1.0, 1.0], (8, 64))).astype(F32)
    p = emu.mulf(a, b)
    fused, plain = emu.fmaf(a, b, p[:, P ^ 1]), p + p[:, P ^ 1]
    differ = (u32(fused) != u32(plain)).sum(1)
    assert np.all(differ >= 16), differ
    return a, b


def launches(emu, case, half2):
    """[(x [nset, NIN, 64], par)]: every launch of one case"""
    mv = move_sets()
    if case in (PL.C_ROW, PL.C_PICK):
        return [(emu.pack(mv), 0)]
    if case == PL.C_BCAST:
        return [(emu.pack(mv, np.roll(mv, 3, 0)), 0)]
    if case == PL.C_PERM:
        rng = np.random.default_rng(3)
        src = rng.integers(0, 64, (8, 64))
        src[0], src[1], src[2], src[3] = P, 63 - P, 63, rng.permutation(64)
        return [(emu.pack(mv, src.astype(F32)), 0)]
    if case == PL.C_MASK:
        return [(emu.pack(pred_sets()), 0)]
    if case == PL.C_COMPACT:
        return [] if half2 else [(emu.pack(pred_sets()), c) for c in COMPACT_COUNTS]
    if case == PL.C_VSUMS:
        return [(emu.pack(*num_sets(3)), 0)]
    if case == PL.C_FSUMS:
        return [(emu.pack(*num_sets(4)), c) for c in (HALF_COUNTS if half2 else WAVE_COUNTS)]
    if case == PL.C_CONTRACT:
        return [(emu.pack(*contraction_inputs(emu)), 0)]
    if case in (PL.C_FMA, PL.C_FNMA, PL.C_MUL):
        return [(emu.pack(*num_sets(3)), v) for v in (0, 1)]
    if case == PL.C_RCP:
        return [(emu.pack(*num_sets(1)), v) for v in (0, 1)]
    raise ValueError(case)


CASE_NAMES = ["row", "pick", "bcast", "perm", "mask", "compact", "vsums", "fsums", "contract", "fma", "fnma", "mul", "rcp"]


# ------------------------------------------------------------------------------------------------------------------ the real models
EXAMPLES = {"go2": "unitree_go2_trot", "h1": "unitree_h1_jog", "h1loco": "unitree_h1_loco", "allegro": "allegro_reorient",
            "allegro_dense": "allegro_reorient", "crate_climb": "unitree_go2_crate_climb", "push_crate": "unitree_h1_push_crate",
            "push_crate_dense": "unitree_h1_push_crate", "capacity_dense": "unitree_go2_trot"}


def model_systems(name):
    """The matrices the kernels really see, from the fp64 oracle at the model's initial pose: the mass matrix M (on the dof tree) and
    H = M + J^T D J over all constraint rows (robot against the world: still on the tree; the Allegro's and the push crate's couple
    moving bodies: dense).  capacity_dense: the Go2's H in the capacity-dimension square, an identity block for the dofs the model
    does not have (rollout_body.h: solve_spd_reg).  Returns A [n, N, N] float32 with exact zeros off the instantiation's pattern and
    b [n, N]."""
    import oracle as O
    from conftest import setup_case
    dc, env, model, task, cfg = setup_case(EXAMPLES[name], 16, 4)
    N, nv = PL.INST[name][1], model.nv
    assert nv == N or name == "capacity_dense"
    d = O.Oracle(model, task, cfg, np.float64).forward_dump(np.array(env._init_q, np.float64), np.zeros(nv))
    M = np.tril(d["qM"]) + np.tril(d["qM"], -1).T
    H = M + d["efc_J"].T @ (d["efc_D"][:, None] * d["efc_J"])
    if name == "capacity_dense":
        Hp = np.eye(N)
        Hp[:nv, :nv] = H
        H = Hp
    mats = {"allegro": [M], "push_crate": [M], "allegro_dense": [H], "push_crate_dense": [H], "capacity_dense": [H]}.get(name, [M, H])
    mask = anc_mask(name)
    for A in mats:
        assert np.abs(A[~mask]).max(initial=0.0) <= 1e-12 * np.abs(A).max(), (name, "the model's matrix leaves the pattern")
        assert np.linalg.eigvalsh(A).min() > 0
    rng = np.random.default_rng(9)
    return np.stack([np.where(mask, A, 0.0).astype(F32) for A in mats]), rng.standard_normal((len(mats), N)).astype(F32)


_SYSTEMS = {}


def all_systems(name):
    """synthetic + real systems of one instantiation (computed once per process; an even number, for the two halves of WaveH)"""
    if name not in _SYSTEMS:
        (A, b), (Am, bm) = chol_systems(name), model_systems(name)
        if len(Am) & 1:
            Am, bm = np.concatenate([Am, Am]), np.concatenate([bm, -bm[::-1]])
        _SYSTEMS[name] = (np.concatenate([A, Am]), np.concatenate([b, bm]))
    return _SYSTEMS[name]


def emu_chol(emu, name):
    """the emulator's results on all_systems(name), per form, and the gate constant they give: C = 4 x the emulator's worst
    ||x - x64|| / ||x64|| / (kappa_2 2^-24) on these inputs (the 4 covers the device's 1-ulp reciprocals and the product build's
    contraction against the emulator's correctly rounded arithmetic)"""
    key = ("emu", name)
    if key not in _SYSTEMS:
        A, b = all_systems(name)
        res = {f: emu.chol(name, f, A, b) for f in ((0, 1, 2) if name == "go2" else (0, 1))}
        worst = max(chol_ratio(A, b, r["x"]).max() for r in res.values())
        _SYSTEMS[key] = (res, 4.0 * worst, worst)
    return _SYSTEMS[key]
