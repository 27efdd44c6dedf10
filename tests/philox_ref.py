"""NumPy restatement of the in-kernel noise: Philox4x32-10 (Salmon et al., SC'11) + Box-Muller, as csrc/philox.h and rng_fill_kernel
compute it.  One Philox call yields the 4 draws of element quad q of sample n: counter = (n, q, iteration, 0), key = (seed_lo, seed_hi).

The uniforms are formed in fp32 exactly as normal_quad forms them, ((float)(u >> 8) + 0.5f) / 2^24 -- the top value rounds to 2^24,
so u1 can be exactly 1 and the normal exactly 0 -- and so is the argument of the trigonometric functions, 6.2831855f * u2.  From there
on the normals are computed in fp64: the device's approximate fp32 log / sqrt / sin / cos are what a test measures against this."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key bumps (Weyl sequence)
TWO_PI_F32 = np.float32(6.283185307179586)
INV_2_24 = np.float32(1.0 / 16777216.0)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint32 arrays (broadcast): counter words c0..c3, key words k0, k1 -> the four output words."""
    c = [np.asarray(x, np.uint64) & 0xFFFFFFFF for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0 = np.asarray(k0, np.uint64) & 0xFFFFFFFF
    k1 = np.asarray(k1, np.uint64) & 0xFFFFFFFF
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & lo, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & lo
        k0 = (k0 + np.uint64(W0)) & lo
        k1 = (k1 + np.uint64(W1)) & lo
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def words(n, q, it, seed):
    """Raw words for (sample n, quad q, iteration it, 64-bit seed): uint32 array [..., 4]."""
    seed = int(seed)
    w = philox4x32_10(n, q, np.uint64(it & 0xFFFFFFFF), 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack(w, -1)


def uniforms(w):
    """normal_quad's fp32 uniforms of raw words w[..., 4]: u1 (words 0, 2) and u2 (words 1, 3), each [..., 2]."""
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * INV_2_24
    return u[..., 0::2], u[..., 1::2]


def box_muller(u1, u2):
    """fp64 normals from the fp32 uniforms [..., 2] -> z[..., 4] in normal_quad's order (r cos, r sin) per pair, and r, the fp32
    argument t = 6.2831855f * u2 and L = ln u1 (what the gate's sensitivity model needs)."""
    L = np.log(u1.astype(np.float64))
    r = np.sqrt(-2.0 * L)
    t = (TWO_PI_F32 * u2).astype(np.float64)          # formed in fp32, as on the device
    z = np.empty(u1.shape[:-1] + (4,), np.float64)
    z[..., 0::2] = r * np.cos(t)
    z[..., 1::2] = r * np.sin(t)
    return z, r, t, L


def quad_keys(n_begin, n_count, C):
    """(n, q) index arrays of rng_fill's quads: samples n_begin .. n_begin + n_count, quads of C elements."""
    nq = (C + 3) // 4
    n = np.repeat(np.arange(n_begin, n_begin + n_count, dtype=np.uint64), nq)
    q = np.tile(np.arange(nq, dtype=np.uint64), n_count)
    return n, q, nq


def normals(seed, counter, n_begin, n_count, C):
    """fp64 restatement of dial_rng_fill: eps[n - n_begin, c] for n_count samples of C (= (Hnode + 1) nu) elements, plus the per-element
    r, t, L of the Box-Muller pair each element came from (all [n_count, C])."""
    n, q, nq = quad_keys(n_begin, n_count, C)
    z, r, t, L = box_muller(*uniforms(words(n, q, counter, seed)))
    pick = lambda a: np.repeat(a, 2, -1).reshape(n_count, nq * 4)[:, :C]   # noqa: E731  (the pair of element e is e // 2)
    return z.reshape(n_count, nq * 4)[:, :C], pick(r), pick(t), pick(L)


def philox_normal(seed, counter, n_count, C, n_begin=0):
    """The draws dial_rng_fill materialises, as fp32 (what the CPU oracle is fed with in place of the device's noise; the device's
    approximate log / sin / cos differ in the last bits)."""
    return normals(seed, counter, n_begin, n_count, C)[0].astype(np.float32)
