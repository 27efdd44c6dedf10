"""fp64 restatements of the planner's reductions (K4a softmax, K4b weighted sums, the mean action regenerated from the noise, the K5
shift) with error bounds derived from the kernels' own summation orders (csrc/dial_hip.hip), and access to a context's device scratch
for the GPU tests (tests/test_gpu_planner_kernels.py).

Error model: fp32 unit roundoff u = 2^-24; a sum of k terms accumulated in some fixed order is off by at most gamma(k) = k u / (1 - k u)
times the sum of the magnitudes of its terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).  Every
bound below names the depth k of the kernel's actual summation tree."""
import ctypes

import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
FLT_MIN = float(np.finfo(np.float32).tiny)
WK_THREADS, WSUM_CHUNKS, YB_CHUNKS = 1024, 64, 128   # csrc/dial_hip.hip


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------------------- K4a (softmax)
def softmax_ref(rews, temp):
    """dial_core.py:121-128 in fp64 on the given (fp32) mean rewards, last entry = the mean trajectory's: weights and the logits
    a_n = logp0_n - max logp0 (<= 0)."""
    r = np.asarray(rews, np.float64)
    logp = (r - r[-1]) / r.std() / float(temp)
    a = logp - logp.max()
    w = np.exp(a)
    return w / w.sum(), a, logp


def softmax_bound(rews, temp):
    """Per-entry bound on |w_gpu - w_fp64| for weights_kernel (fp32 path).  Its reductions: every thread adds its ceil(B / 1024)
    strided entries, the wavefront's DPP butterfly adds 6 levels, the 16 wavefront partials are added in order: depth
    d = ceil(B / 1024) + 6 + 16.  Propagated:
      mean        |dmu| <= gamma(d + 1) mean|r|
      variance    sum (r - mu_f)^2 = S + B (mu - mu_f)^2 (the mean's error enters squared), each term rounded twice, summed at depth d
      std         half the variance's relative error, plus divide / approximate sqrt (4 u)
      logit       l_n - mx = (r_n - r_max) / std / temp: the std's relative error times |l_n - mx|, 4 u of |l_n| and |mx| for the
                  subtraction and the two divisions of each, u |l_n - mx| for their difference
      exp         approximate exp2 of x log2(e): 2 u + u |x|
      normaliser  its terms' errors weighted by the weights, gamma(d) for the sum, 3 u for the final division.
    Absolute floor 2 FLT_MIN: weights below the normal range may be flushed to zero."""
    r = np.asarray(rews, np.float64)
    B = r.size
    w, a, logp = softmax_ref(r, temp)
    d = -(-B // WK_THREADS) + 6 + 16
    S = float(((r - r.mean()) ** 2).sum())
    dmu = gamma(d + 1) * float(np.abs(r).mean())
    dsig = 0.5 * (gamma(d + 3) + B * dmu * dmu / S) + 4 * U
    mx = float(logp.max())
    E = np.abs(a) * dsig + 4 * U * (np.abs(logp) + abs(mx)) + 2 * U * np.abs(a) + 2 * U
    rel = E + float((w * E).sum()) + gamma(d) + 3 * U
    return w * np.expm1(rel) + 2 * FLT_MIN


# ---------------------------------------------------------------------------------------------------------------- K4b (weighted sums)
def wsum_depth(n_rows):
    """wsum_partial_kernel: 64 row chunks of ceil(n_rows / 64) rows, every 4th row per wavefront (one fused multiply-add each), the 4
    wavefront partials added in LDS; wsum_final_kernel adds the 64 chunks in order."""
    per = -(-n_rows // WSUM_CHUNKS)
    return -(-per // 4) + 1 + 3 + WSUM_CHUNKS


def wsum_ref(w, X):
    """fp64 sum_n w_n X[n, :] and its bound gamma(k) sum_n |w_n X[n, :]| (+ FLT_MIN per term: flushed products)."""
    w = np.asarray(w, np.float64)
    X = np.asarray(X, np.float64).reshape(w.size, -1)
    k = wsum_depth(w.size)
    return w @ X, gamma(k) * (np.abs(w) @ np.abs(X)) + w.size * FLT_MIN


# ---------------------------------------------------------------------------------------------------------------- mean action
def ybar_depth(n_total):
    """ybar_partial_kernel: 128 row chunks of ceil((n_total + 1) / 128) rows, every 16th row per thread, 16 row lanes added in LDS;
    ybar_final_kernel adds the 128 chunks in order."""
    per = -(-(n_total + 1) // YB_CHUNKS)
    return -(-per // 16) + 16 + YB_CHUNKS + 1


def candidate_nodes(eps, Ybar, sigma, nu):
    """dial_core.py:110-115 in fp64: rows [n_total + 1, C] -- clip(eps sigma_k + Ybar) with node 0 held at Ybar[0], the mean row
    clip(Ybar) -- plus the magnitude of what was rounded before the clip (|eps sigma_k| + |Ybar|; zero where nothing is)."""
    eps = np.asarray(eps, np.float64)
    n, C = eps.shape
    Y = np.asarray(Ybar, np.float64).reshape(-1)
    s = np.asarray(sigma, np.float64).reshape(-1)
    sc = np.repeat(s if s.size > 1 else np.full(C // nu, s[0]), nu)
    v = eps * sc + Y
    mag = np.abs(eps * sc) + np.abs(Y)
    v[:, :nu] = Y[:nu]
    mag[:, :nu] = 0.0
    rows = np.clip(np.concatenate([v, Y[None]]), -1.0, 1.0)
    return rows, np.concatenate([mag, np.zeros((1, C))]), sc


def ybar_ref(w, eps, Ybar, sigma, nu, eps_err=None):
    """The regenerated mean action in fp64 and its bound: the summation (depth ybar_depth), the 2 u rounding of eps sigma + Ybar before
    the clip, and -- in-kernel noise -- sum_n w_n sigma_k |eps_gpu - eps_ref| (eps_err: a bound of that per draw; clip is 1-Lipschitz)."""
    rows, mag, sc = candidate_nodes(eps, Ybar, sigma, nu)
    w = np.asarray(w, np.float64)
    n_total = rows.shape[0] - 1
    bound = gamma(ybar_depth(n_total)) * (np.abs(w) @ np.abs(rows)) + 2 * U * (w @ mag) + rows.shape[0] * FLT_MIN
    if eps_err is not None:
        e = np.array(eps_err, np.float64)
        e[:, :nu] = 0.0
        bound = bound + (w[:-1] @ e) * sc
    return w @ rows, bound


# ---------------------------------------------------------------------------------------------------------------- K5 (shift)
def shift_ref(W, V, Y):
    """dial_core.py:160-166 in fp64: u = W Y; u = roll(u, -1); u[-1] = 0; Y' = V u -- with the fp32 matrices the kernel is given.
    Bound: the kernel's two dot products (Hnode + 1 and Hsample + 1 terms)."""
    W = np.asarray(W, np.float64)
    V = np.asarray(V, np.float64)
    Y = np.asarray(Y, np.float64)
    u = W @ Y
    u = np.roll(u, -1, axis=0)
    u[-1] = 0.0
    ua = np.abs(W) @ np.abs(Y)
    ua = np.roll(ua, -1, axis=0)
    ua[-1] = 0.0
    g1, g2 = gamma(W.shape[1]), gamma(W.shape[0])
    return V @ u, (g1 + g2 + g1 * g2) * (np.abs(V) @ ua) + FLT_MIN


def cfg_matrices(cfg):
    """cfg.W [Hsample + 1, Hnode + 1] and cfg.V [Hnode + 1, Hsample + 1] as the kernel reads them (fp32)."""
    T, Hn1 = cfg.Hsample + 1, cfg.Hnode + 1
    W = np.array([[cfg.W[t][k] for k in range(Hn1)] for t in range(T)], np.float32)
    V = np.array([[cfg.V[k][t] for t in range(T)] for k in range(Hn1)], np.float32)
    return W, V


# ---------------------------------------------------------------------------------------------------------------- device scratch
SCRATCH = ("Y0s", "rewss", "qss", "qdss", "xss", "weights")


def scratch_ptrs(ctx):
    """Device addresses of the context's rollout scratch (dial_debug_scratch)."""
    ptrs = [ctypes.c_void_p() for _ in SCRATCH]
    assert ctx.lib.dial_debug_scratch(ctx.h, *[ctypes.byref(p) for p in ptrs]) == 0
    return {k: p.value for k, p in zip(SCRATCH, ptrs)}


def row_width(ctx, name):
    T, Hn1 = ctx.cfg.Hsample + 1, ctx.cfg.Hnode + 1
    return dict(Y0s=Hn1 * ctx.nu, rewss=T, qss=T * ctx.nq, qdss=T * ctx.nv, xss=T * ctx.nx, weights=1)[name]


def _hip():
    return ctypes.CDLL("libamdhip64.so")


def download(ctx, name, rows):
    """Host copy of the first `rows` rows of scratch buffer `name`."""
    import torch
    host = np.empty((rows, row_width(ctx, name)), np.float32)
    torch.cuda.synchronize()
    rc = _hip().hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(scratch_ptrs(ctx)[name]), ctypes.c_size_t(host.nbytes),
                          ctypes.c_int(2))
    assert rc == 0, f"hipMemcpy of scratch {name} failed ({rc})"
    return host


def upload(ctx, name, rows, cap):
    """Write host rows [n, width] into scratch buffer `name` (n <= cap, the rows the context holds)."""
    import torch
    a = np.ascontiguousarray(rows, np.float32).reshape(-1, row_width(ctx, name))
    assert a.shape[0] <= cap, (name, a.shape, cap)
    torch.cuda.synchronize()
    rc = _hip().hipMemcpy(ctypes.c_void_p(scratch_ptrs(ctx)[name]), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes),
                          ctypes.c_int(1))
    assert rc == 0, f"hipMemcpy to scratch {name} failed ({rc})"
    torch.cuda.synchronize()


def worst(err, bound):
    """Largest error as a fraction of its bound."""
    return float(np.max(np.abs(err) / bound)) if np.size(err) else 0.0


def isclose_to_bound(got, ref, bound):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - ref) <= bound))


def ulp_sensitivity(r, t, L, z):
    """Box-Muller's sensitivity to the device's approximate fp32 log / sqrt / sin / cos, in units of u, per draw
    (z = r cos t or r sin t, r = sqrt(-2 L), L = ln u1, t = 6.2831855f u2):
      log    an absolute error of about u (1 + |L|) in L moves r by |dL| / r -- unbounded as u1 -> 1, where r -> 0 --, z by that
             times |cos t| <= 1
      sqrt   relative: u r
      trig   the argument is reduced in revolutions (t / 2 pi rounded): absolute u (1 + t) in cos / sin, times r
      product  u |z|.
    u1 = 1 exactly (r = 0) gives z = 0 exactly on both sides and is checked separately."""
    with np.errstate(divide="ignore"):
        s = (1.0 + np.abs(L)) / r + r + r * (1.0 + t) + np.abs(z)
    return np.where(r > 0, s * U, 0.0)

