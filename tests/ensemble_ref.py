"""The aggregation step of robust planning over a model ensemble (csrc/plan_ens_kernel.h, dial_set_plan_ensemble) restated in NumPy
fp64: raw fp32 rewards [R, ...] -> one fp32 reward per candidate.

    mean   the fp64 sum in index order r = 0 .. R - 1, divided by float(R), rounded once to fp32
    min    the smallest x_r
    cvar   k = clamp(ceil(alpha R), 1, R); the k smallest values in ascending order, ties broken by the lower r, summed in fp64 in
           that order, divided by float(k), rounded once to fp32

Every fp32 value is exact in fp64 and the sums are formed term by term in the stated order, so a kernel that follows the statement
agrees with this file bit for bit.  NaNs are outside the statement."""
import math

import numpy as np

AGGREGATES = ("mean", "min", "cvar")


def cvar_k(alpha, R):
    """The size of the CVaR tail.  alpha arrives at the library as an fp32 number: it is rounded to fp32 first, as the C ABI's float
    argument is."""
    return min(max(int(math.ceil(float(np.float32(alpha)) * R)), 1), int(R))


def aggregate(raw, mode, alpha=1.0):
    """raw [R, ...] float32 -> float32 [...]."""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32 and raw.ndim >= 1 and mode in AGGREGATES
    R = raw.shape[0]
    x = raw.reshape(R, -1).astype(np.float64)
    C = x.shape[1]
    if mode == "mean":
        acc = np.zeros(C, np.float64)
        for r in range(R):
            acc = acc + x[r]
        out = (acc / float(R)).astype(np.float32)
    else:
        k = 1 if mode == "min" else cvar_k(alpha, R)   # (the smallest x_r: the first of the smallest values, zeros' signs included)
        order = np.argsort(x, axis=0, kind="stable")   # ascending by value, equal values in index order
        xs = np.take_along_axis(x, order, axis=0)
        acc = np.zeros(C, np.float64)
        for j in range(k):
            acc = acc + xs[j]
        out = (acc / float(k)).astype(np.float32)
    return out.reshape(raw.shape[1:])
