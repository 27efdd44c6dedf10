"""NumPy statement of the elite update rule (include/dial_mpc.h: DIAL_UPDATE_ELITE), from the contract alone.

Order the B candidates of a plan by reward, best first: a NaN ranks below every number (-inf included), -0 equals +0, equal rewards
are ordered by ascending index.  The first K are the elites; each gets the fp32 quotient 1.0f / (float)K, every other candidate +0.0f.
"""
import numpy as np


def reward_key_ref(rews_f32) -> np.ndarray:
    """An int64 key per reward whose order is the contract's: NaN -> -1 (below everything), -0 -> the key of +0, otherwise the fp32
    bit pattern with the usual flip (negative: all bits, non-negative: the sign bit), so that larger rewards have larger keys."""
    r = np.ascontiguousarray(rews_f32, dtype=np.float32)
    bits = r.view(np.uint32).astype(np.int64)
    bits = np.where(bits == 0x80000000, 0, bits)
    key = np.where(bits & 0x80000000, (~bits) & 0xFFFFFFFF, bits | 0x80000000)
    return np.where(np.isnan(r), -1, key)


def elite_order_ref(rews_f32) -> np.ndarray:
    """The candidates' indices, best first: a stable sort on (key descending, index ascending)."""
    return np.argsort(-reward_key_ref(rews_f32), kind="stable")


def elite_weights_ref(rews_f32, K: int) -> np.ndarray:
    """weights [B] float32 of one plan's rewards [B] under the elite rule with elite count K, 1 <= K <= B."""
    r = np.ascontiguousarray(rews_f32, dtype=np.float32)
    assert r.ndim == 1 and 1 <= int(K) <= r.size, (r.shape, K)
    w = np.zeros(r.size, np.float32)
    w[elite_order_ref(r)[:int(K)]] = np.float32(1.0) / np.float32(int(K))   # one fp32 division
    return w
