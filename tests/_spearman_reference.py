"""The int64 reference of the rank transform (spv_rank_values_stage / spv_rank_values, ``rank_ops.rank_transform``) and of the Spearman
tables built on it, on the host.

Keys are formed by ``tests._rank_reference.keys_of`` (numpy's float32 multiply, one rounding: the kernel's key image).  For keys
[n, p]:  c = 2 * scipy.stats.rankdata(keys, "average", axis=0) - (n + 1), an integer (doubled midranks are integers, exact in fp64 far
beyond 2^20), held as int64;  C = c.T @ c in int64;  T[j] = the sum of t^3 - t over the runs of equal keys of column j, from
``np.unique`` counts.  Two identities are asserted here before anything is returned: every column of c sums to 0, and
3 * diag(C) == n^3 - n - T."""
import numpy as np


def rank_block(keys: np.ndarray) -> np.ndarray:
    """keys fp32 [n, p] -> c int64 [n, p], c[i, j] = 2 * average rank of keys[i, j] in column j - (n + 1)"""
    from scipy.stats import rankdata

    keys = np.asarray(keys)
    assert keys.dtype == np.float32 and keys.ndim == 2
    n = keys.shape[0]
    doubled = 2.0 * rankdata(keys, "average", axis=0)
    assert (doubled == np.round(doubled)).all()
    c = doubled.astype(np.int64) - (n + 1)
    assert (c.sum(0) == 0).all()
    return c


def tie_terms(keys: np.ndarray) -> np.ndarray:
    """keys [n, p] -> T int64 [p]: the sum of t^3 - t over the runs of equal keys of every column"""
    out = np.zeros(keys.shape[1], np.int64)
    for j in range(keys.shape[1]):
        t = np.unique(keys[:, j], return_counts=True)[1].astype(np.int64)
        out[j] = int((t ** 3 - t).sum())
    return out


def spearman_tables(keys: np.ndarray):
    """keys fp32 [n, p] -> (c int64 [n, p], C = c.T @ c int64 [p, p], T int64 [p])"""
    c = rank_block(keys)
    n = c.shape[0]
    C = c.T @ c
    T = tie_terms(np.asarray(keys))
    assert C.dtype == np.int64 and (3 * np.diagonal(C) == n ** 3 - n - T).all()
    return c, C, T
