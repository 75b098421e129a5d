"""The int64 reference of the rank-sum tables (spv_rank_stage / spv_rank_sums, ``rank_ops.rank_sums``), on the host.

Keys are formed by numpy's float32 multiply, one rounding, exactly the kernel's key image.  ``rank2`` is computed twice,
independently -- from ``2 * scipy.stats.rankdata(v, "average")`` (doubled midranks are integers, exact in fp64 far beyond 2^20) and
from a plain sort with a count of the smaller and of the smaller-or-equal keys -- and the two are asserted equal before either is
returned.  ``ties`` is the sum of t^3 - t over the runs of equal keys."""
import numpy as np


def keys_of(counts, w=None) -> np.ndarray:
    """counts [n, n_sel] (uint16 or float32, one row per LIST position) -> the fp32 keys: float32(count) * w[p], one fp32 multiply"""
    c = np.asarray(counts).astype(np.float32)
    if w is None:
        return c
    w = np.asarray(w)
    assert w.dtype == np.float32
    k = c * w[:, None]
    assert k.dtype == np.float32
    return k


def rank_tables(keys: np.ndarray, seg, n_seg: int):
    """keys fp32 [n, n_sel], seg int [n] (a code outside [0, n_seg) is ranked but counted in no sum) ->
    (rank2 int64 [n_seg, n_sel], ties int64 [n_sel])"""
    from scipy.stats import rankdata

    keys, seg = np.asarray(keys), np.asarray(seg).astype(np.int64)
    assert keys.dtype == np.float32 and keys.ndim == 2 and seg.shape == (keys.shape[0],)
    n, n_sel = keys.shape
    inside = (seg >= 0) & (seg < n_seg)
    by_rankdata, by_counting = np.zeros((n_seg, n_sel), np.int64), np.zeros((n_seg, n_sel), np.int64)
    ties = np.zeros(n_sel, np.int64)
    for j in range(n_sel):
        v = keys[:, j]
        doubled = 2.0 * rankdata(v, "average")
        assert (doubled == np.round(doubled)).all()
        np.add.at(by_rankdata[:, j], seg[inside], doubled.astype(np.int64)[inside])
        s = np.sort(v)
        term = np.searchsorted(s, v, "left").astype(np.int64) + np.searchsorted(s, v, "right").astype(np.int64) + 1   # L + U + 1
        np.add.at(by_counting[:, j], seg[inside], term[inside])
        t = np.unique(v, return_counts=True)[1].astype(np.int64)
        ties[j] = int((t ** 3 - t).sum())
    assert (by_rankdata == by_counting).all()
    return by_counting, ties
