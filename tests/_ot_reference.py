"""The yardstick of the optimal-transport tests, independent of the code under test (numpy only).  Test infrastructure.

``t_ref(X, Y, h, s)``: the contract's t_ij = fmaf(-c_ij, s, h_j) as float32, computed without an fp32 fma: c_ij is ``exact_d2`` of
tests/_knn_reference.py (the distance chain, one rounding per operation); -c * s is exact in float64 (24 + 24 significant bits); the sum
with h is rounded to float32 ONCE through Knuth's TwoSum and ``_fl32_of_sum`` (the float64 sum and its residual), never twice.
``lse_ref``: float64 log-sum-exp over the finite t of a row (-inf for a row without one).  ``topk_ref``: a stable sort of (-t, j) over the
finite t with the fill rule (-1).  ``sinkhorn_ref``: the log-domain iteration in float64 on the same float32 costs."""
import numpy as np

from tests._knn_reference import _fl32_of_sum, exact_d2


def t_from_cost(c, h, s):
    """float32 [n_q, n_c]: fl32(-c * s + h) with one rounding, from the float32 costs"""
    c, h = np.asarray(c, dtype=np.float32), np.asarray(h, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = -(c.astype(np.float64) * np.float64(np.float32(s)))
        a = np.broadcast_to(h.astype(np.float64)[None, :], p.shape)
        sm = p + a
        bb = sm - p
        e = (p - (sm - bb)) + (a - bb)
        return _fl32_of_sum(sm, e)


def t_ref(X, Y, h, s):
    return t_from_cost(exact_d2(X, Y), h, s)


def lse_ref(t):
    """float64 [n_q]: log sum_j exp(t_ij) over the finite entries of each row"""
    t = np.asarray(t, dtype=np.float64)
    out = np.full(t.shape[0], -np.inf)
    for i in range(t.shape[0]):
        v = t[i][np.isfinite(t[i])]
        if v.size:
            m = v.max()
            out[i] = m + np.log(np.exp(v - m).sum())
    return out


def topk_ref(t, k):
    """(idx int32 [n_q, k], t float32 [n_q, k]): per row the k finite entries with the largest t, equal t to the smaller j; -1 / nan fill"""
    t = np.asarray(t, dtype=np.float32)
    n_q, n_c = t.shape
    idx = np.full((n_q, k), -1, dtype=np.int32)
    tv = np.full((n_q, k), np.nan, dtype=np.float32)
    j = np.arange(n_c)
    for i in range(n_q):
        cand = j[np.isfinite(t[i])]
        order = cand[np.lexsort((cand, -t[i][cand].astype(np.float64)))][:k]
        idx[i, :len(order)] = order
        tv[i, :len(order)] = t[i][order]
    return idx, tv


def _lse_rows(m):
    with np.errstate(invalid="ignore", divide="ignore"):
        top = m.max(1)
        safe = np.where(np.isfinite(top), top, 0.0)
        return np.where(np.isfinite(top), safe + np.log(np.exp(m - safe[:, None]).sum(1)), -np.inf)


def sinkhorn_ref(c, s, log_a, log_b, n_iter):
    """float64 potentials (phi [n0], psi [n1]) after ``n_iter`` iterations from zero on the float32 costs ``c`` [n0, n1]:
    phi = -lse_j(-c s + psi + log b), then psi = -lse_i(-c s + phi + log a)"""
    m = -(np.asarray(c, dtype=np.float32).astype(np.float64) * np.float64(np.float32(s)))
    log_a, log_b = np.asarray(log_a, dtype=np.float64), np.asarray(log_b, dtype=np.float64)
    phi, psi = np.zeros(m.shape[0]), np.zeros(m.shape[1])
    for _ in range(n_iter):
        phi = -_lse_rows(m + (psi + log_b)[None, :])
        psi = -_lse_rows(m.T + (phi + log_a)[None, :])
    return phi, psi
