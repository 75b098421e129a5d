"""The yardstick of the transport-projection tests, independent of the code under test (numpy only).  Test infrastructure.

``project_ref(t, V)``: per row of ``t`` (itself ``tests/_ot_reference.t_ref``) the float64 softmax-weighted mean of the rows of ``V``
over the finite t -> (out float64 [n_q, n_v], L float64 [n_q]); a NaN row and -inf where a row has no finite t.
``project_emulated(t, V, chunks, block)``: the kernel's own sequence of float32 operations (csrc/spv_ot_project.h: otproj_update per
candidate in ascending order within each chunk of knn_chunk's plan, otproj_merge over the chunks in order, one correctly rounded
division) with a correctly rounded exp -> (out float32 [n_q, n_v], L float32 [n_q]).  This interpreter has no ``math.fma``, so a float32
fma is the exact float64 product, Knuth's TwoSum with the addend and ONE rounding of the pair to float32 (``_fl32_of_sum``), the
route ``tests/_ot_reference.py`` takes.  ``block`` is the kernel's column block: columns are walked block by block as the kernel walks
them; a column's operations do not depend on it.
``project_bound(t, V, n_chain, n_split)``: the error bound tests/test_gpu_ot_project.py derives, per entry, float64 [n_q, n_v]."""
import numpy as np

from tests._knn_reference import _fl32_of_sum

U = 2.0 ** -24
F32 = np.float32


def _softmax(t):
    """(p float64 [n_q, n_c] with zeros at the t that are not finite, y = max - t there (0 elsewhere), L)"""
    t = np.asarray(t, dtype=np.float64)
    fin = np.isfinite(t)
    top = np.where(fin, t, -np.inf).max(1, initial=-np.inf)
    safe = np.where(np.isfinite(top), top, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(fin, safe[:, None] - t, 0.0)
        w = np.where(fin, np.exp(-y), 0.0)
    S = w.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = w / S[:, None]
        L = np.where(S > 0, safe + np.log(S), -np.inf)
    return p, y, L


def project_ref(t, V):
    p, _, L = _softmax(t)
    V = np.asarray(V, dtype=np.float64)
    out = np.full((p.shape[0], V.shape[1]), np.nan)
    some = np.isfinite(L)
    out[some] = p[some] @ V if V.shape[0] else np.nan
    return out, L


def _fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays, one rounding"""
    with np.errstate(over="ignore", invalid="ignore"):
        a, b, c = (x.astype(np.float64) for x in np.broadcast_arrays(a, b, c))
        p = a * b   # exact: 24 + 24 significant bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        return _fl32_of_sum(s, e)


def _exp32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(x.astype(np.float64)).astype(F32)


def _scan(t, V, c0, c1):
    """the state (m, S, acc) of every row after the candidates [c0, c1) in ascending order: otproj_update"""
    n_q, n_v = t.shape[0], V.shape[1]
    m, S, acc = np.full(n_q, -np.inf, F32), np.zeros(n_q, F32), np.zeros((n_q, n_v), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(c0, c1):
            tj = t[:, j]
            fin = np.abs(tj) < np.inf
            d = (tj - m).astype(F32)
            e = _exp32(-np.abs(d))
            up = fin & (d > 0)
            rise = _fma32(acc, e[:, None], V[j][None, :])
            stay = _fma32(e[:, None], V[j][None, :], acc)
            acc = np.where(up[:, None], rise, np.where(fin[:, None], stay, acc)).astype(F32)
            S = np.where(up, _fma32(S, e, F32(1)), np.where(fin, (S + e).astype(F32), S)).astype(F32)
            m = np.where(up, tj, m).astype(F32)
    return m, S, acc


def _merge(a, p):
    """otproj_merge: the state p of a later chunk joins a"""
    (m, S, acc), (pm, pS, pacc) = a, p
    with np.errstate(invalid="ignore", over="ignore"):
        later = pm > m
        other = ~later & (pS > 0)
        e = _exp32(np.where(later, m - pm, pm - m).astype(F32))
        acc = np.where(later[:, None], _fma32(acc, e[:, None], pacc), np.where(other[:, None], _fma32(pacc, e[:, None], acc), acc)).astype(F32)
        S = np.where(later, _fma32(S, e, pS), np.where(other, _fma32(pS, e, S), S)).astype(F32)
        m = np.where(later, pm, m).astype(F32)
    return m, S, acc


def project_emulated(t, V, chunks=1, block=32):
    t, V = np.asarray(t, dtype=F32), np.asarray(V, dtype=F32)
    n_q, n_c = t.shape
    per = -(-n_c // chunks) if n_c else 0
    out = np.empty((n_q, V.shape[1]), F32)
    L = None
    for v0 in range(0, V.shape[1], block):
        Vb = V[:, v0:v0 + block]
        if chunks == 1:
            st = _scan(t, Vb, 0, n_c)
        else:
            st = (np.full(n_q, -np.inf, F32), np.zeros(n_q, F32), np.zeros((n_q, Vb.shape[1]), F32))
            for c in range(chunks):
                st = _merge(st, _scan(t, Vb, min(c * per, n_c), min((c + 1) * per, n_c)))
        m, S, acc = st
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, v0:v0 + block] = (acc.astype(np.float64) / S.astype(np.float64)[:, None]).astype(F32)   # 24-bit operands: the double rounding is innocuous
            if L is None:
                L = np.where(S > 0, (m + np.log(S.astype(np.float64)).astype(F32)).astype(F32), F32(-np.inf)).astype(F32)
    return out, L


def project_bound(t, V, n_chain, n_split):
    """|out - ref| may reach, per entry (tests/test_gpu_ot_project.py derives it; ``n_chain`` candidates per chunk, ``n_split`` chunks):
      (3 n_chain + 4 n_split + 18) u A  +  2.5 u sum_j p_j y_j |V_jv|  +  ((3 n_chain + 4 n_split + 2.5 ln(n_c + 1) + 18) u + 2 u) |ref|
    with p the float64 softmax, y_j = max_k t_k - t_j, A = sum_j p_j |V_jv| and ref = sum_j p_j V_jv"""
    p, y, _ = _softmax(t)
    V = np.asarray(V, dtype=np.float64)
    n_c = V.shape[0]
    A, ref, H = p @ np.abs(V), p @ V, (p * y) @ np.abs(V)
    g = 3 * n_chain + 4 * n_split + 18
    return g * U * A + 2.5 * U * H + ((g + 2.5 * np.log(n_c + 1.0)) * U + 2 * U) * np.abs(ref)
