"""The yardstick of the k-nearest-neighbour tests, independent of the code under test.  Test infrastructure.

``exact_d2(Q, C)``: the squared distance as the contract of spv_knn defines it (include/spvipes_hip.h) -- acc = +0, then for t ascending
u = fl32(q[t] - c[t]) and acc = fl32(u * u + acc), ONE rounding per operation -- computed without an fp32 fma:

  * u: numpy's float32 subtraction is the IEEE operation itself;
  * u * u is exact in float64 (24 + 24 significant bits);
  * s = fl64(u * u + acc) with its residual e from Knuth's TwoSum, so u * u + acc == s + e exactly, |e| <= ulp64(s) / 2;
  * fl32(s + e) equals fl32(s) unless s sits exactly on the midpoint of two neighbouring float32 values and e != 0 (any other s is
    at least one ulp64 away from every midpoint, more than |e|, so s + e rounds the way s does; an s that is a float32 value stays the
    nearest one).  On a midpoint the tie that fl32(s) broke to even is no tie: the result is the neighbour on e's side.

``exact_d2_fraction`` is the same chain in rational arithmetic, value by value (slow: small cases only); tests/test_knn_host_cpu.py holds
the vectorised form to it.  ``knn_ref``: ``np.lexsort`` on (distance, index) with the fill rule."""
from fractions import Fraction

import numpy as np


def _fl32_of_sum(s, e):
    """fl32(s + e) for float64 s and its TwoSum residual e"""
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        toward = np.where(s > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        other = np.nextafter(r, toward)
        o64 = other.astype(np.float64)
        mid = np.isfinite(s) & np.isfinite(r64) & np.isfinite(o64) & (s != r64) & ((s - r64) == (o64 - s))
        to_other = mid & np.isfinite(e) & (e != 0) & ((e > 0) == (o64 > r64))
    return np.where(to_other, other, r).astype(np.float32)


def exact_d2(Q, C):
    """float32 [n_q, n_c]: the contract's distance for every (query, candidate) pair"""
    Q, C = np.asarray(Q, dtype=np.float32), np.asarray(C, dtype=np.float32)
    assert Q.ndim == 2 and C.ndim == 2 and Q.shape[1] == C.shape[1]
    acc = np.zeros((Q.shape[0], C.shape[0]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(Q.shape[1]):
            u = (Q[:, t, None] - C[None, :, t]).astype(np.float64)   # the float32 difference, widened exactly
            p, a = u * u, acc.astype(np.float64)
            s = p + a
            bb = s - p
            e = (p - (s - bb)) + (a - bb)
            acc = _fl32_of_sum(s, e)
    return acc


def round_fraction_f32(x: Fraction) -> np.float32:
    """the float32 nearest to a non-negative rational, ties to even (inf beyond the range)"""
    assert x >= 0
    if x == 0:
        return np.float32(0.0)
    n, d = x.numerator, x.denominator
    e = n.bit_length() - d.bit_length()          # 2^(e-1) < x < 2^(e+1)
    if Fraction(2) ** e > x:
        e -= 1                                    # 2^e <= x < 2^(e+1)
    q = max(e - 23, -149)                         # the exponent of the last place (subnormals: fixed at 2^-149)
    scaled = x / Fraction(2) ** q
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    v = Fraction(m) * Fraction(2) ** q
    if v >= Fraction(2) ** 128:
        return np.float32(np.inf)
    return np.float32(float(v))                   # m has at most 25 bits: float() and float32() are exact here


def exact_d2_fraction(q, c) -> np.float32:
    """one pair's distance in rational arithmetic (finite inputs)"""
    q, c = np.asarray(q, dtype=np.float32), np.asarray(c, dtype=np.float32)
    acc = np.float32(0.0)
    with np.errstate(over="ignore"):
        for t in range(q.shape[0]):
            u = np.float32(q[t] - c[t])
            if not np.isfinite(u) or not np.isfinite(acc):
                return np.float32(np.inf)
            acc = round_fraction_f32(Fraction(float(u)) * Fraction(float(u)) + Fraction(float(acc)))
    return acc


def knn_ref(Q, C, k, exclude=None, d2=None):
    """(idx int32 [n_q, k], dist float32 [n_q, k]): per query the k candidates with the smallest (d, j), ascending; a candidate whose d is
    not < +inf and candidate exclude[i] are left out; the remaining slots are -1 / +inf.  ``d2``: ``exact_d2(Q, C)`` if already at hand."""
    d = exact_d2(Q, C) if d2 is None else d2
    n_q, n_c = d.shape
    idx = np.full((n_q, k), -1, dtype=np.int32)
    dist = np.full((n_q, k), np.inf, dtype=np.float32)
    j = np.arange(n_c)
    for i in range(n_q):
        with np.errstate(invalid="ignore"):
            ok = d[i] < np.inf
        if exclude is not None:
            ok &= j != int(exclude[i])
        cand = j[ok]
        order = cand[np.lexsort((cand, d[i][cand]))][:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = d[i][order]
    return idx, dist
