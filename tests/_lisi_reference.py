"""The yardstick of the LISI tests, written from the contract of spv_lisi (include/spvipes_hip.h), not from the kernel.  Test infrastructure.

Per row of a neighbour list (``idx`` [n, k], ``dist`` [n, k]: SQUARED fp32 distances, ascending, -1 / +inf an empty slot), in float64:
r_j = float64(float32(sqrt(dist_j))) -- numpy's float32 square root is the IEEE operation, correctly rounded --, d_j = r_j - r_0; beta from 1,
H = log S + beta T / S with S = sum e_j, T = sum d_j e_j, e_j = exp(-beta d_j); stop at |H - log(perplexity)| < 1e-5 or after 50 updates
(beta doubles / halves while its upper / lower bound is infinite, else goes to the midpoint); p_j = e_j / S; simpson = sum over the labels
of (sum of the label's p_j)^2; lisi = 1 / simpson.  A slot whose index lies outside [0, n_c) or whose code is negative counts in the
calibration and for no label; a slot that is not finite does not count at all; a row whose slot 0 is not finite gets NaN, beta 1.

``paged_ref``: what spv_knn_paged must return, ``np.lexsort`` on (d, j) over ``_knn_reference.exact_d2`` -- ``knn_ref`` asked for k columns
(the reference has no pages)."""
import math

import numpy as np

from tests._knn_reference import exact_d2, knn_ref

STEPS, TOL = 50, 1e-5


def paged_ref(Q, C, k, exclude=None, d2=None):
    return knn_ref(Q, C, k, exclude, d2=exact_d2(Q, C) if d2 is None else d2)


def make_lists(rng, n, k, n_c, n_sets):
    """Neighbour lists as spv_knn_paged writes them (idx int32 [n, k], squared fp32 dist [n, k] ascending, codes int32 [n_sets, n_c]).
    From 4 rows on, rows 1 .. 3 are not ordinary: row 1 is short (its second half empty), row 2 empty, row 3 holds indices outside
    [0, n_c).  One of the four code values is negative."""
    r = np.sort(rng.gamma(4.0, 0.5, (n, k)), axis=1)
    dist = (r * r).astype(np.float32)
    idx = (np.stack([rng.permutation(max(n_c, k))[:k] for _ in range(n)]) % max(n_c, 1)).astype(np.int32)
    if n >= 4:
        short = max(1, k // 2)
        dist[1, short:], idx[1, short:] = np.inf, -1
        dist[2, :], idx[2, :] = np.inf, -1
        idx[3, ::3] = n_c + 5
    codes = rng.integers(0, 4, (n_sets, n_c)).astype(np.int32) * 7 - 3   # the codes -3, 4, 11, 18
    return idx, dist, codes


# (n, k, n_c, n_sets) of tests/test_zz_gpu_lisi.py: every n of {1, 65, 130}, k of {1, 2, 63, 64, 65, 89, 256} and n_sets of 1 .. 8 at least once
GPU_CASES = [(1, 1, 5, 1), (65, 2, 40, 2), (130, 63, 200, 3), (65, 64, 64, 4), (130, 65, 300, 5), (130, 89, 130, 2), (65, 256, 300, 6), (1, 89, 100, 7),
             (130, 256, 256, 8), (65, 1, 9, 3)]


def perplexity_of(k):
    """the target of the GPU cases, one the full rows can meet: a third of the neighbours, as the API picks k = 3 perplexity - 1"""
    return max(1.0, k / 3.0 + 0.5)


def ordinary_rows(n):
    """the rows of ``make_lists`` that are full lists with valid indices"""
    keep = np.ones(n, dtype=bool)
    if n >= 4:
        keep[1:4] = False
    return keep


def lisi_bound(k: int) -> float:
    """The relative bound on |lisi - lisi_ref at the same beta|, u = 2^-53: e_j differs by at most 4 u (two exponentials of the SAME
    argument, each within 1 ulp = 2 u); S, a sum of k positive terms in any order, by 4 u + 2 (k - 1) u; p_j = e_j / S by (2 k + 4) u;
    a label's sum s_j of at most k of them by (4 k + 2) u; p_j s_j by (6 k + 8) u; their sum by (8 k + 6) u; the inverse by (8 k + 8) u."""
    return (8 * k + 8) * 2.0 ** -53


def row_distances(dist_row):
    """(d float64 [k] = r - r_0, valid bool [k]) of one row of squared fp32 distances; nothing is valid when slot 0 is not finite"""
    d2 = np.asarray(dist_row, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        valid = d2 < np.inf
    if not valid[0]:
        return np.zeros(len(d2)), np.zeros(len(d2), dtype=bool)
    r = np.sqrt(np.where(valid, d2, np.float32(0))).astype(np.float32).astype(np.float64)
    return np.maximum(r - r[0], 0.0), valid


def entropy(d, valid, beta):
    """(H, p float64 [k]) at ``beta``: p is 0 on the slots that do not count"""
    e = np.where(valid, np.exp(-beta * d), 0.0)
    S = e.sum()
    return float(np.log(S) + beta * (d * e).sum() / S), e / S


def calibrate(d, valid, perplexity):
    """(beta, converged) of LISI's search"""
    beta, lo, hi, target = 1.0, -np.inf, np.inf, np.log(perplexity)
    tries = 0
    while True:
        diff = entropy(d, valid, beta)[0] - target
        if abs(diff) < TOL or tries == STEPS:
            return beta, abs(diff) < TOL
        if diff > 0:
            lo = beta
            beta = beta * 2 if hi == np.inf else (beta + hi) / 2
        else:
            hi = beta
            beta = beta / 2 if lo == -np.inf else (beta + lo) / 2
        tries += 1


def simpson(p, codes_row):
    """sum over the labels (codes >= 0) of (sum of the label's p)^2; the squares are added by math.fsum, whose correctly rounded sum does
    not depend on the order the labels' names sort in"""
    codes_row = np.asarray(codes_row)
    return math.fsum(float(p[codes_row == c].sum()) ** 2 for c in np.unique(codes_row[codes_row >= 0]))


def lisi_ref(idx, dist, codes, perplexity, beta=None):
    """-> (lisi float64 [n_sets, n], beta [n], n_valid int [n], converged bool [n], H [n]: the entropy at beta, NaN for an empty row).
    ``codes`` [n_sets, n_c].  ``beta`` [n]: evaluate at these instead of searching (``converged`` then says whether H meets the target)."""
    idx, dist, codes = np.asarray(idx), np.asarray(dist, dtype=np.float32), np.atleast_2d(np.asarray(codes))
    n, n_c = idx.shape[0], codes.shape[1]
    out = np.full((codes.shape[0], n), np.nan)
    betas, n_valid, conv, H = np.ones(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.full(n, np.nan)
    for i in range(n):
        d, valid = row_distances(dist[i])
        n_valid[i] = valid.sum()
        if not valid.any():
            continue
        if beta is None:
            betas[i], conv[i] = calibrate(d, valid, perplexity)
        else:
            betas[i] = beta[i]
        H[i], p = entropy(d, valid, betas[i])
        if beta is not None:
            conv[i] = abs(H[i] - np.log(perplexity)) < TOL
        inside = valid & (idx[i] >= 0) & (idx[i] < n_c)
        for t in range(codes.shape[0]):
            row = np.where(inside, codes[t][np.clip(idx[i], 0, max(n_c - 1, 0))] if n_c else -1, -1)
            with np.errstate(divide="ignore"):
                out[t, i] = np.float64(1.0) / np.float64(simpson(p, row))
    return out, betas, n_valid, conv, H
