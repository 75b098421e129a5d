"""The yardstick of the silhouette tests, independent of the code under test.  Test infrastructure.

``segment_sums_ref(Q, C, seg_ptr)``: the contract of spv_silhouette_sums (include/spvipes_hip.h) -- each pair's distance is numpy's float32
square root (the IEEE operation, correctly rounded) of ``tests/_knn_reference.exact_d2``, widened to float64 and summed per segment of the
candidates.  numpy adds pairwise, the kernel in ascending order: the two agree bit for bit exactly where ``sums_are_exact`` holds.
With ``n_split`` the same terms are added in the ORDER the contract states -- ascending candidate within each of n_split chunks of
ceil(n_c / n_split) candidates from +0, the chunks' values in chunk order from +0 -- which is the kernel's result bit for bit on any data.

``sums_are_exact(d, seg_ptr)``: true when, for every query and segment, the sum of the segment's distances fits in 53 bits at the unit of
the last place of the segment's smallest positive term.  Every float32 term is a multiple of that unit, so every partial sum of every
order of addition is such a multiple below 2^53 units, hence a float64 value: no addition rounds and all orders give the same bits.

``silhouette_ref`` / ``group_silhouette_ref``: the silhouette widths straight from their definitions, float64, O(n^2) numpy."""
import numpy as np

from tests._knn_reference import exact_d2


def distances_ref(Q, C):
    """float32 [n_q, n_c]: the contract's distance of every pair"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(exact_d2(Q, C)).astype(np.float32)


def segment_sums_ref(Q, C, seg_ptr, d=None, n_split=None):
    """float64 [n_q, n_seg]; ``d``: ``distances_ref(Q, C)`` if already at hand; ``n_split``: None = numpy's own (pairwise) order, else the
    contract's order of addition for that many chunks"""
    d = distances_ref(Q, C) if d is None else d
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    d64 = d.astype(np.float64)
    n_q, n_c = d.shape
    out = np.zeros((n_q, len(seg_ptr) - 1), dtype=np.float64)
    chunks = [(0, n_c)] if n_split is None else [(min(c * -(-n_c // n_split), n_c), min((c + 1) * -(-n_c // n_split), n_c)) for c in range(n_split)]
    with np.errstate(invalid="ignore", over="ignore"):
        for c0, c1 in chunks:
            for s in range(len(seg_ptr) - 1):
                lo, hi = max(c0, int(seg_ptr[s])), min(c1, int(seg_ptr[s + 1]))
                if hi <= lo:
                    continue
                part = d64[:, lo:hi].sum(axis=1) if n_split is None else np.cumsum(d64[:, lo:hi], axis=1)[:, -1]   # cumsum adds in sequence
                out[:, s] = out[:, s] + part
    return out


def sums_are_exact(d, seg_ptr) -> bool:
    """``d`` float32 [n_q, n_c] distances (finite, non-negative)"""
    d = np.asarray(d, dtype=np.float32)
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    if not np.isfinite(d).all() or (d < 0).any():
        return False
    for s in range(len(seg_ptr) - 1):
        part = d[:, seg_ptr[s]:seg_ptr[s + 1]].astype(np.float64)
        if part.shape[1] == 0:
            continue
        pos = np.where(part > 0, part, np.inf).min(axis=1)                # the smallest positive term of each query
        some = np.isfinite(pos)
        _m, e = np.frexp(np.where(some, pos, 1.0))                         # pos = m * 2^e, 0.5 <= m < 1
        unit = np.ldexp(1.0, np.maximum(e - 24, -149))                     # the last place of a float32 of that size
        total = part.sum(axis=1) * (1.0 + 2.0 ** -40)                      # an upper bound of the true sum
        if (some & ~(total / unit < 2.0 ** 53)).any():
            return False
    return True


def _pairwise(X64):
    X64 = np.asarray(X64, dtype=np.float64)
    return np.sqrt(((X64[:, None, :] - X64[None, :, :]) ** 2).sum(-1))


def _width(a, b):
    m = max(a, b)
    return 0.0 if m == 0 else (b - a) / m


def silhouette_ref(X64, labels, dist=None):
    """(s, a, b, nearest) per cell: a = mean distance to the OTHER cells of its label (NaN for the only cell of a label, s = 0 there),
    b = the smallest mean distance to the cells of another label (ties: the label that sorts first; NaN / None / s = NaN without
    one), s = (b - a) / max(a, b), 0 where max(a, b) = 0.  ``dist``: an [n, n] distance matrix to use instead of X64's."""
    labels = np.asarray(labels)
    D = _pairwise(X64) if dist is None else np.asarray(dist, dtype=np.float64)
    cats = np.unique(labels)
    n = len(labels)
    s, a, b, near = np.zeros(n), np.full(n, np.nan), np.full(n, np.nan), np.empty(n, dtype=object)
    for i in range(n):
        own = labels == labels[i]
        best = None
        for u in cats:
            if u == labels[i]:
                continue
            m = D[i, labels == u].sum() / (labels == u).sum()
            if best is None or m < b[i]:
                b[i], best = m, u
        near[i] = best
        if best is None:
            s[i] = np.nan
        if own.sum() > 1:
            a[i] = D[i, own].sum() / (own.sum() - 1)
            if best is not None:
                s[i] = _width(a[i], b[i])
    return s, a, b, near


def group_silhouette_ref(X64, labels, groups, dist=None):
    """s_g per cell: inside its label, its own group as the cluster and the other group as the neighbour; 0 for the only cell of its
    (label, group); NaN when its label has no cell in the other group"""
    labels, groups = np.asarray(labels), np.asarray(groups)
    D = _pairwise(X64) if dist is None else np.asarray(dist, dtype=np.float64)
    n = len(labels)
    s = np.full(n, np.nan)
    for i in range(n):
        own = (labels == labels[i]) & (groups == groups[i])
        oth = (labels == labels[i]) & (groups != groups[i])
        if not oth.any():
            continue
        if own.sum() == 1:
            s[i] = 0.0
            continue
        s[i] = _width(D[i, own].sum() / (own.sum() - 1), D[i, oth].sum() / oth.sum())
    return s


def scores_ref(s, s_g, labels):
    """(label_asw, group_asw) in scIB's definitions from the per-cell columns"""
    labels = np.asarray(labels)
    parts = [np.mean(1.0 - np.abs(s_g[labels == u])) for u in np.unique(labels) if not np.isnan(s_g[labels == u]).any()]
    return (np.mean(s) + 1.0) / 2.0, (float(np.mean(parts)) if parts else float("nan"))
