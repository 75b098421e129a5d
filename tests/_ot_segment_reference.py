"""The yardstick of the segmented log-sum-exp and cluster-matching tests, independent of the code under test (numpy only).  Test
infrastructure.

``segment_lse_ref(t, seg_ptr)``: ``tests/_ot_reference.lse_ref`` per segment of the columns of ``t`` (itself ``t_ref``): float64
[n_q, n_seg], -inf for a segment without a finite t.  ``lloyd_ref``: a plain Lloyd loop on ``tests/_knn_reference.exact_d2`` with the
product's stated rules, written on its own.  ``cluster_entropies_ref`` / ``entropy_score_ref`` / ``pair_scores_ref``: the clusters'
entropies, the criterion and the block scores from a dense float64 plan."""
import numpy as np

from tests._knn_reference import exact_d2
from tests._ot_reference import lse_ref


def segment_lse_ref(t, seg_ptr):
    t, seg_ptr = np.asarray(t), np.asarray(seg_ptr)
    out = np.full((t.shape[0], len(seg_ptr) - 1), -np.inf)
    for s in range(len(seg_ptr) - 1):
        out[:, s] = lse_ref(t[:, seg_ptr[s]:seg_ptr[s + 1]])
    return out


def lloyd_ref(X, init, max_iter=50):
    """(labels, fp32 centroids, assignment steps, inertia).  Assignment: the nearest centroid by ``exact_d2``, the smaller index on
    equal distances.  Stop when an assignment repeats the one before, or after ``max_iter`` assignments; otherwise new centroids: per
    cluster the float64 sum of its rows, cell by cell in ascending order, over the count, rounded to float32; every cluster without
    a cell, in ascending order, takes the row of the not yet taken cell with the largest squared distance (the smaller index first)."""
    X = np.asarray(X, dtype=np.float32)
    cent = np.asarray(init, dtype=np.float32).copy()
    K, prev = cent.shape[0], None
    for it in range(1, max_iter + 1):
        d = exact_d2(X, cent)
        labels = np.array([min(range(K), key=lambda c: (d[i, c], c)) for i in range(X.shape[0])])
        mine = d[np.arange(X.shape[0]), labels].astype(np.float64)
        if (prev is not None and (labels == prev).all()) or it == max_iter:
            break
        prev = labels
        new = np.zeros_like(cent)
        taken = set()
        for c in range(K):
            members = [i for i in range(X.shape[0]) if labels[i] == c]
            if members:
                acc = np.zeros(X.shape[1], dtype=np.float64)
                for i in members:
                    acc = acc + X[i].astype(np.float64)
                new[c] = (acc / len(members)).astype(np.float32)
            else:
                cell = max((i for i in range(X.shape[0]) if i not in taken), key=lambda i: (mine[i], -i))
                taken.add(cell)
                new[c] = X[cell]
        cent = new
    return labels, cent, it, float(mine.sum())


def cluster_entropies_ref(P, labels, K, axis):
    """per cluster of the cells along ``axis`` (0: the rows of the dense float64 plan ``P``, 1: its columns) the natural-log entropy
    of its summed rows, normalised (0 log 0 = 0); a cluster without mass counts ln(n)"""
    P = np.asarray(P, dtype=np.float64)
    P = P if axis == 0 else P.T
    H = []
    for c in range(K):
        row = P[np.asarray(labels) == c].sum(0)
        if row.sum() > 0:
            p = row / row.sum()
            H.append(-sum(v * np.log(v) for v in p if v > 0))
        else:
            H.append(np.log(P.shape[1]))
    return np.array(H)


def entropy_score_ref(P, labels, K, axis):
    """the reference's criterion for a clustering: minus the mean of ``cluster_entropies_ref``"""
    return -float(np.mean(cluster_entropies_ref(P, labels, K, axis)))


def pair_scores_ref(P, labels0, K0, labels1, K1):
    """(mass, mean entry) of every block of the dense float64 plan; 0 for a block with an empty side"""
    P = np.asarray(P, dtype=np.float64)
    M, S = np.zeros((K0, K1)), np.zeros((K0, K1))
    for a in range(K0):
        for b in range(K1):
            block = P[np.asarray(labels0) == a][:, np.asarray(labels1) == b]
            M[a, b] = block.sum()
            S[a, b] = block.mean() if block.size else 0.0
    return M, S
