"""Clusters per group and their log masses under a transport plan, for ``spVIPES.match_transport_clusters``: Lloyd's k-means whose
assignment step is the exact k-NN kernel (``knn_ops.knn`` with k = 1 against the centroids) and whose update runs on the host in fp64,
and ``cluster_transport_log_mass``: one ``ot_ops.ot_segment_lse`` pass over the candidates arranged by cluster.  The numpy pieces
(seeding, update, criterion, scores, matching) are in ``data``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .data import cluster_segments, kmeans_pp_init, kmeans_update
from .knn_ops import knn
from .ot_ops import SinkhornResult, ot_segment_lse


@dataclass
class KMeansResult:
    """``labels`` int64 [n] and ``centroids`` fp32 [K, D] on the host: the last assignment and the centroids it was measured against;
    ``n_iter``: assignment steps run; ``inertia``: the fp64 sum of the squared distances that assignment returned; ``converged``: the
    last assignment repeated the one before it"""
    labels: np.ndarray
    centroids: np.ndarray
    n_iter: int
    inertia: float
    converged: bool


def kmeans(X_dev: torch.Tensor, init, max_iter: int = 50) -> KMeansResult:
    """Lloyd iterations on the rows of ``X_dev`` (fp32 device tensor [n, D], 1 <= D <= 64) from the centroids ``init`` [K, D].
    Assignment: ``knn(X, centroids, k=1)`` -- exact, the fixed fp32 distance chain, ties to the smaller centroid index.  Update
    (``data.kmeans_update``): fp64 sums in ascending cell order, divided, rounded to fp32; an emptied cluster takes the cell with the
    largest current squared distance, the smaller index on ties.  Stops when an assignment repeats the previous one (the centroids
    are then the means of exactly this assignment) or after ``max_iter`` assignments."""
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"kmeans: max_iter must be a positive integer, got {max_iter!r}")
    cent = np.ascontiguousarray(np.asarray(init, dtype=np.float32))
    if cent.ndim != 2 or cent.shape[0] < 1 or X_dev.dim() != 2 or cent.shape[1] != X_dev.shape[1] or not np.isfinite(cent).all():
        raise ValueError("kmeans: init must be a finite array [K >= 1, D] with X's number of columns")
    K = cent.shape[0]
    X64 = X_dev.detach().cpu().numpy().astype(np.float64)
    prev, converged = None, False
    for it in range(1, int(max_iter) + 1):
        idx, dist = knn(X_dev, torch.from_numpy(cent).to(X_dev.device), 1)
        labels, d2 = idx[:, 0].cpu().numpy().astype(np.int64), dist[:, 0].cpu().numpy().astype(np.float64)
        if (labels < 0).any():
            raise ValueError("kmeans: a row of X has no finite distance to any centroid (non-finite input)")
        converged = prev is not None and np.array_equal(labels, prev)
        if converged or it == int(max_iter):
            break
        prev = labels
        cent = kmeans_update(X64, labels, d2, K)
    return KMeansResult(labels, cent, it, float(d2.sum()), converged)


def kmeans_best(X_dev: torch.Tensor, K: int, n_init: int = 4, seed: int = 0, max_iter: int = 50) -> KMeansResult:
    """``kmeans`` from ``n_init`` k-means++ seedings (``data.kmeans_pp_init`` with the seeds ``seed + r``) -> the run with the lowest
    inertia, the first one on ties"""
    X = X_dev.detach().cpu().numpy()
    best = None
    for r in range(int(n_init)):
        run = kmeans(X_dev, kmeans_pp_init(X, K, int(seed) + r), max_iter)
        if best is None or run.inertia < best.inertia:
            best = run
    return best


def cluster_transport_log_mass(res: SinkhornResult, X_q: torch.Tensor, X_c: torch.Tensor, labels_c, side: int,
                               n_clusters: Optional[int] = None) -> np.ndarray:
    """log T[c, i], T[c, i] = the mass the UNTRUNCATED plan P = a b exp(phi + psi - s c) of the Sinkhorn result ``res`` puts between
    cluster c of the candidate cells ``X_c`` (clusters ``labels_c`` in [0, K)) and query cell i of ``X_q`` -> host fp64 [K, n_q]; -inf
    for a cluster without cells or mass.  ``side``: the group of the QUERIES, 0 (``X_q`` is the X0 the potentials were computed on,
    ``X_c`` the X1) or 1 (the other way round).  The candidates are arranged by cluster (a stable sort), then ONE ``ot_segment_lse``
    call: log T = L[c][i] + r_i with r the queries' potential plus log marginal, added in fp64."""
    if side not in (0, 1):
        raise ValueError(f"side must be 0 or 1, got {side!r}")
    pot_q, pot_c = (res.phi + res.log_a, res.psi + res.log_b)[::1 if side == 0 else -1]
    labels_c = np.asarray(labels_c).ravel()
    if labels_c.shape[0] != X_c.shape[0] or pot_c.shape[0] != X_c.shape[0] or pot_q.shape[0] != X_q.shape[0]:
        raise ValueError("cluster_transport_log_mass: one label per candidate, and the potentials' sizes must match the two sides")
    K = int(labels_c.max()) + 1 if n_clusters is None else int(n_clusters)
    perm, seg_ptr, _ = cluster_segments(labels_c, K)
    perm_dev = torch.from_numpy(perm).to(X_c.device)
    L = ot_segment_lse(X_q, X_c[perm_dev].contiguous(), pot_c[perm_dev].contiguous(), torch.from_numpy(seg_ptr).to(X_c.device), res.inv_eps)
    return L.t().cpu().numpy().astype(np.float64) + pot_q.cpu().numpy().astype(np.float64)[None, :]
