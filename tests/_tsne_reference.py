"""The yardstick of the t-SNE tests, independent of the code under test: float64 numpy, O(n^2).  Test infrastructure.

``repulsion_ref``: Zrow[i] = sum_j w_ij, F[t][i] = sum_j w_ij^2 (q_it - c_jt), w = 1 / (1 + |q_i - c_j|^2), all in float64 from the float32
inputs, and next to each sum the sum of its terms' magnitudes, which the bounds scale with.

The bounds (``repulsion_bound``), u = 2^-24 the unit roundoff of fp32, first order in u with a factor (1 + 2^-10) for the higher orders.
The roundings spv_tsne_repulsion's contract lists, per pair:
    each of the D differences q_t - c_t        1 u    so each square carries 2 u
    each of the D fmas of the chain            1 u    the chain's sum of non-negative terms carries at most D u more     d2: (D + 2) u
    s = fl32(1 + d2)                           1 u    the error of d2 is at most (D + 2) u d2 <= (D + 2) u s             s:  (D + 3) u
    w = fl32(1 / s)                            1 u                                                                     w:  (D + 4) u
    w2 = fl32(w * w)                           1 u                                                                     w2: (2 D + 9) u
    fl32(q_t - c_t) for the force              1 u
    fl32(w2 * difference)                      1 u                                                            the term: (2 D + 11) u
so c_Z(D) = D + 4 and c_F(D) = 2 D + 11, times 2^-24 times the sum of the terms' magnitudes.  An fp32 product below the normal range
loses absolute, not relative, accuracy: 2^-149 (1 + |difference|) per term covers w2 and the product.  The fp64 summation term: n_c
sequential additions, each with relative error 2^-53 of a partial sum that is at most the sum of magnitudes, plus the float64
reference's own few roundings per term: (n_c + 8) 2^-53 sum |term|.

``mutant``: a reference that is WRONG in one way a kernel could be -- "drop_last" leaves out the last candidate of the first chunk (of
``n_split`` chunks), "w_for_w2" weighs the force with w, "self" counts the excluded pair.

``affinities_ref``: the calibration of spv_tsne_affinities' contract, float64.  ``update_ref``: the sparse half and the step with their
bounds.  ``kl_ref`` / ``grad_ref``: the KL divergence of a layout and its analytic gradient, dense float64.  ``layout_ref``: the whole
schedule, dense float64 (small n)."""
import numpy as np

U = 2.0 ** -24
HIGHER = 1.0 + 2.0 ** -10


def c_z(D: int) -> int:
    return D + 4


def c_f(D: int) -> int:
    return 2 * D + 11


def _pairs(Q, C):
    Q64, C64 = np.asarray(Q, dtype=np.float32).astype(np.float64), np.asarray(C, dtype=np.float32).astype(np.float64)
    diff = Q64[:, None, :] - C64[None, :, :]                 # [n_q, n_c, D], exact in float64 up to one rounding
    return diff, 1.0 / (1.0 + (diff * diff).sum(axis=2))


def repulsion_ref(Q, C, exclude=None, mutant=None, n_split=1):
    """-> dict(Z [n_q], F [D, n_q], absZ, absF, absD [D, n_q]: sum_j (1 + |difference|), n_c)"""
    diff, w = _pairs(Q, C)
    n_q, n_c = w.shape
    keep = np.ones((n_q, n_c), dtype=bool)
    if exclude is not None and mutant != "self":
        ex = np.asarray(exclude)
        ok = (ex >= 0) & (ex < n_c)
        keep[np.arange(n_q)[ok], ex[ok]] = False
    if mutant == "drop_last" and n_c:
        keep[:, min(-(-n_c // n_split), n_c) - 1] = False
    wk = np.where(keep, w, 0.0)
    terms = (wk if mutant == "w_for_w2" else wk * wk)[:, :, None] * diff
    return {"Z": wk.sum(axis=1), "F": terms.sum(axis=1).T, "absZ": wk.sum(axis=1), "absF": np.abs(terms).sum(axis=1).T,
            "absD": (keep[:, :, None] * (1.0 + np.abs(diff))).sum(axis=1).T, "n_c": n_c}


def repulsion_bound(ref, D: int):
    """-> (bound of Zrow [n_q], bound of F [D, n_q]) for a reference of ``repulsion_ref``"""
    s64 = (ref["n_c"] + 8) * 2.0 ** -53
    return (c_z(D) * U * HIGHER + s64) * ref["absZ"], (c_f(D) * U * HIGHER + s64) * ref["absF"] + 2.0 ** -149 * ref["absD"]


def summation_bound(ref):
    """what two different n_split may differ by: both sums of the SAME fp32-formed terms, each within n_c 2^-53 sum |term| of the exact
    sum (the terms' magnitudes taken from the reference, a factor 1 + 2^-20 above any rounding of theirs)"""
    s = 2.0 * ref["n_c"] * 2.0 ** -53 * (1.0 + 2.0 ** -20)
    return s * ref["absZ"], s * ref["absF"]


def repulsion_case(kind: str, n_q: int, n_c: int, D: int, seed: int = 0):
    """The inputs of the repulsion tests, GPU and CPU alike -> (Q [n_q, D], C [n_c, D]) float32.  "spread": normal draws at the scale of a
    layout in progress; "same": Q's rows are C's first rows (n_q <= n_c), for exclude; "dups": few distinct points, many pairs at
    distance 0; "far": two clusters 1e8 apart."""
    rng = np.random.default_rng([seed, n_q, n_c, D, sum(map(ord, kind))])
    if kind == "dups":
        pts = rng.standard_normal((5, D)).astype(np.float32) * 3
        return pts[rng.integers(0, 5, n_q)], pts[rng.integers(0, 5, n_c)]
    C = (rng.standard_normal((n_c, D)) * 3).astype(np.float32)
    Q = (rng.standard_normal((n_q, D)) * 3).astype(np.float32)
    if kind == "same":
        Q = C[:n_q].copy()
    if kind == "far":
        C[n_c // 2:] += np.float32(1e8)
        Q[n_q // 2:] += np.float32(1e8)
    return np.ascontiguousarray(Q), np.ascontiguousarray(C)


def exact_case(n_q: int, n_c: int):
    """D = 1 inputs where every partial sum of Zrow and F is exact in float64 whatever the order: every coordinate is 0 or 1, so d2 is 0
    or 1, w is 1 or 1/2, w2 is 1 or 1/4 and a force term 0 or +-1/4.  Every term is a multiple of 1/4 of at most 1; sums of a thousand
    stay far below 2^53 quarters."""
    rng = np.random.default_rng([7, n_q, n_c])
    return rng.integers(0, 2, (n_q, 1)).astype(np.float32), rng.integers(0, 2, (n_c, 1)).astype(np.float32)


# ---- affinities
def entropy_of(P_row):
    """float64 entropy of one row of conditional affinities (zeros do not count)"""
    p = np.asarray(P_row, dtype=np.float64)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def affinities_ref(d2, perplexity: float, steps: int = 100, tol: float = 1e-5):
    """-> (P float64 [n, k], beta [n], converged bool [n]) by the contract's search: d = d2 - d2[:, 0], beta from 1, doubling / halving
    while a bound is infinite, else the midpoint; +inf slots get 0 and do not count"""
    d2 = np.asarray(d2, dtype=np.float32).astype(np.float64)
    n, k = d2.shape
    P, betas, conv = np.zeros((n, k)), np.ones(n), np.zeros(n, dtype=bool)
    target = np.log(perplexity)
    for i in range(n):
        ok = np.isfinite(d2[i])
        if not ok[0]:
            continue
        d = d2[i, ok] - d2[i, 0]
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(steps):
            e = np.exp(-beta * d)
            S = e.sum()
            H = np.log(S) + beta * (d * e).sum() / S
            if abs(H - target) <= tol:
                conv[i] = True
                break
            if H - target > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        e = np.exp(-beta * d)
        P[i, ok] = e / e.sum()
        betas[i] = beta
    return P, betas, conv


# ---- the sparse half and the step
def update_case(n: int = 300, D: int = 2, seed: int = 3, density: float = 0.05):
    """The inputs of the update tests, GPU and CPU alike: a random symmetric CSR P (fp32 values summing to 1; row 5 empty, row 9 full), a
    layout, a previous step and gains, and the float64 Zrow / F of that layout."""
    rng = np.random.default_rng([seed, n, D])
    M = np.triu(rng.random((n, n)) < density, 1)
    M[9, 10:] = True
    M[:9, 9] = True
    M = M | M.T
    M[5, :] = False
    M[:, 5] = False
    V = np.triu(rng.random((n, n)), 1)
    V = np.where(M, V + V.T, 0.0)
    V = (V / V.sum()).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum((V > 0).sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(V > 0)
    y = (rng.standard_normal((n, D)) * 2).astype(np.float32)
    u = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    gain = rng.uniform(0.01, 2.0, (n, D)).astype(np.float32)
    rep = repulsion_ref(y, y, exclude=np.arange(n))
    return {"n": n, "D": D, "indptr": indptr, "cols": cols.astype(np.int32), "vals": V[rows, cols], "y": y, "u": u, "gain": gain,
            "Zrow": rep["Z"], "F": np.ascontiguousarray(rep["F"]), "alpha": 12.0, "momentum": 0.8, "lr": 200.0, "min_gain": 0.01}


def update_ref(c):
    """The contract of spv_tsne_update in float64 on the inputs of ``update_case`` -> dict with grad [D, n], kl_row, gain, u, y_out and
    the bounds e_grad, e_kl, e_u, e_y (u = 2^-24, first order, x (1 + 2^-10)):
        the attractive term: w carries (D + 4) u (above), p w one more, the difference one, the product one: (D + 7) u sum |p w diff|,
            and its fp64 sum (row length + 8) 2^-53 of the same magnitude;  F / Z: both are inputs, fp64 roundings only (Z: n additions)
        kl_row: log w carries w's relative error as an absolute one: (D + 4) u sum p, and fp64 terms
        gain: the SAME fp64 operations and one rounding to fp32 as the reference wherever the sign test agrees: bit for bit there
        u = fl32(momentum u - lr gain g): lr gain e_grad, one fp32 rounding u |u_new|
        y_out = fl32(y + u): e_u and one fp32 rounding."""
    n, D = c["n"], c["D"]
    y64 = c["y"].astype(np.float64)
    indptr, cols, vals = c["indptr"], c["cols"], c["vals"].astype(np.float64)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    diff = y64[rows] - y64[cols]
    w = 1.0 / (1.0 + (diff * diff).sum(axis=1))
    terms = (vals * w)[:, None] * diff
    A, absA = np.zeros((n, D)), np.zeros((n, D))
    np.add.at(A, rows, terms)
    np.add.at(absA, rows, np.abs(terms))
    kl, psum = np.zeros(n), np.zeros(n)
    np.add.at(kl, rows, vals * (np.log(vals) - np.log(w)))
    np.add.at(psum, rows, vals * (1.0 + np.abs(np.log(vals)) + np.abs(np.log(w))))
    Z = c["Zrow"].sum()
    g = 4.0 * (c["alpha"] * A - c["F"].T / Z)
    nnz = np.diff(indptr)[:, None]
    s64 = 2.0 ** -53
    e_grad = 4.0 * (c["alpha"] * ((D + 7) * U * HIGHER + (nnz + 8) * s64) * absA + (n + 8) * s64 * np.abs(c["F"].T) / Z) + 8 * s64 * np.abs(g)
    e_kl = (D + 4) * U * HIGHER * np.bincount(rows, weights=vals, minlength=n) + (nnz[:, 0] + 8) * 4 * s64 * psum
    u64, gain64 = c["u"].astype(np.float64), c["gain"].astype(np.float64)
    gain_new = np.maximum(np.where(u64 * g < 0.0, gain64 + 0.2, gain64 * 0.8), c["min_gain"]).astype(np.float32)
    u_new = c["momentum"] * u64 - c["lr"] * gain_new.astype(np.float64) * g
    e_u = c["lr"] * gain_new.astype(np.float64) * e_grad + U * HIGHER * np.abs(u_new)
    y_new = y64 + u_new
    e_y = e_u + U * HIGHER * np.abs(y_new) + U * np.abs(u_new)
    return {"grad": g.T, "kl_row": kl, "gain": gain_new, "u": u_new, "y_out": y_new, "Z": Z, "e_grad": e_grad.T, "e_kl": e_kl, "e_u": e_u, "e_y": e_y,
            "unsure": np.abs(g) <= e_grad}


# ---- the divergence and its gradient, dense
def dense_p(indptr, cols, vals, n: int):
    P = np.zeros((n, n))
    P[np.repeat(np.arange(n), np.diff(indptr)), cols] = np.asarray(vals, dtype=np.float64)
    return P


def kl_ref(Y, P):
    """KL(P || Q) of the layout Y, float64: Q_ij = w_ij / Z over i != j"""
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(axis=2))
    np.fill_diagonal(w, 0.0)
    m = P > 0
    return float((P[m] * (np.log(P[m]) - np.log(w[m]))).sum() + P.sum() * np.log(w.sum()))


def grad_ref(Y, P, alpha: float = 1.0):
    """the analytic gradient in the kernels' form, g = 4 (alpha A - F / Z) [n, D], float64: A from the entries of P, F and Z from all pairs"""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(axis=2))
    np.fill_diagonal(w, 0.0)
    A = ((P * w)[:, :, None] * diff).sum(axis=1)
    F = ((w * w)[:, :, None] * diff).sum(axis=1)
    return 4.0 * (alpha * A - F / w.sum())


# ---- the whole schedule
def knn_p(X, perplexity: float, k: int):
    """the symmetric joint affinities [n, n] float64 from each row's k exact nearest neighbours (ties to the smaller index)"""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    from tests._knn_reference import exact_d2
    d2 = exact_d2(X, X)
    d2[np.arange(n), np.arange(n)] = np.inf
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :k]
    Pc, _beta, _conv = affinities_ref(np.take_along_axis(d2, order, axis=1), perplexity)
    P = np.zeros((n, n))
    np.put_along_axis(P, order, Pc, axis=1)
    return (P + P.T) / (2.0 * n)


def pca_ref(X, d: int):
    """the "pca" initial layout from the SVD of the centred rows (another route than the covariance's eigenvectors), float64"""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    _u, _s, Vt = np.linalg.svd(Xc, full_matrices=False)
    V = Vt[:d].T
    lead = np.abs(V).argmax(axis=0)
    V = V * np.sign(V[lead, np.arange(V.shape[1])])[None, :]
    Y = Xc @ V
    return Y / Y[:, 0].std() * 1e-4


def layout_ref(P, Y0, n_iter: int, early_exaggeration: float = 12.0, exaggeration_iter: int = 250, momentum=(0.5, 0.8), min_gain: float = 0.01,
               state=np.float64, marks=()):
    """the schedule on dense P from Y0 -> (Y, {step: KL before that step}); ``state``: the dtype Y, the step and the gains are kept in"""
    n = P.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0)
    Y, u, gain = np.asarray(Y0).astype(state), np.zeros_like(Y0, dtype=state), np.ones_like(Y0, dtype=state)
    kls = {}
    for it in range(n_iter):
        if it in marks:
            kls[it] = kl_ref(Y, P)
        early = it < exaggeration_iter
        g = grad_ref(Y, P, early_exaggeration if early else 1.0)
        gain = np.maximum(np.where(u.astype(np.float64) * g < 0.0, gain.astype(np.float64) + 0.2, gain.astype(np.float64) * 0.8), min_gain).astype(state)
        u = (momentum[0 if early else 1] * u.astype(np.float64) - lr * gain.astype(np.float64) * g).astype(state)
        Y = (Y.astype(np.float64) + u.astype(np.float64)).astype(state)
    return Y, kls


def blobs(seed: int, n_per: int = 80, D: int = 10):
    """three Gaussian blobs of n_per cells at unit variance, centres default_rng(seed).standard_normal((3, D)) * 4 / sqrt(2)
    -> (X float32 [3 n_per, D], blob of each cell)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((3, D)) * 4 / np.sqrt(2)
    lab = np.repeat(np.arange(3), n_per)
    return (centres[lab] + rng.standard_normal((3 * n_per, D))).astype(np.float32), lab


def neighbour_share(Y, lab) -> float:
    """the share of cells whose nearest neighbour in the layout has their own blob"""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((lab[d.argmin(axis=1)] == lab).mean())
