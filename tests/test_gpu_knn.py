"""GPU: spv_knn (spvipes_amd.knn_ops.knn) against the yardstick of tests/_knn_reference.py.

The kernel's contract (include/spvipes_hip.h) makes the result exact: the distance is one fixed float32 chain per pair and the order
(distance, index) is total, so wherever the reference can be afforded ``idx`` and ``dist`` must EQUAL it, bit for bit.  Shapes are sized
by the tiles the library reports (TQ queries per workgroup, TC candidates per LDS tile): one below, at and one above a tile, several
tiles, more than one workgroup.  Every call goes through ``_run``: odd or 16-byte-multiple row pitches with NaN in the pitch padding
(a kernel that read it would lose those candidates: a NaN distance is never returned) and sentinels in the output's columns >= k and
rows >= n_q, which must come back untouched.  Every test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests._knn_reference import exact_d2, knn_ref

pytestmark = pytest.mark.gpu

TQ, TC, SPLIT_MAX = 128, 64, 64   # what the parametrisation assumes; test_tiles pins them
IDX_SENTINEL, DIST_SENTINEL = -77, -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _pitch(D, kind):
    """a row pitch >= D: "odd" (no alignment at all) or "x4" (a multiple of 16 bytes, beyond D)"""
    return (D + 1) | 1 if kind == "odd" else (D + 4) // 4 * 4 + 4


def _padded(A, ld, dev):
    buf = torch.full((max(A.shape[0], 1), ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:A.shape[0], :A.shape[1]] = torch.from_numpy(A).to(dev)
    return buf[:A.shape[0], :A.shape[1]]


def _run(dev, Q, C, k, exclude=None, n_split=0, pitch="odd"):
    """knn on padded operands into padded outputs; checks the sentinels; -> (idx, dist) numpy"""
    from spvipes_amd.knn_ops import knn
    n_q, D = Q.shape
    ld_out = k + 3
    idx = torch.full((n_q + 2, ld_out), IDX_SENTINEL, dtype=torch.int32, device=dev)
    dist = torch.full((n_q + 2, ld_out), DIST_SENTINEL, dtype=torch.float32, device=dev)
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).to(dev)
    i, d = knn(_padded(Q, _pitch(D, pitch), dev), _padded(C, _pitch(D, "x4" if pitch == "odd" else "odd"), dev), k, exclude=ex, n_split=n_split,
               out=(idx[:n_q], dist[:n_q]))
    assert i.shape == d.shape == (n_q, k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert (idx[:n_q, k:] == IDX_SENTINEL).all() and (idx[n_q:] == IDX_SENTINEL).all(), "idx written outside [n_q, k]"
    assert (dist[:n_q, k:] == DIST_SENTINEL).all() and (dist[n_q:] == DIST_SENTINEL).all(), "dist written outside [n_q, k]"
    return idx[:n_q, :k], dist[:n_q, :k]


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def _lattice(rng, n, D):
    return rng.integers(-32, 33, (n, D)).astype(np.float32) / 4   # multiples of 1/4 in [-8, 8]


def _real(rng, n, D):
    return rng.standard_normal((n, D)).astype(np.float32)


def test_tiles(dev):
    from spvipes_amd.knn_ops import KNN_DMAX, KNN_KMAX, KNN_SPLIT_MAX, knn_splits, knn_tiles
    assert knn_tiles() == (TQ, TC) and (KNN_DMAX, KNN_KMAX, KNN_SPLIT_MAX) == (64, 64, SPLIT_MAX)
    assert knn_splits(2 * TQ + 3, 2000) == 7 and knn_splits(2 * TQ + 3, 2 * TC + 5) == 1   # what the cases below rely on


# (n_q, n_c, D, k, n_split, pitch): every n_q of {1, TQ-1, TQ, TQ+1, 2TQ+3}, n_c of {0, 1, k-1, k, TC-1, TC, TC+1, 2TC+5}, D of
# {1, 3, 4, 16, 25, 35, 64} and k of {1, 2, 15, 16, 17, 64} at least once
LATTICE = [(1, 0, 3, 2, 0, "odd"), (1, 1, 1, 1, 0, "odd"), (TQ - 1, 14, 4, 15, 0, "x4"), (TQ, 15, 16, 15, 2, "odd"), (TQ + 1, TC - 1, 25, 16, 0, "x4"),
           (2 * TQ + 3, TC, 35, 17, 3, "odd"), (TQ, TC + 1, 64, 64, 0, "x4"), (2 * TQ + 3, 2 * TC + 5, 25, 64, 2, "odd"), (TQ + 1, 2 * TC + 5, 3, 2, 5, "x4"),
           (TQ - 1, TC - 1, 1, 64, 0, "odd"), (1, 2 * TC + 5, 35, 1, 0, "x4"), (2 * TQ + 3, 16, 16, 16, 0, "x4"), (TQ, 1, 4, 17, 0, "odd"),
           (3, 63, 64, 64, 4, "odd"), (TQ + 1, TC + 1, 16, 1, 0, "odd")]


@pytest.mark.parametrize("n_q,n_c,D,k,n_split,pitch", LATTICE, ids=["-".join(map(str, c)) for c in LATTICE])
def test_lattice_data_equals_the_reference(dev, n_q, n_c, D, k, n_split, pitch):
    """every distance is exact and ties are plentiful: the tie rule (smaller index first) and the fill rule (-1 / +inf) are pinned"""
    rng = np.random.default_rng(n_q * 1000 + n_c * 10 + D)
    Q, C = _lattice(rng, n_q, D), _lattice(rng, n_c, D)
    want = knn_ref(Q, C, k)
    if n_c > k and D <= 4:
        assert (np.diff(want[1], axis=1) == 0).any()   # ties among the returned distances
    _same(_run(dev, Q, C, k, n_split=n_split, pitch=pitch), want)


REAL = [(64, 300, 35, 15, 0, "odd"), (33, 257, 25, 16, 3, "x4"), (64, 130, 64, 64, 0, "odd"), (17, 300, 16, 2, 7, "x4"), (5, 100, 3, 17, 0, "odd"), (64, 300, 25, 15, 1, "x4")]


@pytest.mark.parametrize("n_q,n_c,D,k,n_split,pitch", REAL, ids=["-".join(map(str, c)) for c in REAL])
def test_real_valued_data_equals_the_reference(dev, n_q, n_c, D, k, n_split, pitch):
    """``dist`` bit-equal to the exact float32 chain at the returned indices, ``idx`` equal to the reference's"""
    rng = np.random.default_rng(D * 100 + k)
    Q, C = _real(rng, n_q, D), _real(rng, n_c, D)
    d2 = exact_d2(Q, C)
    idx, dist = _run(dev, Q, C, k, n_split=n_split, pitch=pitch)
    np.testing.assert_array_equal(dist.view(np.uint32), np.take_along_axis(d2, idx.astype(np.int64), 1).view(np.uint32))
    _same((idx, dist), knn_ref(Q, C, k, d2=d2))


LARGER = [(2 * TQ + 3, 2000, 25, 15), (2 * TQ + 3, 2000, 35, 64), (TQ + 2, 2000, 64, 17), (2 * TQ + 3, 1999, 16, 50)]


@pytest.mark.parametrize("n_q,n_c,D,k", LARGER, ids=["-".join(map(str, c)) for c in LARGER])
def test_properties_at_larger_shapes(dev, n_q, n_c, D, k):
    """No float32 emulation, float64 distances only (their own error, about D * 2^-53 relative, disappears in the slack below).
    The bound: the chain computes u_t = (q_t - c_t)(1 + a_t) and acc_t = (acc_{t-1} + u_t^2)(1 + b_t) with |a_t|, |b_t| <= 2^-24, one
    rounding each.  Unrolled, term t of the sum carries (1 + a_t)^2 and the factors (1 + b_s) of the D - t additions from its own on:
    at most D + 2 factors, so it is off by at most (1 + 2^-24)^(D+2) - 1 < (D + 2) * 2^-23 relative.  All terms are non-negative, hence
    the same relative bound holds for the sum: |d - d64| <= (D + 2) * 2^-23 * d64.  (The data keep every u_t^2 far above the
    subnormals.)  The chunked route is taken (7 chunks at these shapes, test_tiles)."""
    rng = np.random.default_rng(n_c + D)
    Q, C = _real(rng, n_q, D), _real(rng, n_c, D)
    idx, dist = _run(dev, Q, C, k)
    assert (idx >= 0).all() and (idx < n_c).all()
    d64 = ((Q.astype(np.float64)[:, None, :] - C.astype(np.float64)[None]) ** 2).sum(-1)
    bound = (D + 2) * 2.0 ** -23 * d64
    # rows ascend in (d, j), no candidate twice
    dd, dj = np.diff(dist.astype(np.float64), axis=1), np.diff(idx.astype(np.int64), axis=1)
    assert ((dd > 0) | ((dd == 0) & (dj > 0))).all()
    # every returned distance is the float64 distance of its index, within the bound
    at = np.take_along_axis(d64, idx.astype(np.int64), 1)
    assert (np.abs(dist.astype(np.float64) - at) <= np.take_along_axis(bound, idx.astype(np.int64), 1)).all()
    # no candidate left out lies below the row's k-th returned distance by more than the bound
    left = np.ones((n_q, n_c), dtype=bool)
    np.put_along_axis(left, idx.astype(np.int64), False, 1)
    assert left.sum(1).tolist() == [n_c - k] * n_q
    assert (d64 + bound >= dist[:, -1:].astype(np.float64))[left].all()


@pytest.mark.parametrize("data", ["real", "lattice", "few-candidates"])
def test_every_n_split_gives_the_same_bits(dev, data):
    """1, 2, 3, 7, SPLIT_MAX chunks and the automatic choice; "few-candidates": 40 candidates, so most of 64 chunks hold none"""
    rng = np.random.default_rng(5)
    n_q, n_c, D, k = (TQ + 1, 40, 25, 15) if data == "few-candidates" else (TQ + 1, 300, 25, 15)
    make = _lattice if data == "lattice" else _real
    Q, C = make(rng, n_q, D), make(rng, n_c, D)
    want = knn_ref(Q, C, k)
    for n_split in (1, 2, 3, 7, SPLIT_MAX, 0):
        _same(_run(dev, Q, C, k, n_split=n_split), want)


def test_subset_of_the_queries_and_permutation_of_the_candidates(dev):
    rng = np.random.default_rng(6)
    n_q, n_c, D, k = 2 * TQ + 3, 2 * TC + 5, 25, 16
    Q, C = _real(rng, n_q, D), _real(rng, n_c, D)
    d2 = exact_d2(Q, C)
    assert all(len(np.unique(r)) == n_c for r in d2)   # distinct distances per query
    idx, dist = _run(dev, Q, C, k)
    sub = np.array([n_q - 1, 0, 130, 5, 129, 128, 127])
    _same(_run(dev, Q[sub], C, k), (idx[sub], dist[sub]))
    perm = rng.permutation(n_c)
    idx_p, dist_p = _run(dev, Q, C[perm], k, n_split=3)
    np.testing.assert_array_equal(dist_p.view(np.uint32), dist.view(np.uint32))
    np.testing.assert_array_equal(perm[idx_p], idx)


def test_exclude(dev):
    rng = np.random.default_rng(7)
    n, D, k = TQ + 9, 10, 5
    X = _real(rng, n, D)
    me = np.arange(n, dtype=np.int32)
    plain = _run(dev, X, X, k)
    assert (plain[0][:, 0] == me).all() and (plain[1][:, 0] == 0).all()   # a cell is its own nearest candidate, at distance +0
    own = _run(dev, X, X, k, exclude=me, n_split=2)
    assert (own[0] != me[:, None]).all()
    _same(own, knn_ref(X, X, k, me))
    _same((own[0][:, :k - 1], own[1][:, :k - 1]), (plain[0][:, 1:], plain[1][:, 1:]))   # the rest moves up by one
    for code in (-1, n, 2 ** 31 - 1, -2 ** 31):   # codes outside [0, n_c) exclude nothing
        _same(_run(dev, X, X, k, exclude=np.full(n, code, dtype=np.int64).astype(np.int32)), plain)
    some = rng.integers(-3, n + 3, n).astype(np.int32)
    _same(_run(dev, X, X, k, exclude=some), knn_ref(X, X, k, some))
    short = _run(dev, X[:3], X[:k], k, exclude=me[:3])   # k candidates, one excluded: the last slot is empty
    assert (short[0][:, -1] == -1).all() and np.isinf(short[1][:, -1]).all() and (short[0][:, :-1] >= 0).all()


def test_non_finite_input(dev):
    rng = np.random.default_rng(8)
    n_q, n_c, D, k = TQ + 1, 2 * TC + 5, 25, 15
    Q, C = _real(rng, n_q, D), _real(rng, n_c, D)
    clean = _run(dev, Q, C, k)
    bad = np.array([0, 7, TC - 1, TC, n_c - 1])
    keep = np.setdiff1d(np.arange(n_c), bad)
    C2 = C.copy()
    C2[0, 3], C2[7, :], C2[TC - 1, 24], C2[TC, 0], C2[n_c - 1, :] = np.inf, np.nan, -np.inf, np.nan, 3e19   # 3e19: the sum of squares overflows
    Q2 = Q.copy()
    Q2[5, 2], Q2[TQ, :] = np.nan, np.inf
    idx, dist = _run(dev, Q2, C2, k, n_split=2)
    assert not np.isin(idx, bad).any() and np.isfinite(dist[idx >= 0]).all()
    for i in (5, TQ):   # a non-finite query has no neighbour at all
        assert (idx[i] == -1).all() and np.isinf(dist[i]).all() and (dist[i] > 0).all()
    rest = np.setdiff1d(np.arange(n_q), (5, TQ))
    want = _run(dev, Q[rest], C[keep], k)   # the same problem without the bad rows
    _same((np.where(idx[rest] >= 0, np.searchsorted(keep, idx[rest]), -1).astype(np.int32), dist[rest]), want)
    _same((idx, dist), knn_ref(Q2, C2, k))
    assert not np.array_equal(clean[0][rest], idx[rest])   # the bad rows had been somebody's neighbours


def test_two_calls_agree_bit_for_bit(dev):
    rng = np.random.default_rng(9)
    Q, C = _real(rng, 2 * TQ + 3, 35), _real(rng, 1500, 35)
    a = _run(dev, Q, C, 50)
    b = _run(dev, Q, C, 50)
    _same(a, b)


def test_op_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.knn_ops import knn
    Q, C = torch.zeros((4, 5), device=dev), torch.zeros((9, 5), device=dev)
    for bad in (lambda: knn(Q.double(), C, 2), lambda: knn(Q.cpu(), C, 2), lambda: knn(Q, C[:, :4], 2), lambda: knn(Q.t().contiguous().t(), C, 2),
                lambda: knn(Q, C, 2, exclude=torch.zeros(4, device=dev)), lambda: knn(Q, C, 2, exclude=torch.zeros(3, dtype=torch.int32, device=dev)),
                lambda: knn(Q, C, 2, out=(torch.zeros((4, 1), dtype=torch.int32, device=dev), torch.zeros((4, 2), device=dev)))):
        with pytest.raises(_abi.SpvError):
            bad()
    for bad in (lambda: knn(Q, C, 0), lambda: knn(Q, C, 65), lambda: knn(Q, C, 2, n_split=65), lambda: knn(Q[:0], C, 2),
                lambda: knn(torch.zeros((4, 65), device=dev), torch.zeros((9, 65), device=dev), 2)):
        with pytest.raises(ValueError):
            bad()
