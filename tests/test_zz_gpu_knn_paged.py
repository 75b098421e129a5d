"""GPU: spv_knn_paged (spvipes_amd.knn_ops.knn_paged) against ``paged_ref`` of tests/_lisi_reference.py: np.lexsort on (d, j) over the exact
float32 distance chain of tests/_knn_reference.py, asked for all k columns at once (the reference knows no pages).

The contract (include/spvipes_hip.h) makes the result exact, so ``idx`` and ``dist`` must EQUAL the reference bit for bit: for
n_q in {1, 129}, n_c in {0, 1, 63, 64, 65, 130, 300}, k in {1, 64, 65, 89, 128, 129, 256} and D in {3, 25, 35}; on lattice data whose ties
straddle the places 64 / 65 and 128 / 129 (asserted on the reference: a predicate that compared d alone would drop or repeat the tied
candidates there); on real-valued data; with fewer than k finite candidates, ``exclude`` and non-finite rows; through odd pitches with NaN
padding and sentinels around the outputs (the helpers of tests/test_gpu_knn.py); for every n_split; against spv_knn's own first 64
columns; for subsets of the queries and repeated calls.  Every test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests._knn_reference import exact_d2
from tests._lisi_reference import paged_ref
from tests.test_gpu_knn import DIST_SENTINEL, IDX_SENTINEL, SPLIT_MAX, _lattice, _padded, _pitch, _real, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _run(dev, Q, C, k, exclude=None, n_split=0, pitch="odd", fn=None):
    """knn_paged (or ``fn``) on padded operands into padded outputs; checks the sentinels; -> (idx, dist) numpy"""
    from spvipes_amd.knn_ops import knn_paged
    n_q, D = Q.shape
    ld_out = k + 3
    idx = torch.full((n_q + 2, ld_out), IDX_SENTINEL, dtype=torch.int32, device=dev)
    dist = torch.full((n_q + 2, ld_out), DIST_SENTINEL, dtype=torch.float32, device=dev)
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).to(dev)
    i, d = (fn or knn_paged)(_padded(Q, _pitch(D, pitch), dev), _padded(C, _pitch(D, "x4" if pitch == "odd" else "odd"), dev), k, exclude=ex,
                             n_split=n_split, out=(idx[:n_q], dist[:n_q]))
    assert i.shape == d.shape == (n_q, k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert (idx[:n_q, k:] == IDX_SENTINEL).all() and (idx[n_q:] == IDX_SENTINEL).all(), "idx written outside [n_q, k]"
    assert (dist[:n_q, k:] == DIST_SENTINEL).all() and (dist[n_q:] == DIST_SENTINEL).all(), "dist written outside [n_q, k]"
    return idx[:n_q, :k], dist[:n_q, :k]


def test_limits_and_workspace(dev):
    from spvipes_amd import _abi
    from spvipes_amd.knn_ops import KNN_KMAX, KNN_PAGED_KMAX, knn_paged_ws_bytes, knn_ws_bytes
    assert (KNN_KMAX, KNN_PAGED_KMAX) == (64, 256) and _abi.KNN_PAGED_KMAX == 256
    assert knn_paged_ws_bytes(129, 256, 1) == 0 and knn_paged_ws_bytes(129, 256, 3) == 3 * 129 * 64 * 8 == knn_ws_bytes(129, 64, 3)
    assert knn_paged_ws_bytes(129, 17, 3) == knn_ws_bytes(129, 17, 3)


# (n_q, n_c, D, k, n_split, pitch): every n_q of {1, 129}, n_c of {0, 1, 63, 64, 65, 130, 300}, k of {1, 64, 65, 89, 128, 129, 256} and
# D of {3, 25, 35} at least once
LATTICE = [(1, 0, 3, 65, 0, "odd"), (129, 1, 25, 89, 0, "x4"), (1, 63, 35, 64, 0, "odd"), (129, 64, 3, 65, 2, "x4"), (129, 65, 25, 128, 0, "odd"),
           (1, 130, 35, 129, 3, "x4"), (129, 300, 3, 256, 0, "odd"), (129, 300, 25, 89, 2, "x4"), (1, 300, 3, 1, 0, "odd"), (129, 130, 35, 256, 7, "odd"),
           (129, 65, 3, 64, 0, "x4"), (129, 300, 35, 128, 3, "odd"), (129, 130, 3, 129, 0, "x4")]


@pytest.mark.parametrize("n_q,n_c,D,k,n_split,pitch", LATTICE, ids=["-".join(map(str, c)) for c in LATTICE])
def test_lattice_data_equals_the_reference(dev, n_q, n_c, D, k, n_split, pitch):
    """every distance is exact and ties are plentiful; rows with fewer than k candidates end in -1 / +inf"""
    rng = np.random.default_rng(n_q * 1000 + n_c * 10 + D + k)
    Q, C = _lattice(rng, n_q, D), _lattice(rng, n_c, D)
    _same(_run(dev, Q, C, k, n_split=n_split, pitch=pitch), paged_ref(Q, C, k))


@pytest.mark.parametrize("n_split", [1, 3])
def test_ties_that_straddle_the_page_boundaries(dev, n_split):
    """One lattice dimension: 65 distinct coordinates for 300 candidates, so every distance is shared by several of them, and the
    reference shows equal distances at the places 64 / 65, 128 / 129 and 192 / 193 (columns 63 | 64, 127 | 128, 191 | 192).  Such a
    group must split by INDEX: a page that compared d alone would either skip the rest of the group or return its head again."""
    rng = np.random.default_rng(41)
    Q, C = _lattice(rng, 129, 1), _lattice(rng, 300, 1)
    want = paged_ref(Q, C, 256)
    for c in (64, 128, 192):
        assert (want[1][:, c - 1] == want[1][:, c]).sum() > 30, "the data must put ties across the page boundary"
    got = _run(dev, Q, C, 256, n_split=n_split)
    _same(got, want)
    assert all(len(set(r.tolist())) == 256 for r in got[0])   # no candidate twice


REAL = [(129, 300, 35, 89, 0, "odd"), (129, 300, 25, 256, 3, "x4"), (1, 130, 3, 129, 0, "odd"), (129, 130, 25, 65, 2, "x4"), (129, 65, 35, 128, 0, "odd")]


@pytest.mark.parametrize("n_q,n_c,D,k,n_split,pitch", REAL, ids=["-".join(map(str, c)) for c in REAL])
def test_real_valued_data_equals_the_reference(dev, n_q, n_c, D, k, n_split, pitch):
    rng = np.random.default_rng(D * 100 + k)
    Q, C = _real(rng, n_q, D), _real(rng, n_c, D)
    d2 = exact_d2(Q, C)
    idx, dist = _run(dev, Q, C, k, n_split=n_split, pitch=pitch)
    _same((idx, dist), paged_ref(Q, C, k, d2=d2))


@pytest.mark.parametrize("data", ["real", "lattice", "few-candidates"])
def test_every_n_split_gives_the_same_bits(dev, data):
    rng = np.random.default_rng(5)
    n_q, n_c, D, k = (129, 70, 25, 129) if data == "few-candidates" else (129, 300, 3 if data == "lattice" else 25, 129)
    make = _lattice if data == "lattice" else _real
    Q, C = make(rng, n_q, D), make(rng, n_c, D)
    want = paged_ref(Q, C, k)
    for n_split in (1, 2, 3, 7, SPLIT_MAX, 0):
        _same(_run(dev, Q, C, k, n_split=n_split), want)


def test_the_first_64_columns_are_spv_knn_bit_for_bit(dev):
    from spvipes_amd.knn_ops import knn
    rng = np.random.default_rng(6)
    Q, C = _lattice(rng, 129, 3), _lattice(rng, 300, 3)
    me = rng.integers(-3, 303, 129).astype(np.int32)
    for k in (1, 17, 64):   # one page: the same kernels on the same arguments
        _same(_run(dev, Q, C, k, exclude=me, n_split=2), _run(dev, Q, C, k, exclude=me, n_split=2, fn=knn))
    first = _run(dev, Q, C, 64, exclude=me, fn=knn)
    for k in (65, 89, 256):
        got = _run(dev, Q, C, k, exclude=me, n_split=3)
        _same((got[0][:, :64], got[1][:, :64]), first)


def test_subsets_of_the_queries_and_repeated_calls(dev):
    rng = np.random.default_rng(7)
    Q, C = _real(rng, 129, 25), _real(rng, 300, 25)
    a = _run(dev, Q, C, 200)
    _same(a, _run(dev, Q, C, 200))
    sub = np.array([128, 0, 64, 5, 127])
    _same(_run(dev, Q[sub], C, 200, n_split=2), (a[0][sub], a[1][sub]))


def test_exclude(dev):
    rng = np.random.default_rng(8)
    n, D, k = 130, 10, 129
    X = _real(rng, n, D)
    me = np.arange(n, dtype=np.int32)
    own = _run(dev, X, X, k, exclude=me, n_split=2)
    assert (own[0] != me[:, None]).all() and (own[0] >= 0).all()        # exactly the n - 1 others
    _same(own, paged_ref(X, X, k, me))
    full = _run(dev, X, X, k + 1, exclude=me)                           # one more than there are: the last slot stays empty
    assert (full[0][:, -1] == -1).all() and np.isinf(full[1][:, -1]).all()
    _same((full[0][:, :k], full[1][:, :k]), own)
    some = rng.integers(-3, n + 3, n).astype(np.int32)
    _same(_run(dev, X, X, k, exclude=some), paged_ref(X, X, k, some))


def test_non_finite_input_and_rows_that_run_out(dev):
    rng = np.random.default_rng(9)
    n_q, n_c, D, k = 129, 130, 25, 129
    Q, C = _real(rng, n_q, D), _real(rng, n_c, D)
    C[0, 3], C[7, :], C[63, 24], C[64, 0], C[n_c - 1, :] = np.inf, np.nan, -np.inf, np.nan, 3e19   # 3e19: the sum of squares overflows
    Q[5, 2], Q[128, :] = np.nan, np.inf
    idx, dist = _run(dev, Q, C, k, n_split=2)
    _same((idx, dist), paged_ref(Q, C, k))
    for i in (5, 128):   # a non-finite query has no neighbour on any page
        assert (idx[i] == -1).all() and np.isinf(dist[i]).all() and (dist[i] > 0).all()
    rest = np.setdiff1d(np.arange(n_q), (5, 128))
    assert (idx[rest, :125] >= 0).all() and (idx[rest, 125:] == -1).all()   # 125 finite candidates: the second page ends early, the third gets nothing
    wide = _run(dev, Q, C, 256)
    _same((wide[0][:, :k], wide[1][:, :k]), (idx, dist))
    assert (wide[0][:, 125:] == -1).all() and np.isinf(wide[1][:, 125:]).all()


def test_op_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.knn_ops import knn, knn_paged
    Q, C = torch.zeros((4, 5), device=dev), torch.zeros((9, 5), device=dev)
    for bad in (lambda: knn_paged(Q, C, 0), lambda: knn_paged(Q, C, 257), lambda: knn_paged(Q, C, 2, n_split=65), lambda: knn_paged(Q[:0], C, 2),
                lambda: knn(Q, C, 65)):   # the unpaged search keeps its limit
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: knn_paged(Q.double(), C, 2), lambda: knn_paged(Q, C[:, :4], 2), lambda: knn_paged(Q, C, 2, exclude=torch.zeros(4, device=dev)),
                lambda: knn_paged(Q, C, 70, out=(torch.zeros((4, 69), dtype=torch.int32, device=dev), torch.zeros((4, 70), device=dev)))):
        with pytest.raises(_abi.SpvError):
            bad()
