"""CPU: the yardstick of the cluster-matching tests (tests/_ot_segment_reference.py) against brute force on lattice data, where every
operation is exact: the per-segment log-sum-exp, the Lloyd loop with its update and re-seeding rules, the criterion and the block scores
from a dense plan.  No GPU calls, nothing of the product."""
import numpy as np

from tests._ot_reference import t_ref
from tests._ot_segment_reference import entropy_score_ref, lloyd_ref, pair_scores_ref, segment_lse_ref


def test_segment_lse_on_lattice_data_and_edge_values():
    rng = np.random.default_rng(1)
    X, Y = (rng.integers(-8, 9, (n, 5)).astype(np.float32) / 4 for n in (7, 60))
    h = rng.integers(-6, 7, 60).astype(np.float32) / 2
    seg_ptr = np.array([0, 0, 13, 14, 14, 14, 47, 60, 60])   # empty segments first, in a row and last; one of size 1
    t = t_ref(X, Y, h, 0.5)
    plain = (-0.5 * ((X[:, None, :] - Y[None]) ** 2).sum(-1, dtype=np.float32) + h[None]).astype(np.float64)   # every operation exact
    got = segment_lse_ref(t, seg_ptr)
    assert got.shape == (7, 8) and np.isneginf(got[:, [0, 3, 4, 7]]).all()
    for s in (1, 2, 5, 6):
        np.testing.assert_allclose(got[:, s], np.log(np.exp(plain[:, seg_ptr[s]:seg_ptr[s + 1]]).sum(1)), rtol=1e-14)
    np.testing.assert_array_equal(got[:, 2], plain[:, 13])   # a segment of one candidate is its t
    # the segments add up to the whole
    np.testing.assert_allclose(np.log(np.exp(got).sum(1)), np.log(np.exp(plain).sum(1)), rtol=1e-13)
    # a segment whose every t is not finite is -inf, and only that one
    h2, Y2 = h.copy(), Y.copy()
    h2[14:47] = -np.inf
    h2[2], h2[3] = np.nan, np.inf
    Y2[50, :] = 3e19
    got2 = segment_lse_ref(t_ref(X, Y2, h2, 0.5), seg_ptr)
    assert np.isneginf(got2[:, 5]).all() and np.isfinite(got2[:, [1, 2, 6]]).all()
    keep = np.setdiff1d(np.arange(47, 60), [50])
    np.testing.assert_allclose(got2[:, 6], np.log(np.exp(plain[:, keep]).sum(1)), rtol=1e-14)
    assert np.isneginf(segment_lse_ref(t[:, :0], [0, 0, 0])).all()


def test_lloyd_on_a_case_worked_by_hand():
    """1-D lattice: points 0 0 1 | 8 9 10, centroids start at 0 and 1"""
    X = np.array([[0], [0], [1], [8], [9], [10]], np.float32)
    labels, cent, n_iter, inertia = lloyd_ref(X, np.array([[0], [1]], np.float32))
    # assignment 1: {0, 0} | {1, 8, 9, 10} -> centroids 0, 7; 2: {0, 0, 1} | {8, 9, 10} -> 1/3, 9; 3: the same: stop
    assert labels.tolist() == [0, 0, 0, 1, 1, 1] and n_iter == 3
    np.testing.assert_array_equal(cent, np.array([[np.float32(1 / 3)], [9]], np.float32))
    want = 2 * float(np.float32(np.float32(1 / 3) ** 2)) + float(np.float32(np.float32(1 - np.float32(1 / 3)) ** 2)) + 2.0
    assert abs(inertia - want) < 1e-12
    # ties go to the smaller centroid index: the point 1 between the centroids 0 and 2
    labels, _, _, _ = lloyd_ref(np.array([[0], [1], [2]], np.float32), np.array([[0], [2]], np.float32), max_iter=1)
    assert labels.tolist() == [0, 0, 1]
    # max_iter = 1: one assignment, the centroids stay the given ones
    _, cent, n_iter, _ = lloyd_ref(X, np.array([[0], [1]], np.float32), max_iter=1)
    assert n_iter == 1 and cent.ravel().tolist() == [0, 1]


def test_lloyd_reseeds_an_emptied_cluster():
    """two of the three initial centroids coincide: the later one gets no cell (ties go to the smaller index) and takes the cell
    farthest from its centroid, the smaller index on ties"""
    X = np.array([[0], [1], [2], [10], [12], [12]], np.float32)
    init = np.array([[1], [1], [11]], np.float32)
    d = np.array([1, 0, 1, 1, 1, 1])   # squared distances after assignment 1: all ties at 1 -> cell 0
    assert d.max() == 1
    labels, cent, n_iter, _ = lloyd_ref(X, init, max_iter=2)
    # after assignment 1: clusters {0, 1, 2}, {}, {10, 12, 12} -> centroids 1, X[0] = 0, 34/3
    assert n_iter == 2 and cent.ravel().tolist() == [1.0, 0.0, float(np.float32(34 / 3))]
    assert labels.tolist() == [1, 0, 0, 2, 2, 2]
    labels, cent, n_iter, _ = lloyd_ref(X, init)
    assert labels.tolist() == [1, 0, 0, 2, 2, 2] and cent.ravel().tolist() == [1.5, 0.0, float(np.float32(34 / 3))] and n_iter == 3


def test_criterion_and_scores_from_a_dense_plan():
    # 4 x 6 plan with dyadic entries; clusters rows {0, 1} {2, 3}, columns {0, 1, 2} {3, 4} {5}
    P = np.array([[4, 4, 0, 0, 0, 0], [0, 0, 8, 0, 0, 0], [0, 0, 0, 2, 2, 0], [0, 0, 0, 2, 2, 8]], np.float64) / 32
    l0, l1 = [0, 0, 1, 1], [0, 0, 0, 1, 1, 2]
    # group 0's clusters: rows (4 4 8 0 0 0) / 16 and (0 0 0 4 4 8) / 16: entropies 1.5 ln 2 each
    assert abs(entropy_score_ref(P, l0, 2, 0) + 1.5 * np.log(2)) < 1e-15
    # group 1's clusters: columns summed: (8 8 0 0), (0 0 4 4), (0 0 0 8): entropies ln 2, ln 2, 0
    assert abs(entropy_score_ref(P, l1, 3, 1) + 2 * np.log(2) / 3) < 1e-15
    # ... and with the columns {0, 1} {2, 3, 4} {5}: (8 0 0 0), (0 8 4 4), (0 0 0 8): entropies 0, 1.5 ln 2, 0
    assert abs(entropy_score_ref(P, [0, 0, 1, 1, 1, 2], 3, 1) + 0.5 * np.log(2)) < 1e-15
    # a cluster without mass counts ln(n); a cluster without cells too
    assert abs(entropy_score_ref(P, [0, 0, 1, 1], 3, 0) + (3 * np.log(2) + np.log(6)) / 3) < 1e-15
    M, S = pair_scores_ref(P, l0, 2, l1, 3)
    np.testing.assert_array_equal(M, np.array([[16, 0, 0], [0, 8, 8]]) / 32)
    np.testing.assert_array_equal(S, np.array([[16 / 6, 0, 0], [0, 8 / 4, 8 / 2]]) / 32)
    M, S = pair_scores_ref(P, l0, 3, l1, 3)   # an empty cluster: zeros
    assert (M[2] == 0).all() and (S[2] == 0).all()
