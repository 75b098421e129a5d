"""CPU: the yardstick of the t-SNE tests (tests/_tsne_reference.py) held to what does not depend on it -- its analytic gradient against
central finite differences of its own float64 KL divergence and, where scikit-learn imports, against ``_kl_divergence`` -- and mutation
checks in the manner of tests/test_gemm_reference_cpu.py: a reference that is wrong in one way a kernel could be wrong must leave the
bound the GPU tests hold the kernel to, on the very inputs those tests use.  No GPU."""
import numpy as np
import pytest

from tests import _tsne_reference as R


def _small(D, n=40, seed=0):
    rng = np.random.default_rng([seed, D])
    X = rng.standard_normal((n, 5)).astype(np.float32)
    return R.knn_p(X, 5.0, 15), rng.standard_normal((n, D))


@pytest.mark.parametrize("D", [2, 3])
def test_analytic_gradient_matches_finite_differences_of_the_kl(D):
    """central differences with h = 1e-5: truncation ~ h^2 |third derivative| / 6, rounding ~ 2^-53 KL / h ~ 1e-11 against gradients of 1e-2"""
    P, Y = _small(D)
    assert abs(P.sum() - 1.0) < 1e-12 and np.array_equal(P, P.T)
    g, h = R.grad_ref(Y, P), 1e-5
    fd = np.zeros_like(g)
    for i in range(Y.shape[0]):
        for t in range(D):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, t] += h
            Ym[i, t] -= h
            fd[i, t] = (R.kl_ref(Yp, P) - R.kl_ref(Ym, P)) / (2 * h)
    assert np.abs(g).max() > 1e-3
    assert np.abs(fd - g).max() <= 1e-8 * max(1.0, np.abs(g).max())


@pytest.mark.parametrize("D", [2, 3])
def test_gradient_and_kl_match_scikit_learn(D):
    tsne_mod = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    P, Y = _small(D)
    kl, grad = tsne_mod._kl_divergence(Y.ravel(), squareform(P, checks=False), 1.0, Y.shape[0], D)
    assert abs(kl - R.kl_ref(Y, P)) <= 1e-9 * abs(kl) + 1e-12   # scikit-learn clamps P and Q at 2.2e-16
    assert np.abs(grad.reshape(Y.shape) - R.grad_ref(Y, P)).max() <= 1e-9


def test_update_reference_gradient_is_the_dense_one():
    """``update_ref``'s CSR route and ``grad_ref``'s dense route are two codes for one formula"""
    c = R.update_case()
    r = R.update_ref(c)
    dense = R.grad_ref(c["y"], R.dense_p(c["indptr"], c["cols"], c["vals"], c["n"]), c["alpha"])
    assert np.abs(r["grad"].T - dense).max() <= 1e-12 * np.abs(dense).max()
    assert abs(float(c["vals"].astype(np.float64).sum()) - 1.0) < 1e-5
    assert np.diff(c["indptr"])[5] == 0 and np.diff(c["indptr"])[9] == c["n"] - 2   # an empty row; a full one (all but itself and row 5)


def test_update_case_leaves_few_gain_decisions_open():
    """the GPU test lets a gain differ only where the reference's |g| is below its own error bound: at most 1 % of the elements,
    and this seed keeps the reference alone well under it"""
    for D in (1, 2, 3, 4):
        r = R.update_ref(R.update_case(D=D))
        assert r["unsure"].mean() <= 0.01


# the GPU tests' own shapes (tests/test_tsne_gpu_repulsion.py): every mutant on the largest of them
@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["spread", "same"])
def test_mutants_leave_the_gpu_tests_bound(kind, D):
    n_q, n_c, n_split = 300, 1000, 3
    Q, C = R.repulsion_case(kind, n_q, n_c, D)
    ex = np.arange(n_q) if kind == "same" else None
    ref = R.repulsion_ref(Q, C, ex)
    bZ, bF = R.repulsion_bound(ref, D)
    for mutant in ("drop_last", "w_for_w2") + (("self",) if ex is not None else ()):
        bad = R.repulsion_ref(Q, C, ex, mutant=mutant, n_split=n_split)
        out_z, out_f = np.abs(bad["Z"] - ref["Z"]) > bZ, np.abs(bad["F"] - ref["F"]) > bF
        if mutant == "drop_last":
            assert out_z.all() and out_f.mean() > 0.9, mutant     # one term of a thousand against 1e-6 of their sum
        elif mutant == "w_for_w2":
            assert out_f.mean() > 0.9 and not out_z.any(), mutant  # Z does not use w2
        else:
            assert out_z.all(), mutant                             # w = 1 more per query; its force term is 0


def test_bounds_are_not_vacuous():
    """the bound is a few 1e-7 of the sum: far below any single term of the shapes above"""
    Q, C = R.repulsion_case("spread", 300, 1000, 2)
    ref = R.repulsion_ref(Q, C)
    bZ, bF = R.repulsion_bound(ref, 2)
    assert (bZ <= 4e-7 * ref["absZ"]).all() and (bF <= 1e-6 * ref["absF"] + 1e-40).all()
    assert R.c_z(2) == 6 and R.c_f(2) == 15 and R.c_f(4) == 19


def test_affinities_reference_hits_the_perplexity():
    rng = np.random.default_rng(5)
    d2 = np.sort(rng.gamma(2.0, 2.0, (50, 60)).astype(np.float32), axis=1)
    P, beta, conv = R.affinities_ref(d2, 20.0)
    assert conv.all() and np.allclose(P.sum(axis=1), 1.0, atol=1e-12)
    assert max(abs(R.entropy_of(P[i]) - np.log(20.0)) for i in range(50)) <= 1e-5 + 1e-12
    shifted, beta2, _ = R.affinities_ref(d2 + np.float32(8.0), 20.0)
    assert np.allclose(shifted, P, atol=1e-6)    # d = d2 - d2[0]: a common offset changes only fp32 roundings of the input


def test_planted_blobs_meet_the_api_tests_conditions_in_float64():
    """the GPU API test's conditions (iii) and (iv) on its own inputs, by the float64 prototype of the schedule: the final KL is below
    0.75 of the KL at step 250 and at least 97 % of the cells have their nearest neighbour in their own blob"""
    X, lab = R.blobs(0)
    P = R.knn_p(X, 20.0, 60)
    Y, kls = R.layout_ref(P, R.pca_ref(X, 2), 500, marks=(250,))
    assert R.kl_ref(Y, P) < 0.75 * kls[250]
    assert R.neighbour_share(Y, lab) >= 0.97
