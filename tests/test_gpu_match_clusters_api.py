"""GPU: ``cluster_ops.kmeans`` against the plain Lloyd loop of tests/_ot_segment_reference.py, and
``spVIPES.match_transport_clusters`` end to end on two groups of five Gaussian blobs: the criterion of every candidate against float64
on the same labels, the chosen K, the matched partition, what is written, and a cluster-PoE model trained on the result.  Every test
here needs the feature and fails without it.

The blobs: D = 10, centres 4 x N(0, 1), sigma 0.5, sizes (90, 70, 110, 60, 80) and (50, 80, 40, 70, 60), the second group shifted by 0.3
and its rows permuted.  In float64 on the CPU (500 Sinkhorn iterations at epsilon 0.05 x the mean cost) the criterion picks 5 of
(3, 4, 5, 6, 8) in both groups, 0.08 and 0.05 ahead of the runner-up, and matching by mean mass pairs the true blobs.

THE BOUND ON THE CRITERION.  log T[c, i] = L[c][i] + r_i errs by at most B = ``lse_bound`` (tests/test_gpu_ot_segments.py) plus the
one float64 rounding of the addition.  A cluster's distribution is p_i = T_i / Z; moving every log T_i by at most B moves every log p_i
by at most 2 B (B of its own, B through log Z).  The entropy is H = -sum_i p_i log p_i: to first order its change is
-sum_i dp_i (log p_i + 1) with |dp_i| <= 2 B p_i, i.e. at most 2 B sum_i p_i (|log p_i| + 1) = 2 B (H + 1); twice that, 4 B (H + 1),
covers the second-order terms for the B of these shapes (about 1e-4).  The criterion is a mean of such entropies, so the same bound
holds for it with H the largest of them."""
import numpy as np
import pytest
import torch

from tests._knn_reference import exact_d2
from tests._ot_reference import lse_ref, t_ref
from tests._ot_segment_reference import cluster_entropies_ref, lloyd_ref, pair_scores_ref
from tests.test_gpu_ot_segments import lse_bound

pytestmark = pytest.mark.gpu

SIZES = ((90, 70, 110, 60, 80), (50, 80, 40, 70, 60))
CANDIDATES = (3, 4, 5, 6, 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _blobs(seed=0):
    """[(X float32 [n_g, 10], true blob [n_g])] for the two groups"""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((5, 10))
    out = []
    for g, sizes in enumerate(SIZES):
        true = np.repeat(np.arange(5), sizes)
        X = centres[true] + 0.5 * rng.standard_normal((len(true), 10)) + (0.3 if g == 1 else 0.0)
        if g == 1:
            p = rng.permutation(len(true))
            X, true = X[p], true[p]
        out.append((X.astype(np.float32), true))
    return out


def _adata():
    """the duck (410 / 300 cells, 60 genes each) with the blobs as the common representation"""
    from tests._duck import make_duck
    (X0, t0), (X1, t1) = _blobs()
    ad = make_duck(n=(len(X0), len(X1)), G=(60, 60), seed=4)
    ad.obsm = {"X_rep": np.concatenate([X0, X1])}
    return ad, np.concatenate([t0, t1])


@pytest.mark.parametrize("case", ["plain", "a-cluster-empties"])
def test_kmeans_equals_the_reference_lloyd(dev, case):
    """labels, fp32 centroids, the number of assignment steps and the inertia, all EQUAL: the assignment is the exact k-NN kernel (the
    reference's distance chain, ties to the smaller index), the update is fp64 sums in cell order"""
    from spvipes_amd.cluster_ops import kmeans
    rng = np.random.default_rng(7)
    X = (3.0 * rng.standard_normal((4, 10))[rng.integers(0, 4, 300)] + rng.standard_normal((300, 10))).astype(np.float32)
    init = X[[5, 17, 100, 230, 299]].copy()
    if case == "a-cluster-empties":
        init[3] = init[1]   # two equal centroids: ties go to the smaller index, the later one gets no cell and is re-seeded
    want_labels, want_cent, want_iter, want_inertia = lloyd_ref(X, init)
    if case == "a-cluster-empties":
        first = exact_d2(X, init)
        assert not (np.lexsort((np.broadcast_to(np.arange(5), first.shape), first), axis=1)[:, 0] == 3).any()   # cluster 3 does empty
    got = kmeans(torch.from_numpy(X).to(dev), init)
    assert got.n_iter == want_iter and got.converged and 2 < want_iter < 50
    np.testing.assert_array_equal(got.labels, want_labels)
    np.testing.assert_array_equal(got.centroids.view(np.uint32), want_cent.view(np.uint32))
    assert got.inertia == want_inertia and len(np.unique(got.labels)) == 5
    capped = kmeans(torch.from_numpy(X).to(dev), init, max_iter=2)
    ref = lloyd_ref(X, init, max_iter=2)
    assert capped.n_iter == 2 and not capped.converged
    np.testing.assert_array_equal(capped.labels, ref[0])
    np.testing.assert_array_equal(capped.centroids.view(np.uint32), ref[1].view(np.uint32))


@pytest.fixture(scope="module")
def matched(dev):
    from spvipes_amd.model import spVIPES
    ad, true = _adata()
    plan = spVIPES.compute_transport_plan(ad, "X_rep", k=32, max_iter=500)
    cm = spVIPES.match_transport_clusters(ad, use_rep="X_rep", plan=plan, n_clusters=CANDIDATES)
    return ad, true, plan, cm


def test_criterion_choice_and_matching_on_the_blobs(dev, matched):
    from spvipes_amd.cluster_ops import kmeans_best
    ad, true, plan, cm = matched
    res = plan.sinkhorn
    X = [ad.obsm["X_rep"][:410], ad.obsm["X_rep"][410:]]
    pot = [(res.phi + res.log_a).cpu().numpy(), (res.psi + res.log_b).cpu().numpy()]   # float32 additions, as the driver makes them
    dense = {}
    for g in range(2):
        q = 1 - g   # the queries are the OTHER group's cells
        t = t_ref(X[q], X[g], pot[g], res.inv_eps)
        # the float64 plan from the device's potentials and the kernel's own float32 t: rows = group g's cells
        P = np.exp(t.astype(np.float64).T + pot[q].astype(np.float64)[None, :])
        dense[g] = P
        assert abs(P.sum() - 1) < 1e-2   # a plan
        n_q, n_c = len(X[q]), len(X[g])
        crit64, H_max, B = {}, 0.0, 0.0
        for K in CANDIDATES:
            labels = kmeans_best(torch.from_numpy(X[g]).to(dev), K, 4, 0).labels
            H = cluster_entropies_ref(P, labels, K, 0)
            crit64[K], H_max = -float(H.mean()), max(H_max, float(H.max()))
            L_ref = np.stack([lse_ref(t[:, labels == c]) for c in range(K)], axis=1)
            log_mass = L_ref + pot[q].astype(np.float64)[:, None]
            B = max(B, float(lse_bound(L_ref, n_q, n_c, 0).max()) + 2.0 ** -53 * float(np.abs(log_mass).max()))
        bound = 4 * B * (H_max + 1)
        order = sorted(crit64, key=lambda K: -crit64[K])
        margin = crit64[order[0]] - crit64[order[1]]
        print(f"group {g}: float64 criterion {crit64}, margin {margin:.4f}, device {cm.criterion[g]}, B {B:.3e}, H {H_max:.3f}, bound {bound:.3e}")
        assert order[0] == 5 and margin >= 10 * bound, "the reference's own margin must dwarf the bound"
        assert sorted(cm.criterion[g]) == list(CANDIDATES)
        for K in CANDIDATES:
            assert abs(cm.criterion[g][K] - crit64[K]) <= bound, (g, K)
    assert cm.n_clusters == (5, 5) and cm.candidates == CANDIDATES
    # the partition by processed label is the partition by true blob, across both groups
    lab = np.asarray(ad.obs["processed_transport_labels"])
    assert set(lab) == {f"Cluster_{m}" for m in range(5)}
    for a in range(len(lab)):
        np.testing.assert_array_equal(lab == lab[a], true == true[a])
    # the block masses against the float64 plan: every log mass within B, so every mass within expm1(B) relative
    M_ref, S_ref = pair_scores_ref(dense[0], cm.labels[0], 5, cm.labels[1], 5)
    np.testing.assert_allclose(cm.mass, M_ref, rtol=1e-3)
    np.testing.assert_allclose(cm.score, S_ref, rtol=1e-3)
    assert abs(cm.mass.sum() - dense[0].sum()) < 1e-3


def test_what_is_written_and_that_it_repeats(dev, matched):
    from spvipes_amd.model import spVIPES
    ad, true, plan, cm = matched
    u = ad.uns["cluster_matching"]
    assert u["n_clusters"] == (5, 5) and u["candidates"] == CANDIDATES and u["mass"].shape == u["score"].shape == (5, 5)
    assert sorted(u["row_ind"].tolist()) == list(range(5)) and sorted(u["col_ind"].tolist()) == list(range(5))
    assert [sorted(n) for n in u["names"]] == [[f"Cluster_{m}" for m in range(5)]] * 2 and u["criterion"] == cm.criterion
    assert "labels" not in u and [len(v) for v in cm.labels] == [410, 300]
    gcl, lab = np.asarray(ad.obs["group_cluster_labels"]), np.asarray(ad.obs["processed_transport_labels"])
    for g, rows in enumerate((slice(0, 410), slice(410, 710))):
        np.testing.assert_array_equal(gcl[rows], np.array([f"{g}_{k}" for k in range(5)])[cm.labels[g]])
        np.testing.assert_array_equal(lab[rows], np.array(cm.names[g])[cm.labels[g]])
    # a second call gives identical columns; plan=None computes the plan itself and writes it as usual
    ad2, _ = _adata()
    cm2 = spVIPES.match_transport_clusters(ad2, use_rep="X_rep", plan=plan, n_clusters=CANDIDATES)
    np.testing.assert_array_equal(ad2.obs["processed_transport_labels"], lab)
    np.testing.assert_array_equal(ad2.obs["group_cluster_labels"], gcl)
    assert cm2.criterion == cm.criterion and np.array_equal(cm2.mass, cm.mass)
    ad3, _ = _adata()
    del ad3.obs["indices"]
    cm3 = spVIPES.match_transport_clusters(ad3, use_rep="X_rep", n_clusters=5, n_init=2)
    assert "transport_plan" in ad3.uns and "indices" in ad3.obs and cm3.n_clusters == (5, 5) and cm3.candidates is None
    lab3 = np.asarray(ad3.obs["processed_transport_labels"])
    for a in range(0, len(lab3), 7):
        np.testing.assert_array_equal(lab3 == lab3[a], true == true[a])
    # the user's own clusters with the device's potentials: the true blobs under other names
    ad4, _ = _adata()
    ad4.obs["leiden"] = np.array(["e", "d", "c", "b", "a"])[true]
    cm4 = spVIPES.match_transport_clusters(ad4, use_rep="X_rep", plan=plan, cluster_key="leiden")
    assert cm4.n_clusters == (5, 5) and cm4.row_ind.tolist() == cm4.col_ind.tolist() == list(range(5))
    assert set(np.asarray(ad4.obs["group_cluster_labels"])[:410]) == {f"0_{v}" for v in "abcde"}


def test_cluster_poe_model_trains_on_the_matched_labels(dev, matched):
    from spvipes_amd.model import spVIPES
    ad, _, _, _ = matched
    spVIPES.setup_anndata(ad, groups_key="groups", transport_plan_key="transport_plan", match_clusters=True)
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32")
    assert not model.module.pair_data and model._components is not None   # cluster-PoE mode
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=100, max_epochs=1, train_size=1.0)
    losses = [v for key, vals in model.history.items() if "loss" in key or "elbo" in key for v in vals]
    assert model.is_trained_ and losses and np.isfinite(losses).all()
    # without the column setup_anndata still refuses, and says what to run
    fresh, _ = _adata()
    fresh.uns["transport_plan"] = ad.uns["transport_plan"]
    with pytest.raises(NotImplementedError, match="match_transport_clusters"):
        spVIPES.setup_anndata(fresh, groups_key="groups", transport_plan_key="transport_plan", match_clusters=True)
