"""CPU: the host side of ``match_transport_clusters`` -- tools/ot_segment_host_check.py at its small shapes, the marks and names of
the OTSEG core text, the numpy helpers of ``spvipes_amd.data`` (k-means++ seeding, the centroid update, the entropy criterion, the
block scores, the Hungarian naming) against tests/_ot_segment_reference.py and hand-made cases, the matrix-plan + ``cluster_key`` route
end to end on a duck AnnData without a device, and the refusals and signatures of the new public functions.  No GPU calls."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._ot_segment_reference import entropy_score_ref, pair_scores_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_tool_small_shapes():
    """the kernel's own walk, write-out, finish and merge, compiled for the CPU, against the reference (no sanitizer here)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ot_segment_host_check.py"), "--small"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all within bounds" in r.stdout and "DIFFER" not in r.stdout and r.stdout.count("one segment = softmin ok") >= 5


def test_the_core_text_is_marked_and_names_its_parts():
    text = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_ot_segments.h")).read()
    core = text[text.index("// ---- OTSEG-CORE-BEGIN ----"):text.index("// ---- OTSEG-CORE-END ----")]
    for name in ("OT_SEG_MAX = 256", "otseg_walk_init", "otseg_advance", "otseg_quiet", "otseg_add", "otseg_write", "otseg_finish", "otseg_merge", "otseg_splits",
                 "otseg_ws_bytes", "ot_update", "ot_merge", "ot_lse_value"):
        assert name in core
    assert "atomic" not in core and "__global__" not in core and "threadIdx" not in core
    assert "not bit for bit" in text and "scratch" in text
    for dp in ("16", "32", "64"):   # the resource table is there
        assert any(line.split()[1:2] == [dp] and len(line.split()) >= 7 for line in text.splitlines() if line.startswith("//   "))
    # the staging step the three transport kernels share takes any argument struct
    ot = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_ot.h")).read()
    assert "template <typename Args>\n__device__ __forceinline__ void ot_stage_h(const Args& a" in ot


def test_kmeans_pp_init():
    from spvipes_amd.data import kmeans_pp_init
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 6)).astype(np.float32)
    X[50:60] = X[0]   # duplicates of a row: at most one of them may be chosen
    for K in (1, 2, 7, 40):
        a, b = kmeans_pp_init(X, K, 5), kmeans_pp_init(X, K, 5)
        np.testing.assert_array_equal(a, b)
        assert a.shape == (K, 6) and a.dtype == np.float32 and len(np.unique(a, axis=0)) == K
        assert all((X == row).all(1).any() for row in a)   # rows of X
    assert not np.array_equal(kmeans_pp_init(X, 7, 5), kmeans_pp_init(X, 7, 6))
    # as many centroids as distinct rows: every one is taken; one more: refused
    Y = np.repeat(np.arange(5, dtype=np.float32)[:, None], 3, axis=0)
    assert sorted(kmeans_pp_init(Y, 5, 0).ravel().tolist()) == [0, 1, 2, 3, 4]
    for bad in (lambda: kmeans_pp_init(Y, 6, 0), lambda: kmeans_pp_init(Y, 0, 0), lambda: kmeans_pp_init(Y, 16, 0), lambda: kmeans_pp_init(Y[:, 0], 2, 0),
                lambda: kmeans_pp_init(Y, True, 0)):
        with pytest.raises(ValueError):
            bad()


def test_kmeans_update_and_cluster_segments():
    from spvipes_amd.data import cluster_segments, kmeans_update
    X = np.array([[0], [1], [2], [10], [12], [12]], np.float64)
    cent = kmeans_update(X, np.array([0, 0, 0, 2, 2, 2]), np.array([1, 0, 1, 1, 1, 1.0]), 3)
    assert cent.dtype == np.float32 and cent.ravel().tolist() == [1.0, 0.0, float(np.float32(34 / 3))]   # the empty cluster: cell 0, the first of the ties
    cent = kmeans_update(X, np.array([1, 1, 1, 1, 1, 1]), np.array([0, 3, 1, 3, 2, 0.0]), 4)
    assert cent.ravel().tolist() == [1.0, float(np.float32(37 / 6)), 10.0, 12.0]   # clusters 0, 2, 3 empty: cells 1, 3, then 4 (d 3, 3, 2): rows 1, 10, 12
    perm, seg_ptr, sizes = cluster_segments([2, 0, 2, 2, 0, 3], 5)
    assert perm.tolist() == [1, 4, 0, 2, 3, 5] and seg_ptr.tolist() == [0, 2, 2, 5, 6, 6] and seg_ptr.dtype == np.int32 and sizes.tolist() == [2, 0, 3, 1, 0]
    for bad in (lambda: cluster_segments([0, 5], 5), lambda: cluster_segments([0, -1], 5), lambda: cluster_segments([0], 0), lambda: cluster_segments([0], 257)):
        with pytest.raises(ValueError):
            bad()


def _plan(seed=0, n0=23, n1=31):
    rng = np.random.default_rng(seed)
    P = rng.random((n0, n1)) * (rng.random((n0, n1)) < 0.4)
    return P / P.sum()


def test_criterion_and_pair_scores_against_the_dense_reference():
    from spvipes_amd.data import cluster_entropy_score, cluster_pair_scores, cluster_tables_from_matrix
    import scipy.sparse as sp
    P = _plan()
    rng = np.random.default_rng(1)
    l0, l1 = rng.integers(0, 4, 23), rng.integers(0, 5, 31)
    P[:, l1 == 3] = 0.0     # a cluster of group 1 without any mass: every entry of its row is -inf
    P[l0 == 1, :] *= 1e-30   # and one whose masses are tiny against the others
    for plan in (P, sp.csr_matrix(P), P.astype(np.float32)):
        logT0, logT1 = cluster_tables_from_matrix(plan, l0, 4, l1, 6)   # cluster 5 of group 1 has no cell
        assert logT0.shape == (4, 31) and logT1.shape == (6, 23) and np.isneginf(logT1[[3, 5]]).all() and logT0.dtype == np.float64
        P64 = np.asarray(plan.todense() if sp.issparse(plan) else plan, dtype=np.float64)
        assert abs(cluster_entropy_score(logT0) - entropy_score_ref(P64, l0, 4, 0)) < 1e-12
        assert abs(cluster_entropy_score(logT1) - entropy_score_ref(P64, l1, 6, 1)) < 1e-12
        M, S = cluster_pair_scores(logT1, l0, np.bincount(l1, minlength=6), 4)
        M_ref, S_ref = pair_scores_ref(P64, l0, 4, l1, 6)
        np.testing.assert_allclose(M, M_ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S, S_ref, rtol=1e-12, atol=0)
        assert (M[:, [3, 5]] == 0).all() and (S[:, [3, 5]] == 0).all()
    # far below the range of exp: the criterion works through the row's maximum and does not underflow
    shifted = cluster_tables_from_matrix(P, l0, 4, l1, 6)[0] - 5000.0
    assert abs(cluster_entropy_score(shifted) - entropy_score_ref(P, l0, 4, 0)) < 1e-12
    assert cluster_entropy_score(np.full((3, 7), -np.inf)) == -np.log(7)   # no mass anywhere: every cluster counts as uniform
    assert cluster_entropy_score(np.array([[0.0, -np.inf, -np.inf]])) == 0.0
    for bad in (lambda: cluster_entropy_score(np.zeros(4)), lambda: cluster_entropy_score(np.array([[np.nan, 0.0]])), lambda: cluster_entropy_score(np.array([[np.inf, 0.0]])),
                lambda: cluster_pair_scores(np.zeros((2, 5)), [0, 1, 0], [1, 1]), lambda: cluster_pair_scores(np.zeros((2, 3)), [0, 1, 4], [1, 1], 3),
                lambda: cluster_tables_from_matrix(P[:, :5], l0, 4, l1, 6), lambda: cluster_tables_from_matrix(-P, l0, 4, l1, 6)):
        with pytest.raises(ValueError):
            bad()


def test_match_cluster_labels_on_hand_made_scores():
    from spvipes_amd.data import match_cluster_labels
    # square: the assignment 0-2, 1-0, 2-1, named in row order
    sq = np.array([[.1, .2, .9], [.8, .1, .1], [.2, .7, .1]])
    m = match_cluster_labels(sq)
    assert m["row_ind"].tolist() == [0, 1, 2] and m["col_ind"].tolist() == [2, 0, 1]
    assert m["names"] == (["Cluster_0", "Cluster_1", "Cluster_2"], ["Cluster_1", "Cluster_2", "Cluster_0"])
    # more rows than columns: rows 1 and 3 stay unmatched and get names of their OWN, ascending
    tall = np.array([[.9, .1], [.3, .2], [.1, .8], [.2, .3]])
    m = match_cluster_labels(tall)
    assert m["row_ind"].tolist() == [0, 2] and m["col_ind"].tolist() == [0, 1]
    assert m["names"] == (["Cluster_0", "Cluster_2", "Cluster_1", "Cluster_3"], ["Cluster_0", "Cluster_1"])
    # more columns than rows: group 1's unmatched clusters come after every matched pair
    m = match_cluster_labels(tall.T)
    assert m["row_ind"].tolist() == [0, 1] and m["col_ind"].tolist() == [0, 2]
    assert m["names"] == (["Cluster_0", "Cluster_1"], ["Cluster_0", "Cluster_2", "Cluster_1", "Cluster_3"])
    # both kinds of unmatched clusters cannot occur at once; 1 x 1
    assert match_cluster_labels(np.array([[0.0]]))["names"] == (["Cluster_0"], ["Cluster_0"])
    # ties: every assignment is optimal; the result is one of them, the same on every call, and a valid matching
    for tie in (np.ones((3, 3)), np.zeros((2, 4)), np.array([[1., 1.], [1., 1.], [0., 0.]])):
        a, b = match_cluster_labels(tie), match_cluster_labels(tie.copy())
        assert a["names"] == b["names"] and a["col_ind"].tolist() == b["col_ind"].tolist()
        k = min(tie.shape)
        assert len(a["row_ind"]) == k and len(set(a["col_ind"].tolist())) == k
        assert tie[a["row_ind"], a["col_ind"]].sum() == max(tie[list(r), list(c)].sum() for r, c in _matchings(tie.shape))
        names = a["names"][0] + a["names"][1]
        assert sorted(set(names), key=lambda s: int(s.split("_")[1])) == [f"Cluster_{i}" for i in range(max(tie.shape))]
    for bad in (np.zeros(3), np.zeros((0, 2)), np.array([[np.nan, 1.0]]), np.array([[np.inf, 1.0]])):
        with pytest.raises(ValueError):
            match_cluster_labels(bad)


def _matchings(shape):
    """every complete matching of the smaller side of a K0 x K1 table, as (rows, columns)"""
    from itertools import permutations
    K0, K1 = shape
    if K0 <= K1:
        return [(range(K0), p) for p in permutations(range(K1), K0)]
    return [(p, range(K1)) for p in permutations(range(K0), K1)]


class _Duck:
    def __init__(self, n0, n1, obs=None, obsm=None):
        self.n_obs, self.obs = n0 + n1, dict(obs or {})
        self.uns = {"groups_obs_indices": [np.arange(n0), n0 + np.arange(n1)]}
        if obsm is not None:
            self.obsm = obsm


def _block_case(seed=0):
    """three clusters per group, group 1's in another order and under other names; the plan is heavy on corresponding blocks"""
    rng = np.random.default_rng(seed)
    c0, c1 = rng.permutation(np.repeat([0, 1, 2], [9, 7, 8])), rng.permutation(np.repeat([0, 1, 2], [6, 10, 5]))
    P = 0.01 * rng.random((24, 21)) + 1.0 * (c0[:, None] == c1[None, :]) * rng.random((24, 21))
    P /= P.sum()
    names0, names1 = np.array(["T", "B", "NK"])[c0], np.array(["nk", "t", "b"])[np.array([1, 2, 0])[c1]]   # group 1: t = 0, b = 1, nk = 2
    return c0, c1, P, np.concatenate([names0, names1])


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_matrix_plan_with_cluster_key_needs_no_device(form):
    """the route of a plan made elsewhere and the user's own clusters, end to end on the host: corresponding blocks get one label"""
    import scipy.sparse as sp
    from spvipes_amd.model import spVIPES
    c0, c1, P, col = _block_case()
    ad = _Duck(24, 21, obs={"leiden": col})
    plan = P if form == "dense" else sp.csr_matrix(P.astype(np.float32))
    res = spVIPES.match_transport_clusters(ad, plan=plan, cluster_key="leiden")
    lab = np.asarray(ad.obs["processed_transport_labels"])
    assert lab.shape == (45,) and set(lab) == {"Cluster_0", "Cluster_1", "Cluster_2"}
    true = np.concatenate([c0, c1])
    for a in range(45):   # the partition by label is the partition by true block, across both groups
        np.testing.assert_array_equal(lab == lab[a], true == true[a])
    gcl = np.asarray(ad.obs["group_cluster_labels"])
    assert set(gcl[:24]) == {"0_T", "0_B", "0_NK"} and set(gcl[24:]) == {"1_t", "1_b", "1_nk"} and (gcl == np.char.add(np.repeat(["0_", "1_"], [24, 21]), col)).all()
    u = ad.uns["cluster_matching"]
    assert u["n_clusters"] == (3, 3) and u["candidates"] is None and u["mass"].shape == u["score"].shape == (3, 3) and list(u["criterion"][0]) == [3]
    assert u["cluster_values"] == [["B", "NK", "T"], ["b", "nk", "t"]] and u["row_ind"].tolist() == [0, 1, 2] and u["col_ind"].tolist() == [0, 1, 2]
    assert res.n_clusters == (3, 3) and res.names == u["names"] and [len(v) for v in res.labels] == [24, 21]
    M_ref, S_ref = pair_scores_ref(np.asarray(plan.todense() if form == "sparse" else plan, dtype=np.float64), res.labels[0], 3, res.labels[1], 3)
    np.testing.assert_allclose(u["mass"], M_ref, rtol=1e-12)
    np.testing.assert_allclose(u["score"], S_ref, rtol=1e-12)
    # a second call gives identical columns; setup_anndata then takes match_clusters=True
    again = _Duck(24, 21, obs={"leiden": col})
    spVIPES.match_transport_clusters(again, plan=plan, cluster_key="leiden")
    np.testing.assert_array_equal(again.obs["processed_transport_labels"], lab)
    ad.uns.update({"transport_plan": plan, "groups_lengths": {0: 1, 1: 1}, "groups_var_indices": [np.arange(1), np.arange(1)]})
    ad.obs.update({"groups": np.repeat(["a", "b"], [24, 21]), "indices": np.concatenate([np.arange(24), np.arange(21)])})
    spVIPES.setup_anndata(ad, groups_key="groups", transport_plan_key="transport_plan", match_clusters=True)
    # unequal numbers of clusters: the unmatched one keeps a name of its own
    col2 = col.astype("U8")   # room for the longer name
    col2[:24][(c0 == 2) & (np.arange(24) % 2 == 0)] = "NK2"
    ad2 = _Duck(24, 21, obs={"leiden": col2})
    res2 = spVIPES.match_transport_clusters(ad2, plan=plan, cluster_key="leiden")
    assert res2.n_clusters == (4, 3) and len(set(ad2.obs["processed_transport_labels"])) == 4
    assert len(set(np.asarray(ad2.obs["processed_transport_labels"])[24:])) == 3


def test_setup_anndata_names_the_method_when_the_column_is_absent():
    from spvipes_amd.model import spVIPES
    ad = _Duck(4, 3, obs={"groups": np.repeat(["a", "b"], [4, 3]), "indices": np.arange(7)})
    ad.uns["transport_plan"] = np.ones((4, 3))
    with pytest.raises(NotImplementedError, match="match_transport_clusters"):
        spVIPES.setup_anndata(ad, groups_key="groups", transport_plan_key="transport_plan", match_clusters=True)


def test_match_transport_clusters_refuses_before_any_device_work():
    """each of these returns from an argument check: nothing is written to the AnnData and no device is asked for"""
    from spvipes_amd.model import spVIPES
    rep = {"X_pca": np.zeros((12, 5), np.float32)}
    P = np.ones((7, 5)) / 35

    def duck(**obs):
        return _Duck(7, 5, obs=obs, obsm=rep)
    cases = [(duck(), dict(use_rep="X_umap"), KeyError, "X_umap"), (duck(), dict(use_rep=np.zeros((11, 5))), ValueError, "one row per cell"),
             (duck(), dict(use_rep="X_pca", plan=np.ones((5, 7))), ValueError, "plan must be"), (duck(), dict(use_rep="X_pca", plan="plan"), ValueError, "plan must be"),
             (duck(), dict(use_rep="X_pca", plan=P, n_clusters=0), ValueError, "n_clusters"), (duck(), dict(use_rep="X_pca", plan=P, n_clusters=()), ValueError, "n_clusters"),
             (duck(), dict(use_rep="X_pca", plan=P, n_clusters=(4, 257)), ValueError, "n_clusters"), (duck(), dict(use_rep="X_pca", plan=P, n_clusters=2.0), ValueError, "n_clusters"),
             (duck(), dict(use_rep="X_pca", plan=P, n_clusters=(6, 8)), ValueError, "exceeds"), (duck(), dict(use_rep="X_pca", plan=P, n_init=0), ValueError, "n_init"),
             (duck(), dict(use_rep="X_pca", plan=P, seed=-1), ValueError, "seed"), (duck(), dict(use_rep="X_pca", plan=P, cluster_key="leiden"), KeyError, "leiden"),
             (duck(), dict(plan=P), ValueError, "use_rep is needed"), (duck(), dict(use_rep=np.zeros((12, 65)), plan=P), ValueError, "columns"),
             (duck(), dict(use_rep=np.full((12, 5), np.nan), plan=P), ValueError, "non-finite")]
    for ad, kw, exc, text in cases:
        with pytest.raises(exc, match=text):
            spVIPES.match_transport_clusters(ad, **kw)
        assert "cluster_matching" not in ad.uns and "transport_plan" not in ad.uns and not set(ad.obs) & {"processed_transport_labels", "group_cluster_labels", "indices"}
    ad = duck()
    del ad.uns["groups_obs_indices"]
    with pytest.raises(ValueError, match="groups_obs_indices"):
        spVIPES.match_transport_clusters(ad, "X_pca")


def test_signatures_and_host_tensor_refusals():
    from spvipes_amd import _abi
    from spvipes_amd.cluster_ops import cluster_transport_log_mass, kmeans, kmeans_best
    from spvipes_amd.data import kmeans_pp_init
    from spvipes_amd.model import spVIPES
    from spvipes_amd.ot_ops import ot_segment_lse, ot_segment_splits, ot_segment_ws_bytes
    p = inspect.signature(spVIPES.match_transport_clusters).parameters
    assert list(p) == ["adata", "use_rep", "plan", "n_clusters", "cluster_key", "n_init", "seed", "device"]
    assert [p[n].default for n in list(p)[2:]] == [None, (4, 6, 8, 12, 16, 24, 32), None, 4, 0, None]
    p = inspect.signature(ot_segment_lse).parameters
    assert list(p) == ["X", "Y", "h", "seg_ptr", "inv_eps", "n_split", "out"] and (p["n_split"].default, p["out"].default) == (0, None)
    assert list(inspect.signature(ot_segment_splits).parameters) == ["n_q", "n_c"] and list(inspect.signature(ot_segment_ws_bytes).parameters) == ["n_q", "n_seg", "n_split"]
    p = inspect.signature(kmeans).parameters
    assert list(p) == ["X_dev", "init", "max_iter"] and p["max_iter"].default == 50
    p = inspect.signature(kmeans_best).parameters
    assert list(p)[:4] == ["X_dev", "K", "n_init", "seed"] and (p["n_init"].default, p["seed"].default) == (4, 0)
    assert list(inspect.signature(kmeans_pp_init).parameters) == ["X", "K", "seed"]
    assert list(inspect.signature(cluster_transport_log_mass).parameters)[:5] == ["res", "X_q", "X_c", "labels_c", "side"]
    # the op's own checks come first: a host tensor is refused before the library is asked for anything
    X, Y, h = torch.zeros((4, 5)), torch.zeros((9, 5)), torch.zeros(9)
    with pytest.raises(_abi.SpvError):
        ot_segment_lse(X, Y, h, torch.tensor([0, 9], dtype=torch.int32), 1.0)
    with pytest.raises(_abi.SpvError):
        kmeans(X, np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError, match="init must"):
        kmeans(X, np.zeros((2, 4), np.float32))
