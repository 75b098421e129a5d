"""CPU: the host side of the LISI read-out -- the float64 reference of tests/_lisi_reference.py on known answers, that it converges on at
least 90 % of the ordinary rows of the GPU test's cases, ``paged_ref`` against a plain sort, tools/lisi_host_check.py at its small shapes,
``data.check_lisi_args`` / ``lisi_frame`` / ``lisi_scaled`` / ``check_lisi_keys`` / ``lisi_rep_frame``, and the argument refusals of
``latent_lisi`` / ``spVIPES.lisi`` (on objects that are no model: they must refuse before they touch one).  No GPU calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._lisi_reference import GPU_CASES, calibrate, entropy, lisi_ref, make_lists, ordinary_rows, paged_ref, perplexity_of, row_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(n=7, k=40, n_c=60, seed=0):
    idx, dist, _codes = make_lists(np.random.default_rng(seed), 3, k, n_c, 1)   # 3 rows: no degenerate ones
    return np.repeat(idx, (n + 2) // 3, axis=0)[:n], np.repeat(dist, (n + 2) // 3, axis=0)[:n]


def test_reference_one_label_gives_one():
    idx, dist = _lists()
    out, beta, n_valid, conv, H = lisi_ref(idx, dist, np.full((1, 60), 3), 10.0)
    np.testing.assert_allclose(out, 1.0, rtol=1e-14)
    assert conv.all() and (n_valid == 40).all() and (np.abs(H - np.log(10.0)) < 1e-5).all()


def test_reference_equidistant_neighbours():
    """p_j = 1 / k whatever beta is: 1 / sum (n_l / k)^2"""
    rng = np.random.default_rng(1)
    k, n_c = 30, 50
    idx = np.stack([rng.permutation(n_c)[:k] for _ in range(5)])
    codes = rng.integers(0, 4, (2, n_c))
    out, beta, _nv, conv, _H = lisi_ref(idx, np.full((5, k), np.float32(1.5)), codes, 10.0)
    for t in range(2):
        want = [1.0 / ((np.bincount(codes[t][row], minlength=4) / k) ** 2).sum() for row in idx]
        np.testing.assert_allclose(out[t], want, rtol=1e-13)
    assert not conv.any() and (beta == 2.0 ** 50).all()   # H = log 30 > log 10 at every beta: 50 doublings
    out2, beta2, _nv, conv2, _H = lisi_ref(idx, np.full((5, k), np.float32(1.5)), codes, 30.0)
    assert conv2.all() and (beta2 == 1).all()
    np.testing.assert_allclose(out2, out, rtol=1e-13)


def test_reference_is_invariant_under_renaming():
    idx, dist, codes = make_lists(np.random.default_rng(2), 9, 50, 70, 3)
    a = lisi_ref(idx, dist, codes, 12.0)
    b = lisi_ref(idx, dist, np.where(codes >= 0, 1000 - 3 * codes, -9), 12.0)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_reference_entropy_at_the_returned_beta_and_degenerate_rows():
    idx, dist, codes = make_lists(np.random.default_rng(3), 12, 89, 120, 2)
    out, beta, n_valid, conv, H = lisi_ref(idx, dist, codes, 30.0)
    assert conv[ordinary_rows(12)].all() and (np.abs(H[conv] - np.log(30.0)) < 1e-5).all()
    for i in np.flatnonzero(conv):
        d, valid = row_distances(dist[i])
        assert calibrate(d, valid, 30.0) == (beta[i], True) and abs(entropy(d, valid, beta[i])[0] - np.log(30.0)) < 1e-5
    assert np.isnan(out[:, 2]).all() and beta[2] == 1 and n_valid[2] == 0 and not conv[2] and np.isnan(H[2])   # the empty row
    assert n_valid[1] == 44 and n_valid[3] == 89
    # the invalid indices of row 3 count in the calibration and for no label: dropping their mass lowers the Simpson index
    fixed = idx.copy()
    fixed[3, ::3] = 0
    assert (lisi_ref(fixed, dist, codes, 30.0)[1] == beta).all()
    p = entropy(*row_distances(dist[3]), beta[3])[1]
    keep = np.arange(89) % 3 != 0
    for t in range(2):
        row = codes[t][idx[3][keep]]
        want = sum(p[keep][row == c].sum() ** 2 for c in np.unique(row[row >= 0]))
        assert abs(1 / out[t, 3] - want) < 1e-15
    # 1 <= lisi <= the number of labels where every neighbour has one
    full = lisi_ref(idx[4:], dist[4:], np.abs(codes), 30.0)[0]
    assert (full >= 1 - 1e-12).all() and (full <= 4 + 1e-12).all()


def test_the_reference_converges_on_the_gpu_cases():
    """the GPU test leaves the rows the reference does not converge on out of two of its checks: at most 10 % of the ordinary rows"""
    for n, k, n_c, n_sets in GPU_CASES:
        idx, dist, codes = make_lists(np.random.default_rng(1000 * n + 10 * k + n_sets), n, k, n_c, 1)
        conv = lisi_ref(idx, dist, codes, perplexity_of(k))[3]
        assert conv[ordinary_rows(n)].mean() >= 0.9, (n, k)


def test_paged_reference_is_a_plain_sort():
    rng = np.random.default_rng(4)
    Q, C = (rng.integers(-32, 33, (n, 1)).astype(np.float32) / 4 for n in (6, 200))   # 65 coordinates for 200 candidates: ties everywhere
    plain = ((Q[:, None, :] - C[None]) ** 2).sum(-1, dtype=np.float32)   # exact on this lattice
    ex = np.array([3, -1, 200, 0, 5, 199], np.int32)
    idx, dist = paged_ref(Q, C, 130, ex)
    for i in range(6):
        pairs = sorted((plain[i, j], j) for j in range(200) if j != ex[i])[:130]
        assert [j for _, j in pairs] == idx[i].tolist() and [v for v, _ in pairs] == dist[i].tolist()
    assert (dist[:, 63] == dist[:, 64]).any() and (dist[:, 127] == dist[:, 128]).any()   # ties across the page boundaries
    idx, dist = paged_ref(Q, C[:70], 130)
    assert (idx[:, 70:] == -1).all() and np.isinf(dist[:, 70:]).all() and (idx[:, :70] >= 0).all()


def test_host_check_tool_small_shapes():
    """the paging predicate with the list handling, the calibration and the Simpson step, compiled for the CPU, against the reference"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lisi_host_check.py"), "--small"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all hold" in r.stdout and "DIFFER" not in r.stdout


def test_check_lisi_args():
    from spvipes_amd.data import check_lisi_args, lisi_neighbors
    assert check_lisi_args(50000, 30) == 89 and check_lisi_args(50, 30) == 49 and check_lisi_args(1000, 85.67) == 256 and check_lisi_args(10, 1) == 2
    assert check_lisi_args(1000, np.float64(30.0)) == 89 and lisi_neighbors(30, 2) == 1
    for n, perp, text in ((1000, 86, "k must lie"), (1000, 1000, "k must lie"), (1, 30, "k must lie"), (1000, 0.5, "perplexity"), (1000, float("nan"), "perplexity"),
                          (1000, float("inf"), "perplexity"), (1000, "30", "perplexity"), (1000, True, "perplexity"), (1000, None, "perplexity")):
        with pytest.raises(ValueError, match=text):
            check_lisi_args(n, perp)


def test_lisi_scaled():
    from spvipes_amd.data import lisi_scaled
    assert lisi_scaled(1.5, 2, "ilisi") == 0.5 and lisi_scaled(1.0, 2, "ilisi") == 0.0 and lisi_scaled(2.0, 2, "ilisi") == 1.0
    assert lisi_scaled(1.0, 5, "clisi") == 1.0 and lisi_scaled(5.0, 5, "clisi") == 0.0 and lisi_scaled(2.0, 5, "clisi") == 0.75
    assert np.isnan(lisi_scaled(1.0, 1, "ilisi")) and np.isnan(lisi_scaled(1.0, 1, "clisi")) and np.isnan(lisi_scaled(np.nan, 3, "clisi"))
    with pytest.raises(ValueError):
        lisi_scaled(1.0, 2, "lisi")


def test_lisi_frame():
    from spvipes_amd.data import lisi_frame
    grp = np.array([0, 0, 0, 1, 1, 1])
    cats, codes = np.array(["B", "NK", "T"]), np.array([0, 2, 2, 0, 2, 1])
    il = np.array([1.2, 1.9, np.nan, 1.4, 1.6, 1.0])
    cl = np.array([1.0, 1.5, 2.5, 1.1, np.nan, 3.0])
    f = lisi_frame(list("abcdef"), grp, cats, codes, il, cl, [5, 5, 0, 5, 4, 5], [1, 1, 0, 1, 1, 0], 2.0, 5)
    assert list(f.columns) == ["group", "label", "ilisi", "clisi", "n_neighbors", "converged"] and list(f.index) == list("abcdef")
    assert f["label"].tolist() == ["B", "T", "T", "B", "T", "NK"] and f["converged"].tolist() == [True, True, False, True, True, False]
    assert f["n_neighbors"].tolist() == [5, 5, 0, 5, 4, 5] and f["converged"].dtype == bool
    a = f.attrs
    assert a["ilisi_median"] == 1.4 and a["clisi_median"] == 1.5 and a["ilisi_scaled"] == pytest.approx(0.4) and a["clisi_scaled"] == 0.75
    assert (a["perplexity"], a["n_neighbors"], a["n_unconverged"]) == (2.0, 5, 2)
    per = a["per_label"]
    assert list(per.index) == ["B", "NK", "T"] and list(per.columns) == ["n_group0", "n_group1", "ilisi", "clisi"]
    assert per["n_group0"].tolist() == [1, 0, 2] and per["n_group1"].tolist() == [1, 1, 1]
    np.testing.assert_allclose(per["ilisi"], [1.3, 1.0, 1.75])
    np.testing.assert_allclose(per["clisi"], [1.05, 3.0, 2.0])
    # one group: a NaN ilisi column whatever is passed; one label: NaN scaled score
    g = lisi_frame(np.arange(3), np.zeros(3, dtype=int), np.array(["x"]), np.zeros(3, dtype=int), None, np.ones(3), [2, 2, 2], [1, 1, 1], 1.0, 2)
    assert np.isnan(g["ilisi"]).all() and np.isnan(g.attrs["ilisi_median"]) and np.isnan(g.attrs["ilisi_scaled"])
    assert g.attrs["clisi_median"] == 1.0 and np.isnan(g.attrs["clisi_scaled"]) and g.attrs["n_unconverged"] == 0
    assert np.isnan(lisi_frame(np.arange(3), np.ones(3, dtype=int), None, None, np.full(3, 1.5), None, [2, 2, 2], [1, 1, 1], 1.0, 2)["ilisi"]).all()
    # no labels: no clisi column, no clisi attrs, no per_label
    h = lisi_frame(np.arange(6), grp, None, None, il, None, [5] * 6, [1] * 6, 2.0, 5)
    assert list(h.columns) == ["group", "label", "ilisi", "n_neighbors", "converged"] and h["label"].tolist() == [None] * 6
    assert "clisi_median" not in h.attrs and "clisi_scaled" not in h.attrs and h.attrs["per_label"] is None and h.attrs["ilisi_median"] == 1.4
    with pytest.raises(ValueError):
        lisi_frame(np.arange(6), grp, cats, codes, il[:5], cl, [5] * 6, [1] * 6, 2.0, 5)
    with pytest.raises(ValueError):
        lisi_frame(np.arange(6), grp, cats, codes[:5], il, cl, [5] * 6, [1] * 6, 2.0, 5)


def test_lisi_keys_and_rep_frame():
    from spvipes_amd.data import check_lisi_keys, lisi_rep_frame
    obs = {"batch": np.array(["b", "a", "b", "c"]), "cell_type": np.array([3, 3, 1, 1]), "short": np.array([1, 2])}
    keyed = check_lisi_keys(obs, ["batch", "cell_type"], 4)
    assert [key for key, _c, _k in keyed] == ["batch", "cell_type"] and keyed[0][1].tolist() == ["a", "b", "c"]
    assert keyed[0][2].tolist() == [1, 0, 1, 2] and keyed[0][2].dtype == np.int32 and keyed[1][2].tolist() == [1, 1, 0, 0]
    assert [key for key, _c, _k in check_lisi_keys(obs, "batch", 4)] == ["batch"]
    with pytest.raises(KeyError):
        check_lisi_keys(obs, ["batch", "nope"], 4)
    for bad in ([], ["batch", "batch"], [3], "short"):
        with pytest.raises(ValueError):
            check_lisi_keys(obs, bad, 4)
    f = lisi_rep_frame(list("wxyz"), keyed, np.array([[1.0, 2.0, np.nan, 3.0], [1.0, 1.0, 1.5, 2.0]]), [3, 3, 0, 3], [1, 1, 0, 1], 1.5, 3)
    assert list(f.columns) == ["lisi_batch", "lisi_cell_type", "n_neighbors", "converged"] and list(f.index) == list("wxyz")
    assert f.attrs["lisi_batch_median"] == 2.0 and f.attrs["lisi_cell_type_median"] == 1.25 and (f.attrs["n_batch"], f.attrs["n_cell_type"]) == (3, 2)
    assert (f.attrs["perplexity"], f.attrs["n_neighbors"], f.attrs["n_unconverged"]) == (1.5, 3, 1)
    with pytest.raises(ValueError):
        lisi_rep_frame(list("wxyz"), keyed, np.ones((3, 4)), [3] * 4, [1] * 4, 1.5, 3)


REFUSED = [dict(perplexity=86), dict(perplexity=0.5), dict(perplexity=float("nan")), dict(perplexity="30"), dict(latent="both"), dict(cells=2),
           dict(cells=True), dict(cells="all"), dict(latent="private"), dict(labels=np.zeros(3))]


@pytest.mark.parametrize("kw", REFUSED, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in REFUSED])
def test_latent_lisi_refuses_before_it_touches_the_model(kw):
    """560 cells selected on an object that is no model: a refusal that came after the first use of the model would be an AttributeError"""
    from spvipes_amd.model import spVIPES
    with pytest.raises(ValueError):
        spVIPES.latent_lisi(object(), [list(range(300)), list(range(300, 560))], **kw)


def test_latent_lisi_accepts_what_it_should_and_small_selections():
    from spvipes_amd.model import spVIPES
    gi = [list(range(300)), list(range(300, 560))]
    for kw in (dict(labels=None), dict(labels=None, perplexity=85.67), dict(labels=None, cells=1, latent="private", perplexity=1), dict(labels=np.zeros(560))):
        with pytest.raises(AttributeError):
            spVIPES.latent_lisi(object(), gi, **kw)
    with pytest.raises(ValueError, match="k must lie"):     # one cell: no neighbour
        spVIPES.latent_lisi(object(), [[0], []], labels=None)
    with pytest.raises(ValueError, match="no cells"):
        spVIPES.latent_lisi(object(), [[], []], labels=None)


def test_classmethod_lisi_refusals_need_no_device():
    from spvipes_amd.model import spVIPES

    class Duck:
        n_obs = 400
        obs = {"batch": np.arange(400) % 2}
        obsm = {"X_pca": np.zeros((400, 5)), "wide": np.zeros((400, 65)), "nan": np.full((400, 3), np.nan)}
    with pytest.raises(KeyError):
        spVIPES.lisi(Duck(), "X_umap", "batch")
    for rep, keys, perp, exc in (("wide", "batch", 30, ValueError), ("nan", "batch", 30, ValueError), (np.zeros((99, 5)), "batch", 30, ValueError),
                                 ("X_pca", "batch", 90, ValueError), ("X_pca", "batch", 0, ValueError), ("X_pca", [], 30, ValueError), ("X_pca", "nope", 30, KeyError)):
        with pytest.raises(exc):
            spVIPES.lisi(Duck(), rep, keys, perplexity=perp)


def test_signatures():
    import inspect
    from spvipes_amd.model import spVIPES
    p = inspect.signature(spVIPES.latent_lisi).parameters
    assert list(p) == ["self", "group_indices_list", "labels", "cells", "latent", "give_mean", "perplexity", "batch_size", "_noise"]
    assert (p["labels"].default, p["cells"].default, p["latent"].default, p["give_mean"].default, p["perplexity"].default, p["batch_size"].default) == (
        "cell_type", "both", "shared", True, 30, None)
    p = inspect.signature(spVIPES.lisi).parameters
    assert list(p) == ["adata", "use_rep", "keys", "perplexity", "device"] and (p["perplexity"].default, p["device"].default) == (30, None)
