"""GPU: ``spVIPES.rank_genes_groups`` -- the Wilcoxon rank-sum test on the observed counts -- on the duck AnnData, against
``scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic")`` gene by gene, for dense and sparse ``counts_storage``.

Tolerances (tests/test_rank_test_host_cpu.py derives them): the device delivers exact integers, so U and the z-score agree with
scipy's to rtol 1e-12 and the p-value to rtol 1e-9; the raw integer tables in ``attrs`` are compared for equality."""
import numpy as np
import pytest
import torch

from tests._rank_reference import keys_of, rank_tables

pytestmark = pytest.mark.gpu

TARGET = 1e4


@pytest.fixture(scope="module")
def models():
    """one untrained model per storage on the same data (rank_genes_groups needs no training)"""
    import scipy.sparse as sp

    from spvipes_amd import _abi
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _abi.load()
    out = {}
    for storage in ("dense", "sparse"):
        ad = make_duck(n=(300, 260), seed=2)
        dense_X = ad.X.copy()
        if storage == "sparse":
            ad.X = sp.csr_matrix(ad.X)
        ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
        spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
        torch.manual_seed(0)
        model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32", counts_storage=storage)
        out[storage] = (model, ad, dense_X)
    return out


def _gi(ad):
    return [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]


def _keys(X, cells, var_idx, sel, normalize):
    """the fp32 keys of the listed cells: count * fp32(target_sum / total over ALL of the group's genes) (weight 0 without counts), or the counts"""
    own = X[np.asarray(cells)][:, var_idx]
    if not normalize:
        return keys_of(own[:, sel].astype(np.float32))
    total = own.astype(np.float64).sum(1)
    w = np.where(total > 0, TARGET / np.where(total > 0, total, 1.0), 0.0).astype(np.float32)
    return keys_of(own[:, sel].astype(np.float32), w)


def _check_against_scipy(block, keys, own, tie_correct, ctx):
    from scipy.stats import mannwhitneyu

    rest = ~own
    n1, n2 = int(own.sum()), int(rest.sum())
    n = n1 + n2
    for j in range(keys.shape[1]):
        a, b = keys[own, j].astype(np.float64), keys[rest, j].astype(np.float64)
        res = mannwhitneyu(a, b, use_continuity=False, method="asymptotic", alternative="two-sided")
        assert block["u_statistic"].iloc[j] == pytest.approx(res.statistic, rel=1e-12, abs=0), f"{ctx}: U of gene {j}"
        assert block["auc"].iloc[j] == pytest.approx(res.statistic / (n1 * n2), rel=1e-12, abs=0), f"{ctx}: auc of gene {j}"
        t = np.unique(keys[:, j], return_counts=True)[1].astype(np.float64)
        var = n1 * n2 / 12.0 * ((n + 1) - ((t ** 3 - t).sum() / (n * (n - 1)) if tie_correct else 0.0))
        if var > 0:
            z = (res.statistic - n1 * n2 / 2.0) / np.sqrt(var)
            assert block["scores"].iloc[j] == pytest.approx(z, rel=1e-12, abs=0), f"{ctx}: score of gene {j}"
            if tie_correct:
                assert block["pvals"].iloc[j] == pytest.approx(res.pvalue, rel=1e-9, abs=0), f"{ctx}: p-value of gene {j}"
        else:
            assert block["scores"].iloc[j] == 0.0 and block["pvals"].iloc[j] == 1.0, f"{ctx}: all-tied gene {j}"


def _same(a, b, ctx):
    assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index), ctx
    for c in a.columns:
        x, y = a[c].to_numpy(), b[c].to_numpy()
        assert x.dtype == y.dtype, f"{ctx}: dtype of {c}"
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) if x.dtype == np.float64 else (x == y).all(), f"{ctx}: column {c} differs"


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("storage", ["dense", "sparse"])
def test_groupby_against_scipy_and_the_integer_tables(models, storage, g):
    model, ad, X = models[storage]
    gi = _gi(ad)
    cells, var_idx = np.asarray(gi[g]), np.asarray(ad.uns["groups_var_indices"][g])
    sel = np.arange(0, len(var_idx), 3)
    df = model.rank_genes_groups(gi, g, groupby="cell_type", gene_list=sel)
    labels = np.asarray(ad.obs["cell_type"])[cells]
    names, code = np.unique(labels, return_inverse=True)
    keys = _keys(X, cells, var_idx, sel, True)
    rank2, ties = rank_tables(keys, code, len(names))
    assert (df.attrs["rank2"] == rank2).all() and (df.attrs["ties"] == ties).all()
    assert df.attrs["n_cells"] == {nm: int((code == k).sum()) for k, nm in enumerate(names.tolist())}
    assert len(df) == len(names) * len(sel)
    for k, nm in enumerate(names.tolist()):
        block = df[df["group1"] == nm]
        assert len(block) == len(sel) and (block["comparison"] == f"{nm} vs Rest").all() and (block["group2"] == "Rest").all()
        _check_against_scipy(block, keys, code == k, True, f"{storage} group {g} label {nm}")
        p = block["pvals"].to_numpy()
        order = np.argsort(p, kind="stable")
        adj = np.minimum(np.minimum.accumulate((p[order] * len(p) / (1 + np.arange(len(p))))[::-1])[::-1], 1.0)
        np.testing.assert_allclose(block["pvals_adj"].to_numpy()[order], adj, rtol=1e-15, atol=0)


@pytest.mark.parametrize("normalize,tie_correct", [(True, True), (False, True), (False, False)])
def test_two_populations_against_scipy(models, normalize, tie_correct):
    model, ad, X = models["dense"]
    gi = _gi(ad)
    g = 1
    cells, var_idx = np.asarray(gi[g]), np.asarray(ad.uns["groups_var_indices"][g])
    rng = np.random.default_rng(5)
    idx1 = cells[rng.permutation(len(cells))[: len(cells) // 3]]
    rest = np.setdiff1d(cells, idx1)
    idx2 = rest[rng.permutation(len(rest))[: len(rest) // 2]]
    df = model.rank_genes_groups(gi, g, idx1=idx1, idx2=idx2, normalize=normalize, tie_correct=tie_correct)
    listed = np.concatenate([idx1, idx2])
    keys = _keys(X, listed, var_idx, np.arange(len(var_idx)), normalize)
    own = np.arange(len(listed)) < len(idx1)
    _check_against_scipy(df, keys, own, tie_correct, f"normalize {normalize} tie_correct {tie_correct}")
    rank2, ties = rank_tables(keys, (~own).astype(np.int64), 2)
    assert (df.attrs["rank2"] == rank2).all() and (df.attrs["ties"] == ties).all()
    assert df.attrs["n_cells"] == {"idx1": len(idx1), "idx2": len(idx2)}
    if not normalize:
        assert (ties > 0).all()   # raw counts: heavy ties in every gene
    # idx2=None: every other cell of the group
    df2 = model.rank_genes_groups(gi, g, idx1=idx1, normalize=normalize, tie_correct=tie_correct)
    listed = np.concatenate([idx1, rest])
    keys = _keys(X, listed, var_idx, np.arange(len(var_idx)), normalize)
    _check_against_scipy(df2, keys, np.arange(len(listed)) < len(idx1), tie_correct, "idx2=None")


@pytest.mark.parametrize("mode", ["groupby", "groupby-labels", "idx1"])
def test_rows_and_index_are_those_of_count_statistics(models, mode):
    import pandas as pd

    model, ad, _X = models["dense"]
    gi = _gi(ad)
    cells = np.asarray(gi[0])
    names = np.unique(np.asarray(ad.obs["cell_type"])[cells])
    sel = [f"gene{i}" for i in (7, 2, 2, 11)]
    kw = {"groupby": dict(groupby="cell_type"), "groupby-labels": dict(groupby="cell_type", labels=[names[-1], names[0]]), "idx1": dict(idx1=cells[5:60], idx2=cells[100:130])}[mode]
    ranks = model.rank_genes_groups(gi, 0, gene_list=sel, **kw)
    stats = model.count_statistics(gi, 0, gene_list=sel, **kw)
    assert list(ranks.index) == list(stats.index) and len(ranks) == len(stats)
    if mode != "idx1":
        for c in ("comparison", "group1", "group2"):
            assert (ranks[c].to_numpy() == stats[c].to_numpy()).all()
        if mode == "groupby-labels":
            assert list(pd.unique(ranks["group1"])) == [names[0], names[-1]]
    both = pd.concat([stats, ranks[["scores", "pvals_adj"]]], axis=1)
    assert len(both) == len(stats)
    assert (ranks["scores"].to_numpy()[1] == ranks["scores"].to_numpy()[2])   # the repeated gene


def test_labels_restriction_keeps_the_blocks_of_the_full_frame(models):
    model, ad, _X = models["dense"]
    gi = _gi(ad)
    names = np.unique(np.asarray(ad.obs["cell_type"])[np.asarray(gi[0])])
    full = model.rank_genes_groups(gi, 0, groupby="cell_type")
    part = model.rank_genes_groups(gi, 0, groupby="cell_type", labels=[names[1]])
    _same(part, full[full["group1"] == names[1]], "labels restriction")
    with pytest.raises(KeyError, match="not among the labels"):
        model.rank_genes_groups(gi, 0, groupby="cell_type", labels=["nope"])


@pytest.mark.parametrize("normalize", [True, False])
def test_dense_and_sparse_storage_give_the_same_frame_bit_for_bit(models, normalize):
    frames = {}
    for storage in ("dense", "sparse"):
        model, ad, _X = models[storage]
        frames[storage] = model.rank_genes_groups(_gi(ad), 0, groupby="cell_type", normalize=normalize)
        again = model.rank_genes_groups(_gi(ad), 0, groupby="cell_type", normalize=normalize)
        _same(frames[storage], again, f"{storage}: two calls")
    _same(frames["dense"], frames["sparse"], "dense against sparse")
    assert (frames["dense"].attrs["rank2"] == frames["sparse"].attrs["rank2"]).all()


def test_it_works_on_an_untrained_model(models):
    model, ad, _X = models["dense"]
    assert not getattr(model, "is_trained_", False)
    df = model.rank_genes_groups(_gi(ad), 1, groupby="cell_type")
    assert np.isfinite(df["scores"].to_numpy()).all() and ((df["pvals"] >= 0) & (df["pvals"] <= 1)).all()
