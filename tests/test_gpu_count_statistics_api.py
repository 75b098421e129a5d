"""GPU: ``spVIPES.count_statistics`` -- the raw-count columns next to the differential-expression tables -- against numpy on
``adata.X``, for dense and sparse ``counts_storage`` and both groups of the duck AnnData.

Bounds.  raw_mean and non_zeros_proportion are ONE fp64 division of two exactly carried integers: numpy's division of the same
integers gives the same bits; the tests allow 1 ulp.  raw_normalized_mean is S2 / n_k with S2 a sum of n_k non-negative fp64 terms
count * (target_sum / total), each rounded once after the correctly rounded weight: within n_k * 2^-52 * S2 of math.fsum of the same
terms (tests/test_gpu_count_stats.py derives it), so the mean is within that bound divided by n_k."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COLS = ("raw_mean1", "raw_mean2", "non_zeros_proportion1", "non_zeros_proportion2", "raw_normalized_mean1", "raw_normalized_mean2")
TARGET = 1e4


@pytest.fixture(scope="module")
def models():
    """one untrained model per storage on the same data (count_statistics needs no training)"""
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


def _oracle(X, cells, var_idx, sel):
    """(mean, proportion, normalised mean, S2, n) of the cells ``cells`` (adata rows) over the genes var_idx[sel], in float64"""
    own = X[np.asarray(cells)][:, var_idx].astype(np.float64)
    total = own.sum(1)   # integers below 2^53: exact
    w = np.where(total > 0, TARGET / np.where(total > 0, total, 1.0), 0.0)
    sub = own[:, sel]
    n = len(cells)
    s2 = np.array([math.fsum((sub[:, j] * w).tolist()) for j in range(sub.shape[1])])
    return sub.sum(0) / n, (sub != 0).sum(0) / n, s2 / n, s2, n


def _check_side(df, side, X, cells, var_idx, sel, ctx):
    mean, prop, norm, s2, n = _oracle(X, cells, var_idx, sel)
    for col, ref in ((f"raw_mean{side}", mean), (f"non_zeros_proportion{side}", prop)):
        got = df[col].to_numpy()
        assert got.dtype == np.float64
        assert (np.abs(got - ref) <= np.spacing(ref)).all(), f"{ctx}: {col}"
    got = df[f"raw_normalized_mean{side}"].to_numpy()
    err, bound = np.abs(got - norm), n * 2.0**-52 * s2 / n
    print(f"{ctx} raw_normalized_mean{side}: max err {err.max():.3e}, bound min {bound[bound > 0].min() if (bound > 0).any() else 0:.3e}")
    assert (err <= bound).all(), f"{ctx}: raw_normalized_mean{side}"


def _same(a, b, ctx):
    assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index), ctx
    for c in a.columns:
        x, y = a[c].to_numpy(), b[c].to_numpy()
        assert x.dtype == y.dtype, f"{ctx}: dtype of {c}"
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) if x.dtype == np.float64 else (x == y).all(), f"{ctx}: column {c} differs"


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("storage", ["dense", "sparse"])
def test_two_populations_against_numpy(models, storage, g):
    model, ad, X = models[storage]
    gi = _gi(ad)
    cells, var_idx = np.asarray(gi[g]), np.asarray(ad.uns["groups_var_indices"][g])
    G = len(var_idx)
    rng = np.random.default_rng(5 + g)
    idx1 = cells[rng.permutation(len(cells))[: len(cells) // 3]]
    rest = np.setdiff1d(cells, idx1)
    idx2 = rest[rng.permutation(len(rest))[: len(rest) // 2]]
    ctx = f"[{storage} group {g}]"
    # all genes, explicit idx2
    df = model.count_statistics(gi, g, idx1=idx1, idx2=idx2)
    assert tuple(df.columns) == COLS and len(df) == G and all(df[c].dtype == np.float64 for c in COLS)
    assert list(df.index) == [f"gene{i}" for i in var_idx]
    _check_side(df, 1, X, idx1, var_idx, np.arange(G), ctx)
    _check_side(df, 2, X, idx2, var_idx, np.arange(G), ctx)
    # idx2 = None is every other cell of the group; a gene list by name, shuffled, with a repeat
    names = [f"gene{var_idx[j]}" for j in (5, 0, G - 1, 5, 17, 33)]
    sel = np.array([5, 0, G - 1, 5, 17, 33])
    sub = model.count_statistics(gi, g, idx1=idx1, gene_list=names, target_sum=TARGET)
    assert list(sub.index) == names
    _check_side(sub, 1, X, idx1, var_idx, sel, ctx + " names")
    _check_side(sub, 2, X, rest, var_idx, sel, ctx + " names")
    # a selected column equals the same column of the all-genes frame bit for bit
    everything = model.count_statistics(gi, g, idx1=idx1)
    for c in COLS:
        assert np.array_equal(sub[c].to_numpy().view(np.uint8), everything[c].to_numpy()[sel].view(np.uint8)), f"{ctx}: {c} under a selection"
    # the frame lines up with differential_expression's
    de = model.differential_expression(gi, g, idx1, gene_list=names, use_mean=True, n_pairs=64, batch_size=64)
    assert list(de.index) == list(sub.index)
    de_all = model.differential_expression(gi, g, idx1, idx2, use_mean=True, n_pairs=64, batch_size=64)
    assert list(de_all.index) == list(df.index)


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("storage", ["dense", "sparse"])
def test_groupby_blocks_against_numpy_and_the_two_population_call(models, storage, g):
    import pandas as pd

    model, ad, X = models[storage]
    gi = _gi(ad)
    cells, var_idx = np.asarray(gi[g]), np.asarray(ad.uns["groups_var_indices"][g])
    G = len(var_idx)
    lab = np.asarray(ad.obs["cell_type"])[cells]
    names = np.unique(lab)
    sel = np.array([3, G - 1, 0, 3])
    ctx = f"[{storage} group {g}]"
    for labels in (None, [names[2], names[0]]):
        by = model.count_statistics(gi, g, groupby="cell_type", labels=labels, gene_list=sel)
        compared = list(names) if labels is None else sorted(labels)
        assert tuple(by.columns) == COLS + ("comparison", "group1", "group2") and len(by) == len(compared) * len(sel)
        de = model.differential_expression_by(gi, g, "cell_type", labels=labels, gene_list=sel, use_mean=True, n_pairs=64, batch_size=64, lfc_median=False)
        assert list(de.index) == list(by.index)
        for c in ("comparison", "group1", "group2"):
            assert (de[c].to_numpy() == by[c].to_numpy()).all(), f"{ctx}: {c}"
        both = pd.concat([de, by[list(COLS)]], axis=1)   # the documented use
        assert len(both) == len(de) and both.shape[1] == de.shape[1] + 6
        for i, name in enumerate(compared):
            block = by.iloc[i * len(sel):(i + 1) * len(sel)]
            assert (block["group1"] == name).all() and (block["group2"] == "Rest").all() and (block["comparison"] == f"{name} vs Rest").all()
            own, other = cells[lab == name], cells[lab != name]
            _check_side(block, 1, X, own, var_idx, sel, f"{ctx} label {name}")
            _check_side(block, 2, X, other, var_idx, sel, f"{ctx} label {name}")
            two = model.count_statistics(gi, g, idx1=own, gene_list=sel)
            for c in COLS[:4]:   # one division of the same exact integers: the same bits
                assert np.array_equal(block[c].to_numpy().view(np.uint8), two[c].to_numpy().view(np.uint8)), f"{ctx} label {name}: {c}"
            # side 1 is reduced in the same order by both calls; side 2 is a sum of label sums here and one list there: both within the bound
            assert np.array_equal(block["raw_normalized_mean1"].to_numpy().view(np.uint8), two["raw_normalized_mean1"].to_numpy().view(np.uint8))
            _, _, _, s2, n2 = _oracle(X, other, var_idx, sel)
            assert (np.abs(block["raw_normalized_mean2"].to_numpy() - two["raw_normalized_mean2"].to_numpy()) <= 2 * n2 * 2.0**-52 * s2 / n2).all()


@pytest.mark.parametrize("g", [0, 1])
def test_dense_and_sparse_models_give_the_same_frames_bit_for_bit(models, g):
    (md, ad, _), (ms, as_, _) = models["dense"], models["sparse"]
    gi = _gi(ad)
    cells = np.asarray(gi[g])
    idx1 = cells[::3]
    _same(md.count_statistics(gi, g, idx1=idx1), ms.count_statistics(_gi(as_), g, idx1=idx1), f"two populations, group {g}")
    _same(md.count_statistics(gi, g, groupby="cell_type", gene_list=[4, 1]), ms.count_statistics(_gi(as_), g, groupby="cell_type", gene_list=[4, 1]),
          f"groupby, group {g}")


def test_a_cell_without_counts_gets_the_weight_zero(models):
    """the stated deviation from scvi-tools, which would divide by zero: such a cell adds nothing to the normalised mean"""
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    ad = make_duck(n=(300, 260), seed=2)
    ad.X[7, :] = 0.0
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32", counts_storage="dense")
    gi = _gi(ad)
    df = model.count_statistics(gi, 0, idx1=[7, 8, 9])
    assert np.isfinite(df.to_numpy()).all()
    _check_side(df, 1, ad.X, [7, 8, 9], np.asarray(ad.uns["groups_var_indices"][0]), np.arange(96), "[empty cell]")
