"""GPU: ``spVIPES.count_spearman_matrix`` and ``spVIPES.get_feature_spearman_matrix`` on the duck AnnData.

The device delivers exact integers (tests/test_gpu_rank_transform.py), so ``attrs["sums"]["C"]`` is compared for EQUALITY with the int64
reference (tests/_spearman_reference.py) built from the very values that are ranked -- the host keys of ``rank_genes_groups`` for the
counts, the fp32 matrix ``get_normalized_expression`` returns for the same arguments for the decoded expression -- ``S`` must be exactly
0, and the frame must equal ``data.spearman_table`` of that C bit for bit.
rho is also held to ``scipy.stats.spearmanr`` on the same values within 32 * 2^-53 absolute: both sides are a handful of correctly rounded
operations on exactly represented integers at these sizes (the worst case measured on the host at n = 2 .. 8200 was 2 * 2^-53,
tests/test_spearman_host_cpu.py); NaN must occur in the same places."""
import warnings

import numpy as np
import pytest
import torch

from tests._rank_reference import keys_of
from tests._spearman_reference import spearman_tables
from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

TARGET = 1e4
BS = 40
TOL = 32 * 2.0 ** -53
POS = [np.array([5, 0, 95, 17, 40, 41, 42, 63, 64, 65, 1, 2]), np.array([79, 3, 0, 10, 20])]


def _gi(ad):
    return [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]


def _hold(frame, values, names, n_cells, n_samples=1):
    """the frame and its attrs against the fp32 values [rows, p] that were ranked"""
    from scipy.stats import spearmanr

    from spvipes_amd.data import spearman_table
    values = np.ascontiguousarray(values, dtype=np.float32)
    n, p = values.shape
    _c, Cm, T = spearman_tables(values)
    sums = frame.attrs["sums"]
    assert sums["S"].dtype == np.float64 and sums["S"].shape == (p,) and (sums["S"] == 0.0).all()
    assert sums["C"].dtype == np.float64 and sums["C"].shape == (p, p) and (sums["C"] == Cm.astype(np.float64)).all() and (sums["C"].astype(np.int64) == Cm).all()
    assert frame.attrs["ties"].dtype == np.int64 and (frame.attrs["ties"] == T).all()
    assert frame.attrs["n_cells"] == n_cells and frame.attrs["n_samples"] == n_samples and n == n_cells * n_samples and frame.attrs["exact"] is True
    assert frame.index.tolist() == list(names) and frame.columns.tolist() == list(names)
    got = frame.to_numpy()
    want = spearman_table(Cm.astype(np.float64), n)
    assert got.dtype == np.float64 and np.array_equal(got, want["corr"], equal_nan=True) and (want["tie_term"] == T).all()
    assert np.array_equal(got, got.T, equal_nan=True)
    # scipy gives NaN for every pair with a constant column -- but for a matrix whose FIRST or SECOND column is constant it returns one
    # scalar NaN instead of the matrix, so the constant columns are set to NaN here and scipy sees the others
    rho = np.full((p, p), np.nan)
    varying = np.nonzero((values != values[0]).any(0))[0]
    if len(varying) == 1:
        rho[varying[0], varying[0]] = 1.0
    elif len(varying) > 1:
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # (no constant column is left: scipy must not warn)
            r = np.asarray(spearmanr(values[:, varying].astype(np.float64)).statistic)
        rho[np.ix_(varying, varying)] = r if r.ndim == 2 else np.array([[1.0, float(r)], [float(r), 1.0]])
    assert np.array_equal(np.isnan(got), np.isnan(rho))
    live = ~np.isnan(rho)
    worst = float(np.abs(got[live] - rho[live]).max()) if live.any() else 0.0
    print(f"spearman: n {n} p {p}: worst |rho - scipy| = {worst / 2.0 ** -53:.2f} x 2^-53, NaN entries {int((~live).sum())}")
    assert worst <= TOL
    assert (np.diagonal(got)[np.diagonal(live)] == 1.0).all()


@pytest.fixture(scope="module")
def count_models():
    """one untrained model per storage on the same data (count_spearman_matrix needs no training)"""
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
        out[storage] = (spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32", counts_storage=storage), ad, dense_X)
    return out


def _count_keys(X, cells, var_idx, sel, normalize):
    """the fp32 keys of the listed cells: count * fp32(target_sum / total over ALL of the group's genes) (weight 0 without counts), or the counts"""
    own = X[np.asarray(cells)][:, var_idx]
    if not normalize:
        return keys_of(own[:, sel].astype(np.float32))
    total = own.astype(np.float64).sum(1)
    w = np.where(total > 0, TARGET / np.where(total > 0, total, 1.0), 0.0).astype(np.float32)
    return keys_of(own[:, sel].astype(np.float32), w)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("g", [0, 1])
def test_count_spearman_matrix_dense_and_sparse(count_models, g, normalize):
    frames = {}
    for storage in ("dense", "sparse"):
        model, ad, X = count_models[storage]
        gi = _gi(ad)
        cells, var_idx = np.asarray(gi[g]), np.asarray(ad.uns["groups_var_indices"][g])
        sel = np.arange(len(var_idx))
        df = model.count_spearman_matrix(gi, g, normalize=normalize)
        _hold(df, _count_keys(X, cells, var_idx, sel, normalize), [f"gene{c}" for c in var_idx], len(cells))
        frames[storage] = df
    a, b = frames["dense"], frames["sparse"]
    assert np.array_equal(a.to_numpy().view(np.uint8), b.to_numpy().view(np.uint8)) and all(np.array_equal(a.attrs["sums"][k], b.attrs["sums"][k]) for k in "SC")
    assert (a.attrs["ties"] == b.attrs["ties"]).all()


def test_count_spearman_matrix_gene_list_cells_and_the_ties_of_rank_genes_groups(count_models):
    model, ad, X = count_models["sparse"]
    gi = _gi(ad)
    g = 0
    cells, var_idx = np.asarray(gi[g]), np.asarray(ad.uns["groups_var_indices"][g])
    sel = np.array([7, 2, 2, 11, 40, 0])
    names = [f"gene{var_idx[s]}" for s in sel]
    keep = np.random.default_rng(3).permutation(len(cells))[:101]
    df = model.count_spearman_matrix(gi, g, gene_list=names, cells=cells[keep])
    _hold(df, _count_keys(X, cells[np.sort(keep)], var_idx, sel, True), names, len(keep))   # the rows are ranked in the group's order
    assert df.iloc[1, 2] == 1.0   # the repeated gene
    # a constant gene: only cells without a count of the gene that is zero most often -- NaN in its row and column, as scipy gives
    own = X[cells][:, var_idx]
    j = int(np.argmax((own == 0).sum(0)))
    zero_cells = np.nonzero(own[:, j] == 0)[0]
    assert len(zero_cells) >= 10
    const = model.count_spearman_matrix(gi, g, gene_list=[j, 7, 2], cells=cells[zero_cells])
    _hold(const, _count_keys(X, cells[zero_cells], var_idx, np.array([j, 7, 2]), True), [f"gene{var_idx[s]}" for s in (j, 7, 2)], len(zero_cells))
    assert np.isnan(const.to_numpy()[0]).all() and const.attrs["ties"][0] == len(zero_cells) ** 3 - len(zero_cells)
    whole = model.count_spearman_matrix(gi, g, gene_list=sel)
    ranks = model.rank_genes_groups(gi, g, groupby="cell_type", gene_list=sel)
    assert (whole.attrs["ties"] == ranks.attrs["ties"]).all()
    again = model.count_spearman_matrix(gi, g, gene_list=sel)
    assert again.equals(whole) and np.array_equal(again.attrs["sums"]["C"], whole.attrs["sums"]["C"])
    with pytest.raises(ValueError, match="cells: cell .* is not in group_indices_list\\[0\\]"):
        model.count_spearman_matrix(gi, 0, cells=[gi[1][0]])
    with pytest.raises(KeyError, match="no_such_gene"):
        model.count_spearman_matrix(gi, 0, gene_list=["no_such_gene"])


def test_get_feature_spearman_matrix():
    from spvipes_amd import _abi
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    assert torch.cuda.is_available(), "these tests need the MI355X"
    _abi.load()
    dev = torch.device("cuda:0")
    ad = make_duck(n=(150, 110), seed=2)   # n0 != n1, ragged last batches
    ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32")
    gi = _gi(ad)
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    cols = [np.asarray(ad.uns["groups_var_indices"][g])[POS[g]] for g in range(2)]
    E = {c: model.get_normalized_expression(gi, gene_list=POS, component=c, use_mean=True, batch_size=BS) for c in ("mixture", "shared")}
    model.module.train()   # the call must put the module into eval mode and restore this
    for g in range(2):
        names = [f"gene{c}" for c in cols[g]]
        df = model.get_feature_spearman_matrix(gi, g, gene_list=POS[g], batch_size=BS)
        assert model.module.training   # the training flag is restored
        _hold(df, E["mixture"][g], names, len(gi[g]))
        by_name = model.get_feature_spearman_matrix(gi, g, gene_list=names, batch_size=BS)   # the same selection, by name; two calls agree in bits
        assert by_name.equals(df) and np.array_equal(by_name.attrs["sums"]["C"], df.attrs["sums"]["C"])
        _hold(model.get_feature_spearman_matrix(gi, g, gene_list=POS[g], component="shared", batch_size=BS), E["shared"][g], names, len(gi[g]))
        # a subset of the cells, in an order of its own: the matrix's rows of those cells; all cells are still walked
        keep = np.random.default_rng(g).permutation(len(gi[g]))[: len(gi[g]) // 3]
        sub = model.get_feature_spearman_matrix(gi, g, gene_list=POS[g], cells=np.asarray(gi[g])[keep], batch_size=BS)
        _hold(sub, E["mixture"][g][np.sort(keep)], names, len(keep))
    with pytest.raises(ValueError, match="cells: cell .* is not in group_indices_list\\[0\\]"):
        model.get_feature_spearman_matrix(gi, 0, cells=[gi[1][0]])
    assert model.module.training
    model.module.eval()

    # all of group 1's genes (80: a second store tile)
    full = model.get_feature_spearman_matrix(gi, 1, batch_size=BS)
    _hold(full, model.get_normalized_expression(gi, batch_size=BS)[1], [f"gene{c}" for c in ad.uns["groups_var_indices"][1]], len(gi[1]))

    # sampled latents, n_samples = 2: row sample * n_cells + position holds draw 2 * step + sample of the cell
    g, nf = 0, _noise_fn(dev)
    both = model.get_feature_spearman_matrix(gi, g, gene_list=POS[g], n_samples=2, use_mean=False, batch_size=BS, _noise=nf)
    X2 = np.concatenate([model.get_normalized_expression(gi, gene_list=POS, n_samples=1, use_mean=False, batch_size=BS,
                                                         _noise=lambda d, b0, b1, s=s: nf(2 * d + s, b0, b1))[g] for s in (0, 1)])
    _hold(both, X2, [f"gene{c}" for c in cols[g]], len(gi[g]), n_samples=2)
    with pytest.raises(ValueError, match="use_mean"):
        model.get_feature_spearman_matrix(gi, g, n_samples=2)
