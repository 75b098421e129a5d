"""GPU: spVIPES.get_feature_correlation_matrix on the duck AnnData -- label PoE in fp32, paired PoE in bf16 with its cycling walk, unequal
group sizes, a batch size (40) that is no multiple of the kernel's 32-row chunk and smaller than either group, at most 24 genes.

The yardstick is ``get_normalized_expression`` of the same model with the same arguments: the method sums those very fp32 values, so
everything is held to reductions of that matrix X [n, p] in numpy's 80-bit long double.

Sums.  One spv_gram_f64 call keeps every element within gamma_m (|start| + sum |x_i x_j|), m = n_use + slabs + 1 (tests/test_gpu_gram.py).
A walk is K such calls onto the same tables, one slab each here (40 rows), so an element sees sum_k (n_use_k + 2) = n + 2 K roundings; every
call counts at least one row (steps without one are skipped), so K <= n and m = 3 n bounds every walk: gamma_3n sum |x_i x_j| for C,
gamma_3n sum |x_i| for S.

The frame is compared with the two-pass long-double Pearson r of X.  With e_ij = (gamma_m sum |x_i x_j| + 3 u |S_i S_j| / n) / (n - 1), the
error the one-pass covariance (C_ij - S_i S_j / n) / (n - 1) can carry (the table's, plus three roundings of the formula on a term of size
|S_i S_j| / n), a first-order expansion of r = c_ij / sqrt(v_i v_j) gives

    |dr_ij| <= 2 [ e_ij / sqrt(v_i v_j) + |r_ij| (e_ii / v_i + e_jj / v_j) / 2 ]

the factor 2 covering the second-order terms while e_ii / v_i < 0.01, which is ASSERTED on the reference for every selected gene before any
device value is looked at.  Every test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

BS = 40
LD = np.longdouble
U = 2.0 ** -53
POS = [np.array([5, 0, 95, 17, 40, 41, 42, 63, 64, 65, 1, 2]), np.array([79, 3, 0, 10, 20])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _gamma(m):
    return m * U / (1.0 - m * U)


def _adata(config):
    from tests._duck import make_duck
    paired = config.startswith("paired")
    ad = make_duck(n=(96, 70) if paired else (150, 110), seed=2, with_plan=paired)   # n0 != n1, ragged last batches
    ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
    return ad


def _reference(X):
    """long double, from the matrix X [n, p]: (S, C, sum |x|, sum |x_i x_j|, two-pass variances, two-pass Pearson r)"""
    x = X.astype(LD)
    n = x.shape[0]
    xc = x - x.mean(0)
    cov = xc.T @ xc / (n - 1)
    v = np.diagonal(cov).copy()
    return x.sum(0), x.T @ x, np.abs(x).sum(0), np.abs(x).T @ np.abs(x), v, cov / np.sqrt(np.outer(v, v))


def _hold(frame, X, n_samples=1):
    """the frame and its attrs against the values X [n, p] (float32) it must have reduced"""
    n, p = X.shape
    S, Cm, A, AA, v, r = _reference(X)
    gam = _gamma(3 * n)
    e = (gam * AA + 3 * U * np.abs(np.outer(S, S)) / n) / (n - 1)
    rel = np.diagonal(e) / v
    assert (v > 0).all() and (rel < 0.01).all(), f"the selection does not satisfy e_ii / v_i < 0.01: {rel.max()}"   # the reference first
    sums = frame.attrs["sums"]
    assert sums["S"].dtype == np.float64 and sums["S"].shape == (p,) and sums["C"].dtype == np.float64 and sums["C"].shape == (p, p)
    assert (np.abs(sums["S"].astype(LD) - S) <= gam * A).all()
    assert (np.abs(sums["C"].astype(LD) - Cm) <= gam * AA).all()
    assert np.array_equal(sums["C"], sums["C"].T)
    bound = 2 * (e / np.sqrt(np.outer(v, v)) + np.abs(r) * (rel[:, None] + rel[None, :]) / 2)
    got = frame.to_numpy()
    assert got.shape == (p, p) and got.dtype == np.float64
    worst = float(np.max(np.abs(got.astype(LD) - r) / bound))
    print(f"correlation: n {n} p {p}: worst |dr| / bound = {worst:.3e}, worst |dr| = {float(np.max(np.abs(got.astype(LD) - r))):.3e}")
    assert worst <= 1.0
    assert (np.diagonal(got) == 1.0).all() and np.array_equal(got, got.T) and (np.abs(got) <= 1.0).all()
    assert frame.attrs["n_cells"] * n_samples == n and frame.attrs["n_samples"] == n_samples
    np.testing.assert_array_equal(frame.attrs["mean"], sums["S"] / n)
    assert (np.abs(frame.attrs["var"].astype(LD) - v) <= np.diagonal(e)).all()


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16"])
def test_get_feature_correlation_matrix(dev, tmp_path, config):
    from spvipes_amd.model import spVIPES
    paired = config.startswith("paired")
    ad = _adata(config)
    spVIPES.setup_anndata(ad, groups_key="groups", **({"transport_plan_key": "plan"} if paired else {"label_key": "cell_type"}))
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=config.split("-")[1])
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    cols = [np.asarray(ad.uns["groups_var_indices"][g])[POS[g]] for g in range(2)]
    E = {c: model.get_normalized_expression(gi, gene_list=POS, component=c, use_mean=True, batch_size=BS) for c in ("mixture", "private", "shared")}
    model.module.train()   # the call must put the module into eval mode and restore this
    for g in range(2):
        names = [f"gene{c}" for c in cols[g]]
        df = model.get_feature_correlation_matrix(gi, g, gene_list=POS[g], batch_size=BS)
        assert model.module.training   # the training flag is restored
        assert df.index.tolist() == names and df.columns.tolist() == names
        _hold(df, E["mixture"][g])
        by_name = model.get_feature_correlation_matrix(gi, g, gene_list=names, batch_size=BS)   # the same selection, by name
        assert by_name.equals(df) and by_name.index.tolist() == names
        for comp in ("private", "shared"):
            _hold(model.get_feature_correlation_matrix(gi, g, gene_list=POS[g], component=comp, batch_size=BS), E[comp][g])
        # a subset of the cells, in an order of its own: the matrix's rows of those cells; all cells are still walked
        rng = np.random.default_rng(g)
        keep = rng.permutation(len(gi[g]))[: len(gi[g]) // 3]
        sub = model.get_feature_correlation_matrix(gi, g, gene_list=POS[g], cells=np.asarray(gi[g])[keep], batch_size=BS)
        assert sub.attrs["n_cells"] == len(keep)
        _hold(sub, E["mixture"][g][np.sort(keep)])
    with pytest.raises(ValueError, match="cells: cell .* is not in group_indices_list\\[0\\]"):
        model.get_feature_correlation_matrix(gi, 0, cells=[gi[1][0]])
    with pytest.raises(KeyError, match="no_such_gene"):
        model.get_feature_correlation_matrix(gi, 0, gene_list=["no_such_gene"])
    assert model.module.training
    model.module.eval()

    # two calls agree bit for bit (all of group 1's genes)
    a = model.get_feature_correlation_matrix(gi, 1, batch_size=BS)
    b = model.get_feature_correlation_matrix(gi, 1, batch_size=BS)
    assert a.shape == (80, 80) and a.equals(b) and all(np.array_equal(a.attrs["sums"][k], b.attrs["sums"][k]) for k in "SC")

    # sampled latents, n_samples = 2: both draws of a step add their block -- the sums of the two single-draw tables whose draw d is the
    # double-draw walk's draw 2 d + s.  All values are positive, so sum |x_i x_j| is the exact C itself and each of the three tables lies
    # within gamma_{3 * 2n} of its exact value: the difference within 2 gamma_{6n + 1} (C_a + C_b), the + 1 for C_exact <= (1 + gamma) C.
    g, nf = 0, _noise_fn(dev)
    n = len(gi[g])
    both = model.get_feature_correlation_matrix(gi, g, gene_list=POS[g], n_samples=2, use_mean=False, batch_size=BS, _noise=nf)
    single = [model.get_feature_correlation_matrix(gi, g, gene_list=POS[g], n_samples=1, use_mean=False, batch_size=BS,
                                                   _noise=lambda d, b0, b1, s=s: nf(2 * d + s, b0, b1)) for s in (0, 1)]
    assert both.attrs["n_samples"] == 2 and both.attrs["n_cells"] == n and single[0].attrs["n_samples"] == 1
    assert not np.array_equal(single[0].attrs["sums"]["C"], single[1].attrs["sums"]["C"])
    for k in "SC":
        s2, s1 = both.attrs["sums"][k].astype(LD), single[0].attrs["sums"][k].astype(LD) + single[1].attrs["sums"][k].astype(LD)
        assert (s1 > 0).all() and (np.abs(s2 - s1) <= 2 * _gamma(6 * n + 1) * s1).all()
    X2 = np.concatenate([model.get_normalized_expression(gi, gene_list=POS, n_samples=1, use_mean=False, batch_size=BS,
                                                         _noise=lambda d, b0, b1, s=s: nf(2 * d + s, b0, b1))[g] for s in (0, 1)])
    _hold(both, X2, n_samples=2)
    with pytest.raises(ValueError, match="use_mean"):
        model.get_feature_correlation_matrix(gi, g, n_samples=2)

    # a model restored by save / load returns the same frame
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=_adata(config))
    want = model.get_feature_correlation_matrix(gi, 0, gene_list=POS[0], batch_size=BS)
    got = back.get_feature_correlation_matrix(gi, 0, gene_list=POS[0], batch_size=BS)
    assert not back.module.training
    assert got.equals(want) and all(np.array_equal(got.attrs["sums"][k], want.attrs["sums"][k]) for k in "SC")
