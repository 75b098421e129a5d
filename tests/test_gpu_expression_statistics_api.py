"""GPU: spVIPES.expression_statistics on the duck AnnData -- label PoE in fp32 (dense and CSR input), paired PoE in bf16 with its cycling
walk, unequal group sizes, a batch size that is no multiple of 32 and smaller than either group.

The yardstick is ``get_normalized_expression`` of the same model with the same ``batch_size`` and ``use_mean=True``: its four
``component`` matrices, reduced per population on the host in numpy's 80-bit long double.  The kernel sums those very fp32 values, so

  * a sum of n values (``attrs["sums"]``) lies within gamma_{n-1} * sum|v| of the exact one, gamma_m = m u / (1 - m u), u = 2^-53, whatever
    the order of addition (tests/test_gpu_expression_stats.py states the bound); a mean is held to that bound divided by n, on
    ``attrs["sums"] / n``, and the ``mean`` columns must EQUAL that one fp64 division;
  * a variance is held within 4 gamma_n * sum v^2 / (n - 1): (Q - S^2 / n) / (n - 1) inherits gamma_{n-1} Q from Q and, because
    S^2 / n <= Q (Cauchy-Schwarz), 2 gamma_{n-1} Q from S^2 / n, plus three roundings of the formula itself.
Every test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

BS = 40   # not a multiple of 32, smaller than either group
LD = np.longdouble
COMPONENTS = ("mixture", "private", "shared", "mixing")
MEANS, VARS = ("mean", "mean_private", "mean_shared", "mixing"), ("var", "var_private", "var_shared", "var_mixing")
COLUMNS = ["population", "gene", "n_cells", "n_samples", "mean", "mean_private", "mean_shared", "mixing", "private_fraction",
           "var", "var_private", "var_shared", "var_mixing"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _gamma(m):
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


def _adata(config):
    from tests._duck import make_duck
    paired = config.startswith("paired")
    ad = make_duck(n=(96, 70) if paired else (150, 110), seed=2, with_plan=paired)   # n0 != n1, ragged last batches
    ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
    if config.endswith("csr"):
        import scipy.sparse as sp
        ad.X = sp.csr_matrix(ad.X)
    return ad


def _dense(ad):
    return np.asarray(ad.X.todense()) if hasattr(ad.X, "todense") else np.asarray(ad.X)


def _hold_block(blk, sums, V, n_samples=1):
    """one population's rows of the frame and of ``attrs["sums"]`` against the values V: float32 [4, n values, n_sel]"""
    n = V.shape[1]
    x = V.astype(LD)
    S, A, Q = x.sum(1), np.abs(x).sum(1), (x * x).sum(1)
    assert (np.abs(sums[:4].astype(LD) - S) <= _gamma(n - 1) * A).all()
    assert (np.abs(sums[4:].astype(LD) - Q) <= _gamma(n - 1) * Q).all()
    for w in range(4):
        assert (np.abs(sums[w].astype(LD) / n - S[w] / n) <= _gamma(n - 1) * A[w] / n).all()    # the mean, within the bound / n
        np.testing.assert_array_equal(blk[MEANS[w]].to_numpy(), sums[w] / n)                      # ... and the column is that division
        got = blk[VARS[w]].to_numpy()
        if n < 2:
            assert np.isnan(got).all()
            continue
        mu = S[w] / n
        want = ((x[w] - mu) ** 2).sum(0) / (n - 1)
        assert (np.abs(got.astype(LD) - want) <= 4 * _gamma(n) * Q[w] / (n - 1)).all() and (got >= 0).all()
    pf = blk["private_fraction"].to_numpy()
    np.testing.assert_array_equal(pf, sums[1] / sums[0])
    assert ((pf >= 0) & (pf <= 1)).all()   # (0 <= private part <= mixture mean, value by value)
    assert (blk["n_cells"] * n_samples == n).all() and (blk["n_samples"] == n_samples).all()


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16", "label-fp32-csr"])
def test_expression_statistics(dev, tmp_path, config):
    """``library_size="observed"``, what is derivable.  A cell decoded at the library log T (T its observed total over all genes) has
    rate_k[j] = exp(log T - lse_k + y_k[j]) per component k, the values of library size 1 scaled by T; the kernel forms
    a_k = fl(fl(log T) - lse_k) and exp(fl(y + a_k)) in fp32.  With |log T|, |lse|, |y + a| < 32 each of the three roundings moves the
    exponent by at most 2^-20 (half an ulp below 32 is 2^-20), and the two exp evaluations (1 ulp each) and the product with T add
    3 * 2^-23: the value lies within 3 * 2^-20 + 3 * 2^-23 < 3.3e-6 relative of T * (value at library size 1); 1e-5 is asserted on
    the population means (all terms are positive, so the relative bound carries over to their mean).  The components' rates each sum
    to T over all genes, and a mixture mean lies between its two rates, hence 0 < sum over genes of ``mean`` <= sum of the larger
    rate <= 2 * (mean observed total); equality with the mean total is NOT an identity (the mixing weight differs from gene to gene),
    the ratio is printed."""
    from spvipes_amd.model import spVIPES
    paired = config.startswith("paired")
    ad = _adata(config)
    X = _dense(ad)
    spVIPES.setup_anndata(ad, groups_key="groups", **({"transport_plan_key": "plan"} if paired else {"label_key": "cell_type"}))
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=config.split("-")[1])
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    n = [len(g) for g in gi]
    pos = [np.array([5, 0, 95, 5, 17]), np.array([79, 3, 0])]
    cols = [np.asarray(ad.uns["groups_var_indices"][g])[pos[g]] for g in range(2)]
    by_name = [[f"gene{c}" for c in cols[g]] for g in range(2)]   # the same selection, by name
    E = {c: model.get_normalized_expression(gi, gene_list=pos, component=c, use_mean=True, batch_size=BS) for c in COMPONENTS}
    model.module.train()   # the call must put the module into eval mode and restore this
    for g in range(2):
        V = np.stack([E[c][g] for c in COMPONENTS])   # [4, n_g, n_sel] fp32
        ct = np.asarray(ad.obs["cell_type"])[gi[g]]
        wanted = [3, 1] if g == 0 else [4, 1, 3]   # not sorted, one label left out: the frame follows this order
        for groupby, labels, genes, pops in ((None, None, pos[g], [("all", np.ones(n[g], dtype=bool))]),
                                             ("cell_type", wanted, by_name[g], [(v, ct == v) for v in wanted]),
                                             (ct.copy(), None, pos[g], [(v, ct == v) for v in np.unique(ct).tolist()])):
            df = model.expression_statistics(gi, g, groupby=groupby, labels=labels, gene_list=genes, batch_size=BS)
            assert model.module.training   # the training flag is restored
            assert list(df.columns) == COLUMNS and len(df) == len(pops) * len(pos[g])
            assert df["population"].tolist() == [p for p, _ in pops for _ in pos[g]]
            assert df["gene"].tolist() == [f"gene{c}" for _ in pops for c in cols[g]]
            sums = df.attrs["sums"]
            assert sums.shape == (len(pops), 8, len(pos[g])) and sums.dtype == np.float64
            for k, (name, mask) in enumerate(pops):
                assert mask.sum() > 1
                _hold_block(df.iloc[k * len(pos[g]):(k + 1) * len(pos[g])], sums[k], V[:, mask])
            if g == 0:
                np.testing.assert_array_equal(df["mean"].to_numpy()[3], df["mean"].to_numpy()[0])   # the repeated gene: the same column twice
    with pytest.raises(KeyError, match="99"):
        model.expression_statistics(gi, 0, groupby="cell_type", labels=[99])
    with pytest.raises(KeyError, match="nope"):
        model.expression_statistics(gi, 0, groupby="nope")
    with pytest.raises(KeyError, match="no_such_gene"):
        model.expression_statistics(gi, 0, gene_list=["no_such_gene"])
    with pytest.raises(ValueError):
        model.expression_statistics(gi, 0, groupby=np.zeros(3))
    assert model.module.training
    model.module.eval()

    # two calls agree bit for bit (all genes, every label); another batch size is another order of addition
    a = model.expression_statistics(gi, 1, groupby="cell_type", batch_size=BS)
    b = model.expression_statistics(gi, 1, groupby="cell_type", batch_size=BS)
    assert len(a) == 4 * 80 and a.equals(b) and np.array_equal(a.attrs["sums"], b.attrs["sums"])

    # library_size = "observed": each cell decodes at its own observed total (docstring)
    g = 0
    ct = np.asarray(ad.obs["cell_type"])[gi[g]]
    total = X[np.asarray(gi[g])][:, np.asarray(ad.uns["groups_var_indices"][g])].sum(1).astype(np.float64)
    assert (total > 0).all()
    unit = model.get_normalized_expression(gi, library_size=1.0, use_mean=True, batch_size=BS)[g].astype(np.float64)   # [n_0, 96]
    obs = model.expression_statistics(gi, g, groupby="cell_type", library_size="observed", batch_size=BS)
    labels = np.unique(ct).tolist()
    for k, v in enumerate(labels):
        blk = obs.iloc[k * 96:(k + 1) * 96]
        want = (unit[ct == v] * total[ct == v, None]).mean(0)
        assert (np.abs(blk["mean"].to_numpy() - want) <= 1e-5 * want).all()
        ratio = blk["mean"].sum() / total[ct == v].mean()
        print(f"{config}: label {v}: sum over genes of mean / mean observed total = {ratio:.5f} (derivable: in (0, 2])")
        assert 0.0 < ratio <= 2.0 * (1 + 1e-5)
    latent = model.expression_statistics(gi, g, groupby="cell_type", batch_size=BS)
    np.testing.assert_array_equal(latent["mixing"].to_numpy(), obs["mixing"].to_numpy())   # the mixing weight does not see the library

    # sampled latents, n_samples = 2: both draws of a step add to the table -- the sums of the two single-draw tables whose draw d is
    # the double-draw walk's draw 2 d + s, within the bound of the 2 n values; n_samples is reported and n doubles
    nf = _noise_fn(dev)
    both = model.expression_statistics(gi, g, groupby="cell_type", gene_list=pos[g], n_samples=2, use_mean=False, batch_size=BS, _noise=nf)
    single = [model.expression_statistics(gi, g, groupby="cell_type", gene_list=pos[g], n_samples=1, use_mean=False, batch_size=BS,
                                          _noise=lambda d, b0, b1, s=s: nf(2 * d + s, b0, b1)) for s in (0, 1)]
    assert (both["n_samples"] == 2).all() and (single[0]["n_samples"] == 1).all() and both["n_cells"].equals(single[0]["n_cells"])
    assert not np.array_equal(single[0].attrs["sums"], single[1].attrs["sums"])
    for k, v in enumerate(labels):
        m = int((ct == v).sum())
        s2, s1 = both.attrs["sums"][k].astype(LD), single[0].attrs["sums"][k].astype(LD) + single[1].attrs["sums"][k].astype(LD)
        assert (np.abs(s2 - s1) <= 2 * _gamma(2 * m) * np.abs(s1)).all()   # all terms positive: sum|v| = the sum itself; two tables, each within the bound
        blk = both.iloc[k * len(pos[g]):(k + 1) * len(pos[g])]
        np.testing.assert_array_equal(blk["mean"].to_numpy(), both.attrs["sums"][k, 0] / (2 * m))
        avg = (single[0]["mean"].to_numpy()[k * len(pos[g]):(k + 1) * len(pos[g])] + single[1]["mean"].to_numpy()[k * len(pos[g]):(k + 1) * len(pos[g])]) / 2
        np.testing.assert_allclose(blk["mean"].to_numpy(), avg, rtol=1e-14)
    with pytest.raises(ValueError, match="use_mean"):
        model.expression_statistics(gi, g, n_samples=2)

    # a model restored by save / load returns the same frame
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=_adata(config))
    want = model.expression_statistics(gi, 0, groupby="cell_type", gene_list=pos[0], batch_size=BS)
    got = back.expression_statistics(gi, 0, groupby="cell_type", gene_list=pos[0], batch_size=BS)
    assert not back.module.training
    assert got.equals(want) and np.array_equal(got.attrs["sums"], want.attrs["sums"])
