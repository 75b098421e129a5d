"""GPU: spVIPES.posterior_predictive_check on the duck AnnData -- label PoE in fp32 (dense and CSR input), paired PoE in bf16 with its
cycling walk, unequal group sizes.  The sampled columns are held to the numpy reduction of ``posterior_predictive_sample`` of the same
model with the same seed, injected latents, batch size and ``n_samples``: the integers are the same, so every column agrees to the
last bit after the one division (1 ulp is allowed for the square root in cv).  The observed columns are held to numpy on ``adata.X``.
Every test here needs the feature and fails without it."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

BS, NS = 32, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


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


def _columns(x):
    """x: integer array [N values, n_sel] -> (mean, var, cv, zero_fraction, max) per column, by exact integer / Fraction arithmetic"""
    out = []
    N = x.shape[0]
    for j in range(x.shape[1]):
        v = [int(t) for t in x[:, j]]
        S, NZ, Qs = sum(v), sum(t > 0 for t in v), sum(t * t for t in v)
        mean = float(Fraction(S, N))
        var = float(Fraction(N * Qs - S * S, N * (N - 1))) if N > 1 else float("nan")
        out.append((mean, var, math.sqrt(var) / mean if mean > 0 else float("nan"), float(Fraction(N - NZ, N)), float(max(v))))
    return np.array(out).T


def _close_1ulp(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    both_nan = np.isnan(got) & np.isnan(want)
    assert (both_nan | (np.abs(got - want) <= np.spacing(np.abs(want)))).all(), (got, want)


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16", "label-fp32-csr"])
def test_posterior_predictive_check(dev, tmp_path, config):
    from spvipes_amd.model import spVIPES
    paired = config.startswith("paired")
    ad = _adata(config)
    X = _dense(ad)
    spVIPES.setup_anndata(ad, groups_key="groups", **({"transport_plan_key": "plan"} if paired else {"label_key": "cell_type"}))
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=config.split("-")[1])
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    n, nf = [len(g) for g in gi], _noise_fn(dev)
    pos = [np.array([5, 0, 95, 5, 17]), np.array([79, 3, 0])]
    cols = [np.asarray(ad.uns["groups_var_indices"][g])[pos[g]] for g in range(2)]
    model.module.train()   # the call must put the module into eval mode and restore this
    cube = model.posterior_predictive_sample(gi, n_samples=NS, gene_list=pos, batch_size=BS, seed=3, _noise=nf)   # [n, n_sel, NS]
    stat_cols = ["mean", "var", "cv", "zero_fraction"]
    for g in range(2):
        ct = np.asarray(ad.obs["cell_type"])[gi[g]]
        wanted = [3, 1] if g == 0 else [4, 1, 3]   # not sorted: the frame follows this order
        for groupby, labels, pops in ((None, None, [("all", np.ones(n[g], dtype=bool))]),
                                      ("cell_type", wanted, [(v, ct == v) for v in wanted]),
                                      (ct.copy(), None, [(v, ct == v) for v in np.unique(ct).tolist()])):
            df = model.posterior_predictive_check(gi, g, n_samples=NS, groupby=groupby, labels=labels, gene_list=pos[g], batch_size=BS, seed=3, _noise=nf)
            assert model.module.training   # the training flag is restored
            assert list(df.columns) == ["population", "gene", "n_cells", "n_samples", "obs_mean", "obs_var", "obs_cv", "obs_zero_fraction",
                                        "ppc_mean", "ppc_var", "ppc_cv", "ppc_zero_fraction", "ppc_max"]
            assert len(df) == len(pops) * len(pos[g]) and (df["n_samples"] == NS).all()
            assert df["population"].tolist() == [p for p, _ in pops for _ in pos[g]]
            assert df["gene"].tolist() == [f"gene{c}" for _ in pops for c in cols[g]]
            for k, (name, mask) in enumerate(pops):
                blk = df.iloc[k * len(pos[g]):(k + 1) * len(pos[g])]
                assert mask.sum() > 1 and (blk["n_cells"] == mask.sum()).all()
                # sampled columns: the reduction of the stored draws of the population's cells, all samples together
                x = cube[g][mask].transpose(0, 2, 1).reshape(-1, len(pos[g]))
                want = _columns(x)
                for c, w in zip(stat_cols + ["max"], want):
                    _close_1ulp(blk["ppc_" + c], w)
                    if c != "cv":
                        np.testing.assert_array_equal(blk["ppc_" + c].to_numpy(), w)   # one division of the same integers: equal
                # observed columns: numpy on adata.X
                want = _columns(X[np.asarray(gi[g])[mask]][:, cols[g]].astype(np.int64))
                for c, w in zip(stat_cols, want[:4]):
                    _close_1ulp(blk["obs_" + c], w)
            tot = df.attrs["cell_totals"]
            assert list(tot.columns) == ["obs_total", "ppc_total_mean"] and tot.index.tolist() == gi[g]   # get_latent_representation's row order
            inside = np.zeros(n[g], dtype=bool)
            for _, mask in pops:
                inside |= mask
            np.testing.assert_array_equal(tot["obs_total"].to_numpy()[inside], X[np.asarray(gi[g])][:, cols[g]].sum(1)[inside])
            np.testing.assert_array_equal(tot["ppc_total_mean"].to_numpy()[inside], cube[g].astype(np.int64).sum((1, 2))[inside] / NS)
            assert tot[~inside].isna().all().all()
            if labels is not None:
                assert (~inside).any()   # one label is left out
    with pytest.raises(KeyError, match="99"):
        model.posterior_predictive_check(gi, 0, groupby="cell_type", labels=[99])
    with pytest.raises(KeyError, match="nope"):
        model.posterior_predictive_check(gi, 0, groupby="nope")
    with pytest.raises(ValueError):
        model.posterior_predictive_check(gi, 0, groupby=np.zeros(3))

    # all genes, the other seed: another table; the same seed: the same table
    a = model.posterior_predictive_check(gi, 1, n_samples=2, batch_size=BS, seed=3, _noise=nf)
    b = model.posterior_predictive_check(gi, 1, n_samples=2, batch_size=BS, seed=3, _noise=nf)
    c = model.posterior_predictive_check(gi, 1, n_samples=2, batch_size=BS, seed=4, _noise=nf)
    assert len(a) == 80 and a.equals(b) and a.attrs["cell_totals"].equals(b.attrs["cell_totals"]) and not a["ppc_mean"].equals(c["ppc_mean"])
    assert a[["obs_mean", "obs_var", "obs_cv", "obs_zero_fraction"]].equals(c[["obs_mean", "obs_var", "obs_cv", "obs_zero_fraction"]])
    model.module.eval()

    # library_size="observed": every cell's rates sum to its observed total, so its drawn totals scatter around it
    g = 0
    obs = model.posterior_predictive_check(gi, g, n_samples=64, library_size="observed", batch_size=BS, seed=5, _noise=nf)
    t = obs.attrs["cell_totals"]
    np.testing.assert_array_equal(t["obs_total"].to_numpy(), X[np.asarray(gi[g])][:, np.asarray(ad.uns["groups_var_indices"][g])].sum(1))
    has = t["obs_total"].to_numpy() > 0
    ratio = t["ppc_total_mean"].to_numpy()[has] / t["obs_total"].to_numpy()[has]
    se = ratio.std(ddof=1) / math.sqrt(ratio.size)   # the standard error, from the sampled totals themselves
    print(f"{config}: mean of ppc_total_mean / obs_total over {ratio.size} cells = {ratio.mean():.5f}, standard error {se:.5f}, "
          f"|mean - 1| / (6 se) = {abs(ratio.mean() - 1.0) / (6.0 * se):.3f} (must be <= 1)")
    assert abs(ratio.mean() - 1.0) <= 6.0 * se

    # a model restored by save / load returns the same frame
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=_adata(config))
    want = model.posterior_predictive_check(gi, 0, n_samples=NS, groupby="cell_type", gene_list=pos[0], batch_size=BS, seed=3, _noise=nf)
    got = back.posterior_predictive_check(gi, 0, n_samples=NS, groupby="cell_type", gene_list=pos[0], batch_size=BS, seed=3, _noise=nf)
    assert not back.module.training
    assert got.equals(want) and got.attrs["cell_totals"].equals(want.attrs["cell_totals"])


def test_a_cell_without_counts_draws_zero_at_the_observed_library(dev):
    """the library seam: a per-cell log library wins over ``library_size``; log(0) = -inf gives rate 0 and, by the sampler's rule for zero
    rates, draws 0 -- through the module on one minibatch, and through the method with one cell's cached observed total set to 0"""
    from spvipes_amd.model import spVIPES
    ad = _adata("label-fp32")
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32", counts_storage="dense")
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=1, train_size=1.0)
    nf, g, G = _noise_fn(dev), 0, 96
    step, tensors, (B0, B1) = next(iter(model._eval_minibatches(gi, BS, None)))
    model.module.eval()
    inf = model._infer(tensors, nf, 0, B0, B1)
    lib = torch.full((B0,), math.log(500.0), device=dev)
    lib[3] = float("-inf")
    stats = torch.zeros((1, 4, G), dtype=torch.int64, device=dev)
    total = torch.zeros(B0, dtype=torch.int64, device=dev)
    model.module.sample_count_stats(inf, g, library=lib, library_size=7.0, key=1, sample=0, stats=stats, cell_total=total)
    total = total.cpu().numpy()
    assert total[3] == 0 and (np.delete(total, 3) > 100).all() and int(stats[0, 0].sum()) == total.sum()   # (library 500, not 7)
    # the method: the total count_totals keeps on the resident matrix is the library; cell 5's is set to 0 (its counts stay, so the
    # encoders see the cell as it is)
    from spvipes_amd.count_ops import count_totals
    count_totals(model.counts[g])[5] = 0
    df = model.posterior_predictive_check(gi, g, n_samples=4, library_size="observed", batch_size=BS, seed=1, _noise=nf)
    t = df.attrs["cell_totals"]
    assert t["obs_total"].iloc[5] > 0 and t["ppc_total_mean"].iloc[5] == 0 and (t["ppc_total_mean"].drop(t.index[5]) > 0).all()
    assert np.isfinite(df["ppc_mean"]).all() and np.isfinite(df["obs_mean"]).all()
