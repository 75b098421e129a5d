"""CPU: the host side of ``latent_tsne`` / ``spVIPES.tsne`` -- signatures, what is refused ahead of any device work, the symmetric affinities
as CSR and the PCA initial layout against numpy.  No GPU."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest

from spvipes_amd import data
from spvipes_amd.model import spVIPES
from tests import _tsne_reference as R


def test_signatures():
    p = inspect.signature(spVIPES.latent_tsne).parameters
    assert list(p)[:2] == ["self", "group_indices_list"]
    want = dict(cells="both", latent="shared", give_mean=True, perplexity=30, n_components=2, n_iter=1000, init="pca", seed=0, batch_size=None, _noise=None)
    assert {k: p[k].default for k in want} == want and p["schedule"].kind is inspect.Parameter.VAR_KEYWORD
    c = inspect.signature(spVIPES.tsne).parameters
    assert list(c)[:2] == ["adata", "use_rep"] and c["key_added"].default == "X_tsne" and c["device"].default is None
    assert c["schedule"].kind is inspect.Parameter.VAR_KEYWORD
    from spvipes_amd import tsne_ops
    t = inspect.signature(tsne_ops.tsne).parameters
    assert (t["early_exaggeration"].default, t["exaggeration_iter"].default, t["momentum"].default, t["min_gain"].default, t["n_iter"].default,
            t["learning_rate"].default) == (12.0, 250, (0.5, 0.8), 0.01, 1000, "auto")
    assert set(data.TSNE_SCHEDULE) <= set(t)


def test_neighbours_and_the_perplexity_window():
    assert [data.tsne_neighbors(p, n) for p, n in ((30, 10 ** 4), (20, 240), (5, 1000), (30, 40), (2, 5), (30, 1))] == [64, 60, 15, 39, 4, 0]
    s = data.check_tsne_args(240, 20.0)
    assert s["n_neighbors"] == 60 and s["learning_rate"] == 50.0 and s["momentum"] == (0.5, 0.8) and s["kl_every"] == 50
    assert data.check_tsne_args(50000, 30)["learning_rate"] == 50000 / 12 / 4
    assert data.check_tsne_args(10 ** 4, 32)["n_neighbors"] == 64          # the most the 64 neighbours carry
    for n, perp in ((10 ** 4, 33), (10 ** 4, 1.5), (40, 20), (4, 2), (240, float("nan")), (240, "30"), (240, True)):
        with pytest.raises(ValueError, match="perplexity"):
            data.check_tsne_args(n, perp)


@pytest.mark.parametrize("kw,word", [
    (dict(n_components=0), "n_components"), (dict(n_components=5), "n_components"), (dict(n_components=2.0), "n_components"),
    (dict(n_iter=0), "n_iter"), (dict(n_iter=10.5), "n_iter"), (dict(seed=-1), "seed"), (dict(init="spectral"), "init"),
    (dict(init=np.zeros((239, 2))), "init"), (dict(init=np.full((240, 2), np.nan)), "init"), (dict(early_exaggeration=0.5), "early_exaggeration"),
    (dict(exaggeration_iter=-1), "exaggeration_iter"), (dict(learning_rate=0), "learning_rate"), (dict(learning_rate="fast"), "learning_rate"),
    (dict(momentum=0.5), "momentum"), (dict(momentum=(0.5, 1.0)), "momentum"), (dict(min_gain=0), "min_gain"), (dict(kl_every=0), "kl_every")])
def test_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        data.check_tsne_args(240, 20.0, **kw)


def test_schedule_names_and_representation():
    assert data.check_tsne_schedule({"kl_every": 10, "momentum": (0.4, 0.7)}) == {"kl_every": 10, "momentum": (0.4, 0.7)}
    with pytest.raises(ValueError, match="unknown schedule"):
        data.check_tsne_schedule({"n_jobs": 4})
    rep = data.check_tsne_rep(np.arange(12.0).reshape(6, 2), 6)
    assert rep.dtype == np.float32 and rep.flags.c_contiguous
    for bad, n in ((np.zeros(6), None), (np.zeros((6, 65)), None), (np.zeros((6, 0)), None), (np.zeros((6, 2)), 7), (np.full((6, 2), np.inf), 6)):
        with pytest.raises(ValueError, match="use_rep"):
            data.check_tsne_rep(bad, n)


def test_classmethod_refuses_before_any_device_work():
    """every one of these raises on a machine without a GPU: the checks come first"""
    adata = SimpleNamespace(n_obs=240, obsm={"X_pca": np.random.default_rng(0).standard_normal((240, 10))})
    with pytest.raises(KeyError):
        spVIPES.tsne(adata, "X_missing")
    with pytest.raises(ValueError, match="perplexity"):
        spVIPES.tsne(adata, "X_pca", perplexity=40)
    with pytest.raises(ValueError, match="unknown schedule"):
        spVIPES.tsne(adata, "X_pca", perplexity=20, angle=0.5)
    with pytest.raises(ValueError, match="one row per cell"):
        spVIPES.tsne(adata, np.zeros((10, 3)), perplexity=2)
    assert "X_tsne" not in adata.obsm


def test_latent_tsne_refuses_before_any_device_work():
    model = SimpleNamespace()
    gi = [list(range(100)), list(range(100, 240))]
    for kw, word in ((dict(cells="both", latent="private"), "private"), (dict(cells=2), "cells"), (dict(latent="joint"), "latent"),
                     (dict(perplexity=40), "perplexity"), (dict(n_components=7), "n_components"), (dict(theta=0.5), "unknown schedule")):
        with pytest.raises(ValueError, match=word):
            spVIPES.latent_tsne.__wrapped__(model, gi, **kw)


def test_symmetrisation_against_dense_numpy():
    rng = np.random.default_rng(4)
    n, k = 50, 7
    idx = np.stack([rng.choice(np.delete(np.arange(n), i), k, replace=False) for i in range(n)]).astype(np.int32)
    Pc = rng.random((n, k))
    Pc /= Pc.sum(axis=1, keepdims=True)
    idx[3, 4:] = -1
    Pc[3, 4:] = 0
    Pc[3] /= Pc[3].sum()
    dense = np.zeros((n, n))
    for i in range(n):
        for s in range(k):
            if idx[i, s] >= 0:
                dense[i, idx[i, s]] = Pc[i, s]
    want = (dense + dense.T) / (2 * n)
    indptr, cols, vals = data.tsne_symmetrize(idx, Pc.astype(np.float32), n)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float32 and indptr[0] == 0 and indptr[-1] == len(cols) == len(vals)
    got = R.dense_p(indptr, cols, vals, n)
    assert np.array_equal(got > 0, want > 0) and np.abs(got - want).max() <= 2.0 ** -23 * want.max()
    assert np.array_equal(got, got.T), "symmetric bit for bit: both entries of a pair are one sum"
    assert all((np.diff(cols[indptr[i]:indptr[i + 1]]) > 0).all() for i in range(n)), "columns ascend within a row"
    assert abs(vals.astype(np.float64).sum() - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        data.tsne_symmetrize(np.full((n, k), n), Pc, n)


def test_pca_layout_against_the_svd():
    rng = np.random.default_rng(8)
    X = (rng.standard_normal((120, 6)) * np.array([5, 3, 2, 1, 0.5, 0.1])).astype(np.float32)
    for d in (1, 2, 3):
        Y = data.tsne_pca_layout(X, d)
        assert Y.dtype == np.float32 and Y.shape == (120, d)
        assert np.abs(Y - R.pca_ref(X, d)).max() <= 1e-4 * 1e-5    # float32 rounding of values of size 1e-4 and the two routes' 1e-12
        assert abs(Y[:, 0].astype(np.float64).std() - 1e-4) <= 1e-10 and np.abs(Y.astype(np.float64).mean(axis=0)).max() <= 1e-10
    assert np.array_equal(data.tsne_pca_layout(X, 2), data.tsne_pca_layout(X, 2))
    wide = data.tsne_pca_layout(X[:, :1], 2)
    assert (wide[:, 1] == 0).all()
    r = data.tsne_initial_layout("random", None, 30, 2, 5)
    assert np.array_equal(r, data.tsne_initial_layout("random", None, 30, 2, 5)) and 5e-5 < r.std() < 2e-4
    given = rng.standard_normal((30, 2))
    assert np.array_equal(data.tsne_initial_layout(given, None, 30, 2, 0), given.astype(np.float32))
