"""GPU: the user API of the exact t-SNE.

``spVIPES.tsne`` on a planted ``obsm``: three Gaussian blobs of 80 cells at D = 10 and unit variance, centres
default_rng(0).standard_normal((3, 10)) * 4 / sqrt(2), perplexity 20, 500 steps.  Required: (i) two runs agree bit for bit; (ii) the
reported KL divergence is the float64 one recomputed from the returned embedding and P within the kernels' bound -- kl_row carries
(D + 4) 2^-24 of the mass of P, which is 1, and log Z the relative error of Z, (D + 4) 2^-24 again (tests/test_tsne_gpu_update.py,
tests/test_tsne_gpu_repulsion.py), so 2 (D + 4) (1 + 2^-10) 2^-24 and 1e-10 for the fp64 sums; the recomputation takes log Z once, as
the contract does, not sum(P) times (the fp32 entries sum to 1 within 2^-24 only); (iii) the final KL is below 0.75 of the KL after 250
steps; (iv) at least 97 % of the cells have their nearest neighbour of the layout in their own blob.  (iii) and (iv) are conditions:
the float64 prototype of the schedule gives 0.40 to 0.44 and at least 0.996 on seeds 0 to 2 (tests/test_tsne_reference_cpu.py runs seed 0).

``model.latent_tsne`` on the duck AnnData after two epochs: rows, index, ``group``, shapes, ``cells``, the "private" rule, equality with
the driver on ``_latents_on_device``'s rows, and the training flag.  Every test here needs the feature and fails without it.

This file and its three siblings are named test_tsne_gpu_*, which sorts behind every other GPU test of the suite: docs/lab_notes.md
section AA says why."""
import numpy as np
import pytest
import torch

from tests import _tsne_reference as R

pytestmark = pytest.mark.gpu
BS = 40


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def planted(dev):
    from types import SimpleNamespace
    from spvipes_amd.model import spVIPES
    X, lab = R.blobs(0)
    ad = SimpleNamespace(n_obs=X.shape[0], obsm={"X_rep": X})
    runs = [spVIPES.tsne(ad, "X_rep", perplexity=20, n_iter=500) for _ in range(2)]
    return ad, X, lab, runs


def test_two_runs_agree_bit_for_bit(planted):
    ad, X, _lab, (a, b) = planted
    assert np.array_equal(a.embedding, b.embedding) and a.kl_divergence == b.kl_divergence and np.array_equal(a.kl_history, b.kl_history)
    assert np.array_equal(a.beta, b.beta) and all(np.array_equal(p, q) for p, q in zip(a.affinities, b.affinities))
    assert a.embedding.dtype == np.float32 and a.embedding.shape == (240, 2) and ad.obsm["X_tsne"] is b.embedding
    assert a.n_neighbors == 60 and a.beta.shape == (240,) and (a.beta > 0).all()
    assert np.abs(a.embedding.astype(np.float64).mean(axis=0)).max() <= 2.0 ** -24 * np.abs(a.embedding).max(), "centred in fp64, rounded once"
    assert a.kl_history[:, 0].tolist() == list(range(0, 500, 50)) + [500] and a.kl_history[-1, 1] == a.kl_divergence


def test_affinities_are_the_references(planted):
    """the joint P from the k-NN kernel, the calibration kernel and the host symmetrisation against the dense float64 route"""
    _ad, X, _lab, (a, _b) = planted
    P = R.dense_p(*a.affinities, 240)
    want = R.knn_p(X, 20.0, 60)
    assert np.array_equal(P > 0, want > 0) and np.abs(P - want).max() <= 1e-5 * want.max()   # beta stops anywhere inside the 1e-5 window of the entropy


def test_reported_kl_is_the_layouts(planted):
    _ad, _X, _lab, (a, _b) = planted
    P = R.dense_p(*a.affinities, 240)
    Y = a.embedding
    Z = R.repulsion_ref(Y, Y, np.arange(240))["Z"].sum()
    want = R.kl_ref(Y, P) + (1.0 - P.sum()) * np.log(Z)
    D = 2
    assert abs(a.kl_divergence - want) <= 2 * (D + 4) * R.U * R.HIGHER + 1e-10, abs(a.kl_divergence - want)


def test_the_layout_converges_and_keeps_the_blobs(planted):
    _ad, _X, lab, (a, _b) = planted
    at250 = a.kl_history[a.kl_history[:, 0] == 250, 1][0]
    print(f"KL 250 -> 500: {at250:.4f} -> {a.kl_divergence:.4f} ({a.kl_divergence / at250:.3f}); neighbour share {R.neighbour_share(a.embedding, lab):.4f}")
    assert a.kl_divergence < 0.75 * at250
    assert R.neighbour_share(a.embedding, lab) >= 0.97


def test_latent_tsne_on_the_duck(dev):
    from spvipes_amd.model import spVIPES
    from spvipes_amd.tsne_ops import tsne
    from tests._duck import make_duck
    ad = make_duck(seed=2)   # 300 / 260 cells
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32")
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    n = [len(g) for g in gi]
    kw = dict(n_iter=40, kl_every=10, batch_size=BS)

    model.module.train()   # every call must put the module into eval mode and restore this
    z = model._latents_on_device(gi, batch_size=BS)
    frame = model.latent_tsne(gi, **kw)
    assert model.module.training
    assert list(frame.index) == gi[0] + gi[1] and list(frame.columns) == ["group", "tsne_1", "tsne_2"]
    assert frame["group"].tolist() == [0] * n[0] + [1] * n[1] and frame["tsne_1"].dtype == np.float32
    assert sorted(frame.attrs) == ["kl_divergence", "kl_history", "n_neighbors", "perplexity"]
    assert frame.attrs["perplexity"] == 30.0 and frame.attrs["n_neighbors"] == 64 and frame.attrs["kl_history"].shape == (5, 2)
    direct = tsne(torch.cat([z[0], z[1]]), n_iter=40, kl_every=10)
    assert np.array_equal(frame[["tsne_1", "tsne_2"]].to_numpy(), direct.embedding) and frame.attrs["kl_divergence"] == direct.kl_divergence
    assert np.array_equal(frame.attrs["kl_history"], direct.kl_history)

    three = model.latent_tsne(gi, n_components=3, init="random", seed=4, **kw)
    assert list(three.columns) == ["group", "tsne_1", "tsne_2", "tsne_3"] and three.shape == (n[0] + n[1], 4) and np.isfinite(three.to_numpy()).all()
    for g in (0, 1):
        one = model.latent_tsne(gi, cells=g, **kw)
        assert list(one.index) == gi[g] and (one["group"] == g).all() and one.shape == (n[g], 3)
        assert np.array_equal(one[["tsne_1", "tsne_2"]].to_numpy(), tsne(z[g], n_iter=40, kl_every=10).embedding)
    zp = model._latents_on_device(gi, latent="private", batch_size=BS)
    priv = model.latent_tsne(gi, cells=1, latent="private", **kw)
    assert zp[1].shape[1] == 5 and np.array_equal(priv[["tsne_1", "tsne_2"]].to_numpy(), tsne(zp[1], n_iter=40, kl_every=10).embedding)
    with pytest.raises(ValueError, match="private"):
        model.latent_tsne(gi, latent="private", **kw)
    with pytest.raises(ValueError, match="perplexity"):
        model.latent_tsne(gi, perplexity=33, **kw)
    assert model.module.training
    ad.obs_names = np.array([f"cell{i}" for i in range(ad.n_obs)])
    assert list(model.latent_tsne(gi, cells=1, **kw).index) == [f"cell{i}" for i in gi[1]]
