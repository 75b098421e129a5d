"""GPU: spVIPES.latent_neighbors / transfer_labels / _latents_on_device on the duck AnnData (300 / 260 cells) -- label PoE in fp32, paired
PoE in bf16 with its cycling walk -- after two training epochs.  The yardstick is tests/_knn_reference.py on the very latents the
model embeds: ``knn_ref`` is exact, so indices must be equal and distances must be the float32 square roots of its distances.  Every
test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests._knn_reference import knn_ref
from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

BS = 40   # not a multiple of 32, smaller than either group


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _adata(paired):
    from tests._duck import make_duck
    return make_duck(seed=2, with_plan=paired)   # 300 / 260 cells


def _sqrt32(d2):
    with np.errstate(invalid="ignore"):
        return np.sqrt(d2.astype(np.float32))


def _hold(nb, Zq, Zt, k, exclude=None):
    idx, d2 = knn_ref(Zq, Zt, k, exclude)
    np.testing.assert_array_equal(nb["indices"], idx)
    np.testing.assert_array_equal(nb["distances"].view(np.uint32), _sqrt32(d2).view(np.uint32))
    assert nb["indices"].dtype == np.int32 and nb["distances"].dtype == np.float32


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16"])
def test_latent_neighbors(dev, tmp_path, config):
    from spvipes_amd.data import vote_labels
    from spvipes_amd.model import spVIPES
    paired = config.startswith("paired")
    ad = _adata(paired)
    spVIPES.setup_anndata(ad, groups_key="groups", **({"transport_plan_key": "plan"} if paired else {"label_key": "cell_type"}))
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=config.split("-")[1])
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    n = [len(g) for g in gi]
    nf = _noise_fn(dev)

    # the sampled latents on the device are the ones get_latent_representation returns, bit for bit
    model.module.train()   # every call must put the module into eval mode and restore this
    host = model.get_latent_representation(gi, batch_size=BS, _noise=nf)
    for latent in ("shared", "private"):
        z = model._latents_on_device(gi, latent=latent, give_mean=False, batch_size=BS, _noise=nf)
        for g in range(2):
            assert z[g].is_cuda and z[g].dtype == torch.float32 and tuple(z[g].shape) == host[latent][g].shape and z[g].shape[0] == n[g]
            np.testing.assert_array_equal(z[g].cpu().numpy().view(np.uint32), host[latent][g].view(np.uint32))
    assert model.module.training

    # sampled latents: cross-group, within a group (self excluded, self included), both; private within a group
    S, Pv = host["shared"], host["private"]
    both = np.concatenate([S[0], S[1]])
    kw = dict(give_mean=False, batch_size=BS, _noise=nf)
    nb = model.latent_neighbors(gi, k=15, **kw)
    _hold(nb, S[0], S[1], 15)
    np.testing.assert_array_equal(nb["query_obs"], np.asarray(gi[0]))
    np.testing.assert_array_equal(nb["target_obs"], np.asarray(gi[1]))
    assert (np.diff(nb["distances"], axis=1) >= 0).all() and (nb["distances"] > 0).all()
    _hold(model.latent_neighbors(gi, k=7, query=1, target=0, **kw), S[1], S[0], 7)
    within = model.latent_neighbors(gi, k=16, query=1, target=1, **kw)
    _hold(within, S[1], S[1], 16, np.arange(n[1]))
    assert (within["indices"] != np.arange(n[1])[:, None]).all()
    incl = model.latent_neighbors(gi, k=16, query=1, target=1, include_self=True, **kw)
    _hold(incl, S[1], S[1], 16)
    assert (incl["indices"][:, 0] == np.arange(n[1])).all() and (incl["distances"][:, 0] == 0).all()
    mix = model.latent_neighbors(gi, k=15, query="both", target="both", **kw)
    _hold(mix, both, both, 15, np.arange(n[0] + n[1]))
    np.testing.assert_array_equal(mix["target_obs"], np.concatenate([gi[0], gi[1]]))
    np.testing.assert_array_equal(mix["query_obs"], mix["target_obs"])
    other = (mix["target_obs"][mix["indices"]] >= n[0]) != (mix["query_obs"] >= n[0])[:, None]   # the README's mixing score
    assert 0.0 <= other.mean() <= 1.0
    _hold(model.latent_neighbors(gi, k=15, query=0, target="both", **kw), S[0], both, 15, np.arange(n[0]))
    _hold(model.latent_neighbors(gi, k=15, query=1, target="both", **kw), S[1], both, 15, n[0] + np.arange(n[1]))
    _hold(model.latent_neighbors(gi, k=5, query=0, target=0, latent="private", **kw), Pv[0], Pv[0], 5, np.arange(n[0]))
    assert model.module.training

    # posterior means: deterministic, and neighbours of the means the helper returns
    a = model.latent_neighbors(gi, k=15, batch_size=BS)
    b = model.latent_neighbors(gi, k=15, batch_size=BS)
    np.testing.assert_array_equal(a["indices"], b["indices"])
    np.testing.assert_array_equal(a["distances"].view(np.uint32), b["distances"].view(np.uint32))
    zm = model._latents_on_device(gi, batch_size=BS)
    _hold(a, zm[0].cpu().numpy(), zm[1].cpu().numpy(), 15)
    assert not np.array_equal(zm[0].cpu().numpy(), S[0])   # the means are not the samples
    dv = model.latent_neighbors(gi, k=15, batch_size=BS, return_numpy=False)
    assert dv["indices"].is_cuda and dv["distances"].is_cuda and np.array_equal(dv["indices"].cpu().numpy(), a["indices"])

    # k larger than the target set: a subset of 40 target cells, k = 50
    few = [gi[0], gi[1][:40]]
    short = model.latent_neighbors(few, k=50, batch_size=BS)
    assert (short["indices"][:, 40:] == -1).all() and np.isinf(short["distances"][:, 40:]).all()
    assert (np.sort(short["indices"][:, :40], axis=1) == np.arange(40)).all() and np.isfinite(short["distances"][:, :40]).all()
    np.testing.assert_array_equal(short["target_obs"], np.asarray(gi[1][:40]))

    # transfer_labels: the vote over the returned indices, a frame as specified
    frame = model.transfer_labels(gi, source=1, target=0, labels="cell_type", k=15, batch_size=BS)
    nb = model.latent_neighbors(gi, k=15, query=0, target=1, batch_size=BS)
    cats, codes = np.unique(np.asarray(ad.obs["cell_type"])[gi[1]], return_inverse=True)
    pred, conf, nv = vote_labels(nb["indices"], codes, len(cats))
    assert list(frame.columns) == ["predicted", "confidence", "n_neighbors"] and list(frame.index) == list(gi[0])
    assert frame["predicted"].tolist() == cats[pred].tolist() and (frame["n_neighbors"] == 15).all()
    np.testing.assert_array_equal(frame["confidence"].to_numpy(), conf)
    assert ((conf >= 1 / len(cats)) & (conf <= 1)).all()
    by_array = model.transfer_labels(gi, source=1, target=0, labels=np.asarray(ad.obs["cell_type"])[gi[1]], k=15, batch_size=BS)
    assert by_array.equals(frame)
    back_frame = model.transfer_labels(gi, source=0, target=1, k=3, batch_size=BS)
    assert list(back_frame.index) == list(gi[1]) and set(back_frame["predicted"]) <= set(np.asarray(ad.obs["cell_type"])[gi[0]].tolist())
    ad.obs_names = np.array([f"cell{i}" for i in range(ad.n_obs)])
    named = model.transfer_labels(gi, k=15, batch_size=BS)
    assert list(named.index) == [f"cell{i}" for i in gi[0]] and named["predicted"].tolist() == frame["predicted"].tolist()
    with pytest.raises(ValueError):
        model.transfer_labels(gi, labels=np.zeros(3))
    with pytest.raises(KeyError):
        model.transfer_labels(gi, labels="no_such_column")
    assert model.module.training

    # a model restored by save / load returns the same neighbours
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=_adata(paired))
    got = back.latent_neighbors(gi, k=15, batch_size=BS)
    assert not back.module.training
    np.testing.assert_array_equal(got["indices"], a["indices"])
    np.testing.assert_array_equal(got["distances"].view(np.uint32), a["distances"].view(np.uint32))
