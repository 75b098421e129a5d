"""GPU: spVIPES.latent_lisi / spVIPES.lisi on the duck AnnData of the silhouette API tests (300 / 260 cells; cell types 0..3 in group 0,
1..4 in group 1) -- label PoE in fp32, paired PoE in bf16 -- after two training epochs.

The frame is held to the references of tests/_lisi_reference.py on the very latents the model embeds (``_latents_on_device``, and under
``_noise`` the rows of ``get_latent_representation``): the neighbour lists the method rests on must EQUAL ``paged_ref`` of those latents (the
PoE gives fused cells the same posterior up to rounding, so the shared space holds pairs at distance 0 and ties: the (d, j) order decides),
the frame's columns must be the kernel's values on those lists bit for bit, and these lie within ``lisi_bound(k)`` of the float64
reference evaluated at the kernel's beta, which itself meets the perplexity wherever the reference converges.  Every test here needs the
feature and fails without it."""
import numpy as np
import pytest
import torch

from tests._lisi_reference import lisi_bound, lisi_ref, paged_ref
from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

BS = 40   # not a multiple of 32, smaller than either group


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _same(a, b):
    """two frames agree bit for bit, attrs included"""
    assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index)
    for c in a.columns:
        if a[c].dtype == np.float64:
            np.testing.assert_array_equal(a[c].to_numpy().view(np.uint64), b[c].to_numpy().view(np.uint64))
        else:
            assert a[c].tolist() == b[c].tolist()
    for key in a.attrs:
        if key == "per_label":
            assert (a.attrs[key] is None and b.attrs[key] is None) or a.attrs[key].equals(b.attrs[key])
        else:
            assert np.array_equal(a.attrs[key], b.attrs[key], equal_nan=True), key


def _hold(dev, frame, X, sets, perplexity, k):
    """the frame's LISI columns (``sets``: {column: codes [n]}) against the references, for the fp32 latents X [n, D] of its cells"""
    from spvipes_amd.knn_ops import knn_paged
    from spvipes_amd.lisi_ops import lisi
    n = len(X)
    me = np.arange(n, dtype=np.int32)
    Xd = torch.from_numpy(X).to(dev)
    idx, d2 = knn_paged(Xd, Xd, k, exclude=torch.from_numpy(me).to(dev))
    want = paged_ref(X, X, k, me)
    np.testing.assert_array_equal(idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    codes = np.stack([np.asarray(c) for c in sets.values()]).astype(np.int32)
    out, beta, n_valid, conv = (t.cpu().numpy() for t in lisi(idx, d2, torch.from_numpy(codes).to(dev), perplexity))
    for t, col in enumerate(sets):
        np.testing.assert_array_equal(frame[col].to_numpy().view(np.uint64), out[t].view(np.uint64), err_msg=col)
    assert frame["n_neighbors"].tolist() == n_valid.tolist() == [k] * n and frame["converged"].tolist() == conv.astype(bool).tolist()
    ref = lisi_ref(want[0], want[1], codes, perplexity)
    at = lisi_ref(want[0], want[1], codes, perplexity, beta=beta)
    on = ref[3]
    print(f"n {n} k {k}: reference converged on {int(on.sum())} rows, kernel on {int(conv.sum())}; zero distances {int((want[1] == 0).sum())}; "
          f"largest relative deviation {np.max(np.abs(out / at[0] - 1)):.3e} (bound {lisi_bound(k):.3e})")
    np.testing.assert_array_equal(conv.astype(bool), on)
    assert on.mean() > 0.9 and (np.abs(at[4][on] - np.log(perplexity)) <= 2e-5).all()
    np.testing.assert_allclose(beta[on], ref[1][on], rtol=1e-6, atol=0)
    assert (np.abs(out / at[0] - 1) <= lisi_bound(k)).all()
    assert frame.attrs["n_neighbors"] == k and frame.attrs["perplexity"] == perplexity and frame.attrs["n_unconverged"] == int((~on).sum())


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16"])
def test_latent_lisi(dev, monkeypatch, tmp_path, config):
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    paired = config.startswith("paired")
    ad = make_duck(seed=2, with_plan=paired)   # 300 / 260 cells
    spVIPES.setup_anndata(ad, groups_key="groups", **({"transport_plan_key": "plan"} if paired else {"label_key": "cell_type"}))
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=config.split("-")[1])
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    n = [len(g) for g in gi]
    cell_type = np.asarray(ad.obs["cell_type"])
    groups = np.concatenate([np.zeros(n[0], dtype=np.int64), np.ones(n[1], dtype=np.int64)])
    cats, codes = np.unique(cell_type, return_inverse=True)

    # posterior means, both groups, the standard perplexity: k = 89
    model.module.train()   # every call must put the module into eval mode and restore this
    zm = {g: t.cpu().numpy() for g, t in model._latents_on_device(gi, batch_size=BS).items()}
    Xm = np.concatenate([zm[0], zm[1]])
    frame = model.latent_lisi(gi, batch_size=BS)
    assert model.module.training
    assert list(frame.index) == gi[0] + gi[1] and list(frame.columns) == ["group", "label", "ilisi", "clisi", "n_neighbors", "converged"]
    assert frame["group"].tolist() == groups.tolist() and frame["label"].tolist() == cell_type.tolist()
    _hold(dev, frame, Xm, {"ilisi": groups, "clisi": codes}, 30, 89)
    il, cl = frame["ilisi"].to_numpy(), frame["clisi"].to_numpy()
    assert (il >= 1 - 1e-9).all() and (il <= 2 + 1e-9).all() and (cl >= 1 - 1e-9).all() and (cl <= 5 + 1e-9).all()
    a = frame.attrs
    assert a["ilisi_median"] == np.median(il) and a["clisi_median"] == np.median(cl)
    assert a["ilisi_scaled"] == (np.median(il) - 1) / 1 and a["clisi_scaled"] == (5 - np.median(cl)) / 4
    per = a["per_label"]
    assert list(per.index) == list(cats) and per["n_group0"].tolist() == [int(((cell_type == u) & (groups == 0)).sum()) for u in cats]
    assert per["n_group1"].tolist() == [int(((cell_type == u) & (groups == 1)).sum()) for u in cats]
    assert per["ilisi"].tolist() == [float(np.median(il[cell_type == u])) for u in cats] and per["clisi"].tolist() == [float(np.median(cl[cell_type == u])) for u in cats]
    _same(frame, model.latent_lisi(gi, batch_size=BS))   # give_mean=True twice: the same bits

    # one group: NaN ilisi; no labels: no clisi; another perplexity; the private space within a group
    for g in (0, 1):
        one = model.latent_lisi(gi, cells=g, perplexity=12.5, batch_size=BS)
        assert list(one.index) == gi[g] and np.isnan(one["ilisi"]).all() and np.isnan(one.attrs["ilisi_median"]) and np.isnan(one.attrs["ilisi_scaled"])
        _hold(dev, one, zm[g], {"clisi": np.unique(cell_type[gi[g]], return_inverse=True)[1]}, 12.5, 36)
    bare = model.latent_lisi(gi, labels=None, batch_size=BS)
    assert list(bare.columns) == ["group", "label", "ilisi", "n_neighbors", "converged"] and bare.attrs["per_label"] is None and "clisi_median" not in bare.attrs
    np.testing.assert_array_equal(bare["ilisi"].to_numpy().view(np.uint64), il.view(np.uint64))   # the calibration does not depend on the label sets
    zp = model._latents_on_device(gi, latent="private", batch_size=BS)[0].cpu().numpy()
    priv = model.latent_lisi(gi, cells=0, latent="private", perplexity=85.67, batch_size=BS)
    assert zp.shape[1] == 5 and priv.attrs["n_neighbors"] == 256
    _hold(dev, priv, zp, {"clisi": np.unique(cell_type[gi[0]], return_inverse=True)[1]}, 85.67, 256)

    # sampled latents under _noise: the rows of get_latent_representation
    nf = _noise_fn(dev)
    host = model.get_latent_representation(gi, batch_size=BS, _noise=nf)["shared"]
    sampled = model.latent_lisi(gi, give_mean=False, batch_size=BS, _noise=nf)
    _hold(dev, sampled, np.concatenate([host[0], host[1]]), {"ilisi": groups, "clisi": codes}, 30, 89)
    assert not np.array_equal(sampled["ilisi"].to_numpy(), il)

    # labels as an array; names; the classmethod on an obsm key agrees with latent_lisi on the same rows
    lab = np.array([f"t{c}" for c in cell_type], dtype=object)
    by_array = model.latent_lisi(gi, labels=lab, batch_size=BS)
    np.testing.assert_array_equal(by_array["clisi"].to_numpy().view(np.uint64), cl.view(np.uint64))   # a renaming: every bit stays
    ad.obsm = {"X_shared": Xm, "X_pca": np.random.default_rng(0).standard_normal((ad.n_obs, 25)).astype(np.float32)}
    rep = spVIPES.lisi(ad, "X_shared", ["groups", "cell_type"])
    assert list(rep.columns) == ["lisi_groups", "lisi_cell_type", "n_neighbors", "converged"] and list(rep.index) == list(range(ad.n_obs))
    np.testing.assert_array_equal(rep["lisi_groups"].to_numpy().view(np.uint64), il.view(np.uint64))
    np.testing.assert_array_equal(rep["lisi_cell_type"].to_numpy().view(np.uint64), cl.view(np.uint64))
    assert rep.attrs["lisi_groups_median"] == a["ilisi_median"] and rep.attrs["lisi_cell_type_median"] == a["clisi_median"] and rep.attrs["n_neighbors"] == 89
    assert (rep.attrs["n_groups"], rep.attrs["n_cell_type"]) == (2, 5)
    pca = spVIPES.lisi(ad, "X_pca", "groups")   # random coordinates: the groups mix
    assert list(pca.columns) == ["lisi_groups", "n_neighbors", "converged"] and pca.attrs["lisi_groups_median"] > 1.8
    _same(pca, spVIPES.lisi(ad, ad.obsm["X_pca"], "groups"))

    # save / load: the loaded model gives the same frame
    model.save(str(tmp_path / "m"))
    _same(frame, spVIPES.load(str(tmp_path / "m"), ad).latent_lisi(gi, batch_size=BS))

    # names, and the refusals that need the model
    ad.obs_names = np.array([f"cell{i}" for i in range(ad.n_obs)])
    named = model.latent_lisi(gi, batch_size=BS)
    assert list(named.index) == [f"cell{i}" for i in gi[0] + gi[1]] and named["ilisi"].tolist() == frame["ilisi"].tolist()
    assert list(spVIPES.lisi(ad, "X_pca", "groups").index) == [f"cell{i}" for i in range(ad.n_obs)]
    with pytest.raises(KeyError):
        model.latent_lisi(gi, labels="no_such_column")
    with pytest.raises(ValueError, match="k must lie"):
        model.latent_lisi(gi, perplexity=86)
    bad = {g: torch.as_tensor(zm[g], device=dev).clone() for g in range(2)}
    bad[1][7, 2] = float("nan")
    monkeypatch.setattr(model, "_latents_on_device", lambda *a, **k: bad)
    with pytest.raises(ValueError, match="non-finite"):
        model.latent_lisi(gi, batch_size=BS)
