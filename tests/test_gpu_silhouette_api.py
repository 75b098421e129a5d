"""GPU: spVIPES.latent_silhouette / integration_scores on the duck AnnData (300 / 260 cells; cell types 0..3 in group 0, 1..4 in group 1,
so two labels live in one group only) -- label PoE in fp32, paired PoE in bf16 -- after two training epochs.  Two yardsticks:
tests/_silhouette_reference.py's ``segment_sums_ref`` on the very latents the model embeds, from which ``data.silhouette_table`` must give
the frame's columns EXACTLY, and the float64 ``silhouette_ref`` / ``group_silhouette_ref`` on
the same latents widened to float64, within BOUND.

The sums of the PRIVATE latents are exact in fp64 (``sums_are_exact``, asserted), so numpy's pairwise sums and the kernel's sequential ones
are the same bits.  The sums of the SHARED latents are not, and that is asserted too: the PoE gives the cells it fuses (the cells of a
label in a minibatch, the mates of a plan) the same posterior up to rounding, so the shared space holds pairs at distance 0 and a few
hundred at 1e-10 .. 1e-6 next to a median of 0.22 (measured on this model: smallest positive distance 2.3e-10 in fp32 mode, 5.2e-10 in
bf16 mode), whose last places lie 30 bits below the sums'.  There the frame is held to ``segment_sums_ref(..., n_split=)``, the same
terms added in the order the kernel's contract states, which is bit equality on any data: no less than the pairwise sums would ask.

BOUND = 4 * (D / 2 + 3) * 2^-24: the D-term fp32 chain and the rounded root give each distance a relative error of at most about
(D / 2 + 2) * 2^-24; a silhouette is +-(1 - min / max) of two means of such distances, which at most doubles that error; the bound
carries a further factor of two.  Every test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests._silhouette_reference import distances_ref, group_silhouette_ref, scores_ref, segment_sums_ref, silhouette_ref, sums_are_exact
from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

BS = 40   # not a multiple of 32, smaller than either group
COLS = ["group", "label", "silhouette_label", "a", "b", "nearest_label", "silhouette_group"]


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
    assert np.array_equal([a.attrs["label_asw"], a.attrs["group_asw"]], [b.attrs["label_asw"], b.attrs["group_asw"]], equal_nan=True)
    assert a.attrs["per_label"].equals(b.attrs["per_label"])


def _hold(frame, X, labels, groups, exact):
    """the frame against both yardsticks, for the fp32 latents X [n, D] of its cells; ``exact``: whether their sums are exact in fp64"""
    from spvipes_amd.data import silhouette_segments, silhouette_table
    from spvipes_amd.silhouette_ops import silhouette_splits
    D = X.shape[1]
    bound = 4 * (D / 2 + 3) * 2.0 ** -24
    cats, codes = np.unique(labels, return_inverse=True)
    perm, seg_ptr, sizes = silhouette_segments(codes, groups, len(cats))
    d = distances_ref(X, X[perm])
    # the sums in the order of addition the contract states, for the chunk count the method takes (one for the whole selection): the
    # kernel's bits on any data.  Where the sums are exact, numpy's own order must give the same bits.
    n_split = silhouette_splits(len(X), len(X))
    sums = segment_sums_ref(X, X[perm], seg_ptr, d=d, n_split=n_split)
    is_exact = sums_are_exact(d, seg_ptr)
    print(f"n {len(X)} D {D}: sums exact in fp64: {is_exact}; smallest positive distance {d[d > 0].min():.3e}, median {np.median(d[d > 0]):.3e}")
    assert exact is None or is_exact == exact
    if is_exact:
        np.testing.assert_array_equal(sums.view(np.uint64), segment_sums_ref(X, X[perm], seg_ptr, d=d).view(np.uint64))
    want = silhouette_table(sums, sizes, codes, groups)
    for c in ("a", "b", "silhouette_label", "silhouette_group"):
        np.testing.assert_array_equal(frame[c].to_numpy().view(np.uint64), want[c].view(np.uint64), err_msg=c)
    assert frame["nearest_label"].tolist() == [None if u < 0 else cats[u] for u in want["nearest_label"]]

    X64 = X.astype(np.float64)
    s, a, b, near = silhouette_ref(X64, labels)
    s_g = group_silhouette_ref(X64, labels, groups)
    for got, ref, name in ((frame["silhouette_label"].to_numpy(), s, "silhouette_label"), (frame["silhouette_group"].to_numpy(), s_g, "silhouette_group")):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        err = np.nanmax(np.abs(got - ref)) if (~np.isnan(ref)).any() else 0.0
        print(f"{name}: largest difference from the float64 definition {err:.3e} (bound {bound:.3e})")
        assert err <= bound
    # nearest_label where the reference's two smallest mean distances to other labels differ by more than the bound
    Dm = np.sqrt(((X64[:, None, :] - X64[None, :, :]) ** 2).sum(-1))
    means = np.stack([Dm[:, labels == u].mean(axis=1) for u in cats], axis=1)
    means[np.arange(len(labels)), codes] = np.inf
    two = np.sort(means, axis=1)[:, :2]
    if len(cats) > 2:
        clear = (two[:, 1] - two[:, 0]) > bound * two[:, 1]
        assert clear.sum() > len(labels) // 2
        assert [frame["nearest_label"].iloc[i] for i in np.flatnonzero(clear)] == [near[i] for i in np.flatnonzero(clear)]
    # the scores are the formulas applied to the columns
    want_l, want_g = scores_ref(frame["silhouette_label"].to_numpy(), frame["silhouette_group"].to_numpy(), labels)
    assert abs(frame.attrs["label_asw"] - want_l) <= 1e-12
    assert (np.isnan(want_g) and np.isnan(frame.attrs["group_asw"])) or abs(frame.attrs["group_asw"] - want_g) <= 1e-12
    per = frame.attrs["per_label"]
    assert list(per.index) == list(cats) and list(per.columns) == ["n_group0", "n_group1", "silhouette_label", "group_mixing"]
    assert per["n_group0"].tolist() == [int(((labels == u) & (groups == 0)).sum()) for u in cats]
    assert per["n_group1"].tolist() == [int(((labels == u) & (groups == 1)).sum()) for u in cats]
    for u in cats:
        assert abs(per.loc[u, "silhouette_label"] - frame["silhouette_label"].to_numpy()[labels == u].mean()) <= 1e-12
        mix = 1 - np.abs(frame["silhouette_group"].to_numpy()[labels == u])
        assert (np.isnan(per.loc[u, "group_mixing"]) and np.isnan(mix).all()) or abs(per.loc[u, "group_mixing"] - mix.mean()) <= 1e-12
    assert list(frame.columns) == COLS and frame["group"].tolist() == groups.tolist() and frame["label"].tolist() == labels.tolist()


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16"])
def test_latent_silhouette(dev, monkeypatch, config):
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
    nf = _noise_fn(dev)
    cell_type = np.asarray(ad.obs["cell_type"])
    groups = np.concatenate([np.zeros(n[0], dtype=np.int64), np.ones(n[1], dtype=np.int64)])

    # posterior means, both groups: the frame against the latents the helper returns
    model.module.train()   # every call must put the module into eval mode and restore this
    zm = {g: t.cpu().numpy() for g, t in model._latents_on_device(gi, batch_size=BS).items()}
    Xm = np.concatenate([zm[0], zm[1]])
    frame = model.latent_silhouette(gi, batch_size=BS)
    assert model.module.training
    assert list(frame.index) == gi[0] + gi[1] and len(frame) == n[0] + n[1]
    _hold(frame, Xm, cell_type, groups, exact=False)
    assert np.isnan(frame["silhouette_group"][(cell_type == 0) | (cell_type == 4)]).all()       # labels of one group only
    assert np.isfinite(frame["silhouette_group"][(cell_type >= 1) & (cell_type <= 3)]).all()
    assert 0 <= frame.attrs["label_asw"] <= 1 and 0 <= frame.attrs["group_asw"] <= 1
    _same(frame, model.latent_silhouette(gi, batch_size=BS))                                      # give_mean=True twice: the same bits

    # a tiny forced query block: the same frame bit for bit
    monkeypatch.setattr(spVIPES, "_SILHOUETTE_TABLE_BYTES", 37 * 10 * 8)   # a dozen cells per block: a row of 2 x 5 segments in the table and in two chunks' slabs
    _same(frame, model.latent_silhouette(gi, batch_size=BS))
    monkeypatch.undo()

    # integration_scores: the three attrs of one latent_silhouette call
    sc = model.integration_scores(gi, batch_size=BS)
    assert sorted(sc) == ["group_asw", "label_asw", "per_label"]
    assert sc["label_asw"] == frame.attrs["label_asw"] and sc["group_asw"] == frame.attrs["group_asw"] and sc["per_label"].equals(frame.attrs["per_label"])

    # one group: its rows, NaN group columns; the private space within a group
    for g in (0, 1):
        one = model.latent_silhouette(gi, cells=g, batch_size=BS)
        assert list(one.index) == gi[g] and np.isnan(one["silhouette_group"]).all() and np.isnan(one.attrs["group_asw"])
        _hold(one, zm[g], cell_type[gi[g]], groups[gi[g]], exact=None)   # the fused cells of a plan lie in the other group: either way
    zp = model._latents_on_device(gi, latent="private", batch_size=BS)[0].cpu().numpy()
    priv = model.latent_silhouette(gi, cells=0, latent="private", batch_size=BS)
    assert zp.shape[1] == 5
    _hold(priv, zp, cell_type[gi[0]], groups[gi[0]], exact=True)

    # sampled latents under _noise: the rows of get_latent_representation
    host = model.get_latent_representation(gi, batch_size=BS, _noise=nf)["shared"]
    sampled = model.latent_silhouette(gi, give_mean=False, batch_size=BS, _noise=nf)
    _hold(sampled, np.concatenate([host[0], host[1]]), cell_type, groups, exact=None)
    assert not np.array_equal(sampled["silhouette_label"].to_numpy(), frame["silhouette_label"].to_numpy())

    # labels as an array: a singleton label, and a label made to live in one group
    lab = np.array([f"t{c}" for c in cell_type], dtype=object)
    lab[3] = "lonely"
    lab[(cell_type == 2) & (groups == 1)] = "t2b"
    by_array = model.latent_silhouette(gi, labels=lab, batch_size=BS)
    _hold(by_array, Xm, lab, groups, exact=False)
    assert by_array["silhouette_label"].iloc[3] == 0 and np.isnan(by_array["a"].iloc[3]) and np.isnan(by_array["silhouette_group"].iloc[3])
    assert np.isnan(by_array["silhouette_group"][(lab == "t2b") | (lab == "t2")]).all()
    assert model.module.training

    # names, and the refusals that need the model
    ad.obs_names = np.array([f"cell{i}" for i in range(ad.n_obs)])
    named = model.latent_silhouette(gi, batch_size=BS)
    assert list(named.index) == [f"cell{i}" for i in gi[0] + gi[1]] and named["a"].tolist() == frame["a"].tolist()
    with pytest.raises(ValueError, match="128"):
        model.latent_silhouette(gi, labels=np.arange(n[0] + n[1]), batch_size=BS)
    with pytest.raises(ValueError):
        model.latent_silhouette(gi, labels=np.zeros(3))
    with pytest.raises(KeyError):
        model.latent_silhouette(gi, labels="no_such_column")
    bad = {g: torch.as_tensor(zm[g], device=dev).clone() for g in range(2)}
    bad[1][7, 2] = float("nan")
    monkeypatch.setattr(model, "_latents_on_device", lambda *a, **k: bad)
    with pytest.raises(ValueError, match="non-finite"):
        model.latent_silhouette(gi, batch_size=BS)
