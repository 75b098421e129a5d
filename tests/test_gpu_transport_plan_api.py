"""GPU: spVIPES.compute_transport_plan on the duck AnnData (300 / 260 cells, an ``obsm`` attribute added here) and the paired-PoE model
built from what it writes: the plan goes to the module sparse, as it is, and a model built from the dense ``.toarray()`` of it holds
the same plan and computes the same bits.  Every test here needs the feature and fails without it."""
import numpy as np
import pytest
import torch

from tests.test_gpu_posterior_predictive import _noise_fn

pytestmark = pytest.mark.gpu

K, SINKHORN = 8, dict(epsilon=0.1, max_iter=20, tol=0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _adata(with_indices=True):
    """the duck with a common 10-dimensional representation of both groups' cells around 4 centres, in ``obsm``"""
    from tests._duck import make_duck
    ad = make_duck(seed=2)
    rng = np.random.default_rng(5)
    centres = 3.0 * rng.standard_normal((4, 10))
    ad.obsm = {"X_rep": (centres[rng.integers(0, 4, ad.n_obs)] + rng.standard_normal((ad.n_obs, 10))).astype(np.float32)}
    if not with_indices:
        del ad.obs["indices"]
    return ad


@pytest.fixture(scope="module")
def planned(dev):
    from spvipes_amd.model import spVIPES
    ad = _adata(with_indices=False)
    return ad, spVIPES.compute_transport_plan(ad, "X_rep", k=K, **SINKHORN)


def test_compute_transport_plan_writes_uns_and_obs(dev, planned):
    import scipy.sparse as sp
    from spvipes_amd.model import spVIPES
    from spvipes_amd.ot_ops import transport_plan
    ad, res = planned
    n0, n1 = (len(v) for v in ad.uns["groups_obs_indices"])
    M = ad.uns["transport_plan"]
    assert sp.issparse(M) and M.format == "csr" and M.shape == (n0, n1) and M.dtype == np.float32 and M.has_sorted_indices
    assert (M != res.to_scipy()).nnz == 0 and res.k == K and res.sinkhorn.n_iter == 20
    # every cell keeps at least its own K entries and at most K more per cell that chose it; the values are probabilities
    per_row, per_col = np.diff(M.indptr), np.diff(M.tocsc().indptr)
    assert (per_row >= K).all() and (per_col >= K).all() and M.nnz <= K * (n0 + n1) and (M.data >= 0).all() and M.sum() <= 1 + 1e-4
    # (an iteration ends on the column update: the untruncated plan's column sums ARE b, so a column cannot keep more than all of it)
    assert res.row_kept.shape == (n0,) and res.col_kept.shape == (n1,) and (res.row_kept > 0).all() and (res.col_kept > 0).all() and (res.col_kept <= 1 + 1e-4).all()
    # obs["indices"], absent before: every cell's position within its group
    want = np.concatenate([np.arange(n0), np.arange(n1)])
    np.testing.assert_array_equal(ad.obs["indices"], want)
    assert _adata().obs["indices"].tolist() == want.tolist()   # what the duck carries by default
    # the same plan straight from the op on the two groups' rows
    X = [torch.from_numpy(np.ascontiguousarray(ad.obsm["X_rep"][ad.uns["groups_obs_indices"][g]])).to(dev) for g in range(2)]
    direct = transport_plan(X[0], X[1], k=K, **SINKHORN)
    for a, b in ((direct.indptr, res.indptr), (direct.indices, res.indices), (direct.data.view(np.uint32), res.data.view(np.uint32))):
        np.testing.assert_array_equal(a, b)
    # an array instead of a key, another key to write to, an existing obs["indices"] left alone; repeatable bit for bit
    ad2 = _adata()
    ad2.obs["indices"] = ad2.obs["indices"][::-1].copy()
    kept = ad2.obs["indices"].copy()
    res2 = spVIPES.compute_transport_plan(ad2, ad2.obsm["X_rep"].astype(np.float64), k=K, key_added="ot", device="cuda:0", **SINKHORN)
    assert "transport_plan" not in ad2.uns and (ad2.uns["ot"] != M).nnz == 0
    np.testing.assert_array_equal(ad2.obs["indices"], kept)
    np.testing.assert_array_equal(res2.data.view(np.uint32), res.data.view(np.uint32))
    assert torch.equal(res2.sinkhorn.phi, res.sinkhorn.phi) and torch.equal(res2.sinkhorn.psi, res.sinkhorn.psi)


def _model(ad, precision="fp32"):
    from spvipes_amd.model import spVIPES
    spVIPES.setup_anndata(ad, groups_key="groups", transport_plan_key="transport_plan")
    torch.manual_seed(0)
    return spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=precision)


def test_paired_model_from_the_sparse_plan_equals_the_one_from_the_dense_plan(dev, planned):
    from spvipes_amd.plan import SparsePlan
    ad, res = planned
    sparse_model = _model(ad)
    assert sparse_model.module.transport_plan is ad.uns["transport_plan"]   # handed over as it is: nothing dense was made
    dense_ad = _adata()
    dense_ad.uns["transport_plan"] = ad.uns["transport_plan"].toarray()
    dense_model = _model(dense_ad)
    assert isinstance(dense_model.module.transport_plan, torch.Tensor) and tuple(dense_model.module.transport_plan.shape) == ad.uns["transport_plan"].shape
    sp_s, sp_d = sparse_model.module.sparse_plan(dev), dense_model.module.sparse_plan(dev)
    for name in ("ptr0", "ind0", "val0", "ptr1", "ind1", "val1"):
        assert torch.equal(getattr(sp_s, name), getattr(sp_d, name)), name
    assert sp_s.n0 == sp_d.n0 and sp_s.n1 == sp_d.n1 and int(sp_s.ind0.numel()) == int((res.data > 0).sum())
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    nf = _noise_fn(dev)
    z_s = sparse_model.get_latent_representation(gi, batch_size=40, _noise=nf)
    z_d = dense_model.get_latent_representation(gi, batch_size=40, _noise=nf)
    for key in ("shared", "private"):
        for g in range(2):
            np.testing.assert_array_equal(z_s[key][g].view(np.uint32), z_d[key][g].view(np.uint32))
    # a ready SparsePlan in uns goes through as it is too
    ready_ad = _adata()
    ready_ad.uns["transport_plan"] = res.sparse_plan(dev)
    ready_model = _model(ready_ad)
    assert isinstance(ready_model.module.transport_plan, SparsePlan) and ready_model.module.sparse_plan(dev) is ready_ad.uns["transport_plan"]
    z_r = ready_model.get_latent_representation(gi, batch_size=40, _noise=nf)
    np.testing.assert_array_equal(z_r["shared"][0].view(np.uint32), z_s["shared"][0].view(np.uint32))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_three_training_steps_on_the_computed_plan(dev, planned, precision):
    ad, _ = planned
    model = _model(ad, precision)
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=128, max_epochs=1, train_size=1.0)   # 300 / 260 cells: 3 steps
    losses = [v for key, vals in model.history.items() if "loss" in key or "elbo" in key for v in vals]
    assert model.is_trained_ and losses and np.isfinite(losses).all()
    z = model.get_latent_representation(gi, batch_size=64)
    assert all(np.isfinite(z[key][g]).all() for key in ("shared", "private") for g in range(2))


def test_refusals(dev):
    from spvipes_amd.model import spVIPES
    ad = _adata()
    for kw, exc, text in ((dict(use_rep="X_other"), KeyError, "X_other"), (dict(use_rep="X_rep", k=0), ValueError, "k must"), (dict(use_rep="X_rep", k=65), ValueError, "k must"),
                          (dict(use_rep=np.zeros((ad.n_obs, 65), np.float32)), ValueError, "columns"), (dict(use_rep=np.zeros((ad.n_obs - 1, 10), np.float32)), ValueError, "one row per cell"),
                          (dict(use_rep="X_rep", epsilon=-1.0), ValueError, "epsilon"), (dict(use_rep="X_rep", scale_cost="max"), ValueError, "scale_cost")):
        with pytest.raises(exc, match=text):
            spVIPES.compute_transport_plan(ad, **kw)
        assert "transport_plan" not in ad.uns
    # D mismatch between the two clouds at the op
    from spvipes_amd import _abi
    from spvipes_amd.ot_ops import transport_plan
    with pytest.raises(_abi.SpvError, match="same number of columns"):
        transport_plan(torch.zeros((5, 10), device=dev), torch.zeros((6, 9), device=dev), k=2)
