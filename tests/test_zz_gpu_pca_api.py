"""GPU: ``count_pca`` (joint and ``group=0``) and ``spVIPES.pca`` on a duck-typed AnnData with dense and sparse ``X``, at 333 + 270
cells and 200 / 230 genes of which 160 pair, ``n_comps=5``, against the fp64 reference of tests/_pca_reference.py (the operand with
np.log1p in fp64, the covariance, eigh).  The reference's gap lambda_5 - lambda_6 >= 0.1 lambda_1 is asserted here, so the input
cannot drift.

Bounds.  Eigenvalues: (tol + s) lambda_1 with s the operator's slack, || Z_kernel - Z_fp64 ||_2 / || Z_fp64 ||_2 on this input with a
4 x margin, capped at 9 tol.  Measured: 1.012e-7 (the fp32 log1p, centring and the fp32 sums of 603 rows), so s = 4.05e-7 and the bound is
1.00405e-4 lambda_1.  Subspace: every component lies within residual_i / (0.1 lambda_1 (n - 1)) of the reference's top-5 subspace
(Davis-Kahan with the asserted gap).  Scores: the project bound (K + 2) 2^-24 sum |x||v| of tests/test_zz_gpu_pca.py with K = the genes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import _pca_reference as R  # noqa: E402

TOL = 1e-4
SLACK = 4.05e-7       # 4 x the measured || Z_kernel - Z_fp64 ||_2 / || Z_fp64 ||_2 = 1.012e-7 of this input; capped at 9 * TOL


@pytest.fixture(scope="module")
def planted():
    ad, blocks, uni = R.make_pca_duck(0)
    ref = R.reference_joint(blocks, uni)
    lam = ref["lam"]
    assert lam[4] - lam[5] >= 0.1 * lam[0]
    return ad, blocks, uni, ref


@pytest.fixture(scope="module")
def model(planted):
    from spvipes_amd.model import spVIPES
    ad = planted[0]
    spVIPES.setup_anndata(ad, groups_key="groups")
    return spVIPES(ad, n_hidden=32, n_dimensions_shared=5, n_dimensions_private=3)


@pytest.fixture(scope="module")
def joint(model, planted):
    ad = planted[0]
    return model.count_pca(ad.uns["groups_obs_indices"], n_comps=5)


def _check(res, ref, n_comps=5):
    lam, n = ref["lam"], ref["n"]
    slack = min(SLACK, 9 * TOL)
    assert res.converged and res.n_restarts == 0 and 1 <= res.n_blocks <= 12
    theta1 = res.variance[0] * (n - 1)
    print("residuals / theta_1:", res.residuals / theta1, "blocks:", res.n_blocks)
    assert res.residuals.shape == (n_comps,) and (res.residuals <= TOL * theta1).all()
    print("eigenvalue error / lambda_1:", np.abs(res.variance - lam[:n_comps]) / lam[0])
    assert (np.abs(res.variance - lam[:n_comps]) <= (TOL + slack) * lam[0]).all()
    assert (np.diff(res.variance) <= 0).all()
    # the subspace: Davis-Kahan with the asserted gap
    comp = res.components
    assert comp.shape == (n_comps, ref["X"].shape[1]) and comp.dtype == np.float64
    unit = comp / np.linalg.norm(comp, axis=1, keepdims=True)
    out = unit.T - ref["top"] @ (ref["top"].T @ unit.T)
    assert (np.linalg.norm(out, axis=0) <= res.residuals / (0.1 * lam[0] * (n - 1))).all()
    # the sign rule: the largest |loading| is positive
    lead = comp[np.arange(n_comps), np.argmax(np.abs(comp), axis=1)]
    assert (lead > 0).all()
    # the scores: X_ref . components within the project bound
    X = ref["X"]
    want = X @ comp.T
    K = X.shape[1]
    bound = (K + 2) * 2.0 ** -24 * (np.abs(X) @ np.abs(comp.T))
    assert res.scores.shape == want.shape and res.scores.dtype == np.float32
    assert (np.abs(res.scores - want) <= bound).all(), f"scores: worst {np.max(np.abs(res.scores - want) / bound):.3f} of the bound"
    # the ratio: below 1 in sum, and the reference's within the eigenvalue bound
    assert res.variance_ratio.sum() < 1.0
    assert (np.abs(res.variance_ratio - lam[:n_comps] / ref["total"]) <= (TOL + slack) * lam[0] / ref["total"] * (1 + 1e-6)).all()
    assert np.allclose(res.mean, ref["mean"], rtol=0, atol=1e-6) and np.allclose(res.var, ref["var"], rtol=1e-5, atol=1e-9)


def test_operator_slack_against_an_fp64_operator(model, planted):
    """|| Z_kernel - Z_fp64 ||_2 / || Z_fp64 ||_2 on this input: what SLACK is 4 x of"""
    from spvipes_amd.pca_ops import PcaGroup, PcaOperator
    ad, blocks, uni, ref = planted
    pos = R.paired_positions(uni)
    dev = model.device
    mean32 = ref["mean"].astype(np.float32)
    parts = []
    for g in range(2):
        G = R.N_GENES[g]
        mu, sc = np.zeros(G, np.float32), np.zeros(G, np.float32)
        mu[pos[g]], sc[pos[g]] = mean32, 1.0
        rows = torch.arange(R.N_CELLS[g], dtype=torch.int32, device=dev)
        parts.append(PcaGroup(model.counts[g], rows, torch.from_numpy(R.weights(blocks[g])).to(dev), torch.from_numpy(mu).to(dev), torch.from_numpy(sc).to(dev),
                              torch.from_numpy(pos[g].astype(np.int64)).to(dev)))
    op = PcaOperator(parts)
    V = np.linalg.qr(np.random.default_rng(3).standard_normal((160, 16)))[0].astype(np.float32)
    Z, Y = op.apply(torch.from_numpy(V).to(dev))
    Z2, Y2 = op.apply(torch.from_numpy(V).to(dev))
    assert torch.equal(Z, Z2) and torch.equal(Y, Y2)                      # the kernels' outputs repeat bit for bit
    want = ref["X"].T @ (ref["X"] @ V.astype(np.float64))
    slack = np.linalg.norm(Z.cpu().numpy() - want, 2) / np.linalg.norm(want, 2)
    print(f"operator slack {slack:.3e}")
    assert 4 * slack <= SLACK <= 9 * TOL


def test_count_pca_joint(joint, planted):
    ad, _blocks, uni, ref = planted
    _check(joint, ref)
    assert np.array_equal(joint.obs, np.concatenate(ad.uns["groups_obs_indices"]))
    pos = R.paired_positions(uni)
    assert list(joint.genes[0]) == [f"a_g{uni[0][i]}" for i in pos[0]] and list(joint.genes[1]) == [f"b_g{uni[1][i]}" for i in pos[1]]


def test_count_pca_one_group_and_a_cell_subset(model, planted):
    ad, blocks, _uni, _ref = planted
    keep = np.arange(0, 300, 2)                                           # every other cell of the first 300
    cells = ad.uns["groups_obs_indices"][0][keep]
    ref = R.reference_pca([R.lognorm(blocks[0][keep], R.weights(blocks[0][keep]))], 5)
    assert ref["lam"][4] - ref["lam"][5] >= 0.1 * ref["lam"][0]
    res = model.count_pca([cells, []], n_comps=5, group=0)
    _check(res, ref)
    assert np.array_equal(res.obs, cells) and len(res.genes) == 1 and len(res.genes[0]) == 200


def test_count_pca_scaled(model, planted):
    ad, blocks, uni, _ref = planted
    ref = R.reference_joint(blocks, uni, scale=True)
    assert ref["lam"][4] - ref["lam"][5] >= 0.1 * ref["lam"][0]
    res = model.count_pca(ad.uns["groups_obs_indices"], n_comps=5, scale=True)
    lam, n = ref["lam"], ref["n"]
    assert res.converged and (res.residuals <= TOL * res.variance[0] * (n - 1)).all()
    # the scale is rounded to fp32 (2^-24 relative per gene, twice in X^T X): within the eigenvalue bound all the same
    assert (np.abs(res.variance - lam[:5]) <= (TOL + min(SLACK, 9 * TOL)) * lam[0]).all()
    assert abs(res.variance_ratio.sum() * ref["total"] - lam[:5].sum()) <= 5 * (TOL + SLACK) * lam[0]


@pytest.fixture(scope="module")
def class_runs(planted):
    """spVIPES.pca on the same data with a dense and with a scipy.sparse ``X`` -> {sparse: (adata, result)}, run once"""
    from spvipes_amd.model import spVIPES
    runs = {}
    for sparse in (False, True):
        ad, _b, _u = R.make_pca_duck(0, sparse=sparse)
        runs[sparse] = (ad, spVIPES.pca(ad, n_comps=5))
    return runs


@pytest.mark.parametrize("sparse", [False, True], ids=["dense-X", "sparse-X"])
def test_pca_classmethod_writes_obsm_in_adata_order(class_runs, planted, sparse):
    _ad, _blocks, _uni, ref = planted
    ad, res = class_runs[sparse]
    _check(res, ref)
    out = ad.obsm["X_pca"]
    assert out.shape == (603, 5) and out.dtype == np.float32
    assert np.array_equal(out[res.obs], res.scores) and np.array_equal(res.obs, np.concatenate(ad.uns["groups_obs_indices"]))
    assert set(ad.uns["pca"]) == {"variance", "variance_ratio", "params"} and ad.uns["pca"]["params"]["n_comps"] == 5
    assert np.array_equal(ad.uns["pca"]["variance"], res.variance)


def _vector_bound(res, ref):
    """|| v_i - u_i || of a run's component i against the reference's eigenvector u_i: sqrt 2 sin(angle), sin <= (the residual
    against the fp64 operator) / (the distance of lambda_i to the rest of the spectrum), Davis-Kahan for one vector; the residual
    against the fp64 operator is the reported one plus the operator's slack; the component's norm is 1 within fp32 rounding"""
    lam, n = ref["lam"], ref["n"]
    theta1 = lam[0] * (n - 1)
    out = []
    for i in range(5):
        near = min(lam[i - 1] - lam[i] if i else np.inf, lam[i] - lam[i + 1])
        delta = (near - 2 * TOL * lam[0]) * (n - 1)          # (the Ritz value itself may be off by the eigenvalue bound)
        out.append(np.sqrt(2.0) * (res.residuals[i] + SLACK * theta1) / delta + 2.0 ** -22)
    return np.asarray(out)


def test_dense_and_sparse_X_and_the_model_give_the_same_scores_within_the_certificate(class_runs, joint, planted):
    """the scores of two runs differ by X (v_a - v_b) plus the two project errors; the certificate bounds || v_a - v_b || through the
    reference's eigenvector (the sign rule fixes the sign), the spectrum's inner gaps are the reference's own"""
    _ad, _blocks, _uni, ref = planted
    X = ref["X"]
    rows = np.linalg.norm(X, axis=1)
    runs = [("dense X", class_runs[False][1]), ("sparse X", class_runs[True][1]), ("the model's counts", joint)]
    for (na, a), (nb, b) in ((runs[0], runs[1]), (runs[0], runs[2]), (runs[1], runs[2])):
        assert np.array_equal(a.obs, b.obs)
        dv = _vector_bound(a, ref) + _vector_bound(b, ref)
        got_dv = np.linalg.norm(a.components - b.components, axis=1)
        print(f"{na} / {nb}: || v_a - v_b || {got_dv} of {dv}")
        assert (got_dv <= dv).all()
        project = (X.shape[1] + 2) * 2.0 ** -24 * (np.abs(X) @ (np.abs(a.components.T) + np.abs(b.components.T)))
        bound = rows[:, None] * dv[None, :] + project
        diff = np.abs(a.scores.astype(np.float64) - b.scores.astype(np.float64))
        assert (diff <= bound).all(), f"{na} / {nb}: scores differ by up to {np.max(diff / bound):.3f} of the bound"
        assert np.max(np.abs(a.variance - b.variance)) <= 2 * (TOL + SLACK) * ref["lam"][0]


def test_kernel_outputs_of_dense_and_sparse_storage_agree_bit_for_bit(planted):
    """bit equality is asserted of the KERNEL outputs only, not of the torch algebra around them"""
    from spvipes_amd.data import resident_group_counts
    from spvipes_amd.pca_ops import PcaGroup, PcaOperator, stage_block
    ad, _blocks, uni, _ref = planted
    dev = torch.device("cuda:0")
    pos = R.paired_positions(uni)
    var_idx, obs_idx = ad.uns["groups_var_indices"], ad.uns["groups_obs_indices"]
    outs = []
    for storage in ("dense", "sparse"):
        counts = resident_group_counts(ad.X, obs_idx, var_idx, dev, storage)
        parts, staged = [], []
        for g in range(2):
            G = R.N_GENES[g]
            rows = torch.arange(R.N_CELLS[g], dtype=torch.int32, device=dev)
            sc = torch.zeros(G, dtype=torch.float32, device=dev)
            sc[torch.from_numpy(pos[g]).to(dev)] = 1.0
            staged.append(torch.cat([b.clone() for _p0, b in stage_block(counts[g], rows)]))
            parts.append(PcaGroup(counts[g], rows, None, torch.full((G,), 0.25, dtype=torch.float32, device=dev), sc, torch.from_numpy(pos[g].astype(np.int64)).to(dev)))
        V = torch.from_numpy(np.random.default_rng(1).standard_normal((160, 32)).astype(np.float32)).to(dev)
        outs.append((PcaOperator(parts).apply(V), staged))
    (Zd, Yd), md = outs[0]
    (Zs, Ys), ms = outs[1]
    assert torch.equal(Zd, Zs) and torch.equal(Yd, Ys)
    for g in range(2):
        assert torch.equal(md[g], ms[g])
