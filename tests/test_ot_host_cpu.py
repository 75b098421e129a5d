"""CPU: the host side of the transport-plan feature -- the reference of tests/_ot_reference.py against rational arithmetic and against
itself on lattice data, tools/ot_host_check.py at its small shapes, ``data.plan_union_csr`` (the union of two top-k passes as CSR),
the closed-form mean cost against a full matrix, and the argument refusals of ``compute_transport_plan`` / ``sinkhorn`` /
``transport_plan`` that come ahead of any device work.  No GPU calls."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests._knn_reference import exact_d2, round_fraction_f32
from tests._ot_reference import lse_ref, sinkhorn_ref, t_from_cost, t_ref, topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_t_is_one_rounding_of_the_exact_value():
    """-c * s + h in rational arithmetic, rounded once, for a few hundred pairs at several scales (t <= 0 here: h <= 0, and |t| is rounded)"""
    rng = np.random.default_rng(0)
    for D, s, scale in ((3, 0.37, 1.0), (25, 0.2, 1.0), (10, 7.3, 1e-3), (5, 1e-4, 100.0)):
        X, Y = (rng.standard_normal((9, D)) * scale).astype(np.float32), (rng.standard_normal((11, D)) * scale).astype(np.float32)
        h = -np.abs(rng.standard_normal(11)).astype(np.float32)
        c, t = exact_d2(X, Y), t_ref(X, Y, h, s)
        for i in range(9):
            for j in range(11):
                exact = Fraction(float(c[i, j])) * Fraction(float(np.float32(s))) - Fraction(float(h[j]))
                assert np.float32(-round_fraction_f32(exact)).view(np.uint32) == t[i, j].view(np.uint32)


def test_reference_on_lattice_data_and_edge_values():
    rng = np.random.default_rng(1)
    X, Y = (rng.integers(-8, 9, (n, 5)).astype(np.float32) / 4 for n in (7, 60))
    h = rng.integers(-6, 7, 60).astype(np.float32) / 2
    t = t_ref(X, Y, h, 0.5)
    plain = (-0.5 * ((X[:, None, :] - Y[None]) ** 2).sum(-1, dtype=np.float32) + h[None]).astype(np.float32)   # every operation exact
    np.testing.assert_array_equal(t, plain)
    idx, tv = topk_ref(t, 12)
    for i in range(7):
        pairs = sorted((-plain[i, j], j) for j in range(60))[:12]
        assert [j for _, j in pairs] == idx[i].tolist() and [-v for v, _ in pairs] == tv[i].tolist()
    assert (np.diff(tv, axis=1) == 0).any()   # ties are there
    np.testing.assert_allclose(lse_ref(t), np.log(np.exp(plain.astype(np.float64)).sum(1)), rtol=1e-14)
    h2 = h.copy()
    h2[[0, 3]], h2[5], h2[6] = -np.inf, np.nan, np.inf
    Y2 = Y.copy()
    Y2[8, :] = 3e19
    t2 = t_ref(X, Y2, h2, 0.5)
    assert np.isneginf(t2[:, [0, 3, 8]]).all() and np.isnan(t2[:, 5]).all() and np.isposinf(t2[:, 6]).all()
    idx2, _ = topk_ref(t2, 60)
    assert not np.isin(idx2, [0, 3, 5, 6, 8]).any() and (idx2[:, 55:] == -1).all() and (idx2[:, :55] >= 0).all()
    keep = np.setdiff1d(np.arange(60), [0, 3, 5, 6, 8])
    np.testing.assert_allclose(lse_ref(t2), lse_ref(t[:, keep]), rtol=1e-14)
    assert np.isneginf(lse_ref(t_ref(X, Y, np.full(60, -np.inf, np.float32), 0.5))).all() and np.isneginf(lse_ref(t_ref(X, Y[:0], h[:0], 0.5))).all()


def test_float64_sinkhorn_meets_its_marginals():
    """the reference iteration itself: after convergence the plan's marginals are a and b (zeros included)"""
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((30, 4)).astype(np.float32), rng.standard_normal((20, 4)).astype(np.float32)
    a, b = rng.random(30) + 0.1, rng.random(20) + 0.1
    a[3], b[[0, 7]] = 0.0, 0.0
    a, b = a / a.sum(), b / b.sum()
    with np.errstate(divide="ignore"):
        log_a, log_b = np.log(a), np.log(b)
    c = exact_d2(X, Y)
    phi, psi = sinkhorn_ref(c, 0.5, log_a, log_b, 400)
    with np.errstate(invalid="ignore"):
        P = np.exp((phi + log_a)[:, None] + (psi + log_b)[None, :] - 0.5 * c.astype(np.float64))
    np.testing.assert_allclose(P.sum(1), a, atol=1e-12)
    np.testing.assert_allclose(P.sum(0), b, atol=1e-12)


def test_host_check_tool_small_shapes():
    """the kernels' own t, online update, merge, key and selection, compiled for the CPU, against the reference (no sanitizer here)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ot_host_check.py"), "--small"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all within bounds" in r.stdout and "DIFFER" not in r.stdout


def test_the_core_text_is_marked_and_states_the_n_split_contract():
    text = open(os.path.join(ROOT, "spvipes_amd", "csrc", "spv_ot.h")).read()
    core = text[text.index("// ---- OT-CORE-BEGIN ----"):text.index("// ---- OT-CORE-END ----")]
    for name in ("ot_update", "ot_merge", "ot_key", "ot_t(", "OT_EMPTY"):
        assert name in core
    assert "atomic" not in core and "not bit for bit" in text


def test_plan_union_csr():
    from spvipes_amd.data import plan_union_csr
    # 3 x 4 plan, k = 2; (0, 1) and (2, 3) are kept by both passes, with different values: the row pass's stay
    idx_r = np.array([[1, 0], [2, -1], [3, 0]], np.int32)
    val_r = np.array([[.5, .25], [.125, 0], [.75, .0625]], np.float32)
    idx_c = np.array([[1, -1], [0, 1], [-1, -1], [2, 1]], np.int32)   # per column j: rows i
    val_c = np.array([[.3, 0], [.51, .2], [0, 0], [.76, .1]], np.float32)
    indptr, indices, data = plan_union_csr(idx_r, val_r, idx_c, val_c, 3, 4)
    dense = np.zeros((3, 4), np.float32)
    for j in range(4):
        for s in range(2):
            if idx_c[j, s] >= 0:
                dense[idx_c[j, s], j] = val_c[j, s]
    for i in range(3):
        for s in range(2):
            if idx_r[i, s] >= 0:
                dense[i, idx_r[i, s]] = val_r[i, s]
    import scipy.sparse as sp
    M = sp.csr_matrix((data, indices, indptr), shape=(3, 4))
    assert M.has_sorted_indices and indptr.tolist() == [0, 2, 6, 8] and indices.dtype == np.int32 and data.dtype == np.float32
    np.testing.assert_array_equal(M.toarray(), dense)
    assert dense[0, 1] == np.float32(.5) and dense[2, 3] == np.float32(.75)   # not the column pass's .51 / .76
    # random lists against a dictionary
    rng = np.random.default_rng(3)
    n0, n1, k = 37, 23, 5
    ir = np.stack([rng.permutation(n1)[:k] for _ in range(n0)]).astype(np.int32)
    ic = np.stack([rng.permutation(n0)[:k] for _ in range(n1)]).astype(np.int32)
    ir[rng.random(ir.shape) < 0.2], ic[rng.random(ic.shape) < 0.2] = -1, -1
    vr, vc = rng.random(ir.shape).astype(np.float32), rng.random(ic.shape).astype(np.float32)
    indptr, indices, data = plan_union_csr(ir, vr, ic, vc, n0, n1)
    want = {(int(ic[j, s]), j): vc[j, s] for j in range(n1) for s in range(k) if ic[j, s] >= 0}
    in_cols = dict(want)
    want.update({(i, int(ir[i, s])): vr[i, s] for i in range(n0) for s in range(k) if ir[i, s] >= 0})
    keys = sorted(want)
    rows = np.repeat(np.arange(n0), np.diff(indptr))
    assert list(zip(rows.tolist(), indices.tolist())) == keys and data.tolist() == [want[key] for key in keys]
    in_rows = {(i, int(ir[i, s])) for i in range(n0) for s in range(k) if ir[i, s] >= 0}
    assert any(key in in_rows and key in in_cols and want[key] != in_cols[key] for key in keys)   # pairs in both passes are there
    # nothing kept at all; shapes that do not fit
    indptr, indices, data = plan_union_csr(np.full((2, 3), -1), np.zeros((2, 3)), np.full((4, 3), -1), np.zeros((4, 3)), 2, 4)
    assert indptr.tolist() == [0, 0, 0] and indices.size == data.size == 0
    for bad in (lambda: plan_union_csr(ir, vr, ic, vc, n0 + 1, n1), lambda: plan_union_csr(ir, vr[:, :2], ic, vc, n0, n1),
                lambda: plan_union_csr(ir, vr, ic, vc[:3], n0, n1), lambda: plan_union_csr(np.where(ir >= 0, ir + n1, ir), vr, ic, vc, n0, n1),
                lambda: plan_union_csr(ir, vr, ic - 1, vc, n0, n1)):
        with pytest.raises(ValueError):
            bad()


def test_closed_form_mean_cost_equals_the_full_matrix():
    from spvipes_amd.ot_ops import mean_sq_cost
    rng = np.random.default_rng(4)
    for n0, n1, D, shift in ((50, 31, 3, 0.0), (200, 333, 25, 5.0), (1, 1, 64, 1.0), (17, 400, 10, -30.0)):
        X, Y = rng.standard_normal((n0, D)).astype(np.float32), (rng.standard_normal((n1, D)) + shift).astype(np.float32)
        full = ((X.astype(np.float64)[:, None, :] - Y.astype(np.float64)[None]) ** 2).sum(-1).mean()
        assert abs(mean_sq_cost(torch.from_numpy(X), torch.from_numpy(Y)) - full) <= 1e-11 * max(full, (X.astype(np.float64) ** 2).sum(1).mean())


def test_check_transport_args():
    from spvipes_amd.data import check_transport_args
    rep = np.arange(60, dtype=np.float64).reshape(12, 5)
    obs = [np.array([0, 2, 4, 6, 8, 10, 11]), np.array([1, 3, 5, 7, 9])]
    X0, X1, k = check_transport_args(rep, obs, np.int64(3))
    assert X0.dtype == X1.dtype == np.float32 and X0.flags.c_contiguous and X0.shape == (7, 5) and X1.shape == (5, 5) and k == 3 and type(k) is int
    np.testing.assert_array_equal(X1, rep[obs[1]].astype(np.float32))
    bad_rep = rep.copy()
    bad_rep[3, 2] = np.nan
    for kw, text in ((dict(k=0), "k must"), (dict(k=65), "k must"), (dict(k=2.0), "k must"), (dict(k=True), "k must"), (dict(rep=rep[:, 0]), "n_obs, D"),
                     (dict(rep=np.zeros((12, 65))), "columns"), (dict(rep=np.zeros((12, 0))), "columns"), (dict(rep=bad_rep), "non-finite"),
                     (dict(obs_idx=obs + [np.array([0])]), "two groups"), (dict(obs_idx=[obs[0], np.array([], int)]), "non-empty"),
                     (dict(obs_idx=[obs[0], np.array([12])]), "inside"), (dict(rep=np.array([["a"] * 5] * 12)), "numeric")):
        with pytest.raises(ValueError, match=text):
            check_transport_args(**dict(dict(rep=rep, obs_idx=obs, k=4), **kw))


class _Duck:
    def __init__(self, n=12, with_obsm=True):
        self.n_obs, self.obs = n, {}
        self.uns = {"groups_obs_indices": [np.arange(0, n, 2), np.arange(1, n, 2)]}
        if with_obsm:
            self.obsm = {"X_pca": np.zeros((n, 5), np.float32)}


def test_compute_transport_plan_refuses_before_any_device_work():
    """each of these returns from an argument check: nothing is written to the AnnData and no device is asked for"""
    from spvipes_amd.model import spVIPES
    for ad, kw, exc, text in ((_Duck(), dict(use_rep="X_umap"), KeyError, "X_umap"), (_Duck(with_obsm=False), dict(use_rep="X_pca"), KeyError, "X_pca"),
                              (_Duck(), dict(use_rep="X_pca", k=0), ValueError, "k must"), (_Duck(), dict(use_rep="X_pca", k=65), ValueError, "k must"),
                              (_Duck(), dict(use_rep=np.zeros((11, 5))), ValueError, "one row per cell"), (_Duck(), dict(use_rep=np.zeros((12, 65))), ValueError, "columns"),
                              (_Duck(), dict(use_rep=np.zeros(12)), ValueError, "n_obs, D")):
        with pytest.raises(exc, match=text):
            spVIPES.compute_transport_plan(ad, **kw)
        assert "transport_plan" not in ad.uns and "indices" not in ad.obs
    ad = _Duck()
    del ad.uns["groups_obs_indices"]
    with pytest.raises(ValueError, match="groups_obs_indices"):
        spVIPES.compute_transport_plan(ad, "X_pca")


def test_signatures():
    import inspect
    from spvipes_amd.model import spVIPES
    from spvipes_amd.ot_ops import ot_softmin, ot_topk, sinkhorn, transport_plan
    p = inspect.signature(spVIPES.compute_transport_plan).parameters
    assert list(p) == ["adata", "use_rep", "k", "key_added", "device", "sinkhorn_kwargs"] and (p["k"].default, p["key_added"].default, p["device"].default) == (32, "transport_plan", None)
    assert list(inspect.signature(ot_softmin).parameters) == ["X", "Y", "h", "inv_eps", "n_split", "out"]
    assert list(inspect.signature(ot_topk).parameters) == ["X", "Y", "h", "r", "inv_eps", "k", "n_split", "out"]
    p = inspect.signature(sinkhorn).parameters
    assert list(p) == ["X0", "X1", "epsilon", "scale_cost", "a", "b", "max_iter", "tol", "check_every"]
    assert [p[n].default for n in list(p)[2:]] == [0.05, "mean", None, None, 2000, 1e-3, 10]
    p = inspect.signature(transport_plan).parameters
    assert list(p) == ["X0", "X1", "k", "sinkhorn_kwargs"] and p["k"].default == 32


def test_op_checks_refuse_host_tensors():
    """the ops' own checks come first: a host tensor is refused before the library is asked for anything"""
    from spvipes_amd import _abi
    from spvipes_amd.ot_ops import ot_softmin, ot_topk, sinkhorn, transport_plan
    X, Y, h = torch.zeros((4, 5)), torch.zeros((9, 5)), torch.zeros(9)
    for bad in (lambda: ot_softmin(X, Y, h, 1.0), lambda: ot_topk(X, Y, h, torch.zeros(4), 1.0, 2), lambda: sinkhorn(X, Y), lambda: transport_plan(X, Y, k=2)):
        with pytest.raises(_abi.SpvError):
            bad()
    with pytest.raises(ValueError, match="k must"):
        transport_plan(X, Y, k=0)
