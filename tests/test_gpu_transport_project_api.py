"""GPU: ``spVIPES.transport_project`` end to end on the duck AnnData of tests/_duck.py with two small, well-separated clouds around the
same 4 centres (260 and 130 cells, D = 25, made as the clouds of tests/test_gpu_ot.py are, with their labels kept): coordinates and
one-hot labels pushed through the untruncated plan onto either group, against float64 on the returned potentials; the label frame,
the ``obsm`` layout, the row mass against the marginal, and more than OT_VAL_MAX columns.  Every test here needs the feature and
fails without it.

The centres hold (80, 60, 70, 50) and (40, 30, 35, 25) cells, the SAME shares in both groups, in shuffled order.  That is what makes
"every cell is given its own centre" a property of the plan and not luck: a balanced plan between uniform marginals has to move
every share that differs between the groups ACROSS centres, however far apart they lie (with centres drawn at random, as in
tests/test_gpu_ot.py, a few cells per hundred are rightly sent elsewhere).

The reference takes h = potential + log marginal of the OTHER group in float32, the one addition the wrapper makes (the bits are
checked against the device's), so t is bit-equal and ``project_bound`` (tests/test_gpu_ot_project.py derives it) holds as it stands:
the rounding of h is part of the reference, not an allowance on top."""
import numpy as np
import pytest
import torch

from tests._ot_project_reference import project_bound, project_ref
from tests._ot_reference import t_ref

pytestmark = pytest.mark.gpu

COUNTS = ((80, 60, 70, 50), (40, 30, 35, 25))
N, D = (sum(COUNTS[0]), sum(COUNTS[1])), 25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _clouds(seed=0):
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((4, D))
    X, lab = [], []
    for counts in COUNTS:
        which = rng.permutation(np.repeat(np.arange(4), counts))
        m = len(which)
        X.append((centres[which] + rng.standard_normal((m, D))).astype(np.float32))
        lab.append(which)
    return X, lab


@pytest.fixture(scope="module")
def world(dev):
    """(adata, plan, per group: X, true centre) -- the plan computed once and left unchanged"""
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    X, lab = _clouds()
    ad = make_duck(n=N, G=(8, 8), seed=3)
    ad.obsm = {"X_rep": np.concatenate(X)}
    ad.obs["blob"] = np.array([f"centre{c}" for c in np.concatenate(lab)])
    plan = spVIPES.compute_transport_plan(ad, "X_rep", k=16, epsilon=0.05, max_iter=500, tol=1e-3)
    assert plan.sinkhorn.converged
    return ad, plan, X, lab


def _reference(plan, X, V, onto):
    """(float64 projection [n_onto, n_v], bound, L float64) from the returned potentials"""
    from spvipes_amd.ot_ops import ot_project_splits
    res = plan.sinkhorn
    pots = [(res.phi.cpu().numpy() + res.log_a.cpu().numpy()), (res.psi.cpu().numpy() + res.log_b.cpu().numpy())]   # float32 additions, as the wrapper makes them
    dev_pots = [(res.phi + res.log_a).cpu().numpy(), (res.psi + res.log_b).cpu().numpy()]
    for a, b in zip(pots, dev_pots):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    t = t_ref(X[onto], X[1 - onto], pots[1 - onto], res.inv_eps)
    want, L = project_ref(t, V)
    n_q, n_c = t.shape
    ns = ot_project_splits(n_q, n_c, min(V.shape[1], 256))
    return want, project_bound(t, V, -(-n_c // ns), ns), L, pots[onto]


@pytest.mark.parametrize("onto", [0, 1])
def test_coordinates_land_in_the_other_groups_space(world, onto):
    from spvipes_amd.model import spVIPES
    ad, plan, X, lab = world
    got = spVIPES.transport_project(ad, "X_rep", plan, "X_rep", onto=onto)
    assert isinstance(got, np.ndarray) and got.shape == (N[onto], D) and got.dtype == np.float32
    want, bound, _, _ = _reference(plan, X, X[1 - onto], onto)
    err = np.abs(got.astype(np.float64) - want)
    print(f"coordinates onto {onto}: max err / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()
    same = spVIPES.transport_project(ad, "X_rep", plan, X[1 - onto], onto=onto)   # the array [n_other, n_v] itself
    np.testing.assert_array_equal(same.view(np.uint32), got.view(np.uint32))
    # each cell's image lies with its own centre's cells in the other group
    centre = np.stack([X[1 - onto][lab[1 - onto] == c].mean(0) for c in range(4)])
    assert (np.argmin(((got[:, None, :] - centre[None]) ** 2).sum(2), 1) == lab[onto]).all()


@pytest.mark.parametrize("onto", [0, 1])
def test_label_transfer_frame_and_obsm(world, onto):
    from spvipes_amd.model import spVIPES
    ad, plan, X, lab = world
    before = set(ad.obsm)
    frame = spVIPES.transport_project(ad, "X_rep", plan, "blob", onto=onto, key_added="blob_probs")
    cats = [f"centre{c}" for c in range(4)]
    rows = ad.uns["groups_obs_indices"][onto]
    assert list(frame.columns) == cats + ["predicted", "confidence"] and list(frame.index) == list(rows)
    hot = (lab[1 - onto][:, None] == np.arange(4)[None]).astype(np.float32)
    want, bound, _, _ = _reference(plan, X, hot, onto)
    probs = frame[cats].to_numpy()
    assert probs.dtype == np.float32 and (np.abs(probs.astype(np.float64) - want) <= bound).all()
    assert list(frame["predicted"]) == [f"centre{c}" for c in lab[onto]], "every cell is given its own centre"
    np.testing.assert_array_equal(frame["confidence"].to_numpy(), probs.max(1))
    np.testing.assert_allclose(probs.astype(np.float64).sum(1), 1.0, atol=4 * bound.sum(1).max())
    full = ad.obsm["blob_probs"]
    assert set(ad.obsm) == before | {"blob_probs"} and full.shape == (ad.n_obs, 4) and full.dtype == np.float32
    np.testing.assert_array_equal(full[rows], probs)
    assert np.isnan(full[ad.uns["groups_obs_indices"][1 - onto]]).all()
    del ad.obsm["blob_probs"]


@pytest.mark.parametrize("side", [0, 1])
def test_row_mass_against_the_marginal(dev, world, side):
    """mass_i = exp(L_i + r_i) is the untruncated plan's row mass: the marginal a_i (b_j) once Sinkhorn has converged to tol.  The
    driver's stopping error is the largest log-deviation of the row marginal one half-step earlier; twice tol covers the half-step
    and the float32 roundings (1e-5 at these shapes)."""
    from spvipes_amd.ot_ops import transport_project
    ad, plan, X, lab = world
    Xd = [torch.from_numpy(x).to(dev) for x in X]
    V = torch.from_numpy(X[1 - side][:, :3].copy()).to(dev)
    out, mass = transport_project(plan.sinkhorn, Xd[side], Xd[1 - side], V, side)
    assert out.shape == (N[side], 3) and mass.shape == (N[side],) and mass.dtype == np.float64
    want, bound, L, r = _reference(plan, X, X[1 - side][:, :3], side)
    assert (np.abs(out.cpu().numpy().astype(np.float64) - want) <= bound).all()
    np.testing.assert_allclose(mass, np.exp(L + r.astype(np.float64)), rtol=1e-4)
    dev_log = np.abs(np.log(mass * N[side]))
    print(f"side {side}: max |log(mass / marginal)| = {dev_log.max():.2e}, tol 1e-3, the driver's last error {plan.sinkhorn.error:.2e}")
    assert (dev_log <= 2e-3).all()
    with pytest.raises(ValueError):
        transport_project(plan.sinkhorn, Xd[side], Xd[1 - side], V, 2)
    with pytest.raises(ValueError):
        transport_project(plan.sinkhorn, Xd[1 - side], Xd[side], V, side)


def test_more_columns_than_one_call_takes(world):
    """300 columns are walked in slices of OT_VAL_MAX on the host: each slice's columns are what a call with that slice alone gives"""
    from spvipes_amd.model import spVIPES
    from spvipes_amd.ot_ops import OT_VAL_MAX
    ad, plan, X, lab = world
    V = np.random.default_rng(9).standard_normal((N[1], 300)).astype(np.float32)
    got = spVIPES.transport_project(ad, "X_rep", plan, V, onto=0)
    assert got.shape == (N[0], 300) and OT_VAL_MAX == 256
    for sl in (slice(0, 256), slice(256, 300)):
        part = spVIPES.transport_project(ad, "X_rep", plan, np.ascontiguousarray(V[:, sl]), onto=0)
        np.testing.assert_array_equal(part.view(np.uint32), got[:, sl].view(np.uint32))
    want, bound, _, _ = _reference(plan, X, V, 0)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
