"""GPU: spv_ot_softmin / spv_ot_topk (spvipes_amd.ot_ops) and the Sinkhorn driver on top of them against the yardstick of
tests/_ot_reference.py.  Shapes are sized by the tiles the library reports (TQ queries per workgroup, TC candidates per LDS tile): one
below, at and one above a tile, several tiles, more than one workgroup, and about 2000 candidates so that the automatic chunk count
exceeds 1.  Every call goes through ``_softmin`` / ``_topk``: odd or 16-byte-multiple row pitches with NaN in the pitch padding (a
kernel that read it would lose the candidate: a NaN t contributes nothing and is never selected) and sentinels in the outputs beyond
[n_q] / [n_q, k], which must come back untouched.  Every test here imports the new module and fails without it.

THE BOUND ON L (``lse_bound``), from the kernel's arithmetic (csrc/spv_ot.h), in units of u = 2^-24 (one float32 rounding, relative):
t is bit-equal to the reference's, so only the reduction errs.  Within a chunk of n candidates a lane keeps (m, S), S standing for
sum_j exp(t_j - m).  A term enters either as the exact 1 of a rescale step or as e = exp(-(m - t)), and is later multiplied by the e of
every rescale step and passes through one addition per later step.  The device's exp(x) is v_exp_f32(x * log2 e): the difference d = t - m
rounds (|d| u in the argument), the product with log2 e rounds (|d| u), log2 e itself is off by at most u / 2 relative (|d| u / 2), and
v_exp_f32 is good to one ulp (2 u relative): a factor e carries at most (2.5 |d| + 2) u.
  * The |d| parts telescope: for term j the d of its entry and of all later rescales add up to y_j = m_final - t_j, so term j carries
    2.5 y_j u from them, and weighted by its share p_j = exp(-y_j) / S of the sum that is 2.5 u sum_j p_j y_j <= 2.5 u ln n (the entropy
    of p, y_j being -ln p_j up to the common ln S >= 0).
  * The constant parts: the entry's 2 u counts once per term, weighted by shares that add up to 1: 2 u in all.  A rescale step
    multiplies everything before it by e (2 u) inside one fma (1 u); any other step is one addition (1 u): at most 3 u per step, 3 n u.
  * n_split > 1: a merge is one fma (1 u) and one e (2 u, its |d| part again inside the telescoped sum): 3 u per chunk; 4 is asserted.
  * L = m + log(S): S >= 1, a relative error of S is an absolute one of log S; logf is good to one ulp, 2 u |log S| <= 2 u ln(n_c); the last
    addition rounds once: u |L|.
Together |L - L_ref| <= (3 n_chain + 4 n_split + 5 ln(n_c + 1) + 16) u + 2 u max(|L_ref|, 1) with n_chain the candidates of a chunk; the 16 u
and the second u of the last term are the slack for the second-order terms and for the float64 reference's own error.  (The issue
proposed 2 n_chain + 2 n_split + 16: it counted the fma of a rescale step and left out the ulp of the exp inside it.  The derivation
wins; nothing here was fitted to the kernel's output.)

THE BOUND ON val: val = expf(fl(t + r)).  The addition rounds once, |t + r| u in the argument and therefore relative in the value; expf
is good to one ulp, 2 u: (|t + r| + 2) u to first order.  Asserted: 4 u (|t + r| + 2) relative to the float64 exp(t_ref + r), wherever that
is a normal float32 (a relative bound says nothing below 2^-126; there val must merely not exceed 2^-125)."""
import numpy as np
import pytest
import torch

from tests._knn_reference import exact_d2
from tests._ot_reference import lse_ref, sinkhorn_ref, t_from_cost, t_ref, topk_ref

pytestmark = pytest.mark.gpu

TQ, TC, SPLIT_MAX = 128, 64, 64   # what the parametrisation assumes; test_tiles pins them
U = 2.0 ** -24
L_SENTINEL, IDX_SENTINEL, VAL_SENTINEL, MASS_SENTINEL = -7.5, -77, -7.0, -9.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _pitch(D, kind):
    return (D + 1) | 1 if kind == "odd" else (D + 4) // 4 * 4 + 4


def _padded(A, ld, dev):
    buf = torch.full((max(A.shape[0], 1), ld), float("nan"), dtype=torch.float32, device=dev)
    buf[:A.shape[0], :A.shape[1]] = torch.from_numpy(A).to(dev)
    return buf[:A.shape[0], :A.shape[1]]


def _operands(dev, X, Y, pitch):
    D = X.shape[1]
    return _padded(X, _pitch(D, pitch), dev), _padded(Y, _pitch(D, "x4" if pitch == "odd" else "odd"), dev)


def _softmin(dev, X, Y, h, s, n_split=0, pitch="odd"):
    from spvipes_amd.ot_ops import ot_softmin
    n_q = X.shape[0]
    out = torch.full((n_q + 3,), L_SENTINEL, dtype=torch.float32, device=dev)
    L = ot_softmin(*_operands(dev, X, Y, pitch), torch.from_numpy(h).to(dev), s, n_split=n_split, out=out)
    assert L.shape == (n_q,)
    out = out.cpu().numpy()
    assert (out[n_q:] == L_SENTINEL).all(), "L written beyond n_q"
    return out[:n_q]


def _topk(dev, X, Y, h, r, s, k, n_split=0, pitch="odd"):
    from spvipes_amd.ot_ops import ot_topk
    n_q, ld = X.shape[0], k + 3
    idx = torch.full((n_q + 2, ld), IDX_SENTINEL, dtype=torch.int32, device=dev)
    val = torch.full((n_q + 2, ld), VAL_SENTINEL, dtype=torch.float32, device=dev)
    mass = torch.full((n_q + 3,), MASS_SENTINEL, dtype=torch.float32, device=dev)
    i, v, m = ot_topk(*_operands(dev, X, Y, pitch), torch.from_numpy(h).to(dev), torch.from_numpy(r).to(dev), s, k, n_split=n_split,
                      out=(idx[:n_q], val[:n_q], mass))
    assert i.shape == v.shape == (n_q, k) and m.shape == (n_q,)
    idx, val, mass = idx.cpu().numpy(), val.cpu().numpy(), mass.cpu().numpy()
    assert (idx[:n_q, k:] == IDX_SENTINEL).all() and (idx[n_q:] == IDX_SENTINEL).all(), "idx written outside [n_q, k]"
    assert (val[:n_q, k:] == VAL_SENTINEL).all() and (val[n_q:] == VAL_SENTINEL).all(), "val written outside [n_q, k]"
    assert (mass[n_q:] == MASS_SENTINEL).all(), "mass written beyond n_q"
    return idx[:n_q, :k], val[:n_q, :k], mass[:n_q]


def _lattice(rng, n, D):
    return rng.integers(-8, 9, (n, D)).astype(np.float32) / 4   # multiples of 1/4 in [-2, 2]: every cost and, with s = 1/2, every t exact


def _real(rng, n, D):
    return rng.standard_normal((n, D)).astype(np.float32)


def _data(kind, rng, n_q, n_c, D):
    """(X, Y, h, s): t of the order of -10 whatever D"""
    if kind == "lattice":
        return _lattice(rng, n_q, D), _lattice(rng, n_c, D), rng.integers(-6, 7, n_c).astype(np.float32) / 2, 0.5
    return _real(rng, n_q, D), _real(rng, n_c, D), _real(rng, n_c, 1)[:, 0].copy(), float(np.float32(5.0 / D))


def _resolved(n_q, n_c, n_split):
    from spvipes_amd.ot_ops import ot_splits
    return n_split or ot_splits(n_q, n_c)


def lse_bound(L_want, n_q, n_c, n_split):
    """the module docstring's bound; ``n_split`` as passed (0 = automatic)"""
    ns = _resolved(n_q, n_c, n_split)
    n_chain = -(-n_c // ns)
    return (3 * n_chain + 4 * ns + 5 * np.log(n_c + 1.0) + 16) * U + 2 * U * np.maximum(np.abs(L_want), 1.0)


def _hold_L(L, want, n_q, n_c, n_split, what=""):
    fin = np.isfinite(want)
    assert np.isneginf(L[~fin]).all(), "a row without a contributing candidate must be -inf"
    err, bound = np.abs(L[fin].astype(np.float64) - want[fin]), lse_bound(want[fin], n_q, n_c, n_split)
    if fin.any():
        print(f"softmin {what} n_q {n_q} n_c {n_c} n_split {n_split}: max |L - L_ref| = {err.max():.3e}, bound {bound.min():.3e}, "
              f"the issue's formula {((2 * -(-n_c // _resolved(n_q, n_c, n_split)) + 2 * _resolved(n_q, n_c, n_split) + 16) * U + 2 * U * np.maximum(np.abs(want[fin]), 1)).min():.3e}")
    assert (err <= bound).all()


def test_tiles(dev):
    from spvipes_amd.ot_ops import OT_DMAX, OT_KMAX, OT_SPLIT_MAX, ot_splits, ot_tiles, ot_ws_bytes
    assert ot_tiles() == (TQ, TC) and (OT_DMAX, OT_KMAX, OT_SPLIT_MAX) == (64, 64, SPLIT_MAX)
    assert ot_splits(2 * TQ + 3, 2000) == 7 and ot_splits(2 * TQ + 3, 2 * TC + 5) == 1 and ot_splits(1, 0) == 1   # what the cases below rely on
    assert ot_ws_bytes(300, 0, 1) == 0 and ot_ws_bytes(300, 0, 3) == 3 * 300 * 8 and ot_ws_bytes(300, 15, 3) == 3 * 300 * 15 * 8


# (n_q, n_c, D, n_split, pitch): every n_q of {1, TQ-1, TQ, TQ+1, 2TQ+3}, n_c of {0, 1, k-1, k, TC-1, TC, TC+1, 2TC+5, 2000} (k = 15 / 32 of the
# top-k cases below), D of {1, 3, 16, 25, 50, 64} and n_split of {0, 1, 3, 64} at least once
SOFTMIN = [(1, 0, 3, 0, "odd"), (1, 1, 1, 1, "odd"), (TQ - 1, 14, 3, 0, "x4"), (TQ, 15, 16, 3, "odd"), (TQ + 1, TC - 1, 25, 0, "x4"),
           (2 * TQ + 3, TC, 50, 3, "odd"), (TQ, TC + 1, 64, 64, "x4"), (2 * TQ + 3, 2 * TC + 5, 25, 1, "odd"), (TQ + 1, 2 * TC + 5, 1, 64, "x4"),
           (TQ - 1, 31, 16, 0, "odd"), (1, 32, 50, 3, "x4"), (2 * TQ + 3, 2000, 25, 0, "odd"), (TQ + 1, 1999, 64, 0, "x4"), (3, 2000, 3, 64, "odd")]


@pytest.mark.parametrize("kind", ["real", "lattice"])
@pytest.mark.parametrize("n_q,n_c,D,n_split,pitch", SOFTMIN, ids=["-".join(map(str, c)) for c in SOFTMIN])
def test_softmin_against_float64(dev, kind, n_q, n_c, D, n_split, pitch):
    rng = np.random.default_rng(n_q * 1000 + n_c * 10 + D)
    X, Y, h, s = _data(kind, rng, n_q, n_c, D)
    want = lse_ref(t_ref(X, Y, h, s))
    _hold_L(_softmin(dev, X, Y, h, s, n_split, pitch), want, n_q, n_c, n_split, kind)


def test_softmin_special_rows(dev):
    """candidates without mass, costs that overflow, NaN, rows without any contributing candidate; two calls bit-equal"""
    rng = np.random.default_rng(3)
    n_q, n_c, D = TQ + 1, 2 * TC + 5, 25
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    for n_split in (0, 3):
        assert np.isneginf(_softmin(dev, X, Y, np.full(n_c, -np.inf, np.float32), s, n_split)).all()      # no candidate has mass
        assert np.isneginf(_softmin(dev, X, Y[:0], h[:0], s, n_split)).all()                              # no candidate at all
    h2, Y2, X2 = h.copy(), Y.copy(), X.copy()
    h2[[0, 5, TC - 1, TC, n_c - 1]] = -np.inf                # zero mass, mixed in
    h2[7], h2[9] = np.nan, np.inf                            # skipped
    Y2[11, :], Y2[12, 3] = 3e19, np.nan                      # the cost overflows: t = -inf; a NaN cost
    X2[4, :] = np.inf                                        # a query without any finite t
    t = t_ref(X2, Y2, h2, s)
    assert not np.isfinite(t[:, [0, 5, 7, 9, 11, 12, TC]]).any() and not np.isfinite(t[4]).any()
    want = lse_ref(t)
    assert np.isneginf(want[4]) and np.isfinite(np.delete(want, 4)).all()
    for n_split in (0, 1, 3, SPLIT_MAX):
        L = _softmin(dev, X2, Y2, h2, s, n_split)
        _hold_L(L, want, n_q, n_c, n_split, "special")
        np.testing.assert_array_equal(L.view(np.uint32), _softmin(dev, X2, Y2, h2, s, n_split).view(np.uint32))
    # the rows without the bad candidates: the same problem
    keep = np.isfinite(t[0])
    _hold_L(_softmin(dev, X2, Y2[keep], h2[keep], s, 1), want, n_q, int(keep.sum()), 1, "without the bad rows")


def _hold_topk(got, t, r, k):
    idx, val, mass = got
    want_idx, want_t = topk_ref(t, k)
    np.testing.assert_array_equal(idx, want_idx)
    filled = want_idx >= 0
    assert (val[~filled] == 0).all()
    arg = want_t.astype(np.float64) + r.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        want_val = np.exp(arg)
        normal = filled & (want_val >= 2.0 ** -126)
        tiny = filled & ~normal
        rel = np.abs(val.astype(np.float64) - want_val) / want_val
        assert (rel[normal] <= 4 * U * (np.abs(arg[normal]) + 2)).all(), f"val off by {np.nanmax(rel[normal] / (U * (np.abs(arg[normal]) + 2))):.2f} x u (|t + r| + 2)"
    assert (val[tiny] <= 2.0 ** -125).all()
    if normal.any():
        print(f"topk k {k}: max val error {np.max(rel[normal] / (U * (np.abs(arg[normal]) + 2))):.3f} x u (|t + r| + 2), asserted 4")
    acc = np.zeros(idx.shape[0], dtype=np.float32)
    for s_ in range(k):
        acc = (acc + val[:, s_]).astype(np.float32)
    np.testing.assert_array_equal(mass.view(np.uint32), acc.view(np.uint32))


# (n_q, n_c, D, k, n_split, pitch): every k of {1, 15, 32, 64}; n_c around k, around the tile and at the chunked size; short rows (n_c < k)
TOPK = [(1, 0, 3, 15, 0, "odd"), (1, 1, 1, 1, 1, "odd"), (TQ - 1, 14, 3, 15, 0, "x4"), (TQ, 15, 16, 15, 3, "odd"), (TQ + 1, 31, 25, 32, 0, "x4"),
        (TQ, 32, 50, 32, 64, "odd"), (2 * TQ + 3, TC - 1, 64, 64, 0, "x4"), (TQ + 1, TC, 25, 64, 3, "odd"), (2 * TQ + 3, TC + 1, 16, 1, 1, "x4"),
        (TQ - 1, 2 * TC + 5, 50, 32, 64, "odd"), (2 * TQ + 3, 2000, 25, 32, 0, "odd"), (TQ + 1, 1999, 64, 15, 0, "x4"), (3, 2000, 1, 64, 3, "odd")]


@pytest.mark.parametrize("kind", ["real", "lattice"])
@pytest.mark.parametrize("n_q,n_c,D,k,n_split,pitch", TOPK, ids=["-".join(map(str, c)) for c in TOPK])
def test_topk_equals_the_reference(dev, kind, n_q, n_c, D, k, n_split, pitch):
    """idx EQUAL to the stable sort of (-t, j) -- lattice data is full of equal t --, val within its bound, mass the fp32 sum of val"""
    rng = np.random.default_rng(n_q * 1000 + n_c * 10 + D + k)
    X, Y, h, s = _data(kind, rng, n_q, n_c, D)
    r = _real(rng, n_q, 1)[:, 0].copy()
    t = t_ref(X, Y, h, s)
    if kind == "lattice" and n_c > k and D <= 3:
        assert (np.diff(topk_ref(t, k)[1], axis=1) == 0).any()   # ties among the selected t
    _hold_topk(_topk(dev, X, Y, h, r, s, k, n_split, pitch), t, r, k)


@pytest.mark.parametrize("kind", ["real", "lattice", "few-candidates"])
def test_topk_every_n_split_gives_the_same_bits(dev, kind):
    rng = np.random.default_rng(5)
    n_q, n_c, D, k = (TQ + 1, 40, 25, 15) if kind == "few-candidates" else (TQ + 1, 300, 25, 15)
    X, Y, h, s = _data("lattice" if kind == "lattice" else "real", rng, n_q, n_c, D)
    r = _real(rng, n_q, 1)[:, 0].copy()
    t = t_ref(X, Y, h, s)
    first = None
    for n_split in (1, 3, 7, SPLIT_MAX, 0):
        got = _topk(dev, X, Y, h, r, s, k, n_split)
        _hold_topk(got, t, r, k)
        first = first or got
        for a, b in zip(got, first):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_topk_non_finite_and_zero_signs(dev):
    """a non-finite t is never selected; -0 and +0 are equal t: the smaller index goes first"""
    rng = np.random.default_rng(8)
    n_q, n_c, D, k = TQ + 1, 2 * TC + 5, 25, 15
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    r = np.zeros(n_q, np.float32)
    h[[0, TC]], h[7], h[9] = -np.inf, np.nan, np.inf
    Y[11, :], Y[12, 3] = 3e19, np.nan
    X[4, :] = np.inf
    t = t_ref(X, Y, h, s)
    got = _topk(dev, X, Y, h, r, s, k, 3)
    _hold_topk(got, t, r, k)
    assert not np.isin(got[0], [0, 7, 9, 11, 12, TC]).any() and (got[0][4] == -1).all() and got[2][4] == 0
    # all costs +0 (every point the same) and h = +-0: t = +-0 everywhere, the order is the index order
    Z = np.ones((3, 4), np.float32)
    hz = np.where(np.arange(40) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    i0, v0, m0 = _topk(dev, Z, np.ones((40, 4), np.float32), hz, np.zeros(3, np.float32), 1.0, 15, 1)
    np.testing.assert_array_equal(i0, np.broadcast_to(np.arange(15, dtype=np.int32), (3, 15)))
    assert (v0 == 1).all() and (m0 == 15).all()


def test_op_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.ot_ops import ot_softmin, ot_topk
    X, Y = torch.zeros((4, 5), device=dev), torch.zeros((9, 5), device=dev)
    h, r = torch.zeros(9, device=dev), torch.zeros(4, device=dev)
    for bad in (lambda: ot_softmin(X.double(), Y, h, 1.0), lambda: ot_softmin(X.cpu(), Y, h, 1.0), lambda: ot_softmin(X, Y[:, :4], h, 1.0),
                lambda: ot_softmin(X, Y, h[:8], 1.0), lambda: ot_softmin(X, Y, h.double(), 1.0), lambda: ot_softmin(X, Y, h, 1.0, out=torch.zeros(3, device=dev)),
                lambda: ot_topk(X, Y, h, r[:3], 1.0, 2), lambda: ot_topk(X, Y, h, r, 1.0, 2, out=(torch.zeros((4, 1), dtype=torch.int32, device=dev), torch.zeros((4, 2), device=dev), r))):
        with pytest.raises(_abi.SpvError):
            bad()
    for bad in (lambda: ot_topk(X, Y, h, r, 1.0, 0), lambda: ot_topk(X, Y, h, r, 1.0, 65), lambda: ot_softmin(X, Y, h, 1.0, n_split=65), lambda: ot_softmin(X[:0], Y, h, 1.0),
                lambda: ot_softmin(X, Y, h, 0.0), lambda: ot_softmin(X, Y, h, float("inf")), lambda: ot_softmin(X, Y, h, -1.0),
                lambda: ot_softmin(torch.zeros((4, 65), device=dev), torch.zeros((9, 65), device=dev), h, 1.0)):
        with pytest.raises(ValueError):
            bad()


# ---- the Sinkhorn driver and the plan ----------------------------------------------------------------------------------------------------
def _clouds(seed=0, n=(261, 133), D=25):
    """two clouds around the same 4 centres"""
    rng = np.random.default_rng(seed)
    centres = 3.0 * rng.standard_normal((4, D))
    return [(centres[rng.integers(0, 4, m)] + rng.standard_normal((m, D))).astype(np.float32) for m in n]


@pytest.fixture(scope="module")
def clouds():
    X0, X1 = _clouds()
    return X0, X1, exact_d2(X0, X1)   # the costs, computed once and left unchanged


@pytest.mark.parametrize("marginals", ["uniform", "with-zeros"])
def test_sinkhorn_follows_the_float64_iteration(dev, clouds, marginals):
    """30 iterations, tol = 0, against the float64 iteration on the same float32 costs.  One half-step errs by at most
    H = lse_bound + u (max |h| + max |L| + ln n_c): the kernel's bound, the rounding of h = psi + log b (every t moves by at most u |h|), and
    the rounding of t itself (u |t_j|, weighted by the term's share p_j of the sum: sum_j p_j |t_j| <= |L| + sum_j p_j (L - t_j) <= |L| + ln n_c,
    the entropy again).  Log-sum-exp is 1-Lipschitz in the sup norm, so what a half-step inherits it passes on unchanged and the errors
    of the 60 half-steps add up, they do not grow: 60 H."""
    from spvipes_amd.ot_ops import mean_sq_cost, sinkhorn
    X0, X1, c = clouds
    n0, n1 = c.shape
    a = b = None
    if marginals == "with-zeros":
        rng = np.random.default_rng(1)
        a, b = rng.random(n0) + 0.1, rng.random(n1) + 0.1
        a[[0, 17, n0 - 1]], b[[3, n1 - 2]] = 0.0, 0.0
    res = sinkhorn(torch.from_numpy(X0).to(dev), torch.from_numpy(X1).to(dev), epsilon=0.1, a=a, b=b, max_iter=30, tol=0)
    assert res.n_iter == 30 and not res.converged and np.isnan(res.error)
    mean = c.astype(np.float64).mean()
    assert abs(res.cost_scale - mean) <= (X0.shape[1] + 2) * 2.0 ** -23 * mean   # the float32 chain's own bound (tests/test_gpu_knn.py)
    assert abs(mean_sq_cost(torch.from_numpy(X0), torch.from_numpy(X1)) - res.cost_scale) <= 1e-12 * mean
    assert res.inv_eps == float(np.float32(1.0 / (0.1 * res.cost_scale)))
    log_a, log_b = res.log_a.cpu().numpy(), res.log_b.cpu().numpy()
    if marginals == "with-zeros":
        assert np.isneginf(log_a[[0, 17, n0 - 1]]).all() and np.isneginf(log_b[[3, n1 - 2]]).all() and np.isfinite(log_a).sum() == n0 - 3
        np.testing.assert_allclose(np.exp(log_a.astype(np.float64)), a / a.sum(), rtol=1e-6)
    else:
        assert (log_a == np.float32(-np.log(n0))).all() and (log_b == np.float32(-np.log(n1))).all()
    phi64, psi64 = sinkhorn_ref(c, res.inv_eps, log_a, log_b, 30)
    phi, psi = res.phi.cpu().numpy().astype(np.float64), res.psi.cpu().numpy().astype(np.float64)
    fin_a, fin_b = np.isfinite(log_a), np.isfinite(log_b)
    big = max(np.abs(phi64).max(), np.abs(psi64).max())
    h_max = big + max(np.abs(log_a[fin_a]).max(), np.abs(log_b[fin_b]).max())
    H = max(lse_bound(np.array([big]), n0, n1, 0)[0], lse_bound(np.array([big]), n1, n0, 0)[0]) + U * (h_max + big + np.log(max(n0, n1)))
    err = max(np.abs(phi - phi64).max(), np.abs(psi - psi64).max())
    print(f"sinkhorn {marginals}: max potential error {err:.3e}, 60 H = {60 * H:.3e}")
    assert err <= 60 * H


def test_sinkhorn_stops_on_tol_and_repeats(dev, clouds):
    from spvipes_amd.ot_ops import sinkhorn
    X0, X1 = (torch.from_numpy(x).to(dev) for x in clouds[:2])
    res = sinkhorn(X0, X1, epsilon=0.5, max_iter=200, tol=1e-3, check_every=5)
    assert res.converged and res.error <= 1e-3 and res.n_iter % 5 == 0 and res.n_iter < 200
    again = sinkhorn(X0, X1, epsilon=0.5, max_iter=200, tol=1e-3, check_every=5)
    assert again.n_iter == res.n_iter and torch.equal(again.phi, res.phi) and torch.equal(again.psi, res.psi)
    for bad in (dict(epsilon=0.0), dict(scale_cost="median"), dict(max_iter=0), dict(tol=-1.0), dict(a=np.ones(5)), dict(b=-np.ones(X1.shape[0]))):
        with pytest.raises(ValueError):
            sinkhorn(X0, X1, **bad)


def test_transport_plan_is_the_union_of_the_reference_lists(dev, clouds):
    """On the device's own potentials: both passes' lists from the reference, their union built here in plain numpy.  No threshold on
    the captured mass is asserted: how much of a row the k largest entries hold is a property of entropic OT at the chosen epsilon
    (0.3 to 0.5 of it at epsilon = 0.05 x the mean cost and k = 16 on clouds like these), for the user to read in row_kept / col_kept."""
    from spvipes_amd.ot_ops import ot_topk, transport_plan
    X0, X1, c = clouds
    n0, n1 = c.shape
    k = 16
    d0, d1 = torch.from_numpy(X0).to(dev), torch.from_numpy(X1).to(dev)
    plan = transport_plan(d0, d1, k=k, epsilon=0.05, max_iter=30, tol=0)
    res = plan.sinkhorn
    h = (res.psi + res.log_b).cpu().numpy()   # float32 additions, as the driver makes them
    r = (res.phi + res.log_a).cpu().numpy()
    np.testing.assert_array_equal(h.view(np.uint32), (res.psi.cpu().numpy() + res.log_b.cpu().numpy()).view(np.uint32))
    t_rows, t_cols = t_from_cost(c, h, res.inv_eps), t_from_cost(c.T, r, res.inv_eps)
    rows = ot_topk(d0, d1, res.psi + res.log_b, res.phi + res.log_a, res.inv_eps, k)
    cols = ot_topk(d1, d0, res.phi + res.log_a, res.psi + res.log_b, res.inv_eps, k)
    rows, cols = [x.cpu().numpy() for x in rows], [x.cpu().numpy() for x in cols]
    _hold_topk(rows, t_rows, r, k)
    _hold_topk(cols, t_cols, h, k)
    want = {}
    for j, (ii, vv) in enumerate(zip(*topk_ref(t_cols, k))):
        for i in ii[ii >= 0]:
            want[(int(i), j)] = ("col", cols[1][j][list(ii).index(i)])
    both = []
    for i, (jj, vv) in enumerate(zip(*topk_ref(t_rows, k))):
        for s_, j in enumerate(jj[jj >= 0]):
            if (i, int(j)) in want:
                both.append((rows[1][i][s_], want[(i, int(j))][1], t_rows[i, j], r[i], t_cols[j, i], h[j]))
            want[(i, int(j))] = ("row", rows[1][i][s_])
    keys = sorted(want)
    M = plan.to_scipy()
    assert M.shape == (n0, n1) and M.dtype == np.float32 and plan.nnz == len(keys)
    np.testing.assert_array_equal(plan.indptr, np.searchsorted([i for i, _ in keys], np.arange(n0 + 1)))
    np.testing.assert_array_equal(plan.indices, np.array([j for _, j in keys], dtype=np.int32))
    np.testing.assert_array_equal(plan.data.view(np.uint32), np.array([want[key][1] for key in keys], dtype=np.float32).view(np.uint32))
    # pairs both passes found: each value is within the val bound of ITS float64 exp(t + r), and the two arguments, fl(-c s + h_j) + r_i
    # and fl(-c s + r_i) + h_j, are the same number up to the one rounding inside either t: u (|t_row| + |t_col|) more
    assert len(both) > 0
    rv, cv, tr, rr, tc, hh = (np.array(x, dtype=np.float64) for x in zip(*both))
    allowed = (4 * U * (np.abs(tr + rr) + 2) + 4 * U * (np.abs(tc + hh) + 2) + U * (np.abs(tr) + np.abs(tc))) * np.maximum(rv, cv)
    print(f"transport_plan: {len(both)} pairs in both passes, max |row - col| / allowed = {(np.abs(rv - cv) / allowed).max():.3f}")
    assert (np.abs(rv - cv) <= allowed).all()
    # the masses are the kernels' own sums, the kept shares follow from them
    np.testing.assert_array_equal(plan.row_mass.view(np.uint32), rows[2].view(np.uint32))
    np.testing.assert_array_equal(plan.col_mass.view(np.uint32), cols[2].view(np.uint32))
    # ... and equal the reference's: every entry within the val bound, k additions of non-negative terms with one rounding each
    for mass, t_all, off in ((plan.row_mass, t_rows, r), (plan.col_mass, t_cols, h)):
        arg = topk_ref(t_all, k)[1].astype(np.float64) + off[:, None]
        want_mass = np.exp(arg).sum(1)
        assert (np.abs(mass - want_mass) <= (4 * U * (np.abs(arg) + 2) * np.exp(arg)).sum(1) + k * U * want_mass).all()
    np.testing.assert_allclose(plan.row_kept, plan.row_mass * n0, rtol=1e-6)
    np.testing.assert_allclose(plan.col_kept, plan.col_mass * n1, rtol=1e-6)
    print(f"transport_plan: nnz {plan.nnz}, kept share of a row's mass {plan.row_kept.min():.3f} .. {plan.row_kept.max():.3f}")
    sp = plan.sparse_plan(dev)
    assert sp.n0 == n0 and sp.n1 == n1 and int(sp.ind0.numel()) == int((plan.data > 0).sum())
