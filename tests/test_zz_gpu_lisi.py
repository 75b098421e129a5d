"""GPU: spv_lisi (spvipes_amd.lisi_ops.lisi) against the float64 reference of tests/_lisi_reference.py, at n in {1, 65, 130},
k in {1, 2, 63, 64, 65, 89, 256} and 1 to 8 label sets, on the lists of ``make_lists`` (short, empty and invalid-index rows and a negative
code among them; tests/test_lisi_host_cpu.py holds the reference itself to known answers and checks that it converges on at least
90 % of the ordinary rows of exactly these cases).  The three GPU files of this feature are named ``test_zz_gpu_*``: they sort, and so
run, behind every other GPU test, which therefore sees the allocation history it always saw (docs/lab_notes.md section AA has the reason).

Three kinds of check:
  * bits: two calls agree, renaming the codes changes nothing, a subset of the rows gives the rows' bits;
  * ``lisi`` against the reference evaluated at the KERNEL's beta, within ``lisi_bound(k)`` = (8 k + 8) 2^-53 relative.  The derivation
    (``_lisi_reference.lisi_bound``) rests on the documented accuracy of the two exponentials: HIP's math API lists double-precision exp
    with a maximum error of 1 ulp, and glibc's is below 1 ulp; the argument -beta d_j is one IEEE product on both sides, the same bits.
    The largest deviation seen is printed next to the bound (about 1e-15 at every k: the worst-case bound is far from tight);
  * calibration: on the rows the reference converges on, the entropy at the kernel's beta is within 2e-5 of log(perplexity) and beta
    matches the reference's to rtol 1e-6; n_valid and converged equal the reference's on every row.
Every test here needs the feature and fails without it."""
import functools

import numpy as np
import pytest
import torch

from tests._lisi_reference import GPU_CASES as CASES, lisi_bound, lisi_ref, make_lists, ordinary_rows, perplexity_of

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def case(n, k, n_c, n_sets):
    """(idx, dist, codes, perplexity, the reference's own result): computed once, shared, never changed"""
    idx, dist, codes = make_lists(np.random.default_rng(1000 * n + 10 * k + n_sets), n, k, n_c, n_sets)
    for a in (idx, dist, codes):
        a.setflags(write=False)
    return idx, dist, codes, perplexity_of(k), lisi_ref(idx, dist, codes, perplexity_of(k))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _run(dev, idx, dist, codes, perplexity, pad=3):
    """lisi on rows with a pitch of k + pad (NaN / sentinel in the padding) -> numpy (lisi [n_sets, n], beta, n_valid, converged)"""
    from spvipes_amd.lisi_ops import lisi
    n, k = idx.shape
    ib = torch.full((n, k + pad), -77, dtype=torch.int32, device=dev)
    db = torch.full((n, k + pad), float("nan"), dtype=torch.float32, device=dev)
    ib[:, :k], db[:, :k] = torch.from_numpy(np.array(idx)).to(dev), torch.from_numpy(np.array(dist)).to(dev)
    out = lisi(ib[:, :k], db[:, :k], torch.from_numpy(np.array(codes)).to(dev), perplexity)
    assert out[0].shape == (np.atleast_2d(codes).shape[0], n) and out[0].dtype == torch.float64
    return tuple(t.cpu().numpy() for t in out)


def _bits(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)


@pytest.mark.parametrize("n,k,n_c,n_sets", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_against_the_float64_reference(dev, n, k, n_c, n_sets):
    idx, dist, codes, perp, ref = case(n, k, n_c, n_sets)
    got = _run(dev, idx, dist, codes, perp)
    # calibration
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3].astype(bool), ref[3])
    on = ref[3]
    assert on[ordinary_rows(n)].mean() >= 0.9
    at = lisi_ref(idx, dist, codes, perp, beta=got[1])
    print(f"n {n} k {k}: reference converged on {int(on.sum())}/{n} rows; entropy off by at most {np.max(np.abs(at[4][on] - np.log(perp)), initial=0):.2e}; "
          f"beta off by at most {np.max(np.abs(got[1][on] / ref[1][on] - 1), initial=0):.2e} relative")
    assert (np.abs(at[4][on] - np.log(perp)) <= 2e-5).all()
    np.testing.assert_allclose(got[1][on], ref[1][on], rtol=1e-6, atol=0)
    # the values at the kernel's beta
    np.testing.assert_array_equal(np.isnan(got[0]), np.isnan(at[0]))
    fin = np.isfinite(at[0])
    np.testing.assert_array_equal(got[0][~fin & ~np.isnan(at[0])], at[0][~fin & ~np.isnan(at[0])])   # +inf: a row without a labelled neighbour
    err = float(np.max(np.abs(got[0][fin] / at[0][fin] - 1), initial=0.0))
    print(f"lisi: largest relative deviation from float64 at the kernel's beta {err:.3e} (bound {lisi_bound(k):.3e})")
    assert err <= lisi_bound(k)
    if n >= 4:   # the empty row
        assert np.isnan(got[0][:, 2]).all() and got[1][2] == 1.0 and got[2][2] == 0 and got[3][2] == 0
        assert got[2][1] == max(1, k // 2) and (got[2][ordinary_rows(n)] == k).all()


@pytest.mark.parametrize("n,k,n_c,n_sets", [(130, 89, 130, 2), (65, 256, 300, 6), (65, 2, 40, 2)], ids=["130-89", "65-256", "65-2"])
def test_repeatability_renaming_and_subsets(dev, n, k, n_c, n_sets):
    idx, dist, codes, perp, _ref = case(n, k, n_c, n_sets)
    a = _run(dev, idx, dist, codes, perp)
    _bits(a, _run(dev, idx, dist, codes, perp, pad=0))                       # twice, and under another pitch
    renamed = np.where(codes >= 0, 1000003 - 13 * codes, -6)   # an injective renaming of the labels; negative stays negative
    _bits(a, _run(dev, idx, dist, renamed.astype(np.int32), perp))
    sub = np.array([n - 1, 0, 3, 64, 1, 2])
    b = _run(dev, idx[sub], dist[sub], codes, perp)
    _bits((a[0][:, sub], a[1][sub], a[2][sub], a[3][sub]), b)
    one = _run(dev, idx, dist, codes[1], perp)                                # one label set alone: the same calibration, the same values
    _bits((a[0][1:2], a[1]), (one[0], one[1]))


def test_known_answers(dev):
    rng = np.random.default_rng(3)
    n, k, n_c = 65, 89, 120
    idx, dist, _c = make_lists(rng, n, k, n_c, 1)
    idx, dist = np.array(idx), np.array(dist)
    idx[1:4], dist[1:4] = idx[4:7], dist[4:7]   # ordinary rows only
    # one label: 1
    got = _run(dev, idx, dist, np.full((1, n_c), 9, dtype=np.int32), 30.0)
    assert (np.abs(got[0] - 1) <= lisi_bound(k)).all()
    # equidistant neighbours with label counts n_l: 1 / sum (n_l / k)^2, whatever beta the search ends on (it cannot converge: H = log k)
    flat = np.full((n, k), np.float32(2.25))
    codes = rng.integers(0, 5, (1, n_c)).astype(np.int32)
    got = _run(dev, idx, flat, codes, 30.0)
    counts = np.stack([np.bincount(codes[0][row], minlength=5) for row in idx])
    want = 1.0 / ((counts / k) ** 2).sum(1)
    assert (np.abs(got[0][0] / want - 1) <= lisi_bound(k)).all()
    assert (got[3] == 0).all() and (got[1] == 2.0 ** 50).all() and (got[2] == k).all()   # H = log 89 > log 30 at every beta: beta doubles 50 times
    got = _run(dev, idx, flat, codes, float(k))   # perplexity = k: H = log k at once
    assert (got[3] == 1).all() and (got[1] == 1.0).all() and (np.abs(got[0][0] / want - 1) <= lisi_bound(k)).all()
    # k far below the perplexity: the entropy of 2 neighbours never reaches log 30, beta halves 50 times
    got = _run(dev, idx[:, :2], dist[:, :2], codes, 30.0)
    assert (got[3] == 0).all() and (got[1] == 2.0 ** -50).all()
    # every code negative: no label has a neighbour, simpson = 0
    got = _run(dev, idx, dist, np.full((1, n_c), -4, dtype=np.int32), 30.0)
    assert np.isposinf(got[0]).all()
    # no candidate rows at all: every index is outside [0, 0)
    got = _run(dev, idx, dist, np.zeros((2, 0), dtype=np.int32), 30.0)
    assert np.isposinf(got[0]).all()


def test_op_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.lisi_ops import lisi
    idx = torch.zeros((4, 5), dtype=torch.int32, device=dev)
    dist = torch.zeros((4, 5), device=dev)
    codes = torch.zeros((2, 9), dtype=torch.int32, device=dev)
    for bad in (lambda: lisi(idx.long(), dist, codes), lambda: lisi(idx, dist.double(), codes), lambda: lisi(idx, dist, codes.long()),
                lambda: lisi(idx, dist[:3], codes), lambda: lisi(idx, dist, torch.zeros((9, 9), dtype=torch.int32, device=dev)),
                lambda: lisi(torch.zeros((4, 257), dtype=torch.int32, device=dev), torch.zeros((4, 257), device=dev), codes), lambda: lisi(idx.cpu(), dist, codes)):
        with pytest.raises(_abi.SpvError):
            bad()
    for perp in (0.5, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            lisi(idx, dist, codes, perp)
