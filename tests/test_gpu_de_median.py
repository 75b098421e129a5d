"""GPU: the exact per-gene median of the pairs' lfc -- spv_de_median through de_ops.de_median -- against the two middle elements of
the float64 lfc values, computed HERE from the bank contents on the host and the same pair rows and sorted per gene.

Bound.  An order statistic is 1-Lipschitz in the sup norm: if every fp32 term is within ``tol`` of its float64 value, the value of
every rank is within ``tol`` of the float64 value of that rank.  ``tol`` is the per-term bound of tests/test_gpu_de.py, restated (U = 2^-24, L =
the largest |log2(max(x + eps, FLT_MIN))| over the two banks, the hardware log2 good to 1 ulp):

    tol = 2 * (1 * 2 U L)  the two logarithms   +  U * 2 L  the rounding of their difference   +  2 U / ln 2  the rounding of x + eps

No element is left out of the selection, so the bound needs no cap and holds for mid_lo, mid_hi and their mean alike."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
LOG2_ULPS = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _bank(rng, rows, ng, ld, planted, which):
    """fp32 [rows, ld] (columns >= ng hold NaN: they must never be read into a result): exp2 of normals clipped to |log2 x| <= 40"""
    b = np.full((rows, ld), np.nan, np.float32)
    b[:, :ng] = np.exp2(np.clip(rng.normal(0.0, 12.0, (rows, ng)), -40.0, 40.0)).astype(np.float32)
    if planted and ng >= 8:
        b[:, 0] = (3.5, 0.75)[which]                                                  # constant columns: lfc = log2(3.5 / 0.75)
        b[:, 1] = 0.3                                                                  # the same constant on both sides: lfc = 0
        b[:, 2] = np.exp2((10.0, -10.0)[which] + rng.normal(0.0, 1e-2 / math.sqrt(2.0), rows)).astype(np.float32)   # lfc = 20 +- 1e-2
        b[:, 3] = (FLT_MIN * (1.0 + 3.0 * rng.random(rows))).astype(np.float32)        # tiny, never subnormal
        assert (b[:, 3] >= FLT_MIN).all()
    return b


def _tol(b1, b2, ng, eps):
    e = float(np.float32(eps))
    L = max(float(np.abs(np.log2(np.maximum(b[:, :ng].astype(np.float64) + e, FLT_MIN))).max()) for b in (b1, b2))
    return 2 * LOG2_ULPS * 2 * U * L + U * 2 * L + 2 * U / math.log(2.0), L


def _reference(b1, b2, r1, r2, ng, eps):
    """the two middle elements of the float64 lfc values per gene (numpy's), columns in blocks to bound host memory"""
    e = float(np.float32(eps))
    i1, i2 = np.clip(r1, 0, b1.shape[0] - 1), np.clip(r2, 0, b2.shape[0] - 1)
    n = len(r1)
    lo, hi = np.empty(ng), np.empty(ng)
    step = max(1, min(ng, (1 << 23) // n))
    for c0 in range(0, ng, step):
        c = slice(c0, min(ng, c0 + step))
        d = np.log2(np.maximum(b1[i1, c].astype(np.float64) + e, FLT_MIN)) - np.log2(np.maximum(b2[i2, c].astype(np.float64) + e, FLT_MIN))
        d = np.partition(d, sorted({(n - 1) // 2, n // 2}), axis=0)   # both ranks are in their sorted places
        lo[c], hi[c] = d[(n - 1) // 2], d[n // 2]
    return lo, hi


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---- 1. kernel vs float64, and its exact ties to spv_de_pairs on the same inputs -------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1, 5, 0.0), (3, 2, 1, 2, 1, 1, 0.0), (37, 50, 65, 777, 65, 72, 1e-6), (300, 200, 1000, 10_000, 1000, 1000, 0.0),
                                   (64, 64, 64, 1 << 18, 64, 72, 1e-6), (500, 400, 10_003, 1000, 10_003, 10_048, 0.0)],
                         ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_kernel_against_float64(dev, shape):
    """(the 2^18-pair case puts 262 144 equal keys into the planted constant columns: more than a 16-bit counter holds)"""
    from spvipes_amd.de_ops import de_median, de_median_workspace, de_pairs
    rows_1, rows_2, ng, n_pairs, ld1, ld2, eps = shape
    rng = np.random.default_rng(0)
    b1, b2 = _bank(rng, rows_1, ng, ld1, True, 0), _bank(rng, rows_2, ng, ld2, True, 1)
    r1, r2 = rng.integers(0, rows_1, n_pairs).astype(np.int32), rng.integers(0, rows_2, n_pairs).astype(np.int32)
    ctx = f"[{rows_1} x {rows_2} rows, {ng} genes, {n_pairs} pairs, eps {eps:g}]"
    tol, L = _tol(b1, b2, ng, eps)
    ref_lo, ref_hi = _reference(b1, b2, r1, r2, ng, eps)
    d1, d2 = torch.from_numpy(b1).to(dev)[:, :ng], torch.from_numpy(b2).to(dev)[:, :ng]   # row stride ld, ng columns
    t1, t2 = _dev(dev, r1, r2)
    got = _host(de_median(d1, d2, t1, t2, eps=eps, ws=de_median_workspace(ng, n_pairs, dev)))
    lo, hi = got["mid_lo"].astype(np.float64), got["mid_hi"].astype(np.float64)
    assert got["mid_lo"].dtype == np.float32 and lo.shape == hi.shape == (ng,)
    assert np.isfinite(lo).all() and np.isfinite(hi).all(), f"{ctx}: non-finite values (the NaN padding was read?)"
    errs = {"mid_lo": np.abs(lo - ref_lo), "mid_hi": np.abs(hi - ref_hi), "median": np.abs(0.5 * (lo + hi) - 0.5 * (ref_lo + ref_hi))}
    print(f"{ctx} L = {L:.1f}, tol = {tol:.3e}")
    for k, e in errs.items():
        print(f"{ctx} {k}: max err {float(e.max()):.3e}, max err / bound {float(e.max()) / tol:.3f}")
    for k, e in errs.items():
        assert float(e.max()) <= tol, f"{ctx} {k}: outside the bound by {float(e.max()) - tol:.3e}"
    # the same fp32 numbers as spv_de_pairs reduces: the order statistics nest, exactly
    st = _host(de_pairs(d1, d2, t1, t2, delta=0.25, eps=eps))
    assert (st["lfc_min"] <= got["mid_lo"]).all() and (got["mid_lo"] <= got["mid_hi"]).all() and (got["mid_hi"] <= st["lfc_max"]).all()
    if n_pairs == 1:
        for k in ("mid_lo", "mid_hi"):
            np.testing.assert_array_equal(got[k], st["lfc_min"]), np.testing.assert_array_equal(got[k], st["lfc_max"])
    if n_pairs == 2:
        np.testing.assert_array_equal(got["mid_lo"], st["lfc_min"]), np.testing.assert_array_equal(got["mid_hi"], st["lfc_max"])
    if ng >= 8:
        for col in (0, 1):   # the constant planted columns
            assert got["mid_lo"][col] == got["mid_hi"][col] == st["lfc_min"][col] == st["lfc_max"][col]
        if eps == 0.0:
            assert got["mid_lo"][1] == 0.0


# ---- 2. exactness under ties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", [4096, 4097])
def test_powers_of_two_are_exact(dev, n_pairs):
    """banks of powers of two, eps 0: every lfc is a whole number in [-80, 80] (heavy ties), and both outputs equal the float64 values"""
    from spvipes_amd.de_ops import de_median
    rng = np.random.default_rng(11)
    ng = 777
    b1, b2 = (np.exp2(rng.integers(-40, 41, (500, ng)).astype(np.float64)).astype(np.float32) for _ in range(2))
    r1, r2 = rng.integers(0, 500, n_pairs).astype(np.int32), rng.integers(0, 500, n_pairs).astype(np.int32)
    d = np.sort(np.log2(b1[r1].astype(np.float64)) - np.log2(b2[r2].astype(np.float64)), axis=0)
    assert (d == np.round(d)).all()
    got = _host(de_median(*_dev(dev, b1, b2, r1, r2), eps=0.0))
    np.testing.assert_array_equal(got["mid_lo"].astype(np.float64), d[(n_pairs - 1) // 2])
    np.testing.assert_array_equal(got["mid_hi"].astype(np.float64), d[n_pairs // 2])


@pytest.mark.parametrize("half", [1, 5, 2048, 50_000])
def test_a_column_split_in_two_halves(dev, half):
    """lfc = -1 for exactly ``half`` pairs and 0 for ``half`` more, from explicit pair rows, in several arrangements over 70 genes
    (more than one gene tile): mid_lo == -1 and mid_hi == 0; one more pair of either kind and both outputs are that kind's value"""
    from spvipes_amd.de_ops import de_median
    rng = np.random.default_rng(half)
    ng = 70
    b1 = np.empty((2, ng), np.float32)
    b1[0], b1[1] = 0.5, 1.0                          # row 0 against 1.0: lfc -1; row 1: lfc 0
    b1[:, 1::2] = b1[::-1, 1::2]                     # odd genes: the other way round
    b2 = np.ones((3, ng), np.float32)
    kinds = np.concatenate([np.zeros(half, np.int32), np.ones(half, np.int32)])
    for name, r1 in (("blocks", kinds), ("interleaved", np.tile(np.array([0, 1], np.int32), half)), ("shuffled", rng.permutation(kinds))):
        r2 = rng.integers(0, 3, 2 * half).astype(np.int32)
        got = _host(de_median(*_dev(dev, b1, b2, r1, r2), eps=0.0))
        assert (got["mid_lo"] == -1.0).all() and (got["mid_hi"] == 0.0).all(), f"{name}: {got}"
        for extra in (0, 1):   # one more pair: row `extra` of bank 1
            e1, e2 = np.append(r1, np.int32(extra)), np.append(r2, np.int32(0))
            got = _host(de_median(*_dev(dev, b1, b2, e1, e2), eps=0.0))
            want = np.where(b1[extra] == 0.5, -1.0, 0.0).astype(np.float32)
            np.testing.assert_array_equal(got["mid_lo"], want, err_msg=f"{name} + row {extra}")
            np.testing.assert_array_equal(got["mid_hi"], want, err_msg=f"{name} + row {extra}")


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
def test_identities(dev):
    from spvipes_amd.de_ops import de_median
    rng = np.random.default_rng(21)
    ng, n_pairs = 1500, 5000
    b1, b2 = _bank(rng, 700, ng, ng + 4, True, 0), _bank(rng, 90, ng, ng, True, 1)
    r1, r2 = rng.integers(0, 700, n_pairs).astype(np.int32), rng.integers(0, 90, n_pairs).astype(np.int32)
    d1, d2 = torch.from_numpy(b1).to(dev)[:, :ng], torch.from_numpy(b2).to(dev)
    t1, t2 = _dev(dev, r1, r2)
    a = de_median(d1, d2, t1, t2, eps=1e-6)
    b = de_median(d1, d2, t1, t2, eps=1e-6)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two calls differ"
    assert bool(torch.isfinite(torch.stack(list(a.values()))).all())   # the NaN padding beyond n_genes was never read
    assert bool((a["mid_lo"] < a["mid_hi"]).any())                     # an even number of pairs: the two ranks do differ somewhere
    s = de_median(d2, d1, t2, t1, eps=1e-6)   # swapped: every lfc changes sign, so the order turns round
    assert torch.equal(s["mid_lo"], -a["mid_hi"]) and torch.equal(s["mid_hi"], -a["mid_lo"])
    # row numbers outside a bank are clamped into it: -5 behaves as 0, n_rows + 5 as n_rows - 1
    wild1, wild2 = r1.copy(), r2.copy()
    lo, hi = np.nonzero(r1 == 0)[0], np.nonzero(r2 == 89)[0]
    assert lo.size and hi.size
    wild1[lo], wild2[hi] = -5, 89 + 6
    wild1[np.nonzero(r1 == 699)[0]] = 699 + 6
    c = de_median(d1, d2, *_dev(dev, wild1, wild2), eps=1e-6)
    for k in a:
        assert torch.equal(a[k], c[k]), f"{k}: clamped row numbers change the result"
    # a caller's output array with a wider row stride: same numbers, columns beyond n_genes untouched
    out = torch.full((2, ng + 9), -7.0, device=dev)
    o = de_median(d1, d2, t1, t2, eps=1e-6, out=out)
    for k in a:
        assert torch.equal(a[k], o[k])
    assert bool((out[:, ng:] == -7.0).all())
    # an odd number of pairs: one middle element
    odd = de_median(d1, d2, t1[:-1], t2[:-1], eps=1e-6)
    assert torch.equal(odd["mid_lo"], odd["mid_hi"])


def test_argument_errors_are_reported(dev):
    import ctypes as C
    from spvipes_amd import _abi
    from spvipes_amd.de_ops import de_median, de_median_workspace
    bank = torch.ones(8, 100, device=dev)
    rows = torch.zeros(50, dtype=torch.int32, device=dev)
    mid, ws = torch.empty(2, 100, device=dev), de_median_workspace(100, 50, dev)
    assert ws.numel() * ws.element_size() == _abi.load().spv_de_median_ws_bytes(100, 50)

    def args(**kw):
        a = _abi.SpvDeMedianArgs()
        a.bank1, a.bank2, a.ld1, a.ld2, a.rows1, a.rows2, a.n_rows1, a.n_rows2 = bank.data_ptr(), bank.data_ptr(), 100, 100, rows.data_ptr(), rows.data_ptr(), 8, 8
        a.n_genes, a.n_pairs, a.eps, a.mid, a.ld_mid, a.ws, a.ws_bytes = 100, 50, 0.0, mid.data_ptr(), 100, ws.data_ptr(), ws.numel() * ws.element_size()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    _abi.call("spv_de_median", C.byref(args()), _abi.stream_ptr())   # the good call
    torch.cuda.synchronize()
    assert bool((mid == 0.0).all())
    for bad in (dict(bank1=None), dict(bank2=None), dict(rows1=None), dict(rows2=None), dict(mid=None), dict(ws=None), dict(n_pairs=0), dict(n_pairs=-3),
                dict(n_pairs=(1 << 24) + 1), dict(ld1=99), dict(ld2=99), dict(ld_mid=99), dict(n_genes=0), dict(n_rows1=0), dict(n_rows2=-1),
                dict(ws_bytes=ws.numel() * ws.element_size() - 4), dict(ws=ws.data_ptr() + 2), dict(eps=-1.0), dict(eps=float("nan"))):
        with pytest.raises(_abi.SpvError, match="spv_de_median"):
            _abi.call("spv_de_median", C.byref(args(**bad)), _abi.stream_ptr())
    torch.cuda.synchronize()
    with pytest.raises(_abi.SpvError):
        de_median(bank.double(), bank, rows, rows)
    with pytest.raises(_abi.SpvError):
        de_median(bank.t(), bank.t(), rows, rows)   # column stride != 1
    with pytest.raises(_abi.SpvError):
        de_median(bank, bank, rows.long(), rows)
    with pytest.raises(_abi.SpvError):
        de_median(bank, bank[:, :50], rows, rows)
    with pytest.raises(_abi.SpvError):
        de_median(bank, bank, rows, rows, ws=ws[:-1])
    with pytest.raises(_abi.SpvError):
        de_median(bank, bank, rows, rows, out=torch.empty(7, 100, device=dev))
    with pytest.raises(ValueError):
        de_median(bank, bank, rows, rows[:10])
    with pytest.raises(ValueError):
        de_median(bank, bank, rows, rows, eps=-1e-6)
