"""GPU: spv_gram_f64 through its wrapper (``gram_ops.gram_accumulate``) and, for the sentinels, through the raw ABI.

Lattice operands (integer-valued fp32, |x| <= 2^10, at most 2^12 rows): every sum is an integer below 2^53, so the tables must EQUAL the
int64 reference bit for bit -- the test that catches a wrong lane map of the f64 MFMA, a wrong tile or mirror address, a wrong slab bound.
Shapes: rows 1 / 3 / 4 / 5 / 31 / 33 / 70 / 257 (the MFMA's K = 4 step, the 32-row staging chunk, which is also the slab minimum) by columns
1 / 15 / 16 / 17 / 63 / 64 / 65 / 130 (fragment edges, tile edges, an off-diagonal tile and its mirror), with ld_x > n and ld_gram > n.

Real operands (mixed sign, column scales over six decades): the yardstick is the long-double sum of the products, which are exact in
fp64 and in long double (48 bits of 53 / 64; the long-double sum's own error, m 2^-64 relative, is 2^-11 of the bound and ignored).  Every
element must lie within gamma_m (|start| + sum |x_i x_j|), gamma_m = m u / (1 - m u), u = 2^-53, m = n_use + slabs + 1: the bound of ANY
order of m - 1 additions of exact terms (Higham, Accuracy and Stability, section 4.2; n_use - 1 inside the slabs, the slabs' merge, the
add onto the start).  A sequential fp64 sum of the same products is held to the same bound first.  The worst measured fraction of the
bound is printed (DESIGN.md section 26 records it).  Every test here needs the feature and fails without it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ROWS = (1, 3, 4, 5, 31, 33, 70, 257)
COLS = (1, 15, 16, 17, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _lattice(rng, n_rows, n, ld_x):
    x = np.full((n_rows, ld_x), np.nan, np.float32)   # padding columns are never read
    x[:, :n] = rng.integers(-1024, 1025, (n_rows, n)).astype(np.float32)
    return x


def _real(rng, n_rows, n, ld_x):
    x = np.full((n_rows, ld_x), np.nan, np.float32)
    x[:, :n] = (rng.standard_normal((n_rows, n)) * 10.0 ** rng.uniform(-3, 3, (1, n))).astype(np.float32)
    return x


def _run(dev, x, n, rows=None, start=None, ld_gram=None, ws="auto"):
    """-> (sums [n], gram [n, n], the padding columns of gram) after one gram_accumulate onto ``start`` = (sums, gram) or zeros"""
    from spvipes_amd.gram_ops import gram_accumulate, gram_workspace
    ld_gram = ld_gram or n
    xd = torch.as_tensor(x, device=dev)[:, :n]
    s = torch.zeros(n, dtype=torch.float64, device=dev)
    g = torch.full((n, ld_gram), -7.25, dtype=torch.float64, device=dev)
    g[:, :n] = 0.0
    if start is not None:
        s.copy_(torch.as_tensor(start[0])), g[:, :n].copy_(torch.as_tensor(start[1]))
    r = None if rows is None else torch.as_tensor(np.asarray(rows, np.int32), device=dev)
    n_use = x.shape[0] if rows is None else len(rows)
    gram_accumulate(xd, rows=r, sums=s, gram=g[:, :n], ws=gram_workspace(n, n_use, dev) if ws == "auto" else ws)
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    return s.cpu().numpy(), g[:, :n].copy(), g[:, n:]


def _exact(x, n, rows=None, start=None):
    """long-double (sums, gram, sum |x|, sum |x_i x_j|) over the counted rows, the start included in the first two"""
    xs = (x if rows is None else x[np.asarray(rows, np.int64)])[:, :n].astype(np.longdouble)
    s0, g0 = (np.zeros(n), np.zeros((n, n))) if start is None else start
    return xs.sum(0) + s0, xs.T @ xs + g0, np.abs(xs).sum(0) + np.abs(s0), np.abs(xs).T @ np.abs(xs) + np.abs(g0)


def _gamma(n_use, slabs):
    m = n_use + slabs + 1
    return m * U / (1 - m * U)


def _fraction(got, exact, mag, gam):
    """the worst |got - exact| as a fraction of the bound gam * mag (0 / 0 counts as 0: an exact zero)"""
    err, bound = np.abs(got - exact).astype(np.float64), (gam * mag).astype(np.float64)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))))


@pytest.mark.parametrize("n_rows", ROWS)
def test_lattice_tables_equal_the_int64_reference_bit_for_bit(dev, n_rows):
    from spvipes_amd.gram_ops import gram_slabs
    rng = np.random.default_rng(100 + n_rows)
    merged = 0
    for n in COLS:
        x = _lattice(rng, n_rows, n, n + 3)
        xi = x[:, :n].astype(np.int64)
        s, g, pad = _run(dev, x, n, ld_gram=n + 5)
        assert np.array_equal(_bits(s), _bits(xi.sum(0).astype(np.float64))), f"sums differ at rows {n_rows}, n {n}"
        assert np.array_equal(_bits(g), _bits((xi.T @ xi).astype(np.float64))), f"gram differs at rows {n_rows}, n {n}"
        assert (pad == -7.25).all(), f"columns >= n of gram were written at rows {n_rows}, n {n}"
        merged += gram_slabs(n, n_rows) >= 2
    if n_rows >= 70:
        assert merged == len(COLS) and gram_slabs(130, 257) == 8 and gram_slabs(17, 70) == 2   # the merge pass is covered here
    if n_rows <= 33:
        assert merged == 0


def test_lattice_at_its_row_limit_onto_a_nonzero_start(dev):
    """2^12 rows of |x| <= 2^10, one column at the limit throughout: every sum stays below 2^20 * 2^12 = 2^32, so does the integer start
    (symmetric, as every table of the kernel's making is), and the accumulated tables are exact"""
    from spvipes_amd.gram_ops import gram_slabs
    rng = np.random.default_rng(7)
    n_rows, n = 4096, 65
    x = _lattice(rng, n_rows, n, n)
    x[:, 0] = 1024.0                                      # the largest sum the lattice allows: 2^12 * 2^20
    xi = x.astype(np.int64)
    g0 = np.triu(rng.integers(-10 ** 6, 10 ** 6, (n, n))).astype(np.float64)
    g0 = g0 + np.triu(g0, 1).T
    s0 = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.float64)
    assert gram_slabs(n, n_rows) >= 2
    s, g, _ = _run(dev, x, n, start=(s0, g0))
    assert np.array_equal(s, xi.sum(0) + s0) and np.array_equal(g, (xi.T @ xi) + g0)


REAL = [(257, 130, None), (70, 17, None), (33, 64, None), (300, 65, 200), (5, 15, 3)]


@pytest.mark.parametrize("n_rows,n,n_listed", REAL, ids=[f"r{r}-n{n}-{'all' if k is None else k}" for r, n, k in REAL])
def test_real_operands_lie_within_the_summation_bound(dev, n_rows, n, n_listed):
    from spvipes_amd.gram_ops import gram_slabs
    rng = np.random.default_rng(n_rows * 1000 + n)
    x = _real(rng, n_rows, n, n + 1)
    rows = None if n_listed is None else np.sort(rng.choice(n_rows, n_listed, replace=False))
    if rows is not None:
        x[np.setdiff1d(np.arange(n_rows), rows)] = np.nan   # uncounted rows are never read
    n_use = n_rows if rows is None else n_listed
    g0 = np.triu(rng.standard_normal((n, n)))
    start = (rng.standard_normal(n), g0 + np.triu(g0, 1).T)
    S, Cm, magS, magC = _exact(x, n, rows, start)
    gam = _gamma(n_use, gram_slabs(n, n_use))
    # the reference first: a sequential fp64 sum of the same exact products, from the start
    x64 = (x if rows is None else x[rows])[:, :n].astype(np.float64)
    seq_s, seq_c = start[0].copy(), start[1].copy()
    for r in range(n_use):
        seq_s += x64[r]
        seq_c += np.outer(x64[r], x64[r])
    f_ref = max(_fraction(seq_s, S, magS, gam), _fraction(seq_c, Cm, magC, gam))
    assert f_ref <= 1.0, f"the sequential fp64 reference itself leaves the bound: {f_ref}"
    s, g, _ = _run(dev, x, n, rows=rows, start=start)
    f_s, f_c = _fraction(s, S, magS, gam), _fraction(g, Cm, magC, gam)
    print(f"gram bound fractions rows {n_use} n {n}: sums {f_s:.3e} gram {f_c:.3e} (sequential fp64 reference {f_ref:.3e})")
    assert f_s <= 1.0 and f_c <= 1.0
    assert np.array_equal(_bits(g), _bits(g.T))


def test_rows_subset_arange_and_nan_outside_the_counted_part(dev):
    rng = np.random.default_rng(3)
    n_rows, n = 70, 65
    x = _lattice(rng, n_rows, n, n + 2)
    xi = x[:, :n].astype(np.int64)
    whole = _run(dev, x, n)
    listed = _run(dev, x, n, rows=np.arange(n_rows))
    assert np.array_equal(_bits(whole[0]), _bits(listed[0])) and np.array_equal(_bits(whole[1]), _bits(listed[1]))   # arange == NULL
    rows = np.sort(rng.choice(n_rows, 37, replace=False))
    clean = _run(dev, x, n, rows=rows)
    assert np.array_equal(clean[1], (xi[rows].T @ xi[rows]).astype(np.float64)) and np.array_equal(clean[0], xi[rows].sum(0).astype(np.float64))
    dirty = x.copy()
    dirty[np.setdiff1d(np.arange(n_rows), rows)] = np.nan
    got = _run(dev, dirty, n, rows=rows)
    assert np.array_equal(_bits(got[0]), _bits(clean[0])) and np.array_equal(_bits(got[1]), _bits(clean[1]))
    # real data: the same with rounding in play
    xr = _real(rng, n_rows, n, n + 2)
    a = _run(dev, xr, n, rows=rows)
    xr[np.setdiff1d(np.arange(n_rows), rows)] = np.nan
    b = _run(dev, xr, n, rows=rows)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_two_halves_against_the_whole_repeats_and_symmetry(dev):
    from spvipes_amd.gram_ops import gram_slabs
    rng = np.random.default_rng(4)
    n_rows, n = 257, 130
    x = _real(rng, n_rows, n, n)
    whole = _run(dev, x, n)
    again = _run(dev, x, n)
    assert np.array_equal(_bits(whole[0]), _bits(again[0])) and np.array_equal(_bits(whole[1]), _bits(again[1]))   # bit-equal repeats
    assert np.array_equal(_bits(whole[1]), _bits(whole[1].T))                                                   # bit-exact symmetry
    first = _run(dev, x, n, rows=np.arange(0, 128))
    both = _run(dev, x, n, rows=np.arange(128, n_rows), start=(first[0], first[1]))
    S, Cm, magS, magC = _exact(x, n)
    # two calls: each element saw (128 + slabs + 1) and (129 + slabs' + 1) roundings at the most; gamma is monotone, so their sum's gamma bounds it
    gam = _gamma(n_rows, gram_slabs(n, 128) + gram_slabs(n, 129) + 1)
    assert _fraction(both[0], S, magS, gam) <= 1.0 and _fraction(both[1], Cm, magC, gam) <= 1.0
    assert _fraction(whole[0], S, magS, _gamma(n_rows, gram_slabs(n, n_rows))) <= 1.0
    assert np.array_equal(_bits(both[1]), _bits(both[1].T))


def test_sentinels_around_gram_and_the_workspace_through_the_raw_abi(dev):
    from spvipes_amd import _abi
    lib = _abi.load()
    rng = np.random.default_rng(5)
    n_rows, n, ld_x, ld_gram = 70, 65, 70, 72
    assert lib.spv_gram_slabs(n, n_rows) >= 2
    need = int(lib.spv_gram_ws_bytes(n, n_rows))
    assert need > 0 and need % 8 == 0
    x = _lattice(rng, n_rows, n, ld_x)
    xd = torch.as_tensor(x, device=dev)
    s = torch.zeros(n + 4, dtype=torch.float64, device=dev)
    s[n:] = -7.25
    g = torch.full((n, ld_gram), -7.25, dtype=torch.float64, device=dev)
    g[:, :n] = 0.0
    ws = torch.full((need // 8 + 64,), -7.25, dtype=torch.float64, device=dev)
    a = _abi.SpvGramArgs()
    a.x, a.ld_x, a.n_rows, a.rows, a.n_use, a.n = xd.data_ptr(), ld_x, n_rows, None, 0, n
    a.sums, a.gram, a.ld_gram, a.ws, a.ws_bytes = s.data_ptr(), g.data_ptr(), ld_gram, ws.data_ptr(), need
    _abi.call("spv_gram_f64", C.byref(a), _abi.stream_ptr())
    torch.cuda.synchronize()
    xi = x[:, :n].astype(np.int64)
    g, s, ws = g.cpu().numpy(), s.cpu().numpy(), ws.cpu().numpy()
    assert np.array_equal(g[:, :n], (xi.T @ xi).astype(np.float64)) and np.array_equal(s[:n], xi.sum(0).astype(np.float64))
    assert (g[:, n:] == -7.25).all() and (s[n:] == -7.25).all() and (ws[need // 8:] == -7.25).all()
    a.ws_bytes = need - 8
    assert lib.spv_gram_f64(C.byref(a), _abi.stream_ptr()) == -1 and b"ws_bytes" in lib.spv_last_error()


def test_no_counted_row_is_a_no_op_and_the_operand_checks(dev):
    from spvipes_amd import _abi
    from spvipes_amd.gram_ops import gram_accumulate
    rng = np.random.default_rng(6)
    n = 17
    x = torch.as_tensor(_real(rng, 8, n, n), device=dev)
    s0, g0 = torch.randn(n, dtype=torch.float64, device=dev), torch.randn((n, n), dtype=torch.float64, device=dev)
    s, g = s0.clone(), g0.clone()
    gram_accumulate(x, rows=torch.empty(0, dtype=torch.int32, device=dev), sums=s, gram=g)
    gram_accumulate(x[:0], sums=s, gram=g)
    a = _abi.SpvGramArgs()   # the ABI's own no-op: rows given, n_use = 0
    a.x, a.ld_x, a.n_rows, a.rows, a.n_use, a.n = x.data_ptr(), n, 8, x.data_ptr(), 0, n
    a.sums, a.gram, a.ld_gram, a.ws, a.ws_bytes = s.data_ptr(), g.data_ptr(), n, None, 0
    _abi.call("spv_gram_f64", C.byref(a), _abi.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(s, s0) and torch.equal(g, g0)
    ok = dict(sums=s, gram=g)
    for bad, kw, exc in (
            (x.double(), ok, _abi.SpvError), (x.cpu(), ok, _abi.SpvError), (x.t(), ok, _abi.SpvError), (x[0], ok, _abi.SpvError),
            (x, dict(ok, rows=torch.arange(3, device=dev)), _abi.SpvError), (x, dict(ok, rows=torch.arange(9, dtype=torch.int32, device=dev)), ValueError),
            (x, dict(ok, sums=s.float()), _abi.SpvError), (x, dict(ok, sums=s[:n - 1]), _abi.SpvError),
            (x, dict(ok, gram=g[:, :n - 1]), _abi.SpvError), (x, dict(ok, gram=g.cpu()), _abi.SpvError),
            (x, dict(ok, ws=torch.empty(3, dtype=torch.float32, device=dev)), _abi.SpvError)):
        with pytest.raises(exc, match="gram_accumulate: "):
            gram_accumulate(bad, **kw)
    with pytest.raises(ValueError, match="at most 4096 columns"):
        gram_accumulate(torch.empty((1, 4097), dtype=torch.float32, device=dev), sums=torch.empty(4097, dtype=torch.float64, device=dev),
                        gram=torch.empty((1, 1), dtype=torch.float64, device=dev))
