"""GPU: spv_count_stats / spv_count_totals / spv_csr_totals through spvipes_amd.count_ops, against numpy on the host copy.

Bounds.  Row 0 of uint16 counts and row 1 are sums of integers carried exactly: equality.  Row 0 of fp32 counts and row 2 are sums of
n_k non-negative fp64 terms, each formed with at most one rounding (the widening is exact, count * w rounds once), added in some
order with fewer than n_k roundings: the result is within n_k * 2^-53 of the exact sum, relatively; the tests allow twice that,
n_k * 2^-52 * value, against math.fsum (which returns the correctly rounded sum of the same terms).  The totals: G * 2^-52 likewise."""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = 60000
TILE, SLAB = 512, 512   # what the library reports (checked below); parametrisation happens before a library can be loaded


def _ts():
    from spvipes_amd import count_ops

    return count_ops.count_stats_tile(), count_ops.count_stats_slab()


def _shapes():
    """(G, n, col_off, layout) -- a subset of {1, 7, T-1, T, T+1, 2T+3} x {1, 3, S-1, S, S+1, 2S+5}; layout "odd": an odd row pitch
    (rows start at every alignment: the element-wise kernel), "aligned": a pitch and column offset of whole 16-byte pieces (the
    vector kernel, with its straddling lane where G is no multiple of the piece)"""
    T, S = TILE, SLAB
    return [(1, 1, 0, "odd"), (7, 3, 3, "odd"), (7, 2 * S + 5, 8, "aligned"), (T - 1, S - 1, 8, "odd"), (T - 1, S - 1, 8, "aligned"),
            (T, S, 0, "aligned"), (T, S, 3, "odd"), (T + 1, S + 1, 0, "aligned"), (T + 1, 3, 3, "odd"), (2 * T + 3, 2 * S + 5, 8, "aligned"),
            (2 * T + 3, 2 * S + 5, 3, "odd"), (2 * T + 3, 1, 0, "aligned")]


def test_the_library_reports_the_tile_and_slab_the_shapes_assume():
    assert _ts() == (TILE, SLAB)


@functools.lru_cache(maxsize=None)
def _case(G, n, col_off, layout, dtype):
    """host data of one case and its oracle (computed once, shared by the tests that need it, never modified)"""
    rng = np.random.default_rng(G * 7919 + n * 31 + col_off + (dtype == "f32"))
    pool = min(n, 500)                       # listed cells are the even rows 0, 2, ..; the odd rows exist and are never listed
    M = 2 * pool + 1
    ld = col_off + G + 5
    if layout == "odd":
        ld += 1 - ld % 2
    else:
        ld = (ld + 7) // 8 * 8
    keep = rng.random((M, G)) < 0.3          # about 70 % zeros
    if dtype == "u16":
        vals = rng.integers(1, 60, (M, G))
        vals[rng.random((M, G)) < 0.02] = 65535
        X = np.full((M, ld), SENTINEL, np.uint16)
        X[:, col_off:col_off + G] = (vals * keep).astype(np.uint16)
    else:
        X = np.full((M, ld), float(SENTINEL), np.float32)
        X[:, col_off:col_off + G] = (rng.random((M, G)) * 10.0 * keep).astype(np.float32)
    X[1::2] = SENTINEL
    rows = (2 * rng.integers(0, pool, n)).astype(np.int32)   # non-monotone, with repeats as soon as n exceeds a few
    if n >= 3:
        rows[1] = rows[0]
    sizes = [n // 3, 0, n - n // 3]
    w = rng.random(n) * 3.0
    w[n // 2] = 0.0
    own = X[:, col_off:col_off + G]
    want = np.zeros((3, 3, G))
    pos = 0
    for k, s in enumerate(sizes):
        sub = own[rows[pos:pos + s]].astype(np.float64)       # exact widening
        prod = sub * w[pos:pos + s, None]                      # one fp64 rounding per term, as the kernel forms it
        pos += s
        for j in range(G):
            want[k, 0, j] = math.fsum(sub[:, j].tolist())
            want[k, 2, j] = math.fsum(prod[:, j].tolist())
        want[k, 1] = (sub != 0).sum(0)
    return {"X": X, "rows": rows, "sizes": sizes, "w": w, "want": want, "G": G, "col_off": col_off}


def _device(case):
    from spvipes_amd.ops import GroupCounts

    X = case["X"]
    t = torch.from_numpy(X.view(np.int16) if X.dtype == np.uint16 else X).cuda()
    counts = GroupCounts(t, case["G"], case["col_off"])
    return counts, torch.from_numpy(case["rows"]).cuda(), torch.from_numpy(case["w"]).cuda()


def _check(got, case, dtype):
    want, sizes = case["want"], case["sizes"]
    assert got.shape == want.shape and got.dtype == np.float64
    for k, n_k in enumerate(sizes):
        assert np.array_equal(got[k, 1], want[k, 1]), f"segment {k}: non-zero tally"
        if dtype == "u16":
            assert np.array_equal(got[k, 0], want[k, 0]), f"segment {k}: integer sum"
        rows_to_bound = (2,) if dtype == "u16" else (0, 2)
        for f in rows_to_bound:
            err, bound = np.abs(got[k, f] - want[k, f]), n_k * 2.0**-52 * want[k, f]
            print(f"segment {k} row {f}: max err {err.max() if err.size else 0:.3e}, min slack {(bound - err).min() if err.size else 0:.3e}")
            assert (err <= bound).all(), f"segment {k} row {f}: {err.max()} over the bound"
    assert np.array_equal(got[1], np.zeros_like(got[1])), "the empty segment must be zeros"


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("G,n,col_off,layout", _shapes())
def test_count_stats_against_numpy(G, n, col_off, layout, dtype):
    from spvipes_amd import count_ops

    case = _case(G, n, col_off, layout, dtype)
    counts, rows, w = _device(case)
    out = count_ops.count_stats(counts, rows, case["sizes"], w=w)
    got = out.cpu().numpy()
    _check(got, case, dtype)
    again = count_ops.count_stats(counts, rows, case["sizes"], w=w, ws=count_ops.count_stats_workspace(G, case["sizes"], rows.device))
    assert torch.equal(out, again), "two calls must agree bit for bit"
    # w = None is the weight 1: row 2 repeats row 0 (every product is exact)
    plain = count_ops.count_stats(counts, rows, case["sizes"])
    assert torch.equal(plain[:, 0], plain[:, 2]) and torch.equal(plain[:, :2], out[:, :2])


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("G,n,col_off,layout", [s for s in _shapes() if s[0] in (7, TILE + 1, 2 * TILE + 3) and s[1] > 1])
def test_gene_selection_equals_the_columns_of_the_all_genes_call_and_leaves_the_rest_of_out_alone(G, n, col_off, layout, dtype):
    from spvipes_amd import count_ops

    case = _case(G, n, col_off, layout, dtype)
    counts, rows, w = _device(case)
    full = count_ops.count_stats(counts, rows, case["sizes"], w=w)
    rng = np.random.default_rng(5)
    sel = rng.integers(0, G, 9).astype(np.int32)
    sel[3], sel[4] = sel[0], G - 1          # repeats, any order, the last gene
    out = torch.full((3, 3, len(sel) + 4), -7.0, dtype=torch.float64, device="cuda")
    got = count_ops.count_stats(counts, rows, case["sizes"], w=w, genes=torch.from_numpy(sel).cuda(), out=out)
    assert got.shape == (3, 3, len(sel)) and got.data_ptr() == out.data_ptr()
    assert torch.equal(got, full[:, :, torch.from_numpy(sel).long().cuda()])
    assert bool((out[:, :, len(sel):] == -7.0).all()), "columns >= n_sel of out must not be written"


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("G,n,col_off,layout", [s for s in _shapes() if s[1] in (3, SLAB + 1, 2 * SLAB + 5)])
def test_sparse_counts_give_the_dense_result_bit_for_bit(G, n, col_off, layout, dtype):
    from spvipes_amd import count_ops
    from spvipes_amd.ops import SparseGroupCounts

    case = _case(G, n, col_off, layout, dtype)
    counts, rows, w = _device(case)
    sparse = SparseGroupCounts.from_dense(counts)
    sel = torch.tensor([G - 1, 0, G // 2], dtype=torch.int32, device="cuda")
    for genes in (None, sel):
        assert torch.equal(count_ops.count_stats(sparse, rows, case["sizes"], w=w, genes=genes),
                           count_ops.count_stats(counts, rows, case["sizes"], w=w, genes=genes))


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_a_list_longer_than_one_chunk_of_the_sparse_route(dtype):
    from spvipes_amd import count_ops
    from spvipes_amd.ops import SparseGroupCounts

    S = count_ops.count_stats_slab()
    n = count_ops.COUNT_CHUNK_ROWS + S + 7   # more than one chunk: a chunk ends on a slab boundary
    case = _case(41, 600, 8, "odd", dtype)   # the matrix only; the list below is longer than its own
    counts, _, _ = _device(case)
    rng = np.random.default_rng(9)
    rows_h = (2 * rng.integers(0, 500, n)).astype(np.int32)
    w_h = rng.random(n)
    sizes = [S + 3, 0, n - S - 3]
    rows, w = torch.from_numpy(rows_h).cuda(), torch.from_numpy(w_h).cuda()
    dense = count_ops.count_stats(counts, rows, sizes, w=w)
    assert torch.equal(count_ops.count_stats(SparseGroupCounts.from_dense(counts), rows, sizes, w=w), dense)
    own = case["X"][:, 8:8 + 41].astype(np.float64)
    got, pos = dense.cpu().numpy(), 0
    for k, s in enumerate(sizes):
        sub = own[rows_h[pos:pos + s]]
        prod = sub * w_h[pos:pos + s, None]
        pos += s
        assert np.array_equal(got[k, 1], (sub != 0).sum(0))
        for f, terms in ((0, sub), (2, prod)):
            ref = np.array([math.fsum(terms[:, j].tolist()) for j in range(41)])
            if f == 0 and dtype == "u16":
                assert np.array_equal(got[k, f], ref)
            else:
                assert (np.abs(got[k, f] - ref) <= s * 2.0**-52 * ref).all()


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("G,col_off,layout", [(1, 0, "odd"), (63, 3, "odd"), (64, 8, "aligned"), (2 * TILE + 3, 8, "aligned"), (2 * TILE + 3, 3, "odd")])
def test_count_totals_dense_and_csr(G, col_off, layout, dtype):
    from spvipes_amd import count_ops
    from spvipes_amd.ops import SparseGroupCounts

    case = _case(G, 2 * SLAB + 5 if G == 2 * TILE + 3 else 3, col_off, layout, dtype)
    counts, _, _ = _device(case)
    dense = count_ops.count_totals(counts)
    assert dense.dtype == torch.float64 and dense.shape == (counts.n_cells,)
    assert count_ops.count_totals(counts) is dense, "the totals are computed once per resident matrix"
    csr = count_ops.count_totals(SparseGroupCounts.from_dense(counts))
    assert torch.equal(dense, csr), "dense and CSR totals must agree bit for bit"
    own = case["X"][:, col_off:col_off + G].astype(np.float64)
    ref = np.array([math.fsum(r.tolist()) for r in own])
    got = dense.cpu().numpy()
    if dtype == "u16":
        assert np.array_equal(got, ref)
    else:
        err = np.abs(got - ref)
        print(f"totals: max err {err.max():.3e}, bound {(G * 2.0**-52 * ref).max():.3e}")
        assert (err <= G * 2.0**-52 * ref).all()


def test_rows_outside_the_matrix_are_refused_on_the_host():
    from spvipes_amd import _abi, count_ops

    case = _case(7, 3, 3, "odd", "u16")
    counts, rows, w = _device(case)
    for bad in (-1, counts.n_cells):
        r = rows.clone()
        r[1] = bad
        with pytest.raises(ValueError, match="rows must lie in"):
            count_ops.count_stats(counts, r, case["sizes"], w=w)
    with pytest.raises(ValueError, match="genes must lie in"):
        count_ops.count_stats(counts, rows, case["sizes"], genes=torch.tensor([7], dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="add up"):
        count_ops.count_stats(counts, rows, [1, 1])
    with pytest.raises(_abi.SpvError):
        count_ops.count_stats(counts, rows.long(), case["sizes"])
    with pytest.raises(_abi.SpvError):
        count_ops.count_stats(counts, rows, case["sizes"], w=w.float())
    out = count_ops.count_stats(counts, rows[:0], [0, 0])   # nothing listed: zeros
    assert out.shape == (2, 3, 7) and not out.any()
