"""GPU: the fused decode-and-reduce kernel -- spv_dec_expected_stats through dec_ops.expected_expression_stats, on the harness of
tests/test_gpu_sample_stats.py (``_synthetic_module``, eval mode, 83 genes; bf16, fp32 and the wide layout).  The yardstick is
``dec_ops.expected_expression`` on the SAME operands: its four fp32 outputs (what = 0 .. 3), summed per tile plan on the host.

The bound.  A table entry is a sum of n doubles (n = the counted values of the segment; every fp32 value and every square of one is
exact as a double), added in SOME order.  For any order |computed - exact| <= gamma_{n-1} * sum|v|, gamma_m = m u / (1 - m u),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Onto a non-zero starting value the start is one more
term: gamma_n * (|start| + sum|v|).  The host sums are formed in numpy's 80-bit long double (64-bit significand), whose own error,
about n * 2^-64 * sum|v|, is 2^-11 of u per term and is not added to the bound.  A value that differed from spv_dec_expected's by one
fp32 ulp would be off by 2^-24 relative, eight orders of magnitude above the bound.
Every test here needs the feature and fails without it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_sample_stats import _make_case, _selections

pytestmark = pytest.mark.gpu

BN, G1, SENT, PAD, TILE = 96, 83, 7.0, 5, 32
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the host reference needs an extended-precision long double"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=[("fp32", 0), ("bf16", 0), ("fp32", 12)], ids=lambda p: f"{p[0]}-nb{p[1]}")
def case(request, dev):
    c = _make_case(dev, *request.param, Bn=BN)
    assert c.module.dec_slots.kslots == (1 if request.param[1] == 12 else 0)
    c.values = {}
    return c


def _gamma(m):
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


def _rows(c, rows):
    """the operand rows ``rows`` (a count = the first rows, or an index array) -> contiguous (first, second, library)"""
    if isinstance(rows, (int, np.integer)):
        return c.first[:rows].contiguous(), c.second[:rows].contiguous(), c.lib[:rows].contiguous()
    idx = torch.as_tensor(np.asarray(rows), dtype=torch.int64, device=c.dev)
    return c.first.index_select(0, idx).contiguous(), c.second.index_select(0, idx).contiguous(), c.lib.index_select(0, idx).contiguous()


def _values(c, b, genes):
    """the yardstick's inputs: spv_dec_expected's four outputs for the first ``b`` operand rows -> float32 [4, b, n]"""
    from spvipes_amd import dec_ops
    m, g = c.module, c.g
    f, s, lib = _rows(c, b)
    return np.stack([dec_ops.expected_expression(m.decoders[g], m.px_r[g], f, s, lib, False, m.nsplit, m._workspace(g, c.dev), par=c.par, genes=genes,
                                                 what=w).cpu().numpy() for w in range(4)])


def _all_values(c, name):
    """the four outputs for all BN rows and one selection, computed once per case and left unchanged"""
    if name not in c.values:
        c.values[name] = _values(c, BN, _selections()[name])
        c.values[name].setflags(write=False)
    return c.values[name]


def _stats(c, rows, tile_seg, tile_n, n_seg, stats, genes=None, **kw):
    from spvipes_amd import dec_ops
    m, g = c.module, c.g
    f, s, lib = _rows(c, rows)
    i32 = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=torch.int32, device=c.dev)
    return dec_ops.expected_expression_stats(m.decoders[g], m.px_r[g], f, s, lib, False, m.nsplit, m._workspace(g, c.dev), par=c.par, genes=genes,
                                             tile_seg=i32(tile_seg), tile_n=i32(tile_n), n_seg=n_seg, stats=stats, **kw)


def _counted_rows(b, tile_seg, tile_n, n_seg):
    """operand rows counted per segment, by the entry point's rules -> {segment: row numbers}"""
    rows = {}
    for t in range(-(-b // TILE)):
        sg = int(tile_seg[t])
        if sg < 0 or sg >= n_seg:
            continue
        n = max(0, min(int(tile_n[t]), TILE, b - TILE * t))
        if n:
            rows.setdefault(sg, []).extend(range(TILE * t, TILE * t + n))
    return rows


def _reference(V, rows, n_seg):
    """V float32 [4, b, n], rows {segment: row numbers} -> (sums S, sums of magnitudes A: long double [n_seg, 8, n]; counts [n_seg])"""
    n = V.shape[2]
    S, A, cnt = np.zeros((n_seg, 8, n), dtype=LD), np.zeros((n_seg, 8, n), dtype=LD), np.zeros(n_seg, dtype=np.int64)
    for k, r in rows.items():
        x = V[:, np.asarray(r)].astype(LD)
        S[k, :4], S[k, 4:] = x.sum(1), (x * x).sum(1)
        A[k, :4], A[k, 4:] = np.abs(x).sum(1), S[k, 4:]
        cnt[k] = len(r)
    return S, A, cnt


def _hold(got, start, S, A, cnt, label=""):
    """every entry of ``got`` (float64 [n_seg, 8, >= n]) against the long-double sums; everything else must still read ``start``"""
    n = S.shape[2]
    np.testing.assert_array_equal(got[:, :, n:], start)                  # columns >= n_genes
    worst = 0.0
    for k in range(S.shape[0]):
        if cnt[k] == 0:
            np.testing.assert_array_equal(got[k], start)                 # rows of a segment no counted tile belongs to
            continue
        tol = _gamma(cnt[k] - 1) * A[k] if start == 0.0 else _gamma(cnt[k]) * (A[k] + abs(start))
        err = np.abs(got[k, :, :n].astype(LD) - (LD(start) + S[k]))
        assert (err <= tol).all(), (label, k, int(cnt[k]), float(err.max()), float(tol.min()))
        worst = max(worst, float((err / np.maximum(tol, LD(1e-300))).max()))
    return worst


def _table(c, n_seg, n, start):
    return torch.full((n_seg, 8, n + PAD), start, dtype=torch.float64, device=c.dev)


def _plans(b):
    """(tile_seg, tile_n, n_seg) over the tiles of ``b`` rows; entries of tiles beyond the rows are cut off"""
    nt = -(-b // TILE)
    cut = lambda *a: tuple(np.asarray(x[:nt], dtype=np.int32) for x in a)
    return {
        "one-segment": (*cut([0, 0, 0], [32, 32, 32]), 1),
        # a full tile, a one-cell tile and a skipped tile (code -1); segments 1 and 3 have no tile
        "three-tiles": (*cut([2, 0, -1], [32, 1, 32]), 4),
        # the skipped tile first, its code >= n_seg; tile_n above 32 means 32 and a partial last tile is cut at the rows there are
        "skipped-first": (*cut([5, 2, 0], [32, 40, 32]), 4),
        # a segment spread over two tiles that are not neighbours, partial tiles
        "spread": (*cut([0, 1, 0], [32, 7, 20]), 2),
    }


@pytest.mark.parametrize("b", [1, 31, 33, 70, 96])
def test_tables_equal_the_reduction_of_the_stored_values(case, b):
    """every shape x every selection x every plan, onto a sentinel table (start + sums, untouched entries included) and onto zeros (the
    bound with n - 1, and private + shared against mixture)"""
    c, worst = case, 0.0
    for sname, genes in _selections().items():
        V = _values(c, b, genes)
        n = V.shape[2]
        assert V.shape == (4, b, G1 if genes is None else len(genes)) and np.isfinite(V).all() and (V[0] > 0).any()
        for pname, (tile_seg, tile_n, n_seg) in _plans(b).items():
            rows = _counted_rows(b, tile_seg, tile_n, n_seg)
            S, A, cnt = _reference(V, rows, n_seg)
            for start in (SENT, 0.0):
                stats = _table(c, n_seg, n, start)
                got = _stats(c, b, tile_seg, tile_n, n_seg, stats, genes=genes)
                assert got.data_ptr() == stats.data_ptr()
                got = stats.cpu().numpy()
                worst = max(worst, _hold(got, start, S, A, cnt, (sname, pname, start)))
            # (zero start) private + shared against mixture: each fp32 mixture value is the rounded sum of its two parts, half an fp32
            # ulp each, on top of the three sums' own bounds
            for k in range(n_seg):
                if cnt[k]:
                    parts = got[k, 1, :n].astype(LD) + got[k, 2, :n].astype(LD)
                    tol = _gamma(cnt[k] - 1) * (A[k, 0] + A[k, 1] + A[k, 2]) + LD(2.0 ** -24) * A[k, 0]
                    assert (np.abs(parts - got[k, 0, :n].astype(LD)) <= tol).all()
            if sname == "shuffled" and pname == "one-segment":
                np.testing.assert_array_equal(got[0, :, n - 1], got[0, :, 2])   # a repeated gene fills its own column with the same sums
            if pname == "three-tiles" and b == BN:
                assert cnt.tolist() == [1, 0, 32, 0]
    print(f"b = {b}: worst error / bound = {worst:.3f}")


def test_workspace_and_table_stay_untouched_outside_what_is_written(case):
    """the raw entry point on a workspace of its own: everything beyond ws_bytes, the partial slots of skipped tiles and of the tiles
    beyond the rows keep the sentinel; the slots of counted tiles are all written"""
    from spvipes_amd import _abi, dec_ops
    from spvipes_amd._abi import ptr, stream_ptr
    c, b, n_seg = case, 70, 3
    m, g = c.module, c.g
    genes = _selections()["33"]
    f, s, lib = _rows(c, b)
    o, gidx, n = dec_ops._readout_operands(m.decoders[g], m.px_r[g], f, s, lib, False, m.nsplit, m._workspace(g, c.dev), c.par, genes, "latent", "test")
    n_tiles = o.Bp // TILE
    assert n_tiles == 4   # three tiles with rows, one beyond them
    need = int(_abi.load().spv_dec_expected_stats_ws_bytes(n, n_tiles))
    assert need == n_tiles * 8 * n * 8
    ws = torch.full((need // 8 + 64,), SENT, dtype=torch.float64, device=c.dev)
    stats = _table(c, n_seg, n, SENT)
    tile_seg = torch.tensor([1, -1, 0, 2], dtype=torch.int32, device=c.dev)   # tile 3 lies beyond the rows: its entries are not even read
    tile_n = torch.tensor([32, 32, 32, 32], dtype=torch.int32, device=c.dev)
    a = _abi.SpvDecExpectedStatsArgs()
    dec_ops._fill_readout(a, o, m.nsplit, gidx, n)
    a.n_seg, a.tile_seg, a.tile_n, a.stats, a.ld_stats, a.ws = n_seg, ptr(tile_seg), ptr(tile_n), ptr(stats), stats.stride(1), ptr(ws)
    _abi.call("spv_dec_expected_stats", C.byref(o.p), C.byref(a), stream_ptr())
    w = ws.cpu().numpy()
    np.testing.assert_array_equal(w[need // 8:], SENT)
    part = w[:need // 8].reshape(n_tiles, 8, n)
    np.testing.assert_array_equal(part[1], SENT)
    np.testing.assert_array_equal(part[3], SENT)
    assert (part[[0, 2]] != SENT).all() and np.isfinite(part[[0, 2]]).all() and (part[[0, 2]] > 0).all()
    V = _all_values(c, "33")[:, :b]
    S, A, cnt = _reference(V, _counted_rows(b, tile_seg.cpu().numpy(), tile_n.cpu().numpy(), n_seg), n_seg)
    assert cnt.tolist() == [6, 32, 0]
    _hold(stats.cpu().numpy(), SENT, S, A, cnt)
    # the partial sums themselves: one tile's rows each
    for t, k in ((0, 1), (2, 0)):
        assert (np.abs(part[t].astype(LD) - S[k]) <= _gamma(cnt[k] - 1) * A[k]).all()


def test_two_identical_calls_agree_bit_for_bit_and_two_halves_add_up(case):
    c, n_seg = case, 3
    tile_seg, tile_n = np.array([1, 0, 1], dtype=np.int32), np.array([32, 30, 17], dtype=np.int32)
    out = []
    for _ in range(2):
        stats = torch.zeros((n_seg, 8, G1), dtype=torch.float64, device=c.dev)
        _stats(c, BN, tile_seg, tile_n, n_seg, stats)
        out.append(stats)
    assert float(out[0].sum()) > 0 and torch.equal(out[0], out[1])   # no floating-point atomics: the arrival order cannot show
    # the plan in two halves (the other half's tiles skipped), accumulated into one table: the whole, within the bound
    V = _all_values(c, "none")
    S, A, cnt = _reference(V, _counted_rows(BN, tile_seg, tile_n, n_seg), n_seg)
    halves = torch.zeros((n_seg, 8, G1), dtype=torch.float64, device=c.dev)
    _stats(c, BN, np.array([1, -1, -1]), tile_n, n_seg, halves)
    first = halves.clone()
    _stats(c, BN, np.array([-1, 0, 1]), tile_n, n_seg, halves)
    assert not torch.equal(first, halves) and torch.equal(first[0], torch.zeros_like(first[0]))
    for t in (out[0], halves):
        _hold(t.cpu().numpy(), 0.0, S, A, cnt)


def test_padding_rows_and_positions_do_not_matter(case):
    c, n_seg = case, 2
    tile_seg, tile_n = np.array([0, 1, 0], dtype=np.int32), np.array([32, 9, 20], dtype=np.int32)
    V = _all_values(c, "none")

    def run(rows, ts=tile_seg, tn=tile_n):
        stats = torch.zeros((n_seg, 8, G1), dtype=torch.float64, device=c.dev)
        _stats(c, rows, ts, tn, n_seg, stats)
        return stats

    ident = np.arange(BN)
    base = run(ident)
    # padding rows (at and beyond tile_n) filled with other cells: not a bit changes
    other = ident.copy()
    other[32 + 9:64] = 5
    other[64 + 20:] = np.arange(12)[::-1] + 40
    assert torch.equal(run(other), base)
    # whole tiles permuted, and a cell moved to another slot of its tile: another order of addition, within the bound of the same sums
    S, A, cnt = _reference(V, _counted_rows(BN, tile_seg, tile_n, n_seg), n_seg)
    _hold(base.cpu().numpy(), 0.0, S, A, cnt)
    order = [2, 0, 1]
    tiles = np.concatenate([ident[TILE * t:TILE * (t + 1)] for t in order])
    _hold(run(tiles, tile_seg[order], tile_n[order]).cpu().numpy(), 0.0, S, A, cnt)
    moved = ident.copy()
    moved[[3, 28]] = moved[[28, 3]]
    moved[[64, 64 + 19]] = moved[[64 + 19, 64]]
    got = run(moved)
    _hold(got.cpu().numpy(), 0.0, S, A, cnt)
    torch.testing.assert_close(got[1], base[1], rtol=0, atol=0)   # segment 1's tile was not touched


@pytest.fixture(scope="module")
def big(dev):
    """4096 cells x 2100 genes, bf16 (the larger case of tests/test_gpu_sample_stats.py)"""
    return _make_case(dev, "bf16", 0, Bn=4096, Gs=(70, 2100), seed=4)


def test_a_wave_that_walks_several_gene_tiles(big):
    """4096 cells x 2100 genes, bf16: 128 workgroup columns leave 16 gene slices of 4 waves for 66 tiles, so waves take a second tile
    (the grid note of tests/test_gpu_sample_stats.py) and the transpose tile is reused across tiles.  20 labels over 128 cell tiles."""
    from spvipes_amd import dec_ops
    c, Bn, Gn, n_seg = big, 4096, 2100, 20
    m, g, dev = c.module, c.g, c.dev
    nt = Bn // TILE
    tile_seg = (np.arange(nt) * 13 % n_seg).astype(np.int32)
    tile_seg[::17] = -1
    tile_n = (1 + np.arange(nt) * 7 % TILE).astype(np.int32)
    rows = _counted_rows(Bn, tile_seg, tile_n, n_seg)
    assert len(rows) == n_seg and min(len(r) for r in rows.values()) > 1
    stats = torch.zeros((n_seg, 8, Gn), dtype=torch.float64, device=dev)
    dec_ops.expected_expression_stats(m.decoders[g], m.px_r[g], c.first, c.second, c.lib, False, m.nsplit, m._workspace(g, dev), par=c.par,
                                      tile_seg=torch.as_tensor(tile_seg, device=dev), tile_n=torch.as_tensor(tile_n, device=dev), n_seg=n_seg, stats=stats)
    got = stats.cpu().numpy()
    for w in range(4):
        v = dec_ops.expected_expression(m.decoders[g], m.px_r[g], c.first, c.second, c.lib, False, m.nsplit, m._workspace(g, dev), par=c.par, what=w).cpu().numpy()
        for k in range(n_seg):
            x = v[np.asarray(rows[k])].astype(LD)
            n = x.shape[0]
            assert (np.abs(got[k, w].astype(LD) - x.sum(0)) <= _gamma(n - 1) * np.abs(x).sum(0)).all()
            q = (x * x).sum(0)
            assert (np.abs(got[k, 4 + w].astype(LD) - q) <= _gamma(n - 1) * q).all()


def test_gathered_rows_keep_the_values_of_their_minibatch(big):
    """The softmax denominators are added up in gene splits whose number follows the padded row count: 896 rows x 2100 genes take 72
    splits, the 1024 padded rows of their tile plan would take 36, and the rates would move in their last bits.  With ``batch_rows`` the
    gathered rows keep the split of the minibatch they came from: the sums are those of expected_expression on the 896 rows."""
    from spvipes_amd import dec_ops
    from spvipes_amd.data import expression_tile_plan
    from spvipes_amd.ops import _gene_splits
    c, b, n_seg = big, 896, 3
    m, g, dev = c.module, c.g, c.dev
    seg = np.random.default_rng(2).integers(0, n_seg, size=b)
    seg[::150] = -1   # a few cells outside every segment
    perm, tile_seg, tile_n = expression_tile_plan(seg, n_seg)
    assert _gene_splits(896, 2304) != _gene_splits(-(-perm.size // 128) * 128, 2304)   # the case does what it is here for
    f, s, lib = _rows(c, perm)
    stats = torch.zeros((n_seg, 8, 2100), dtype=torch.float64, device=dev)
    dec_ops.expected_expression_stats(m.decoders[g], m.px_r[g], f, s, lib, False, m.nsplit, m._workspace(g, dev), par=c.par, batch_rows=b,
                                      tile_seg=torch.as_tensor(tile_seg, device=dev), tile_n=torch.as_tensor(tile_n, device=dev), n_seg=n_seg, stats=stats)
    f, s, lib = _rows(c, b)
    V = np.stack([dec_ops.expected_expression(m.decoders[g], m.px_r[g], f, s, lib, False, m.nsplit, m._workspace(g, dev), par=c.par, what=w).cpu().numpy()
                  for w in range(4)])
    S, A, cnt = _reference(V, {k: np.nonzero(seg == k)[0] for k in range(n_seg)}, n_seg)
    assert cnt.min() > 200 and cnt.sum() < b
    _hold(stats.cpu().numpy(), 0.0, S, A, cnt)


def test_argument_errors_are_raised(case):
    from spvipes_amd import _abi
    c = case
    stats = torch.zeros((2, 8, G1), dtype=torch.float64, device=c.dev)
    seg, cnt = torch.zeros(3, dtype=torch.int32, device=c.dev), torch.full((3,), 32, dtype=torch.int32, device=c.dev)
    for bad in (dict(stats=stats[:1]), dict(stats=stats.float()), dict(stats=stats[:, :4]), dict(stats=stats[:, :, :50]), dict(stats=stats.cpu()),
                dict(tile_seg=seg[:2]), dict(tile_n=cnt.long()), dict(tile_seg=seg.cpu()), dict(tile_n=cnt[:2])):
        kw = dict(dict(tile_seg=seg, tile_n=cnt, stats=stats), **bad)
        with pytest.raises(_abi.SpvError, match="expected_expression_stats"):
            _stats(c, BN, kw["tile_seg"], kw["tile_n"], 2, kw["stats"])
    with pytest.raises(ValueError, match="n_seg"):
        _stats(c, BN, seg, cnt, 0, stats)
    with pytest.raises(IndexError, match=str(G1)):
        _stats(c, BN, seg, cnt, 2, stats, genes=[0, G1])
    with pytest.raises(_abi.SpvError, match="library override"):
        _stats(c, BN, seg, cnt, 2, stats, log_library=torch.zeros(BN - 1, device=c.dev))
    assert not bool(stats.any())   # nothing was launched


def test_training_mode_is_refused(case):
    from spvipes_amd import _abi, dec_ops
    c = case
    m, g = c.module, c.g
    stats = torch.zeros((1, 8, G1), dtype=torch.float64, device=c.dev)
    seg, cnt = torch.zeros(3, dtype=torch.int32, device=c.dev), torch.full((3,), 32, dtype=torch.int32, device=c.dev)
    with pytest.raises(_abi.SpvError, match="eval mode"):
        dec_ops.expected_expression_stats(m.decoders[g], m.px_r[g], c.first, c.second, c.lib, True, m.nsplit, m._workspace(g, c.dev), par=c.par,
                                          tile_seg=seg, tile_n=cnt, n_seg=1, stats=stats)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            m.expression_stats({}, g, perm=torch.arange(BN, device=c.dev), tile_seg=seg, tile_n=cnt, n_seg=1, stats=stats)
    finally:
        m.eval()
    assert not bool(stats.any())
