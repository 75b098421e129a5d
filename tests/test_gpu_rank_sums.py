"""GPU: spv_rank_stage / spv_rank_sums through spvipes_amd.rank_ops.rank_sums, against tests/_rank_reference.py.

Every device output is an integer (doubled midranks, t^3 - t), so every comparison here is EQUALITY of whole tables: there is no
tolerance and nothing is left out.  Shapes are the smallest that reach each hazard: n = 1, 2 and one below / at / above the ballot
width (64), the stage tile, the radix tile and the capacity of the LDS-resident sort (taken from the library's shape functions), with
columns whose number of NON-ZERO keys -- what is sorted -- sits exactly at those sizes."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests._rank_reference import keys_of, rank_tables  # noqa: E402

SENTINEL = 60000
DEV = "cuda"


def _lib_sizes():
    from spvipes_amd import rank_ops

    return rank_ops.rank_stage_tile(), rank_ops.rank_sort_tile(), rank_ops.rank_lds_capacity()


def _matrix(rng, n_rows, G, dtype, col_off=0, pad=0):
    """the host matrix [n_rows, col_off + G + pad] (sentinels outside the group's own genes) with the genes 0..5 made to measure:
    0 all distinct and non-zero | 1 distinct, zero in row 0 only | 2 distinct, zero in rows 0 and 1 | 3 all zero | 4 all equal and
    non-zero | 5 one non-zero | 6.. about 70 % zeros, small counts (heavy ties)"""
    assert G >= 8 and n_rows < 65535
    own = rng.integers(1, 6, (n_rows, G)) * (rng.random((n_rows, G)) < 0.3)
    r = np.arange(n_rows)
    own[:, 0], own[:, 1], own[:, 2], own[:, 3], own[:, 4], own[:, 5] = r + 1, r, np.maximum(r - 1, 0), 0, 7, 0
    own[n_rows // 2, 5] = 3
    if dtype == "u16":
        X = np.full((n_rows, col_off + G + pad), SENTINEL, np.uint16)
        X[:, col_off:col_off + G] = own.astype(np.uint16)
    else:
        X = np.full((n_rows, col_off + G + pad), float(SENTINEL), np.float32)
        X[:, col_off:col_off + G] = own.astype(np.float32) * np.float32(0.25)
    return X


def _device_counts(X, G, col_off, storage):
    from spvipes_amd.ops import GroupCounts, SparseGroupCounts

    t = torch.from_numpy(X.view(np.int16) if X.dtype == np.uint16 else X).to(DEV)
    dense = GroupCounts(t, G, col_off)
    return dense if storage == "dense" else SparseGroupCounts.from_dense(dense)


def _run(X, G, col_off, rows, seg, n_seg, w=None, genes=None, storage="dense"):
    from spvipes_amd.rank_ops import rank_sums

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    rank2, ties = rank_sums(_device_counts(X, G, col_off, storage), dev(rows), dev(seg), n_seg, w=dev(w), genes=dev(genes))
    assert rank2.dtype == torch.int64 and ties.dtype == torch.int64
    return rank2.cpu().numpy(), ties.cpu().numpy()


def _want(X, G, col_off, rows, seg, n_seg, w=None, genes=None):
    own = X[:, col_off:col_off + G][rows]
    if genes is not None:
        own = own[:, genes]
    return rank_tables(keys_of(own, w), seg, n_seg)


def _check(got, want, ctx):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, ctx
    assert (got[0] == want[0]).all(), f"{ctx}: rank2 differs in {(got[0] != want[0]).sum()} of {want[0].size} entries"
    assert (got[1] == want[1]).all(), f"{ctx}: ties differ in {(got[1] != want[1]).sum()} of {want[1].size} genes"


def _sizes():
    """n: 1, 2, and one below / at / above the ballot width, the stage tile, twice the stage tile, the radix tile and the LDS capacity --
    taken from the library's shape functions -- and a length of several radix tiles with a part"""
    tile, sort_tile, cap = _lib_sizes()
    out = [1, 2]
    for edge in sorted({64, tile, 2 * tile, sort_tile, cap}):
        out += [edge - 1, edge, edge + 1]
    return out + [cap + 2 * sort_tile + 37]


def test_the_library_reports_its_sizes():
    from spvipes_amd import _abi

    tile, sort_tile, cap = _lib_sizes()
    assert tile >= 64 and tile % 64 == 0 and sort_tile % 64 == 0 and cap >= sort_tile and cap & (cap - 1) == 0
    assert int(_abi.load().spv_rank_gene_slab()) >= 70   # the one-slab case below holds 70 genes


@functools.lru_cache(maxsize=None)
def _size_case(n, dtype, weighted):
    """each listed cell once, in a shuffled order: gene 0 has n non-zero keys, gene 1 has n - 1, gene 2 has n - 2 -- with n one above
    the LDS capacity the three columns sit above, at and below the switch between the sort paths"""
    rng = np.random.default_rng(n * 13 + (dtype == "f32") + 2 * weighted)
    X = _matrix(rng, n, 9, dtype)
    rows = rng.permutation(n).astype(np.int32)
    seg = rng.integers(0, 3, n).astype(np.int32)
    w = (rng.integers(1, 4, n) * 0.5).astype(np.float32) if weighted else None   # non-zero: the sorted lengths stay n, n - 1, n - 2
    return X, rows, seg, w, _want(X, 9, 0, rows, seg, 3, w)


def test_every_size_edge_raw_counts():
    """the edges move with the library: they are computed from its shape functions here, not listed"""
    for n in _sizes():
        X, rows, seg, w, want = _size_case(n, "u16", False)
        _check(_run(X, 9, 0, rows, seg, 3), want, f"n {n}")


def test_size_edges_weighted_fp32_counts():
    tile, sort_tile, cap = _lib_sizes()
    for n in (1, 2, tile - 1, tile + 1, sort_tile + 1, cap - 1, cap, cap + 1, cap + 2 * sort_tile + 37):
        X, rows, seg, w, want = _size_case(n, "f32", True)
        _check(_run(X, 9, 0, rows, seg, 3, w=w), want, f"n {n}")


def test_radix_passes_that_are_skipped_and_passes_that_run():
    """beyond the LDS capacity: raw uint16 counts as fp32 keys -- gene 0 (all distinct) has a constant low byte, so pass 0 is skipped and
    the other three run; gene 4 (all equal) has every digit constant, so all four are skipped -- and, weighted, keys that differ in every
    byte (all four passes run)"""
    cap = _lib_sizes()[2]
    n = cap + 700
    X, rows, seg, w, want = _size_case(n, "u16", False)
    keys = keys_of(X[rows][:, [0, 4]]).view(np.uint32)
    assert ((keys[:, 0] & 0xFF) == 0).all() and all(len(np.unique((keys[:, 0] >> s) & 255)) > 1 for s in (8, 16, 24))
    assert len(np.unique(keys[:, 1])) == 1 and keys[0, 1] != 0
    _check(_run(X, 9, 0, rows, seg, 3), want, "skipped passes")
    rng = np.random.default_rng(31)
    w = (rng.random(n) + 0.5).astype(np.float32)
    keys = keys_of(X[rows][:, :1], w).view(np.uint32)
    assert all(len(np.unique((keys >> s) & 255)) > 1 for s in (0, 8, 16, 24))
    _check(_run(X, 9, 0, rows, seg, 3, w=w), _want(X, 9, 0, rows, seg, 3, w), "no pass skipped")


def test_more_genes_than_one_stage_tile_in_one_slab():
    """70 genes in ONE call: the stage's second gene tile (its gene offset, no segment tally of its own), a selection and all genes"""
    from spvipes_amd import rank_ops

    rng = np.random.default_rng(41)
    G, n_rows, n = 70, 150, 300
    assert rank_ops.rank_gene_slab(n) >= G
    X = _matrix(rng, n_rows, G, "u16", col_off=1, pad=1)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    seg = rng.integers(-1, 5, n).astype(np.int32)
    w = (rng.random(n) * 2).astype(np.float32)
    _check(_run(X, G, 1, rows, seg, 4, w=w), _want(X, G, 1, rows, seg, 4, w), "70 genes, all")
    genes = rng.permutation(G)[:67].astype(np.int32)
    _check(_run(X, G, 1, rows, seg, 4, w=w, genes=genes), _want(X, G, 1, rows, seg, 4, w, genes), "67 selected genes")


def test_sorted_lengths_at_the_switch_point_take_both_paths():
    """what the case above relies on: with n = capacity + 1 the columns 0, 1, 2 hold capacity + 1, capacity and capacity - 1 non-zero keys"""
    cap = _lib_sizes()[2]
    X, rows, _seg, _w, _want_ = _size_case(cap + 1, "u16", False)
    assert [(X[rows][:, j] != 0).sum() for j in (0, 1, 2)] == [cap + 1, cap, cap - 1]


@functools.lru_cache(maxsize=None)
def _general_case(dtype):
    """600 listed positions over 211 cells: shuffled, with repeats, a col_off and a padded pitch"""
    rng = np.random.default_rng(77 + (dtype == "f32"))
    G, col_off, n, n_rows = 40, 3, 600, 211
    X = _matrix(rng, n_rows, G, dtype, col_off, pad=2)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    rows[1] = rows[0]
    w = (rng.random(n) * 3).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.0
    return X, G, col_off, rows, w


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("weighted", [False, True])
def test_shuffled_rows_with_repeats_col_off_and_zero_weights(dtype, weighted):
    X, G, col_off, rows, w = _general_case(dtype)
    seg = np.random.default_rng(3).integers(0, 5, len(rows)).astype(np.int32)
    w = w if weighted else None
    assert not weighted or (w == 0).any()
    _check(_run(X, G, col_off, rows, seg, 5, w=w), _want(X, G, col_off, rows, seg, 5, w), f"{dtype} weighted {weighted}")


def test_different_counts_whose_fp32_products_collide():
    rng = np.random.default_rng(9)
    n, G = 300, 8
    X = np.zeros((n, G), np.uint16)
    X[:, :] = rng.integers(0, 7, (n, G))
    w = rng.choice(np.array([1.0, 1.5, 1.0 / 3.0, 0.5, 2.0 / 3.0], np.float32), n)
    rows = np.arange(n, dtype=np.int32)
    keys = keys_of(X, w)
    c = X[:, 0].astype(np.int64)
    assert ((keys[:, 0][:, None] == keys[:, 0][None, :]) & (c[:, None] != c[None, :]) & (keys[:, 0][:, None] != 0)).any()   # e.g. 2 * 1.5 and 3 * 1.0
    assert np.float32(3) * np.float32(1.0 / 3.0) == np.float32(1)                                                               # and one made by rounding
    seg = rng.integers(0, 2, n).astype(np.int32)
    _check(_run(X, G, 0, rows, seg, 2, w=w), rank_tables(keys, seg, 2), "colliding products")


@pytest.mark.parametrize("n_seg", [1, 1024])
def test_segment_edges(n_seg):
    """one segment; 1024 segments with an empty one, a one-cell one, and codes outside [0, n_seg) that are ranked but counted nowhere"""
    X, G, col_off, rows, w = _general_case("u16")
    rng = np.random.default_rng(n_seg)
    n = len(rows)
    if n_seg == 1:
        seg = np.zeros(n, np.int32)
        seg[::7] = np.array([-1, 1, 5000, -2**31, 2**31 - 1], np.int64)[np.arange(len(seg[::7])) % 5].astype(np.int32)
    else:
        seg = rng.integers(2, n_seg, n).astype(np.int32)   # segment 0 stays empty
        seg[::11] = np.array([-1, n_seg, n_seg + 7], np.int32)[np.arange(len(seg[::11])) % 3]
        seg[seg == 1] = 2
        seg[5], seg[6] = 1, 1023                            # segment 1 has one cell; the last segment is used
        assert (seg == 0).sum() == 0 and (seg == 1).sum() == 1 and (seg == 1023).any()
    want = _want(X, G, col_off, rows, seg, n_seg, w)
    got = _run(X, G, col_off, rows, seg, n_seg, w=w)
    _check(got, want, f"n_seg {n_seg}")
    if n_seg == 1024:
        assert (got[0][0] == 0).all() and (got[0][1] > 0).all()


def test_gene_selection_with_repeats_and_across_a_slab_boundary(monkeypatch):
    """a selected column equals the same column of the all-genes call; with the workspace budget cut to 16 genes' worth the 40 genes
    (and a selection of 70 with repeats) cross gene-slab boundaries"""
    from spvipes_amd import rank_ops

    X, G, col_off, rows, w = _general_case("u16")
    seg = np.random.default_rng(4).integers(0, 4, len(rows)).astype(np.int32)
    assert rank_ops.rank_gene_slab(len(rows)) >= G
    whole = _run(X, G, col_off, rows, seg, 4, w=w)
    _check(whole, _want(X, G, col_off, rows, seg, 4, w), "all genes, one slab")
    monkeypatch.setattr(rank_ops, "WS_BUDGET_BYTES", 16 * len(rows) * 16)
    assert rank_ops.rank_gene_slab(len(rows)) == 16
    _check(_run(X, G, col_off, rows, seg, 4, w=w), whole, "all genes, three slabs")
    genes = np.random.default_rng(5).integers(0, G, 70).astype(np.int32)
    genes[:3] = [39, 39, 0]
    got = _run(X, G, col_off, rows, seg, 4, w=w, genes=genes)
    _check(got, (whole[0][:, genes], whole[1][genes]), "selection with repeats over five slabs")


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_csr_equals_dense_bit_for_bit_across_a_chunk_boundary(dtype):
    from spvipes_amd.rank_ops import COUNT_CHUNK_ROWS

    rng = np.random.default_rng(21 + (dtype == "f32"))
    n_rows, G = 900, 10
    n = COUNT_CHUNK_ROWS + 300
    X = _matrix(rng, n_rows, G, dtype)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    seg = rng.integers(0, 6, n).astype(np.int32)
    w = (rng.random(n) * 2).astype(np.float32)
    dense = _run(X, G, 0, rows, seg, 6, w=w)
    sparse = _run(X, G, 0, rows, seg, 6, w=w, storage="sparse")
    _check(sparse, dense, "csr against dense")
    _check(dense, _want(X, G, 0, rows, seg, 6, w), "dense against the reference")


def test_two_calls_agree_bit_for_bit():
    X, rows, seg, w, want = _size_case(_sizes()[-1], "f32", True)
    a, b = _run(X, 9, 0, rows, seg, 3, w=w), _run(X, 9, 0, rows, seg, 3, w=w)
    _check(a, b, "two calls")


def test_sentinels_beside_the_tables_and_behind_the_workspace_survive():
    """the ABI directly: rank2 with a pitch of n_sel + 3, ties and the workspace with sentinel bytes behind what the contract lets be touched"""
    from spvipes_amd import _abi
    from spvipes_amd.ops import GroupCounts

    X, G, col_off, rows, w = _general_case("u16")
    n, n_seg, n_sel = len(rows), 5, G
    seg = np.random.default_rng(8).integers(0, n_seg, n).astype(np.int32)
    counts = GroupCounts(torch.from_numpy(X.view(np.int16)).to(DEV), G, col_off)
    need = int(_abi.load().spv_rank_ws_bytes(n, n_sel))
    assert need == 8192 + 16 * n * n_sel
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    table = torch.full((n_seg, n_sel + 3), -77, dtype=torch.int64, device=DEV)
    ties = torch.full((n_sel + 2,), -77, dtype=torch.int64, device=DEV)
    rows_d, seg_d, w_d = (torch.from_numpy(v).to(DEV) for v in (rows, seg, w))
    a = _abi.SpvRankArgs()
    a.x, a.G, a.n_rows, a.n_piece, a.pos_off, a.n, a.n_seg, a.n_sel, a.reset = counts.c_struct(rows_d), G, counts.n_cells, n, 0, n, n_seg, n_sel, 1
    a.seg, a.w, a.genes, a.rank2, a.ld_rank2, a.ties, a.ws, a.ws_bytes = seg_d.data_ptr(), w_d.data_ptr(), None, table.data_ptr(), n_sel + 3, ties.data_ptr(), ws.data_ptr(), need
    _abi.call("spv_rank_stage", C.byref(a), _abi.stream_ptr())
    _abi.call("spv_rank_sums", C.byref(a), _abi.stream_ptr())
    torch.cuda.synchronize()
    want = _want(X, G, col_off, rows, seg, n_seg, w)
    _check((table[:, :n_sel].cpu().numpy(), ties[:n_sel].cpu().numpy()), want, "direct call")
    assert (table[:, n_sel:] == -77).all() and (ties[n_sel:] == -77).all() and (ws[need:] == 0x5A).all()


def test_host_refusals_come_before_any_launch():
    from spvipes_amd import _abi
    from spvipes_amd.rank_ops import rank_sums

    X, G, col_off, rows, w = _general_case("u16")
    counts = _device_counts(X, G, col_off, "dense")
    r, s = torch.from_numpy(rows).to(DEV), torch.zeros(len(rows), dtype=torch.int32, device=DEV)
    bad = r.clone()
    bad[3] = counts.n_cells
    with pytest.raises(ValueError, match="rows must lie"):
        rank_sums(counts, bad, s, 1)
    with pytest.raises(ValueError, match="n_seg"):
        rank_sums(counts, r, s, 1025)
    with pytest.raises(_abi.SpvError, match="seg"):
        rank_sums(counts, r, s[:-1].contiguous(), 1)
    with pytest.raises(_abi.SpvError, match="w must"):
        rank_sums(counts, r, s, 1, w=torch.ones(len(rows), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="genes must lie"):
        rank_sums(counts, r, s, 1, genes=torch.tensor([0, G], dtype=torch.int32, device=DEV))
