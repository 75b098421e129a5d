"""GPU: spv_rank_values_stage / spv_rank_values through spvipes_amd.rank_ops.rank_transform, and spv_gram_f64 on the block it writes,
against tests/_spearman_reference.py.

Every device output is an integer (doubled midranks minus n + 1, t^3 - t, and -- below 208 063 rows -- every sum of products), so every
comparison here is EQUALITY of whole arrays: there is no tolerance and nothing is left out.  ``_check`` holds EVERY case of this file to
the block c, the tie terms T, and the Gram: S exactly 0 and C == c.T @ c in int64.  Shapes are the smallest that reach each hazard: n = 1,
2 and one below / at / above the ballot width (64), the stage tile, twice the stage tile, the radix tile and the capacity of the
LDS-resident sort (taken from the library's shape functions), with columns whose number of NON-ZERO keys -- what is sorted -- sits exactly
at those sizes; one list of 70 001 positions, whose position words need more than 16 bits on the radix route."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests._rank_reference import keys_of  # noqa: E402
from tests._spearman_reference import spearman_tables  # noqa: E402
from tests.test_gpu_rank_sums import _device_counts, _lib_sizes, _matrix, _sizes  # noqa: E402

DEV = "cuda"
PAD = -12345.0


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(X, G, col_off, rows, w=None, genes=None, storage="dense", out=None):
    from spvipes_amd.rank_ops import rank_transform

    block, ties = rank_transform(_device_counts(X, G, col_off, storage), _dev(rows), w=_dev(w), genes=_dev(genes), out=out, ties=True)
    assert block.dtype == torch.float32 and ties.dtype == torch.int64 and block.shape == (len(rows), G if genes is None else len(genes))
    return block, ties


def _keys(X, G, col_off, rows, w=None, genes=None):
    own = X[:, col_off:col_off + G][rows]
    if genes is not None:
        own = own[:, genes]
    return keys_of(own, w)


def _gram(block):
    from spvipes_amd.gram_ops import gram_accumulate

    p = block.shape[1]
    S = torch.zeros(p, dtype=torch.float64, device=DEV)
    Cm = torch.zeros((p, p), dtype=torch.float64, device=DEV)
    gram_accumulate(block, sums=S, gram=Cm)
    return S.cpu().numpy(), Cm.cpu().numpy()


def _check(got, keys, ctx):
    """the block, the ties and the block's Gram against the int64 reference of ``keys``: equality of whole arrays"""
    block, ties = got
    c, Cm, T = spearman_tables(keys)
    n = keys.shape[0]
    assert n ** 3 < 2 ** 53   # every sum of products is an exact integer in fp64
    b = block.cpu().numpy()
    assert b.shape == c.shape, ctx
    assert (b == c).all(), f"{ctx}: the block differs in {(b != c).sum()} of {c.size} entries"
    assert (ties.cpu().numpy() == T).all(), f"{ctx}: ties differ in {(ties.cpu().numpy() != T).sum()} of {T.size} genes"
    S, G2 = _gram(block)
    assert (S == 0.0).all(), f"{ctx}: a column does not sum to 0"
    assert (G2 == Cm.astype(np.float64)).all() and (G2.astype(np.int64) == Cm).all(), f"{ctx}: the Gram differs in {(G2 != Cm).sum()} of {Cm.size} entries"
    return b


@functools.lru_cache(maxsize=None)
def _size_case(n, dtype, weighted):
    """each listed cell once, in a shuffled order: gene 0 has n non-zero keys, gene 1 has n - 1, gene 2 has n - 2 -- with n one above
    the LDS capacity the three columns sit above, at and below the switch between the sort paths; genes 3 all zero, 4 all equal, 5 one
    non-zero, 6.. heavy ties"""
    rng = np.random.default_rng(n * 17 + (dtype == "f32") + 2 * weighted)
    X = _matrix(rng, n, 9, dtype)
    rows = rng.permutation(n).astype(np.int32)
    w = (rng.integers(1, 4, n) * 0.5).astype(np.float32) if weighted else None   # non-zero: the sorted lengths stay n, n - 1, n - 2
    return X, rows, w


def test_every_size_edge_raw_counts():
    """the edges move with the library: they are computed from its shape functions here, not listed"""
    for n in _sizes():
        X, rows, w = _size_case(n, "u16", False)
        _check(_run(X, 9, 0, rows), _keys(X, 9, 0, rows), f"n {n}")


def test_size_edges_weighted_fp32_counts():
    tile, sort_tile, cap = _lib_sizes()
    for n in (1, 2, 63, 65, tile - 1, tile + 1, 2 * tile + 1, sort_tile + 1, cap - 1, cap, cap + 1, cap + 2 * sort_tile + 37):
        X, rows, w = _size_case(n, "f32", True)
        _check(_run(X, 9, 0, rows, w=w), _keys(X, 9, 0, rows, w), f"n {n}")


def test_positions_beyond_16_bits_on_the_radix_route():
    """70 001 positions, 3 genes, fp32: all distinct and non-zero (radix, every position word up to 70 000 comes back); 10 % non-zero
    (the zero run's fill, then an LDS sort of ~7000 entries scattered over the whole column); heavy ties, all non-zero (radix)"""
    rng = np.random.default_rng(70001)
    n = 70001
    X = np.zeros((n, 3), np.float32)
    X[:, 0] = (rng.permutation(n) + 1) * np.float32(0.25)
    X[:, 1] = rng.integers(1, 9, n) * (rng.random(n) < 0.1)
    X[:, 2] = rng.integers(1, 5, n)
    rows = rng.permutation(n).astype(np.int32)
    assert _lib_sizes()[2] < (X[:, 0] != 0).sum() and (X[:, 1] != 0).sum() < _lib_sizes()[2] and rows.max() > 65535
    b = _check(_run(X, 3, 0, rows), _keys(X, 3, 0, rows), "n 70001")
    assert b[:, 0].min() == -(n - 1) and b[:, 0].max() == n - 1


def test_radix_passes_that_are_skipped_and_passes_that_run():
    """beyond the LDS capacity: raw uint16 counts as fp32 keys -- gene 0 (all distinct) has a constant low byte, so pass 0 is skipped and
    the other three run; gene 4 (all equal) has every digit constant, so all four are skipped -- and, weighted, keys that differ in every
    byte (all four passes run)"""
    cap = _lib_sizes()[2]
    n = cap + 700
    X, rows, _w = _size_case(n, "u16", False)
    bits = keys_of(X[rows][:, [0, 4]]).view(np.uint32)
    assert ((bits[:, 0] & 0xFF) == 0).all() and all(len(np.unique((bits[:, 0] >> s) & 255)) > 1 for s in (8, 16, 24))
    assert len(np.unique(bits[:, 1])) == 1 and bits[0, 1] != 0
    b = _check(_run(X, 9, 0, rows), _keys(X, 9, 0, rows), "skipped passes")
    assert (b[:, 4] == 0).all() and (b[:, 3] == 0).all()   # all equal / all zero: every rank is the middle one
    w = (np.random.default_rng(31).random(n) + 0.5).astype(np.float32)
    bits = keys_of(X[rows][:, :1], w).view(np.uint32)
    assert all(len(np.unique((bits >> s) & 255)) > 1 for s in (0, 8, 16, 24))
    _check(_run(X, 9, 0, rows, w=w), _keys(X, 9, 0, rows, w), "no pass skipped")


@functools.lru_cache(maxsize=None)
def _general_case(dtype):
    """600 listed positions over 211 cells: shuffled, with repeats, a col_off and a padded pitch with sentinels, weights with zeros"""
    rng = np.random.default_rng(79 + (dtype == "f32"))
    G, col_off, n, n_rows = 70, 3, 600, 211
    X = _matrix(rng, n_rows, G, dtype, col_off, pad=2)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    rows[1] = rows[0]
    w = (rng.random(n) * 3).astype(np.float32)
    w[rng.random(n) < 0.1] = 0.0
    return X, G, col_off, rows, w


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("weighted", [False, True])
def test_shuffled_rows_with_repeats_col_off_sentinels_and_zero_weights(dtype, weighted):
    """70 genes in ONE call: the stage's and the store's second gene tile"""
    X, G, col_off, rows, w = _general_case(dtype)
    w = w if weighted else None
    assert not weighted or (w == 0).any()
    _check(_run(X, G, col_off, rows, w=w), _keys(X, G, col_off, rows, w), f"{dtype} weighted {weighted}")


@pytest.mark.parametrize("n_sel", [1, 63, 64, 65])
def test_gene_lists_with_repeats_around_the_store_tile(n_sel):
    X, G, col_off, rows, w = _general_case("u16")
    genes = np.random.default_rng(n_sel).integers(0, G, n_sel).astype(np.int32)
    if n_sel > 2:
        genes[:3] = [G - 1, G - 1, 0]
    _check(_run(X, G, col_off, rows, w=w, genes=genes), _keys(X, G, col_off, rows, w, genes), f"n_sel {n_sel}")


def test_three_gene_slabs_equal_one(monkeypatch):
    from spvipes_amd import rank_ops

    X, G, col_off, rows, w = _general_case("u16")
    genes = np.arange(40, dtype=np.int32)
    assert rank_ops.rank_values_gene_slab(len(rows)) >= 40
    whole = _run(X, G, col_off, rows, w=w, genes=genes)
    _check(whole, _keys(X, G, col_off, rows, w, genes), "one slab")
    monkeypatch.setattr(rank_ops, "WS_BUDGET_BYTES", 16 * len(rows) * 20)
    assert rank_ops.rank_values_gene_slab(len(rows)) == 16   # 40 genes: slabs of 16, 16 and 8
    parts = _run(X, G, col_off, rows, w=w, genes=genes)
    assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1])
    _check(parts, _keys(X, G, col_off, rows, w, genes), "three slabs")
    sub = _run(X, G, col_off, rows, w=w)   # all 70 genes without a list: five slabs, the later ones through a made-up list
    assert torch.equal(sub[0][:, :40], whole[0])


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_csr_equals_dense_bit_for_bit_across_a_chunk_boundary(dtype):
    from spvipes_amd.rank_ops import COUNT_CHUNK_ROWS

    rng = np.random.default_rng(23 + (dtype == "f32"))
    n_rows, G = 900, 10
    n = COUNT_CHUNK_ROWS + 300
    X = _matrix(rng, n_rows, G, dtype)
    rows = rng.integers(0, n_rows, n).astype(np.int32)
    w = (rng.random(n) * 2).astype(np.float32)
    dense = _run(X, G, 0, rows, w=w)
    sparse = _run(X, G, 0, rows, w=w, storage="sparse")
    assert torch.equal(dense[0], sparse[0]) and torch.equal(dense[1], sparse[1])
    _check(dense, _keys(X, G, 0, rows, w), "dense against the reference")


def test_in_place_equals_out_of_place_and_other_overlaps_are_refused():
    from spvipes_amd.ops import GroupCounts
    from spvipes_amd.rank_ops import rank_transform

    cap = _lib_sizes()[2]
    n = cap + 300
    X, _rows, _w = _size_case(n, "f32", False)
    rows = np.arange(n, dtype=np.int32)
    apart = _run(X, 9, 0, rows)
    _check(apart, _keys(X, 9, 0, rows), "out of place")
    t = _dev(X)
    back = rank_transform(GroupCounts(t, 9, 0), _dev(rows), out=t)
    assert back.data_ptr() == t.data_ptr() and torch.equal(t, apart[0])
    t = _dev(X)
    counts = GroupCounts(t, 9, 0)
    with pytest.raises(ValueError, match="overlaps the matrix"):   # a shuffled list
        rank_transform(counts, _dev(rows[::-1].copy()), out=t)
    with pytest.raises(ValueError, match="overlaps the matrix"):   # a gene list
        rank_transform(counts, _dev(rows), genes=_dev(np.arange(9, dtype=np.int32)), out=t)
    with pytest.raises(ValueError, match="overlaps the matrix"):   # a col_off
        rank_transform(GroupCounts(t, 8, 1), _dev(rows), out=t[:, :8])
    assert torch.equal(t, _dev(X))   # nothing was launched


def test_a_padded_out_keeps_its_padding():
    X, G, col_off, rows, w = _general_case("f32")
    n = len(rows)
    big = torch.full((n, G + 5), PAD, dtype=torch.float32, device=DEV)
    got = _run(X, G, col_off, rows, w=w, out=big[:, :G])
    assert got[0].data_ptr() == big.data_ptr() and (big[:, G:] == PAD).all()
    _check(got, _keys(X, G, col_off, rows, w), "ld_out = n_sel + 5")


def test_ties_equal_rank_sums_ties_and_two_calls_agree_in_bits():
    from spvipes_amd.rank_ops import rank_sums

    n = _sizes()[-1]
    X, rows, w = _size_case(n, "f32", True)
    a, b = _run(X, 9, 0, rows, w=w), _run(X, 9, 0, rows, w=w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    seg = torch.zeros(n, dtype=torch.int32, device=DEV)
    _rank2, ties = rank_sums(_device_counts(X, 9, 0, "dense"), _dev(rows), seg, 1, w=_dev(w))
    assert torch.equal(ties, a[1])


def test_sentinels_beside_the_outputs_and_behind_the_workspace_survive():
    """the ABI directly: out with a pitch of n_sel + 3, ties, nonzero and the workspace with sentinels behind what the contract lets be touched"""
    from spvipes_amd import _abi
    from spvipes_amd.ops import GroupCounts

    X, G, col_off, rows, w = _general_case("u16")
    n, n_sel = len(rows), G
    counts = GroupCounts(torch.from_numpy(X.view(np.int16)).to(DEV), G, col_off)
    need = int(_abi.load().spv_rank_values_ws_bytes(n, n_sel))
    assert need == 8192 + 20 * n * n_sel
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full((n, n_sel + 3), PAD, dtype=torch.float32, device=DEV)
    ties = torch.full((n_sel + 2,), -77, dtype=torch.int64, device=DEV)
    nonzero = torch.full((n_sel + 2,), -77, dtype=torch.int32, device=DEV)
    rows_d, w_d = _dev(rows), _dev(w)
    a = _abi.SpvRankValuesArgs()
    a.x, a.G, a.n_rows, a.n_piece, a.pos_off, a.n, a.n_sel, a.reset = counts.c_struct(rows_d), G, counts.n_cells, n, 0, n, n_sel, 1
    a.w, a.genes, a.out, a.ld_out, a.ties, a.nonzero, a.ws, a.ws_bytes = w_d.data_ptr(), None, out.data_ptr(), n_sel + 3, ties.data_ptr(), nonzero.data_ptr(), ws.data_ptr(), need
    _abi.call("spv_rank_values_stage", C.byref(a), _abi.stream_ptr())
    _abi.call("spv_rank_values", C.byref(a), _abi.stream_ptr())
    torch.cuda.synchronize()
    keys = _keys(X, G, col_off, rows, w)
    _check((out[:, :n_sel].contiguous(), ties[:n_sel]), keys, "direct call")
    assert (nonzero[:n_sel].cpu().numpy() == (keys != 0).sum(0)).all()
    assert (out[:, n_sel:] == PAD).all() and (ties[n_sel:] == -77).all() and (nonzero[n_sel:] == -77).all() and (ws[need:] == 0x5A).all()


def test_host_refusals_come_before_any_launch():
    from spvipes_amd import _abi
    from spvipes_amd.ops import GroupCounts
    from spvipes_amd.rank_ops import rank_transform

    X, G, col_off, rows, w = _general_case("f32")
    counts = _device_counts(X, G, col_off, "dense")
    r = _dev(rows)
    bad = r.clone()
    bad[3] = counts.n_cells
    with pytest.raises(ValueError, match="rows must lie"):
        rank_transform(counts, bad)
    with pytest.raises(ValueError, match="genes must lie"):
        rank_transform(counts, r, genes=torch.tensor([0, G], dtype=torch.int32, device=DEV))
    with pytest.raises(_abi.SpvError, match="w must"):
        rank_transform(counts, r, w=torch.ones(len(rows), dtype=torch.float64, device=DEV))
    with pytest.raises(_abi.SpvError, match="out must"):
        rank_transform(counts, r, out=torch.empty((len(rows), G + 1), dtype=torch.float32, device=DEV))
    for poison in (-0.25, float("nan")):
        Y = X.copy()
        Y[7, col_off + 2] = poison
        with pytest.raises(ValueError, match="non-negative"):
            rank_transform(GroupCounts(_dev(Y), G, col_off), r)
