"""CPU: the host side of spVIPES.expression_statistics -- ``data.expression_tile_plan`` (the arrangement of a step's cells into
single-segment tiles) on hand-made and random code vectors, ``data.expression_stats_table`` against numpy on synthetic sums, and the
signatures and argument errors of every layer.  No GPU calls."""
import inspect

import numpy as np
import pytest

TILE = 32


def _check_plan(seg, n_seg, tile=TILE):
    """every property the kernel relies on -> (perm, tile_seg, tile_n)"""
    from spvipes_amd.data import expression_tile_plan
    seg = np.asarray(seg)
    perm, tile_seg, tile_n = expression_tile_plan(seg, n_seg, tile)
    assert perm.dtype == np.int64 and tile_seg.dtype == np.int32 and tile_n.dtype == np.int32
    assert perm.ndim == tile_seg.ndim == tile_n.ndim == 1
    assert perm.size % tile == 0 and tile_seg.size == tile_n.size == perm.size // tile
    counted = np.nonzero((seg >= 0) & (seg < n_seg))[0] if seg.size else np.zeros(0, dtype=np.int64)
    if not counted.size:
        assert perm.size == 0
        return perm, tile_seg, tile_n
    assert perm.min() >= 0 and perm.max() < seg.size                      # padding slots hold a valid index too
    assert np.isin(perm, counted).all()                                   # uncounted cells never appear, not even as padding
    assert ((tile_n >= 1) & (tile_n <= tile)).all()
    assert (np.diff(tile_seg) >= 0).all()                                 # segments in ascending order
    assert set(tile_seg.tolist()) == set(seg[counted].tolist())           # exactly the segments present
    slots = perm.reshape(-1, tile)
    mask = np.arange(tile)[None, :] < tile_n[:, None]                     # the counted slots
    assert (seg[slots] == tile_seg[:, None]).all()                        # every tile is single-segment, padding included
    np.testing.assert_array_equal(np.sort(slots[mask]), counted)          # every counted cell exactly once among the counted slots
    for k in np.unique(tile_seg):
        tiles = np.nonzero(tile_seg == k)[0]
        assert (np.diff(tiles) == 1).all() and (tile_n[tiles[:-1]] == tile).all()   # one run; only its last tile is partial
        run = slots[tiles]
        np.testing.assert_array_equal(run[mask[tiles]], np.nonzero(seg == k)[0])   # walk order within the segment
        assert (run[~mask[tiles]] == run[0, 0]).all()                     # the padding repeats the run's first cell
    return perm, tile_seg, tile_n


def test_tile_plan_on_hand_made_codes():
    # segment sizes 1, 32, 33 and 64; segment 2 absent; codes -1 and >= n_seg are left out
    seg = np.concatenate([np.full(33, 4), [-1], np.full(64, 0), [7, 9], np.full(1, 1), np.full(32, 3), [-5]])
    rng = np.random.default_rng(0)
    seg = seg[rng.permutation(seg.size)]
    perm, tile_seg, tile_n = _check_plan(seg, 5)
    np.testing.assert_array_equal(tile_seg, [0, 0, 1, 3, 4, 4])
    np.testing.assert_array_equal(tile_n, [32, 32, 1, 32, 32, 1])
    assert perm.size == 6 * TILE
    # a small example written out in full (tile = 4)
    perm, tile_seg, tile_n = _check_plan([1, -1, 0, 1, 1, 3, 1, 1], 2, tile=4)
    np.testing.assert_array_equal(perm, [2, 2, 2, 2, 0, 3, 4, 6, 7, 0, 0, 0])
    np.testing.assert_array_equal(tile_seg, [0, 1, 1])
    np.testing.assert_array_equal(tile_n, [1, 4, 1])
    # the default tile is the kernel's 32 cells
    from spvipes_amd import dec_ops
    from spvipes_amd.data import expression_tile_plan
    assert inspect.signature(expression_tile_plan).parameters["tile"].default == dec_ops.EXPRESSION_TILE == 32


def test_tile_plan_empty_steps_and_single_sizes():
    for seg in ([], [-1, -1, -1], [5, 6], np.full(40, 2)):
        perm, tile_seg, tile_n = _check_plan(np.asarray(seg, dtype=np.int64), 2)
        assert perm.size == 0 and tile_seg.size == 0 and tile_n.size == 0   # nothing counted: the caller skips the step
    for n in (1, 31, 32, 33, 63, 64, 65):
        perm, tile_seg, tile_n = _check_plan(np.zeros(n, dtype=np.int32), 1)
        assert perm.size == -(-n // TILE) * TILE and tile_n.sum() == n
        np.testing.assert_array_equal(perm[:n], np.arange(n))


@pytest.mark.parametrize("seed", range(6))
def test_tile_plan_on_random_codes(seed):
    rng = np.random.default_rng(seed)
    n, n_seg = int(rng.integers(1, 400)), int(rng.integers(1, 9))
    seg = rng.integers(-2, n_seg + 2, size=n)
    if seed % 2:
        seg[seg == n_seg // 2] = -1   # an absent segment
    _check_plan(seg, n_seg)
    _check_plan(seg, n_seg, tile=5)


def test_tile_plan_argument_errors():
    from spvipes_amd.data import expression_tile_plan
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="n_seg"):
            expression_tile_plan([0, 1], bad)
    for bad in (0, -4, 2.0, False):
        with pytest.raises(ValueError, match="tile"):
            expression_tile_plan([0, 1], 2, bad)
    with pytest.raises(TypeError):
        expression_tile_plan([0.5, 1.0], 2)


# ---- expression_stats_table ------------------------------------------------------------------------------------------------------
def test_stats_table_against_numpy_on_synthetic_values():
    from spvipes_amd.data import EXPRESSION_STATS, expression_stats_table
    rng = np.random.default_rng(3)
    n_sel, counts = 7, [0, 1, 2, 50, 1000]
    t = np.zeros((len(counts), 8, n_sel))
    vals = {}
    for k, n in enumerate(counts):
        v = rng.gamma(0.7, 3.0, size=(4, n, n_sel)).astype(np.float32).astype(np.float64)
        v[3] = rng.random((n, n_sel)).astype(np.float32)
        v[1] = (v[3] * v[1]).astype(np.float32)
        v[0] = (v[1].astype(np.float32) + v[2].astype(np.float32)).astype(np.float32)
        if n:
            v[:, :, 2] = 0.0          # a gene the model expects nothing of: zero mixture sum
            v[:, :, 4] = v[:, :1, 4]  # a constant column
        vals[k] = v
        t[k, :4], t[k, 4:] = v.sum(1), (v * v).sum(1)
    df = expression_stats_table(t, counts)
    assert list(df.columns) == ["segment", "column"] + list(EXPRESSION_STATS) and len(df) == len(counts) * n_sel
    assert EXPRESSION_STATS == ("mean", "mean_private", "mean_shared", "mixing", "private_fraction", "var", "var_private", "var_shared", "var_mixing")
    assert all(df[c].dtype == np.float64 for c in EXPRESSION_STATS)
    np.testing.assert_array_equal(df["segment"], np.repeat(np.arange(len(counts)), n_sel))
    np.testing.assert_array_equal(df["column"], np.tile(np.arange(n_sel), len(counts)))
    mean_cols, var_cols = ("mean", "mean_private", "mean_shared", "mixing"), ("var", "var_private", "var_shared", "var_mixing")
    for k, n in enumerate(counts):
        blk = df.iloc[k * n_sel:(k + 1) * n_sel]
        if n == 0:
            assert blk[list(EXPRESSION_STATS)].isna().all().all()
            continue
        for w in range(4):
            np.testing.assert_allclose(blk[mean_cols[w]], vals[k][w].mean(0), rtol=1e-13, atol=0)
            if n == 1:
                assert blk[var_cols[w]].isna().all()          # one value: no variance
            else:
                want = vals[k][w].var(0, ddof=1)
                scale = (vals[k][w] ** 2).sum(0) / (n - 1)    # what the cancellation in Q - S^2 / n is relative to
                assert (np.abs(blk[var_cols[w]].to_numpy() - want) <= 1e-13 * scale + 1e-300).all()
                assert (blk[var_cols[w]] >= 0).all()
        pf = blk["private_fraction"].to_numpy()
        assert np.isnan(pf[2]) and blk["mean"].to_numpy()[2] == 0.0    # zero mixture sum
        keep = np.arange(n_sel) != 2
        np.testing.assert_allclose(pf[keep], vals[k][1].sum(0)[keep] / vals[k][0].sum(0)[keep], rtol=1e-13)


def test_stats_table_clamps_a_negative_variance_at_zero():
    from spvipes_amd.data import expression_stats_table
    t = np.zeros((1, 8, 2))
    # three equal values 0.1f: S^2 / n may exceed the rounded Q by an ulp -> clamped; and a hand-made Q slightly below S^2 / n
    x = float(np.float32(0.1))
    t[0, :4, 0], t[0, 4:, 0] = 3 * x, 3 * x * x
    t[0, :4, 1], t[0, 4:, 1] = 6.0, 12.0 * (1 - 1e-15)
    df = expression_stats_table(t, [3])
    assert (df[["var", "var_private", "var_shared", "var_mixing"]].to_numpy() >= 0).all()
    assert df["var"][1] == 0.0 and df["mean"][1] == 2.0 and df["private_fraction"][1] == 1.0
    assert abs(df["var"][0]) <= 1e-16
    for bad_t, bad_c in ((t.astype(np.float32), [3]), (t[:, :7], [3]), (t, [3, 3]), (t, [-1]), (t, [1.5])):
        with pytest.raises(ValueError):
            expression_stats_table(bad_t, bad_c)


# ---- signatures and argument errors ----------------------------------------------------------------------------------------------
def test_entry_points_exist_on_every_layer():
    from spvipes_amd import data, dec_ops
    from spvipes_amd.model import spVIPES
    from spvipes_amd.module import spVIPESmodule
    sig = inspect.signature(dec_ops.expected_expression_stats)
    assert list(sig.parameters)[:9] == list(inspect.signature(dec_ops.expected_expression).parameters)[:9]
    assert list(sig.parameters)[9:] == ["genes", "library_size", "log_library", "tile_seg", "tile_n", "n_seg", "stats", "batch_rows"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[9:]) and sig.parameters["batch_rows"].default is None
    sig = inspect.signature(spVIPESmodule.expression_stats)
    assert list(sig.parameters)[1:] == ["inference_outputs", "group", "genes", "library_size", "library", "use_mean", "perm", "tile_seg", "tile_n", "n_seg", "stats"]
    sig = inspect.signature(spVIPES.expression_statistics)
    assert list(sig.parameters)[1:] == ["group_indices_list", "group", "groupby", "labels", "gene_list", "library_size", "n_samples", "use_mean", "batch_size", "_noise"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["groupby"], d["labels"], d["gene_list"], d["library_size"], d["n_samples"], d["use_mean"], d["batch_size"], d["_noise"]) == (None, None, None, "latent", 1, True, None, None)
    assert callable(data.expression_tile_plan) and callable(data.expression_stats_table)
    assert len(dec_ops.EXPECTED_STATS) == 8
    for word in ("31 padded rows", "bit for bit", "batch_size"):
        assert word in spVIPES.expression_statistics.__doc__


def test_argument_checks_raise_without_a_device():
    import torch
    from spvipes_amd import _abi, dec_ops
    from spvipes_amd.model import spVIPES
    # the method checks before it touches the model or a device
    with pytest.raises(ValueError, match="library_size"):
        spVIPES.expression_statistics(object(), [[0], [0]], 0, library_size="raw")
    with pytest.raises(ValueError, match="library_size"):
        spVIPES.expression_statistics(object(), [[0], [0]], 0, library_size=-1.0)
    with pytest.raises(ValueError, match="n_samples"):
        spVIPES.expression_statistics(object(), [[0], [0]], 0, n_samples=0, use_mean=False)
    with pytest.raises(ValueError, match="use_mean"):
        spVIPES.expression_statistics(object(), [[0], [0]], 0, n_samples=2)
    with pytest.raises(ValueError, match="group"):
        spVIPES.expression_statistics(object(), [[0], [0]], 2)
    # the op refuses training mode ahead of any operand preparation
    with pytest.raises(_abi.SpvError, match="eval mode"):
        dec_ops.expected_expression_stats(None, None, None, None, None, True, 1, None, tile_seg=None, tile_n=None, n_seg=1, stats=None)
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="batch_rows"):
            dec_ops.expected_expression_stats(None, None, None, None, None, False, 1, None, tile_seg=None, tile_n=None, n_seg=1, stats=None, batch_rows=bad)
    # the tables: host tensors, wrong dtypes, wrong shapes
    f64, i32 = torch.zeros((2, 8, 8), dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    for kw in (dict(tile_seg=i32, tile_n=i32, n_seg=2, stats=f64),           # nothing is on a device
               dict(tile_seg=None, tile_n=i32, n_seg=2, stats=f64),
               dict(tile_seg=i32.long(), tile_n=i32, n_seg=2, stats=f64)):
        with pytest.raises(_abi.SpvError, match="expected_expression_stats"):
            dec_ops.check_expected_stats_tables(70, 8, **kw)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="n_seg"):
            dec_ops.check_expected_stats_tables(70, 8, i32, i32, bad, f64)
