"""CPU: the pieces the model's read-out methods share -- the argument resolvers (``data.check_group`` / ``data.group_cell_labels``) and the
order their errors come in, the walk positions (``data.walk_positions``), the draw index (``spVIPES._draws``), the gene selection
(``spVIPES._genes``), the block collector (``data.RowBlocks``), the one-vs-rest frames (``data.vs_rest_frames``) and the host arithmetic behind
``posterior_predictive_check`` (``data.ppc_observed_columns`` against ``fractions.Fraction`` / float64 numpy, ``data.ppc_frame``).  No GPU calls."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

OBS = ("obs_mean", "obs_var", "obs_cv", "obs_zero_fraction")
PPC = ("ppc_mean", "ppc_var", "ppc_cv", "ppc_zero_fraction", "ppc_max")
SIZES = [1, 2, 7]   # one population of a single cell


def _counts():
    """10 cells x 5 genes of small integers, cut into populations of 1, 2 and 7 cells; gene 2 is zero everywhere"""
    X = np.random.default_rng(5).integers(0, 9, size=(sum(SIZES), 5)).astype(np.int64)
    X[:, 2] = 0
    X[3:, 4] *= np.arange(7) % 2   # some zeros in a gene that is not all zero
    return X


def _moments(X):
    """(sums [n_seg, 3, n_sel] as count_stats gives them, square sums [n_seg, n_sel]) of the populations of SIZES, formed with numpy"""
    cut = np.cumsum([0] + SIZES)
    pops = [X[a:b] for a, b in zip(cut[:-1], cut[1:])]
    sums = np.stack([np.stack([p.sum(0), (p > 0).sum(0), np.zeros(X.shape[1])]) for p in pops]).astype(np.float64)
    return pops, sums, np.stack([(p * p).sum(0) for p in pops])


# ---- ppc_observed_columns --------------------------------------------------------------------------------------------------------
def test_observed_columns_exact_route_equals_fraction_arithmetic():
    from spvipes_amd.data import ppc_observed_columns
    X = _counts()
    pops, sums, sq = _moments(X)
    assert sq.dtype == np.int64
    df = ppc_observed_columns(sums, sq, SIZES)
    assert len(df) == len(SIZES) * X.shape[1]
    for k, p in enumerate(pops):
        N = len(p)
        for j in range(X.shape[1]):
            S, NZ, Q = int(p[:, j].sum()), int((p[:, j] > 0).sum()), int((p[:, j] ** 2).sum())
            mean = float(Fraction(S, N))
            var = float(Fraction(N * Q - S * S, N * (N - 1))) if N >= 2 else float("nan")
            want = (mean, var, (np.sqrt(var) / mean) if mean > 0 else float("nan"), float(1 - Fraction(NZ, N)))
            got = tuple(float(df[c][k * X.shape[1] + j]) for c in OBS)
            for c, g, w in zip(OBS, got, want):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (k, j, c, g, w)   # equal as fp64 numbers, not merely close
    var, cv = df["obs_var"].to_numpy().reshape(3, 5), df["obs_cv"].to_numpy().reshape(3, 5)
    assert np.isnan(var[0]).all() and np.isfinite(var[1:]).all()                  # var: NaN for N < 2 and only there
    assert np.array_equal(np.isnan(cv), np.isnan(var) | (sums[:, 0] == 0))        # cv: NaN at mean 0 (and where var is)
    assert np.isnan(cv[:, 2]).all() and (var[1:, 2] == 0).all() and (df["obs_zero_fraction"].to_numpy().reshape(3, 5)[:, 2] == 1).all()
    # whole-number fp64 square sums below 2^53 (what fp32 count storage gives for integral counts) take the same route
    assert df.equals(ppc_observed_columns(sums, sq.astype(np.float64), SIZES))


def test_observed_columns_fp64_route_equals_numpy_moments():
    from spvipes_amd.data import ppc_observed_columns
    X = _counts().astype(np.float64)
    X[4, 1] += 0.5   # one fractional count, in the population of 7
    pops, sums, sq = _moments(X)
    assert sq.dtype == np.float64 and sums[2, 0, 1] != np.floor(sums[2, 0, 1])
    df = ppc_observed_columns(sums, sq, SIZES)
    assert "segment" not in df.columns   # not ppc_table's frame: the fp64 route
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.stack([p.mean(0) for p in pops])
        var = np.stack([p.var(0, ddof=1) if len(p) > 1 else np.full(X.shape[1], np.nan) for p in pops])
        want = {"obs_mean": mean, "obs_var": var, "obs_cv": np.where(mean > 0, np.sqrt(var) / mean, np.nan),
                "obs_zero_fraction": np.stack([(p == 0).mean(0) for p in pops])}
    for c in OBS:
        got = df[c].to_numpy().reshape(3, 5)
        assert np.array_equal(np.isnan(got), np.isnan(want[c])), c
        np.testing.assert_allclose(got, want[c], rtol=1e-12, atol=0, equal_nan=True, err_msg=c)
    assert np.isnan(df["obs_var"][:5]).all() and np.isnan(df["obs_cv"].to_numpy().reshape(3, 5)[:, 2]).all()


# ---- ppc_frame -------------------------------------------------------------------------------------------------------------------
def test_frame_assembly_rows_columns_dtypes_and_cell_totals():
    import pandas as pd
    from spvipes_amd.data import ppc_frame
    names, sizes, index, n_samples = ["b", "a"], [2, 2], np.array(["g0", "g1", "g2"]), 4
    cells = np.array([10, 11, 12, 13, 14])           # adata row numbers
    code = np.array([1, 0, -1, 0, 1])                # cell 12 is in no population
    kept = np.nonzero(code >= 0)[0]
    order = kept[np.argsort(code[kept], kind="stable")]
    rng = np.random.default_rng(0)
    obs = pd.DataFrame({"segment": 0, **{c: rng.random(6) for c in OBS}, "obs_max": 0.0})
    ppc = pd.DataFrame({"segment": 0, "column": 0, **{c: rng.random(6) for c in PPC}})
    obs_totals = np.array([5.0, 7.0, 1.0, 3.0])                      # in ``order``: cells 11, 13, 10, 14
    ppc_totals = np.array([8, 12, 999, 4, 6], dtype=np.uint64)       # per position, summed over the samples; position 2 is never counted
    df = ppc_frame(names, sizes, index, obs, ppc, n_samples, cells, order, kept, obs_totals, ppc_totals)
    assert list(df.columns) == ["population", "gene", "n_cells", "n_samples", *OBS, *PPC]
    assert [str(t) for t in df.dtypes] == ["object", "object", "int64", "int64"] + ["float64"] * 9
    assert df["population"].tolist() == ["b"] * 3 + ["a"] * 3 and df["gene"].tolist() == ["g0", "g1", "g2"] * 2   # population-major, then gene
    assert df["n_cells"].tolist() == [2] * 6 and df["n_samples"].tolist() == [4] * 6 and list(df.index) == list(range(6))
    for src, cols in ((obs, OBS), (ppc, PPC)):
        for c in cols:
            assert np.array_equal(df[c].to_numpy(), src[c].to_numpy())
    tot = df.attrs["cell_totals"]
    assert list(tot.columns) == ["obs_total", "ppc_total_mean"] and np.array_equal(tot.index.to_numpy(), cells)   # indexed by the adata row numbers
    np.testing.assert_array_equal(tot["obs_total"].to_numpy(), [1.0, 5.0, np.nan, 7.0, 3.0])
    np.testing.assert_array_equal(tot["ppc_total_mean"].to_numpy(), [8 / 4, 12 / 4, np.nan, 4 / 4, 6 / 4])       # total / n_samples
    assert tot.iloc[2].isna().all()   # a cell outside every population: NaN in both


# ---- the walk, the draws, the gene selection, the collector, the one-vs-rest frames ---------------------------------------------
def test_walk_positions_mark_the_replayed_rows_cut():
    from spvipes_amd.data import walk_positions
    out = list(walk_positions([(0, "t0", (4, 4)), (1, "t1", (4, 4))], 1, 5))
    assert [o[:4] for o in out] == [(0, "t0", (4, 4), 0), (1, "t1", (4, 4), 4)]
    assert out[0][4].dtype == np.int64
    np.testing.assert_array_equal(out[0][4], [0, 1, 2, 3])
    np.testing.assert_array_equal(out[1][4], [4, -1, -1, -1])   # positions 5, 6, 7 are cut
    pos = np.concatenate([o[4] for o in out])
    assert sorted(pos[pos >= 0].tolist()) == [0, 1, 2, 3, 4]    # 0 .. 4 are each kept once
    # the other group's sizes do not matter; a walk that ends at the group's size cuts nothing
    out = list(walk_positions([(0, None, (3, 9)), (1, None, (2, 9))], 0, 5))
    assert [o[3] for o in out] == [0, 3]
    np.testing.assert_array_equal(np.concatenate([o[4] for o in out]), [0, 1, 2, 3, 4])
    assert list(walk_positions([], 0, 5)) == []


def test_draw_index_is_step_times_n_samples_plus_sample():
    from spvipes_amd.model import spVIPES
    seen = []
    stub = SimpleNamespace(_infer=lambda tensors, noise, draw, B0, B1: seen.append((tensors, noise, draw, B0, B1)) or f"out{draw}")
    assert list(spVIPES._draws(stub, 3, "t", (4, 5), 4, "nf")) == [(0, "out12"), (1, "out13"), (2, "out14"), (3, "out15")]
    assert seen == [("t", "nf", 12 + s, 4, 5) for s in range(4)]
    assert list(spVIPES._draws(stub, 0, "t", (1, 1), 1, None)) == [(0, "out0")]


def _bare_model():
    import torch
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    m = spVIPES.__new__(spVIPES)   # the argument checks run before anything of the device is touched
    m.adata = make_duck(seed=2)
    m.adata.uns["groups_var_names"] = [np.array([f"a{i}" for i in range(96)]), np.array([f"b{i}" for i in range(80)])]
    m.module, m.device = SimpleNamespace(input_dims={0: 96, 1: 80}), torch.device("cpu")
    return m, [list(range(300)), list(range(300, 560))]


def test_gene_selection_is_the_same_for_one_group_and_for_two():
    m, _ = _bare_model()
    sel, dev, n, index = m._genes(1, [None, ["b7", "b2", "b7"]])
    assert sel.tolist() == [7, 2, 7] and dev.tolist() == [7, 2, 7] and str(dev.dtype) == "torch.int32" and n == 3 and index.tolist() == ["b7", "b2", "b7"]
    own = m._genes(1, ["b7", "b2", "b7"], own=True)
    assert own[0].tolist() == [7, 2, 7] and own[2] == 3 and own[3].tolist() == index.tolist()
    sel, dev, n, index = m._genes(0, [None, [1]])
    assert sel is None and dev is None and n == 96 and index.tolist() == [f"a{i}" for i in range(96)]
    assert m._genes(0, None)[2:3] == (96,) and m._genes(1, None, own=True)[2] == 80
    with pytest.raises(KeyError, match=r"gene_list\[1\]: gene .*zz.* is not among the genes of group 1"):
        m._genes(1, "zz", own=True)
    with pytest.raises(KeyError, match=r"gene_list\[1\]: gene .*zz.* is not among the genes of group 1"):
        m._genes(0, [None, ["zz"]])   # either group's call resolves the whole list: the first error is the same
    with pytest.raises(IndexError, match=r"gene_list\[0\]: position 96"):
        m._genes(0, [96], own=True)
    with pytest.raises(ValueError, match="one entry per group"):
        m._genes(0, [[1]])            # the outer list's shape is resolve_gene_list's check
    m.adata.uns["groups_var_names"] = None
    assert m._genes(0, [3, 1], own=True)[3].tolist() == [3, 1] and m._genes(1, None, own=True)[3].tolist() == list(range(80))


def test_row_blocks_concatenate_and_cut_on_the_host_or_the_device():
    import torch
    from spvipes_amd.data import RowBlocks
    steps = [[torch.arange(8).reshape(4, 2), torch.arange(3).reshape(3, 1)], [torch.arange(8, 16).reshape(4, 2), 10 + torch.arange(3).reshape(3, 1)]]
    for return_numpy in (True, False):
        blocks = RowBlocks([5, 6], return_numpy)
        for s in steps:
            blocks.add(s)
        res = blocks.result()
        assert sorted(res) == [0, 1] and isinstance(res[0], np.ndarray if return_numpy else torch.Tensor)
        np.testing.assert_array_equal(np.asarray(res[0]), np.arange(10).reshape(5, 2))            # cut at n[0] = 5
        np.testing.assert_array_equal(np.asarray(res[1]).ravel(), [0, 1, 2, 10, 11, 12])          # nothing to cut


def test_vs_rest_frames_append_the_comparison_columns_in_label_order():
    from spvipes_amd.data import vs_rest_frames
    index = np.array(["g0", "g1"])
    df = vs_rest_frames(((name, {"x": np.array([k, k + 0.5]), "y": np.array([True, False])}) for k, name in enumerate(["B", 3])), index)
    assert list(df.columns) == ["x", "y", "comparison", "group1", "group2"] and list(df.index) == ["g0", "g1", "g0", "g1"]
    assert df["comparison"].tolist() == ["B vs Rest"] * 2 + ["3 vs Rest"] * 2 and df["group1"].tolist() == ["B", "B", 3, 3] and df["group2"].tolist() == ["Rest"] * 4
    assert df["x"].tolist() == [0.0, 0.5, 1.0, 1.5] and df["y"].dtype == bool


# ---- argument resolvers and the order of the errors ------------------------------------------------------------------------------
def test_check_group():
    from spvipes_amd.data import check_group
    assert check_group(0) == 0 and check_group(1) == 1 and type(check_group(np.int64(1))) is int
    for bad in (2, -1, "0", None, 0.5):
        with pytest.raises(ValueError) as e:
            check_group(bad)
        assert str(e.value) == f"group must be 0 or 1, got {bad!r}"


def test_group_cell_labels():
    from spvipes_amd.data import group_cell_labels
    obs = {"t": np.array(["x", "y", "z", "y"])}
    assert group_cell_labels(obs, "t", np.array([3, 0]), 1).tolist() == ["y", "x"]
    assert group_cell_labels(obs, [[5, 6]], np.array([3, 0]), 1).tolist() == [5, 6]   # an array is flattened
    assert group_cell_labels(obs, "t", np.array([1, 1]), 0).tolist() == ["y", "y"]    # repeats pass unless ``unique``
    with pytest.raises(ValueError) as e:
        group_cell_labels(obs, "t", np.array([1, 1]), 0, unique=True)
    assert str(e.value) == "group_indices_list[0] lists a cell more than once"
    with pytest.raises(KeyError) as e:
        group_cell_labels(obs, "u", np.array([1, 1]), 0, unique=True)   # the groupby errors come first
    assert e.value.args[0] == "groupby: adata.obs has no column 'u'"
    with pytest.raises(ValueError) as e:
        group_cell_labels(obs, [1, 2, 3], np.array([1, 1]), 1, unique=True)
    assert str(e.value) == "groupby: an array must hold one label per cell of group_indices_list[1] (2), got 3"


METHODS = {
    "differential_expression_by": lambda m, gil, group, groupby, **kw: m.differential_expression_by(gil, group, groupby, **kw),
    "count_statistics": lambda m, gil, group, groupby, **kw: m.count_statistics(gil, group, groupby=groupby, **kw),
    "posterior_predictive_check": lambda m, gil, group, groupby, **kw: m.posterior_predictive_check(gil, group, groupby=groupby, **kw),
}
GROUPBY_ERRORS = [
    ("unknown-column", 0, "nope", KeyError, "groupby: adata.obs has no column 'nope'"),
    ("short-array", 0, np.arange(7), ValueError, "groupby: an array must hold one label per cell of group_indices_list[0] (300), got 7"),
    ("short-array-group-1", 1, np.arange(7), ValueError, "groupby: an array must hold one label per cell of group_indices_list[1] (260), got 7"),
    ("bad-group-first", 2, "nope", ValueError, "group must be 0 or 1, got 2"),
]


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("name,group,groupby,exc,text", GROUPBY_ERRORS, ids=[c[0] for c in GROUPBY_ERRORS])
def test_groupby_errors_are_the_same_in_every_method(method, name, group, groupby, exc, text):
    m, gil = _bare_model()
    with pytest.raises(exc) as e:
        METHODS[method](m, gil, group, groupby)
    assert e.value.args[0] == text


@pytest.mark.parametrize("method", sorted(METHODS))
def test_a_methods_own_argument_errors_come_before_the_groupby_errors(method):
    m, gil = _bare_model()
    first = {"differential_expression_by": (dict(n_samples=0), "n_samples must be a positive integer, got 0"),
             "count_statistics": (dict(target_sum=0), "target_sum must be a positive finite number, got 0"),
             "posterior_predictive_check": (dict(seed=-5), "seed must be an integer in [0, 2^32), got -5")}[method]
    with pytest.raises(ValueError) as e:
        METHODS[method](m, gil, 2, "nope", **first[0])
    assert str(e.value) == first[1]


@pytest.mark.parametrize("method", ["differential_expression_by", "count_statistics"])
def test_a_repeated_cell_is_reported_after_the_groupby_errors(method):
    m, gil = _bare_model()
    dup = [[0, 1, 1, 2], gil[1]]
    with pytest.raises(ValueError) as e:
        METHODS[method](m, dup, 0, "cell_type")
    assert str(e.value) == "group_indices_list[0] lists a cell more than once"
    with pytest.raises(KeyError, match="no column"):
        METHODS[method](m, dup, 0, "nope")
    with pytest.raises(KeyError, match="not among the labels"):   # ... and before the labels are looked at
        METHODS[method](m, gil, 0, "cell_type", labels=[99])
