"""CPU: the host side of spVIPES.get_feature_correlation_matrix -- ``data.correlation_table`` (Pearson from one-pass fp64 sums) against
``np.corrcoef``, its edge cases, ``data.correlation_cells`` / ``data.check_correlation_args``, the method's signature and the refusals it
makes before any device work, and one run of the kernel core's host check (tools/gram_host_check.py --small).  No GPU calls."""
import inspect
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def _sums(x):
    """fp64 (S, C) rounded once from long-double sums of the fp32 data's exact products"""
    xl = x.astype(LD)
    return xl.sum(0).astype(np.float64), (xl.T @ xl).astype(np.float64)


def test_correlation_table_matches_corrcoef_on_random_fp32_data():
    from spvipes_amd.data import correlation_table
    rng = np.random.default_rng(0)
    n, p = 500, 12
    x = (rng.standard_normal((n, p)) @ rng.standard_normal((p, p)) + rng.uniform(-3, 3, p)).astype(np.float32)
    S, Cm = _sums(x)
    t = correlation_table(S, Cm, n)
    assert set(t) == {"mean", "cov", "var", "corr"} and all(v.dtype == np.float64 for v in t.values())
    x64 = x.astype(np.float64)
    # mean^2 / var is below 100 here, so the one-pass cancellation costs two digits at the most: 1e-12 leaves three more to spare
    np.testing.assert_allclose(t["corr"], np.corrcoef(x64, rowvar=False), rtol=0, atol=1e-12)
    np.testing.assert_allclose(t["cov"], np.cov(x64, rowvar=False), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(t["var"], x64.var(0, ddof=1), rtol=1e-12)
    np.testing.assert_array_equal(t["mean"], S / n)
    assert (np.diagonal(t["corr"]) == 1.0).all() and (np.abs(t["corr"]) <= 1.0).all()
    assert np.array_equal(t["corr"], t["corr"].T) and np.array_equal(t["cov"], t["cov"].T)   # a symmetric C gives symmetric tables, in bits


def test_constant_column_copies_and_the_clip():
    from spvipes_amd.data import correlation_table
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 5)).astype(np.float32)
    x[:, 2] = 3.5                  # no variance: NaN in its row and column
    x[:, 4] = -2 * x[:, 0]         # r = -1 up to rounding: clipped into [-1, 1]
    t = correlation_table(*_sums(x), 40)
    assert t["var"][2] == 0.0 and np.isnan(t["corr"][2]).all() and np.isnan(t["corr"][:, 2]).all()
    live = [0, 1, 3, 4]
    sub = t["corr"][np.ix_(live, live)]
    assert np.isfinite(sub).all() and (np.diagonal(sub) == 1.0).all() and (np.abs(sub) <= 1.0).all()
    assert abs(t["corr"][0, 4] + 1.0) < 1e-12
    # a column whose one-pass variance comes out negative is clamped to 0 and reads as constant
    S, Cm = np.array([3.0, 1.0]), np.array([[3.0 - 1e-9, 1.0], [1.0, 5.0]])   # C_00 < S_0^2 / n
    t = correlation_table(S, Cm, 3)
    assert t["var"][0] == 0.0 and t["cov"][0, 0] < 0 and np.isnan(t["corr"][0]).all() and t["corr"][1, 1] == 1.0


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_observations(n):
    from spvipes_amd.data import correlation_table
    t = correlation_table(np.array([2.0, 4.0]) * n, np.array([[4.0, 8.0], [8.0, 16.0]]) * n, n)
    assert np.isnan(t["corr"]).all() and np.isnan(t["cov"]).all() and np.isnan(t["var"]).all() and t["corr"].shape == (2, 2)
    if n == 0:
        assert np.isnan(t["mean"]).all()
    else:
        np.testing.assert_array_equal(t["mean"], [2.0, 4.0])


def test_correlation_table_argument_errors_and_docstring():
    from spvipes_amd.data import correlation_table
    with pytest.raises(ValueError, match="float64"):
        correlation_table(np.zeros(2, np.float32), np.zeros((2, 2)), 3)
    with pytest.raises(ValueError, match="float64"):
        correlation_table(np.zeros(2), np.zeros((2, 3)), 3)
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError, match="non-negative integer"):
            correlation_table(np.zeros(2), np.zeros((2, 2)), bad)
    assert "2 sqrt(n 2^-53)" in correlation_table.__doc__   # the one-pass formula's limit is stated


def test_signature_and_refusals_ahead_of_any_device_work():
    import torch
    from spvipes_amd.data import check_correlation_args
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    sig = inspect.signature(spVIPES.get_feature_correlation_matrix)
    assert list(sig.parameters) == ["self", "group_indices_list", "group", "gene_list", "cells", "component", "library_size", "n_samples", "use_mean",
                                    "correlation_type", "batch_size", "_noise"]
    want = dict(gene_list=None, cells=None, component="mixture", library_size="latent", n_samples=1, use_mean=True, correlation_type="pearson",
                batch_size=None, _noise=None)
    assert {k: sig.parameters[k].default for k in want} == want
    f = spVIPES.get_feature_correlation_matrix
    gi = [[0], [0]]
    with pytest.raises(NotImplementedError, match="spearman"):
        f(object(), gi, 0, correlation_type="spearman")
    for bad in ("kendall", "Pearson", None, 1):
        with pytest.raises(ValueError, match="correlation_type must be 'pearson'"):
            f(object(), gi, 0, correlation_type=bad)
    with pytest.raises(ValueError, match="component"):
        f(object(), gi, 0, component="both")
    with pytest.raises(ValueError, match="library_size"):
        f(object(), gi, 0, library_size=-1.0)
    with pytest.raises(ValueError, match="use_mean"):
        f(object(), gi, 0, n_samples=2)
    with pytest.raises(ValueError, match="group must be 0 or 1"):
        f(object(), gi, 2)
    # ``cells``: idx1's rules of differential_expression, named ``cells`` -- all ahead of the model
    gi = [list(range(300)), list(range(300, 560))]
    for cells, words in (([300], r"cells: cell 300 is not in group_indices_list\[0\]"), ([], "cells is empty"), ([3, 4, 3], "cells: cell 3 is listed more than once"),
                         ([0.5], "cells must hold adata row numbers"), (np.array([True, False]), "cells must hold adata row numbers")):
        with pytest.raises(ValueError, match=words):
            f(object(), gi, 0, cells=cells)
    # more than 4096 genes: refused with the table's size, before anything is allocated (the model below has no device at all)
    m = spVIPES.__new__(spVIPES)
    m.adata = make_duck(seed=2)
    m.module, m.device = SimpleNamespace(input_dims={0: 96, 1: 80}), torch.device("cpu")
    with pytest.raises(ValueError, match=rf"4800 genes selected: .* n_sel\^2 x 8 = {4800 * 4800 * 8} bytes"):
        f(m, gi, 0, gene_list=list(range(96)) * 50)
    m.module = SimpleNamespace(input_dims={0: 5000, 1: 80})
    with pytest.raises(ValueError, match="5000 genes selected"):
        f(m, gi, 0)
    check_correlation_args("pearson", 4096)   # the limit itself passes


def test_correlation_cells_masks_positions():
    from spvipes_amd.data import correlation_cells, de_populations
    gi = [10, 11, 12, 13, 11]   # a repeated cell: its first position stands for it, as in de_populations
    assert correlation_cells(gi, None).tolist() == [True] * 5
    assert correlation_cells(gi, [13, 11]).tolist() == [False, True, False, True, False]
    assert correlation_cells(gi, np.array([12], np.int32), group=1).tolist() == [False, False, True, False, False]
    assert sorted(de_populations(gi, [13, 11])[0].tolist()) == [1, 3]   # the same positions idx1 resolves to
    with pytest.raises(ValueError, match=r"cells: cell 14 is not in group_indices_list\[1\]"):
        correlation_cells(gi, [14], group=1)


def test_the_kernel_core_passes_its_host_check():
    """the text between the GRAM-CORE marks, compiled for the CPU around an emulation of the 64 lanes: whole tables against numpy"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gram_host_check.py"), "--small"], capture_output=True, text=True)
    assert res.returncode == 0 and "all equal" in res.stdout and "DIFFER" not in res.stdout and "TOUCHED" not in res.stdout, res.stdout + res.stderr
    assert "gram_tile_of: 0 mismatches" in res.stdout and "gram_slabs(1984, 4096) = 2  gram_ws_bytes = 32537600" in res.stdout
