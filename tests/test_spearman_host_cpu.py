"""CPU: the host side of the Spearman read-outs -- ``data.spearman_table`` and its exactness bound, the reference of the GPU tests held
to its own identities, the signatures of ``get_feature_spearman_matrix`` / ``count_spearman_matrix`` and every refusal that comes ahead
of device work, and tools/spearman_host_check.py (the kernels' core compiled for the CPU) run as a test.  No GPU calls."""
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _keys(n, rng):
    """fp32 keys [n, 6]: all distinct | heavy ties | mostly zeros | constant | one non-zero | distinct with one tie"""
    k = np.zeros((n, 6), np.float32)
    k[:, 0] = rng.permutation(n) + 1
    k[:, 1] = rng.integers(0, 4, n)
    k[:, 2] = rng.integers(1, 9, n) * (rng.random(n) < 0.1)
    k[:, 3] = 2.5
    k[n // 2, 4] = 3.0
    k[:, 5] = rng.permutation(n)
    k[0, 5] = k[n - 1, 5]
    return k


@pytest.mark.parametrize("n", [2, 129, 600, 8200])
def test_the_reference_satisfies_its_identities_and_spearman_table_reads_it(n):
    from scipy.stats import spearmanr

    from spvipes_amd.data import spearman_table
    from tests._spearman_reference import spearman_tables
    keys = _keys(n, np.random.default_rng(n))
    c, Cm, T = spearman_tables(keys)   # asserts c.sum(0) == 0 and 3 diag(C) == n^3 - n - T
    assert np.abs(c).max() <= n - 1 and T[0] == 0 and T[3] == n ** 3 - n and (c[:, 3] == 0).all()
    t = spearman_table(Cm.astype(np.float64), n)
    assert (t["tie_term"] == T).all() and (t["mean"] == 0).all()
    rho = t["corr"]
    dead = np.diagonal(Cm) == 0
    assert dead[3] and (n == 2 or not dead[[0, 1, 2, 5]].any())
    assert np.isnan(rho[dead]).all() and np.isnan(rho[:, dead]).all() and not np.isnan(rho[~dead][:, ~dead]).any()
    assert (np.diagonal(rho)[~dead] == 1.0).all() and np.array_equal(rho, rho.T, equal_nan=True)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.asarray(spearmanr(keys).statistic)
    assert np.array_equal(np.isnan(want), np.isnan(rho))
    worst = np.nanmax(np.abs(want - rho)) if (~np.isnan(rho)).any() else 0.0
    print(f"n {n}: worst |rho - scipy| = {worst / 2.0 ** -53:.1f} x 2^-53")
    assert worst <= 32 * 2.0 ** -53


def test_spearman_table_tables_and_argument_errors():
    from spvipes_amd.data import SPEARMAN_EXACT_ROWS, correlation_table, spearman_table
    assert SPEARMAN_EXACT_ROWS == 208063 and SPEARMAN_EXACT_ROWS ** 3 < 2 ** 53 <= (SPEARMAN_EXACT_ROWS + 1) ** 3
    assert "208063^3 < 2^53" in spearman_table.__doc__
    # n = 3: columns (1, 2, 3) -> c = (-2, 0, 2); (3, 2, 1) -> (2, 0, -2); (5, 5, 5) -> 0; (1, 1, 2) -> (-1, -1, 2)
    c = np.array([[-2, 2, 0, -1], [0, 0, 0, -1], [2, -2, 0, 2]], np.float64)
    t = spearman_table(c.T @ c, 3)
    assert t["corr"][0, 1] == -1.0 and t["corr"][0, 0] == 1.0 and np.isnan(t["corr"][2]).all() and np.isnan(t["corr"][:, 2]).all()
    assert t["corr"][0, 3] == t["corr"][3, 0] and abs(t["corr"][0, 3] - 6.0 / np.sqrt(8.0 * 6.0)) <= 2.0 ** -52 and t["tie_term"].tolist() == [0.0, 0.0, 24.0, 6.0]
    same = correlation_table(np.zeros(4), c.T @ c, 3)
    assert all(np.array_equal(t[k], same[k], equal_nan=True) for k in same)
    with pytest.raises(ValueError, match="square float64"):
        spearman_table(np.zeros((2, 3)), 3)
    with pytest.raises(ValueError, match="square float64"):
        spearman_table(np.zeros((2, 2), np.float32), 3)
    with pytest.raises(ValueError, match="non-negative integer"):
        spearman_table(np.zeros((2, 2)), 2.0)


def test_the_pearson_refusal_names_the_new_method():
    from spvipes_amd.data import check_correlation_args
    with pytest.raises(NotImplementedError, match="spearman.*get_feature_spearman_matrix"):
        check_correlation_args("spearman")
    with pytest.raises(ValueError, match="correlation_type must be 'pearson'"):
        check_correlation_args("kendall")


def test_signatures_and_refusals_ahead_of_any_device_work():
    import torch
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    pearson = inspect.signature(spVIPES.get_feature_correlation_matrix)
    sig = inspect.signature(spVIPES.get_feature_spearman_matrix)
    assert list(sig.parameters) == [k for k in pearson.parameters if k != "correlation_type"]
    assert all(sig.parameters[k].default == pearson.parameters[k].default for k in sig.parameters)
    sig = inspect.signature(spVIPES.count_spearman_matrix)
    assert list(sig.parameters) == ["self", "group_indices_list", "group", "gene_list", "cells", "normalize", "target_sum"]
    assert {k: sig.parameters[k].default for k in ("gene_list", "cells", "normalize", "target_sum")} == dict(gene_list=None, cells=None, normalize=True, target_sum=1e4)
    f, c = spVIPES.get_feature_spearman_matrix, spVIPES.count_spearman_matrix
    gi = [[0], [0]]
    with pytest.raises(ValueError, match="component"):
        f(object(), gi, 0, component="both")
    with pytest.raises(ValueError, match="library_size"):
        f(object(), gi, 0, library_size=-1.0)
    with pytest.raises(ValueError, match="use_mean"):
        f(object(), gi, 0, n_samples=2)
    with pytest.raises(ValueError, match="target_sum"):
        c(object(), gi, 0, target_sum=-1.0)
    for fn in (f, c):
        with pytest.raises(ValueError, match="group must be 0 or 1"):
            fn(object(), gi, 2)
    gi = [list(range(300)), list(range(300, 560))]
    for cells, words in (([300], r"cells: cell 300 is not in group_indices_list\[0\]"), ([], "cells is empty"), ([3, 4, 3], "cells: cell 3 is listed more than once"),
                         ([0.5], "cells must hold adata row numbers"), (np.array([True, False]), "cells must hold adata row numbers")):
        for fn in (f, c):
            with pytest.raises(ValueError, match=words):
                fn(object(), gi, 0, cells=cells)
    # the limits: more than 4096 genes, more than 2^20 rows -- refused before anything is allocated (the model below has no device at all)
    m = spVIPES.__new__(spVIPES)
    m.adata = make_duck(seed=2)
    m.module, m.device = SimpleNamespace(input_dims={0: 96, 1: 80}), torch.device("cpu")
    for fn in (f, c):
        with pytest.raises(ValueError, match=rf"4800 genes selected: .* n_sel\^2 x 8 = {4800 * 4800 * 8} bytes"):
            fn(m, gi, 0, gene_list=list(range(96)) * 50)
    big = [list(range((1 << 20) + 1)), [0]]
    with pytest.raises(ValueError, match=r"1048577 rows .* at most 2\^20"):
        c(m, big, 0)
    with pytest.raises(ValueError, match=r"1048577 rows .* at most 2\^20"):
        f(m, big, 0)
    with pytest.raises(ValueError, match=r"1048578 rows .* at most 2\^20"):
        f(m, [big[0][: (1 << 19) + 1], [0]], 0, n_samples=2, use_mean=False)


def test_the_kernels_core_on_the_host():
    """tools/spearman_host_check.py: stage with position entries (one list beyond 65 535 positions), fill-then-scatter, the store's maps,
    the workspace layout -- whole arrays equal to numpy's"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import spearman_host_check as tool
    finally:
        sys.path.pop(0)
    assert max(s[0] for s in tool.SHAPES) > 65536
    assert tool.run(tool.SHAPES, verbose=False) == 0
