"""CPU: the host side of the rank-sum test (spVIPES.rank_genes_groups): ``data.rank_test_table`` against
``scipy.stats.mannwhitneyu(use_continuity=False, method="asymptotic")`` gene by gene, the uncorrected variance, the degenerate genes,
Benjamini-Hochberg against a plain implementation, the signatures, every argument error that is raised before anything touches the
device, and one run of tools/rank_host_check.py --small.

Tolerances.  The inputs of ``rank_test_table`` are exact integers (doubled rank sums, t^3 - t); U, the variance and the z-score follow
from them in a handful of fp64 roundings each, and scipy forms the same quantities from the same ranks: scores and U agree to rtol
1e-12.  The p-value goes through erfc / the normal survival function, whose implementations differ in the last digits: rtol 1e-9."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from tests._rank_reference import keys_of, rank_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _populations(seed, n1=37, n2=55, n_genes=12):
    """counts of two populations with heavy ties, and per gene the integers the kernel would deliver for population 1"""
    rng = np.random.default_rng(seed)
    c = (rng.integers(1, 9, (n1 + n2, n_genes)) * (rng.random((n1 + n2, n_genes)) < 0.4)).astype(np.uint16)
    w = (1e4 / np.maximum(c.sum(1), 1)).astype(np.float32)
    keys = keys_of(c, w)
    keys[:, 0] = rng.permutation(n1 + n2) + 1            # no ties at all
    seg = np.concatenate([np.zeros(n1, np.int64), np.ones(n2, np.int64)])
    rank2, ties = rank_tables(keys, seg, 2)
    return keys, rank2, ties, n1, n2


@pytest.mark.parametrize("seed", [0, 1])
def test_table_equals_scipy_mannwhitneyu_gene_by_gene(seed):
    from scipy.stats import mannwhitneyu

    from spvipes_amd.data import RANK_COLUMNS, rank_test_table

    keys, rank2, ties, n1, n2 = _populations(seed)
    for k, (own, m1) in enumerate(((slice(0, n1), n1), (slice(n1, None), n2))):
        tab = rank_test_table(rank2[k], ties, m1, n1 + n2)
        assert tuple(tab) == RANK_COLUMNS and all(v.dtype == np.float64 and v.shape == (keys.shape[1],) for v in tab.values())
        other = slice(n1, None) if k == 0 else slice(0, n1)
        for j in range(keys.shape[1]):
            a, b = keys[own, j].astype(np.float64), keys[other, j].astype(np.float64)
            res = mannwhitneyu(a, b, use_continuity=False, method="asymptotic", alternative="two-sided")
            assert tab["u_statistic"][j] == pytest.approx(res.statistic, rel=1e-12, abs=0)
            assert tab["auc"][j] == pytest.approx(res.statistic / (len(a) * len(b)), rel=1e-12, abs=0)
            assert tab["pvals"][j] == pytest.approx(res.pvalue, rel=1e-9, abs=0)
            # scipy keeps its z to itself: the score against the formula on scipy's own U, mean and tie-corrected variance
            n = n1 + n2
            t = np.unique(np.concatenate([a, b]), return_counts=True)[1].astype(np.float64)
            var = len(a) * len(b) / 12.0 * ((n + 1) - (t ** 3 - t).sum() / (n * (n - 1)))
            z = (res.statistic - len(a) * len(b) / 2.0) / np.sqrt(var)
            assert tab["scores"][j] == pytest.approx(z, rel=1e-12, abs=0)   # (both numerators are exact half-integers: a balanced gene gives 0 == 0)


def test_tie_correct_false_is_the_uncorrected_formula():
    from spvipes_amd.data import rank_test_table

    _keys, rank2, ties, n1, n2 = _populations(2)
    n = n1 + n2
    tab = rank_test_table(rank2[0], ties, n1, n, tie_correct=False)
    r = rank2[0].astype(np.float64) / 2.0
    z = (r - n1 * (n + 1) / 2.0) / np.sqrt(n1 * n2 * (n + 1) / 12.0)    # scanpy's default
    np.testing.assert_allclose(tab["scores"], z, rtol=1e-12, atol=0)
    corrected = rank_test_table(rank2[0], ties, n1, n)
    tied = ties > 0
    assert tied.any() and (~tied).any()
    assert (np.abs(corrected["scores"][tied]) > np.abs(tab["scores"][tied])).all()       # ties shrink the variance
    assert (corrected["scores"][~tied] == tab["scores"][~tied]).all()
    assert (corrected["u_statistic"] == tab["u_statistic"]).all()


def test_all_tied_gene_and_empty_side():
    from spvipes_amd.data import RANK_COLUMNS, rank_test_table

    n1, n = 4, 10
    # every key equal: every cell has the average rank (n + 1) / 2, one run of n
    tab = rank_test_table([n1 * (n + 1)], [n ** 3 - n], n1, n)
    assert tab["scores"][0] == 0.0 and tab["pvals"][0] == 1.0 and tab["pvals_adj"][0] == 1.0
    assert tab["u_statistic"][0] == n1 * (n - n1) / 2.0 and tab["auc"][0] == 0.5
    for empty in (0, n):
        tab = rank_test_table([0, 5], [0, 6], empty, n)
        assert tuple(tab) == RANK_COLUMNS and all(np.isnan(v).all() and v.shape == (2,) for v in tab.values())
    for bad in ((-1, 5), (6, 5), (True, 5), (2.0, 5), (0, 0)):
        with pytest.raises(ValueError):
            rank_test_table([1], [0], *bad)
    with pytest.raises(ValueError):
        rank_test_table([1, 2], [0], 1, 3)


def test_benjamini_hochberg_against_a_plain_implementation():
    from spvipes_amd.data import benjamini_hochberg

    rng = np.random.default_rng(3)
    p = np.concatenate([rng.random(40) ** 3, [0.0, 1.0, 0.5, 0.5]])
    m = len(p)
    want = np.empty(m)
    order = sorted(range(m), key=lambda i: p[i])
    for place, i in enumerate(order):
        want[i] = min(1.0, min(p[l] * m / (q + 1) for q, l in enumerate(order) if q >= place))
    np.testing.assert_allclose(benjamini_hochberg(p), want, rtol=1e-15, atol=0)
    with_nan = benjamini_hochberg([0.01, np.nan, 0.04])
    assert np.isnan(with_nan[1]) and with_nan[0] == 0.02 and with_nan[2] == 0.04
    assert benjamini_hochberg([]).shape == (0,)


def test_signatures():
    from spvipes_amd import rank_ops
    from spvipes_amd.data import rank_test_table
    from spvipes_amd.model import spVIPES

    sig = inspect.signature(rank_ops.rank_sums)
    assert list(sig.parameters) == ["counts", "rows", "seg", "n_seg", "w", "genes"]
    assert sig.parameters["w"].default is None and sig.parameters["genes"].default is None
    sig = inspect.signature(rank_test_table)
    assert list(sig.parameters) == ["rank2_k", "ties", "n1", "n", "tie_correct"] and sig.parameters["tie_correct"].default is True
    sig = inspect.signature(spVIPES.rank_genes_groups)
    assert list(sig.parameters) == ["self", "group_indices_list", "group", "idx1", "idx2", "groupby", "labels", "gene_list", "target_sum", "normalize", "tie_correct"]
    assert all(sig.parameters[k].default is None for k in ("idx1", "idx2", "groupby", "labels", "gene_list"))
    assert sig.parameters["target_sum"].default == 1e4 and sig.parameters["normalize"].default is True and sig.parameters["tie_correct"].default is True


def _bare_model():
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    m = spVIPES.__new__(spVIPES)   # the argument checks run before anything of the device is touched
    m.adata = make_duck(seed=2)
    return m, [list(range(300)), list(range(300, 560))]


def test_argument_errors_come_before_any_device_work():
    m, gil = _bare_model()
    with pytest.raises(ValueError, match="exactly one"):
        m.rank_genes_groups(gil, 0)
    with pytest.raises(ValueError, match="exactly one"):
        m.rank_genes_groups(gil, 0, idx1=[0, 1], groupby="cell_type")
    for bad in (0, -1.0, float("inf"), float("nan"), "1e4", None, True):
        with pytest.raises(ValueError, match="target_sum"):
            m.rank_genes_groups(gil, 0, idx1=[0, 1], target_sum=bad)
        with pytest.raises(ValueError, match="target_sum"):
            m.rank_genes_groups(gil, 0, idx1=[0, 1], target_sum=bad, normalize=False)
    with pytest.raises(ValueError, match="group must be"):
        m.rank_genes_groups(gil, 2, idx1=[0, 1])
    with pytest.raises(KeyError, match="not among the labels"):
        m.rank_genes_groups(gil, 0, groupby="cell_type", labels=[99])
    with pytest.raises(KeyError, match="no column"):
        m.rank_genes_groups(gil, 0, groupby="nope")
    with pytest.raises(ValueError, match="one label per cell"):
        m.rank_genes_groups(gil, 0, groupby=np.zeros(7))
    with pytest.raises(ValueError, match="at least two distinct labels"):
        m.rank_genes_groups(gil, 0, groupby=np.zeros(300))
    with pytest.raises(ValueError, match="overlap"):
        m.rank_genes_groups(gil, 0, idx1=[0, 1, 2], idx2=[2, 3])
    with pytest.raises(ValueError, match="not in group_indices_list"):
        m.rank_genes_groups(gil, 0, idx1=[400])
    with pytest.raises(ValueError, match="listed more than once"):
        m.rank_genes_groups(gil, 0, idx1=[1, 1])
    with pytest.raises(ValueError, match="is empty"):
        m.rank_genes_groups(gil, 0, idx1=[])
    with pytest.raises(ValueError, match="labels goes with groupby"):
        m.rank_genes_groups(gil, 0, idx1=[0], labels=[1])
    with pytest.raises(ValueError, match="idx2 goes with idx1"):
        m.rank_genes_groups(gil, 0, groupby="cell_type", idx2=[1])


def test_rank_sums_refuses_foreign_counts_without_the_library():
    from spvipes_amd import _abi, rank_ops

    with pytest.raises(_abi.SpvError, match="GroupCounts"):
        rank_ops.rank_sums(object(), None, None, 1)
    with pytest.raises(_abi.SpvError, match="GroupCounts"):
        rank_ops.rank_sums(np.zeros((2, 2)), None, None, 1)


def test_host_check_of_the_kernel_core_small():
    """tools/rank_host_check.py --small: the RANK-CORE text of the header as plain C++ behind an emulated workgroup, whole tables equal"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rank_host_check.py"), "--small"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "all equal" in res.stdout and "DIFFER" not in res.stdout and "TOUCHED" not in res.stdout
    assert "radix 5" in res.stdout and "lds 66" in res.stdout   # both sort paths ran
