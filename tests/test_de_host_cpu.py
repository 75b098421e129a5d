"""CPU: the host side of differential expression (spVIPES.differential_expression): the C ABI of spv_de_pairs (header, cross-compiled
library, ctypes mirror), pair drawing, argument checks, population resolution and the result table with its FDR set.  No GPU calls."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_spv_de_pairs():
    from spvipes_amd import _abi
    from spvipes_amd.build import HEADERS, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_de_pairs\s*\(\s*const\s+spv_de_pairs_args\s*\*", src)
    assert re.search(r"\bint32_t\s+spv_de_pairs_splits\s*\(", src)
    assert "spv_de_pairs" in _abi.EXPORTED_SYMBOLS and "spv_de_pairs_splits" in _abi.EXPORTED_SYMBOLS
    assert "spv_de.h" in HEADERS   # part of the staleness fingerprint
    build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "spv_de_pairs") and hasattr(lib, "spv_de_pairs_splits")
    res, args = _abi._SIGNATURES["spv_de_pairs"]
    assert res is ctypes.c_int and len(args) == 2


def test_de_pairs_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    fields = ["ld1", "rows1", "n_rows1", "n_genes", "delta", "stats", "ld_stats", "ws", "ws_bytes"]
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(spv_de_pairs_args),',
        "         " + ", ".join(f"offsetof(spv_de_pairs_args, {f})" for f in fields) + ");",
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = _abi.SpvDePairsArgs
    assert got == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    body = re.search(r"typedef struct spv_de_pairs_args \{(.*?)\} spv_de_pairs_args;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_fields = sum(d.count(",") + 1 for d in (x.strip() for x in body.split(";")) if d)
    assert n_fields == len(M._fields_)


def test_pair_splits_fill_the_chip_and_bound_the_fp32_chains():
    """spv_de_pairs_splits is plain host code: about 6144 waves (4 per workgroup) whatever n_genes is, never fewer than 16 pairs per wave"""
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    f = lib.spv_de_pairs_splits
    f.restype, f.argtypes = ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32]
    assert f(0, 10) == 0 and f(10, 0) == 0 and f(-1, -1) == 0
    assert f(1, 1) == 1 and f(10_000, 1) == 1
    for n_genes, n_pairs in ((64, 10_000), (1000, 10_000), (10_000, 10_000), (10_003, 777), (64, 1 << 20), (64, 1 << 24)):
        s, tiles = f(n_genes, n_pairs), (n_genes + 63) // 64
        assert 1 <= s <= n_pairs
        assert tiles * s * 4 <= 6144 + 4 * tiles   # not more waves than the target (rounded up to whole workgroups)
        assert s == 1 or n_pairs // (4 * (s - 1)) >= 16   # one split fewer would still leave >= 16 pairs per wave: s is not oversized
        assert tiles * s >= min(256, n_pairs // 64)   # a workgroup per CU wherever there are pairs for it
    assert f(64, 10_000) * 1 >= 150 and f(10_000, 10_000) * 157 >= 1024


def test_de_entry_points_exist_on_every_layer():
    import inspect
    from spvipes_amd import de_ops
    from spvipes_amd.model import spVIPES
    sig = inspect.signature(de_ops.de_pairs)
    assert list(sig.parameters)[:4] == ["bank1", "bank2", "rows1", "rows2"]
    for k in ("delta", "eps", "ws"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(spVIPES.differential_expression)
    assert list(sig.parameters)[1:] == ["group_indices_list", "group", "idx1", "idx2", "gene_list", "component", "library_size", "n_samples", "use_mean",
                                        "n_pairs", "delta", "pseudocount", "fdr_target", "max_cells", "seed", "batch_size", "_noise", "_pair_rows"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["idx2"], d["component"], d["library_size"], d["n_samples"], d["use_mean"]) == (None, "mixture", 1.0, 1, False)
    assert (d["n_pairs"], d["delta"], d["pseudocount"], d["fdr_target"], d["max_cells"], d["seed"]) == (10_000, 0.25, 0.0, 0.05, None, 0)
    assert "lfc_median" in spVIPES.differential_expression.__doc__   # its absence is stated


# ---- pairs ---------------------------------------------------------------------------------------------------------------------
def test_de_pair_rows_are_seeded_in_range_and_reproducible():
    from spvipes_amd.data import de_pair_rows
    r1, r2 = de_pair_rows(37, 5000, 4000, seed=3)
    assert r1.dtype == np.int32 and r2.dtype == np.int32 and r1.shape == r2.shape == (4000,)
    assert r1.min() >= 0 and r1.max() < 37 and r2.min() >= 0 and r2.max() < 5000
    assert len(np.unique(r1)) == 37 and r2.max() > 4000   # with replacement, over the whole range
    a1, a2 = de_pair_rows(37, 5000, 4000, seed=3)
    np.testing.assert_array_equal(r1, a1), np.testing.assert_array_equal(r2, a2)
    b1, b2 = de_pair_rows(37, 5000, 4000, seed=4)
    assert not np.array_equal(r1, b1) and not np.array_equal(r2, b2)
    rng = np.random.default_rng(3)   # the documented recipe: one generator, r1 first
    np.testing.assert_array_equal(r1, rng.integers(0, 37, 4000)), np.testing.assert_array_equal(r2, rng.integers(0, 5000, 4000))
    one = de_pair_rows(1, 1, 5, seed=0)
    assert one[0].tolist() == [0] * 5 and one[1].tolist() == [0] * 5
    for bad in (dict(rows_1=0, rows_2=3, n_pairs=5), dict(rows_1=3, rows_2=0, n_pairs=5), dict(rows_1=3, rows_2=3, n_pairs=0),
                dict(rows_1=3, rows_2=3, n_pairs=(1 << 24) + 1), dict(rows_1=3, rows_2=3, n_pairs=2.5), dict(rows_1=3, rows_2=3, n_pairs=True)):
        with pytest.raises(ValueError):
            de_pair_rows(**bad)


def test_de_argument_checks():
    from spvipes_amd.data import check_de_args
    assert check_de_args(10_000, 0.25, 0.0, 0.05) == (10_000, 0.25, 0.0, 0.05, None)
    assert check_de_args(np.int64(7), 0, 1e-6, 1, 50) == (7, 0.0, 1e-6, 1.0, 50)
    assert check_de_args(1 << 24, 0.25, 0.0, 0.0, None)[0] == 1 << 24
    for bad in (0, -1, (1 << 24) + 1, 1.5, True, "10", None):
        with pytest.raises(ValueError, match="n_pairs"):
            check_de_args(bad, 0.25, 0.0, 0.05)
    for bad in (-0.1, float("nan"), float("inf"), None, "x", True):
        with pytest.raises(ValueError, match="delta"):
            check_de_args(10, bad, 0.0, 0.05)
        with pytest.raises(ValueError, match="pseudocount"):
            check_de_args(10, 0.25, bad, 0.05)
    for bad in (-0.01, 1.01, float("nan"), None):
        with pytest.raises(ValueError, match="fdr_target"):
            check_de_args(10, 0.25, 0.0, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_cells"):
            check_de_args(10, 0.25, 0.0, 0.05, bad)


# ---- populations ---------------------------------------------------------------------------------------------------------------
def test_populations_resolve_to_positions_within_the_group_list():
    from spvipes_amd.data import de_populations, de_subsample
    gi = [40, 10, 30, 20, 50, 60]   # adata rows of the group, in the caller's order
    p1, p2 = de_populations(gi, [30, 40], [60, 10])
    assert p1.tolist() == [2, 0] and p2.tolist() == [5, 1]   # positions follow idx order
    p1, p2 = de_populations(gi, np.array([20]), None)
    assert p1.tolist() == [3] and p2.tolist() == [0, 1, 2, 4, 5]   # every other cell, in list order
    with pytest.raises(ValueError, match="cell 70 is not in group_indices_list\\[1\\]"):
        de_populations(gi, [10, 70], None, group=1)
    with pytest.raises(ValueError, match="idx2: cell 5 "):
        de_populations(gi, [10], [5])
    with pytest.raises(ValueError, match="overlap.*cell 30"):
        de_populations(gi, [10, 30], [30, 50])
    with pytest.raises(ValueError, match="idx1 is empty"):
        de_populations(gi, [], [10])
    with pytest.raises(ValueError, match="idx2 is empty"):
        de_populations(gi, [10], [])
    with pytest.raises(ValueError, match="leaves no cell"):
        de_populations(gi, gi, None)
    with pytest.raises(ValueError, match="more than once"):
        de_populations(gi, [10, 10], None)
    with pytest.raises(ValueError, match="integers"):
        de_populations(gi, [True, False, True, False, True, False], None)
    pos = np.arange(100)
    assert de_subsample(pos, None, 0) is pos and de_subsample(pos, 100, 0) is pos
    sub = de_subsample(pos, 10, 5)
    assert len(sub) == 10 and len(np.unique(sub)) == 10 and (np.diff(sub) > 0).all()
    np.testing.assert_array_equal(sub, de_subsample(pos, 10, 5))
    assert not np.array_equal(sub, de_subsample(pos, 10, 6))


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _stats(counts):
    n = len(counts)
    z = np.zeros(n, np.float32)
    return {"count_de": np.asarray(counts, np.float32), "lfc_mean": z + 1, "lfc_std": z + 2, "lfc_min": z + 3, "lfc_max": z + 4, "scale1": z + 5, "scale2": z + 6}


def test_de_table_probabilities_and_bayes_factor():
    from spvipes_amd.data import DE_COLUMNS, de_table
    t = de_table(_stats([0, 25, 50, 100]), 100, 0.05)
    assert list(t) == list(DE_COLUMNS) + ["is_de_fdr_0.05"]
    np.testing.assert_array_equal(t["proba_de"], [0.0, 0.25, 0.5, 1.0])
    np.testing.assert_array_equal(t["proba_not_de"], [1.0, 0.75, 0.5, 0.0])
    want = [math.log(1e-8) - math.log(1.0 + 1e-8), math.log(0.25 + 1e-8) - math.log(0.75 + 1e-8), 0.0, math.log(1.0 + 1e-8) - math.log(1e-8)]
    np.testing.assert_allclose(t["bayes_factor"], want, rtol=0, atol=1e-12)
    assert t["bayes_factor"][0] == -t["bayes_factor"][3] and abs(t["bayes_factor"][3] - 8 * math.log(10.0)) < 2e-8   # log(1 + 1e-8) - log(1e-8)
    for k, v in (("lfc_mean", 1), ("lfc_std", 2), ("lfc_min", 3), ("lfc_max", 4), ("scale1", 5), ("scale2", 6)):
        assert (t[k] == v).all()   # passed through


def test_de_table_fdr_set_by_hand():
    from spvipes_amd.data import de_table
    # proba_not_de, best first: 0.00, 0.02, 0.04, 0.10, 0.30 -> running means 0.00, 0.01, 0.02, 0.04, 0.092
    counts = [70, 100, 96, 90, 98]   # genes 1, 4, 2, 3, 0 by decreasing proba_de
    assert de_table(_stats(counts), 100, 0.05)["is_de_fdr_0.05"].tolist() == [False, True, True, True, True]   # 0.04 <= 0.05 < 0.092
    assert de_table(_stats(counts), 100, 0.025)["is_de_fdr_0.025"].tolist() == [False, True, True, False, True]   # 0.02 <= 0.025 < 0.04
    assert de_table(_stats(counts), 100, 0.005)["is_de_fdr_0.005"].tolist() == [False, True, False, False, False]
    assert de_table(_stats(counts), 100, 0.1)["is_de_fdr_0.1"].tolist() == [True] * 5
    # no gene qualifies: the best gene alone already has proba_not_de 0.1 > 0.05
    assert de_table(_stats([90, 80, 0]), 100, 0.05)["is_de_fdr_0.05"].tolist() == [False, False, False]
    assert de_table(_stats([0, 0]), 100, 0.05)["is_de_fdr_0.05"].tolist() == [False, False]
    # ties are taken in gene order: proba_not_de 0.00, 0.06, 0.06, 0.06 -> running means 0.00, 0.03, 0.04, 0.045; at 0.035 only the
    # first of the three tied genes fits
    tied = [94, 100, 94, 94]
    assert de_table(_stats(tied), 100, 0.035)["is_de_fdr_0.035"].tolist() == [True, True, False, False]
    assert de_table(_stats(tied), 100, 0.042)["is_de_fdr_0.042"].tolist() == [True, True, True, False]
    assert de_table(_stats(tied), 100, 0.05)["is_de_fdr_0.05"].tolist() == [True, True, True, True]
    assert de_table(_stats([100, 100, 100]), 100, 0.0)["is_de_fdr_0.0"].tolist() == [True, True, True]   # target 0: only certain genes
