"""CPU: the host side of the raw-count statistics (spVIPES.count_statistics): signatures, the slab plan, the table assembly and
the one-vs-rest sums against numpy, the argument errors that are raised before anything touches the device, and the C ABI (the
library builds for gfx950 and exports the new symbols; the new args struct has the size the C header gives)."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spv_count_stats", "spv_count_stats_partial", "spv_count_stats_merge", "spv_count_stats_tile", "spv_count_stats_slab",
               "spv_count_stats_ws_bytes", "spv_count_totals", "spv_csr_totals")


def test_signatures_of_the_new_ops_and_method():
    from spvipes_amd import count_ops
    from spvipes_amd.model import spVIPES

    assert list(inspect.signature(count_ops.count_totals).parameters) == ["counts"]
    sig = inspect.signature(count_ops.count_stats)
    assert list(sig.parameters) == ["counts", "rows", "seg_sizes", "w", "genes", "ws", "out"]
    assert all(sig.parameters[k].default is None for k in ("w", "genes", "ws", "out"))
    sig = inspect.signature(spVIPES.count_statistics)
    assert list(sig.parameters) == ["self", "group_indices_list", "group", "idx1", "idx2", "groupby", "labels", "gene_list", "target_sum"]
    assert all(sig.parameters[k].default is None for k in ("idx1", "idx2", "groupby", "labels", "gene_list"))
    assert sig.parameters["target_sum"].default == 1e4


def test_the_three_de_methods_and_de_columns_are_untouched():
    from spvipes_amd import data
    from spvipes_amd.model import spVIPES

    assert data.DE_COLUMNS == ("proba_de", "proba_not_de", "bayes_factor", "scale1", "scale2", "lfc_mean", "lfc_std", "lfc_min", "lfc_max")
    assert data.COUNT_COLUMNS == ("raw_mean1", "raw_mean2", "non_zeros_proportion1", "non_zeros_proportion2", "raw_normalized_mean1",
                                  "raw_normalized_mean2")
    for name in ("differential_expression", "differential_expression_median", "differential_expression_by"):
        assert "target_sum" not in inspect.signature(getattr(spVIPES, name)).parameters


@pytest.mark.parametrize("sizes,slab", [([5], 4), ([0, 7, 0, 8, 1], 4), ([1024, 1, 1023, 0, 2053], 1024), ([0, 0], 8), ([3, 3, 3], 1)])
def test_slab_plan_covers_every_position_once_and_never_crosses_a_segment(sizes, slab):
    from spvipes_amd.data import count_slab_plan

    slabs, seg_slabs = count_slab_plan(sizes, slab)
    assert slabs.dtype == np.int32 and seg_slabs.dtype == np.int32 and slabs.shape[1] == 3 and seg_slabs.shape == (len(sizes) + 1,)
    seg_of = np.repeat(np.arange(len(sizes)), sizes)
    seen = np.zeros(sum(sizes), int)
    for b, e, k in slabs.tolist():
        assert 0 < e - b <= slab
        assert (seg_of[b:e] == k).all()
        seen[b:e] += 1
    assert (seen == 1).all()
    assert seg_slabs[0] == 0 and seg_slabs[-1] == len(slabs)
    for k, s in enumerate(sizes):
        own = slabs[seg_slabs[k]:seg_slabs[k + 1]]
        assert len(own) == -(-s // slab) and (own[:, 2] == k).all()
        assert int((own[:, 1] - own[:, 0]).sum()) == s
    assert (np.diff(slabs[:, 0]) > 0).all()


def test_slab_plan_refuses_bad_arguments():
    from spvipes_amd.data import count_slab_plan

    with pytest.raises(ValueError):
        count_slab_plan([3, -1], 4)
    with pytest.raises(ValueError):
        count_slab_plan([3], 0)


def test_rest_is_prefix_plus_suffix_and_exact_on_integers():
    from spvipes_amd.data import count_rest

    rng = np.random.default_rng(0)
    s = rng.integers(0, 1 << 40, size=(5, 3, 7)).astype(np.float64)
    s[2] = 0.0   # an empty segment
    rest = count_rest(s)
    want = np.stack([np.delete(s, k, axis=0).astype(np.int64).sum(0) for k in range(5)])
    assert rest.dtype == np.float64 and np.array_equal(rest, want.astype(np.float64))
    # no cancellation: a tiny segment next to a huge one keeps every bit, where total - own would lose it
    t = np.array([[1e-3], [1e20], [2e-3]])
    assert count_rest(t)[1, 0] == 1e-3 + 2e-3
    assert np.array_equal(count_rest(np.ones((1, 3, 2))), np.zeros((1, 3, 2)))


def test_table_assembly_against_numpy():
    from spvipes_amd.data import COUNT_COLUMNS, count_rest, count_table

    rng = np.random.default_rng(1)
    X = (rng.poisson(2.0, (40, 6)) * (rng.random((40, 6)) < 0.4)).astype(np.int64)
    lab = rng.integers(0, 3, 40)
    sums = np.stack([np.stack([X[lab == k].sum(0), (X[lab == k] != 0).sum(0), 3 * X[lab == k].sum(0)]) for k in range(3)]).astype(np.float64)
    rest = count_rest(sums)
    for k in range(3):
        n1, n2 = int((lab == k).sum()), int((lab != k).sum())
        t = count_table(sums[k], n1, rest[k], n2)
        assert tuple(t) == COUNT_COLUMNS and all(v.dtype == np.float64 and v.shape == (6,) for v in t.values())
        assert np.array_equal(t["raw_mean1"], X[lab == k].sum(0) / n1) and np.array_equal(t["raw_mean2"], X[lab != k].sum(0) / n2)
        assert np.array_equal(t["non_zeros_proportion1"], (X[lab == k] != 0).sum(0) / n1)
        assert np.array_equal(t["non_zeros_proportion2"], (X[lab != k] != 0).sum(0) / n2)
        assert np.array_equal(t["raw_normalized_mean1"], 3 * X[lab == k].sum(0) / n1)
        assert np.array_equal(t["raw_normalized_mean2"], 3 * X[lab != k].sum(0) / n2)
    with pytest.raises(ValueError):
        count_table(sums[0], 0, sums[1], 3)
    with pytest.raises(ValueError):
        count_table(sums[0][:2], 1, sums[1], 3)


def _bare_model():
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    m = spVIPES.__new__(spVIPES)   # the argument checks run before anything of the device is touched
    m.adata = make_duck(seed=2)
    return m, [list(range(300)), list(range(300, 560))]


def test_argument_errors_come_before_any_device_work():
    m, gil = _bare_model()
    with pytest.raises(ValueError, match="exactly one"):
        m.count_statistics(gil, 0)
    with pytest.raises(ValueError, match="exactly one"):
        m.count_statistics(gil, 0, idx1=[0, 1], groupby="cell_type")
    for bad in (0, -1.0, float("inf"), float("nan"), "1e4", None, True):
        with pytest.raises(ValueError, match="target_sum"):
            m.count_statistics(gil, 0, idx1=[0, 1], target_sum=bad)
    with pytest.raises(ValueError, match="group must be"):
        m.count_statistics(gil, 2, idx1=[0, 1])
    with pytest.raises(KeyError, match="not among the labels"):
        m.count_statistics(gil, 0, groupby="cell_type", labels=[99])
    with pytest.raises(KeyError, match="no column"):
        m.count_statistics(gil, 0, groupby="nope")
    with pytest.raises(ValueError, match="overlap"):
        m.count_statistics(gil, 0, idx1=[0, 1, 2], idx2=[2, 3])
    with pytest.raises(ValueError, match="not in group_indices_list"):
        m.count_statistics(gil, 0, idx1=[400])
    with pytest.raises(ValueError, match="labels goes with groupby"):
        m.count_statistics(gil, 0, idx1=[0], labels=[1])
    with pytest.raises(ValueError, match="idx2 goes with idx1"):
        m.count_statistics(gil, 0, groupby="cell_type", idx2=[1])


def test_check_target_sum_returns_a_float():
    from spvipes_amd.data import check_target_sum

    assert check_target_sum(10) == 10.0 and isinstance(check_target_sum(np.float32(2.5)), float)


def test_library_builds_and_exports_the_new_symbols():
    from spvipes_amd import _abi, build

    assert "spv_count_stats.h" in build.HEADERS
    build.build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spvipes_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _abi.EXPORTED_SYMBOLS and f"{n}(" in header
    lib = _abi.load()
    T, S = lib.spv_count_stats_tile(), lib.spv_count_stats_slab()
    assert T > 0 and T % 8 == 0
    assert 0 < S <= (2**31 - 1) // 65535   # a slab's uint16 counts add in 32-bit integers without overflow
    assert lib.spv_count_stats_ws_bytes(10, 3) == 3 * 3 * 10 * 8 and lib.spv_count_stats_ws_bytes(0, 3) == 0


def test_count_stats_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi

    src = tmp_path / "sizes.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "spvipes_hip.h")}"', "int main(void) {",
                              '  printf("%zu %zu %zu %zu %zu\\n", sizeof(spv_count_stats_args), offsetof(spv_count_stats_args, w), offsetof(spv_count_stats_args, n_sel),',
                              '         offsetof(spv_count_stats_args, out), offsetof(spv_count_stats_args, ws_bytes));', "  return 0;", "}"]))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = _abi.SpvCountStatsArgs
    assert got == [ctypes.sizeof(A), A.w.offset, A.n_sel.offset, A.out.offset, A.ws_bytes.offset]


def test_host_refuses_rows_outside_the_matrix_without_a_launch():
    """count_stats checks its arguments' types first; the row-range refusal itself needs device tensors and is covered on the GPU
    (tests/test_gpu_count_stats.py) -- here: a counts object of the wrong type never reaches the library"""
    from spvipes_amd import _abi, count_ops

    with pytest.raises(_abi.SpvError, match="GroupCounts"):
        count_ops.count_stats(object(), None, [1])
    with pytest.raises(_abi.SpvError, match="GroupCounts"):
        count_ops.count_totals(np.zeros((2, 2)))
