"""CPU: the host side of the exact lfc median and of one-label-against-the-rest differential expression: the C ABI of spv_de_median
(header, cross-compiled library, ctypes mirror), the lfc_median column of de_table, and the label / population / bank-row bookkeeping
of differential_expression_by.  No GPU calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_spv_de_median():
    from spvipes_amd import _abi
    from spvipes_amd.build import HEADERS, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_de_median\s*\(\s*const\s+spv_de_median_args\s*\*", src)
    assert re.search(r"\bint64_t\s+spv_de_median_ws_bytes\s*\(\s*int32_t\s+n_genes\s*,\s*int32_t\s+n_pairs\s*\)", src)
    assert "spv_de_median" in _abi.EXPORTED_SYMBOLS and "spv_de_median_ws_bytes" in _abi.EXPORTED_SYMBOLS
    assert "spv_de_median.h" in HEADERS   # part of the staleness fingerprint
    build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "spv_de_median") and hasattr(lib, "spv_de_median_ws_bytes")
    res, args = _abi._SIGNATURES["spv_de_median"]
    assert res is ctypes.c_int and len(args) == 2


def test_de_median_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    fields = ["ld1", "rows1", "n_rows1", "n_genes", "n_pairs", "eps", "mid", "ld_mid", "ws", "ws_bytes"]
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(spv_de_median_args),',
        "         " + ", ".join(f"offsetof(spv_de_median_args, {f})" for f in fields) + ");",
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)   # the header stays C99
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = _abi.SpvDeMedianArgs
    assert got == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    body = re.search(r"typedef struct spv_de_median_args \{(.*?)\} spv_de_median_args;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_fields = sum(d.count(",") + 1 for d in (x.strip() for x in body.split(";")) if d)
    assert n_fields == len(M._fields_)


def test_median_workspace_grows_with_genes_only():
    """spv_de_median_ws_bytes is plain host code: 0 for a non-positive argument, and never anything like n_pairs x n_genes"""
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    f = lib.spv_de_median_ws_bytes
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]
    assert f(0, 10) == 0 and f(10, 0) == 0 and f(-1, -1) == 0
    for n_genes in (1, 64, 10_003, 40_000):
        sizes = {f(n_genes, n_pairs) for n_pairs in (1, 777, 10_000, 1 << 24)}
        assert len(sizes) == 1   # the pairs do not enter
        b = sizes.pop()
        assert 0 < b <= 4096 * n_genes and b % 4 == 0 and b >= 256 * 4 * n_genes   # 256 uint32 bins per gene, and little more
    assert f(40_000, 1 << 24) < 1 << 26   # 670 GB it is not


def test_median_entry_points_exist_on_every_layer():
    import inspect
    from spvipes_amd import de_ops
    from spvipes_amd.model import spVIPES
    sig = inspect.signature(de_ops.de_median)
    assert list(sig.parameters) == ["bank1", "bank2", "rows1", "rows2", "eps", "ws", "out"]
    for k in ("eps", "ws", "out"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(de_ops.de_median_workspace).parameters) == ["n_genes", "n_pairs", "device"]
    sig = inspect.signature(spVIPES.differential_expression_by)
    assert list(sig.parameters)[1:] == ["group_indices_list", "group", "groupby", "labels", "gene_list", "component", "library_size", "n_samples", "use_mean",
                                        "n_pairs", "delta", "pseudocount", "fdr_target", "max_cells", "seed", "batch_size", "lfc_median", "_noise"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["labels"], d["component"], d["library_size"], d["n_samples"], d["use_mean"], d["lfc_median"]) == (None, "mixture", 1.0, 1, False, True)
    assert (d["n_pairs"], d["delta"], d["pseudocount"], d["fdr_target"], d["max_cells"], d["seed"]) == (10_000, 0.25, 0.0, 0.05, None, 0)
    one = inspect.signature(spVIPES.differential_expression)
    med = inspect.signature(spVIPES.differential_expression_median)
    assert [k for k in med.parameters if k != "lfc_median"] == list(one.parameters)   # the same call, plus the switch
    assert med.parameters["lfc_median"].default is True
    for k, q in one.parameters.items():
        assert med.parameters[k].default == q.default


# ---- the table -----------------------------------------------------------------------------------------------------------------
def _stats(counts):
    n = len(counts)
    z = np.zeros(n, np.float32)
    return {"count_de": np.asarray(counts, np.float32), "lfc_mean": z + 1, "lfc_std": z + 2, "lfc_min": z + 3, "lfc_max": z + 4, "scale1": z + 5, "scale2": z + 6}


def test_de_table_puts_lfc_median_after_lfc_mean_and_only_when_given():
    from spvipes_amd.data import DE_COLUMNS, de_table
    assert DE_COLUMNS == ("proba_de", "proba_not_de", "bayes_factor", "scale1", "scale2", "lfc_mean", "lfc_std", "lfc_min", "lfc_max")
    plain = de_table(_stats([0, 25, 50, 100]), 100, 0.05)
    assert list(plain) == list(DE_COLUMNS) + ["is_de_fdr_0.05"]
    st = _stats([0, 25, 50, 100])
    st["lfc_median"] = np.array([0.5, 1.5, 2.5, 3.5])
    t = de_table(st, 100, 0.05)
    cols = list(DE_COLUMNS)
    cols.insert(cols.index("lfc_mean") + 1, "lfc_median")
    assert list(t) == cols + ["is_de_fdr_0.05"]
    assert t["lfc_median"].dtype == np.float64 and t["lfc_median"].tolist() == [0.5, 1.5, 2.5, 3.5]
    for k in plain:   # every other column is what it is without the key
        np.testing.assert_array_equal(t[k], plain[k])
        assert t[k].dtype == plain[k].dtype


# ---- labels, populations, bank rows ----------------------------------------------------------------------------------------------
def test_label_populations_by_hand():
    from spvipes_amd.data import de_label_populations
    lab = np.array(["t", "b", "t", "nk", "b", "t", "nk", "b"])
    names, compared, kept, places = de_label_populations(lab)
    assert names.tolist() == ["b", "nk", "t"] and compared == [0, 1, 2]   # np.unique order
    assert kept.tolist() == list(range(8))
    assert places[0][0].tolist() == [1, 4, 7] and places[0][1].tolist() == [0, 2, 3, 5, 6]   # the label's cells / the rest, position order
    assert places[1][0].tolist() == [3, 6] and places[1][1].tolist() == [0, 1, 2, 4, 5, 7]
    assert places[2][0].tolist() == [0, 2, 5] and places[2][1].tolist() == [1, 3, 4, 6, 7]
    # labels= restricts what is compared, not what the rest is made of; the order stays the sorted one
    names, compared, kept, places = de_label_populations(lab, labels=["t", "b"])
    assert compared == [0, 2] and sorted(places) == [0, 2] and kept.tolist() == list(range(8))
    assert places[2][1].tolist() == [1, 3, 4, 6, 7]
    assert de_label_populations(np.array([3, 1, 2, 1]), labels=[2])[1] == [1]   # numeric labels
    with pytest.raises(KeyError, match="'x'"):
        de_label_populations(lab, labels=["t", "x"])
    with pytest.raises(ValueError, match="two distinct labels"):
        de_label_populations(np.array(["a", "a", "a"]))
    with pytest.raises(ValueError, match="no cells"):
        de_label_populations(np.array([]))
    with pytest.raises(ValueError, match="empty"):
        de_label_populations(lab, labels=[])


def test_label_populations_cap_each_label_with_its_own_seed():
    from spvipes_amd.data import de_label_populations, de_subsample
    rng = np.random.default_rng(0)
    lab = rng.choice(np.array([10, 20, 30]), size=200, p=[0.65, 0.3, 0.05])
    names, compared, kept, places = de_label_populations(lab, max_cells=25, seed=7)
    per = [de_subsample(np.nonzero(lab == v)[0], 25, 7 + 1 + k) for k, v in enumerate(names.tolist())]   # seed + 1 + k
    assert [len(p) for p in per] == [25, 25, int((lab == 30).sum())] and (lab == 30).sum() <= 25   # the small label is kept whole
    np.testing.assert_array_equal(kept, np.sort(np.concatenate(per)))
    assert (np.diff(kept) > 0).all()
    for k in compared:
        p1, p2 = places[k]
        np.testing.assert_array_equal(kept[p1], per[k])                                                    # the label's kept cells, position order
        np.testing.assert_array_equal(kept[p2], np.sort(np.concatenate([per[o] for o in compared if o != k])))   # rest = the others' kept cells
        assert len(p1) + len(p2) == len(kept)
    other = de_label_populations(lab, max_cells=25, seed=8)[2]
    assert not np.array_equal(other, kept)


def test_bank_rows_follow_the_per_population_numbering():
    """index i of a population = draw i // n_pop, its (i % n_pop)-th cell; the shared bank's row = draw * n_kept + that cell's place"""
    from spvipes_amd.data import de_bank_rows
    place, n_kept = np.array([1, 4, 7]), 8
    rows = de_bank_rows(np.arange(9), place, n_kept)   # three draws
    assert rows.dtype == np.int32 and rows.tolist() == [1, 4, 7, 9, 12, 15, 17, 20, 23]
    assert de_bank_rows(np.array([8, 0, 4, 4], np.int32), place, n_kept).tolist() == [23, 1, 12, 12]
    # the same thing said with banks: gathering the shared bank at the mapped rows gives the per-population bank's rows
    rng = np.random.default_rng(1)
    n_samples, kept_cells = 3, 8
    shared = rng.random((n_samples * kept_cells, 5))
    own = np.concatenate([shared[d * kept_cells + place] for d in range(n_samples)])   # row = draw * n_pop + i
    idx = rng.integers(0, len(own), 50)
    np.testing.assert_array_equal(shared[de_bank_rows(idx, place, kept_cells)], own[idx])
