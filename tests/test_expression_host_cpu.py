"""CPU: the host side of the denoised-expression read-out (spVIPES.get_normalized_expression): gene-list resolution, argument
checks, and the C ABI of spv_dec_expected (header, cross-compiled library, ctypes mirror).  No GPU calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")


# ---- gene-list resolution ----------------------------------------------------------------------------------------------------
NAMES = [np.array(["a0", "a1", "a2", "a3", "a4"]), np.array(["b0", "b1", "b2"])]


def test_gene_list_none_means_all_genes_of_every_group():
    from spvipes_amd.data import resolve_gene_list
    assert resolve_gene_list(None, [5, 3], NAMES) == [None, None]
    assert resolve_gene_list([None, None], [5, 3]) == [None, None]


def test_gene_list_positions_keep_order_and_repeats():
    from spvipes_amd.data import resolve_gene_list
    out = resolve_gene_list([[4, 0, 0, 2], np.array([1], dtype=np.int64)], [5, 3])
    assert out[0].dtype == np.int32 and out[0].tolist() == [4, 0, 0, 2]
    assert out[1].dtype == np.int32 and out[1].tolist() == [1]


def test_gene_list_names_resolve_like_positions_and_mix_per_group():
    from spvipes_amd.data import resolve_gene_list
    out = resolve_gene_list([["a3", "a0", "a3"], None], [5, 3], NAMES)
    assert out[0].tolist() == [3, 0, 3] and out[1] is None
    out = resolve_gene_list([None, ["b2"]], [5, 3], NAMES)
    assert out[0] is None and out[1].tolist() == [2]
    out = resolve_gene_list([[1, 2], ["b0", "b1"]], [5, 3], NAMES)   # positions for one group, names for the other
    assert out[0].tolist() == [1, 2] and out[1].tolist() == [0, 1]
    assert resolve_gene_list(["a1", None], [5, 3], NAMES)[0].tolist() == [1]   # a single name


def test_gene_list_errors_name_the_offender():
    from spvipes_amd.data import resolve_gene_list
    with pytest.raises(KeyError, match="nope"):
        resolve_gene_list([["a0", "nope"], None], [5, 3], NAMES)
    with pytest.raises(KeyError, match="b0"):   # a name of the OTHER group is unknown in this one
        resolve_gene_list([["b0"], None], [5, 3], NAMES)
    with pytest.raises(IndexError, match="5"):
        resolve_gene_list([[0, 5], None], [5, 3])
    with pytest.raises(IndexError, match="-1"):
        resolve_gene_list([None, [-1]], [5, 3])
    with pytest.raises(KeyError, match="var_names"):   # names, but the AnnData has none
        resolve_gene_list([["a0"], None], [5, 3], [None, None])
    with pytest.raises(ValueError):
        resolve_gene_list([[0]], [5, 3])   # one entry per group
    with pytest.raises(ValueError):
        resolve_gene_list([[], None], [5, 3])
    with pytest.raises(TypeError):
        resolve_gene_list([[0.5], None], [5, 3])
    with pytest.raises(TypeError):
        resolve_gene_list([[True, False, True, False, True], None], [5, 3])


def test_group_var_names_follow_get_loadings_lookup():
    from spvipes_amd.data import group_var_names
    from tests._duck import make_duck
    ad = make_duck(n=(4, 3), G=(5, 3))
    assert group_var_names(ad) == [None, None]
    ad.uns["groups_var_names"] = {"x": list(NAMES[0]), "y": list(NAMES[1])}
    got = group_var_names(ad)
    assert got[0].tolist() == NAMES[0].tolist() and got[1].tolist() == NAMES[1].tolist()
    ad.var_names = np.array([f"v{i}" for i in range(8)])   # var_names win, cut by the groups' own column indices
    got = group_var_names(ad)
    assert got[0].tolist() == ["v0", "v1", "v2", "v3", "v4"] and got[1].tolist() == ["v5", "v6", "v7"]


# ---- argument checks of get_normalized_expression -----------------------------------------------------------------------------
def test_expression_argument_checks():
    import math
    from spvipes_amd.data import check_expression_args, expression_log_library, expression_what
    assert [expression_what(c) for c in ("mixture", "private", "shared", "mixing")] == [0, 1, 2, 3]
    assert check_expression_args("mixture", "latent", 1, True) == (0, None, 1)
    what, log_l, n = check_expression_args("shared", 1e4, 7, False)
    assert (what, n) == (2, 7) and log_l == math.log(1e4)
    assert expression_log_library(1) == 0.0
    for bad in ("mean", "", None, 4, -1, True):
        with pytest.raises(ValueError):
            check_expression_args(bad, "latent", 1, True)
    for bad in (0, -3.0, float("nan"), float("inf"), "observed", None):
        with pytest.raises(ValueError):
            check_expression_args("mixture", bad, 1, True)
    with pytest.raises(ValueError, match="use_mean"):
        check_expression_args("mixture", "latent", 2, True)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            check_expression_args("mixture", "latent", bad, False)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_spv_dec_expected():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_dec_expected\s*\(\s*const\s+spv_dec_params\s*\*", src)
    assert "spv_dec_expected" in _abi.EXPORTED_SYMBOLS
    build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(lib, "spv_dec_expected")
    res, args = _abi._SIGNATURES["spv_dec_expected"]
    assert res is ctypes.c_int and len(args) == 3


def test_expected_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu %zu %zu %zu %zu\\n", sizeof(spv_dec_expected_args), offsetof(spv_dec_expected_args, genes),',
        "         offsetof(spv_dec_expected_args, out), offsetof(spv_dec_expected_args, ld_out), offsetof(spv_dec_expected_args, alpha));",
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = _abi.SpvDecExpectedArgs
    assert got == [ctypes.sizeof(M), M.genes.offset, M.out.offset, M.ld_out.offset, M.alpha.offset]
    body = re.search(r"typedef struct spv_dec_expected_args \{(.*?)\} spv_dec_expected_args;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_fields = sum(d.count(",") + 1 for d in (x.strip() for x in body.split(";")) if d)
    assert n_fields == len(M._fields_)


def test_read_out_entry_points_exist_on_every_layer():
    import inspect
    from spvipes_amd import dec_ops
    from spvipes_amd.model import spVIPES
    from spvipes_amd.module import spVIPESmodule
    sig = inspect.signature(dec_ops.expected_expression)
    for k in ("genes", "what", "library_size", "out", "alpha", "accumulate"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(spVIPESmodule.expected_expression)
    sig = inspect.signature(spVIPES.get_normalized_expression)
    assert list(sig.parameters)[1:] == ["group_indices_list", "gene_list", "library_size", "component", "n_samples", "use_mean", "batch_size",
                                        "return_numpy", "_noise"]
    assert sig.parameters["use_mean"].default is True and sig.parameters["component"].default == "mixture"
