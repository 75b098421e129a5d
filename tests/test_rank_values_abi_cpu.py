"""CPU: the C ABI of spv_rank_values_stage / spv_rank_values -- header, cross-compiled library, ctypes mirror against gcc, the pure
shape function, and what the wrappers REJECT ahead of any HIP call, with which return code and which ``spv_last_error()`` text (in the
manner of tests/test_rank_abi_cpu.py: pointers are made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q4, Q2 = 0x7F0000001000, 0x7F0000001004, 0x7F0000001002   # made-up device addresses: on a 16-byte boundary / 4 bytes / 2 bytes off one
FIELDS = ["x", "G", "n_rows", "n_piece", "pos_off", "n", "n_sel", "reset", "w", "genes", "out", "ld_out", "ties", "nonzero", "ws", "ws_bytes"]
SYMBOLS = ("spv_rank_values_stage", "spv_rank_values", "spv_rank_values_ws_bytes")
NEED = 8192 + 20 * 600 * 40


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_library_exports_and_binding_mirrors_the_symbols(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("spv_rank_values_stage", "spv_rank_values"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+spv_rank_values_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
        assert _abi._SIGNATURES[name] == (C.c_int, [C.POINTER(_abi.SpvRankValuesArgs), C.c_void_p])
    assert re.search(r"\bint64_t\s+spv_rank_values_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert _abi._SIGNATURES["spv_rank_values_ws_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    raw = C.CDLL(_abi.LIB_PATH)
    for name in SYMBOLS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)


def test_the_new_header_is_part_of_the_build_fingerprint_and_marks_its_core():
    from spvipes_amd import build
    assert "spv_rank_values.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_rank_values.h"))
    text = open(os.path.join(build.CSRC, "spv_rank_values.h")).read()
    core = text[text.index("// ---- RANK-VALUES-CORE-BEGIN ----"):text.index("// ---- RANK-VALUES-CORE-END ----")]
    for name in ("rank_values_col_off", "rank_values_ws_bytes", "rank_value_zero", "rank_value_term", "rank_tr_row", "rank_tr_lane", "rank_tr_clamp", "rank_tr_src",
                 "rank_tr_dst"):
        assert name + "(" in core
    assert "__builtin_amdgcn" not in core and "atomic" not in core
    # the walk and the store use no atomic of any kind: the word appears in this header's comments only
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code.lower()
    rank = open(os.path.join(build.CSRC, "spv_rank.h")).read()
    rank_core = rank[rank.index("// ---- RANK-CORE-BEGIN ----"):rank.index("// ---- RANK-CORE-END ----")]
    assert "rank_pos_entry(" in rank_core and "rank_sort_column(" in rank and "rank_sort_column(" in code


def test_rank_values_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvRankValuesArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_rank_values_args));',
        *[f'  printf(" %zu", offsetof(spv_rank_values_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_the_workspace_size_is_pure_and_aligned(lib):
    """bytes = spv_rank_ws_bytes (8192 + 16 n n_sel) + the fp32 columns (4 n n_sel), rounded up to 8; 0 outside the ranges"""
    w, r = lib.spv_rank_values_ws_bytes, lib.spv_rank_ws_bytes
    slab = lib.spv_rank_gene_slab()
    assert w(1, 1) == 8192 + 16 + 8 and w(3, 1) == 8192 + 48 + 16 and w(600, 40) == NEED and w(50000, 1024) == 8192 + 20 * 50000 * 1024
    assert w(1 << 20, slab) == 8192 + 20 * (1 << 20) * 1024 > 2**32            # 64-bit arithmetic
    for n, s in ((0, 5), (5, 0), (-1, 5), (5, -3), ((1 << 20) + 1, 1), (1, slab + 1)):
        assert w(n, s) == 0
    for n, s in ((1, 1), (3, 7), (129, 65), (8193, 3)):
        assert w(n, s) % 8 == 0 and w(n, s) == (r(n, s) + 4 * n * s + 7) // 8 * 8 and w(n, s) == w(n, s)


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(G=40, n_rows=211, n_piece=600, pos_off=0, n=600, n_sel=40, reset=1, w=P, genes=None, out=P, ld_out=40, ties=P, nonzero=P, ws=P, ws_bytes=NEED), **o)
    s = _abi.SpvRankValuesArgs()
    s.x = _abi.SpvCounts(f.pop("X", P), f.pop("ld", 48), f.pop("rows", P), f.pop("col_off", 3), f.pop("dtype", 1))
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


BOTH = [
    ("null-args", lambda: None, "null arguments"),
    ("n-0", lambda: _args(n=0), "n must lie in [1, 2^20]"),
    ("n-above-cap", lambda: _args(n=(1 << 20) + 1), "n must lie in [1, 2^20]"),
    ("n_sel-0", lambda: _args(n_sel=0), "n_sel must lie in [1, spv_rank_gene_slab()]"),
    ("n_sel-above-slab", lambda: _args(n_sel=1025, ld_out=1025), "n_sel must lie in [1, spv_rank_gene_slab()]"),
    ("null-ws", lambda: _args(ws=None), "null ws"),
    ("ws-misaligned", lambda: _args(ws=Q4), "ws must be 8-byte aligned"),
    ("ws-short", lambda: _args(ws_bytes=NEED - 1), "ws_bytes is less than spv_rank_values_ws_bytes(n, n_sel)"),
    ("ws-of-the-rank-sums", lambda: _args(ws_bytes=8192 + 16 * 600 * 40), "ws_bytes is less than spv_rank_values_ws_bytes(n, n_sel)"),
]
STAGE = [
    ("null-matrix", lambda: _args(X=None), "null count matrix"),
    ("dtype", lambda: _args(dtype=2), "unknown count dtype"),
    ("G-0", lambda: _args(G=0), "G and n_rows must be positive"),
    ("n_rows-0", lambda: _args(n_rows=0), "G and n_rows must be positive"),
    ("piece-empty", lambda: _args(n_piece=0), "the piece [pos_off, pos_off + n_piece) must be non-empty and lie in [0, n)"),
    ("piece-negative-offset", lambda: _args(pos_off=-1), "the piece [pos_off, pos_off + n_piece) must be non-empty and lie in [0, n)"),
    ("piece-beyond-the-list", lambda: _args(pos_off=1), "the piece [pos_off, pos_off + n_piece) must be non-empty and lie in [0, n)"),
    ("no-rows-more-positions-than-rows", lambda: _args(rows=None), "without a row list n_piece must not exceed n_rows"),
    ("ld-short", lambda: _args(ld=42), "ld < col_off + G"),
    ("col_off-negative", lambda: _args(col_off=-1), "ld < col_off + G"),
    ("n_sel-above-G", lambda: _args(G=39, ws_bytes=1 << 30), "without a gene list n_sel must not exceed G"),
]
VALUES = [
    ("null-out", lambda: _args(out=None), "null out"),
    ("ld_out-short", lambda: _args(ld_out=39), "ld_out < n_sel"),
    ("out-misaligned", lambda: _args(out=Q2), "out must be 4-byte aligned"),
    ("ties-misaligned", lambda: _args(ties=Q4), "ties must be 8-byte aligned"),
    ("nonzero-misaligned", lambda: _args(nonzero=Q2), "nonzero must be 4-byte aligned"),
]
CASES = [("spv_rank_values_stage", *c) for c in BOTH + STAGE] + [("spv_rank_values", *c) for c in BOTH + VALUES]


@pytest.mark.parametrize("fn,name,make,text", CASES, ids=[f"{c[0][16:] or 'values'}-{c[1]}" for c in CASES])
def test_rank_values_entry_points_reject_without_a_device(lib, fn, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call (a null stream, no device here)"""
    rc = getattr(lib, fn)(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"{fn}: {text}"
