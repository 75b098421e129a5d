"""CPU: the C ABI of spv_rank_stage / spv_rank_sums -- header, cross-compiled library, ctypes mirror against gcc, the pure shape
functions, and what the wrappers REJECT ahead of any HIP call, with which return code and which ``spv_last_error()`` text (in the manner
of tests/test_gram_abi_cpu.py: pointers are made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q4 = 0x7F0000001000, 0x7F0000001004   # made-up device addresses: on a 16-byte boundary / 4 bytes off one
FIELDS = ["x", "G", "n_rows", "n_piece", "pos_off", "n", "n_seg", "n_sel", "reset", "seg", "w", "genes", "rank2", "ld_rank2", "ties", "ws", "ws_bytes"]
SYMBOLS = ("spv_rank_stage", "spv_rank_sums", "spv_rank_gene_slab", "spv_rank_ws_bytes", "spv_rank_lds_capacity", "spv_rank_stage_tile", "spv_rank_sort_tile")


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_library_exports_and_binding_mirrors_the_symbols(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("spv_rank_stage", "spv_rank_sums"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+spv_rank_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
        assert _abi._SIGNATURES[name] == (C.c_int, [C.POINTER(_abi.SpvRankArgs), C.c_void_p])
    assert re.search(r"\bint64_t\s+spv_rank_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    for name in ("spv_rank_gene_slab", "spv_rank_lds_capacity", "spv_rank_stage_tile", "spv_rank_sort_tile"):
        assert re.search(rf"\bint32_t\s+{name}\s*\(\s*void\s*\)", src) and _abi._SIGNATURES[name] == (C.c_int32, [])
    assert _abi._SIGNATURES["spv_rank_ws_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    assert re.search(r"#define\s+SPV_RANK_MAX_N\s+\(1 << 20\)", src) and _abi.RANK_MAX_N == 1 << 20
    assert re.search(rf"#define\s+SPV_RANK_MAX_SEG\s+{_abi.RANK_MAX_SEG}\b", src) and _abi.RANK_MAX_SEG == 1024
    raw = C.CDLL(_abi.LIB_PATH)
    for name in SYMBOLS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)


def test_the_new_header_is_part_of_the_build_fingerprint_and_marks_its_core():
    from spvipes_amd import build
    assert "spv_rank.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_rank.h"))
    text = open(os.path.join(build.CSRC, "spv_rank.h")).read()
    core = text[text.index("// ---- RANK-CORE-BEGIN ----"):text.index("// ---- RANK-CORE-END ----")]
    for name in ("rank_ws_bytes", "rank_ws_half_off", "rank_key_bits", "rank_entry", "rank_bitonic_cx", "rank_digit", "rank_peers", "rank_run_begin", "rank_run_end",
                 "rank_elem_term", "rank_tie_term", "rank_zero_term"):
        assert name + "(" in core
    # integer atomics only: every atomicAdd of the file adds an int / unsigned / unsigned long long (no float or double operand anywhere near one)
    assert "__builtin_amdgcn" not in core and "atomic" not in core
    assert not re.search(r"atomicAdd\([^;]*(float|double|\d\.\d*f?\b)", text) and "unsafeAtomicAdd" not in text


def test_rank_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvRankArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_rank_args));',
        *[f'  printf(" %zu", offsetof(spv_rank_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_shape_functions_are_pure_and_aligned(lib):
    """bytes = 8192 (1024 gene cursors + 1024 segment counts, int32) + 2 halves * n * n_sel entries of 8 bytes; 0 outside the ranges"""
    w = lib.spv_rank_ws_bytes
    slab = lib.spv_rank_gene_slab()
    assert slab == 1024 and lib.spv_rank_lds_capacity() == 8192 and lib.spv_rank_stage_tile() == 128 and lib.spv_rank_sort_tile() == 1024
    assert w(1, 1) == 8192 + 16 and w(600, 40) == 8192 + 16 * 600 * 40 and w(50000, 1024) == 8192 + 16 * 50000 * 1024
    assert w(1 << 20, slab) == 8192 + 16 * (1 << 20) * 1024 > 2**32            # 64-bit arithmetic
    for n, s in ((0, 5), (5, 0), (-1, 5), (5, -3), ((1 << 20) + 1, 1), (1, slab + 1)):
        assert w(n, s) == 0
    for n, s in ((1, 1), (3, 7), (129, 65), (8193, 3)):
        assert w(n, s) % 8 == 0 and w(n, s) == w(n, s)
    assert [lib.spv_rank_gene_slab() for _ in range(3)] == [slab] * 3


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(G=40, n_rows=211, n_piece=600, pos_off=0, n=600, n_seg=5, n_sel=40, reset=1, seg=P, w=P, genes=None, rank2=P, ld_rank2=40, ties=P, ws=P,
                  ws_bytes=8192 + 16 * 600 * 40), **o)
    s = _abi.SpvRankArgs()
    s.x = _abi.SpvCounts(f.pop("X", P), f.pop("ld", 48), f.pop("rows", P), f.pop("col_off", 3), f.pop("dtype", 1))
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


BOTH = [
    ("null-args", lambda: None, "null arguments"),
    ("n-0", lambda: _args(n=0), "n must lie in [1, 2^20]"),
    ("n-above-cap", lambda: _args(n=(1 << 20) + 1), "n must lie in [1, 2^20]"),
    ("n_seg-0", lambda: _args(n_seg=0), "n_seg must lie in [1, 1024]"),
    ("n_seg-1025", lambda: _args(n_seg=1025), "n_seg must lie in [1, 1024]"),
    ("n_sel-0", lambda: _args(n_sel=0), "n_sel must lie in [1, spv_rank_gene_slab()]"),
    ("n_sel-above-slab", lambda: _args(n_sel=1025, ld_rank2=1025), "n_sel must lie in [1, spv_rank_gene_slab()]"),
    ("null-ws", lambda: _args(ws=None), "null ws"),
    ("ws-misaligned", lambda: _args(ws=Q4), "ws must be 8-byte aligned"),
    ("ws-short", lambda: _args(ws_bytes=8192 + 16 * 600 * 40 - 1), "ws_bytes is less than spv_rank_ws_bytes(n, n_sel)"),
]
STAGE = [
    ("null-matrix", lambda: _args(X=None), "null count matrix"),
    ("null-seg", lambda: _args(seg=None), "null seg"),
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
SUMS = [
    ("null-rank2", lambda: _args(rank2=None), "null rank2"),
    ("null-ties", lambda: _args(ties=None), "null ties"),
    ("ld_rank2-short", lambda: _args(ld_rank2=39), "ld_rank2 < n_sel"),
    ("rank2-misaligned", lambda: _args(rank2=Q4), "rank2 must be 8-byte aligned"),
    ("ties-misaligned", lambda: _args(ties=Q4), "ties must be 8-byte aligned"),
]
CASES = [("spv_rank_stage", *c) for c in BOTH + STAGE] + [("spv_rank_sums", *c) for c in BOTH + SUMS]


@pytest.mark.parametrize("fn,name,make,text", CASES, ids=[f"{c[0][9:]}-{c[1]}" for c in CASES])
def test_rank_entry_points_reject_without_a_device(lib, fn, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call (a null stream, no device here)"""
    rc = getattr(lib, fn)(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"{fn}: {text}"
