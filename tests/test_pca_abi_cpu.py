"""CPU: the C ABI of spv_pca_stage / spv_pca_project / spv_pca_back -- header, cross-compiled library, ctypes mirror against gcc, the
shape functions at hand-computed values, and what the wrappers REJECT ahead of any HIP call, with which return code and which
``spv_last_error()`` text (in the manner of tests/test_gram_abi_cpu.py: pointers are made-up device addresses the host code never
dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q4 = 0x7F0000001000, 0x7F0000001004   # made-up device addresses: on a 16-byte boundary / 4 bytes off one
FIELDS = ["x", "G", "n_rows", "n_piece", "pos_off", "n", "l", "w", "mu", "scale", "block", "ld_block", "V", "ld_v", "Y", "ld_y", "Z", "ld_z", "ws", "ws_bytes"]
ENTRIES = ("spv_pca_stage", "spv_pca_project", "spv_pca_back")


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_library_exports_and_binding_mirrors_the_six_symbols(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+spv_pca_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
        assert _abi._SIGNATURES[name] == (C.c_int, [C.POINTER(_abi.SpvPcaArgs), C.c_void_p])
    assert re.search(r"\bint32_t\s+spv_pca_slab\s*\(\s*void\s*\)", src) and re.search(r"\bint32_t\s+spv_pca_cell_tile\s*\(\s*void\s*\)", src)
    assert re.search(r"\bint64_t\s+spv_pca_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert _abi._SIGNATURES["spv_pca_slab"] == (C.c_int32, []) and _abi._SIGNATURES["spv_pca_cell_tile"] == (C.c_int32, [])
    assert _abi._SIGNATURES["spv_pca_ws_bytes"] == (C.c_int64, [C.c_int32, C.c_int32, C.c_int32])
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ENTRIES + ("spv_pca_slab", "spv_pca_cell_tile", "spv_pca_ws_bytes"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)


def test_the_new_header_is_part_of_the_build_fingerprint_and_marks_its_core():
    from spvipes_amd import build
    assert "spv_pca.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_pca.h"))
    text = open(os.path.join(build.CSRC, "spv_pca.h")).read()
    core = text[text.index("// ---- PCA-CORE-BEGIN ----"):text.index("// ---- PCA-CORE-END ----")]
    for name in ("pca_slabs", "pca_ws_floats", "pca_ws_at", "pca_position", "pca_source", "pca_pj_gene", "pca_pj_cell", "pca_col", "pca_k4", "pca_operand_at",
                 "pca_result_row", "pca_result_col", "pca_log1p", "pca_operand", "pca_merge"):
        assert name + "(" in core
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in text and "v_mfma_f32_32x32x2" in text
    assert "__builtin" not in core and "atomic" not in text.lower()


def test_pca_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvPcaArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_pca_args));',
        *[f'  printf(" %zu", offsetof(spv_pca_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_shape_functions_at_hand_computed_values(lib):
    """slab 1024 (it divides the CSR chunk of 4096), cell tile 64; bytes = 4 * ceil(n_piece / 1024) * round_up(G, 64) * l"""
    from spvipes_amd.count_ops import COUNT_CHUNK_ROWS
    w = lib.spv_pca_ws_bytes
    assert lib.spv_pca_slab() == 1024 and COUNT_CHUNK_ROWS % lib.spv_pca_slab() == 0 and lib.spv_pca_cell_tile() == 64
    assert w(200, 70, 16) == 4 * 1 * 256 * 16 == 16384
    assert w(97, 2 * 1024 + 37, 48) == 4 * 3 * 128 * 48 == 73728
    assert w(64, 1024, 64) == 4 * 1 * 64 * 64 and w(65, 1025, 32) == 4 * 2 * 128 * 32
    assert w(10000, 4096, 64) == 4 * 4 * 10048 * 64 == 10289152
    assert w(10000, 16384, 64) == 4 * 16 * 10048 * 64 == 41156608
    assert w(0, 70, 16) == 0 and w(200, 0, 16) == 0 and w(200, 70, 40) == 0 and w(200, 70, 0) == 0 and w(-1, -1, 64) == 0


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(G=200, n_rows=90, n_piece=70, pos_off=0, n=70, l=32, w=P, mu=P, scale=P, block=P, ld_block=200, V=P, ld_v=32, Y=P, ld_y=32,
                  Z=P, ld_z=32, ws=P, ws_bytes=4 * 256 * 32), **o)
    x = dict(X=P, ld=205, rows=P, col_off=5, dtype=1)
    for k in list(f):
        if k.startswith("x_"):
            x[k[2:]] = f.pop(k)
    s = _abi.SpvPcaArgs()
    for k, v in x.items():
        setattr(s.x, k, v)
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


ALL, YL, ST, PJ, BK = ENTRIES, ENTRIES[1:], ENTRIES[:1], ENTRIES[1:2], ENTRIES[2:]
PIECE = "the piece [pos_off, pos_off + n_piece) must be non-empty and lie in [0, n)"
REJECTIONS = [
    ("null-args", ALL, lambda: None, "null arguments"),
    ("null-matrix", ALL, lambda: _args(x_X=None), "null count matrix"),
    ("dtype-2", ALL, lambda: _args(x_dtype=2), "unknown count dtype"),
    ("dtype-negative", ALL, lambda: _args(x_dtype=-1), "unknown count dtype"),
    ("G-0", ALL, lambda: _args(G=0), "G and n_rows must be positive"),
    ("n_rows-0", ALL, lambda: _args(n_rows=0), "G and n_rows must be positive"),
    ("n-0", ALL, lambda: _args(n=0), "n < 1"),
    ("n_piece-0", ALL, lambda: _args(n_piece=0), PIECE),
    ("pos_off-negative", ALL, lambda: _args(pos_off=-1024), PIECE),
    ("piece-past-the-list", ALL, lambda: _args(n_piece=71), PIECE),
    ("piece-past-the-list-offset", ALL, lambda: _args(n=2000, pos_off=1024, n_piece=977), PIECE),
    ("no-row-list-short-matrix", ALL, lambda: _args(x_rows=None, n_rows=69), "without a row list n_piece must not exceed n_rows"),
    ("ld-short", ALL, lambda: _args(x_ld=204), "ld < col_off + G"),
    ("col_off-negative", ALL, lambda: _args(x_col_off=-1), "ld < col_off + G"),
    ("null-block", ST, lambda: _args(block=None), "null block"),
    ("ld_block-short", ST, lambda: _args(ld_block=199), "ld_block < G"),
    ("l-0", YL, lambda: _args(l=0), "l must be 16, 32, 48 or 64"),
    ("l-40", YL, lambda: _args(l=40), "l must be 16, 32, 48 or 64"),
    ("l-80", YL, lambda: _args(l=80, ld_v=80, ld_y=80, ld_z=80), "l must be 16, 32, 48 or 64"),
    ("null-Y", YL, lambda: _args(Y=None), "null Y"),
    ("ld_y-short", YL, lambda: _args(ld_y=31), "ld_y < l"),
    ("null-V", PJ, lambda: _args(V=None), "null V"),
    ("ld_v-short", PJ, lambda: _args(ld_v=31), "ld_v < l"),
    ("pos_off-off-a-slab", BK, lambda: _args(n=2000, pos_off=512, n_piece=70), "pos_off must be a multiple of spv_pca_slab()"),
    ("null-Z", BK, lambda: _args(Z=None), "null Z"),
    ("Z-misaligned", BK, lambda: _args(Z=Q4), "Z must be 8-byte aligned"),
    ("ld_z-short", BK, lambda: _args(ld_z=31), "ld_z < l"),
    ("null-ws", BK, lambda: _args(ws=None), "null ws"),
    ("ws-misaligned", BK, lambda: _args(ws=Q4), "ws must be 8-byte aligned"),
    ("ws-short", BK, lambda: _args(ws_bytes=4 * 256 * 32 - 1), "ws_bytes is less than spv_pca_ws_bytes(G, n_piece, l)"),
    ("ws-short-two-slabs", BK, lambda: _args(n=1100, n_piece=1100, n_rows=1100), "ws_bytes is less than spv_pca_ws_bytes(G, n_piece, l)"),
    ("2:null-matrix-and-G", ALL, lambda: _args(x_X=None, G=0), "null count matrix"),
    ("2:l-and-null-Y", YL, lambda: _args(l=17, Y=None), "l must be 16, 32, 48 or 64"),
]
CASES = [(f"{name}-{entry[8:]}", entry, make, text) for name, entries, make, text in REJECTIONS for entry in entries]


@pytest.mark.parametrize("name,entry,make,text", CASES, ids=[c[0] for c in CASES])
def test_pca_rejects_without_a_device(lib, name, entry, make, text):
    """every case returns from an argument check, ahead of the first HIP call (a null stream, no device here)"""
    rc = getattr(lib, entry)(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"{entry}: {text}"
