"""CPU: the C ABI of spv_gram_f64 -- header, cross-compiled library, ctypes mirror against gcc, the slab plan and the workspace size at
hand-computed shapes, and what the wrapper REJECTS ahead of any HIP call, with which return code and which ``spv_last_error()`` text (in
the manner of tests/test_lisi_abi_cpu.py: pointers are made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q4, Q2 = 0x7F0000001000, 0x7F0000001004, 0x7F0000001002   # made-up device addresses: on a 16-byte boundary / 4 bytes / 2 bytes off one
FIELDS = ["x", "ld_x", "n_rows", "rows", "n_use", "n", "sums", "gram", "ld_gram", "ws", "ws_bytes"]


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_library_exports_and_binding_mirrors_the_three_symbols(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_gram_f64\s*\(\s*const\s+spv_gram_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_gram_slabs\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\buint64_t\s+spv_gram_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(rf"#define\s+SPV_GRAM_MAX_N\s+{_abi.GRAM_MAX_N}\b", src) and _abi.GRAM_MAX_N == 4096
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ("spv_gram_f64", "spv_gram_slabs", "spv_gram_ws_bytes"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    assert _abi._SIGNATURES["spv_gram_f64"] == (C.c_int, [C.POINTER(_abi.SpvGramArgs), C.c_void_p])
    assert _abi._SIGNATURES["spv_gram_slabs"] == (C.c_int32, [C.c_int32, C.c_int32])
    assert _abi._SIGNATURES["spv_gram_ws_bytes"] == (C.c_uint64, [C.c_int32, C.c_int32])


def test_the_new_header_is_part_of_the_build_fingerprint_and_marks_its_core():
    from spvipes_amd import build
    assert "spv_gram.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_gram.h"))
    text = open(os.path.join(build.CSRC, "spv_gram.h")).read()
    core = text[text.index("// ---- GRAM-CORE-BEGIN ----"):text.index("// ---- GRAM-CORE-END ----")]
    for name in ("gram_tile_of", "gram_slabs", "gram_slab_rows", "gram_ws_doubles", "gram_source_row", "gram_load", "gram_counts", "gram_operand", "gram_result_row", "gram_result_col",
                 "gram_add", "gram_merge"):
        assert name + "(" in core
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in text and "__builtin" not in core and not re.search(r"atomic\w*\s*\(", text)


def test_gram_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvGramArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_gram_args));',
        *[f'  printf(" %zu", offsetof(spv_gram_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_slab_plan_and_workspace_size_at_hand_computed_shapes(lib):
    """tiles = nt (nt + 1) / 2 with nt = ceil(n / 64); slabs = min(ceil(512 / tiles), n_use // 32, 128), 1 from 512 tiles on; bytes =
    slabs * (tiles * 4096 + nt * 64) * 8 beyond one slab"""
    s, w = lib.spv_gram_slabs, lib.spv_gram_ws_bytes
    assert s(64, 4096) == 128 and w(64, 4096) == 128 * (4096 + 64) * 8 == 4259840            # one tile: the slab cap
    assert s(24, 40) == 1 and w(24, 40) == 0                                                 # a duck-sized step: 40 // 32
    assert s(17, 70) == 2 and w(17, 70) == 2 * (4096 + 64) * 8
    assert s(130, 257) == 8 and w(130, 257) == 8 * (6 * 4096 + 3 * 64) * 8 == 1585152        # 6 tiles: 257 // 32
    assert s(512, 4096) == 15 and w(512, 4096) == 15 * (36 * 4096 + 512) * 8                 # 36 tiles: ceil(512 / 36)
    assert s(1984, 4096) == 2 and w(1984, 4096) == 2 * (496 * 4096 + 1984) * 8 == 32537600   # the largest workspace: 496 tiles twice
    assert s(1985, 4096) == 1 and s(2048, 4096) == 1 and s(4096, 1 << 30) == 1 and w(2048, 4096) == 0 and w(4096, 4096) == 0
    assert s(64, 63) == 1 and s(64, 64) == 2 and s(64, 31) == 1 and s(1, 0) == 1 and s(0, 100) == 1 and s(4097, 100) == 1 and s(64, -5) == 1
    assert w(0, 100) == 0 and w(4097, 4096) == 0 and w(64, 0) == 0
    assert max(w(n, 1 << 30) for n in range(1, 4097, 1)) == 32537600                         # the bound DESIGN.md section 26 states


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(x=P, ld_x=130, n_rows=257, rows=None, n_use=0, n=130, sums=P, gram=P, ld_gram=130, ws=P, ws_bytes=1585152), **o)
    s = _abi.SpvGramArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


W = "spv_gram_f64: "
REJECTIONS = [
    ("null-args", lambda: None, W + "null arguments"),
    ("null-x", lambda: _args(x=None), W + "null x"),
    ("null-sums", lambda: _args(sums=None), W + "null sums"),
    ("null-gram", lambda: _args(gram=None), W + "null gram"),
    ("null-ws-needed", lambda: _args(ws=None), W + "null ws"),
    ("n-0", lambda: _args(n=0), W + "n must lie in [1, 4096]"),
    ("n-4097", lambda: _args(n=4097, ld_x=4097, ld_gram=4097), W + "n must lie in [1, 4096]"),
    ("n_rows-negative", lambda: _args(n_rows=-1), W + "n_rows < 0"),
    ("n_use-negative", lambda: _args(rows=P, n_use=-1), W + "n_use < 0"),
    ("ld_x-short", lambda: _args(ld_x=129), W + "ld_x < n"),
    ("ld_gram-short", lambda: _args(ld_gram=129), W + "ld_gram < n"),
    ("x-misaligned", lambda: _args(x=Q2), W + "x must be 4-byte aligned"),
    ("sums-misaligned", lambda: _args(sums=Q4), W + "sums must be 8-byte aligned"),
    ("gram-misaligned", lambda: _args(gram=Q4), W + "gram must be 8-byte aligned"),
    ("ws-misaligned", lambda: _args(ws=Q4), W + "ws must be 8-byte aligned"),
    ("ws-short", lambda: _args(ws_bytes=1585151), W + "ws_bytes is less than spv_gram_ws_bytes(n, n_use)"),
    ("ws-short-listed-rows", lambda: _args(rows=P, n_use=64, ws_bytes=2 * (6 * 4096 + 192) * 8 - 8), W + "ws_bytes is less than spv_gram_ws_bytes(n, n_use)"),
    ("2:null-x-and-n", lambda: _args(x=None, n=0), W + "null x"),
    ("2:n-and-ld", lambda: _args(n=5000, ld_x=10), W + "n must lie in [1, 4096]"),
]


@pytest.mark.parametrize("name,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_gram_rejects_without_a_device(lib, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call (a null stream, no device here)"""
    rc = lib.spv_gram_f64(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text


def test_nothing_counted_succeeds_without_a_device(lib):
    """n_use == 0 with rows, or no rows at all: success ahead of any launch; a null ws is fine where the shape needs none"""
    assert lib.spv_gram_f64(_args(rows=P, n_use=0, ws=None, ws_bytes=0), None) == 0
    assert lib.spv_gram_f64(_args(n_rows=0, ws=None, ws_bytes=0), None) == 0
