"""CPU: the C ABI of spv_knn -- header, cross-compiled library, ctypes mirror, and what the wrapper REJECTS ahead of any HIP call, with
which return code and which ``spv_last_error()`` text (in the manner of tests/test_expression_stats_abi_cpu.py: pointers are made-up
device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q = 0x7F0000001000, 0x7F0000001002   # made-up device addresses: on a 16-byte boundary / 2 bytes off one
FIELDS = ["Q", "ld_q", "n_q", "C", "ld_c", "n_c", "D", "k", "exclude", "n_split", "idx", "dist", "ld_out", "ws"]


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_knn\s*\(\s*const\s+spv_knn_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_knn_splits\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint64_t\s+spv_knn_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_knn_tile_q\s*\(\s*void\s*\)", src) and re.search(r"\bint32_t\s+spv_knn_tile_c\s*\(\s*void\s*\)", src)
    for name, value in (("SPV_KNN_DMAX", _abi.KNN_DMAX), ("SPV_KNN_KMAX", _abi.KNN_KMAX), ("SPV_KNN_SPLIT_MAX", _abi.KNN_SPLIT_MAX)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src)
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ("spv_knn", "spv_knn_splits", "spv_knn_ws_bytes", "spv_knn_tile_q", "spv_knn_tile_c"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    res, args = _abi._SIGNATURES["spv_knn"]
    assert res is C.c_int and len(args) == 2
    assert _abi._SIGNATURES["spv_knn_ws_bytes"][0] is C.c_int64 and _abi._SIGNATURES["spv_knn_splits"][0] is C.c_int32


def test_the_new_header_is_part_of_the_build_fingerprint():
    from spvipes_amd import build
    assert "spv_knn.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_knn.h"))


def test_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvKnnArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_knn_args));',
        *[f'  printf(" %zu", offsetof(spv_knn_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=25, n_q=300, C=P, ld_c=25, n_c=260, D=25, k=15, exclude=None, n_split=2, idx=P, dist=P, ld_out=15, ws=P), **o)
    s = _abi.SpvKnnArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


W = "spv_knn: "
REJECTIONS = [
    ("null-args", lambda: None, W + "null arguments"),
    ("null-Q", lambda: _args(Q=None), W + "null Q"),
    ("null-C", lambda: _args(C=None), W + "null C"),
    ("null-idx", lambda: _args(idx=None), W + "null idx"),
    ("null-dist", lambda: _args(dist=None), W + "null dist"),
    ("null-ws-2-chunks", lambda: _args(ws=None), W + "null ws"),
    ("null-ws-automatic-chunks", lambda: _args(ws=None, n_split=0, n_q=1, n_c=10 ** 6), W + "null ws"),   # spv_knn_splits(1, 10^6) = 64
    ("misaligned-ws", lambda: _args(ws=Q), W + "ws must be 8-byte aligned"),
    ("D-0", lambda: _args(D=0), W + "D must lie in [1, 64]"),
    ("D-65", lambda: _args(D=65, ld_q=65, ld_c=65), W + "D must lie in [1, 64]"),
    ("k-0", lambda: _args(k=0), W + "k must lie in [1, 64]"),
    ("k-65", lambda: _args(k=65, ld_out=65), W + "k must lie in [1, 64]"),
    ("n_split-negative", lambda: _args(n_split=-1), W + "n_split must be 0 or lie in [1, 64]"),
    ("n_split-65", lambda: _args(n_split=65), W + "n_split must be 0 or lie in [1, 64]"),
    ("n_q-0", lambda: _args(n_q=0), W + "n_q < 1"),
    ("n_q-negative", lambda: _args(n_q=-4), W + "n_q < 1"),
    ("n_c-negative", lambda: _args(n_c=-1), W + "n_c < 0"),
    ("ld_q-short", lambda: _args(ld_q=24), W + "ld_q < D"),
    ("ld_c-short", lambda: _args(ld_c=24), W + "ld_c < D"),
    ("ld_out-short", lambda: _args(ld_out=14), W + "ld_out < k"),
    ("out-beyond-2^31", lambda: _args(n_q=1 << 20, ld_out=1 << 11, n_split=1), W + "n_q * ld_out exceeds 2^31 - 1"),
    ("ld_out-beyond-2^31", lambda: _args(n_q=1, ld_out=1 << 31, n_split=1), W + "n_q * ld_out exceeds 2^31 - 1"),
    ("ws-beyond-2^31", lambda: _args(n_q=1 << 20, k=64, ld_out=64, n_split=32), W + "the workspace (n_split * n_q * k entries) exceeds 2^31 - 1"),
    # which of two faults is reported
    ("2:null-Q-and-k", lambda: _args(Q=None, k=0), W + "null Q"),
    ("2:D-and-ld_q", lambda: _args(D=0, ld_q=-1), W + "D must lie in [1, 64]"),
    ("2:n_q-and-null-ws", lambda: _args(n_q=0, ws=None), W + "n_q < 1"),
]


@pytest.mark.parametrize("name,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_wrapper_rejects_without_a_device(lib, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_knn(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text
