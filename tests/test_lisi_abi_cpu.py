"""CPU: the C ABI of spv_knn_paged and spv_lisi -- header, cross-compiled library, ctypes mirrors against gcc, the pure workspace size
function, and what the wrappers REJECT ahead of any HIP call, with which return code and which ``spv_last_error()`` text (in the manner
of tests/test_knn_abi_cpu.py: pointers are made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q = 0x7F0000001000, 0x7F0000001002   # made-up device addresses: on a 16-byte boundary / 2 bytes off one
LISI_FIELDS = ["idx", "dist", "ld", "n", "k", "codes", "n_c", "n_sets", "perplexity", "lisi", "beta", "n_valid", "converged"]


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_knn_paged\s*\(\s*const\s+spv_knn_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint64_t\s+spv_knn_paged_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint\s+spv_lisi\s*\(\s*const\s+spv_lisi_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    for name, value in (("SPV_KNN_PAGED_KMAX", _abi.KNN_PAGED_KMAX), ("SPV_LISI_KMAX", _abi.LISI_KMAX), ("SPV_LISI_SETS_MAX", _abi.LISI_SETS_MAX),
                        ("SPV_KNN_KMAX", 64)):   # the unpaged limit stays
        assert re.search(rf"#define\s+{name}\s+{value}\b", src)
    assert (_abi.KNN_PAGED_KMAX, _abi.LISI_KMAX, _abi.LISI_SETS_MAX, _abi.KNN_KMAX) == (256, 256, 8, 64)
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ("spv_knn_paged", "spv_knn_paged_ws_bytes", "spv_lisi"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    assert _abi._SIGNATURES["spv_knn_paged"] == (C.c_int, [C.POINTER(_abi.SpvKnnArgs), C.c_void_p])
    assert _abi._SIGNATURES["spv_lisi"] == (C.c_int, [C.POINTER(_abi.SpvLisiArgs), C.c_void_p])
    assert _abi._SIGNATURES["spv_knn_paged_ws_bytes"][0] is C.c_int64


def test_the_new_header_is_part_of_the_build_fingerprint():
    from spvipes_amd import build
    assert "spv_lisi.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_lisi.h"))
    core = open(os.path.join(build.CSRC, "spv_knn.h")).read()
    core = core[core.index("// ---- KNN-CORE-BEGIN ----"):core.index("// ---- KNN-CORE-END ----")]
    assert "knn_after(" in core and "__host__ __device__ __forceinline__ bool knn_after" in core   # the predicate sits in the core


def test_lisi_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvLisiArgs
    assert [f for f, _ in M._fields_] == LISI_FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_lisi_args));',
        *[f'  printf(" %zu", offsetof(spv_lisi_args, {f}));' for f in LISI_FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in LISI_FIELDS]


def test_workspace_size_is_a_pure_function(lib):
    w = lib.spv_knn_paged_ws_bytes
    assert w(50000, 89, 3) == 3 * 50000 * 64 * 8 and w(50000, 256, 3) == 3 * 50000 * 64 * 8 and w(50000, 15, 3) == 3 * 50000 * 15 * 8
    assert w(50000, 89, 1) == 0 and w(50000, 89, 0) == 0 and w(0, 89, 3) == 0 and w(5, 0, 3) == 0
    assert w(2 ** 31 - 1, 256, 64) == (2 ** 31 - 1) * 64 * 64 * 8     # 64-bit arithmetic
    for k in (1, 17, 64):
        assert w(300, k, 5) == lib.spv_knn_ws_bytes(300, k, 5)


def _knn(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=25, n_q=300, C=P, ld_c=25, n_c=260, D=25, k=89, exclude=None, n_split=2, idx=P, dist=P, ld_out=89, ws=P), **o)
    s = _abi.SpvKnnArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


W = "spv_knn_paged: "
PAGED_REJECTIONS = [
    ("null-args", lambda: None, W + "null arguments"),
    ("null-Q", lambda: _knn(Q=None), W + "null Q"),
    ("null-C", lambda: _knn(C=None), W + "null C"),
    ("null-idx", lambda: _knn(idx=None), W + "null idx"),
    ("null-dist", lambda: _knn(dist=None), W + "null dist"),
    ("null-ws-2-chunks", lambda: _knn(ws=None), W + "null ws"),
    ("null-ws-automatic-chunks", lambda: _knn(ws=None, n_split=0, n_q=1, n_c=10 ** 6), W + "null ws"),
    ("misaligned-ws", lambda: _knn(ws=Q), W + "ws must be 8-byte aligned"),
    ("D-0", lambda: _knn(D=0), W + "D must lie in [1, 64]"),
    ("D-65", lambda: _knn(D=65, ld_q=65, ld_c=65), W + "D must lie in [1, 64]"),
    ("k-0", lambda: _knn(k=0), W + "k must lie in [1, 256]"),
    ("k-257", lambda: _knn(k=257, ld_out=257), W + "k must lie in [1, 256]"),
    ("n_split-negative", lambda: _knn(n_split=-1), W + "n_split must be 0 or lie in [1, 64]"),
    ("n_split-65", lambda: _knn(n_split=65), W + "n_split must be 0 or lie in [1, 64]"),
    ("n_q-0", lambda: _knn(n_q=0), W + "n_q < 1"),
    ("n_c-negative", lambda: _knn(n_c=-1), W + "n_c < 0"),
    ("ld_q-short", lambda: _knn(ld_q=24), W + "ld_q < D"),
    ("ld_c-short", lambda: _knn(ld_c=24), W + "ld_c < D"),
    ("ld_out-short", lambda: _knn(ld_out=88), W + "ld_out < k"),
    ("ld_out-one-page-only", lambda: _knn(k=256, ld_out=64), W + "ld_out < k"),
    ("out-beyond-2^31", lambda: _knn(n_q=1 << 20, ld_out=1 << 11, n_split=1), W + "n_q * ld_out exceeds 2^31 - 1"),
    ("ld_out-beyond-2^31", lambda: _knn(n_q=1, ld_out=1 << 31, n_split=1), W + "n_q * ld_out exceeds 2^31 - 1"),
    ("ws-beyond-2^31", lambda: _knn(n_q=1 << 20, k=256, ld_out=256, n_split=32), W + "the workspace (n_split * n_q * min(k, 64) entries) exceeds 2^31 - 1"),
    ("2:null-Q-and-k", lambda: _knn(Q=None, k=0), W + "null Q"),
    ("2:n_q-and-null-ws", lambda: _knn(n_q=0, ws=None), W + "n_q < 1"),
]


@pytest.mark.parametrize("name,make,text", PAGED_REJECTIONS, ids=[c[0] for c in PAGED_REJECTIONS])
def test_knn_paged_rejects_without_a_device(lib, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_knn_paged(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text


def test_spv_knn_keeps_its_limit(lib):
    rc = lib.spv_knn(_knn(k=65, ld_out=65), None)
    assert rc == ERR_ARG and lib.spv_last_error().decode() == "spv_knn: k must lie in [1, 64]"


def _lisi(**o):
    from spvipes_amd import _abi
    f = dict(dict(idx=P, dist=P, ld=89, n=300, k=89, codes=P, n_c=300, n_sets=2, perplexity=30.0, lisi=P, beta=P, n_valid=P, converged=P), **o)
    s = _abi.SpvLisiArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


L = "spv_lisi: "
LISI_REJECTIONS = [
    ("null-args", lambda: None, L + "null arguments"),
    *[(f"null-{f}", (lambda f=f: _lisi(**{f: None})), L + f"null {f}") for f in ("idx", "dist", "codes", "lisi", "beta", "n_valid", "converged")],
    ("n-0", lambda: _lisi(n=0), L + "n < 1"),
    ("k-0", lambda: _lisi(k=0), L + "k must lie in [1, 256]"),
    ("k-257", lambda: _lisi(k=257, ld=257), L + "k must lie in [1, 256]"),
    ("ld-short", lambda: _lisi(ld=88), L + "ld < k"),
    ("n_c-negative", lambda: _lisi(n_c=-1), L + "n_c < 0"),
    ("n_sets-0", lambda: _lisi(n_sets=0), L + "n_sets must lie in [1, 8]"),
    ("n_sets-9", lambda: _lisi(n_sets=9), L + "n_sets must lie in [1, 8]"),
    ("perplexity-below-1", lambda: _lisi(perplexity=0.999), L + "perplexity must be a finite number >= 1"),
    ("perplexity-nan", lambda: _lisi(perplexity=float("nan")), L + "perplexity must be a finite number >= 1"),
    ("perplexity-inf", lambda: _lisi(perplexity=float("inf")), L + "perplexity must be a finite number >= 1"),
    ("2:null-idx-and-k", lambda: _lisi(idx=None, k=0), L + "null idx"),
    ("2:k-and-ld", lambda: _lisi(k=300, ld=10), L + "k must lie in [1, 256]"),
]


@pytest.mark.parametrize("name,make,text", LISI_REJECTIONS, ids=[c[0] for c in LISI_REJECTIONS])
def test_lisi_rejects_without_a_device(lib, name, make, text):
    rc = lib.spv_lisi(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text
