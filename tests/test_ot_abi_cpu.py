"""CPU: the C ABI of spv_ot_softmin / spv_ot_topk -- header, cross-compiled library, ctypes mirror, and what the wrappers REJECT ahead of
any HIP call, with which return code and which ``spv_last_error()`` text (in the manner of tests/test_knn_abi_cpu.py: pointers are
made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q = 0x7F0000001000, 0x7F0000001002   # made-up device addresses: on a 16-byte boundary / 2 bytes off one
FIELDS = ["Q", "ld_q", "n_q", "C", "ld_c", "n_c", "D", "k", "h", "r", "inv_eps", "n_split", "L", "idx", "val", "ld_out", "mass", "ws"]
ENTRY_POINTS = ("spv_ot_softmin", "spv_ot_topk", "spv_ot_splits", "spv_ot_ws_bytes", "spv_ot_tile_q", "spv_ot_tile_c")


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("spv_ot_softmin", "spv_ot_topk"):
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+spv_ot_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_ot_splits\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint64_t\s+spv_ot_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_ot_tile_q\s*\(\s*void\s*\)", src) and re.search(r"\bint32_t\s+spv_ot_tile_c\s*\(\s*void\s*\)", src)
    for name, value in (("SPV_OT_DMAX", _abi.OT_DMAX), ("SPV_OT_KMAX", _abi.OT_KMAX), ("SPV_OT_SPLIT_MAX", _abi.OT_SPLIT_MAX)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src)
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    for name in ("spv_ot_softmin", "spv_ot_topk"):
        res, args = _abi._SIGNATURES[name]
        assert res is C.c_int and len(args) == 2
    assert _abi._SIGNATURES["spv_ot_ws_bytes"][0] is C.c_int64 and _abi._SIGNATURES["spv_ot_splits"][0] is C.c_int32


def test_the_new_header_is_part_of_the_build_fingerprint():
    from spvipes_amd import build
    assert "spv_ot.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_ot.h"))


def test_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvOtArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_ot_args));',
        *[f'  printf(" %zu", offsetof(spv_ot_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_shape_functions_without_a_device(lib):
    """pure functions of the shapes: the tiles, the chunk plan (spv_knn's) and the workspace, softmin's (k = 0) and topk's"""
    assert (lib.spv_ot_tile_q(), lib.spv_ot_tile_c()) == (lib.spv_knn_tile_q(), lib.spv_knn_tile_c())
    for n_q, n_c in ((1, 0), (1, 10 ** 6), (300, 260), (259, 2000), (50000, 50000), (10 ** 6, 10 ** 6)):
        assert lib.spv_ot_splits(n_q, n_c) == lib.spv_knn_splits(n_q, n_c)
    assert lib.spv_ot_ws_bytes(300, 0, 1) == 0 and lib.spv_ot_ws_bytes(300, 15, 0) == 0 and lib.spv_ot_ws_bytes(0, 15, 3) == 0 and lib.spv_ot_ws_bytes(300, -1, 3) == 0
    assert lib.spv_ot_ws_bytes(300, 0, 3) == 3 * 300 * 8 and lib.spv_ot_ws_bytes(300, 15, 3) == 3 * 300 * 15 * 8
    assert lib.spv_ot_ws_bytes(1 << 20, 64, 31) == 31 * (1 << 20) * 64 * 8   # beyond 32 bits


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=25, n_q=300, C=P, ld_c=25, n_c=260, D=25, k=15, h=P, r=P, inv_eps=2.0, n_split=2, L=P, idx=P, val=P, ld_out=15,
                  mass=P, ws=P), **o)
    s = _abi.SpvOtArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


# (name, arguments, text after "<entry point>: ", which entry points: "both", "softmin" or "topk")
REJECTIONS = [
    ("null-args", lambda: None, "null arguments", "both"),
    ("null-Q", lambda: _args(Q=None), "null Q", "both"),
    ("null-C", lambda: _args(C=None), "null C", "both"),
    ("null-h", lambda: _args(h=None), "null h", "both"),
    ("null-L", lambda: _args(L=None), "null L", "softmin"),
    ("null-r", lambda: _args(r=None), "null r", "topk"),
    ("null-idx", lambda: _args(idx=None), "null idx", "topk"),
    ("null-val", lambda: _args(val=None), "null val", "topk"),
    ("null-mass", lambda: _args(mass=None), "null mass", "topk"),
    ("null-ws-2-chunks", lambda: _args(ws=None), "null ws", "both"),
    ("null-ws-automatic-chunks", lambda: _args(ws=None, n_split=0, n_q=1, n_c=10 ** 6), "null ws", "both"),   # spv_ot_splits(1, 10^6) = 64
    ("misaligned-ws", lambda: _args(ws=Q), "ws must be 8-byte aligned", "both"),
    ("D-0", lambda: _args(D=0), "D must lie in [1, 64]", "both"),
    ("D-65", lambda: _args(D=65, ld_q=65, ld_c=65), "D must lie in [1, 64]", "both"),
    ("k-0", lambda: _args(k=0), "k must lie in [1, 64]", "topk"),
    ("k-65", lambda: _args(k=65, ld_out=65), "k must lie in [1, 64]", "topk"),
    ("n_split-negative", lambda: _args(n_split=-1), "n_split must be 0 or lie in [1, 64]", "both"),
    ("n_split-65", lambda: _args(n_split=65), "n_split must be 0 or lie in [1, 64]", "both"),
    ("n_q-0", lambda: _args(n_q=0), "n_q < 1", "both"),
    ("n_q-negative", lambda: _args(n_q=-4), "n_q < 1", "both"),
    ("n_c-negative", lambda: _args(n_c=-1), "n_c < 0", "both"),
    ("ld_q-short", lambda: _args(ld_q=24), "ld_q < D", "both"),
    ("ld_c-short", lambda: _args(ld_c=24), "ld_c < D", "both"),
    ("inv_eps-0", lambda: _args(inv_eps=0.0), "inv_eps must be a positive finite number", "both"),
    ("inv_eps-negative", lambda: _args(inv_eps=-1.0), "inv_eps must be a positive finite number", "both"),
    ("inv_eps-inf", lambda: _args(inv_eps=float("inf")), "inv_eps must be a positive finite number", "both"),
    ("inv_eps-nan", lambda: _args(inv_eps=float("nan")), "inv_eps must be a positive finite number", "both"),
    ("ld_out-short", lambda: _args(ld_out=14), "ld_out < k", "topk"),
    ("out-beyond-2^31", lambda: _args(n_q=1 << 20, ld_out=1 << 11, n_split=1), "n_q * ld_out exceeds 2^31 - 1", "topk"),
    ("ld_out-beyond-2^31", lambda: _args(n_q=1, ld_out=1 << 31, n_split=1), "n_q * ld_out exceeds 2^31 - 1", "topk"),
    ("ws-beyond-2^31-topk", lambda: _args(n_q=1 << 20, k=64, ld_out=64, n_split=32), "the workspace (n_split * n_q [* k] entries) exceeds 2^31 - 1", "topk"),
    ("ws-beyond-2^31-softmin", lambda: _args(n_q=(1 << 31) - 1, n_split=2), "the workspace (n_split * n_q [* k] entries) exceeds 2^31 - 1", "softmin"),
    # which of two faults is reported
    ("2:null-Q-and-D", lambda: _args(Q=None, D=0), "null Q", "both"),
    ("2:D-and-ld_q", lambda: _args(D=0, ld_q=-1), "D must lie in [1, 64]", "both"),
    ("2:n_q-and-null-ws", lambda: _args(n_q=0, ws=None), "n_q < 1", "both"),
    ("2:inv_eps-and-null-ws", lambda: _args(inv_eps=0.0, ws=None), "inv_eps must be a positive finite number", "both"),
]
CASES = [(f"{entry}-{name}", entry, make, text) for name, make, text, which in REJECTIONS for entry in ("softmin", "topk") if which in ("both", entry)]


@pytest.mark.parametrize("case,entry,make,text", CASES, ids=[c[0] for c in CASES])
def test_wrapper_rejects_without_a_device(lib, case, entry, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = getattr(lib, f"spv_ot_{entry}")(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"spv_ot_{entry}: {text}"


def test_softmin_ignores_the_topk_fields(lib):
    """k, r and the lists are not softmin's business: bad values there do not change which fault it reports"""
    rc = lib.spv_ot_softmin(_args(k=0, r=None, idx=None, val=None, mass=None, ld_out=0, D=0), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == "spv_ot_softmin: D must lie in [1, 64]"
