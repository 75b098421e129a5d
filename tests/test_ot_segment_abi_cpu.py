"""CPU: the C ABI of spv_ot_segment_lse -- header, cross-compiled library, ctypes mirror, and what the wrapper REJECTS ahead of any HIP
call, with which return code and which ``spv_last_error()`` text (in the manner of tests/test_ot_abi_cpu.py: pointers are made-up
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
FIELDS = ["Q", "ld_q", "n_q", "C", "ld_c", "n_c", "D", "h", "inv_eps", "seg_ptr", "n_seg", "n_split", "L", "ld_l", "ws"]
ENTRY_POINTS = ("spv_ot_segment_lse", "spv_ot_segment_splits", "spv_ot_segment_ws_bytes")


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_ot_segment_lse\s*\(\s*const\s+spv_ot_seg_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_ot_segment_splits\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint64_t\s+spv_ot_segment_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(rf"#define\s+SPV_OT_SEG_MAX\s+{_abi.OT_SEG_MAX}\b", src) and _abi.OT_SEG_MAX == 256
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    res, args = _abi._SIGNATURES["spv_ot_segment_lse"]
    assert res is C.c_int and len(args) == 2
    assert _abi._SIGNATURES["spv_ot_segment_ws_bytes"][0] is C.c_int64 and _abi._SIGNATURES["spv_ot_segment_splits"][0] is C.c_int32


def test_the_new_header_is_part_of_the_build_fingerprint():
    from spvipes_amd import build
    assert "spv_ot_segments.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_ot_segments.h"))


def test_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvOtSegArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_ot_seg_args));',
        *[f'  printf(" %zu", offsetof(spv_ot_seg_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_the_ot_args_struct_is_untouched():
    """the new kernel has a struct of its own: spv_ot_args keeps the fields tests/test_ot_abi_cpu.py pins"""
    from spvipes_amd import _abi
    assert not {"seg_ptr", "n_seg", "ld_l"} & {f for f, _ in _abi.SpvOtArgs._fields_}


def test_shape_functions_without_a_device(lib):
    """pure functions of the shapes: the chunk plan aims at several rounds of resident workgroups (5120 against spv_ot_splits' 1024),
    never at chunks of fewer than 4 LDS tiles, at most 64; the workspace is 8 bytes per (chunk, segment, query), in 64-bit arithmetic"""
    tq, tc = lib.spv_ot_tile_q(), lib.spv_ot_tile_c()
    for n_q, n_c in ((1, 0), (0, 100), (1, 10 ** 6), (300, 260), (259, 2000), (25000, 25000), (50000, 50000), (10 ** 6, 10 ** 6), (2 ** 31 - 1, 2 ** 31 - 1)):
        tiles = -(-n_q // tq)
        want = 1 if (n_q < 1 or n_c < 1 or tiles >= 5120) else max(1, min(-(-5120 // tiles), n_c // (4 * tc), 64))
        assert lib.spv_ot_segment_splits(n_q, n_c) == want, (n_q, n_c)
    assert lib.spv_ot_segment_splits(50000, 50000) == 14 and lib.spv_ot_splits(50000, 50000) == 3
    assert lib.spv_ot_segment_splits(1, 10 ** 6) == 64
    for bad in ((300, 7, 1), (300, 7, 0), (0, 7, 3), (300, 0, 3), (300, 7, -2), (-5, 7, 3)):
        assert lib.spv_ot_segment_ws_bytes(*bad) == 0
    assert lib.spv_ot_segment_ws_bytes(300, 7, 3) == 3 * 7 * 300 * 8
    assert lib.spv_ot_segment_ws_bytes(1 << 20, 256, 64) == 64 * 256 * (1 << 20) * 8   # beyond 32 bits


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=25, n_q=300, C=P, ld_c=25, n_c=260, D=25, h=P, inv_eps=2.0, seg_ptr=P, n_seg=7, n_split=2, L=P, ld_l=300, ws=P), **o)
    s = _abi.SpvOtSegArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


# (name, arguments, text after "spv_ot_segment_lse: ")
REJECTIONS = [
    ("null-args", lambda: None, "null arguments"),
    ("null-Q", lambda: _args(Q=None), "null Q"),
    ("null-C", lambda: _args(C=None), "null C"),
    ("null-h", lambda: _args(h=None), "null h"),
    ("null-seg_ptr", lambda: _args(seg_ptr=None), "null seg_ptr"),
    ("null-L", lambda: _args(L=None), "null L"),
    ("null-ws-2-chunks", lambda: _args(ws=None), "null ws"),
    ("null-ws-automatic-chunks", lambda: _args(ws=None, n_split=0, n_q=1, ld_l=1, n_c=10 ** 6), "null ws"),   # spv_ot_segment_splits(1, 10^6) = 64
    ("misaligned-ws", lambda: _args(ws=Q), "ws must be 8-byte aligned"),
    ("misaligned-ws-one-chunk", lambda: _args(ws=Q, n_split=1), "ws must be 8-byte aligned"),
    ("D-0", lambda: _args(D=0), "D must lie in [1, 64]"),
    ("D-65", lambda: _args(D=65, ld_q=65, ld_c=65), "D must lie in [1, 64]"),
    ("n_split-negative", lambda: _args(n_split=-1), "n_split must be 0 or lie in [1, 64]"),
    ("n_split-65", lambda: _args(n_split=65), "n_split must be 0 or lie in [1, 64]"),
    ("n_q-0", lambda: _args(n_q=0), "n_q < 1"),
    ("n_q-negative", lambda: _args(n_q=-4), "n_q < 1"),
    ("n_c-negative", lambda: _args(n_c=-1), "n_c < 0"),
    ("ld_q-short", lambda: _args(ld_q=24), "ld_q < D"),
    ("ld_c-short", lambda: _args(ld_c=24), "ld_c < D"),
    ("inv_eps-0", lambda: _args(inv_eps=0.0), "inv_eps must be a positive finite number"),
    ("inv_eps-negative", lambda: _args(inv_eps=-1.0), "inv_eps must be a positive finite number"),
    ("inv_eps-inf", lambda: _args(inv_eps=float("inf")), "inv_eps must be a positive finite number"),
    ("inv_eps-nan", lambda: _args(inv_eps=float("nan")), "inv_eps must be a positive finite number"),
    ("n_seg-0", lambda: _args(n_seg=0), "n_seg must lie in [1, 256]"),
    ("n_seg-257", lambda: _args(n_seg=257), "n_seg must lie in [1, 256]"),
    ("ld_l-short", lambda: _args(ld_l=299), "ld_l < n_q"),
    ("out-beyond-2^31", lambda: _args(n_q=1 << 23, ld_l=1 << 23, n_seg=256, n_split=1), "n_seg * ld_l exceeds 2^31 - 1"),
    ("ld_l-beyond-2^31", lambda: _args(n_q=1, ld_l=1 << 31, n_seg=1, n_split=1), "n_seg * ld_l exceeds 2^31 - 1"),
    ("ws-beyond-2^31", lambda: _args(n_q=1 << 20, ld_l=1 << 20, n_seg=64, n_split=32), "the workspace (n_split * n_seg * n_q entries) exceeds 2^31 - 1"),
    # which of two faults is reported
    ("2:null-Q-and-D", lambda: _args(Q=None, D=0), "null Q"),
    ("2:D-and-ld_q", lambda: _args(D=0, ld_q=-1), "D must lie in [1, 64]"),
    ("2:n_q-and-null-ws", lambda: _args(n_q=0, ws=None), "n_q < 1"),
    ("2:null-h-and-n_seg", lambda: _args(h=None, n_seg=0), "null h"),
    ("2:inv_eps-and-n_seg", lambda: _args(inv_eps=0.0, n_seg=0), "inv_eps must be a positive finite number"),
    ("2:n_seg-and-ld_l", lambda: _args(n_seg=257, ld_l=0), "n_seg must lie in [1, 256]"),
    ("2:ld_l-and-null-ws", lambda: _args(ld_l=0, ws=None), "ld_l < n_q"),
]


@pytest.mark.parametrize("case,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_wrapper_rejects_without_a_device(lib, case, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_ot_segment_lse(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"spv_ot_segment_lse: {text}"
