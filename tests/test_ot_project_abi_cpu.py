"""CPU: the C ABI of spv_ot_project -- header, cross-compiled library, ctypes mirror, and what the wrapper REJECTS ahead of any HIP
call, with which return code and which ``spv_last_error()`` text (in the manner of tests/test_ot_segment_abi_cpu.py: pointers are
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
FIELDS = ["Q", "ld_q", "n_q", "C", "ld_c", "n_c", "D", "h", "inv_eps", "V", "ld_v", "n_v", "n_split", "out", "ld_out", "L", "ws"]
ENTRY_POINTS = ("spv_ot_project", "spv_ot_project_splits", "spv_ot_project_ws_bytes", "spv_ot_project_block")


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    i32 = r"\s*int32_t\s+\w+\s*"
    assert re.search(r"\bint\s+spv_ot_project\s*\(\s*const\s+spv_ot_proj_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(rf"\bint32_t\s+spv_ot_project_splits\s*\({i32},{i32},{i32}\)", src)
    assert re.search(rf"\bint64_t\s+spv_ot_project_ws_bytes\s*\({i32},{i32},{i32}\)", src)
    assert re.search(rf"\bint32_t\s+spv_ot_project_block\s*\({i32}\)", src)
    assert re.search(rf"#define\s+SPV_OT_VAL_MAX\s+{_abi.OT_VAL_MAX}\b", src) and _abi.OT_VAL_MAX == 256
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    res, args = _abi._SIGNATURES["spv_ot_project"]
    assert res is C.c_int and len(args) == 2
    assert _abi._SIGNATURES["spv_ot_project_ws_bytes"][0] is C.c_int64 and _abi._SIGNATURES["spv_ot_project_splits"][0] is C.c_int32


def test_the_new_header_is_part_of_the_build_fingerprint():
    from spvipes_amd import build
    assert "spv_ot_project.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_ot_project.h"))


def test_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvOtProjArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_ot_proj_args));',
        *[f'  printf(" %zu", offsetof(spv_ot_proj_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_the_other_ot_structs_are_untouched():
    """the new kernel has a struct of its own"""
    from spvipes_amd import _abi
    for M in (_abi.SpvOtArgs, _abi.SpvOtSegArgs):
        assert not {"V", "ld_v", "n_v", "out"} & {f for f, _ in M._fields_}


def test_shape_functions_without_a_device(lib):
    """pure functions of the shapes.  The chunk plan is spv_ot_splits' with the column blocks (of 32, whatever D) counted among the
    workgroups; the workspace is 4 bytes per (chunk, row, query) with n_v + 2 * ceil(n_v / 16) rows (the narrowest block width has the
    most (m, sum) rows), in 64-bit arithmetic"""
    tq, tc = lib.spv_ot_tile_q(), lib.spv_ot_tile_c()
    assert [lib.spv_ot_project_block(D) for D in (0, 1, 16, 17, 32, 33, 64, 65, -3)] == [0, 32, 32, 32, 32, 16, 16, 0, 0]
    for n_q, n_c, n_v in ((1, 0, 5), (0, 100, 5), (5, 100, 0), (1, 10 ** 6, 1), (300, 260, 25), (259, 2000, 1), (259, 2000, 256), (25000, 25000, 64),
                          (50000, 50000, 1), (50000, 50000, 256), (2 ** 31 - 1, 2 ** 31 - 1, 256)):
        wg = -(-n_q // tq) * -(-n_v // 32)
        want = 1 if (n_q < 1 or n_c < 1 or n_v < 1 or 2 * wg >= 1024) else max(1, min(-(-1024 // wg), n_c // (4 * tc), 64))
        assert lib.spv_ot_project_splits(n_q, n_c, n_v) == want, (n_q, n_c, n_v)
    for n_q, n_c in ((259, 2000), (300, 260), (50000, 50000), (1, 10 ** 6)):
        assert lib.spv_ot_project_splits(n_q, n_c, 1) == lib.spv_ot_project_splits(n_q, n_c, 32) == lib.spv_ot_splits(n_q, n_c)
    assert lib.spv_ot_project_splits(259, 2000, 1) == 7 and lib.spv_ot_project_splits(50000, 50000, 1) == 3 and lib.spv_ot_project_splits(50000, 50000, 64) == 1
    for bad in ((300, 7, 1), (300, 7, 0), (0, 7, 3), (300, 0, 3), (300, 7, -2), (-5, 7, 3)):
        assert lib.spv_ot_project_ws_bytes(*bad) == 0
    assert lib.spv_ot_project_ws_bytes(300, 7, 3) == 3 * (7 + 2) * 300 * 4
    assert lib.spv_ot_project_ws_bytes(300, 33, 3) == 3 * (33 + 2 * 3) * 300 * 4
    assert lib.spv_ot_project_ws_bytes(1 << 22, 256, 64) == 64 * (256 + 32) * (1 << 22) * 4   # beyond 32 bits


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=25, n_q=300, C=P, ld_c=25, n_c=260, D=25, h=P, inv_eps=2.0, V=P, ld_v=7, n_v=7, n_split=2, out=P, ld_out=300, L=P, ws=P), **o)
    s = _abi.SpvOtProjArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


# (name, arguments, text after "spv_ot_project: ")
REJECTIONS = [
    ("null-args", lambda: None, "null arguments"),
    ("null-Q", lambda: _args(Q=None), "null Q"),
    ("null-C", lambda: _args(C=None), "null C"),
    ("null-h", lambda: _args(h=None), "null h"),
    ("null-out", lambda: _args(out=None), "null out"),
    ("null-V", lambda: _args(V=None), "null V"),
    ("null-ws-2-chunks", lambda: _args(ws=None), "null ws"),
    ("null-ws-automatic-chunks", lambda: _args(ws=None, n_split=0, n_q=1, ld_out=1, n_c=10 ** 6), "null ws"),   # spv_ot_project_splits(1, 10^6, 7) = 64
    ("misaligned-ws", lambda: _args(ws=Q), "ws must be 8-byte aligned"),
    ("misaligned-ws-one-chunk", lambda: _args(ws=Q, n_split=1), "ws must be 8-byte aligned"),
    ("D-0", lambda: _args(D=0), "D must lie in [1, 64]"),
    ("D-65", lambda: _args(D=65, ld_q=65, ld_c=65), "D must lie in [1, 64]"),
    ("n_v-0", lambda: _args(n_v=0), "n_v must lie in [1, 256]"),
    ("n_v-257", lambda: _args(n_v=257, ld_v=257), "n_v must lie in [1, 256]"),
    ("n_split-negative", lambda: _args(n_split=-1), "n_split must be 0 or lie in [1, 64]"),
    ("n_split-65", lambda: _args(n_split=65), "n_split must be 0 or lie in [1, 64]"),
    ("n_q-0", lambda: _args(n_q=0), "n_q < 1"),
    ("n_q-negative", lambda: _args(n_q=-4), "n_q < 1"),
    ("n_c-negative", lambda: _args(n_c=-1), "n_c < 0"),
    ("ld_q-short", lambda: _args(ld_q=24), "ld_q < D"),
    ("ld_c-short", lambda: _args(ld_c=24), "ld_c < D"),
    ("ld_v-short", lambda: _args(ld_v=6), "ld_v < n_v"),
    ("ld_out-short", lambda: _args(ld_out=299), "ld_out < n_q"),
    ("inv_eps-0", lambda: _args(inv_eps=0.0), "inv_eps must be a positive finite number"),
    ("inv_eps-negative", lambda: _args(inv_eps=-1.0), "inv_eps must be a positive finite number"),
    ("inv_eps-inf", lambda: _args(inv_eps=float("inf")), "inv_eps must be a positive finite number"),
    ("inv_eps-nan", lambda: _args(inv_eps=float("nan")), "inv_eps must be a positive finite number"),
    ("out-beyond-2^31", lambda: _args(n_q=1 << 23, ld_out=1 << 23, n_v=256, ld_v=256, n_split=1), "n_v * ld_out exceeds 2^31 - 1"),
    ("ld_out-beyond-2^31", lambda: _args(n_q=1, ld_out=1 << 31, n_v=1, n_split=1), "n_v * ld_out exceeds 2^31 - 1"),
    ("ws-beyond-2^31", lambda: _args(n_q=1 << 20, ld_out=1 << 20, n_v=64, ld_v=64, n_split=32),
     "the workspace (n_split * (n_v + 2 * blocks) * n_q words) exceeds 2^31 - 1"),
    # which of two faults is reported
    ("2:null-Q-and-D", lambda: _args(Q=None, D=0), "null Q"),
    ("2:D-and-ld_q", lambda: _args(D=0, ld_q=-1), "D must lie in [1, 64]"),
    ("2:n_q-and-null-ws", lambda: _args(n_q=0, ws=None), "n_q < 1"),
    ("2:null-h-and-n_v", lambda: _args(h=None, n_v=0), "null h"),
    ("2:inv_eps-and-n_v", lambda: _args(inv_eps=0.0, n_v=0), "inv_eps must be a positive finite number"),
    ("2:n_v-and-ld_out", lambda: _args(n_v=257, ld_out=0), "n_v must lie in [1, 256]"),
    ("2:ld_out-and-null-ws", lambda: _args(ld_out=0, ws=None), "ld_out < n_q"),
]


@pytest.mark.parametrize("case,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_wrapper_rejects_without_a_device(lib, case, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_ot_project(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"spv_ot_project: {text}"
