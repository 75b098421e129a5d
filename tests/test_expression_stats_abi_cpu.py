"""CPU: the C ABI of spv_dec_expected_stats -- header, cross-compiled library, ctypes mirror, the workspace size, and what the wrapper
REJECTS ahead of any HIP call, with which return code and which ``spv_last_error()`` text (in the manner of
tests/test_abi_rejections_cpu.py: pointers are made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q = 0x7F0000001000, 0x7F0000001008   # made-up device addresses: on a 16-byte boundary / 8 bytes off one


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_dec_expected_stats\s*\(\s*const\s+spv_dec_params\s*\*\s*\w*\s*,\s*const\s+spv_dec_expected_stats_args\s*\*\s*\w*\s*,\s*void\s*\*", src)
    assert re.search(r"\bint64_t\s+spv_dec_expected_stats_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ("spv_dec_expected_stats", "spv_dec_expected_stats_ws_bytes"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    res, args = _abi._SIGNATURES["spv_dec_expected_stats"]
    assert res is C.c_int and len(args) == 3
    assert _abi._SIGNATURES["spv_dec_expected_stats_ws_bytes"][0] is C.c_int64


def test_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvDecExpectedStatsArgs
    fields = [f for f, _ in M._fields_]
    assert fields == ["Am_hi", "Am_lo", "Wm_hi", "Wm_lo", "K", "nsplit", "genes", "n_genes", "n_seg", "tile_seg", "tile_n", "stats", "ld_stats", "ws"]
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_dec_expected_stats_args));',
        *[f'  printf(" %zu", offsetof(spv_dec_expected_stats_args, {f}));' for f in fields],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in fields]
    shared = ("Am_hi", "Am_lo", "Wm_hi", "Wm_lo", "K", "nsplit", "genes", "n_genes")   # what _fill_readout fills: same names as spv_dec_expected_args
    assert all(f in [n for n, _ in _abi.SpvDecExpectedArgs._fields_] for f in shared)


def test_workspace_size(lib):
    """[cell tiles][8][n_genes] doubles; 4096 cells in 20 labels are at most 128 + 20 tiles: the 95 MB of DESIGN.md at 10 000 genes"""
    f = lib.spv_dec_expected_stats_ws_bytes
    assert f(83, 4) == 4 * 8 * 83 * 8 and f(1, 1) == 64
    assert f(10000, 148) == 148 * 8 * 10000 * 8 == 94_720_000
    assert f(50000, 1 << 15) == (1 << 15) * 8 * 50000 * 8   # beyond 2^31: 64-bit arithmetic
    assert f(0, 4) == 0 and f(83, 0) == 0 and f(-1, -1) == 0


def _dec_p(**o):
    """spv_dec_params with every pointer set: 128 cells x 64 genes, narrow layout (the baseline of tests/test_abi_rejections_cpu.py)"""
    from spvipes_amd import _abi
    ptrs = ("X", "logits", "Wps_hi", "Wps_lo", "Aps_hi", "Aps_lo", "gene_tab", "cnt_tab", "a_p", "a_s", "lse_p", "lse_s", "w_row", "part_max_p", "part_sum_p",
            "part_max_s", "part_sum_s", "rec_part", "tp_part", "ts_part", "dtheta_part", "dL", "tP", "tS")
    f = dict(dict({k: P for k in ptrs}, ldx=64, rows=None, col_off=0, count_is_u16=1, B=128, G=64, Bp=128, Gp=64, n_gene_tiles=2, logits_f32=0,
                  gene_splits=1, genes_per_split=64, grads_f32=0, nb_splits=1, nb_genes_per_split=64, nb_cell_tiles=1, kslots=0), **o)
    s = _abi.SpvDecParams()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Am_hi=P, Am_lo=None, Wm_hi=P, Wm_lo=None, K=64, nsplit=1, genes=None, n_genes=64, n_seg=2, tile_seg=P, tile_n=P, stats=P, ld_stats=64, ws=P), **o)
    s = _abi.SpvDecExpectedStatsArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


W = "spv_dec_expected_stats: "
REJECTIONS = [
    # null p / a / stats / ws / tile_seg / tile_n
    ("null-params", lambda: (None, _args()), "decoder: null params"),
    ("null-args", lambda: (_dec_p(), None), W + "null arguments"),
    ("null-stats", lambda: (_dec_p(), _args(stats=None)), W + "null pointer"),
    ("null-Am_hi", lambda: (_dec_p(), _args(Am_hi=None)), W + "null pointer"),
    ("null-a_s", lambda: (_dec_p(a_s=None), _args()), W + "null pointer"),
    ("null-ws", lambda: (_dec_p(), _args(ws=None)), W + "null workspace"),
    ("null-tile_seg", lambda: (_dec_p(), _args(tile_seg=None)), W + "null tile_seg"),
    ("null-tile_n", lambda: (_dec_p(), _args(tile_n=None)), W + "null tile_n"),
    # K not a multiple of 32 or above 320
    ("K-0", lambda: (_dec_p(), _args(K=0)), W + "K must be a multiple of 32, at most 320"),
    ("K-48", lambda: (_dec_p(), _args(K=48)), W + "K must be a multiple of 32, at most 320"),
    ("K-352", lambda: (_dec_p(), _args(K=352)), W + "K must be a multiple of 32, at most 320"),
    # n_genes, n_seg, ld_stats
    ("n_genes-0", lambda: (_dec_p(), _args(n_genes=0)), W + "n_genes must be positive (and at most G without a gene list)"),
    ("n_genes-negative", lambda: (_dec_p(), _args(n_genes=-2)), W + "n_genes must be positive (and at most G without a gene list)"),
    ("n_genes-65-no-list", lambda: (_dec_p(), _args(n_genes=65, ld_stats=65)), W + "n_genes must be positive (and at most G without a gene list)"),
    ("n_seg-0", lambda: (_dec_p(), _args(n_seg=0)), W + "n_seg < 1"),
    ("n_seg-negative", lambda: (_dec_p(), _args(n_seg=-3)), W + "n_seg < 1"),
    ("ld_stats-short", lambda: (_dec_p(), _args(ld_stats=63)), W + "ld_stats < n_genes"),
    # misaligned operand images, nsplit
    ("misaligned-Am_hi", lambda: (_dec_p(), _args(Am_hi=Q)), W + "operand images must be 16-byte aligned"),
    ("misaligned-Wm_hi", lambda: (_dec_p(), _args(Wm_hi=Q)), W + "operand images must be 16-byte aligned"),
    ("misaligned-Wm_lo", lambda: (_dec_p(), _args(nsplit=3, Am_lo=P, Wm_lo=Q)), W + "operand images must be 16-byte aligned"),
    ("nsplit-2", lambda: (_dec_p(), _args(nsplit=2)), W + "nsplit must be 1 or 3"),
    ("nsplit-0", lambda: (_dec_p(), _args(nsplit=0)), W + "nsplit must be 1 or 3"),
    ("nsplit-3-no-lo", lambda: (_dec_p(), _args(nsplit=3, Wm_lo=P)), W + "nsplit=3 needs lo images"),
    # the decoder parameters are checked as every decoder entry point checks them
    ("kslots-2", lambda: (_dec_p(kslots=2), _args()), "decoder: kslots must be 0 (16 / 32 K slots) or 1 (32 / 64)"),
    ("Bp-odd", lambda: (_dec_p(Bp=160), _args()), "decoder: Bp must be a multiple of 128 and Gp of 32"),
    # which of two faults is reported
    ("2:misaligned-and-n_seg", lambda: (_dec_p(), _args(Am_hi=Q, n_seg=0)), W + "operand images must be 16-byte aligned"),
    ("2:null-ws-and-ld_stats", lambda: (_dec_p(), _args(ws=None, ld_stats=0)), W + "null workspace"),
]


@pytest.mark.parametrize("name,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_wrapper_rejects_without_a_device(lib, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_dec_expected_stats(*make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text
