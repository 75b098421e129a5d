"""CPU: the C ABI of spv_tsne_repulsion / spv_tsne_affinities / spv_tsne_update -- header, cross-compiled library, ctypes mirrors, and what
the wrappers REJECT ahead of any HIP call, with which return code and which ``spv_last_error()`` text (in the manner of
tests/test_ot_project_abi_cpu.py: pointers are made-up device addresses the host code never dereferences).  No GPU calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q, P2 = 0x7F0000001000, 0x7F0000001002, 0x7F0000002000   # made-up device addresses: on a 16-byte boundary / 2 bytes off one / another
REP_FIELDS = ["Q", "ld_q", "n_q", "C", "ld_c", "n_c", "D", "exclude", "n_split", "Zrow", "F", "ld_f", "ws"]
UPD_FIELDS = ["y_in", "y_out", "ld_y", "n", "D", "indptr", "cols", "vals", "Zrow", "F", "ld_f", "Z", "u", "gain", "alpha", "momentum", "lr", "min_gain",
              "kl_row", "grad"]
ENTRY_POINTS = ("spv_tsne_repulsion", "spv_tsne_splits", "spv_tsne_ws_bytes", "spv_tsne_affinities", "spv_tsne_update")


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
    assert re.search(r"\bint\s+spv_tsne_repulsion\s*\(\s*const\s+spv_tsne_rep_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint\s+spv_tsne_update\s*\(\s*const\s+spv_tsne_upd_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint\s+spv_tsne_affinities\s*\(\s*const\s+float\s*\*", src)
    assert re.search(rf"\bint32_t\s+spv_tsne_splits\s*\({i32},{i32}\)", src)
    assert re.search(rf"\bint64_t\s+spv_tsne_ws_bytes\s*\({i32},{i32},{i32}\)", src)
    assert re.search(rf"#define\s+SPV_TSNE_DMAX\s+{_abi.TSNE_DMAX}\b", src) and _abi.TSNE_DMAX == 4
    assert re.search(r"#define\s+SPV_KNN_KMAX\s+64\b", src), "the neighbour limit stays 64"
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)


def test_the_new_header_is_part_of_the_build_fingerprint():
    from spvipes_amd import build
    assert "spv_tsne.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_tsne.h"))


@pytest.mark.parametrize("struct,mirror,fields", [("spv_tsne_rep_args", "SpvTsneRepArgs", REP_FIELDS), ("spv_tsne_upd_args", "SpvTsneUpdArgs", UPD_FIELDS)])
def test_args_structs_match_their_ctypes_mirrors(tmp_path, struct, mirror, fields):
    from spvipes_amd import _abi
    M = getattr(_abi, mirror)
    assert [f for f, _ in M._fields_] == fields
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        f'  printf("%zu", sizeof({struct}));',
        *[f'  printf(" %zu", offsetof({struct}, {f}));' for f in fields],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in fields]


def test_shape_functions_without_a_device(lib):
    """pure functions of the shapes: knn_splits' plan with a target of 8192 workgroups; the workspace is [chunk][1 + D][n_q] doubles in
    64-bit arithmetic"""
    tq, tc = lib.spv_knn_tile_q(), lib.spv_knn_tile_c()
    for n_q, n_c in ((1, 0), (0, 100), (1, 10 ** 6), (300, 260), (259, 2000), (25000, 25000), (50000, 50000), (100000, 100000), (2 ** 31 - 1, 2 ** 31 - 1)):
        tiles = -(-n_q // tq)
        want = 1 if (n_q < 1 or n_c < 1 or tiles >= 8192) else max(1, min(-(-8192 // tiles), n_c // (4 * tc), 64))
        assert lib.spv_tsne_splits(n_q, n_c) == want, (n_q, n_c)
    assert lib.spv_tsne_splits(300, 260) == 1 and lib.spv_tsne_splits(50000, 50000) == 21 and lib.spv_tsne_splits(1, 10 ** 6) == 64
    for bad in ((300, 2, 1), (300, 2, 0), (0, 2, 3), (300, 0, 3), (300, 2, -2), (-5, 2, 3)):
        assert lib.spv_tsne_ws_bytes(*bad) == 0
    assert lib.spv_tsne_ws_bytes(300, 2, 3) == 3 * 3 * 300 * 8
    assert lib.spv_tsne_ws_bytes(1 << 24, 4, 64) == 64 * 5 * (1 << 24) * 8   # beyond 32 bits


def _rep(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=2, n_q=300, C=P, ld_c=2, n_c=260, D=2, exclude=None, n_split=2, Zrow=P, F=P, ld_f=300, ws=P), **o)
    s = _abi.SpvTsneRepArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


REP_REJECTIONS = [
    ("null-args", lambda: None, "null arguments"),
    ("null-Q", lambda: _rep(Q=None), "null Q"),
    ("null-C", lambda: _rep(C=None), "null C"),
    ("null-Zrow", lambda: _rep(Zrow=None), "null Zrow"),
    ("null-F", lambda: _rep(F=None), "null F"),
    ("null-ws-2-chunks", lambda: _rep(ws=None), "null ws"),
    ("null-ws-automatic-chunks", lambda: _rep(ws=None, n_split=0, n_q=1, ld_f=1, n_c=10 ** 6), "null ws"),   # spv_tsne_splits(1, 10^6) = 64
    ("misaligned-ws", lambda: _rep(ws=Q), "ws must be 8-byte aligned"),
    ("misaligned-ws-one-chunk", lambda: _rep(ws=Q, n_split=1), "ws must be 8-byte aligned"),
    ("D-0", lambda: _rep(D=0), "D must lie in [1, 64]"),          # the scan's own check comes first
    ("D-5", lambda: _rep(D=5, ld_q=5, ld_c=5), "D must lie in [1, 4]"),
    ("D-65", lambda: _rep(D=65, ld_q=65, ld_c=65), "D must lie in [1, 64]"),
    ("n_split-negative", lambda: _rep(n_split=-1), "n_split must be 0 or lie in [1, 64]"),
    ("n_split-65", lambda: _rep(n_split=65), "n_split must be 0 or lie in [1, 64]"),
    ("n_q-0", lambda: _rep(n_q=0), "n_q < 1"),
    ("n_c-negative", lambda: _rep(n_c=-1), "n_c < 0"),
    ("ld_q-short", lambda: _rep(ld_q=1), "ld_q < D"),
    ("ld_c-short", lambda: _rep(ld_c=1), "ld_c < D"),
    ("ld_f-short", lambda: _rep(ld_f=299), "ld_f < n_q"),
    ("2:null-Q-and-D", lambda: _rep(Q=None, D=0), "null Q"),
    ("2:D-5-and-null-F", lambda: _rep(D=5, ld_q=5, ld_c=5, F=None), "D must lie in [1, 4]"),
    ("2:ld_f-and-null-ws", lambda: _rep(ld_f=0, ws=None), "ld_f < n_q"),
]


@pytest.mark.parametrize("case,make,text", REP_REJECTIONS, ids=[c[0] for c in REP_REJECTIONS])
def test_repulsion_rejects_without_a_device(lib, case, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_tsne_repulsion(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"spv_tsne_repulsion: {text}"


# (name, (d2, P, ld, n, k, perplexity, beta), text)
AFF_REJECTIONS = [
    ("null-d2", (None, P, 60, 300, 60, 20.0, P), "null d2"),
    ("null-P", (P, None, 60, 300, 60, 20.0, P), "null P"),
    ("null-beta", (P, P, 60, 300, 60, 20.0, None), "null beta"),
    ("n-0", (P, P, 60, 0, 60, 20.0, P), "n < 1"),
    ("k-0", (P, P, 60, 300, 0, 20.0, P), "k must lie in [1, 64]"),
    ("k-65", (P, P, 65, 300, 65, 20.0, P), "k must lie in [1, 64]"),
    ("ld-short", (P, P, 59, 300, 60, 20.0, P), "ld < k"),
    ("perplexity-below-1", (P, P, 60, 300, 60, 0.5, P), "perplexity must be a finite number >= 1"),
    ("perplexity-nan", (P, P, 60, 300, 60, float("nan"), P), "perplexity must be a finite number >= 1"),
    ("perplexity-inf", (P, P, 60, 300, 60, float("inf"), P), "perplexity must be a finite number >= 1"),
]


@pytest.mark.parametrize("case,args,text", AFF_REJECTIONS, ids=[c[0] for c in AFF_REJECTIONS])
def test_affinities_rejects_without_a_device(lib, case, args, text):
    rc = lib.spv_tsne_affinities(*args, None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"spv_tsne_affinities: {text}"


def _upd(**o):
    from spvipes_amd import _abi
    f = dict(dict(y_in=P, y_out=P2, ld_y=2, n=300, D=2, indptr=P, cols=P, vals=P, Zrow=P, F=P, ld_f=300, Z=P, u=P, gain=P, alpha=12.0, momentum=0.5,
                  lr=200.0, min_gain=0.01, kl_row=None, grad=None), **o)
    s = _abi.SpvTsneUpdArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


_NUMBERS = "alpha, momentum, lr and min_gain must be finite and not negative"
UPD_REJECTIONS = [("null-args", lambda: None, "null arguments")] + [(f"null-{f}", (lambda f=f: _upd(**{f: None})), f"null {f}")
                                                                    for f in ("y_in", "y_out", "indptr", "cols", "vals", "Zrow", "F", "Z", "u", "gain")] + [
    ("y_out-is-y_in", lambda: _upd(y_out=P), "y_out must not be y_in"),
    ("n-0", lambda: _upd(n=0), "n < 1"),
    ("D-0", lambda: _upd(D=0), "D must lie in [1, 4]"),
    ("D-5", lambda: _upd(D=5, ld_y=5), "D must lie in [1, 4]"),
    ("ld_y-short", lambda: _upd(ld_y=1), "ld_y < D"),
    ("ld_f-short", lambda: _upd(ld_f=299), "ld_f < n"),
    ("alpha-negative", lambda: _upd(alpha=-1.0), _NUMBERS),
    ("momentum-nan", lambda: _upd(momentum=float("nan")), _NUMBERS),
    ("lr-inf", lambda: _upd(lr=float("inf")), _NUMBERS),
    ("min_gain-negative", lambda: _upd(min_gain=-0.01), _NUMBERS),
    ("2:null-u-and-n", lambda: _upd(u=None, n=0), "null u"),
    ("2:n-and-D", lambda: _upd(n=0, D=0), "n < 1"),
]


@pytest.mark.parametrize("case,make,text", UPD_REJECTIONS, ids=[c[0] for c in UPD_REJECTIONS])
def test_update_rejects_without_a_device(lib, case, make, text):
    rc = lib.spv_tsne_update(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == f"spv_tsne_update: {text}"
