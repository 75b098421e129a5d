"""CPU: the host side of latent_silhouette / integration_scores -- the per-cell values and scores from the distance sums
(``data.silhouette_table`` against tests/_silhouette_reference.py fed with float64 sums: both sides run in fp64, so they agree to 1e-12
absolute), the arrangement by (label, group), the argument refusals of both methods ahead of any model access, the SIL-CORE text on
the CPU (tools/silhouette_host_check.py), and the C ABI of spv_silhouette_sums: header, exports, ctypes mirror, the pure size functions
and what the wrapper REJECTS ahead of any HIP call (made-up device addresses the host code never dereferences).  No GPU calls.  Every
test here needs the feature and fails without it."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests._silhouette_reference import group_silhouette_ref, scores_ref, silhouette_ref, sums_are_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
TOL = 1e-12


def _float64_sums(X64, codes, groups, n_labels):
    """the (label, group) distance sums of every cell, from the float64 distance matrix, in silhouette_segments' arrangement"""
    from spvipes_amd.data import silhouette_segments
    perm, seg_ptr, sizes = silhouette_segments(codes, groups, n_labels)
    D = np.sqrt(((X64[:, None, :] - X64[None, :, :]) ** 2).sum(-1))
    S = np.stack([D[:, perm[seg_ptr[s]:seg_ptr[s + 1]]].sum(axis=1) for s in range(len(sizes))], axis=1)
    return S, sizes


def _case(name):
    rng = np.random.default_rng(5)
    if name == "mixed":   # a singleton label (3), a label in one group only (2), a singleton (label, group) segment (label 1 in group 1)
        n = 60
        codes = rng.integers(0, 2, n)
        groups = rng.integers(0, 2, n)
        codes[:9], groups[:9] = 2, 0
        codes[9] = 3
        groups[codes == 1] = 0
        groups[np.flatnonzero(codes == 1)[0]] = 1
        X = rng.standard_normal((n, 7)) + codes[:, None]
        return X, codes, groups, 4
    if name == "identical":   # max(a, b) = 0 everywhere
        return np.ones((12, 3)), np.arange(12) % 3, np.arange(12) % 2, 3
    if name == "two-labels":
        n = 25
        return rng.standard_normal((n, 1)), np.arange(n) % 2, rng.integers(0, 2, n), 2
    if name == "absent-code":   # code 1 has no cell: its two segments are empty and it is nobody's neighbour
        n = 30
        return rng.standard_normal((n, 64)), (np.arange(n) % 2) * 2, rng.integers(0, 2, n), 3
    raise KeyError(name)


@pytest.mark.parametrize("name", ["mixed", "identical", "two-labels", "absent-code"])
def test_table_matches_the_definitions(name):
    from spvipes_amd.data import silhouette_scores, silhouette_table
    X, codes, groups, L = _case(name)
    S, sizes = _float64_sums(X, codes, groups, L)
    t = silhouette_table(S, sizes, codes, groups)
    s, a, b, near = silhouette_ref(X, codes)
    s_g = group_silhouette_ref(X, codes, groups)
    for got, want in ((t["silhouette_label"], s), (t["a"], a), (t["b"], b), (t["silhouette_group"], s_g)):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=0, atol=TOL)
    assert t["nearest_label"].tolist() == [int(u) for u in near]
    if name == "identical":
        assert (t["silhouette_label"] == 0).all() and (t["silhouette_group"] == 0).all() and (t["a"] == 0).all() and (t["b"] == 0).all()
        assert t["nearest_label"].tolist() == [0 if c else 1 for c in codes]   # every other label ties at 0: the one that sorts first
    if name == "mixed":
        assert t["silhouette_label"][9] == 0 and np.isnan(t["a"][9])                       # the singleton label
        assert np.isnan(t["silhouette_group"][codes == 2]).all() and np.isnan(t["silhouette_group"][9])   # labels of one group only
        lone = np.flatnonzero((codes == 1) & (groups == 1))
        assert len(lone) == 1 and t["silhouette_group"][lone[0]] == 0                       # the singleton (label, group) segment
        assert np.isfinite(t["silhouette_group"][codes == 0]).all()
    sc = silhouette_scores(t, sizes, codes)
    want_l, want_g = scores_ref(s, s_g, codes)
    assert abs(sc["label_asw"] - want_l) <= TOL
    assert (np.isnan(sc["group_asw"]) and np.isnan(want_g)) or abs(sc["group_asw"] - want_g) <= TOL
    assert 0.0 <= sc["label_asw"] <= 1.0


def test_one_label_and_one_group():
    from spvipes_amd.data import silhouette_scores, silhouette_table
    rng = np.random.default_rng(1)
    X, codes, groups = rng.standard_normal((10, 4)), np.zeros(10, dtype=int), np.zeros(10, dtype=int)
    S, sizes = _float64_sums(X, codes, groups, 1)
    t = silhouette_table(S, sizes, codes, groups)
    assert np.isnan(t["b"]).all() and np.isnan(t["silhouette_label"]).all() and (t["nearest_label"] == -1).all()
    assert np.isnan(t["silhouette_group"]).all() and np.isfinite(t["a"]).all()
    assert np.isnan(silhouette_scores(t, sizes, codes)["group_asw"])


def test_against_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    from spvipes_amd.data import silhouette_table
    for D in (1, 25, 35, 64):
        rng = np.random.default_rng(D)
        n = 80
        codes = rng.integers(0, 4, n)
        codes[codes == 3] = 0
        codes[0] = 3   # a singleton label
        X = rng.standard_normal((n, D)) + codes[:, None]
        groups = rng.integers(0, 2, n)
        S, sizes = _float64_sums(X, codes, groups, 4)
        got = silhouette_table(S, sizes, codes, groups)
        np.testing.assert_allclose(got["silhouette_label"], sk.silhouette_samples(X, codes), rtol=0, atol=TOL)


def test_segments():
    from spvipes_amd.data import silhouette_segments
    codes = np.array([2, 0, 2, 2, 0, 3, 2, 0])
    groups = np.array([1, 0, 0, 1, 0, 1, 0, 1])
    perm, seg_ptr, sizes = silhouette_segments(codes, groups, 5)
    assert perm.dtype == np.int64 and seg_ptr.dtype == np.int32 and sizes.dtype == np.int64
    assert sizes.tolist() == [2, 1, 0, 0, 2, 2, 0, 1, 0, 0]          # (0,0) (0,1) (1,0) (1,1) (2,0) (2,1) (3,0) (3,1) (4,0) (4,1)
    assert seg_ptr.tolist() == [0, 2, 3, 3, 3, 5, 7, 7, 8, 8, 8] and seg_ptr[-1] == len(codes)
    assert perm.tolist() == [1, 4, 7, 2, 6, 0, 3, 5]                 # within a segment: the given order
    assert sorted(perm.tolist()) == list(range(8))
    empty = silhouette_segments(np.zeros(0, dtype=int), np.zeros(0, dtype=int), 2)
    assert empty[0].size == 0 and empty[1].tolist() == [0] * 5 and empty[2].tolist() == [0] * 4
    for bad in (lambda: silhouette_segments([0, 5], [0, 1], 5), lambda: silhouette_segments([0], [2], 1), lambda: silhouette_segments([0], [0, 1], 1),
                lambda: silhouette_segments([0], [0], 0), lambda: silhouette_segments([0], [0], 129)):
        with pytest.raises(ValueError):
            bad()


def test_query_blocks():
    from spvipes_amd.data import silhouette_query_blocks
    assert silhouette_query_blocks(10, 32, 96) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert silhouette_query_blocks(10, 32, 1) == [(i, i + 1) for i in range(10)]
    assert silhouette_query_blocks(10, 32, 256 << 20) == [(0, 10)]


def test_refusals_come_before_the_model_and_signatures():
    from spvipes_amd.data import check_silhouette_args
    from spvipes_amd.model import spVIPES
    assert check_silhouette_args("both", "shared") == (0, 1) and check_silhouette_args(1, "private") == (1,) and check_silhouette_args(0, "shared") == (0,)
    gi = [[0, 1], [2, 3]]
    bad = [dict(cells=2), dict(cells="all"), dict(cells=True), dict(cells=None), dict(latent="both"), dict(latent="private"),
           dict(latent="private", cells="both")]
    for kw in bad:
        with pytest.raises(ValueError):
            spVIPES.latent_silhouette(object(), gi, **kw)      # object() has no adata, no module: the refusal comes first
        with pytest.raises(ValueError):
            spVIPES.integration_scores(object(), gi, **kw)
    with pytest.raises(ValueError, match="private"):
        check_silhouette_args("both", "private")
    p = inspect.signature(spVIPES.latent_silhouette).parameters
    assert list(p) == ["self", "group_indices_list", "labels", "cells", "latent", "give_mean", "batch_size", "_noise"]
    assert (p["labels"].default, p["cells"].default, p["latent"].default, p["give_mean"].default, p["batch_size"].default, p["_noise"].default) \
        == ("cell_type", "both", "shared", True, None, None)
    q = inspect.signature(spVIPES.integration_scores).parameters
    assert list(q) == ["self", "group_indices_list", "labels", "kwargs"] and q["labels"].default == "cell_type" and q["kwargs"].kind is inspect.Parameter.VAR_KEYWORD


def test_sums_are_exact_tells_the_two_kinds_of_data_apart():
    rng = np.random.default_rng(0)
    d = (1.0 + rng.random((4, 50))).astype(np.float32)
    assert sums_are_exact(d, [0, 20, 20, 50])
    d[:, 3], d[:, 4] = 1e-12, 1e6                                   # 2^-40 next to 2^20 at 24 bits each: beyond 53 bits
    assert not sums_are_exact(d, [0, 20, 20, 50]) and sums_are_exact(d, [0, 3, 4, 50])   # apart, each segment's sums fit
    assert sums_are_exact(np.zeros((2, 3), dtype=np.float32), [0, 3])


def test_core_runs_on_the_cpu():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "silhouette_host_check.py"), "--small"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().splitlines()[-1] == "all equal" and "DIFFER" not in res.stdout


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
ERR_ARG = -1
P, Q = 0x7F0000001000, 0x7F0000001002   # made-up device addresses: on a 16-byte boundary / 2 bytes off one
FIELDS = ["Q", "ld_q", "n_q", "C", "ld_c", "n_c", "D", "seg_ptr", "n_seg", "n_split", "S", "ld_s", "ws"]


@pytest.fixture(scope="module")
def lib():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    return _abi.load()


def test_header_declares_and_library_exports_the_entry_points(lib):
    from spvipes_amd import _abi, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_silhouette_sums\s*\(\s*const\s+spv_silhouette_args\s*\*\s*\w*\s*,\s*void\s*\*\s*\w*\s*\)", src)
    assert re.search(r"\bint32_t\s+spv_silhouette_splits\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint64_t\s+spv_silhouette_ws_bytes\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", src)
    assert re.search(rf"#define\s+SPV_SILHOUETTE_SEG_MAX\s+{_abi.SIL_SEG_MAX}\b", src) and _abi.SIL_SEG_MAX == 256
    raw = C.CDLL(_abi.LIB_PATH)
    for name in ("spv_silhouette_sums", "spv_silhouette_splits", "spv_silhouette_ws_bytes"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name)
    assert _abi._SIGNATURES["spv_silhouette_ws_bytes"][0] is C.c_int64 and _abi._SIGNATURES["spv_silhouette_splits"][0] is C.c_int32
    assert "spv_silhouette.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "spv_silhouette.h"))


def test_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvSilhouetteArgs
    assert [f for f, _ in M._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_silhouette_args));',
        *[f'  printf(" %zu", offsetof(spv_silhouette_args, {f}));' for f in FIELDS],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in FIELDS]


def test_splits_and_workspace_sizes(lib):
    # ceil(5120 / query tiles), at most n_c / 256 (a chunk is worth four LDS tiles) and 64; 1 for an empty side
    assert lib.spv_silhouette_splits(50000, 50000) == 14 and lib.spv_silhouette_splits(100000, 100000) == 7
    assert lib.spv_silhouette_splits(560, 560) == 2 and lib.spv_silhouette_splits(300, 1100) == 4 and lib.spv_silhouette_splits(1, 10 ** 6) == 64
    assert lib.spv_silhouette_splits(1, 0) == 1 and lib.spv_silhouette_splits(0, 100) == 1 and lib.spv_silhouette_splits(300, 255) == 1
    assert lib.spv_silhouette_splits(5120 * 128, 10 ** 6) == 1 and lib.spv_silhouette_splits(5119 * 128, 10 ** 6) == 2
    assert lib.spv_silhouette_splits(2 ** 31 - 1, 2 ** 31 - 1) == 1
    assert lib.spv_silhouette_ws_bytes(300, 40, 2) == 2 * 40 * 300 * 8
    assert lib.spv_silhouette_ws_bytes(50000, 40, 14) == 224_000_000
    assert lib.spv_silhouette_ws_bytes(2_000_000, 256, 64) == 262_144_000_000        # beyond 2^32: 64-bit arithmetic
    assert lib.spv_silhouette_ws_bytes(2 ** 31 - 1, 256, 64) == (2 ** 31 - 1) * 256 * 64 * 8
    for zero in ((300, 40, 1), (300, 40, 0), (0, 40, 2), (300, 0, 2), (-1, 40, 2), (300, 40, -3)):
        assert lib.spv_silhouette_ws_bytes(*zero) == 0


def _args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Q=P, ld_q=25, n_q=300, C=P, ld_c=25, n_c=260, D=25, seg_ptr=P, n_seg=40, n_split=2, S=P, ld_s=300, ws=P), **o)
    s = _abi.SpvSilhouetteArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


W = "spv_silhouette_sums: "
REJECTIONS = [
    ("null-args", lambda: None, W + "null arguments"),
    ("null-Q", lambda: _args(Q=None), W + "null Q"),
    ("null-C", lambda: _args(C=None), W + "null C"),
    ("null-seg_ptr", lambda: _args(seg_ptr=None), W + "null seg_ptr"),
    ("null-S", lambda: _args(S=None), W + "null S"),
    ("null-ws-2-chunks", lambda: _args(ws=None), W + "null ws"),
    ("null-ws-automatic-chunks", lambda: _args(ws=None, n_split=0, n_q=1, ld_s=1, n_c=10 ** 6), W + "null ws"),   # spv_silhouette_splits(1, 10^6) = 64
    ("misaligned-ws", lambda: _args(ws=Q), W + "ws must be 8-byte aligned"),
    ("D-0", lambda: _args(D=0), W + "D must lie in [1, 64]"),
    ("D-65", lambda: _args(D=65, ld_q=65, ld_c=65), W + "D must lie in [1, 64]"),
    ("n_seg-0", lambda: _args(n_seg=0), W + "n_seg must lie in [1, 256]"),
    ("n_seg-257", lambda: _args(n_seg=257), W + "n_seg must lie in [1, 256]"),
    ("n_split-negative", lambda: _args(n_split=-1), W + "n_split must be 0 or lie in [1, 64]"),
    ("n_split-65", lambda: _args(n_split=65), W + "n_split must be 0 or lie in [1, 64]"),
    ("n_q-0", lambda: _args(n_q=0), W + "n_q < 1"),
    ("n_q-negative", lambda: _args(n_q=-4), W + "n_q < 1"),
    ("n_c-negative", lambda: _args(n_c=-1), W + "n_c < 0"),
    ("ld_q-short", lambda: _args(ld_q=24), W + "ld_q < D"),
    ("ld_c-short", lambda: _args(ld_c=24), W + "ld_c < D"),
    ("ld_s-short", lambda: _args(ld_s=299), W + "ld_s < n_q"),
    # which of two faults is reported
    ("2:null-Q-and-n_seg", lambda: _args(Q=None, n_seg=0), W + "null Q"),
    ("2:D-and-ld_q", lambda: _args(D=0, ld_q=-1), W + "D must lie in [1, 64]"),
    ("2:n_q-and-null-ws", lambda: _args(n_q=0, ws=None), W + "n_q < 1"),
]


@pytest.mark.parametrize("name,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_wrapper_rejects_without_a_device(lib, name, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    rc = lib.spv_silhouette_sums(make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text
