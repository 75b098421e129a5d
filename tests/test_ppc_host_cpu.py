"""CPU: the host side of the posterior-predictive check (spVIPES.posterior_predictive_check) -- the C ABI of spv_dec_sample_stats (header,
cross-compiled library, ctypes mirror, what the wrapper rejects ahead of any HIP call), the argument checks of every layer, and the
two pure host functions ``data.ppc_segments`` / ``data.ppc_table``, the latter against ``fractions.Fraction`` arithmetic.  No GPU calls."""
import ctypes as C
import inspect
import os
import re
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")
ERR_ARG = -1
P, Q = 0x7F0000001000, 0x7F0000001008   # made-up device addresses (never dereferenced by the host code): aligned / 8 bytes off


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_spv_dec_sample_stats():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_dec_sample_stats\s*\(\s*const\s+spv_dec_params\s*\*\s*\w*\s*,\s*const\s+spv_dec_sample_stats_args\s*\*\s*\w*\s*,\s*void\s*\*", src)
    build()
    lib = C.CDLL(_abi.LIB_PATH)
    assert "spv_dec_sample_stats" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "spv_dec_sample_stats")
    res, args = _abi._SIGNATURES["spv_dec_sample_stats"]
    assert res is C.c_int and len(args) == 3
    txt = open(HEADER).read()
    i = txt.index("typedef struct spv_dec_sample_stats_args")
    assert "spVIPESmodule.py:751-759" in txt[txt.rfind("/*", 0, i):i]   # the comment in front of the entry cites the reference lines


def test_sample_stats_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    M = _abi.SpvDecSampleStatsArgs
    fields = [f for f, _ in M._fields_]
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_dec_sample_stats_args));',
        *[f'  printf(" %zu", offsetof(spv_dec_sample_stats_args, {f}));' for f in fields],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(M)] + [getattr(M, f).offset for f in fields]
    body = re.search(r"typedef struct spv_dec_sample_stats_args \{(.*?)\} spv_dec_sample_stats_args;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_fields = sum(d.count(",") + 1 for d in (x.strip() for x in body.split(";")) if d)
    assert n_fields == len(fields)
    shared = ("Am_hi", "Am_lo", "Wm_hi", "Wm_lo", "K", "nsplit", "genes", "n_genes")   # what _fill_readout fills: same names as spv_dec_sample_args
    assert all(f in fields and f in [n for n, _ in _abi.SpvDecSampleArgs._fields_] for f in shared)


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


def _stats_args(**o):
    from spvipes_amd import _abi
    f = dict(dict(Am_hi=P, Am_lo=None, Wm_hi=P, Wm_lo=None, K=64, nsplit=1, genes=None, n_genes=64, n_seg=2, theta=P, cell_ids=None, key=1, sample=0,
                  seg=P, stats=P, ld_stats=64, cell_total=P), **o)
    s = _abi.SpvDecSampleStatsArgs()
    for k, v in f.items():
        setattr(s, k, v)
    return C.pointer(s)


W = "spv_dec_sample_stats: "
REJECTIONS = [
    # what spv_dec_sample refuses, in the same words under this entry point's name
    ("null-params", lambda: (None, _stats_args()), "decoder: null params"),
    ("kslots-2", lambda: (_dec_p(kslots=2), _stats_args()), "decoder: kslots must be 0 (16 / 32 K slots) or 1 (32 / 64)"),
    ("null-args", lambda: (_dec_p(), None), W + "null arguments"),
    ("null-Am_hi", lambda: (_dec_p(), _stats_args(Am_hi=None)), W + "null pointer"),
    ("null-a_p", lambda: (_dec_p(a_p=None), _stats_args()), W + "null pointer"),
    ("K-0", lambda: (_dec_p(), _stats_args(K=0)), W + "K must be a multiple of 32, at most 320"),
    ("K-352", lambda: (_dec_p(), _stats_args(K=352)), W + "K must be a multiple of 32, at most 320"),
    ("nsplit-2", lambda: (_dec_p(), _stats_args(nsplit=2)), W + "nsplit must be 1 or 3"),
    ("nsplit-3-no-lo", lambda: (_dec_p(), _stats_args(nsplit=3, Wm_lo=P)), W + "nsplit=3 needs lo images"),
    ("misaligned-Wm_hi", lambda: (_dec_p(), _stats_args(Wm_hi=Q)), W + "operand images must be 16-byte aligned"),
    ("n_genes-0", lambda: (_dec_p(), _stats_args(n_genes=0)), W + "n_genes must be positive (and at most G without a gene list)"),
    ("n_genes-65-no-list", lambda: (_dec_p(), _stats_args(n_genes=65, ld_stats=65)), W + "n_genes must be positive (and at most G without a gene list)"),
    ("null-theta", lambda: (_dec_p(), _stats_args(theta=None)), W + "null pointer"),
    # its own
    ("null-stats", lambda: (_dec_p(), _stats_args(stats=None)), W + "null pointer"),
    ("n_seg-0", lambda: (_dec_p(), _stats_args(n_seg=0)), W + "n_seg < 1"),
    ("n_seg-negative", lambda: (_dec_p(), _stats_args(n_seg=-3)), W + "n_seg < 1"),
    ("ld_stats-short", lambda: (_dec_p(), _stats_args(ld_stats=63)), W + "ld_stats < n_genes"),
    ("2:misaligned-and-n_seg", lambda: (_dec_p(), _stats_args(Am_hi=Q, n_seg=0)), W + "operand images must be 16-byte aligned"),
]


@pytest.mark.parametrize("name,make,text", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_wrapper_rejects_without_a_device(name, make, text):
    """every case returns from an argument check, ahead of the first HIP call"""
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    build()
    lib = _abi.load()
    rc = lib.spv_dec_sample_stats(*make(), None)
    assert rc == ERR_ARG and (lib.spv_last_error() or b"").decode() == text


# ---- argument checks and signatures --------------------------------------------------------------------------------------------
def test_argument_checks_raise_without_a_device():
    import torch
    from spvipes_amd import _abi, dec_ops
    from spvipes_amd.data import check_ppc_library
    from spvipes_amd.model import spVIPES
    assert check_ppc_library("observed") == "observed" and check_ppc_library("latent") == "latent" and check_ppc_library(1e4) == 1e4
    for bad in (0, -3.0, float("nan"), "raw", None):
        with pytest.raises(ValueError, match="library_size"):
            check_ppc_library(bad)
    # the method checks before it touches the model or a device
    with pytest.raises(ValueError, match="n_samples"):
        spVIPES.posterior_predictive_check(object(), [[0], [0]], 0, n_samples=0)
    with pytest.raises(ValueError, match="seed"):
        spVIPES.posterior_predictive_check(object(), [[0], [0]], 0, seed=-5)
    with pytest.raises(ValueError, match="library_size"):
        spVIPES.posterior_predictive_check(object(), [[0], [0]], 0, library_size="raw")
    with pytest.raises(ValueError, match="group"):
        spVIPES.posterior_predictive_check(object(), [[0], [0]], 2)
    # the op's stream arguments, ahead of any operand preparation
    for kw in (dict(key=-1), dict(key=1 << 64), dict(sample=1 << 32), dict(sample=True)):
        with pytest.raises(ValueError, match="sample_count_stats"):
            dec_ops.sample_count_stats(None, None, None, None, None, False, 1, None, stats=None, **kw)
    # the tables: host tensors, wrong dtypes, wrong shapes
    i64, i32 = torch.zeros((2, 4, 8), dtype=torch.int64), torch.zeros(5, dtype=torch.int32)
    for kw in (dict(seg=i32, n_seg=2, stats=i64, cell_total=None),           # nothing is on a device
               dict(seg=None, n_seg=2, stats=i64, cell_total=None),
               dict(seg=None, n_seg=2, stats=i64.float(), cell_total=None)):
        with pytest.raises(_abi.SpvError, match="sample_count_stats"):
            dec_ops.check_sample_stats_tables(5, 8, **kw)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="n_seg"):
            dec_ops.check_sample_stats_tables(5, 8, None, bad, i64, None)
    assert dec_ops.SAMPLE_STATS == ("sum", "non_zeros", "sum_squares", "max")


def test_entry_points_exist_on_every_layer():
    from spvipes_amd import count_ops, data, dec_ops
    from spvipes_amd.model import spVIPES
    from spvipes_amd.module import spVIPESmodule
    sig = inspect.signature(dec_ops.sample_count_stats)
    assert list(sig.parameters)[:9] == list(inspect.signature(dec_ops.sample_counts).parameters)[:9]
    for k in ("genes", "library_size", "log_library", "key", "sample", "cell_ids", "seg", "n_seg", "stats", "cell_total"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(spVIPESmodule.sample_count_stats)
    assert list(sig.parameters)[1:] == ["inference_outputs", "group", "genes", "library_size", "library", "use_mean", "key", "sample", "cell_ids", "seg",
                                        "n_seg", "stats", "cell_total"]
    sig = inspect.signature(spVIPES.posterior_predictive_check)
    assert list(sig.parameters)[1:] == ["group_indices_list", "group", "n_samples", "groupby", "labels", "gene_list", "library_size", "seed", "batch_size", "_noise"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_samples"], d["groupby"], d["labels"], d["gene_list"], d["library_size"], d["seed"], d["batch_size"], d["_noise"]) == (25, None, None, None, "latent", 0, None, None)
    # the older read-outs keep their signatures
    assert list(inspect.signature(dec_ops.sample_counts).parameters)[9:] == ["genes", "library_size", "key", "sample", "cell_ids", "out"]
    assert list(inspect.signature(dec_ops.expected_expression).parameters)[9:] == ["genes", "what", "library_size", "out", "alpha", "accumulate"]
    assert callable(data.ppc_segments) and callable(data.ppc_table) and callable(count_ops.count_square_sums)


# ---- ppc_segments ----------------------------------------------------------------------------------------------------------------
def test_ppc_segments_codes_cut_and_label_order():
    from spvipes_amd.data import ppc_segments
    lab = np.array(["b", "a", "c", "a", "b", "a", "d"])
    names, sizes, seg = ppc_segments(lab)
    assert names == ["a", "b", "c", "d"] and sizes == [3, 2, 1, 1] and seg.dtype == np.int32
    np.testing.assert_array_equal(seg, [1, 0, 2, 0, 1, 0, 3])
    # ``labels`` gives the order; cells of other labels are left out
    names, sizes, seg = ppc_segments(lab, labels=["c", "a"])
    assert names == ["c", "a"] and sizes == [1, 3]
    np.testing.assert_array_equal(seg, [-1, 1, 0, 1, -1, 1, -1])
    # a walk: positions at or beyond the group's size are the replayed rows a read-out cuts off
    names, sizes, seg = ppc_segments(lab, labels=["c", "a"], positions=np.arange(4, 12))
    assert sizes == [1, 3]   # the sizes count the group's cells, not the walk's
    np.testing.assert_array_equal(seg, [-1, 1, -1, -1, -1, -1, -1, -1])
    np.testing.assert_array_equal(ppc_segments(lab, positions=[6, 7, 0])[2], [3, -1, 1])
    # one population
    names, sizes, seg = ppc_segments(None, n_cells=5, positions=np.arange(3, 8))
    assert names == ["all"] and sizes == [5]
    np.testing.assert_array_equal(seg, [0, 0, -1, -1, -1])
    np.testing.assert_array_equal(ppc_segments(None, n_cells=3)[2], [0, 0, 0])
    # integer labels keep their type in the names
    assert ppc_segments(np.array([3, 1, 3]), labels=[3])[0] == [3]
    with pytest.raises(KeyError, match="'z'"):
        ppc_segments(lab, labels=["a", "z"])
    with pytest.raises(ValueError, match="more than once"):
        ppc_segments(lab, labels=["a", "a"])
    with pytest.raises(ValueError):
        ppc_segments(lab, labels=[])
    with pytest.raises(ValueError):
        ppc_segments(None, labels=["a"], n_cells=3)
    with pytest.raises(ValueError):
        ppc_segments(None)
    with pytest.raises(ValueError):
        ppc_segments(lab, n_cells=6)
    with pytest.raises(ValueError):
        ppc_segments(lab, positions=[-1])


# ---- ppc_table -------------------------------------------------------------------------------------------------------------------
def _fraction_columns(S, NZ, Qs, M, N):
    """the four derived numbers of one (segment, gene) by Fraction arithmetic, rounded to fp64 once"""
    mean = float(Fraction(S, N))
    zf = float(1 - Fraction(NZ, N))
    var = float(Fraction(N * Qs - S * S, N * (N - 1))) if N >= 2 else float("nan")
    cv = (np.sqrt(var) / mean) if mean > 0 else float("nan")
    return mean, var, cv, zf, float(M)


def test_ppc_table_equals_fraction_arithmetic_on_random_integer_tables():
    from spvipes_amd.data import PPC_STATS, ppc_table
    rng = np.random.default_rng(11)
    n_seg, n_sel = 3, 40
    counts = [7, 1000, 123457]
    t = np.zeros((n_seg, 4, n_sel), dtype=np.uint64)
    truth = {}
    for k, N in enumerate(counts):
        for j in range(n_sel):
            # N values of very different sizes: up to 2^5, 2^17 or 2^21 (N * max^2 stays far below 2^64), many zeros in some columns
            hi = (1 << 5, 1 << 17, 1 << 21)[j % 3]
            x = rng.integers(0, hi, size=min(N, 64)).astype(object) * (rng.random(min(N, 64)) < (0.2, 0.9)[j % 2])
            x = [int(v) for v in x] + [0] * (N - min(N, 64))
            if j == 5:
                x = [0] * N   # mean 0
            S, NZ, Qs, M = sum(x), sum(v > 0 for v in x), sum(v * v for v in x), max(x)
            t[k, :, j] = [S, NZ, Qs, M]
            truth[(k, j)] = _fraction_columns(S, NZ, Qs, M, N)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no overflow warning here
        df = ppc_table(t, counts)
        same = ppc_table(t.view(np.int64), counts)   # int64 storage holds the same bits
    assert list(df.columns) == ["segment", "column"] + ["ppc_" + c for c in PPC_STATS] and len(df) == n_seg * n_sel
    assert df.equals(same)
    for (k, j), want in truth.items():
        row = df.iloc[k * n_sel + j]
        assert (row["segment"], row["column"]) == (k, j)
        got = tuple(float(row["ppc_" + c]) for c in PPC_STATS)
        for c, g, w in zip(PPC_STATS, got, want):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (k, j, c, g, w)   # equal as fp64 numbers, not merely close
    assert np.isnan(df.iloc[5]["ppc_cv"]) and df.iloc[5]["ppc_var"] == 0.0 and df.iloc[5]["ppc_zero_fraction"] == 1.0   # mean 0: NaN cv
    assert list(ppc_table(t, counts, prefix="obs_").columns)[2:] == ["obs_" + c for c in PPC_STATS]
    # a large-count case where the float formula E[x^2] - mean^2 would lose everything: N values of 2^31 +- 1
    N = 1 << 20
    big = np.zeros((1, 4, 1), dtype=np.uint64)
    a, b = (1 << 31) - 1, (1 << 31) + 1
    S, Qs = (N // 2) * (a + b), (N // 2) * (a * a + b * b)
    assert N * b * b >= 1 << 64 and Qs >= 1 << 64   # ... it is beyond the overflow rule: NaN with a warning, even with the true square sum's low bits
    big[0, :, 0] = [S, N, Qs % (1 << 64), b]
    with pytest.warns(RuntimeWarning, match="1 "):
        assert np.isnan(ppc_table(big, [N])["ppc_var"][0])


def test_ppc_table_variance_is_nan_for_a_single_value_and_empty_segments_are_nan():
    from spvipes_amd.data import ppc_table
    t = np.zeros((2, 4, 2), dtype=np.uint64)
    t[0, :, 0] = [9, 1, 81, 9]
    df = ppc_table(t, [1, 0])
    assert df["ppc_mean"][0] == 9.0 and np.isnan(df["ppc_var"][0]) and np.isnan(df["ppc_cv"][0]) and df["ppc_zero_fraction"][0] == 0.0
    assert df["ppc_mean"][1] == 0.0 and np.isnan(df["ppc_var"][1]) and np.isnan(df["ppc_cv"][1]) and df["ppc_zero_fraction"][1] == 1.0
    assert df.iloc[2:][["ppc_mean", "ppc_var", "ppc_cv", "ppc_zero_fraction", "ppc_max"]].isna().all().all()   # N = 0
    with pytest.raises(ValueError):
        ppc_table(t, [1])
    with pytest.raises(ValueError):
        ppc_table(t.astype(np.float64), [1, 1])
    with pytest.raises(ValueError):
        ppc_table(t[:, :3], [1, 1])


def test_ppc_table_overflow_rule():
    """N * max^2 >= 2^64: the modular square sum may have wrapped -> NaN var / cv and ONE warning that counts the entries; just below the
    bound the value is finite and equals the Fraction result rounded to fp64."""
    from spvipes_amd.data import ppc_table
    N = 4
    M_bad = 1 << 31            # 4 * 2^62 = 2^64: at the bound
    M_ok = (1 << 31) - 1       # 4 * (2^31 - 1)^2 < 2^64: just below
    t = np.zeros((1, 4, 3), dtype=np.uint64)
    for j, M in enumerate((M_bad, M_ok, M_bad)):
        x = [M, M, M, M] if j != 1 else [M, M, M, 5]
        t[0, :, j] = [sum(x), 4, sum(v * v for v in x) % (1 << 64), M]
    assert int(t[0, 2, 0]) == 0   # the sum of squares of column 0 has wrapped to 0 exactly: a variance from it would be garbage
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        df = ppc_table(t, [N])
    mine = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(mine) == 1 and "2 (segment, gene)" in str(mine[0].message)
    assert np.isnan(df["ppc_var"][0]) and np.isnan(df["ppc_cv"][0]) and np.isnan(df["ppc_var"][2])
    assert df["ppc_mean"][0] == float(M_bad) and df["ppc_max"][0] == float(M_bad) and df["ppc_zero_fraction"][0] == 0.0   # the other columns stand
    x = [M_ok, M_ok, M_ok, 5]
    S, Qs = sum(x), sum(v * v for v in x)
    want = float(Fraction(N * Qs - S * S, N * (N - 1)))
    assert np.isfinite(df["ppc_var"][1]) and df["ppc_var"][1] == want and df["ppc_cv"][1] == np.sqrt(want) / float(Fraction(S, N))
