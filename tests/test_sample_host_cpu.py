"""CPU: the host side of the count sampler (spVIPES.posterior_predictive_sample) -- the statistical yardstick the GPU tests use
(tests/_nb_sampling_check.py), the C ABI of spv_dec_sample / spv_nbmix_sample (header, cross-compiled library, ctypes mirror) and the
argument checks.  No GPU calls."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _nb_sampling_check as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spvipes_hip.h")


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------
def test_checker_accepts_numpy_draws_on_the_grid_and_rejects_wrong_samplers():
    """The one test of this pull request's files that passes without the feature: it checks the checker.  numpy's own Bernoulli /
    gamma / poisson draws pass all 144 grid points (every ratio <= 1: room for a correct sampler), and draws made with theta * 1.25 or
    with both rates * 1.03 are rejected at (theta, m1, m2, pi) = (3, 12, 80, 0) and (30, 300, 3000, 0) (power against a wrong one)."""
    assert len(S.GRID) == 144
    rng = np.random.default_rng(0)
    worst = np.zeros(3)
    tables = {}
    for (th, m1, m2, pi) in S.GRID:
        p = tables[(th, m1, m2, pi)] = S.pmf_table(m1, m2, th, pi)
        assert 1.0 - p.sum() < S.TAIL and p.size >= S.table_extent(m1, m2, th) + 1
        r = S.check(S.numpy_draws(rng, m1, m2, th, pi), p)
        worst = np.maximum(worst, r)
        assert max(r) <= 1.0, ((th, m1, m2, pi), r)
    print("worst ratios of numpy's draws (distribution, mean, variance):", worst)
    for (th, m1, m2, pi) in ((3.0, 12.0, 80.0, 0.0), (30.0, 300.0, 3000.0, 0.0)):
        p = tables[(th, m1, m2, pi)]
        assert max(S.check(S.numpy_draws(rng, m1, m2, th * 1.25, pi), p)) > 1.0
        assert max(S.check(S.numpy_draws(rng, m1 * 1.03, m2 * 1.03, th, pi), p)) > 1.0
    m, v, _ = S.moments(S.pmf_table(12.0, 80.0, 3.0, 0.1))   # the table's moments are the mixture's closed-form moments
    mean, second = 0.1 * 12.0 + 0.9 * 80.0, 0.1 * (12.0 + 144.0 / 3.0 + 144.0) + 0.9 * (80.0 + 6400.0 / 3.0 + 6400.0)
    assert abs(m - mean) < 1e-8 * mean and abs(v - (second - mean * mean)) < 1e-8 * v
    assert S.check(np.array([0, p.size]), p) == (np.inf, np.inf, np.inf)   # a draw outside the table
    assert S.check(np.array([-1, 0]), p) == (np.inf, np.inf, np.inf)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_sampling_entry_points():
    from spvipes_amd import _abi
    from spvipes_amd.build import build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+spv_dec_sample\s*\(\s*const\s+spv_dec_params\s*\*\s*\w*\s*,\s*const\s+spv_dec_sample_args\s*\*", src)
    m = re.search(r"\bint\s+spv_nbmix_sample\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m is not None
    n_header_args = m.group(1).count(",") + 1
    build()
    lib = ctypes.CDLL(_abi.LIB_PATH)
    for name in ("spv_dec_sample", "spv_nbmix_sample"):
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    res, args = _abi._SIGNATURES["spv_dec_sample"]
    assert res is ctypes.c_int and len(args) == 3
    res, args = _abi._SIGNATURES["spv_nbmix_sample"]
    assert res is ctypes.c_int and len(args) == n_header_args == 13
    txt = open(HEADER).read()
    for decl in ("typedef struct spv_dec_sample_args", "int spv_nbmix_sample("):   # the comment in front of each entry cites the reference lines
        i = txt.index(decl)
        assert "spVIPESmodule.py:751-759" in txt[txt.rfind("/*", 0, i):i], decl


def test_sample_args_struct_matches_its_ctypes_mirror(tmp_path):
    from spvipes_amd import _abi
    fields = ("genes", "ld_gene", "theta", "cell_ids", "key", "sample", "out", "ld_out")
    src = tmp_path / "size.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {",
        '  printf("%zu", sizeof(spv_dec_sample_args));',
        *[f'  printf(" %zu", offsetof(spv_dec_sample_args, {f}));' for f in fields],
        "  return 0;", "}"]))
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    M = _abi.SpvDecSampleArgs
    assert got == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    body = re.search(r"typedef struct spv_dec_sample_args \{(.*?)\} spv_dec_sample_args;", open(HEADER).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_fields = sum(d.count(",") + 1 for d in (x.strip() for x in body.split(";")) if d)
    assert n_fields == len(M._fields_)


# ---- argument checks and signatures --------------------------------------------------------------------------------------------
def test_sample_argument_checks_raise_without_a_device():
    import math
    from spvipes_amd.data import check_sample_args
    from spvipes_amd.model import spVIPES
    assert check_sample_args(1, 0, "latent") == (1, 0, None)
    assert check_sample_args(np.int64(3), 2 ** 32 - 1, 1e4) == (3, 2 ** 32 - 1, math.log(1e4))
    for bad in (0, -1, 1.5, True, None, "2"):
        with pytest.raises(ValueError, match="n_samples"):
            check_sample_args(bad, 0, "latent")
    for bad in (-1, 2 ** 32, 0.5, True, None):
        with pytest.raises(ValueError, match="seed"):
            check_sample_args(1, bad, "latent")
    for bad in (0, -3.0, float("nan"), float("inf"), "observed", None):
        with pytest.raises(ValueError, match="library_size"):
            check_sample_args(1, 0, bad)
    # the method itself checks before it touches the model or a device
    with pytest.raises(ValueError, match="n_samples"):
        spVIPES.posterior_predictive_sample(object(), [[0], [0]], n_samples=0)
    with pytest.raises(ValueError, match="seed"):
        spVIPES.posterior_predictive_sample(object(), [[0], [0]], seed=-5)
    with pytest.raises(ValueError, match="library_size"):
        spVIPES.posterior_predictive_sample(object(), [[0], [0]], library_size="observed")


def test_sample_key_is_a_64_bit_key_that_carries_the_seed():
    from spvipes_amd.dec_ops import sample_key
    keys = {sample_key(s) for s in (0, 1, 2 ** 32 - 1)}
    assert len(keys) == 3 and all(0 <= k < 2 ** 64 for k in keys)
    assert [sample_key(s) & 0xFFFFFFFF for s in (0, 7, 2 ** 32 - 1)] == [0, 7, 2 ** 32 - 1]


def test_sampling_entry_points_exist_on_every_layer():
    from spvipes_amd import dec_ops
    from spvipes_amd.model import spVIPES
    from spvipes_amd.module import spVIPESmodule
    sig = inspect.signature(dec_ops.sample_counts)
    for k in ("genes", "library_size", "key", "sample", "cell_ids", "out"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(spVIPESmodule.sample_counts)
    assert list(sig.parameters)[1:] == ["inference_outputs", "group", "genes", "library_size", "use_mean", "key", "sample", "cell_ids", "out"]
    assert sig.parameters["use_mean"].default is False and sig.parameters["use_mean"].kind is inspect.Parameter.KEYWORD_ONLY   # as expected_expression
    for k in ("genes", "library_size", "key", "sample", "cell_ids", "out"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(spVIPES.posterior_predictive_sample)
    assert list(sig.parameters)[1:] == ["group_indices_list", "n_samples", "gene_list", "library_size", "seed", "batch_size", "return_numpy", "_noise"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_samples"], d["gene_list"], d["library_size"], d["seed"], d["batch_size"], d["return_numpy"], d["_noise"]) == (1, None, "latent", 0, None, True, None)
