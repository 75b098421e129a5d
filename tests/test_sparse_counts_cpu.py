"""CPU: CSR-resident counts -- the host conversion of one group's slice of a sparse AnnData.X (data.csr_group_arrays) and the
C-ABI struct of spv_csr_gather.  No GPU."""
import ctypes
import os
import subprocess
import tracemalloc

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(indptr, cols, vals, G):
    from spvipes_amd.data import csr_to_dense
    return csr_to_dense(indptr, cols, vals, G)


def _messy(seed=0, n=60, n_var=50, fractional=False, big=False):
    """COO data with duplicate entries, unordered columns, explicit zeros and empty rows"""
    rng = np.random.default_rng(seed)
    nnz = 400
    r = rng.integers(0, n, nnz)
    r[(r % 7) == 3] = 0          # rows 3, 10, 17, ... stay empty
    c = rng.integers(0, n_var, nnz)
    v = rng.integers(0, 20, nnz).astype(np.float64)
    v[::17] = 0.0                 # explicit zeros
    if fractional:
        v = v + 0.25
    if big:   # (cell 4, gene 49 is inside the group the test selects)
        r, c, v = np.append(r, 4), np.append(c, 49), np.append(v, 70000.0)
        nnz += 1
    perm = rng.permutation(nnz)
    return sp.coo_matrix((v[perm], (r[perm], c[perm])), shape=(n, n_var))


@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
@pytest.mark.parametrize("kind", ["int", "fractional", "big"])
def test_csr_group_arrays_densify_to_the_slice(fmt, kind):
    from spvipes_amd import _abi
    from spvipes_amd.data import csr_group_arrays

    coo = _messy(fractional=kind == "fractional", big=kind == "big")
    want_full = coo.toarray()   # (sums the duplicates)
    if fmt == "csr":   # a CSR with duplicates and unsorted columns, built by hand (scipy would canonicalise it on conversion)
        order = np.argsort(coo.row, kind="stable")
        counts = np.bincount(coo.row, minlength=coo.shape[0])
        X = sp.csr_matrix((coo.data[order], coo.col[order], np.concatenate([[0], np.cumsum(counts)])), shape=coo.shape)
        assert not X.has_canonical_format
    else:
        X = coo.asformat(fmt)
    obs_idx = np.array([4, 0, 3, 10, 11, 59, 30, 3])            # unordered, repeated, empty rows
    var_idx = np.array([49, 2, 3, 4, 17, 18, 40, 41, 42, 0])     # non-contiguous, out of order
    indptr, cols, vals, dtype = csr_group_arrays(X, obs_idx, var_idx)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and len(indptr) == len(obs_idx) + 1
    for i in range(len(obs_idx)):
        c = cols[indptr[i]:indptr[i + 1]]
        assert np.all(np.diff(c) > 0), "columns sorted and unique within a row"
    want = want_full[obs_idx][:, var_idx]
    if kind == "int":
        assert dtype == _abi.SPV_COUNT_U16 and vals.dtype == np.uint16
    else:
        assert dtype == _abi.SPV_COUNT_F32 and vals.dtype == np.float32
    np.testing.assert_array_equal(_dense(indptr, cols, vals, len(var_idx)), want.astype(vals.dtype))
    if fmt == "csr":
        assert not X.has_canonical_format   # the user's matrix is only read


def test_dtype_rule_follows_to_group_counts():
    from spvipes_amd import _abi
    from spvipes_amd.data import csr_group_arrays

    for vals, want in (([1.0, 65535.0], _abi.SPV_COUNT_U16), ([1.0, 65536.0], _abi.SPV_COUNT_F32), ([1.0, 2.5], _abi.SPV_COUNT_F32),
                       ([0.0, 0.0], _abi.SPV_COUNT_U16)):
        X = sp.csr_matrix((np.array(vals), ([0, 1], [0, 1])), shape=(2, 2))
        ip, c, v, dt = csr_group_arrays(X, [0, 1], [0, 1])
        assert dt == want
        np.testing.assert_array_equal(_dense(ip, c, v, 2), X.toarray().astype(v.dtype))
    # no stored entry at all: an all-zero block is uint16 on the dense path too
    assert csr_group_arrays(sp.csr_matrix((3, 4)), [0, 2], [1, 3])[3] == _abi.SPV_COUNT_U16


def test_negative_values_raise_the_dense_paths_error():
    from spvipes_amd.data import csr_group_arrays, to_group_counts

    X = sp.csr_matrix(np.array([[0.0, -1.0], [2.0, 0.0]]))
    with pytest.raises(ValueError) as dense_err:
        to_group_counts(X.toarray(), "cpu")
    with pytest.raises(ValueError) as sparse_err:
        csr_group_arrays(X, [0, 1], [0, 1])
    assert str(sparse_err.value) == str(dense_err.value)
    # a negative value outside the group's columns is not the group's business
    ip, c, v, _ = csr_group_arrays(X, [0, 1], [0])
    np.testing.assert_array_equal(_dense(ip, c, v, 1), [[0], [2]])


def test_dense_input_and_sparse_input_give_the_same_arrays():
    from spvipes_amd.data import csr_group_arrays

    X = _messy(seed=3)
    obs, var = np.arange(5, 40), np.array([1, 7, 8, 9, 30, 31])
    a = csr_group_arrays(X, obs, var)
    b = csr_group_arrays(X.toarray(), obs, var)
    np.testing.assert_array_equal(_dense(*a[:3], len(var)), _dense(*b[:3], len(var)))
    assert a[3] == b[3]


def test_conversion_never_densifies():
    """200 000 cells x 30 000 genes (24 GB as dense float32) with ~2 M stored entries"""
    from spvipes_amd.data import csr_group_arrays

    rng = np.random.default_rng(0)
    n, G, per_row = 200_000, 30_000, 10
    indptr = np.arange(0, n * per_row + 1, per_row, dtype=np.int64)
    cols = np.sort(rng.integers(0, G // per_row, (n, per_row)) + np.arange(per_row) * (G // per_row), axis=1).astype(np.int32).ravel()
    X = sp.csr_matrix((rng.integers(1, 50, n * per_row).astype(np.float32), cols, indptr), shape=(n, G))
    obs = np.arange(0, n, 2)
    var = np.arange(0, G, 3)
    tracemalloc.start()
    ip, c, v, _ = csr_group_arrays(X, obs, var)
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    assert peak < 200 * 2**20, f"peak {peak / 2**20:.0f} MB"
    assert len(ip) == len(obs) + 1 and ip[-1] == len(c) == len(v)
    # spot-check rows against scipy's own slicing
    for i in (0, 1, 77_777, len(obs) - 1):
        np.testing.assert_array_equal(_dense(ip[i:i + 2] - ip[i], c[ip[i]:ip[i + 1]], v[ip[i]:ip[i + 1]], len(var))[0],
                                      X[obs[i]].toarray()[0, var])


def test_gather_struct_matches_the_header(tmp_path):
    from spvipes_amd import _abi

    src = tmp_path / "sizes.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "spvipes_hip.h")}"', "int main(void) {",
        '  printf("%zu %zu %zu %zu %d\\n", sizeof(spv_csr_gather_args), offsetof(spv_csr_gather_args, rows),'
        ' offsetof(spv_csr_gather_args, xb_split), offsetof(spv_csr_gather_args, library), SPV_CSR_GATHER_MAXG);',
        "  return 0;", "}"]))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, o_rows, o_split, o_lib, maxg = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    S = _abi.SpvCsrGatherArgs
    assert size == ctypes.sizeof(S)
    assert (o_rows, o_split, o_lib) == (S.rows.offset, S.xb_split.offset, S.library.offset)
    assert maxg == _abi.SPV_CSR_GATHER_MAXG
    assert "spv_csr_gather" in _abi.EXPORTED_SYMBOLS


def test_model_keyword_defaults_to_auto():
    """counts_storage is a model-level keyword; a saved model without it (older files) is rebuilt with the default, "auto" """
    import inspect

    from spvipes_amd.model import spVIPES

    sig = inspect.signature(spVIPES.__init__)
    assert sig.parameters["counts_storage"].default == "auto"
