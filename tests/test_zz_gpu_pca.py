"""GPU: spv_pca_stage / spv_pca_project / spv_pca_back through the C ABI (ctypes calls on resident matrices), against the fp64
definition of the operand and fp64 products of the DUMPED stage block.

Shapes are the smallest that can still go wrong: G in {97, 200, 230} (off every K tile of 32 and gene tile of 64), an outer-joined
matrix with col_off > 0, uint16 counts with a 65535 and fp32 counts, a cell without counts, a row list with gaps, n = 70 and
2 * spv_pca_slab() + 37 (the merge sees three slabs), every l, a scale with zeros, the list in one piece and in slab-aligned pieces,
dense against CSR storage.  (The file sorts behind every existing GPU test on purpose: docs/lab_notes.md, section AF.)

Bounds.  project: the elementwise classical bound (K + 2) 2^-24 sum |x||v| of a length-K fp32 dot product, K = G, which holds for any
order of summation.  back: the same with K = the slab length, plus n_slabs 2^-53 |Z| for the merge's fp64 additions.  The stage block
against the fp64 definition with np.log1p: ``STAGE_UNITS`` units of 2^-24 max(1, a).  Measured on the inputs of this file: the worst
error is 0.955 units (the kernel's log1p is an fp32 polynomial kernel with a compensated 1 + u; a sweep over 1e-30 .. 1e9 on the CPU
model gives 1.86), so the bound is 4 x that = 3.82 units, below the cap of 16.  The block must also EQUAL the numpy fp32 model of the operand
(tools/pca_host_check.py) bit for bit: the same operations in the same order, nothing contracted."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda"
STAGE_UNITS = 3.82   # 4 x the worst error measured on this file's inputs (0.955 units of 2^-24 max(1, a)); never above 16
LS = (16, 32, 48, 64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _model():
    spec = importlib.util.spec_from_file_location("pca_host_check", os.path.join(ROOT, "tools", "pca_host_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _slab():
    from spvipes_amd import pca_ops
    return pca_ops.pca_slab()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> dict of the host matrix and vectors of one case (made once, shared, never changed)"""
    slab = 1024
    n, G, dtype, col_off, listed, weighted, centred, scaled = {
        "u16-small": (70, 97, "u16", 5, True, True, True, True),
        "f32-plain": (70, 200, "f32", 0, False, False, False, False),
        "u16-slabs": (2 * slab + 37, 230, "u16", 3, True, True, True, True),
        "f32-slabs": (2 * slab + 37, 97, "f32", 0, True, True, True, False),
    }[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    n_rows, ld = n + 20, col_off + G + 4
    own = (rng.poisson(3.0, (n_rows, G)) * (rng.random((n_rows, G)) < 0.25)).astype(np.float64)
    own[1, :] = 0                                                      # a cell with total 0
    if dtype == "u16":
        own[2, G // 2] = 65535
        X = np.full((n_rows, ld), 0xFFFF, np.uint16)                   # the other group's columns / padding: never read as data
        X[:, col_off:col_off + G] = own.astype(np.uint16)
    else:
        own = own * 1.5
        X = np.full((n_rows, ld), np.nan, np.float32)
        X[:, col_off:col_off + G] = own.astype(np.float32)
    if listed:                                                         # a row list with gaps, any order; rows 1 and 2 are in it
        rows = np.concatenate([[1, 2, 0], rng.permutation(np.arange(3, n_rows))[:n - 3]]).astype(np.int32)
    else:
        rows = np.arange(n, dtype=np.int32)
    c = own[rows]
    tot = c.sum(1)
    w = np.where(tot > 0, 1e4 / np.where(tot > 0, tot, 1), 0).astype(np.float32) if weighted else None
    mu = rng.random(G).astype(np.float32) if centred else None
    scale = None
    if scaled:
        scale = (0.5 + rng.random(G)).astype(np.float32)
        scale[rng.random(G) < 0.2] = 0
    V = rng.standard_normal((G, 64)).astype(np.float32)
    return dict(n=n, G=G, col_off=col_off, X=X, rows=rows, listed=listed, c=c, w=w, mu=mu, scale=scale, V=V, n_rows=n_rows)


def _counts(case, storage):
    from spvipes_amd.ops import GroupCounts, SparseGroupCounts
    X = case["X"]
    dense = GroupCounts(_dev(X.view(np.int16) if X.dtype == np.uint16 else X), case["G"], case["col_off"])
    return dense if storage == "dense" else SparseGroupCounts.from_dense(dense)


def _run(case, l, storage="dense", piece_rows=None, rows=None, Z0=None, no_rows=False):
    """stage, project and back over the list, piece by piece, through the C ABI -> (block [n, G], Y [n, l], Z [G, l]) as numpy"""
    from spvipes_amd import _abi, pca_ops
    rows = case["rows"] if rows is None else rows
    n, G = len(rows), case["G"]
    counts = _counts(case, storage)
    d_rows, w, mu, scale, V = _dev(rows), _dev(case["w"] if len(rows) == case["n"] else None), _dev(case["mu"]), _dev(case["scale"]), _dev(case["V"][:, :l])
    block = torch.full((n, G + 3), -777.0, dtype=torch.float32, device=DEV)
    Y = torch.full((n, l + 2), -777.0, dtype=torch.float32, device=DEV)
    Z = torch.zeros((G, l + 1), dtype=torch.float64, device=DEV)
    if Z0 is not None:
        Z[:, :l] = _dev(Z0)
    Z[:, l] = -777.0
    a = _abi.SpvPcaArgs()
    a.G, a.n, a.l, a.w, a.mu, a.scale = G, n, l, _abi.ptr(w), _abi.ptr(mu), _abi.ptr(scale)
    a.ld_block, a.V, a.ld_v, a.Y, a.ld_y, a.Z, a.ld_z = G + 3, _abi.ptr(V), l, _abi.ptr(Y), l + 2, _abi.ptr(Z), l + 1
    if no_rows:   # rows == NULL: cell p of the matrix is list position p
        assert storage == "dense" and piece_rows is None
        todo = [(counts.c_struct(None), counts.n_cells, 0, n)]
    else:
        todo = pca_ops.pieces(counts, d_rows, piece_rows or (1 << 20))
    for cs, n_rows, p0, m in todo:
        ws = torch.empty(pca_ops.pca_ws_bytes(G, m, l), dtype=torch.uint8, device=DEV)
        a.x, a.n_rows, a.pos_off, a.n_piece = cs, n_rows, p0, m
        a.block, a.ws, a.ws_bytes = block.data_ptr() + 4 * p0 * (G + 3), _abi.ptr(ws), ws.numel()
        for entry in ("spv_pca_stage", "spv_pca_project", "spv_pca_back"):
            _abi.call(entry, C.byref(a), _abi.stream_ptr())
    torch.cuda.synchronize()
    b, y, z = block.cpu().numpy(), Y.cpu().numpy(), Z.cpu().numpy()
    assert (b[:, G:] == -777.0).all() and (y[:, l:] == -777.0).all() and (z[:, l] == -777.0).all()   # nothing beyond the stated columns
    return np.ascontiguousarray(b[:, :G]), np.ascontiguousarray(y[:, :l]), np.ascontiguousarray(z[:, :l])


@functools.lru_cache(maxsize=None)
def _result(name, l, storage="dense", piece_rows=None):
    return _run(_case(name), l, storage, piece_rows)


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_the_library_reports_its_sizes():
    from spvipes_amd import pca_ops
    from spvipes_amd.count_ops import COUNT_CHUNK_ROWS
    assert COUNT_CHUNK_ROWS % pca_ops.pca_slab() == 0 and pca_ops.pca_slab() == 1024 and pca_ops.pca_cell_tile() == 64
    assert pca_ops.pca_ws_bytes(97, 2 * 1024 + 37, 48) == 4 * 3 * 128 * 48


@pytest.mark.parametrize("name,l", [("u16-small", 16), ("f32-plain", 48), ("u16-slabs", 64), ("f32-slabs", 32)])
def test_stage_block_against_the_fp64_definition_and_the_fp32_model(name, l):
    case = _case(name)
    block, _Y, _Z = _result(name, l)
    c, w, mu, scale = case["c"], case["w"], case["mu"], case["scale"]
    c32 = c.astype(np.float32)
    u = c32 if w is None else (c32 * w[:, None]).astype(np.float32)
    a64 = np.log1p(u.astype(np.float64))
    mu64 = np.zeros(case["G"]) if mu is None else mu.astype(np.float64)
    sc64 = np.ones(case["G"]) if scale is None else scale.astype(np.float64)
    # the log itself, where the scale lets it through: a = x / scale + mu up to two fp32 roundings -- measured on the model of a instead
    model = _model()
    a32 = model.log1p_model(u).astype(np.float64)
    units = float(np.max(np.abs(a32 - a64) / (2.0 ** -24 * np.maximum(1.0, a64))))
    print(f"{name}: log1p worst {units:.3f} units of 2^-24 max(1, a)")
    assert units <= STAGE_UNITS <= 16.0
    # the block: the fp32 model bit for bit, hence within the log's bound plus the subtract's and the multiply's roundings of the definition
    want = model.operand_model(c32, w, mu, scale)
    assert (_bits(block) == _bits(want)).all(), f"{name}: {(_bits(block) != _bits(want)).sum()} of {want.size} elements differ from the fp32 model"
    x64 = (a64 - mu64) * sc64
    bound = (STAGE_UNITS * 2.0 ** -24 * np.maximum(1.0, a64) + 2.0 ** -24 * np.abs(a64 - mu64)) * np.abs(sc64) + 2.0 ** -24 * np.abs(x64)
    assert (np.abs(block - x64) <= bound * (1.0 + 2.0 ** -20)).all()   # (the factor covers the second-order terms)
    # zero counts give exactly -mu * scale; a gene with scale 0 gives exactly 0
    zero = u == 0
    expect0 = np.broadcast_to(((np.float32(0) - mu64.astype(np.float32)) * sc64.astype(np.float32)).astype(np.float32), block.shape)
    assert zero.any() and (_bits(block[zero]) == _bits(np.ascontiguousarray(expect0[zero]))).all()
    if scale is not None:
        assert (scale == 0).any() and (block[:, scale == 0] == 0).all()
    assert np.isfinite(block).all()


def _check_products(case, block, Y, Z, l, Z0=None):
    G, n = case["G"], block.shape[0]
    b64, v64 = block.astype(np.float64), case["V"][:, :l].astype(np.float64)
    Yref = b64 @ v64
    Ybound = (G + 2) * 2.0 ** -24 * (np.abs(b64) @ np.abs(v64))
    assert (np.abs(Y - Yref) <= Ybound).all(), f"project: worst {np.max(np.abs(Y - Yref) / np.maximum(Ybound, 1e-300)):.3f} of the bound"
    y64 = Y.astype(np.float64)
    start = np.zeros((G, l)) if Z0 is None else Z0
    Zref = start + b64.T @ y64
    n_slabs = -(-n // _slab())
    Zbound = (_slab() + 2) * 2.0 ** -24 * (np.abs(b64).T @ np.abs(y64)) + n_slabs * 2.0 ** -53 * np.abs(Zref)
    assert (np.abs(Z - Zref) <= Zbound).all(), f"back: worst {np.max(np.abs(Z - Zref) / np.maximum(Zbound, 1e-300)):.3f} of the bound"
    if case["scale"] is not None:   # a gene with scale 0 contributes exactly 0
        assert (Z[case["scale"] == 0] == start[case["scale"] == 0]).all()


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("name", ["u16-small", "f32-plain"])
def test_project_and_back_against_fp64_products_of_the_dumped_block_every_l(name, l):
    block, Y, Z = _result(name, l)
    _check_products(_case(name), block, Y, Z, l)


@pytest.mark.parametrize("name,l", [("u16-slabs", 64), ("f32-slabs", 32), ("u16-slabs", 48)])
def test_three_slabs_against_fp64_products_and_an_accumulating_start(name, l):
    case = _case(name)
    block, Y, Z = _result(name, l)
    _check_products(case, block, Y, Z, l)
    Z0 = np.random.default_rng(5).standard_normal((case["G"], l)) * 100.0
    block2, Y2, Z2 = _run(case, l, Z0=Z0)                       # back ADDS onto what Z holds
    assert (_bits(block2) == _bits(block)).all() and (_bits(Y2) == _bits(Y)).all()
    _check_products(case, block2, Y2, Z2, l, Z0=Z0)


@pytest.mark.parametrize("name,l", [("u16-slabs", 64), ("f32-slabs", 32), ("u16-small", 16)])
def test_repeats_pieces_and_storage_agree_bit_for_bit(name, l):
    one = _result(name, l)
    again = _run(_case(name), l)
    sparse = _result(name, l, "sparse")
    runs = [("a second call", again), ("CSR storage", sparse)]
    if _case(name)["n"] > _slab():
        runs += [(f"pieces of {k} slabs", _result(name, l, "dense", k * _slab())) for k in (1, 2)]
    for what, got in runs:
        for x, y, part in zip(one, got, ("block", "Y", "Z")):
            assert (_bits(x) == _bits(y)).all(), f"{what}: {part} differs in {(_bits(x) != _bits(y)).sum()} of {x.size} elements"


def test_a_row_of_project_does_not_depend_on_the_other_rows():
    case = _case("u16-slabs")
    # the weights travel with the list: a case without them for the sub-lists
    plain = dict(case, w=None)
    _b, Y, _Z = _run(plain, 64)
    for p in (0, 1, 63, 64, 1023, 1024, case["n"] - 1):
        _b1, y1, _z1 = _run(plain, 64, rows=case["rows"][p:p + 1])
        assert (_bits(y1[0]) == _bits(Y[p])).all(), f"row {p} alone differs from row {p} among the others"
    sub = np.ascontiguousarray(case["rows"][100:171][::-1])
    _b2, y2, _z2 = _run(plain, 64, rows=sub)
    assert (_bits(y2) == _bits(np.ascontiguousarray(Y[100:171][::-1]))).all()


def test_no_row_list_and_null_vectors():
    """rows == NULL: cell p is list position p; w, mu and scale NULL read as 1, 0 and 1"""
    case = _case("f32-plain")
    assert not case["listed"] and case["w"] is None and case["mu"] is None and case["scale"] is None
    listed = _result("f32-plain", 48)
    direct = _run(case, 48, no_rows=True)
    for x, y in zip(listed, direct):
        assert (_bits(x) == _bits(y)).all()
    block = direct[0]
    assert (block[case["c"] == 0] == 0).all() and (block >= 0).all()
