"""GPU: spv_silhouette_sums through its wrapper (``silhouette_ops.segment_distance_sums``) against tests/_silhouette_reference.py, at the
smallest shapes at which it can go wrong: query counts around the 128-query tile, candidate counts around the 64-candidate LDS tile and
over several chunks, D in all three register forms with their padding, segment boundaries inside a tile, on a tile edge and on a chunk
edge, empty segments first / last / two in a row, segments of one candidate and 256 segments, n_split forced to 1, 2, 3 and automatic.

On data whose sums are exact in fp64 (``sums_are_exact``, ASSERTED on the reference first: then every order of addition gives the same
bits) the table must equal ``segment_sums_ref`` bit for bit for every n_split.  On one data set built to fail that condition the table
must agree within n_c * 2^-53 relative, the worst-case bound for n_c sequential fp64 additions of non-negative terms.  Every test here
needs the feature and fails without it."""
import math

import numpy as np
import pytest
import torch

from tests._silhouette_reference import distances_ref, segment_sums_ref, sums_are_exact

pytestmark = pytest.mark.gpu

SPLITS = (1, 2, 3, 0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _data(seed, n_q, n_c, D, kind="real"):
    rng = np.random.default_rng(seed)
    if kind == "lattice":
        return tuple(rng.integers(-32, 33, (n, D)).astype(np.float32) / 4 for n in (n_q, n_c))
    return tuple(rng.standard_normal((n, D)).astype(np.float32) for n in (n_q, n_c))


def _run(dev, Q, C, seg_ptr, n_split=0, **kw):
    from spvipes_amd.silhouette_ops import segment_distance_sums
    out = segment_distance_sums(torch.as_tensor(Q, device=dev), torch.as_tensor(C, device=dev), torch.as_tensor(seg_ptr, device=dev), n_split=n_split, **kw)
    assert out.dtype == torch.float64 and tuple(out.shape) == (Q.shape[0], len(seg_ptr) - 1) and out.t().is_contiguous()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# (n_q, n_c, D, segment sizes, data).  Chunks: n_split 2 cuts 1100 at 550, n_split 3 at 367 and 734, the automatic 4 at 275 / 550 / 825.
CASES = [
    (1, 0, 3, [0], "real"),
    (1, 1, 1, [1], "real"),
    (127, 63, 16, [63], "real"),
    (128, 64, 17, [64], "real"),
    (129, 65, 25, [64, 1], "real"),                                        # a boundary on the tile edge, then a segment of one
    (300, 260, 35, [0, 5, 1, 1, 0, 0, 100, 28, 125, 0], "real"),           # empty first, two in a row, last; boundaries inside tiles
    (300, 1100, 64, [128, 422, 184, 91, 275], "real"),                     # boundaries at 128 (tile), 550 / 734 / 825 (chunk edges)
    (129, 260, 3, [2] * 4 + [1] * 252, "real"),                            # 256 segments
    (300, 1100, 25, [275] * 4, "lattice"),
    (127, 1100, 1, [1, 0, 0, 1098, 1], "lattice"),
    (128, 63, 64, [3, 60], "lattice"),
]


@pytest.mark.parametrize("case", CASES, ids=[f"q{c[0]}-c{c[1]}-D{c[2]}-s{len(c[3])}-{c[4]}" for c in CASES])
def test_sums_equal_the_reference_bit_for_bit(dev, case):
    n_q, n_c, D, sizes, kind = case
    Q, C = _data(n_q * 1000 + n_c + D, n_q, n_c, D, kind)
    if n_c > 8:
        C[5] = Q[0]   # a query that is a candidate: +0
    seg_ptr = _ptr(sizes)
    assert seg_ptr[-1] == n_c
    d = distances_ref(Q, C)
    assert sums_are_exact(d, seg_ptr)   # the condition of bit equality, on the reference: a data set that fails it fails the test
    want = segment_sums_ref(Q, C, seg_ptr, d=d)
    for n_split in SPLITS:
        got = _run(dev, Q, C, seg_ptr, n_split)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"n_split {n_split}")
    for s, size in enumerate(sizes):
        if size == 0:
            assert (_bits(got[:, s]) == 0).all()   # +0, not -0


def test_inexact_sums_stay_within_the_sequential_bound(dev):
    n_q, n_c, D = 129, 1100, 25
    Q, C = _data(3, n_q, n_c, D)
    Q *= np.float32(1e-13)                                                                  # the queries next to the origin: d(i, j) ~ |c_j|
    C *= (10.0 ** np.random.default_rng(4).uniform(-12, 6, (n_c, 1))).astype(np.float32)   # distances from 1e-12 to 1e6 within every segment
    seg_ptr = _ptr([600, 0, 500])
    d = distances_ref(Q, C)
    assert not sums_are_exact(d, seg_ptr)
    want = segment_sums_ref(Q, C, seg_ptr, d=d)
    exact = np.array([[math.fsum(d[i, seg_ptr[s]:seg_ptr[s + 1]].astype(np.float64)) for s in range(3)] for i in range(n_q)])
    bound = n_c * 2.0 ** -53
    for n_split in SPLITS:
        got = _run(dev, Q, C, seg_ptr, n_split)
        for ref in (want, exact):
            rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
            print(f"n_split {n_split}: largest relative difference {rel.max():.3e} (bound {bound:.3e})")
            assert rel.max() <= bound
        np.testing.assert_array_equal(_bits(got), _bits(_run(dev, Q, C, seg_ptr, n_split)))   # two calls agree bit for bit


def test_strides_out_reuse_subsets_self_and_nan(dev):
    from spvipes_amd.silhouette_ops import segment_distance_sums
    n_q, n_c, D = 300, 260, 25
    Q, C = _data(9, n_q, n_c, D)
    sizes = [64, 0, 100, 96]
    seg_ptr = _ptr(sizes)
    full = _run(dev, Q, C, seg_ptr, 2)
    np.testing.assert_array_equal(_bits(full), _bits(_run(dev, Q, C, seg_ptr, 2)))           # two calls agree bit for bit

    # row strides larger than D, and out= with a row stride larger than n_q: nothing else is written
    Qw, Cw = torch.full((n_q, D + 5), 7.0, device=dev), torch.full((n_c, D + 3), -3.0, device=dev)
    Qw[:, :D], Cw[:, :D] = torch.as_tensor(Q, device=dev), torch.as_tensor(C, device=dev)
    buf = torch.full((len(sizes), n_q + 7), -1.0, dtype=torch.float64, device=dev)
    pd = torch.as_tensor(seg_ptr, device=dev)
    for n_split in (2, 1):   # the second call reuses the buffer
        got = segment_distance_sums(Qw[:, :D], Cw[:, :D], pd, n_split=n_split, out=buf)
        assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (n_q, len(sizes))
        assert (buf[:, n_q:] == -1.0).all()
        if n_split == 2:
            np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(full))
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(_run(dev, Q, C, seg_ptr, 1)))

    # a query's sums do not depend on the other queries of the call
    rows = np.array([299, 0, 128, 127, 5, 200])
    np.testing.assert_array_equal(_bits(_run(dev, Q[rows], C, seg_ptr, 2)), _bits(full[rows]))
    np.testing.assert_array_equal(_bits(_run(dev, Q[7:8], C, seg_ptr, 2)), _bits(full[7:8]))

    # a query that is one of the candidates adds exactly zero for itself: without that candidate the sums are the same bits
    C2 = C.copy()
    C2[70] = Q[3]                                             # candidate 70 lies in segment 2
    assert sums_are_exact(distances_ref(Q[3:4], C2), seg_ptr)  # so the chunk edge that moves by one candidate cannot change a bit either
    for n_split in (1, 2):
        with_self = _run(dev, Q[3:4], C2, seg_ptr, n_split)
        without = _run(dev, Q[3:4], np.delete(C2, 70, axis=0), _ptr([64, 0, 99, 96]), n_split)
        np.testing.assert_array_equal(_bits(with_self), _bits(without))

    # a NaN in one candidate poisons exactly its segment's column
    C3 = C.copy()
    C3[200, 4] = np.nan                                       # segment 3
    got = _run(dev, Q, C3, seg_ptr, 2)
    assert np.isnan(got[:, 3]).all()
    np.testing.assert_array_equal(_bits(got[:, :3]), _bits(full[:, :3]))
    C3[200, 4] = np.inf
    got = _run(dev, Q, C3, seg_ptr, 0)
    assert np.isposinf(got[:, 3]).all() and np.isfinite(got[:, :3]).all()


def test_wrapper_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.silhouette_ops import segment_distance_sums
    Q, C = (torch.zeros((4, 3), device=dev) for _ in range(2))
    p = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    for bad in (lambda: segment_distance_sums(Q.double(), C, p), lambda: segment_distance_sums(Q, C[:, :2], p), lambda: segment_distance_sums(Q.cpu(), C, p),
                lambda: segment_distance_sums(Q, C, p.long()), lambda: segment_distance_sums(Q, C, p.cpu()),
                lambda: segment_distance_sums(Q, C, p, out=torch.zeros((1, 3), dtype=torch.float64, device=dev)),
                lambda: segment_distance_sums(Q, C, p, out=torch.zeros((1, 4), dtype=torch.float32, device=dev))):
        with pytest.raises(_abi.SpvError):
            bad()
    for bad in (lambda: segment_distance_sums(Q[:0], C, p), lambda: segment_distance_sums(Q, C, p, n_split=65), lambda: segment_distance_sums(Q, C, p, n_split=-1),
                lambda: segment_distance_sums(Q, C, p[:1]), lambda: segment_distance_sums(Q, C, torch.zeros(258, dtype=torch.int32, device=dev)),
                lambda: segment_distance_sums(torch.zeros((4, 65), device=dev), torch.zeros((4, 65), device=dev), p)):
        with pytest.raises(ValueError):
            bad()
