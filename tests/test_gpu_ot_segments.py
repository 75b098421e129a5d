"""GPU: spv_ot_segment_lse (spvipes_amd.ot_ops.ot_segment_lse; csrc/spv_ot_segments.h) against the yardstick of
tests/_ot_segment_reference.py, in the harness style of tests/test_gpu_ot.py: odd or 16-byte-multiple row pitches with NaN in the pitch
padding (a kernel that read it would lose the candidate), sentinels around the segment-major output, real and lattice data.  Shapes
are sized by the tiles (TQ queries per workgroup, TC candidates per LDS tile): one below, at and one above a tile, several tiles, more
than one workgroup, about 2000 candidates so that the automatic chunk count exceeds 1.  Segment layouts put boundaries at TC - 1 / TC /
TC + 1, at a chunk's edge, one segment across three chunks, runs of size-1 segments inside a tile, and empty segments first, last and
several in a row.  Every test here calls the new op and fails without it.

THE BOUND.  tests/test_gpu_ot.py derives, for ot_softmin's L over n_c candidates in n_split chunks of n_chain candidates,
    |L - L_ref| <= (3 n_chain + 4 n_split + 5 ln(n_c + 1) + 16) u + 2 u max(|L_ref|, 1),   u = 2^-24.
It holds for L[s][i] as it stands, term by term:
  * t is the same bits as ot_softmin's and the reference's, so again only the reduction errs, and the reduction of one segment is
    ot_softmin's on the candidates of that segment: the same ot_update per candidate, the same ot_merge per chunk, the same ot_lse_value.
  * 3 n_chain u: the running pair is re-initialised at a boundary, so inside one chunk a segment's chain of steps is the part of the
    chunk the segment covers -- no longer than the chunk.
  * 4 n_split u: a segment's value is merged from all n_split chunk states.  A chunk that does not reach the segment contributes the
    empty state (-inf, 0), and ot_merge of an empty state changes nothing, exactly; the chunks that do reach it cost 3 u each as before.
  * 5 ln(n_c + 1) u (the telescoped |d| parts, 2.5 u ln n, and logf's 2 u ln n) has the number of terms n of the SEGMENT in it, which
    n_c overstates.
  * the 16 u slack and 2 u max(|L_ref|, 1) are untouched: L_ref is the segment's own float64 value.
Nothing was fitted to the kernel's output.  For the sum over segments: log sum_s exp(L[s][i]) in float64 against ot_softmin's L[i]
differs by at most the two bounds added, since log-sum-exp is 1-Lipschitz in the sup norm (every L[s][i] within its bound of the
segment's true value moves the total by at most the largest of them) and ot_softmin's L is within its own bound of the same total."""
import numpy as np
import pytest
import torch

from tests._ot_reference import lse_ref, t_ref
from tests._ot_segment_reference import segment_lse_ref
from tests.test_gpu_ot import L_SENTINEL, SPLIT_MAX, TC, TQ, U, _data, _operands, _softmin
from tests.test_gpu_ot import lse_bound as softmin_bound

pytestmark = pytest.mark.gpu

SEG_MAX = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _resolved(n_q, n_c, n_split):
    from spvipes_amd.ot_ops import ot_segment_splits
    return n_split or ot_segment_splits(n_q, n_c)


def lse_bound(L_want, n_q, n_c, n_split):
    """the module docstring's bound: tests/test_gpu_ot.py's formula with this kernel's own automatic chunk count for n_split = 0"""
    ns = _resolved(n_q, n_c, n_split)
    n_chain = -(-n_c // ns)
    return (3 * n_chain + 4 * ns + 5 * np.log(n_c + 1.0) + 16) * U + 2 * U * np.maximum(np.abs(L_want), 1.0)


def _seg_lse(dev, X, Y, h, seg_ptr, s, n_split=0, pitch="odd"):
    """one call with sentinels all around the segment-major output -> float32 [n_q, n_seg] on the host"""
    from spvipes_amd.ot_ops import ot_segment_lse
    n_q, n_seg = X.shape[0], len(seg_ptr) - 1
    buf = torch.full((n_seg + 2, n_q + 3), L_SENTINEL, dtype=torch.float32, device=dev)
    L = ot_segment_lse(*_operands(dev, X, Y, pitch), torch.from_numpy(h).to(dev), torch.from_numpy(np.asarray(seg_ptr, dtype=np.int32)).to(dev), s,
                       n_split=n_split, out=buf[1:n_seg + 1])
    assert L.shape == (n_q, n_seg)
    got = buf.cpu().numpy()
    assert (got[0] == L_SENTINEL).all() and (got[n_seg + 1] == L_SENTINEL).all() and (got[:, n_q:] == L_SENTINEL).all(), "L written outside [n_seg, n_q]"
    np.testing.assert_array_equal(L.cpu().numpy().view(np.uint32), got[1:n_seg + 1, :n_q].T.view(np.uint32))
    return np.ascontiguousarray(got[1:n_seg + 1, :n_q].T)


def _seg_ptr(layout, rng, n_c, n_seg, per):
    """n_seg + 1 ascending entries from 0 to n_c: the layout's own cuts first, random cuts for the rest"""
    must = {"one": [], "even": [],
            "tile": [TC - 1, TC, TC + 1],                                   # boundaries around the LDS tile's edge
            "chunk": [per - 1, per, per + 1, 2 * per],                      # ... and at a chunk's edge
            "span": [per - 70, 2 * per + 70],                               # one segment over three chunks
            "ones": list(range(TC + 2, TC + 2 + min(n_seg - 1, 40))),       # runs of size-1 segments inside one tile
            "empty": [0, 0, n_c // 2, n_c // 2, n_c // 2, n_c, n_c]}[layout]   # empty segments first, several in a row, last
    must = [min(max(c, 0), n_c) for c in must][:n_seg - 1]
    top = must[0] if layout == "span" else n_c   # "span": the other cuts stay ahead of the long segment
    cuts = np.sort(np.concatenate([must, rng.integers(0, top + 1, n_seg - 1 - len(must))])).astype(np.int64)
    return np.concatenate([[0], cuts, [n_c]]).astype(np.int32)


def _hold(L, want, n_q, n_c, n_split, what=""):
    fin = np.isfinite(want)
    assert np.isneginf(L[~fin]).all(), "a segment without a contributing candidate must be -inf"
    if fin.any():
        err, bound = np.abs(L[fin].astype(np.float64) - want[fin]), lse_bound(want[fin], n_q, n_c, n_split)
        print(f"segment lse {what} n_q {n_q} n_c {n_c} n_split {n_split}: max |L - L_ref| = {err.max():.3e}, bound {bound.min():.3e}")
        assert (err <= bound).all()


def test_shape_functions_and_the_bound(dev):
    from spvipes_amd.ot_ops import OT_SEG_MAX, ot_segment_splits, ot_segment_ws_bytes, ot_splits, ot_tiles
    assert ot_tiles() == (TQ, TC) and OT_SEG_MAX == SEG_MAX
    assert ot_segment_splits(2 * TQ + 3, 2000) == 7 and ot_segment_splits(TQ + 1, 2 * TC + 5) == 1 and ot_segment_splits(1, 0) == 1   # what the cases rely on
    assert ot_segment_splits(50000, 50000) > ot_splits(50000, 50000)   # several rounds of resident workgroups
    assert ot_segment_ws_bytes(300, 7, 1) == 0 and ot_segment_ws_bytes(300, 7, 3) == 3 * 7 * 300 * 8
    want = np.array([-3.0, 40.0])
    for n_split in (1, 3, 64):   # with explicit chunks the bound IS tests/test_gpu_ot.py's
        np.testing.assert_array_equal(lse_bound(want, 259, 2000, n_split), softmin_bound(want, 259, 2000, n_split))


# (n_q, n_c, D, n_split, n_seg, layout, pitch): every n_q of {1, TQ-1, TQ, TQ+1, 2TQ+3}, n_c of {0, 1, TC-1, TC, TC+1, 2TC+5, 2000}, D of
# {1, 3, 16, 25, 50, 64}, n_split of {0, 1, 3, 64} and n_seg of {1, 2, 7, 256} at least once, and every layout
CASES = [(1, 0, 3, 0, 2, "even", "odd"), (1, 1, 1, 1, 1, "one", "odd"), (TQ - 1, TC - 1, 3, 0, 7, "empty", "x4"), (TQ, TC, 16, 3, 7, "empty", "odd"),
         (TQ + 1, TC + 1, 25, 1, 7, "tile", "x4"), (2 * TQ + 3, 2 * TC + 5, 50, 3, 7, "tile", "odd"), (TQ, 2 * TC + 5, 64, 64, 2, "even", "x4"),
         (TQ + 1, 2 * TC + 5, 16, 1, 256, "ones", "odd"), (2 * TQ + 3, 2000, 25, 0, 7, "chunk", "odd"), (TQ + 1, 2000, 16, 3, 7, "span", "x4"),
         (3, 2000, 3, 64, 256, "ones", "odd"), (TQ + 1, 1999, 64, 0, 256, "even", "x4"), (TQ - 1, 2000, 50, 64, 7, "chunk", "odd"),
         (2 * TQ + 3, 2000, 1, 3, 2, "even", "x4")]


@pytest.mark.parametrize("kind", ["real", "lattice"])
@pytest.mark.parametrize("n_q,n_c,D,n_split,n_seg,layout,pitch", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_segment_lse_against_float64(dev, kind, n_q, n_c, D, n_split, n_seg, layout, pitch):
    rng = np.random.default_rng(n_q * 1000 + n_c * 10 + D + n_seg)
    X, Y, h, s = _data(kind, rng, n_q, n_c, D)
    ns = _resolved(n_q, n_c, n_split)
    seg_ptr = _seg_ptr(layout, rng, n_c, n_seg, -(-n_c // ns))
    if layout == "span":
        per = -(-n_c // ns)
        assert ns == 3 and any(seg_ptr[k] < per and seg_ptr[k + 1] > 2 * per for k in range(n_seg)), "no segment spans three chunks"
    if layout == "empty" and n_c > 1:
        sizes = np.diff(seg_ptr)
        assert sizes[0] == 0 and sizes[-1] == 0 and ((sizes[1:-2] == 0) & (sizes[2:-1] == 0)).any()
    want = segment_lse_ref(t_ref(X, Y, h, s), seg_ptr)
    _hold(_seg_lse(dev, X, Y, h, seg_ptr, s, n_split, pitch), want, n_q, n_c, n_split, f"{kind} {layout}")


@pytest.mark.parametrize("n_q,n_c,D", [(2 * TQ + 3, 2000, 25), (TQ + 1, 2 * TC + 5, 50), (1, 1, 3)])
def test_one_segment_equals_ot_softmin_bit_for_bit(dev, n_q, n_c, D):
    """n_seg = 1: the walk meets no boundary, the chunk plan of an explicit n_split is ot_softmin's, the lane's operations are the same"""
    rng = np.random.default_rng(n_q + n_c)
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    for n_split in (1, 3, SPLIT_MAX):
        L = _seg_lse(dev, X, Y, h, [0, n_c], s, n_split)
        np.testing.assert_array_equal(L[:, 0].view(np.uint32), _softmin(dev, X, Y, h, s, n_split).view(np.uint32))


@pytest.mark.parametrize("n_split", [0, 1, 3, SPLIT_MAX])
def test_segments_add_up_to_ot_softmin(dev, n_split):
    """float64 log-sum-exp over the segments of L[s][i] against ot_softmin's L[i]: within the two bounds added (module docstring)"""
    rng = np.random.default_rng(17)
    n_q, n_c, D, n_seg = TQ + 1, 2000, 25, 7
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    seg_ptr = _seg_ptr("empty", rng, n_c, n_seg, 0)
    L = _seg_lse(dev, X, Y, h, seg_ptr, s, n_split).astype(np.float64)
    total = lse_ref(L)
    flat = _softmin(dev, X, Y, h, s, n_split).astype(np.float64)
    allowed = lse_bound(total, n_q, n_c, n_split) + softmin_bound(flat, n_q, n_c, n_split)
    print(f"segments -> total, n_split {n_split}: max difference {np.abs(total - flat).max():.3e}, allowed {allowed.min():.3e}")
    assert (np.abs(total - flat) <= allowed).all()


def test_special_rows_subsets_and_repeats(dev):
    """h = -inf for a whole segment: -inf in that column only; NaN and overflowing candidate rows add nothing; a query without a finite
    t is -inf everywhere; a subset of the queries gives the same bits at the same explicit n_split; two calls are bit-equal"""
    rng = np.random.default_rng(3)
    n_q, n_c, D, n_seg = TQ + 5, 2 * TC + 5, 25, 7
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    seg_ptr = np.array([0, 10, 10, 40, TC, TC + 1, 100, n_c], dtype=np.int32)
    h[10:40] = -np.inf                          # segment 2 without mass
    h[3], h[45] = np.nan, np.inf                # skipped
    Y[5, :], Y[50, 3] = 3e19, np.nan            # the cost overflows: t = -inf; a NaN cost
    Y[TC, :] = np.nan                           # segment 4 is this one row
    X[4, :] = np.inf                            # a query without any finite t
    t = t_ref(X, Y, h, s)
    want = segment_lse_ref(t, seg_ptr)
    assert np.isneginf(want[:, [1, 2, 4]]).all() and np.isneginf(want[4]).all() and np.isfinite(np.delete(want[:, [0, 3, 5, 6]], 4, axis=0)).all()
    keep = np.isfinite(t[0])
    assert not keep[[3, 5, 45, 50, TC]].any()
    for n_split in (0, 1, 3, SPLIT_MAX):
        L = _seg_lse(dev, X, Y, h, seg_ptr, s, n_split)
        _hold(L, want, n_q, n_c, n_split, "special")
        np.testing.assert_array_equal(L.view(np.uint32), _seg_lse(dev, X, Y, h, seg_ptr, s, n_split).view(np.uint32))
        if n_split:
            rows = np.r_[0:3, 7, TQ - 1:n_q]   # across the first workgroup's end
            np.testing.assert_array_equal(_seg_lse(dev, X[rows], Y, h, seg_ptr, s, n_split, pitch="x4").view(np.uint32), L[rows].view(np.uint32))
    # the problem without the bad rows: the same values within the bound
    kept_ptr = np.concatenate([[0], np.cumsum(keep)[seg_ptr[1:] - 1]]).astype(np.int32)
    _hold(_seg_lse(dev, X, Y[keep], h[keep], kept_ptr, s, 1), want, n_q, int(keep.sum()), 1, "without the bad rows")


def test_op_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.ot_ops import ot_segment_lse
    X, Y, h = torch.zeros((4, 5), device=dev), torch.zeros((9, 5), device=dev), torch.zeros(9, device=dev)
    sp = torch.tensor([0, 4, 9], dtype=torch.int32, device=dev)
    for bad in (lambda: ot_segment_lse(X.double(), Y, h, sp, 1.0), lambda: ot_segment_lse(X.cpu(), Y, h, sp, 1.0), lambda: ot_segment_lse(X, Y[:, :4], h, sp, 1.0),
                lambda: ot_segment_lse(X, Y, h[:8], sp, 1.0), lambda: ot_segment_lse(X, Y, h, sp.long(), 1.0), lambda: ot_segment_lse(X, Y, h, sp.cpu(), 1.0),
                lambda: ot_segment_lse(X, Y, h, sp, 1.0, out=torch.zeros((2, 3), device=dev)), lambda: ot_segment_lse(X, Y, h, sp, 1.0, out=torch.zeros((3, 4), device=dev)),
                lambda: ot_segment_lse(X, Y, h, sp, 1.0, out=torch.zeros((2, 4), dtype=torch.float64, device=dev))):
        with pytest.raises(_abi.SpvError):
            bad()
    for bad in (lambda: ot_segment_lse(X, Y, h, sp[:1], 1.0), lambda: ot_segment_lse(X, Y, h, torch.zeros(SEG_MAX + 2, dtype=torch.int32, device=dev), 1.0),
                lambda: ot_segment_lse(X, Y, h, sp, 1.0, n_split=65), lambda: ot_segment_lse(X[:0], Y, h, sp, 1.0), lambda: ot_segment_lse(X, Y, h, sp, 0.0),
                lambda: ot_segment_lse(X, Y, h, sp, float("inf")), lambda: ot_segment_lse(X, Y, h, sp, float("nan"))):
        with pytest.raises(ValueError):
            bad()
