"""GPU: spv_ot_project (spvipes_amd.ot_ops.ot_project) against the yardstick of tests/_ot_project_reference.py.  Shapes are sized by the
tiles the library reports (TQ queries per workgroup, TC candidates per LDS tile) and by the column block VB of the kernel form that
serves D: one below, at and one above a tile / a block, several of them, more than one workgroup, and about 2000 candidates so that the
automatic chunk count exceeds 1.  Every call goes through ``_project``: odd or 16-byte-multiple row pitches with NaN in the pitch
padding of X, Y and V (a kernel that read it would lose the candidate or poison a column) and sentinels around the value-major
output and behind L, which must come back untouched.  Every test here imports the new function and fails without it.

THE BOUND ON out (``project_bound`` of tests/_ot_project_reference.py), from the kernel's arithmetic (csrc/spv_ot_project.h), in units
of u = 2^-24.  t is bit-equal to the reference's, so only the reduction errs.  out_v = N_v / S: S is ot_softmin's running sum,
N_v = sum_j w_j V_jv the column's accumulator, w_j = exp(t_j - m).  Write p for the float64 softmax, y_j = max_k t_k - t_j,
A_v = sum_j p_j |V_jv| and ref_v = sum_j p_j V_jv, |ref_v| <= A_v.
  * The numerator.  Term j enters as V_jv itself (a rescale step) or as e V_jv inside one fma, and is later multiplied by the e of every
    rescale step.  A factor e = exp(-|d|) carries at most (2.5 |d| + 2) u (tests/test_gpu_ot.py: the difference, the product with
    log2 e, log2 e itself, the ulp of v_exp_f32).  The |d| parts of term j telescope to 2.5 y_j u -- through the merges as well, whose
    d completes the way from the chunk's maximum to the final one -- so together they are 2.5 u sum_j w_j y_j |V_jv|, relative to
    S: 2.5 u sum_j p_j y_j |V_jv|.  Where |V| is constant this is at most 2.5 u ln(n_c) A_v (the entropy of p); where it is not, no
    multiple of A_v bounds it (a huge value behind a tiny weight), so the term is computed from the data in float64 as it stands.
  * The constant parts: the entry's 2 u once per term, 2 u A_v in all.  Every step rounds its fma once, relative to the accumulator,
    which is at most the sum of the |terms| so far: u A_v per step; a rescale step also multiplies everything before it by e (2 u).
    At most 3 u A_v per step, 3 n_chain u A_v.  A merge is one fma and one e: 3 u A_v per chunk; 4 is asserted.
  * The denominator has ot_softmin's relative error, (3 n_chain + 3 n_split + 2.5 ln n_c + 2) u (tests/test_gpu_ot.py, without the
    logarithm's part); it multiplies |ref_v|.  The errors of N_v and S share their factors e and cancel in part -- for a column of ones
    entirely -- but nothing here counts on that.  The division rounds once: u |ref_v|.
Together
    |out_v - ref_v| <= (3 n_chain + 4 n_split + 18) u A_v + 2.5 u sum_j p_j y_j |V_jv| + ((3 n_chain + 4 n_split + 2.5 ln(n_c + 1) + 18) u + 2 u) |ref_v|
with n_chain the candidates of a chunk; the 16 u beyond the entry's 2 u and the second u of the last term are the slack for the
second-order terms and the float64 reference's own error.  tests/test_ot_project_reference_cpu.py shows the bound still rejects a
candidate of a thousandth of a row's mass left out, V shifted by a row, and weights rounded to fp16.  Nothing was fitted to the
kernel's output."""
import numpy as np
import pytest
import torch

from tests._ot_project_reference import project_bound, project_ref
from tests._ot_reference import t_ref
from tests.test_gpu_ot import _data, _operands, _padded, _pitch, _softmin
from tests.test_gpu_ot_segments import _seg_lse
from tests.test_gpu_ot_segments import lse_bound as seg_bound

pytestmark = pytest.mark.gpu

TQ, TC, SPLIT_MAX, VAL_MAX = 128, 64, 64, 256   # what the parametrisation assumes; test_tiles_and_shape_functions pins them
U = 2.0 ** -24
OUT_SENTINEL, L_SENTINEL = -7.25, -7.5


def _vb(D):
    return 16 if D > 32 else 32   # test_tiles_and_shape_functions pins it against the library


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _resolved(n_q, n_c, n_v, n_split):
    from spvipes_amd.ot_ops import ot_project_splits
    return n_split or ot_project_splits(n_q, n_c, n_v)


def _project(dev, X, Y, h, V, s, n_split=0, pitch="odd"):
    """one call with NaN in every pitch padding and sentinels all around the value-major output and behind L
    -> (out float32 [n_q, n_v], L float32 [n_q]) on the host"""
    from spvipes_amd.ot_ops import ot_project
    n_q, n_v = X.shape[0], V.shape[1]
    buf = torch.full((n_v + 2, n_q + 3), OUT_SENTINEL, dtype=torch.float32, device=dev)
    Lb = torch.full((n_q + 3,), L_SENTINEL, dtype=torch.float32, device=dev)
    Vd = _padded(V, _pitch(n_v, pitch), dev)
    out, L = ot_project(*_operands(dev, X, Y, pitch), torch.from_numpy(h).to(dev), Vd, s, n_split=n_split, out=(buf[1:n_v + 1], Lb), return_lse=True)
    assert out.shape == (n_q, n_v) and L.shape == (n_q,)
    buf, Lb = buf.cpu().numpy(), Lb.cpu().numpy()
    assert (buf[0] == OUT_SENTINEL).all() and (buf[n_v + 1] == OUT_SENTINEL).all() and (buf[:, n_q:] == OUT_SENTINEL).all(), "out written outside [n_v][n_q]"
    assert (Lb[n_q:] == L_SENTINEL).all(), "L written beyond n_q"
    return np.ascontiguousarray(buf[1:n_v + 1, :n_q].T), Lb[:n_q]


def _values(kind, rng, n_c, n_v):
    V = (rng.integers(-8, 9, (n_c, n_v)).astype(np.float32) / 4) if kind == "lattice" else rng.standard_normal((n_c, n_v)).astype(np.float32)
    if n_v > 1:
        V[:, -1] = 1.0
    return V


def _hold(out, L, t, V, n_q, n_c, n_split, what=""):
    """out within the bound of the float64 mean, NaN and -inf exactly where a row has no finite t"""
    ns = _resolved(n_q, n_c, V.shape[1], n_split)
    want, want_L = project_ref(t, V)
    some = np.isfinite(want_L)
    assert np.isnan(out[~some]).all() and np.isneginf(L[~some]).all(), "a row without a contributing candidate: NaN and -inf"
    assert not np.isnan(out[some]).any()
    if some.any():
        err, bound = np.abs(out[some].astype(np.float64) - want[some]), project_bound(t, V, -(-n_c // ns), ns)[some]
        print(f"project {what} n_q {n_q} n_c {n_c} n_v {V.shape[1]} n_split {n_split} ({ns}): max |out - ref| = {err.max():.3e}, "
              f"max err / bound = {np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max():.4f}")
        assert (err <= bound).all()
    return some


def test_tiles_and_shape_functions(dev):
    from spvipes_amd.ot_ops import OT_VAL_MAX, ot_project_block, ot_project_splits, ot_project_ws_bytes, ot_tiles
    assert ot_tiles() == (TQ, TC) and OT_VAL_MAX == VAL_MAX
    assert [ot_project_block(D) for D in (1, 17, 25, 33, 64)] == [_vb(D) for D in (1, 17, 25, 33, 64)] == [32, 32, 32, 16, 16]
    assert ot_project_splits(300, 2000, 33) == 7 and ot_project_splits(127, 2001, 1) == 7 and ot_project_splits(300, 200, 35) == 1   # what the cases rely on
    assert ot_project_ws_bytes(300, 7, 1) == 0 and ot_project_ws_bytes(300, 7, 3) == 3 * 9 * 300 * 4


# (n_q, n_c, D, n_v as (blocks, extra): blocks * VB + extra, n_split, pitch): every n_q of {1, TQ-1, TQ, TQ+1, 300}, n_c of {1, TC-1, TC, TC+1,
# 200, 2000}, D of {1, 17, 25, 33, 64}, n_v of {1, VB-1, VB, VB+1, 2VB+3} and n_split of {0, 1, 2, 7} at least once
CASES = [(1, 1, 1, (0, 1), 1, "odd"), (TQ - 1, TC - 1, 17, (1, -1), 0, "x4"), (TQ, TC, 25, (1, 0), 2, "odd"), (TQ + 1, TC + 1, 33, (1, 1), 7, "x4"),
         (300, 200, 64, (2, 3), 2, "odd"), (300, 2000, 25, (1, 1), 0, "odd"), (TQ + 1, 2000, 64, (2, 3), 7, "x4"), (TQ - 1, 2001, 17, (0, 1), 0, "odd"),
         (1, 200, 33, (1, 0), 1, "x4"), (TQ, 1, 1, (1, -1), 2, "odd"), (300, TC + 1, 1, (2, 3), 7, "x4")]


@pytest.mark.parametrize("kind", ["real", "lattice"])
@pytest.mark.parametrize("n_q,n_c,D,nv,n_split,pitch", CASES, ids=["-".join(map(str, c[:3] + c[3] + c[4:])) for c in CASES])
def test_project_against_float64(dev, kind, n_q, n_c, D, nv, n_split, pitch):
    """the bound; L equal to ot_softmin's at the same chunk count; the column of ones exactly 1; two calls, any column subset and any
    query subset the same bits (at the resolved chunk count passed explicitly: the automatic one depends on n_q and n_v)"""
    n_v = nv[0] * _vb(D) + nv[1]
    rng = np.random.default_rng(n_q * 1000 + n_c * 10 + D)
    X, Y, h, s = _data(kind, rng, n_q, n_c, D)
    V = _values(kind, rng, n_c, n_v)
    t = t_ref(X, Y, h, s)
    out, L = _project(dev, X, Y, h, V, s, n_split, pitch)
    some = _hold(out, L, t, V, n_q, n_c, n_split, kind)
    assert some.all()
    ns = _resolved(n_q, n_c, n_v, n_split)
    np.testing.assert_array_equal(L.view(np.uint32), _softmin(dev, X, Y, h, s, ns, pitch).view(np.uint32))
    if n_v > 1:
        assert (out[:, -1] == 1.0).all(), "a column of ones performs the sum's very operations"
    again, L2 = _project(dev, X, Y, h, V, s, ns, "x4" if pitch == "odd" else "odd")   # other pitches, the chunk count explicit
    np.testing.assert_array_equal(again.view(np.uint32), out.view(np.uint32))
    np.testing.assert_array_equal(L2.view(np.uint32), L.view(np.uint32))
    cols = np.flatnonzero(rng.random(n_v) < 0.4)
    cols = cols if cols.size else np.array([n_v - 1])
    sub, _ = _project(dev, X, Y, h, np.ascontiguousarray(V[:, cols]), s, ns, pitch)
    np.testing.assert_array_equal(sub.view(np.uint32), out[:, cols].view(np.uint32))
    rows = np.arange(n_q)[::3]
    few, Lf = _project(dev, X[rows], Y, h, V, s, ns, pitch)
    np.testing.assert_array_equal(few.view(np.uint32), out[rows].view(np.uint32))
    np.testing.assert_array_equal(Lf.view(np.uint32), L[rows].view(np.uint32))


@pytest.mark.parametrize("n_split", [1, 7, 0])
def test_one_hot_values_agree_with_the_segment_kernel(dev, n_split):
    """V = the one-hot encoding of contiguous segments: out[i, s] is the segment's share of row i, which spv_ot_segment_lse gives as
    exp(L[s][i] - L[i]).  The share from the logarithms errs by the two lse bounds added (relative: they stand in an exponent); out
    by its own bound."""
    rng = np.random.default_rng(31)
    n_q, n_c, D, n_seg = TQ + 1, 2000, 25, 7
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    seg_ptr = np.concatenate([[0], np.sort(rng.integers(0, n_c + 1, n_seg - 1)), [n_c]]).astype(np.int32)
    V = np.zeros((n_c, n_seg), np.float32)
    for g in range(n_seg):
        V[seg_ptr[g]:seg_ptr[g + 1], g] = 1.0
    out, L = _project(dev, X, Y, h, V, s, n_split)
    t = t_ref(X, Y, h, s)
    _hold(out, L, t, V, n_q, n_c, n_split, "one-hot")
    Ls = _seg_lse(dev, X, Y, h, seg_ptr, s, n_split).astype(np.float64)
    ns = _resolved(n_q, n_c, n_seg, n_split)
    share = np.exp(Ls - L.astype(np.float64)[:, None])
    with np.errstate(invalid="ignore"):
        rel = np.where(np.isfinite(Ls), seg_bound(Ls, n_q, n_c, n_split) + seg_bound(L.astype(np.float64), n_q, n_c, ns)[:, None], 0.0)
    allowed = project_bound(t, V, -(-n_c // ns), ns) + share * np.expm1(rel) * 1.01
    assert (np.abs(out.astype(np.float64) - share) <= allowed).all()
    np.testing.assert_allclose(out.astype(np.float64).sum(1), 1.0, atol=n_seg * allowed.max())


@pytest.mark.parametrize("n_split", [1, 2, 0])
def test_candidates_without_mass_and_queries_without_candidates(dev, n_split):
    """h = -inf candidates, NaN and overflowing candidate rows add nothing, even with huge value rows behind them; a query with no
    finite t gets NaN and -inf and its neighbours are not touched; n_c = 0 gives NaN and -inf everywhere"""
    rng = np.random.default_rng(5)
    n_q, n_c, D, n_v = TQ + 3, 2000, 25, 35
    X, Y, h, s = _data("real", rng, n_q, n_c, D)
    V = _values("real", rng, n_c, n_v)
    dead = np.concatenate([np.arange(0, n_c, 7), [TC - 1, TC, n_c - 1]])
    h[dead[::3]] = -np.inf
    Y[dead[1::3]] = np.nan
    Y[dead[2::3], 0] = 3e19            # the squared difference overflows: t = -inf
    V[dead, :-1] = 3e38
    X[[2, TQ]] = np.nan                # queries with no finite t
    t = t_ref(X, Y, h, s)
    assert not np.isfinite(t[:, dead]).any() and not np.isfinite(t[[2, TQ]]).any()
    out, L = _project(dev, X, Y, h, V, s, n_split)
    some = _hold(out, L, t, V, n_q, n_c, n_split, "edge")
    assert list(np.flatnonzero(~some)) == [2, TQ]
    assert np.abs(out[some]).max() < 10 and (out[some, -1] == 1.0).all()
    ns = _resolved(n_q, n_c, n_v, n_split)
    alive = np.setdiff1d(np.arange(n_c), dead)   # the same candidates without the dead ones: the same sums in the same order per chunk only at ONE chunk
    if ns == 1:
        kept, Lk = _project(dev, X, Y[alive], h[alive], V[alive], s, 1)
        np.testing.assert_array_equal(kept[some].view(np.uint32), out[some].view(np.uint32))
        np.testing.assert_array_equal(Lk.view(np.uint32), L.view(np.uint32))
    empty, L0 = _project(dev, X, Y[:0], h[:0], V[:0], s, n_split)
    assert empty.shape == (n_q, n_v) and np.isnan(empty).all() and np.isneginf(L0).all()


def test_wrapper_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.ot_ops import ot_project
    X, Y = torch.zeros((5, 3), device=dev), torch.zeros((8, 3), device=dev)
    h, V = torch.zeros(8, device=dev), torch.zeros((8, 4), device=dev)
    assert ot_project(X, Y, h, V, 1.0).shape == (5, 4)
    for bad in (dict(V=V[:7]), dict(V=V.double()), dict(V=V.cpu()), dict(V=torch.zeros((4, 8), device=dev).t()), dict(V=V[:, 0]), dict(V=torch.zeros((8, 0), device=dev)),
                dict(h=h[:7]), dict(Y=Y[:, :2]), dict(X=X.cpu()), dict(out=torch.zeros((4, 4), device=dev)), dict(out=torch.zeros((5, 5), device=dev)),
                dict(out=torch.zeros((5, 4), device=dev).t()), dict(out=(torch.zeros((4, 5), device=dev), torch.zeros(5, device=dev))),
                dict(out=(torch.zeros((4, 5), device=dev), torch.zeros(4, device=dev)), return_lse=True)):
        kw = dict(dict(X=X, Y=Y, h=h, V=V, inv_eps=1.0), **bad)
        with pytest.raises(_abi.SpvError):
            ot_project(**kw)
    for bad in (dict(V=torch.zeros((8, VAL_MAX + 1), device=dev)), dict(inv_eps=0.0), dict(inv_eps=float("inf")), dict(n_split=-1), dict(n_split=SPLIT_MAX + 1),
                dict(n_split=True), dict(X=X[:0])):
        kw = dict(dict(X=X, Y=Y, h=h, V=V, inv_eps=1.0), **bad)
        with pytest.raises(ValueError):
            ot_project(**kw)
    wide = ot_project(X, Y, h, torch.zeros((8, 64), device=dev)[:, :4], 1.0)   # a row stride beyond n_v is fine
    assert wide.shape == (5, 4) and not torch.isnan(wide).any()
