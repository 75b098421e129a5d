"""GPU: spv_tsne_repulsion (spvipes_amd.tsne_ops.repulsion) against the float64 yardstick of tests/_tsne_reference.py.  Shapes: one below, at
and one above the 128-query tile and the 64-candidate LDS tile, several tiles, no candidates, chunk counts that leave a chunk without
candidates.  Every call goes through ``_run``: padded row pitches with NaN in the padding and in rows past the end of Q and C (a kernel
that read them would poison a sum), and sentinels around Zrow and the dimension-major F, which must come back untouched.  Every test
here imports the new function and fails without it.

THE BOUND (``repulsion_bound``), u = 2^-24, from the roundings the contract lists (include/spvipes_hip.h), first order in u:
    d2: D differences (1 u each, 2 u on each square) and D fmas (1 u each on a sum of non-negative terms): (D + 2) u
    s = fl32(1 + d2): the error of d2 is at most (D + 2) u d2 <= (D + 2) u s, and one rounding: (D + 3) u
    w = fl32(1 / s): one more, (D + 4) u  -- the terms of Zrow: c_Z(D) = D + 4
    w2 = fl32(w w): 2 (D + 4) + 1 = (2 D + 9) u; the difference for the force 1 u; the product 1 u: c_F(D) = 2 D + 11
so |Zrow - ref| <= ((D + 4) (1 + 2^-10) 2^-24 + (n_c + 8) 2^-53) sum_j |w_j|, the same for F with c_F and sum_j |w_j^2 (q_t - c_jt)|, plus
2^-149 (1 + |q_t - c_jt|) per term for fp32 products below the normal range.  The factor 1 + 2^-10 covers the higher orders, the fp64 term
the kernel's n_c sequential additions and the reference's own roundings.  tests/test_tsne_reference_cpu.py shows that a reference that
drops one candidate, weighs the force with w, or counts the excluded pair leaves this bound on these inputs.  Nothing was fitted to
the kernel's output."""
import numpy as np
import pytest
import torch

from tests import _tsne_reference as R

pytestmark = pytest.mark.gpu

N_Q = (1, 127, 128, 129, 300)
N_C = (0, 1, 3, 63, 64, 65, 257, 1000)
N_SPLIT = (0, 1, 2, 3, 5)
Z_SENTINEL, F_SENTINEL = -7.25, -7.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _padded(dev, A, extra_rows=2, pitch=3):
    """A's rows inside a NaN-filled buffer with a longer pitch and rows past the end"""
    n, D = A.shape
    buf = torch.full((n + extra_rows, D + pitch), float("nan"), dtype=torch.float32, device=dev)
    if n:
        buf[:n, :D] = torch.from_numpy(A).to(dev)
    return buf[:n, :D]


def _run(dev, Q, C, exclude=None, n_split=0):
    """-> (Zrow [n_q], F [D, n_q]) float64 on the host, after checking the sentinels"""
    from spvipes_amd.tsne_ops import repulsion
    n_q, D = Q.shape
    Zb = torch.full((n_q + 2,), Z_SENTINEL, dtype=torch.float64, device=dev)
    Fb = torch.full((D + 1, n_q + 3), F_SENTINEL, dtype=torch.float64, device=dev)
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).to(dev)
    Zv = Zb[:n_q]
    Z, F = repulsion(_padded(dev, Q), _padded(dev, C), exclude=ex, n_split=n_split, out=(Zv, Fb[:D]))
    torch.cuda.synchronize()
    Zh, Fh = Zb.cpu().numpy(), Fb.cpu().numpy()
    assert (Zh[n_q:] == Z_SENTINEL).all() and (Fh[D] == F_SENTINEL).all() and (Fh[:, n_q:] == F_SENTINEL).all(), "wrote outside Zrow / F"
    return Zh[:n_q].copy(), Fh[:D, :n_q].copy()


def _hold(Z, F, ref, D):
    bZ, bF = R.repulsion_bound(ref, D)
    eZ, eF = np.abs(Z - ref["Z"]), np.abs(F - ref["F"])
    assert np.isfinite(Z).all() and np.isfinite(F).all()
    assert (eZ <= bZ).all(), f"Zrow: worst {np.nanmax(eZ / np.maximum(bZ, 1e-300)):.3g} of its bound"
    assert (eF <= bF).all(), f"F: worst {np.nanmax(eF / np.maximum(bF, 1e-300)):.3g} of its bound"


def _slice(ref, n_q):
    return {k: (v[:n_q] if k in ("Z", "absZ") else v[:, :n_q] if k != "n_c" else v) for k, v in ref.items()}


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_all_shapes_and_chunk_counts_q_not_c(dev, D):
    """every n_q x n_c x n_split: the reference once per n_c at 300 queries (a query's row does not depend on the others, which
    test_rows_are_independent checks on the kernel)"""
    for n_c in N_C:
        Q, C = R.repulsion_case("spread", max(N_Q), n_c, D)
        ref = R.repulsion_ref(Q, C)
        for n_q in N_Q:
            for n_split in N_SPLIT:   # 3 candidates in 5 chunks: two chunks without candidates
                Z, F = _run(dev, Q[:n_q], C, n_split=n_split)
                _hold(Z, F, _slice(ref, n_q), D)
                if n_c == 0:
                    assert not Z.any() and not F.any() and not np.signbit(Z).any() and not np.signbit(F).any(), "+0 everywhere"


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_q_is_c_with_exclude(dev, D):
    for n in (1, 129, 300):
        Q, C = R.repulsion_case("same", n, n, D)
        ex = np.arange(n)
        ref = R.repulsion_ref(Q, C, ex)
        for n_split in N_SPLIT:
            Z, F = _run(dev, Q, C, exclude=ex, n_split=n_split)
            _hold(Z, F, ref, D)
    # an exclude outside [0, n_c) skips nothing; without exclude the self pair adds exactly w = 1 and a force of 0
    Z0, F0 = _run(dev, Q, C, n_split=1)
    Z1, F1 = _run(dev, Q, C, exclude=np.full(n, -1), n_split=1)
    Z2, F2 = _run(dev, Q, C, exclude=np.full(n, n), n_split=1)
    assert np.array_equal(Z0, Z1) and np.array_equal(Z0, Z2) and np.array_equal(F0, F1) and np.array_equal(F0, F2)
    _hold(Z0, F0, R.repulsion_ref(Q, C), D)


@pytest.mark.parametrize("kind", ["dups", "far"])
@pytest.mark.parametrize("D", [1, 2, 4])
def test_duplicate_and_far_apart_points(dev, kind, D):
    Q, C = R.repulsion_case(kind, 129, 257, D)
    ref = R.repulsion_ref(Q, C)
    for n_split in (1, 3):
        Z, F = _run(dev, Q, C, n_split=n_split)
        _hold(Z, F, ref, D)
    if kind == "dups":
        assert (Z >= 257 / 5 * 0.3).all(), "many pairs at distance 0 weigh 1 each"


def test_two_calls_agree_bit_for_bit(dev):
    Q, C = R.repulsion_case("spread", 300, 1000, 2)
    for n_split in (0, 1, 5):
        a, b = _run(dev, Q, C, n_split=n_split), _run(dev, Q, C, n_split=n_split)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_rows_are_independent(dev):
    """a query's sums are the same bits whichever other queries share the call, and whichever lane and tile it lands in"""
    Q, C = R.repulsion_case("spread", 300, 1000, 3)
    for n_split in (1, 3):
        Z, F = _run(dev, Q, C, n_split=n_split)
        for rows in (np.arange(130, 300), np.array([299, 0, 128, 5]), np.array([77])):
            Zs, Fs = _run(dev, Q[rows], C, n_split=n_split)
            assert np.array_equal(Zs, Z[rows]) and np.array_equal(Fs, F[:, rows])


def test_chunk_counts_agree_within_the_summation_term(dev):
    Q, C = R.repulsion_case("spread", 129, 1000, 2)
    ref = R.repulsion_ref(Q, C)
    sZ, sF = R.summation_bound(ref)
    base = _run(dev, Q, C, n_split=1)
    for n_split in (2, 3, 5, 64):
        Z, F = _run(dev, Q, C, n_split=n_split)
        assert (np.abs(Z - base[0]) <= sZ).all() and (np.abs(F - base[1]) <= sF).all()


def test_exact_partial_sums_agree_bit_for_bit_across_chunk_counts(dev):
    """coordinates 0 / 1 at D = 1: every term is a multiple of 1/4 and every partial sum exact, so no order of addition can change a
    bit, and the float64 reference is the result itself"""
    Q, C = R.exact_case(300, 1000)
    ref = R.repulsion_ref(Q, C)
    for n_split in (0, 1, 2, 3, 5):
        Z, F = _run(dev, Q, C, n_split=n_split)
        assert np.array_equal(Z, ref["Z"]) and np.array_equal(F, ref["F"])


def test_automatic_chunks_and_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.tsne_ops import repulsion, tsne_splits, tsne_ws_bytes
    assert tsne_splits(300, 1000) == 3 and tsne_splits(300, 257) == 1 and tsne_ws_bytes(300, 2, 3) == 3 * 3 * 300 * 8
    Q = torch.zeros((4, 5), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        repulsion(Q, Q)
    Q = Q[:, :2]
    with pytest.raises(ValueError, match="n_split"):
        repulsion(Q, Q, n_split=65)
    with pytest.raises(_abi.SpvError, match="exclude"):
        repulsion(Q, Q, exclude=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(_abi.SpvError, match="out F"):
        repulsion(Q, Q, out=(torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros((2, 3), dtype=torch.float64, device=dev)))
