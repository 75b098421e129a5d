"""CPU: the yardstick of the transport-projection tests against itself (tests/_ot_project_reference.py): ``project_ref`` against a dense
float64 softmax(t) @ V on hand cases, the bound against the kernel's own float32 sequence (``project_emulated``) at several
chunkings, and the bound against three mutants it must reject -- it was derived, not fitted, and is still sharp enough to see a
candidate of a thousandth of a row's mass go missing.  The seeds below were checked on the CPU: each mutant moves at least one entry
past the bound (the test prints by how much)."""
import numpy as np
import pytest

from tests._ot_project_reference import project_bound, project_emulated, project_ref
from tests._ot_reference import t_ref


def _case(seed, n_q=6, n_c=150, D=5, n_v=5, s=1.5):
    rng = np.random.default_rng(seed)
    X, Y = rng.standard_normal((n_q, D)).astype(np.float32), rng.standard_normal((n_c, D)).astype(np.float32)
    h = rng.standard_normal(n_c).astype(np.float32)
    V = rng.standard_normal((n_c, n_v)).astype(np.float32)
    V[:, 0] = 1.0
    return t_ref(X, Y, h, s), V


def test_project_ref_on_hand_cases():
    t = np.array([[0.0, np.log(3.0), -np.inf, np.nan], [-np.inf, np.nan, np.inf, -np.inf], [5.0, 5.0, 5.0, 5.0]])
    V = np.array([[1.0, 10.0], [5.0, -10.0], [1e30, 1e30], [-1e30, 7.0]])
    out, L = project_ref(t, V)
    np.testing.assert_allclose(out[0], [0.25 * 1 + 0.75 * 5, 0.25 * 10 - 0.75 * 10], rtol=1e-15)
    assert np.isnan(out[1]).all() and np.isneginf(L[1])
    np.testing.assert_allclose(out[2], V.mean(0), rtol=1e-15)
    np.testing.assert_allclose(L, [np.log(4.0), -np.inf, 5 + np.log(4.0)], rtol=1e-15)
    tt, VV = _case(3)
    w = np.exp(tt.astype(np.float64))
    np.testing.assert_allclose(project_ref(tt, VV)[0], (w / w.sum(1, keepdims=True)) @ VV.astype(np.float64), rtol=1e-12, atol=1e-14)
    out0, L0 = project_ref(np.zeros((2, 0), np.float32), np.zeros((0, 3), np.float32))
    assert out0.shape == (2, 3) and np.isnan(out0).all() and np.isneginf(L0).all()


@pytest.mark.parametrize("chunks", [1, 2, 7, 64])
@pytest.mark.parametrize("seed", [3, 4])
def test_the_bound_accepts_the_emulated_kernel(seed, chunks):
    t, V = _case(seed)
    t[1, 10:20], t[2, :] = -np.inf, np.nan
    n_c = t.shape[1]
    out, L = project_emulated(t, V, chunks=chunks, block=2)
    want, want_L = project_ref(t, V)
    bound = project_bound(t, V, -(-n_c // chunks), chunks)
    assert np.isnan(out[2]).all() and np.isneginf(L[2]) and np.isnan(want[2]).all()
    rows = [0, 1, 3, 4, 5]
    err = np.abs(out[rows].astype(np.float64) - want[rows])
    print(f"chunks {chunks}: max err / bound = {(err / bound[rows]).max():.3f}")
    assert (err <= bound[rows]).all()
    assert (out[rows, 0] == 1.0).all(), "a column of ones repeats the sum's operations"
    assert np.array_equal(project_emulated(t, V, chunks=chunks, block=5)[0][rows], out[rows]), "a column must not depend on its block"


@pytest.mark.parametrize("mutant", ["candidate-left-out", "V-shifted-by-a-row", "fp16-weights"])
def test_the_bound_rejects_mutants(mutant):
    t, V = _case(5)
    want, _ = project_ref(t, V)
    n_c = t.shape[1]
    t64 = t.astype(np.float64)
    p = np.exp(t64 - t64.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    if mutant == "candidate-left-out":
        i = 0
        j = int(np.flatnonzero(p[i] >= 1e-3)[np.argmin(p[i][p[i] >= 1e-3])])   # the lightest candidate that still holds a thousandth of row 0
        t2 = t.copy()
        t2[i, j] = -np.inf
        got = project_ref(t2, V)[0]
    elif mutant == "V-shifted-by-a-row":
        got = project_ref(t, np.roll(V, 1, axis=0))[0]
    else:
        p16 = p.astype(np.float16).astype(np.float64)
        got = (p16 @ V.astype(np.float64)) / p16.sum(1, keepdims=True)
    worst = 0.0
    for chunks in (1, 7):
        bound = project_bound(t, V, -(-n_c // chunks), chunks)
        worst = max(worst, float((np.abs(got - want) / bound).max()))
        assert (np.abs(got - want) > bound).any(), f"{mutant} passes the bound at {chunks} chunk(s)"
    print(f"{mutant}: worst entry at {worst:.1f} bounds")
