"""No GPU: the float64 reference, the derived bounds and the float32 transcription of tests/_poe_reference.py check themselves.
  (a) the oracle's definitions and tests/_torch_poe.py agree in float64 on every case, values and autograd gradients, to 1e-12 of each
      output's maximum; so does the kernel's chain as tests/_poe_reference.chain writes it (evaluated in float64): the closed-form backward
      the bounds are derived from is the gradient of the definition;
  (b) the numpy-float32 transcription of the kernels' formulas stays inside the derived bounds on every case of the GPU grid;
  (c) the CAP: on every STANDARD case each forward bound is at most 2e-5 x max|reference| of its output and each gradient bound at most
      1e-4 x max|reference| of its gradient -- the bounds cannot hide a failure.  Computed from the reference alone;
  (d) no cell of a committed case has its scale* within its own bound of the 1e-6 clamp (the ``live`` branch is decided);
  (e) five deliberate mistakes in the transcription each fall outside the bounds: the bounds bite."""
import pytest
import torch

from tests import _poe_reference as R

KEYS = R.FWD_KEYS + R.GRAD_KEYS
PAIRINGS = ("label", "paired", "cluster")


def _standard(pairing, n):
    return [R.standard_case(pairing, nn, B0, B1) for (nn, B0, B1) in R.standard_grid(pairing) if nn == n]


def _where(c):
    return f"({c['pairing']}, n {c['n']}, B {c['B']}, {c['kind']})"


def _agree(a, b, c, what, rel=1e-12):
    for k in KEYS:
        top = max(a[k].abs().max().item(), 1e-300)
        d = (a[k] - b[k].reshape(a[k].shape)).abs().max().item()
        assert d <= rel * top, f"{what} {k} {_where(c)}: {d:.3e} against max {top:.3e}"


def _inside(got, ref, bnd, c, what):
    for k in KEYS:
        err = (got[k].reshape(ref[k].shape) - ref[k]).abs()
        assert torch.isfinite(err).all(), (what, k, _where(c))
        over = err > bnd[k]
        assert not over.any(), f"{what} {k} {_where(c)}: error {err[over].max():.3e} over its bound {bnd[k][over].min():.3e}"


def _outside(got, ref, bnd) -> bool:
    return any(bool(((got[k].reshape(ref[k].shape) - ref[k]).abs() > bnd[k]).any()) for k in KEYS)


def _check_case(c):
    ref = R.reference(c)
    _agree(ref, R.reference_torch_poe(c), c, "_torch_poe")
    val, bnd, margin = R.bounds(c)
    _agree(ref, val, c, "chain", rel=1e-9)     # (float64 through another order of operations, at exp(30) in the clamp cases)
    assert margin is None or margin > 0.0, f"{_where(c)}: a scale* within its bound of the clamp ({margin:.3e})"
    _inside(R.transcription(c), ref, bnd, c, "transcription")
    return ref, bnd


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_standard_cases_agree_stay_inside_and_meet_the_cap(pairing, n):
    for c in _standard(pairing, n):
        ref, bnd = _check_case(c)
        worst = R.cap_ratios(c, ref, bnd)
        k = max(worst, key=worst.get)
        assert worst[k] <= 1.0, f"{k} {_where(c)}: bound {worst[k] * R.cap_of(k):.3e} x max|reference| over the cap {R.cap_of(k):.0e}"


@pytest.mark.parametrize("name", sorted(R.STRUCTURED))
def test_structured_cases_agree_and_stay_inside(name):
    _check_case(R.structured_case(name))


def test_structured_cases_reach_their_branches():
    """the committed structures are what their names say"""
    S = {k: R.structure(R.structured_case(k)) for k in R.STRUCTURED}
    count = lambda name, g, m: int((S[name]["mode"][g] == m).sum())
    assert count("label-one_side_0", 0, 2) > 0 and count("label-one_side_0", 1, 2) == 0
    assert count("label-one_side_1", 1, 2) > 0 and count("label-one_side_1", 0, 2) == 0
    assert count("label-more_on_0", 0, 1) > 0 and count("label-more_on_1", 1, 1) > 0
    assert count("label-each_own", 0, 0) == 30 and sorted(S["label-each_own"]["partner"][0]) == list(range(30))
    labs = R.structured_case("label-codes_edge")["labels"]
    assert all(int(l.min()) == 0 and int(l.max()) == 1023 for l in labs)
    p = S["paired-mostly_empty"]["partner"]
    assert all(int((p[g][32 * w: 32 * w + 32] == 0).sum()) >= 20 for g in (0, 1) for w in range(4))
    p = S["paired-shared_ws"]["partner"][0]
    assert p[0] == p[5] == p[31] == p[32] == 9 and int((p == 9).sum()) == 4
    p = S["paired-diagonal"]["partner"]
    assert all(len(set(p[g].tolist())) == 45 for g in (0, 1))
    blk = R.block_of(R.structured_case("paired-ties"))
    assert int((blk == blk.max(1, keepdim=True).values).sum(1).max()) >= 2
    assert count("cluster-lone", 0, 2) > 0 and count("cluster-lone", 1, 2) > 0
    assert count("cluster-unequal", 0, 1) + count("cluster-unequal", 1, 1) > 0
    W = S["cluster-empty_rows"]["W"]
    assert all(int((W[g].sum(1) == 0).sum()) > 5 for g in (0, 1))
    c = R.structured_case("cluster-absent")
    gone = torch.ones(c["plan"].shape[1], dtype=torch.bool)
    gone[c["idx"][1].long()] = False
    assert int((torch.as_tensor(c["plan"])[c["idx"][0].long()][:, gone] > 0).sum()) > 50
    for name in ("paired-clamp", "cluster-clamp"):
        ref = R.reference(R.structured_case(name))
        assert all(float(ref[f"scale{g}"].median()) < 5e-7 for g in (0, 1))


MUTATION_CASES = {
    "drop_gk_jl": ("label-codes_edge", "paired-shared_ws", "cluster-lone"),
    "t1_mode2": ("label-one_side_0", "label-one_side_1"),
    "drop_second": ("paired-shared_ws", "paired-mostly_empty"),
    "no_live": ("paired-clamp", "cluster-clamp"),
    "no_passthrough": ("cluster-lone",),
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutations_of_the_transcription_fall_outside_the_bounds(mut):
    for name in MUTATION_CASES[mut]:
        c = R.structured_case(name)
        ref, (_, bnd, _) = R.reference(c), R.bounds(c)
        _inside(R.transcription(c), ref, bnd, c, "transcription")
        assert _outside(R.transcription(c, mut), ref, bnd), f"{mut} on {name}: still inside the bounds"
