"""No GPU: the float64 reference, the derived bounds and the float32 transcription of tests/_poe_n_reference.py (the N-group component
PoE, csrc/spv_poe_n.h) check themselves.
  (a) the definition with autograd and the six kernels' chain as tests/_poe_n_reference.chain writes it (evaluated in float64) agree on
      every case, values and gradients, to 1e-12 of each output's maximum (1e-9 on the clamp cases: exp(30)): the closed-form backward
      the bounds are derived from is the gradient of the definition.  The one tie to upstream semantics: for two groups with the same
      codes at the same positions and statistics constant inside a component, the definition equals oracle.poe_cluster on a plan that
      is uniform inside each component, to 1e-12 -- and not beyond that condition, which the header of csrc/spv_poe_n.h now says;
  (b) the numpy-float32 transcription of the kernels' formulas and reduction orders stays inside the derived bounds on every case;
  (c) the CAP: on every STANDARD case each forward bound is at most 2e-5 x max|reference| of its output and each gradient bound at most
      1e-4 x max|reference| of its gradient, computed from the reference alone.  The two grid points over it (OVER_CAP, both n = 1) and
      ``lopsided`` are held to their bound only;
  (d) no cell of a committed case has its scale* within its own bound of the 1e-6 clamp, and the structured cases reach the branches
      their names promise;
  (e) eight deliberate mistakes in the transcription each fall outside the bounds: the bounds bite."""
import numpy as np
import pytest
import torch

from oracle import spvipes_oracle as O
from tests import _poe_n_reference as R

_DONE = {}


def _where(c):
    return f"({c['kind']}, n {c['n']}, B {c['B']}, ncomp {c['ncomp']})"


def _agree(a, b, c, what, rel=1e-12, keys=None):
    for k in (R.keys(c) if keys is None else keys):
        top = max(a[k].abs().max().item(), 1e-300)
        d = (a[k] - b[k].reshape(a[k].shape)).abs().max().item()
        assert d <= rel * top, f"{what} {k} {_where(c)}: {d:.3e} against max {top:.3e}"


def _inside(got, ref, bnd, c, what):
    for k in R.keys(c):
        err = (got[k].reshape(ref[k].shape) - ref[k]).abs()
        assert torch.isfinite(err).all(), (what, k, _where(c))
        over = err > bnd[k]
        assert not over.any(), f"{what} {k} {_where(c)}: error {err[over].max():.3e} over its bound {bnd[k][over].min():.3e}"


def _outside(got, ref, bnd, c) -> bool:
    return any(bool(((got[k].reshape(ref[k].shape) - ref[k]).abs() > bnd[k]).any()) for k in R.keys(c))


def _ref_bounds(c):
    if id(c) not in _DONE:
        _DONE[id(c)] = (c, R.reference(c), R.bounds(c))
    return _DONE[id(c)][1:]


def _check_case(c):
    ref, (val, bnd, margin) = _ref_bounds(c)
    _agree(ref, val, c, "chain", rel=1e-9 if c["kind"].startswith("clamp") else 1e-12)
    assert margin > 0.0, f"{_where(c)}: a scale* within its bound of the clamp ({margin:.3e})"
    _inside(R.transcription(c), ref, bnd, c, "transcription")
    return ref, bnd


def test_the_grid_is_complete():
    """five latent sizes x six group-size tuples, every ncomp of (1, 5, 7, 12, 64) in use and 64 beside n = 32"""
    pts = R.grid_points()
    assert len(pts) == 30 and len(R.standard_grid()) == 30 - len(R.OVER_CAP) and all(p in pts for p in R.OVER_CAP)
    assert set(R.GRID_B.values()) == {1, 5, 7, 12, 64} and R.grid_case(32, (130, 130))["ncomp"] == 64


@pytest.mark.parametrize("n", R.NS)
def test_standard_cases_agree_stay_inside_and_meet_the_cap(n):
    for (nn, B) in R.standard_grid():
        if nn != n:
            continue
        c = R.grid_case(n, B)
        ref, bnd = _check_case(c)
        worst = R.cap_ratios(c, ref, bnd)
        k = max(worst, key=worst.get)
        assert worst[k] <= 1.0, f"{k} {_where(c)}: bound {worst[k] * R.cap_of(k):.3e} x max|reference| over the cap {R.cap_of(k):.0e}"


@pytest.mark.parametrize("name", R.structured_names())
def test_structured_cases_agree_and_stay_inside(name):
    _check_case(R.structured_case(name))


def test_two_groups_on_a_uniform_plan_are_the_upstream_cluster_poe():
    """the tie the header of csrc/spv_poe_n.h claims, under the condition it needs (see two_group_uniform_plan_case)"""
    c = R.two_group_uniform_plan_case()
    code = [torch.as_tensor(k) for k in R.codes_of(c)]
    assert torch.equal(code[0], code[1]) and len(torch.unique(code[0])) == c["ncomp"]
    plan = 0.37 * (code[0][:, None] == code[1][None, :]).double() + 0.11     # uniform inside a component; outside it the plan is masked off
    sh = [dict(logtheta_loc=c["loc"][g].double(), logtheta_logvar=c["logvar"][g].double(), logtheta_scale=torch.exp(0.5 * c["logvar"][g].double()))
          for g in (0, 1)]
    up = O.poe_cluster(sh[0], sh[1], plan, code[0], code[1])
    ref = R.reference(c)
    got = {f"{k}{g}": up[g][f"logtheta_{k}"] for g in (0, 1) for k in ("loc", "logvar", "scale")}
    _agree(ref, got, c, "oracle.poe_cluster", keys=sorted(got))


# ==== (d) the structures are what their names say ===========================================================================================
def _counts(c):
    """[g][code] cells of every group per component"""
    return [np.bincount(k[k >= 0], minlength=c["ncomp"]) for k in R.codes_of(c)]


def test_structured_cases_reach_their_branches():
    c = R.structured_case("absent")
    n = np.stack(_counts(c))
    assert int((n == 0).sum()) >= 6 and (n[:, 4] > 0).tolist() == [False, True, False] and n[1, 0] == 0 and n[2, 3] == 0
    c = R.structured_case("disjoint")
    n = np.stack(_counts(c))
    assert not ((n[2] > 0) & ((n[0] > 0) | (n[1] > 0))).any() and ((n[0] > 0) & (n[1] > 0)).sum() == 5
    c = R.structured_case("bad_codes")
    bad = [np.nonzero(k < 0)[0].tolist() for k in R.codes_of(c)]
    assert bad == [list(R.BAD_CELLS[0]), [], list(R.BAD_CELLS[2])]
    stored = torch.cat([c["comp"][g][list(R.BAD_CELLS[g])] for g in (0, 2)])
    assert int(torch.isnan(stored).sum()) == 2 and set(stored[~torch.isnan(stored)].tolist()) == {-1.0, 4.0, 1000.0}
    assert all(c["coef"][g][k] is not None for g in range(3) for k in R.DIFF)
    for name in ("clamp", "clamp-kl_logz"):
        c = R.structured_case(name)
        ref = R.reference(c)
        for g in range(c["NG"]):
            tiny = ref[f"scale{g}"] < 5e-7      # (scale* = 3e-7 exp(N / 4) on the clamp cells: 97 % of them below 5e-7, all below 1e-6)
            assert float(tiny[::2].double().mean()) > 0.9 and bool((ref[f"scale{g}"][::2] < 1e-6).all()) and not bool(tiny[1::2].any()), (name, g)
    c = R.structured_case("partial_grads-group1_unused")
    assert all(v is None for v in c["coef"][1].values()) and float(R.reference(c)["dloc1"].abs().max()) > 0
    c = R.structured_case("partial_grads-only_loc0")
    assert [k for g in range(3) for k, v in c["coef"][g].items() if v is not None] == ["loc"] and c["coef"][0]["loc"] is not None
    for name in ("partial_grads-kl_logz", "partial_grads-kl_logz-4"):
        c = R.structured_case(name)
        assert all(sorted(k for k, v in d.items() if v is not None) == ["kl", "logz"] for d in c["coef"])
    c = R.structured_case("one_component")
    assert c["NG"] == 4 and c["ncomp"] == 1 and all(int(n[0]) == b for n, b in zip(_counts(c), c["B"]))
    c = R.structured_case("edge_code")
    assert c["ncomp"] == 64 and all(n[63] > 0 and n[0] == 0 for n in _counts(c))
    assert R.structured_case("lopsided")["B"] == (300, 17, 64, 9)
    assert max(R.cap_ratios(R.structured_case("lopsided")).values()) > 1.0      # why it is no standard case


def test_a_disjoint_group_is_alone_and_unseen():
    """group 2 of ``disjoint`` shares no code: it is prior + own expert only, and groups 0, 1 are the two-group problem without it"""
    c = R.structured_case("disjoint")
    ref = R.reference(c)
    two = R.reference(R.sub_case(c, (0, 1)))
    for k, v in two.items():
        assert torch.equal(ref[k], v), k
    loc, lv = c["loc"][2].double(), c["logvar"][2].double()
    prec = 1.0 + torch.exp(-lv)
    assert torch.allclose(ref["loc2"], loc * torch.exp(-lv) / prec, rtol=1e-14, atol=0) and torch.allclose(ref["logvar2"], -torch.log(prec), rtol=1e-14, atol=1e-16)


def test_a_cell_without_a_code_has_its_own_gradient_only():
    """``bad_codes``: such a cell is the one-group problem of itself (prior + own expert) and adds to nobody's gradient: the others'
    values and gradients are those of the problem without these cells"""
    c = R.structured_case("bad_codes")
    ref = R.reference(c)
    keep = [torch.as_tensor(k >= 0) for k in R.codes_of(c)]
    cut = dict(c, B=tuple(int(k.sum()) for k in keep))
    for key in ("loc", "logvar", "eps", "comp"):
        cut[key] = [t[k] for t, k in zip(c[key], keep)]
    cut["coef"] = [{name: v[k] for name, v in d.items()} for d, k in zip(c["coef"], keep)]
    without = R.reference(cut)
    for k in R.keys(c):
        g = int(k[-1])
        assert torch.allclose(ref[k][keep[g]], without[k], rtol=1e-13, atol=1e-15), k
    for g in (0, 2):
        out = ~keep[g]
        loc = c["loc"][g][out].double().requires_grad_(True)
        lv = c["logvar"][g][out].double().requires_grad_(True)
        prec = 1.0 + torch.exp(-lv)
        jl, jv = loc * torch.exp(-lv) / prec, -torch.log(prec)
        sq = torch.exp(0.5 * jv)
        z = jl + sq * c["eps"][g][out].double()
        kl = (0.5 * (sq * sq + jl * jl - 1.0 - torch.log(sq * sq))).sum(1)
        w = {k: v[out].double() for k, v in c["coef"][g].items()}
        L = (w["loc"] * jl).sum() + (w["logvar"] * jv).sum() + (w["scale"] * sq).sum() + (w["logz"] * z).sum() + (w["kl"] * kl).sum()
        dl, dv = torch.autograd.grad(L, (loc, lv))
        assert torch.allclose(ref[f"dloc{g}"][out], dl, rtol=1e-13, atol=1e-15) and torch.allclose(ref[f"dlogvar{g}"][out], dv, rtol=1e-13, atol=1e-15)


# ==== (e) the bounds bite ======================================================================================================================
MUTATION_CASES = {
    "include_self": ("absent", "one_component", "edge_code"),
    "absent_as_unit": ("absent", "disjoint"),
    "drop_gk_jl": ("partial_grads-kl_logz", "bad_codes", "lopsided"),
    "no_live": ("clamp", "clamp-kl_logz"),
    "apply_no_div": ("one_component", "partial_grads-only_loc0", "lopsided"),
    "skip_last_group": ("absent", "partial_grads-group1_unused", "edge_code"),
    "seg_tail": ("lopsided", "partial_grads-kl_logz-4", "disjoint"),
    "j_from_prec_sign": ("bad_codes", "partial_grads-only_loc0", "clamp"),
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutations_of_the_transcription_fall_outside_the_bounds(mut):
    for name in MUTATION_CASES[mut]:
        c = R.structured_case(name)
        ref, (_, bnd, _) = _ref_bounds(c)
        _inside(R.transcription(c), ref, bnd, c, "transcription")
        assert _outside(R.transcription(c, mut), ref, bnd, c), f"{mut} on {name}: still inside the bounds"
