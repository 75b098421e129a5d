"""GPU: the N-group component PoE (csrc/spv_poe_n.h: pn_stats, pn_means, pn_fuse_fwd, pn_cell_bwd, pn_comp_bwd, pn_apply_bwd) through
nn_ops.PoEComponents ``.apply`` and ``.backward()``, as module.py drives them, against the float64 autograd definition of
tests/_poe_n_reference.py.

Every output (loc*, logvar*, scale*, log_z, theta, kl) and both input gradients of every group are held to reference +- the bound DERIVED
in the module docstring of tests/_poe_n_reference.py (the kernels' roundings times 2^-24 in running-error form, the two-stage reductions
included); no tolerance is picked here.  tests/test_poe_n_reference_cpu.py shows that a float32 transcription stays inside those bounds,
that on the standard cases they are at most 2e-5 (forward) and 1e-4 (gradients) of the output's largest value, and that eight deliberate
mistakes fall outside them.  Everything else is bit equality: the kernels use no atomics, so two calls, a wide row pitch, a shared
workspace and a third group without a common code must not move a bit, and through the C ABI nothing may land outside the outputs.
Shapes: a few hundred cells at most per case (tests/_poe_n_reference.py: GRID_B, STRUCTURED).
Largest error / bound measured on the MI355X: logvar* 0.97 (clamp cases, logvar* ~ -30; 0.66 elsewhere), every other output and both
gradients at most 0.39 (docs/lab_notes.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _poe_n_reference as R

pytestmark = pytest.mark.gpu

SENT = -7.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from spvipes_amd import ops
    return ops.Workspace(dev)


_REF = {}


def ref_of(c):
    """(reference, bounds) of a case, computed once"""
    if id(c) not in _REF:
        _, bnd, margin = R.bounds(c)
        assert margin > 0.0
        _REF[id(c)] = (c, R.reference(c), bnd)
    return _REF[id(c)][1:]


def forward(c, dev, ws, pitch: int = 0):
    """PoEComponents.apply on the case -> (outputs on the device keyed like the reference plus qscale, the loss, the leaves).
    pitch > 0: loc / logvar are the adjacent views buf[:, :n], buf[:, n:2n] of a [B][2n + pitch] buffer (the no-copy path)."""
    from spvipes_amd.nn_ops import PoEComponents
    n, NG = c["n"], c["NG"]
    leaves, stats = [], []
    for g in range(NG):
        if pitch:
            buf = torch.cat([c["loc"][g], c["logvar"][g], torch.full((c["B"][g], pitch), 3.25)], 1).to(dev).requires_grad_(True)
            leaves.append(buf)
            stats += [buf[:, :n], buf[:, n:2 * n]]
        else:
            lv = [c[k][g].to(dev).requires_grad_(True) for k in ("loc", "logvar")]
            leaves += lv
            stats += lv
    o = PoEComponents.apply([k.to(dev) for k in c["comp"]], c["ncomp"], [e.to(dev) for e in c["eps"]], ws, *stats)
    res, L = {}, None
    for g in range(NG):
        for j, k in enumerate(R.OUT):
            res[f"{k}{g}"] = o[7 * g + j]
        res[f"qscale{g}"] = o[7 * g + 6]
        for k in R.DIFF:
            w = c["coef"][g][k]
            if w is not None:
                t = (w.to(dev) * res[f"{k}{g}"]).sum()
                L = t if L is None else L + t
    return res, L, leaves


def finish(c, res, L, leaves, pitch: int = 0, backward: bool = True) -> dict:
    n = c["n"]
    if backward:
        L.backward()
        for g in range(c["NG"]):
            if pitch:
                gr = leaves[g].grad
                res[f"dloc{g}"], res[f"dlogvar{g}"], res[f"dpad{g}"] = gr[:, :n], gr[:, n:2 * n], gr[:, 2 * n:]
            else:
                res[f"dloc{g}"], res[f"dlogvar{g}"] = leaves[2 * g].grad, leaves[2 * g + 1].grad
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}


def run_case(c, dev, ws, pitch: int = 0, backward: bool = True) -> dict:
    """the case through the autograd Function; fp32 CPU tensors keyed like the reference, plus qscale (and dpad under a pitch)"""
    return finish(c, *forward(c, dev, ws, pitch), pitch=pitch, backward=backward)


def _where(c):
    return f"({c['kind']}, n {c['n']}, B {c['B']}, ncomp {c['ncomp']})"


def ratios(got, c) -> dict:
    """per output the largest error / bound (0 / 0 = 0)"""
    ref, bnd = ref_of(c)
    out = {}
    for k in R.keys(c):
        err = (got[k].double().reshape(ref[k].shape) - ref[k]).abs()
        out[k] = float(torch.where(err > 0, err / bnd[k], torch.zeros_like(err)).max())
    return out


def hold(got, c):
    ref, bnd = ref_of(c)
    for k in R.keys(c):
        g = got[k].double().reshape(ref[k].shape)
        assert bool(torch.isfinite(g).all()), f"{k} {_where(c)}: not finite"
        err = (g - ref[k]).abs()
        over = err > bnd[k]
        if bool(over.any()):
            i = int(torch.argmax((err - bnd[k]).flatten()))
            raise AssertionError(f"{k} {_where(c)}: {int(over.sum())} of {over.numel()} over the bound; worst at flat index {i}: "
                                 f"got {g.flatten()[i]:.9g} ref {ref[k].flatten()[i]:.9g} error {err.flatten()[i]:.3e} "
                                 f"bound {bnd[k].flatten()[i]:.3e}")


def qscale_is_the_clamp(got, c):
    """the scale of the reference's Normal: the fp32 clamp of the stored scale*, 1e-6f where the reference scale is below 5e-7"""
    ref, _ = ref_of(c)
    for g in range(c["NG"]):
        assert torch.equal(got[f"qscale{g}"], got[f"scale{g}"].clamp(min=1e-6)), f"qscale{g} {_where(c)}"
        tiny = ref[f"scale{g}"] < 5e-7
        assert bool((got[f"qscale{g}"][tiny] == float(np.float32(1e-6))).all()), f"qscale{g} {_where(c)}"


def same_bits(a, b, keys, what, rename=lambda k: k):
    for k in keys:
        assert torch.equal(a[k].contiguous().view(torch.int32), b[rename(k)].contiguous().view(torch.int32)), f"{what}: {k} differs"


# ==== the standard grid =====================================================================================================================
@pytest.mark.parametrize("n", R.NS)
def test_standard_cases_within_the_bounds(dev, ws, n):
    for (nn, B) in R.standard_grid():
        if nn != n:
            continue
        c = R.grid_case(n, B)
        got = run_case(c, dev, ws)
        hold(got, c)
        qscale_is_the_clamp(got, c)


# ==== the structured cases (and the grid points over the cap) ================================================================================
@pytest.mark.parametrize("name", R.structured_names())
def test_structured_cases_within_the_bounds(dev, ws, name):
    c = R.structured_case(name)
    got = run_case(c, dev, ws)
    hold(got, c)
    qscale_is_the_clamp(got, c)
    ref, _ = ref_of(c)
    if c["kind"].startswith("clamp"):
        assert all(int((ref[f"scale{g}"] < 5e-7).sum()) > 0.45 * ref[f"scale{g}"].numel() for g in range(c["NG"]))
    for g in range(c["NG"]):   # partial gradients: a group none of whose outputs is used still receives the others' through its means
        if all(v is None for v in c["coef"][g].values()) and float(ref[f"dloc{g}"].abs().max()) > 0:
            assert float(got[f"dloc{g}"].abs().max()) > 0 and float(got[f"dlogvar{g}"].abs().max()) > 0


def test_a_disjoint_third_group_moves_no_bit_of_the_others(dev, ws):
    """group 2 of ``disjoint`` shares no code with groups 0 and 1: every output and gradient of those two has the bits of the two-group
    problem without it (its cells are skipped inside the same fixed-order reductions)"""
    c = R.structured_case("disjoint")
    three, two = run_case(c, dev, ws), run_case(R.sub_case(c, (0, 1)), dev, ws)
    same_bits(two, three, sorted(two), "groups 0, 1 beside a disjoint group")


# ==== bit-level properties ===================================================================================================================
@pytest.mark.parametrize("name", ["lopsided", "absent", "clamp"])
def test_repeated_calls_give_the_same_bits(dev, ws, name):
    c = R.structured_case(name)
    a, b = run_case(c, dev, ws), run_case(c, dev, ws)
    same_bits(a, b, R.keys(c), f"{name} twice")    # no atomics: forward AND backward


@pytest.mark.parametrize("name", ["lopsided", "bad_codes", "edge_code"])
def test_wide_pitch_views_give_the_same_bits(dev, ws, name):
    c = R.structured_case(name)
    a, b = run_case(c, dev, ws), run_case(c, dev, ws, pitch=5)
    same_bits(a, b, R.keys(c), f"{name} pitch 2n + 5")
    for g in range(c["NG"]):
        assert b[f"dpad{g}"].shape == (c["B"][g], 5) and float(b[f"dpad{g}"].abs().max()) == 0.0, "gradient in the columns beyond 2n"


# from the largest ``poen_part`` to the smallest; clamp and partial_grads-kl_logz have one shape, the others differ in NG, n and ncomp
SHARED = ("edge_code", "lopsided", "clamp", "partial_grads-kl_logz", "partial_grads-only_loc0", "one_component")


@pytest.mark.parametrize("order", ["large_then_small", "small_then_large"])
def test_a_shared_workspace_leaks_nothing(dev, order):
    """one Workspace across cases of different NG, n and ncomp, in both orders, with the forwards of two cases queued before either
    backward: a stale ``poen_part`` must not reach a result -- the bits are a fresh workspace's"""
    from spvipes_amd import ops
    names = SHARED if order == "large_then_small" else SHARED[::-1]
    fresh = {k: run_case(R.structured_case(k), dev, ops.Workspace(dev)) for k in names}
    shared = ops.Workspace(dev)
    for a, b in zip(names[0::2], names[1::2]):
        ca, cb = R.structured_case(a), R.structured_case(b)
        fa, fb = forward(ca, dev, shared), forward(cb, dev, shared)
        ga, gb = finish(ca, *fa), finish(cb, *fb)
        same_bits(fresh[a], ga, R.keys(ca), f"{a} before {b} in a shared workspace")
        same_bits(fresh[b], gb, R.keys(cb), f"{b} after {a} in a shared workspace")
    for k in names:
        same_bits(fresh[k], run_case(R.structured_case(k), dev, shared), R.keys(R.structured_case(k)), f"{k} in a used workspace")


# ==== canaries through the C ABI =============================================================================================================
def _canary(dev, numel, margin=256):
    buf = torch.full((numel + 2 * margin,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[margin:margin + numel]


def _framed_ok(buf, view, name):
    numel, margin = view.numel(), (buf.numel() - view.numel()) // 2
    out = buf.cpu()
    assert bool((out[:margin] == SENT).all()) and bool((out[margin + numel:] == SENT).all()), f"{name}: written outside its extent"
    return out[margin:margin + numel]


_CANARY = {}


def canary_case(n, B, ncomp):
    if (n, B) not in _CANARY:
        _CANARY[n, B] = R.make_case(n, ncomp, B, kind="canary")
    return _CANARY[n, B]


@pytest.mark.parametrize("n,B,ncomp,pad", [(31, (70, 9, 33), 7, 0), (10, (9, 70), 5, 3)])
def test_nothing_is_written_outside_the_outputs(dev, ws, n, B, ncomp, pad):
    """spv_poe_comp_fwd / _bwd through the C ABI with every output, dpn, d_stats, part and mean in sentinel-framed allocations (stats and
    d_stats at a row pitch of 2n + pad): the grids are sized by the largest group and rounded up to 8 cells of 32 lanes, and nothing may
    land outside [B][n] (kl: [B]; dpn: [B][2n]; d_stats: columns below 2n); inside, the values are the autograd path's bits"""
    from spvipes_amd import _abi
    from spvipes_amd._abi import POE_COMP_SEG, ptr, stream_ptr
    c = canary_case(n, B, ncomp)
    want = run_case(c, dev, ws)
    hold(want, c)
    NG, W, ld = len(B), 2 * n + 1, 2 * n + pad
    a = _abi.SpvPoeCompArgs()
    a.ngroups, a.n, a.ncomp = NG, n, ncomp
    frames = {"part": _canary(dev, NG * POE_COMP_SEG * ncomp * W), "mean": _canary(dev, NG * ncomp * W)}
    a.part, a.mean = ptr(frames["part"][1]), ptr(frames["mean"][1])
    hold_on = []
    for g, Bg in enumerate(B):
        stats = torch.cat([c["loc"][g], c["logvar"][g], torch.full((Bg, pad), 3.25)], 1).contiguous().to(dev)
        eps, comp = c["eps"][g].contiguous().to(dev), c["comp"][g].contiguous().to(dev)
        grads = [None if c["coef"][g][k] is None else c["coef"][g][k].contiguous().to(dev) for k in R.DIFF]
        hold_on += [stats, eps, comp, grads]
        a.stats[g], a.ld[g], a.eps[g], a.comp[g], a.B[g] = ptr(stats), ld, ptr(eps), ptr(comp), Bg
        a.g_loc[g], a.g_logvar[g], a.g_scale[g], a.g_logz[g], a.g_kl[g] = (ptr(t) for t in grads)
        for k in R.OUT:
            frames[k, g] = _canary(dev, Bg if k == "kl" else Bg * n)
        frames["dpn", g], frames["d_stats", g] = _canary(dev, Bg * 2 * n), _canary(dev, Bg * ld)
        a.loc[g], a.logvar[g], a.scale[g], a.logz[g], a.theta[g], a.kl[g] = (ptr(frames[k, g][1]) for k in R.OUT)
        a.dpn[g], a.d_stats[g] = ptr(frames["dpn", g][1]), ptr(frames["d_stats", g][1])
    _abi.call("spv_poe_comp_fwd", C.byref(a), stream_ptr())
    _abi.call("spv_poe_comp_bwd", C.byref(a), stream_ptr())
    torch.cuda.synchronize()
    for key, (buf, view) in frames.items():
        inner = _framed_ok(buf, view, key)
        if key in ("part", "mean"):
            continue
        k, g = key
        if k in R.OUT:
            assert torch.equal(inner.view(torch.int32), want[f"{k}{g}"].reshape(-1).view(torch.int32)), f"{k}{g}"
        elif k == "d_stats":
            d = inner.view(B[g], ld)
            assert bool((d[:, 2 * n:] == SENT).all()), f"d_stats{g}: written into the columns at or beyond 2n"
            assert torch.equal(d[:, :n].contiguous().view(torch.int32), want[f"dloc{g}"].view(torch.int32)), f"dloc{g}"
            assert torch.equal(d[:, n:2 * n].contiguous().view(torch.int32), want[f"dlogvar{g}"].view(torch.int32)), f"dlogvar{g}"
