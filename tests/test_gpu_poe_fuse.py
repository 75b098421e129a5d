"""GPU: the two-group PoE fusion (csrc/spv_small.h poe_fuse_fwd_kernel, poe_fuse_bwd_kernel<AGG>; for the cluster pairing also
plan_expert_fwd / _bwd) through nn_ops.PoELabel / PoEPaired / PoECluster ``.apply`` and ``.backward()``, as the module calls them, against
the float64 definition of tests/_poe_reference.py.

Every output (loc*, logvar*, scale*, log_z, theta, kl) and both input gradients are held to reference +- the bound DERIVED in the module
docstring of tests/_poe_reference.py (the kernel's roundings times 2^-24 in running-error form); no tolerance is picked here.
tests/test_poe_reference_cpu.py shows that a float32 transcription stays inside those bounds, that on the standard cases they are at
most 2e-5 (forward) and 1e-4 (gradients) of the output's largest value, and that five deliberate mistakes fall outside them.
Pairings (partner, mode) are exact and compared with oracle.label_partner; the forward of all three pairings and the label backward are
bit-reproducible (a label pair adds at most twice per element); the paired and cluster backward use atomics and are only held to the bound.
Shapes: a few hundred cells at most per case (tests/_poe_reference.py: standard_grid, STRUCTURED)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _poe_reference as R

pytestmark = pytest.mark.gpu

SENT = -7.5
KEYS = R.FWD_KEYS + R.GRAD_KEYS


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
        assert margin is None or margin > 0.0
        _REF[id(c)] = (c, R.reference(c), bnd)
    return _REF[id(c)][1:]


def sparse_plan(c, dev):
    import scipy.sparse as sp
    from spvipes_amd.plan import SparsePlan
    return SparsePlan.from_scipy(sp.csr_matrix(c["plan"]), dev)


def run_case(c, dev, ws, pitch: int = 0, backward: bool = True) -> dict:
    """the case through the pairing's autograd Function; fp32 CPU tensors keyed like the reference, plus qscale / partner / mode.
    pitch > 0: loc / logvar are the adjacent views buf[:, :n], buf[:, n:2n] of a [B][2n + pitch] buffer (the no-copy path)."""
    from spvipes_amd.nn_ops import PoECluster, PoELabel, PoEPaired, label_partners
    n = c["n"]
    leaves, stats = [], []
    for g in (0, 1):
        if pitch:
            buf = torch.cat([c["loc"][g], c["logvar"][g], torch.full((c["B"][g], pitch), 3.25)], 1).to(dev).requires_grad_(True)
            leaves.append(buf)
            stats += [buf[:, :n], buf[:, n:2 * n]]
        else:
            lv = [c[k][g].to(dev).requires_grad_(True) for k in ("loc", "logvar")]
            leaves += lv
            stats += lv
    eps = [e.to(dev) for e in c["eps"]]
    res = {}
    if c["pairing"] == "label":
        pre = label_partners([l.to(dev).float() for l in c["labels"]], ws)
        o = PoELabel.apply([l.to(dev).float() for l in c["labels"]], eps, ws, pre, *stats)
        stride = 6
        res.update(partner0=pre[0][0], partner1=pre[0][1], mode0=pre[1][0], mode1=pre[1][1])
    else:
        idx = [i.to(dev) for i in c["idx"]]
        if c["pairing"] == "paired":
            o = PoEPaired.apply(sparse_plan(c, dev), idx, eps, ws, *stats)
        else:
            o = PoECluster.apply(sparse_plan(c, dev), idx, [x.to(dev) for x in c["comp"]], eps, ws, *stats)
        stride = 7
    L = None
    for g in (0, 1):
        for j, k in enumerate(R.OUT):
            res[f"{k}{g}"] = o[stride * g + j]
        if stride == 7:
            res[f"qscale{g}"] = o[7 * g + 6]
        for k in R.DIFF:
            w = c["coef"][g][k]
            if w is not None:
                t = (w.to(dev) * res[f"{k}{g}"]).sum()
                L = t if L is None else L + t
    if backward:
        L.backward()
        for g in (0, 1):
            if pitch:
                gr = leaves[g].grad
                res[f"dloc{g}"], res[f"dlogvar{g}"], res[f"dpad{g}"] = gr[:, :n], gr[:, n:2 * n], gr[:, 2 * n:]
            else:
                res[f"dloc{g}"], res[f"dlogvar{g}"] = leaves[2 * g].grad, leaves[2 * g + 1].grad
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in res.items()}


def _where(c):
    return f"({c['pairing']}, n {c['n']}, B {c['B']}, {c['kind']})"


def ratios(got, ref, bnd, keys=KEYS) -> dict:
    """per output the largest error / bound (0 / 0 = 0)"""
    out = {}
    for k in keys:
        err = (got[k].double().reshape(ref[k].shape) - ref[k]).abs()
        out[k] = float(torch.where(err > 0, err / bnd[k], torch.zeros_like(err)).max())
    return out


def hold(got, c, keys=KEYS):
    ref, bnd = ref_of(c)
    for k in keys:
        g = got[k].double().reshape(ref[k].shape)
        assert bool(torch.isfinite(g).all()), f"{k} {_where(c)}: not finite"
        err = (g - ref[k]).abs()
        over = err > bnd[k]
        if bool(over.any()):
            i = int(torch.argmax((err - bnd[k]).flatten()))
            raise AssertionError(f"{k} {_where(c)}: {int(over.sum())} of {over.numel()} over the bound; worst at flat index {i}: "
                                 f"got {g.flatten()[i]:.9g} ref {ref[k].flatten()[i]:.9g} error {err.flatten()[i]:.3e} "
                                 f"bound {bnd[k].flatten()[i]:.3e}")


def pairing_is_the_oracles(got, c):
    S = R.structure(c)
    for g in (0, 1):
        assert np.array_equal(got[f"partner{g}"].numpy(), S["partner"][g]) and np.array_equal(got[f"mode{g}"].numpy(), S["mode"][g]), _where(c)


def same_bits(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), f"{what}: {k} differs"


# ==== the standard grid =====================================================================================================================
@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("pairing", ("label", "paired", "cluster"))
def test_standard_cases_within_the_bounds(dev, ws, pairing, n):
    for (nn, B0, B1) in R.standard_grid(pairing):
        if nn != n:
            continue
        c = R.standard_case(pairing, n, B0, B1)
        got = run_case(c, dev, ws)
        hold(got, c)
        if pairing == "label":
            pairing_is_the_oracles(got, c)


# ==== the structured cases ==================================================================================================================
@pytest.mark.parametrize("name", sorted(R.STRUCTURED))
def test_structured_cases_within_the_bounds(dev, ws, name):
    c = R.structured_case(name)
    got = run_case(c, dev, ws)
    hold(got, c)
    ref, _ = ref_of(c)
    if c["pairing"] == "label":
        pairing_is_the_oracles(got, c)
    else:
        for g in (0, 1):   # the scale of the reference's Normal: the fp32 clamp of the stored scale*, 1e-6f below it
            assert torch.equal(got[f"qscale{g}"], got[f"scale{g}"].clamp(min=1e-6))
            tiny = ref[f"scale{g}"] < 5e-7
            assert bool((got[f"qscale{g}"][tiny] == float(np.float32(1e-6))).all())
            if c["kind"] == "clamp":
                assert int(tiny.sum()) > tiny.numel() // 2
    use = R.STRUCTURED[name][5]
    if use is not None:   # partial gradients: a group none of whose outputs is used still receives its partner's gradient
        for g in (0, 1):
            if all(gg != g for _, gg in use) and float(ref[f"dloc{g}"].abs().max()) > 0:
                assert float(got[f"dloc{g}"].abs().max()) > 0 and float(got[f"dlogvar{g}"].abs().max()) > 0


# ==== pitch: adjacent views of a wider buffer =================================================================================================
@pytest.mark.parametrize("name", ["label-more_on_0", "paired-shared_ws", "cluster-lone"])
def test_wide_pitch_views_give_the_same_bits(dev, ws, name):
    c = R.structured_case(name)
    a, b = run_case(c, dev, ws), run_case(c, dev, ws, pitch=5)
    same_bits(a, b, R.FWD_KEYS, f"{name} pitch 2n + 5")
    if c["pairing"] == "label":
        same_bits(a, b, R.GRAD_KEYS, f"{name} pitch 2n + 5")
    hold(b, c)
    for g in (0, 1):
        assert float(b[f"dpad{g}"].abs().max()) == 0.0, "gradient written into the columns beyond 2n"


# ==== bit-level properties ===================================================================================================================
@pytest.mark.parametrize("name", ["label-codes_edge", "paired-mostly_empty", "cluster-unequal"])
def test_repeated_calls_give_the_same_bits(dev, ws, name):
    c = R.structured_case(name)
    a, b = run_case(c, dev, ws), run_case(c, dev, ws)
    same_bits(a, b, R.FWD_KEYS, f"{name} forward twice")
    if c["pairing"] == "label":   # at most two adds per element: order-independent.  (paired / cluster: atomics, no such claim)
        same_bits(a, b, R.GRAD_KEYS, f"{name} backward twice")


def _canary(dev, numel, margin=256):
    buf = torch.full((numel + 2 * margin,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[margin:margin + numel]


@pytest.mark.parametrize("pairing,n,B0,B1", [("label", 10, 9, 70), ("label", 31, 70, 9), ("paired", 25, 33, 33)])
def test_forward_writes_nothing_outside_its_outputs(dev, ws, pairing, n, B0, B1):
    """spv_poe_fuse_fwd through the C ABI into canary-framed allocations: the grid is sized by the larger group and rounded up to 8 cells
    of 32 lanes, and nothing may land outside [B][n] (kl: [B]) of either group; inside, the values are those of the autograd path"""
    from spvipes_amd import _abi
    from spvipes_amd._abi import ptr, stream_ptr
    from spvipes_amd.nn_ops import label_partners
    c = R.standard_case(pairing, n, B0, B1)
    want = run_case(c, dev, ws, backward=False)
    a = _abi.SpvPoeArgs()
    a.n, a.clamp_scale, a.lone_passthrough = n, int(pairing != "label"), 0
    hold_on, frames = [], {}
    if pairing == "label":
        partner, mode, lab, order, rank, tables = label_partners([l.to(dev).float() for l in c["labels"]], ws)
        a.tables = ptr(tables)
    else:
        S = R.structure(c)
        partner = [torch.as_tensor(S["partner"][g], dtype=torch.int32).to(dev) for g in (0, 1)]
        mode = [torch.zeros(c["B"][g], dtype=torch.int32, device=dev) for g in (0, 1)]
    for g, B in enumerate(c["B"]):
        stats = torch.cat([c["loc"][g], c["logvar"][g]], 1).contiguous().to(dev)
        eps = c["eps"][g].contiguous().to(dev)
        hold_on += [stats, eps]
        a.stats[g], a.ld[g], a.eps[g], a.B[g], a.partner[g], a.mode[g] = ptr(stats), 2 * n, ptr(eps), B, ptr(partner[g]), ptr(mode[g])
        if pairing == "label":
            a.lab[g], a.order[g], a.rank[g] = ptr(lab[g]), ptr(order[g]), ptr(rank[g])
        for k in R.OUT:
            frames[k, g] = _canary(dev, B if k == "kl" else B * n)
        a.loc[g], a.logvar[g], a.scale[g], a.logz[g], a.theta[g], a.kl[g] = (ptr(frames[k, g][1]) for k in R.OUT)
    _abi.call("spv_poe_fuse_fwd", C.byref(a), stream_ptr())
    torch.cuda.synchronize()
    for (k, g), (buf, view) in frames.items():
        numel, margin = view.numel(), (buf.numel() - view.numel()) // 2
        out = buf.cpu()
        assert bool((out[:margin] == SENT).all()) and bool((out[margin + numel:] == SENT).all()), f"{k}{g}: written outside its extent"
        assert torch.equal(out[margin:margin + numel].view(torch.int32), want[f"{k}{g}"].reshape(-1).view(torch.int32)), f"{k}{g}"
