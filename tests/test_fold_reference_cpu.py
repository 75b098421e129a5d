"""No GPU: the float64 reference and the derived bounds of tests/_fold_reference.py check themselves.
  (a) the reference IS BatchNorm1d: forward and autograd equal torch.nn.BatchNorm1d(eps=1e-3).double() applied to z W^T (+ b);
  (b) a numpy-float32 transcription of the kernels' formulas stays inside the derived bounds on every case of the GPU grid -- the bounds
      hold for a correct implementation;
  (c) on every STANDARD case (latent column means within one standard deviation of zero, spread 1, |w| ~ 1 / sqrt(K)) each output's bound
      is at most 1e-3 x max|reference| of that output tensor -- the bounds cannot hide a failure.  Computed from the reference alone.
      Batches of one or two cells have no spread to speak of (B = 1: every variance is exactly zero and inv = gamma / sqrt(eps)); they are
      held to (a) and (b) and to the GPU assertions, not to the cap."""
import numpy as np
import pytest
import torch

from tests import _fold_reference as R

FWD_KEYS, _bwd_keys = R.FWD_KEYS, R.bwd_keys


def _all_cases():
    out = [("fwd", K, G, B, False) for w in (False, True) for (K, G, B) in R.fwd_cases(w)]
    out += [("bwd", K, G, B, False) for w in (False, True) for (K, G, B) in R.bwd_cases(w)]
    out += [("both", K, N, B, True) for (K, N, B) in R.trunk_cases()]
    return out


def _check(name, got, ref, bound, where):
    err = (torch.as_tensor(np.asarray(got, np.float64)) - ref).abs()
    assert torch.isfinite(err).all(), (name, where)
    over = err > bound
    assert not over.any(), f"{name} {where}: error {err[over].max():.3e} over its bound {bound[over].min():.3e}"


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("trunk", [False, True])
def test_reference_is_batchnorm1d(training, trunk):
    for (K, G, B) in ((5, 7, 9), (17, 33, 2), (3, 4, 37)):
        c = R.make_case(K, G, B, trunk=trunk)
        m = R.f32(R.MOMENTUM)
        ref = R.reference(c, training, backward=True)
        bn = torch.nn.BatchNorm1d(G, eps=1e-3, momentum=m).double()
        with torch.no_grad():
            bn.weight.copy_(c["gamma"].double()); bn.bias.copy_(c["beta"].double())
            bn.running_mean.copy_(c["rm"].double()); bn.running_var.copy_(c["rv"].double())
        bn.train(training)
        z = c["z"].double().requires_grad_(True)
        W = c["W"].double().requires_grad_(True)
        b = c["bias"].double().requires_grad_(True) if trunk else None
        y = z @ W.T + (b if trunk else 0.0)
        out = bn(y)
        tol = 1e-11 * (1 + out.abs().max().item())
        assert (out - (c["z"].double() @ ref["Wf"].T + ref["cf"])).abs().max() < tol
        if training:
            assert (ref["y_mean"] - (ref["mean0"] + (c["bias"].double() if trunk else 0.0))).abs().max() < 1e-12
            assert (ref["y_var"] - ref["var"]).abs().max() < 1e-12
        assert (bn.running_mean - ref["rm"]).abs().max() < 1e-13 and (bn.running_var - ref["rv"]).abs().max() < 1e-13
        # backward: with R [B][G] the upstream gradient of the layer's output, d W' = R^T z and d c = colsum(R); the module's d z carries
        # the direct path R W' on top of the statistics path, which is what the fold's backward forms
        Rr = torch.randn(B, G, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        dWeff = torch.cat([Rr.T @ c["z"].double(), Rr.sum(0)[:, None]], 1)
        c2 = dict(c, dWeff=dWeff)
        ref = R.reference(c2, training, backward=True)
        (out * Rr).sum().backward()
        scale = lambda t: 1e-10 * (1 + t.abs().max().item())
        dW_direct = Rr.T @ c["z"].double() * ref["inv"][:, None]
        assert (bn.weight.grad - ref["dgamma"]).abs().max() < scale(ref["dgamma"])
        assert (bn.bias.grad - ref["dbeta"]).abs().max() < scale(ref["dbeta"])
        assert (W.grad - ref["dW"]).abs().max() < scale(ref["dW"]), (W.grad - dW_direct).abs().max()
        dz_stat = ref["dz"] if training else torch.zeros_like(z)
        assert (z.grad - (Rr @ ref["Wf"] + dz_stat)).abs().max() < scale(z.grad)
        if trunk:
            assert (b.grad - ref["dbias"]).abs().max() < scale(Rr.sum(0))
            if training:
                assert b.grad.abs().max() < scale(Rr.sum(0))   # the bias cancels in the batch mean


def _emulate_and_check(what, K, G, B, trunk, training, kind="standard", use_bias=True):
    c = R.standard_case(K, G, B, trunk) if kind == "standard" else R.make_case(K, G, B, kind=kind, trunk=trunk)
    zsum, zz = R.stats_f32(c["z"])
    where = (what, K, G, B, trunk, training, kind)
    ref = R.reference(c, training, use_bias=use_bias, backward=what != "fwd")
    if what in ("fwd", "both"):
        bnd = R.forward_bounds(c, ref, training, use_bias=use_bias, image=False)
        got = R.emulate_forward(c, zsum, zz, training, use_bias=use_bias)
        for k in FWD_KEYS:
            _check(k, got[k], ref[k], bnd[k], where)
        assert (got["var"] >= 0).all()
    if what in ("bwd", "both"):
        bnd = R.backward_bounds(c, ref, training, use_bias=use_bias)
        got = R.emulate_backward(c, zsum, zz, ref["mean0"].float(), ref["var"].float(), training)
        assert np.array_equal(got["dbeta"], c["dWeff"][:, K].numpy())
        for k in _bwd_keys(training, trunk):
            _check(k, got[k], ref[k], bnd[k], where)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("what", ["fwd", "bwd", "both"])
def test_float32_transcription_stays_inside_the_bounds(what, training):
    for (w, K, G, B, trunk) in _all_cases():
        if w == what:
            _emulate_and_check(what, K, G, B, trunk, training)


@pytest.mark.parametrize("kind", R.KINDS_DEGENERATE)
def test_float32_transcription_on_degenerate_inputs(kind):
    for (K, G, B) in ((15, 300, 1100), (31, 65, 37), (47, 257, 130)):
        _emulate_and_check("both", K, G, B, False, True, kind=kind)
    _emulate_and_check("both", 33, 65, 130, True, True, kind=kind)


def test_mixed_batch_cases_stay_inside_the_bounds():
    for (G, K) in R.MIXED_BATCH:
        _emulate_and_check("fwd", K, G, 37, False, True)


def test_bounds_are_capped_on_standard_cases():
    """(c): bound <= 1e-3 max|reference| per output tensor, from the reference alone"""
    worst = {}
    for (what, K, G, B, trunk) in _all_cases():
        if B < 3:
            continue   # (module docstring: no spread to speak of)
        for k, ratio in R.cap_ratios(R.standard_case(K, G, B, trunk)).items():
            worst[k] = max(worst.get(k, 0.0), ratio)
            assert ratio <= R.CAP, f"{k} ({what}, K {K}, G {G}, B {B}, trunk {trunk}): bound / max|ref| = {ratio:.2e}"
    print("largest bound / max|reference| per output:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_split_bf16_transcription():
    v = torch.tensor([0.0, 1.0, -1.0, 1.00390625, 1.005859375, 3.14159274, -2.5e-3, 1e-20], dtype=torch.float32)
    hi, lo = R.split_bf16(v)
    assert hi[1].item() == 0x3F80 and lo[1].item() == 0 and hi[0].item() == 0
    assert hi[3].item() == 0x3F80          # 1 + 2^-8: a tie, to even (down)
    assert hi[4].item() == 0x3F81          # 1 + 1.5 * 2^-8: up
    val = R.bf16_value(hi) + R.bf16_value(lo)
    assert ((val - v.double()).abs() <= R.SPLIT * v.double().abs()).all()
    assert (R.bf16_value(lo).abs() <= R.bf16_ulp(hi) / 2).all()
    # hi = bf16(hi + lo) holds for a correct split except where lo rounded up to exactly half an ulp of hi (the sum is then a tie)
    w = torch.randn(1 << 20, generator=torch.Generator().manual_seed(3))
    hi, lo = R.split_bf16(w)
    vh, vl = R.bf16_value(hi), R.bf16_value(lo)
    differs = (vh + vl).float().to(torch.bfloat16).double() != vh
    assert differs.any() and (vl.abs()[differs] == R.bf16_ulp(hi)[differs] / 2).all()
