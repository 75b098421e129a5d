"""GPU: DecoderFused decides its schedule ONCE, in forward (ops.dec_schedule), and carries it to its backward pass on ``ctx``.  The
process-global "small step" flag (ops.set_step_shape: set by every spVIPESmodule forward) may change between a step's forward and its
backward -- a validation pass, a read-out, a second model of another shape -- and must not move the backward's launch list or a bit of a
gradient (module/spVIPESmodule.py:733-824 and its backward)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, GS, H, N_S, N_P, CELLS = 128, (300, 280), 32, 10, 5, 512


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _step(dev, monkeypatch, small_elems, between, precision="bf16"):
    """one training forward and backward from seed 0 with the "small step" threshold ``small_elems`` during forward; ``between(module,
    inference outputs, generative outputs)`` runs after the forward and before the backward.  Returns (entry points the backward called, in
    order; every parameter's gradient; every BatchNorm buffer)"""
    from spvipes_amd import _abi, ops
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    groups = [make_synthetic_group(g, CELLS, GS[g], dev) for g in range(2)]
    module = spVIPESmodule({0: GS[0], 1: GS[1]}, use_labels=True, n_hidden=H, n_dimensions_shared=N_S, n_dimensions_private=N_P,
                           dropout_rate=0.0, precision=precision).to(dev)
    trainer = Trainer(module, [g.counts for g in groups], labels=[g.labels for g in groups])
    module.train()
    rows = [torch.tensor(rng.permutation(CELLS)[:B], dtype=torch.int32, device=dev) for _ in range(2)]
    gen = torch.Generator().manual_seed(1)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen).to(dev) for g in range(2) for k, n in (("private", N_P), ("shared", N_S))}
    noise.update({f"poe_{g}": torch.randn(B, N_S, generator=gen).to(dev) for g in range(2)})
    with monkeypatch.context() as mp:
        mp.setattr(ops, "SMALL_STEP_ELEMS", small_elems)
        inf, gen, lo = module(trainer.minibatch(rows), inference_kwargs={"noise": noise}, loss_kwargs={"kl_weight": 1.0})
    trainer.fp.grad.zero_()
    between(module, inf, gen)
    names, call = [], _abi.call

    def spy(name, *a):
        names.append(name)
        return call(name, *a)
    with monkeypatch.context() as mp:
        mp.setattr(_abi, "call", spy)
        lo.loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in module.named_parameters() if p.grad is not None}
    stats = {n: b.clone() for n, b in module.named_buffers() if n.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    return names, grads, stats


@pytest.mark.parametrize("forward_small", [True, False])
def test_backward_keeps_the_schedule_its_forward_chose(dev, monkeypatch, forward_small):
    """forward as a small step (one stream, pair grids), then the global says "large step" before backward -- and the other way round
    (forward with the threshold at 0: a large step's per-group launches on two streams; then the global says "small step")"""
    from spvipes_amd import ops
    monkeypatch.setattr(ops, "DEC_PAIR", "auto")
    monkeypatch.setattr(ops, "SERIAL_AUTO", True)
    monkeypatch.setattr(ops, "SERIAL_STREAMS", False)
    small_elems = ops.SMALL_STEP_ELEMS if forward_small else 0
    flip = (lambda *_: ops.set_step_shape(4096, 10_000, 2)) if forward_small else (lambda *_: ops.set_step_shape(B, max(GS), 2))
    try:
        want_names, want, _ = _step(dev, monkeypatch, small_elems, lambda *_: None)
        got_names, got, _ = _step(dev, monkeypatch, small_elems, flip)
    finally:
        ops.set_step_shape(4096, 10_000, 2)
    grouped = "spv_dec_heads_bwd_grouped" in want_names
    assert grouped == forward_small and ("spv_dec_heads_bwd" in want_names) != grouped   # (the two schedules do differ in their launches)
    assert got_names == want_names
    assert got.keys() == want.keys() and len(want) > 0
    for n in want:
        assert torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)), n


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_readouts_between_forward_and_backward_leave_the_step_alone(dev, monkeypatch, precision):
    """a read-out may run between a step's forward and its backward: for both groups ``px_rate_private`` read off the ``generative`` output
    (LazyNBMixture.materialize: the whole front end again, tiled logits included) and ``expected_expression``.  They write workspace arrays
    of their own names and run their BatchNorm with momentum 0, so the backward's launches, every gradient bit and every BatchNorm running
    statistic are those of the undisturbed step"""
    from spvipes_amd import ops

    def readouts(module, inf, gen):
        for g in range(2):
            assert gen["private_poe"][str(g)]["px_rate_private"].shape == (B, GS[g])
            assert module.expected_expression(inf, g).shape == (B, GS[g])
    try:
        want_names, want, want_stats = _step(dev, monkeypatch, ops.SMALL_STEP_ELEMS, lambda *_: None, precision)
        got_names, got, got_stats = _step(dev, monkeypatch, ops.SMALL_STEP_ELEMS, readouts, precision)
    finally:
        ops.set_step_shape(4096, 10_000, 2)
    assert got_names == want_names and len(want_names) > 0
    assert got.keys() == want.keys() and len(want) > 0
    for n in want:
        assert torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)), n
    assert got_stats.keys() == want_stats.keys() and any("decoder" in n for n in want_stats)   # (encoders' and decoders' BatchNorm layers)
    for n in want_stats:
        assert torch.equal(got_stats[n], want_stats[n]), n
