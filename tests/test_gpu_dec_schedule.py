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


def _step(dev, monkeypatch, small_elems, between):
    """one training forward and backward from seed 0 with the "small step" threshold ``small_elems`` during forward; ``between`` runs after
    the forward and before the backward.  Returns (entry points the backward called, in order; every parameter's gradient)"""
    from spvipes_amd import _abi, ops
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    groups = [make_synthetic_group(g, CELLS, GS[g], dev) for g in range(2)]
    module = spVIPESmodule({0: GS[0], 1: GS[1]}, use_labels=True, n_hidden=H, n_dimensions_shared=N_S, n_dimensions_private=N_P,
                           dropout_rate=0.0, precision="bf16").to(dev)
    trainer = Trainer(module, [g.counts for g in groups], labels=[g.labels for g in groups])
    module.train()
    rows = [torch.tensor(rng.permutation(CELLS)[:B], dtype=torch.int32, device=dev) for _ in range(2)]
    gen = torch.Generator().manual_seed(1)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen).to(dev) for g in range(2) for k, n in (("private", N_P), ("shared", N_S))}
    noise.update({f"poe_{g}": torch.randn(B, N_S, generator=gen).to(dev) for g in range(2)})
    with monkeypatch.context() as mp:
        mp.setattr(ops, "SMALL_STEP_ELEMS", small_elems)
        _, _, lo = module(trainer.minibatch(rows), inference_kwargs={"noise": noise}, loss_kwargs={"kl_weight": 1.0})
    trainer.fp.grad.zero_()
    between()
    names, call = [], _abi.call

    def spy(name, *a):
        names.append(name)
        return call(name, *a)
    with monkeypatch.context() as mp:
        mp.setattr(_abi, "call", spy)
        lo.loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in module.named_parameters() if p.grad is not None}
    return names, grads


@pytest.mark.parametrize("forward_small", [True, False])
def test_backward_keeps_the_schedule_its_forward_chose(dev, monkeypatch, forward_small):
    """forward as a small step (one stream, pair grids), then the global says "large step" before backward -- and the other way round
    (forward with the threshold at 0: a large step's per-group launches on two streams; then the global says "small step")"""
    from spvipes_amd import ops
    monkeypatch.setattr(ops, "DEC_PAIR", "auto")
    monkeypatch.setattr(ops, "SERIAL_AUTO", True)
    monkeypatch.setattr(ops, "SERIAL_STREAMS", False)
    small_elems = ops.SMALL_STEP_ELEMS if forward_small else 0
    flip = (lambda: ops.set_step_shape(4096, 10_000, 2)) if forward_small else (lambda: ops.set_step_shape(B, max(GS), 2))
    try:
        want_names, want = _step(dev, monkeypatch, small_elems, lambda: None)
        got_names, got = _step(dev, monkeypatch, small_elems, flip)
    finally:
        ops.set_step_shape(4096, 10_000, 2)
    grouped = "spv_dec_heads_bwd_grouped" in want_names
    assert grouped == forward_small and ("spv_dec_heads_bwd" in want_names) != grouped   # (the two schedules do differ in their launches)
    assert got_names == want_names
    assert got.keys() == want.keys() and len(want) > 0
    for n in want:
        assert torch.equal(got[n].view(torch.int32), want[n].view(torch.int32)), n
