"""GPU: spv_linear_bwd -- a small layer's input and weight gradients as ONE launch, the slice sum of the weight gradient riding in the
next such launch or run alone (spv_linear_reduce_pending) -- against the separate spv_linear_dgrad / spv_linear_wgrad launches.  The one
grid runs the separate kernels' bodies with their block coordinates, so EQUALITY OF BITS is the criterion everywhere: at the entry points
on the shapes of the three call sites (mu / logvar heads, fc2, mixing trunk: nn/networks.py:120-124, 322-323 and their autograd) and for
whole training steps with ops.LINEAR_BWD on and off, eagerly and under hipGraph replay."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPV_ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


class _Layer:
    """One call site's pair of batches over shared random inputs.  new_out() -> fresh gradient tensors (NaN filled; the trunk's
    dX pre-filled with the values it accumulates into), build(out) -> (bd, bw) writing into them."""

    def __init__(self, dev, B, kind, seed):
        g = torch.Generator().manual_seed(seed)
        self.rn = lambda *s: torch.randn(*s, generator=g).to(dev)
        self.dev, self.B, self.kind = dev, B, kind
        rn = self.rn
        if kind == "heads":   # 8 weight-gradient problems N 5 / 10, K 64, odd pitch 2N; 4 input-gradient problems over (W | W2)
            self.ns = (5, 10, 5, 10)
            self.h2 = [rn(B, 64) for _ in self.ns]
            self.d_pre = [rn(B, 2 * n) for n in self.ns]
            self.Wmu, self.Wlv = [rn(n, 64) for n in self.ns], [rn(n, 64) for n in self.ns]
            self.relu, self.drop_p, self.acc = False, 0.0, False
        elif kind == "fc2":   # N = K = 64, rectifier + dropout mask recovered from Y > 0; X / dX are column blocks of a [B][128] matrix
            self.h1, self.W = rn(B, 128), [rn(64, 64) for _ in range(2)]
            self.Y = [torch.relu(rn(B, 64)) * (torch.rand(B, 64, generator=g) >= 0.25).to(dev) for _ in range(2)]
            self.dY = [rn(B, 64) for _ in range(2)]
            self.relu, self.drop_p, self.acc = True, 0.25, False
        else:                 # trunk: N 256, K 35 (no multiple of 8: the non-vector loads), rectifier, accumulation into a filled dX
            self.X, self.W = [rn(B, 35) for _ in range(2)], [rn(256, 35) for _ in range(2)]
            self.Y, self.dY = [torch.relu(rn(B, 256)) for _ in range(2)], [rn(B, 256) for _ in range(2)]
            self.dX0 = [rn(B, 35) for _ in range(2)]
            self.relu, self.drop_p, self.acc = True, 0.0, True

    def new_out(self):
        nan = lambda *s: torch.full(s, float("nan"), device=self.dev)   # (an element no launch writes then fails the comparison)
        B = self.B
        if self.kind == "heads":
            return {"dX": [nan(B, 64) for _ in self.ns], "dW": [nan(n, 64) for n in self.ns for _ in range(2)], "db": [nan(n) for n in self.ns for _ in range(2)]}
        if self.kind == "fc2":
            return {"dX": [nan(B, 128)], "dW": [nan(64, 64) for _ in range(2)], "db": [nan(64) for _ in range(2)]}
        return {"dX": [t.clone() for t in self.dX0], "dW": [nan(256, 35) for _ in range(2)], "db": [nan(256) for _ in range(2)]}

    def build(self, out):
        from spvipes_amd._abi import ptr
        from spvipes_amd.nn_ops import _add_lin, _fptr, _lin_batch
        B = self.B
        bd, bw = _lin_batch(B, relu=self.relu, drop_p=self.drop_p, accumulate=self.acc), _lin_batch(B, relu=self.relu, drop_p=self.drop_p)
        if self.kind == "heads":
            for i, n in enumerate(self.ns):
                _add_lin(bw, N=n, K=64, W=ptr(self.Wmu[i]), X=ptr(self.h2[i]), ldx=64, dY=_fptr(self.d_pre[i], 0), lddy=2 * n, dW=ptr(out["dW"][2 * i]), db=ptr(out["db"][2 * i]))
                _add_lin(bw, N=n, K=64, W=ptr(self.Wlv[i]), X=ptr(self.h2[i]), ldx=64, dY=_fptr(self.d_pre[i], n), lddy=2 * n, dW=ptr(out["dW"][2 * i + 1]), db=ptr(out["db"][2 * i + 1]))
                _add_lin(bd, N=2 * n, K=64, W=ptr(self.Wmu[i]), W2=ptr(self.Wlv[i]), n_w2=n, dY=ptr(self.d_pre[i]), lddy=2 * n, dX=ptr(out["dX"][i]), lddx=64)
        elif self.kind == "fc2":
            for i in range(2):
                _add_lin(bw, N=64, K=64, W=ptr(self.W[i]), X=_fptr(self.h1, 64 * i), ldx=128, Y=ptr(self.Y[i]), ldy=64, dY=ptr(self.dY[i]), lddy=64, dW=ptr(out["dW"][i]), db=ptr(out["db"][i]))
                _add_lin(bd, N=64, K=64, W=ptr(self.W[i]), Y=ptr(self.Y[i]), ldy=64, dY=ptr(self.dY[i]), lddy=64, dX=_fptr(out["dX"][0], 64 * i), lddx=128)
        else:
            for i in range(2):
                _add_lin(bw, N=256, K=35, W=ptr(self.W[i]), X=ptr(self.X[i]), ldx=35, Y=ptr(self.Y[i]), ldy=256, dY=ptr(self.dY[i]), lddy=256, dW=ptr(out["dW"][i]), db=ptr(out["db"][i]))
                _add_lin(bd, N=256, K=35, W=ptr(self.W[i]), Y=ptr(self.Y[i]), ldy=256, dY=ptr(self.dY[i]), lddy=256, dX=ptr(out["dX"][i]), lddx=35)
        return bd, bw

    def reference(self, ws):
        """the separate launches: spv_linear_dgrad, spv_linear_wgrad (+ its reduce)"""
        from spvipes_amd import _abi
        from spvipes_amd.nn_ops import _wgrad
        out = self.new_out()
        bd, bw = self.build(out)
        _abi.call("spv_linear_dgrad", C.byref(bd), _abi.stream_ptr())
        _wgrad(bw, ws)
        torch.cuda.synchronize()
        return out


def _same(ref, got, keys=("dX", "dW", "db"), what=""):
    for k in keys:
        for i, (a, b) in enumerate(zip(ref[k], got[k])):
            assert torch.isfinite(a).all(), (what, k, i)
            assert torch.equal(a, b), (what, k, i, float((a - b).abs().nan_to_num(float("inf")).max()))


@pytest.fixture(scope="module")
def cases(dev):
    """(layers, references) per minibatch size, computed once: 96 = the direct form (ragged against the 64-row blocks), 272 = the smallest
    sliced case (slices 0-3 full, slice 4 of 16 rows, 11 empty), 1100 = ragged 128-row slices"""
    from spvipes_amd.ops import Workspace
    res = {}
    for B in (96, 272, 1100):
        layers = {k: _Layer(dev, B, k, seed=B + j) for j, k in enumerate(("heads", "fc2", "trunk"))}
        res[B] = (layers, {k: l.reference(Workspace(dev)) for k, l in layers.items()})
    return res


@pytest.mark.parametrize("B", [96, 272, 1100])
def test_one_launch_gives_the_bits_of_the_separate_launches(dev, cases, B):
    """the chain of the encoder tails -- heads, then fc2 with the heads' slice sum riding, then fc2's slice sum alone -- and the trunk's
    launch with its lone reduce"""
    from spvipes_amd.nn_ops import _linear_bwd, _reduce_pending
    from spvipes_amd.ops import Workspace
    layers, refs = cases[B]
    ws = Workspace(dev)
    outs = {k: l.new_out() for k, l in layers.items()}
    bd, bw = layers["heads"].build(outs["heads"])
    pend = _linear_bwd(bd, bw, ws, "part_heads")
    assert (pend is None) == (B <= 256)   # the direct form leaves nothing to sum
    bd2, bw2 = layers["fc2"].build(outs["fc2"])
    pend2 = _linear_bwd(bd2, bw2, ws, "part_fc2", pend)
    _reduce_pending(pend2)
    bd3, bw3 = layers["trunk"].build(outs["trunk"])
    _reduce_pending(_linear_bwd(bd3, bw3, ws, "part_trunk"))
    torch.cuda.synchronize()
    for k in layers:
        _same(refs[k], outs[k], what=k)


@pytest.mark.parametrize("B", [272, 1100])
def test_parts_alone_and_the_pending_reduce_through_every_door(dev, cases, B):
    """weight gradients alone (d NULL), input gradients alone with a pending record (w NULL), the record through spv_linear_bwd(NULL, NULL)"""
    from spvipes_amd import _abi
    from spvipes_amd.nn_ops import _linear_bwd
    from spvipes_amd.ops import Workspace
    layers, refs = cases[B]
    ws = Workspace(dev)
    for k, other in (("heads", "fc2"), ("trunk", "heads")):
        out, out_o = layers[k].new_out(), layers[other].new_out()
        _, bw = layers[k].build(out)
        pend = _linear_bwd(None, bw, ws, "part_" + k)
        bd_o, _ = layers[other].build(out_o)
        assert _linear_bwd(bd_o, None, ws, "unused", pend) is None
        torch.cuda.synchronize()
        _same(refs[k], out, keys=("dW", "db"), what=k)
        _same(refs[other], out_o, keys=("dX",), what=other)
        for t in out["dW"] + out["db"]:
            t.fill_(float("nan"))
        _abi.call("spv_linear_bwd", None, None, None, 0, C.byref(pend), _abi.stream_ptr())
        torch.cuda.synchronize()
        _same(refs[k], out, keys=("dW", "db"), what=k + " (record alone)")


def test_direct_form_parts_alone(dev, cases):
    from spvipes_amd.nn_ops import _linear_bwd
    from spvipes_amd.ops import Workspace
    layers, refs = cases[96]
    ws = Workspace(dev)
    for k in layers:
        out = layers[k].new_out()
        bd, bw = layers[k].build(out)
        assert _linear_bwd(None, bw, ws, "part") is None and _linear_bwd(bd, None, ws, "part") is None
        torch.cuda.synchronize()
        _same(refs[k], out, what=k)


def test_bad_pairings_are_rejected(dev, cases):
    """different B / relu / drop_p between the two batches, accumulate on the weight-gradient batch, the pending workspace as this launch's
    workspace, nothing to do: SPV_ERR_ARG, and nothing is launched"""
    from spvipes_amd import _abi
    from spvipes_amd.nn_ops import _linear_bwd
    lib = _abi.load()
    layers, _ = cases[272]
    out = layers["fc2"].new_out()
    part = torch.empty(2 * 16 * 64 * 65, device=dev)
    args = lambda bd, bw, pend=None, p=part: (C.byref(bd), C.byref(bw), _abi.ptr(p), p.numel(), C.byref(pend) if pend is not None else None, _abi.stream_ptr())
    bd, bw = layers["fc2"].build(out)
    assert lib.spv_linear_bwd(*args(bd, bw)) == 0
    for field, value in (("B", 271), ("relu", 0), ("drop_p", 0.5), ("accumulate", 1)):
        bd, bw = layers["fc2"].build(out)
        setattr(bw, field, value)
        assert lib.spv_linear_bwd(*args(bd, bw)) == SPV_ERR_ARG, field
    bd, bw = layers["fc2"].build(out)
    bd.B = 300
    assert lib.spv_linear_bwd(*args(bd, bw)) == SPV_ERR_ARG
    bd, bw = layers["fc2"].build(out)
    big =torch.empty(part.numel() + 64, device=dev)

    class _In:   # (a workspace that hands out the head of `big`, so that a shifted window of it is large enough AND overlaps)
        get = staticmethod(lambda name, shape, dtype: big[:shape[0]])
    pend = _linear_bwd(None, bw, _In, "part")
    own = big[:part.numel()]
    assert lib.spv_linear_bwd(*args(bd, bw, pend, own)) == SPV_ERR_ARG            # the very workspace the record names
    assert lib.spv_linear_bwd(*args(bd, bw, pend, own[64:])) == SPV_ERR_ARG       # ... or a part of it
    assert lib.spv_linear_bwd(*args(bd, bw, pend)) == 0
    assert lib.spv_linear_bwd(None, None, None, 0, None, _abi.stream_ptr()) == SPV_ERR_ARG
    assert lib.spv_linear_reduce_pending(None, _abi.stream_ptr()) == SPV_ERR_ARG
    pend.nprob = 0
    assert lib.spv_linear_reduce_pending(C.byref(pend), _abi.stream_ptr()) == SPV_ERR_ARG
    torch.cuda.synchronize()


# ---- whole steps -------------------------------------------------------------------------------------------------------------------
def _run(dev, groups, genes, B, precision, use_graph, on, monkeypatch, steps=2):
    from spvipes_amd import ops
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    monkeypatch.setattr(ops, "LINEAR_BWD", on)
    torch.manual_seed(0)
    module = spVIPESmodule({0: genes[0], 1: genes[1]}, use_labels=True, n_hidden=64, n_dimensions_shared=25, n_dimensions_private=10, dropout_rate=0.1,
                           precision=precision).to(dev)
    trainer = Trainer(module, [g.counts for g in groups], labels=[g.labels for g in groups])
    module.train()
    trainer._ensure_images()
    rng = np.random.default_rng(11)
    n = min(g.counts.X.shape[0] for g in groups)
    batches = [[torch.tensor(rng.permutation(n)[:B].astype(np.int32), device=dev) for _ in range(2)] for _ in range(steps + 1)]
    if use_graph:
        keep = {k: b.clone() for k, b in module.named_buffers()}
        trainer.capture(batches[steps])
        with torch.no_grad():
            for k, b in module.named_buffers():
                b.copy_(keep[k])
    out = []
    for i in range(steps):
        lo = trainer.step(batches[i], kl_weight=0.7)
        torch.cuda.synchronize()
        out.append((lo.loss.detach().clone(), trainer.fp.grad.clone()))
    state = {"flat": trainer.fp.flat.clone(), "m": trainer.opt.m.clone(), "v": trainer.opt.v.clone(), **{k: b.clone() for k, b in module.named_buffers()}}
    return out, state


@pytest.fixture(scope="module")
def step_groups(dev):
    from spvipes_amd.data import make_synthetic_group
    return [make_synthetic_group(g, 1000, 512, dev) for g in range(2)]


@pytest.mark.parametrize("B,precision,use_graph", [(320, "bf16", False), (320, "bf16", True), (320, "fp32", False), (320, "fp32", True),
                                                   (128, "bf16", False), (128, "bf16", True)])
def test_steps_keep_their_bits(dev, step_groups, B, precision, use_graph, monkeypatch):
    """two groups, G 512, H 64, label PoE, dropout on: loss, every gradient, parameters, Adam moments and BatchNorm buffers with the one-launch
    backward equal those of the separate launches (B 128: the direct form inside a step)"""
    (ref, s_ref), (got, s_got) = (_run(dev, step_groups, (512, 512), B, precision, use_graph, on, monkeypatch) for on in (False, True))
    for i, ((l0, g0), (l1, g1)) in enumerate(zip(ref, got)):
        assert torch.isfinite(l0) and torch.equal(torch.isnan(g0), torch.isnan(g1)), i
        assert torch.equal(l0, l1), (i, float(l0), float(l1))
        assert torch.equal(torch.nan_to_num(g0), torch.nan_to_num(g1)), (i, float((torch.nan_to_num(g0) - torch.nan_to_num(g1)).abs().max()))
    for k in s_ref:
        assert torch.equal(torch.nan_to_num(s_ref[k]), torch.nan_to_num(s_got[k])), k
