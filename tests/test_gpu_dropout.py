"""GPU: the dropout masks that ``linear_fwd_kernel`` draws on the device (csrc/spv_small.h: ``dropout_keep``) and the steps that run with them.

Every other comparison with a reference runs with dropout off or with recorded masks injected through ``dropout_masks=`` (which never reaches
``dropout_keep``), and the tests that do draw on the device compare the HIP path with itself.  Here the masks a run REALLY used are read back
-- directly (``spv_linear_fwd`` with W = 0, bias = 1, relu: Y is 0 or fl(1 / (1 - p))) or from the fc2 outputs ``EncoderTails`` saves for its
backward -- and

  1. held to the Bernoulli(1 - p) law: rates of whole masks, columns and rows, correlations between masks and inside one (the bounds are the
     binomial law with a union bound over the checks made, n the number of draws behind a figure: never a recorded table of bits),
  2. handed to a float64 torch restatement of the encoder tails (values, input / parameter gradients, BatchNorm running statistics),
  3. handed to the CPU oracle of the whole training step (loss, every parameter gradient), and to the injected-mask path of the same module
     (bit for bit),
  4. required to be independent between ALL encoders of a three-group step (two EncoderTails launches).

Every test prints its worst figure next to the bound before it asserts."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests._step_inputs import _move_relu_kinks_away, _move_trunk_kinks_away, sweep_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


# ---- reading masks back -----------------------------------------------------------------------------------------------------------------
def _scale(p):
    """what the kernel multiplies a kept element by: 1.0f / (1.0f - p)"""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def _draw(dev, p, B, N, K, nprob, seed=0, seed_dev=None, ldy=None, x_random=False):
    """Y [nprob, B, ldy] of one spv_linear_fwd launch with W = 0, bias = 1, relu and dropout p: kept elements hold fl(1 / (1 - p)), dropped
    ones 0, columns beyond N keep the -7 they were filled with.  ``seed``: the host seed; ``seed_dev``: None or the value behind seed_ptr."""
    from spvipes_amd import _abi
    from spvipes_amd._abi import SpvLinearBatch, ptr, stream_ptr
    ldy = N if ldy is None else ldy
    X = torch.randn(B, K, device=dev) if x_random else torch.ones(B, K, device=dev)
    W, bias = torch.zeros(N, K, device=dev), torch.ones(N, device=dev)
    Y = torch.full((nprob, B, ldy), -7.0, device=dev)
    ctr = None if seed_dev is None else torch.full((), int(seed_dev), dtype=torch.int64, device=dev)
    b = SpvLinearBatch()
    b.nprob, b.B, b.relu, b.drop_p, b.seed, b.seed_ptr, b.accumulate = nprob, B, 1, float(p), int(seed), ptr(ctr), 0
    for i in range(nprob):
        q = b.p[i]
        q.X, q.ldx, q.W, q.bias, q.Y, q.ldy, q.N, q.K = ptr(X), K, ptr(W), ptr(bias), ptr(Y[i]), ldy, N, K
    _abi.call("spv_linear_fwd", C.byref(b), stream_ptr())
    torch.cuda.synchronize()
    return Y.cpu().numpy()


def _spy_on_tails(monkeypatch):
    """Records, per EncoderTails.apply call, the fc2 outputs (after relu and dropout) that the call saved for its backward:
    ctx.save_for_backward(*inputs, *h2, *pre, ...) in EncoderTails.forward."""
    from spvipes_amd.nn_ops import EncoderTails
    calls = []
    real = EncoderTails.apply

    def apply(specs, *rest):
        outs = real(specs, *rest)
        calls.append(_saved_h2(outs, specs))
        return outs

    monkeypatch.setattr(EncoderTails, "apply", staticmethod(apply))
    return calls


def _saved_h2(outs, specs):
    from spvipes_amd.nn_ops import N_ENC_PARAMS
    E = len(specs)
    n_in = max(s.h1_group for s in specs) + 1 + E * N_ENC_PARAMS
    return [t.detach().clone() for t in outs[5].grad_fn.saved_tensors[n_in:n_in + E]]


def _exact_fc2(module_or_encoders):
    """fc2.weight = 0, fc2.bias = 1 in every encoder: the saved h2 is then exactly keep / (1 - p)"""
    encs = module_or_encoders if isinstance(module_or_encoders, (list, tuple)) else [e for pair in module_or_encoders.encoders.values() for e in pair.values()]
    with torch.no_grad():
        for e in encs:
            e.fc2.weight.zero_()
            e.fc2.bias.fill_(1.0)


# ---- the statistics (numpy, float64) ------------------------------------------------------------------------------------------------------
def _rate_z(keep, p):
    """(kept fraction - (1 - p)) in units of its binomial sigma, along the last axis"""
    n = keep.shape[-1]
    return (keep.mean(axis=-1, dtype=np.float64) - (1.0 - p)) / math.sqrt(p * (1.0 - p) / n)


def _corr(M):
    """Pearson correlations of the rows of M [m, n]"""
    X = M.astype(np.float64)
    X -= X.mean(axis=1, keepdims=True)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return X @ X.T


def _worst_pair(M):
    c = np.abs(_corr(M))
    np.fill_diagonal(c, 0.0)
    return float(c.max()), np.unravel_index(int(c.argmax()), c.shape)


# ---- 1. the mask obeys the Bernoulli(1 - p) law -------------------------------------------------------------------------------------------
LAW_B, LAW_N, LAW_PROBS, LAW_SEEDS = 4096, 128, 4, 6
_LAW = {}


def _law_masks(dev, p):
    """Y of the 24 masks [6 effective seeds x 4 problems, B, N] for one p (one launch per seed; the seed sits behind seed_ptr, as in training)"""
    if p not in _LAW:
        _LAW[p] = np.concatenate([_draw(dev, p, LAW_B, LAW_N, LAW_N, LAW_PROBS, seed=0, seed_dev=s) for s in range(LAW_SEEDS)])
    return _LAW[p]


PS = [0.1, 0.25, 0.5]


@pytest.mark.parametrize("p", PS)
def test_mask_values_and_rates(dev, p):
    Y = _law_masks(dev, p)
    assert Y.shape == (LAW_SEEDS * LAW_PROBS, LAW_B, LAW_N)
    keep = Y != 0
    assert np.array_equal(Y[keep], np.full(int(keep.sum()), _scale(p), np.float32)), "a kept element is not exactly 1.0f / (1.0f - p)"
    n = LAW_B * LAW_N
    z_all = np.abs(_rate_z(keep.reshape(len(keep), n), p)).max()
    z_col = np.abs(_rate_z(keep.transpose(0, 2, 1), p)).max()   # [mask, column, 4096 draws]
    z_row = np.abs(_rate_z(keep, p)).max()                      # [mask, row, 128 draws]
    print(f"\np {p}: kept fraction worst {z_all:.2f} sigma (bound 5), column {z_col:.2f} (bound 6), row {z_row:.2f} (bound 6)")
    assert z_all <= 5.0
    assert z_col <= 6.0
    assert z_row <= 6.0


@pytest.mark.parametrize("p", PS)
def test_masks_of_other_problems_and_seeds_are_uncorrelated(dev, p):
    keep = _law_masks(dev, p) != 0
    n = LAW_B * LAW_N
    worst, (i, j) = _worst_pair(keep.reshape(len(keep), n))
    print(f"\np {p}: worst pair correlation {worst * math.sqrt(n):.2f} / sqrt(n) (bound 5), masks {i} and {j} of 24 (seed = index // 4, problem = index % 4)")
    assert worst <= 5.0 / math.sqrt(n), (i, j)


@pytest.mark.parametrize("p", PS)
def test_one_mask_is_uncorrelated_with_itself_shifted(dev, p):
    m = (_law_masks(dev, p)[0] != 0).reshape(-1)
    n = m.size
    worst = {}
    for lag in (1, 2, 64, LAW_N, LAW_N + 1, LAW_B):
        worst[lag] = abs(float(_corr(np.stack([m[:-lag], m[lag:]]))[0, 1]))
    print(f"\np {p}: lag correlations in units of 1 / sqrt(n) (bound 5): " + ", ".join(f"lag {k}: {v * math.sqrt(n):.2f}" for k, v in worst.items()))
    for lag, c in worst.items():
        assert c <= 5.0 / math.sqrt(n), lag


def test_host_seed_and_device_counter_add(dev):
    a = _draw(dev, 0.25, 256, LAW_N, LAW_N, 2, seed=3, seed_dev=4)
    b = _draw(dev, 0.25, 256, LAW_N, LAW_N, 2, seed=7, seed_dev=None)
    c = _draw(dev, 0.25, 256, LAW_N, LAW_N, 2, seed=8, seed_dev=None)
    assert np.array_equal(a, b)
    assert not np.array_equal(b[0], c[0]) and not np.array_equal(b[0], b[1])


def test_mask_is_keyed_by_element_not_by_launch_shape(dev):
    p = 0.25
    full = _law_masks(dev, p)[0]                                   # seed 0, problem 0
    assert np.array_equal(_draw(dev, p, 37, LAW_N, LAW_N, 1, seed=0, seed_dev=0)[0], full[:37]), "B = 37 is not the first 37 rows of B = 4096"
    wide = _draw(dev, p, 130, LAW_N, LAW_N, 1, seed=0, seed_dev=0, ldy=LAW_N + 32)[0]
    assert np.array_equal(wide[:, :LAW_N], full[:130]), "the mask moved with ldy"
    assert (wide[:, LAW_N:] == -7.0).all(), "the launch wrote beyond column N"


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,N", [(37, 24), (130, 100)])   # partial 64 x 64 tiles; K = 100 takes the non-vector operand loads
def test_partial_tiles_draw_the_same_law(dev, B, N, p):
    Y = _draw(dev, p, B, N, N, LAW_PROBS, seed=0, seed_dev=11, x_random=True)
    keep = Y != 0
    assert np.array_equal(Y[keep], np.full(int(keep.sum()), _scale(p), np.float32))
    z = np.abs(_rate_z(keep.reshape(LAW_PROBS, B * N), p)).max()
    print(f"\nB {B} N {N} p {p}: kept fraction worst {z:.2f} sigma (bound 5)")
    assert z <= 5.0
    assert not np.array_equal(keep[0], keep[1])


# ---- 2. encoder tails with a device-drawn mask against float64 autograd ------------------------------------------------------------------
def _torch_tail_dropout(enc, h, eps, keep, p):
    """tests/test_gpu_small_ops.py::_torch_tail with the dropout of nn/networks.py:121 on a given keep-mask"""
    import torch.nn.functional as F
    pre = enc.fc2(h)
    h = F.relu(pre) * keep / (1.0 - p)
    loc, logvar = enc.mu_encoder(h), enc.lvar_encoder(h)
    scale = (0.5 * logvar).exp()
    logz = loc + scale * eps
    kl = (0.5 * (scale * scale + loc * loc - 1 - logvar)).sum(1)
    return (loc, logvar, scale, logz, F.softmax(logz, -1), kl), pre.detach()


@pytest.mark.parametrize("linear_bwd", [True, False], ids=["one-launch-bwd", "split-bwd"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,H,ns", [(100, 24, (3, 6, 5, 9)), (700, 128, (10, 25, 10, 25))])
def test_encoder_tails_with_device_dropout_match_float64(dev, monkeypatch, B, H, ns, p, linear_bwd):
    """test_encoder_tails_match_torch's set-up in training mode with the masks drawn by the kernel; its tolerances, unchanged"""
    from spvipes_amd import ops
    from spvipes_amd.module import Encoder
    from spvipes_amd.nn_ops import EncoderSpec, EncoderTails
    from spvipes_amd.ops import Workspace
    monkeypatch.setattr(ops, "LINEAR_BWD", linear_bwd)
    torch.manual_seed(0)
    encs = [Encoder(40, n, H, p).to(dev) for n in ns]
    for e in encs:
        for bn in (e.mu_encoder[1], e.lvar_encoder[1]):
            bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.normal_(0, 0.2)
            bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
        e.train(True)
    refs = [copy.deepcopy(e).cpu().double() for e in encs]
    h1 = [torch.randn(B, 2 * H, device=dev).requires_grad_(True) for _ in range(2)]
    h1r = [t.detach().cpu().double().requires_grad_(True) for t in h1]
    eps = [torch.randn(B, n, device=dev) for n in ns]
    specs = [EncoderSpec(encs[0], 0, 0), EncoderSpec(encs[1], 0, H), EncoderSpec(encs[2], 1, 0), EncoderSpec(encs[3], 1, H)]
    flat = [q for s in specs for q in s.params()]
    outs = EncoderTails.apply(specs, eps, True, p, 5, Workspace(dev), None, *h1, *flat)
    keeps = [(t != 0).cpu() for t in _saved_h2(outs, specs)]
    want, kept, seen = [], 0, 0
    for i, (e, s) in enumerate(zip(refs, specs)):
        o, pre = _torch_tail_dropout(e, h1r[s.h1_group][:, s.h1_col:s.h1_col + H], eps[i].cpu().double(), keeps[i].double(), p)
        want += list(o)
        live = pre > 1e-3    # where the rectifier lets the draw show
        kept, seen = kept + int((keeps[i] & live).sum()), seen + int(live.sum())
    z = (kept / seen - (1.0 - p)) / math.sqrt(p * (1.0 - p) / seen)
    print(f"\nB {B} H {H} p {p}: kept fraction of {seen} live elements {z:+.2f} sigma (bound 5)")
    assert abs(z) <= 5.0
    gen = torch.Generator(device=dev).manual_seed(1)
    coef = [torch.randn(o.shape, device=dev, generator=gen) for o in outs]
    use = lambda k: (k % 6) != 4  # theta is not differentiable through the fused op
    sum((o * c).sum() for k, (o, c) in enumerate(zip(outs, coef)) if use(k)).backward()
    sum((o * c.cpu().double()).sum() for k, (o, c) in enumerate(zip(want, coef)) if use(k)).backward()
    torch.cuda.synchronize()
    f64 = lambda t: t.detach().cpu().double()
    worst = {"out": 0.0, "d h1": 0.0, "d param": 0.0}
    rel = lambda a, b, floor: float(((a - b).abs() / (b.abs() + floor)).max())
    for k, (o, w) in enumerate(zip(outs, want)):
        worst["out"] = max(worst["out"], rel(f64(o), w.detach(), 0.1))
        torch.testing.assert_close(f64(o), w.detach(), rtol=2e-4, atol=2e-5, msg=lambda m: f"output {k}: {m}")
    for a, b in zip(h1, h1r):
        worst["d h1"] = max(worst["d h1"], float((f64(a.grad) - b.grad).abs().max() / b.grad.abs().max()))
        torch.testing.assert_close(f64(a.grad), b.grad, rtol=2e-3, atol=2e-4 * float(b.grad.abs().max()))
    for e, r in zip(encs, refs):
        gmax = max(float(q.grad.abs().max()) for q in r.parameters() if q.grad is not None)  # biases ahead of a train-mode BN have zero gradient: noise floor
        for (name, q), (_, qr) in zip(e.named_parameters(), r.named_parameters()):
            if qr.grad is None and q.grad is None:
                continue  # fc1 is not part of the tail
            g = torch.zeros_like(qr) if qr.grad is None else qr.grad
            worst["d param"] = max(worst["d param"], float((f64(q.grad) - g).abs().max()) / max(float(g.abs().max()), 0.05 * gmax))
            torch.testing.assert_close(f64(q.grad), g, rtol=2e-3, atol=3e-4 * max(float(g.abs().max()), 0.05 * gmax), msg=lambda m: f"{name}: {m}")
        for bn, rbn in ((e.mu_encoder[1], r.mu_encoder[1]), (e.lvar_encoder[1], r.lvar_encoder[1])):
            torch.testing.assert_close(f64(bn.running_mean), rbn.running_mean, rtol=1e-4, atol=1e-6)
            torch.testing.assert_close(f64(bn.running_var), rbn.running_var, rtol=1e-4, atol=1e-6)
    print(f"worst errors: outputs {worst['out']:.1e} (relative, floor 0.1), d h1 {worst['d h1']:.1e} of max |g|, parameter gradients {worst['d param']:.1e} of max |g|")


# ---- 3. the training step with device-drawn dropout against the oracle -------------------------------------------------------------------
STEP_CASES = [  # B, G0, G1, H, n_s, n_p, counts dtype (of tests/test_gpu_shape_sweep.py)
    (37, 45, 51, 16, 6, 3, "f32"),
    (130, 1000, 777, 128, 12, 15, "u16"),
    (200, 129, 257, 256, 10, 5, "u16"),
]
STEP_IDS = [f"B{c[0]}-G{c[1]}x{c[2]}-H{c[3]}-s{c[4]}p{c[5]}-{c[6]}" for c in STEP_CASES]
MASK_NAMES = ["enc_0_private", "enc_0_shared", "enc_1_private", "enc_1_shared"]   # the order of the encoders in module.inference's one launch


def _step_trainer(dev, module, case, counts_h, labels_h, **kw):
    from spvipes_amd.ops import GroupCounts
    from spvipes_amd.train import Trainer
    cdt = case[6]
    to_dev = (lambda c: torch.tensor(c.astype(np.uint16).view(np.int16)).to(dev)) if cdt == "u16" else (lambda c: torch.tensor(c).to(dev))
    counts = [GroupCounts(to_dev(c), c.shape[1], 0, resident=True) for c in counts_h]
    trainer = Trainer(module, counts, labels=[torch.tensor(l, device=dev) for l in labels_h], **kw)
    module.train()
    return trainer


@pytest.mark.parametrize("precision", ["fp32"])
@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_training_step_with_device_dropout_matches_oracle(dev, monkeypatch, case, precision):
    """test_training_step_matches_oracle with dropout_rate 0.1 and the masks the kernel drew handed to the oracle: the two sides then compute
    the same function, so that test's tolerances hold without a margin for dropout.  The same module state run again with the recorded masks
    injected must reproduce the device-drawn step bit for bit.

    fp32 only.  The bf16 cases passed on the shipped kernels (loss within 9e-7 of the oracle's, bound 2e-3) but the first of them ended in a GPU
    memory fault when the file ran against two deliberately wrong builds of csrc/spv_small.h in which earlier tests of the file had failed; the
    cause was not found, so they stay out until it is (the body below still handles precision = "bf16")."""
    from oracle import spvipes_oracle as O
    from spvipes_amd.module import spVIPESmodule
    B, G0, G1, H, n_s, n_p, cdt = case
    P = 0.1
    counts_h, labels_h, rows_h, noise = sweep_inputs(case)
    x_h = [torch.tensor(c[r]) for c, r in zip(counts_h, rows_h)]
    lab_h = [torch.tensor(l[r]) for l, r in zip(labels_h, rows_h)]
    oracle = lambda sd_, x_, noise_, masks_: O.forward_loss(
        sd_, x_, n_dimensions_shared=n_s, n_dimensions_private=n_p, noise=noise_, mode="label", labels=lab_h, training=True, kl_weight=0.7,
        dropout_rate=P, dropout_masks=masks_)
    torch.manual_seed(B)
    module = spVIPESmodule({0: G0, 1: G1}, use_labels=True, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=P, precision=precision).to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    _move_relu_kinks_away(sd, [c[r] for c, r in zip(counts_h, rows_h)])
    calls = _spy_on_tails(monkeypatch)
    rows = [torch.tensor(r, device=dev) for r in rows_h]
    noise_d = {k: v.to(dev) for k, v in noise.items()}
    # The decoder trunk's kinks depend on the latents, hence on the masks; the draw depends on (step counter, encoder, element) alone, not on
    # the parameters: a first forward of a copy with fc2 = (0, 1) shows the masks of this step exactly, before the parameters are final.
    probe = copy.deepcopy(module)
    _exact_fc2(probe)
    probe(_step_trainer(dev, probe, case, counts_h, labels_h).minibatch(rows), inference_kwargs={"noise": noise_d}, loss_kwargs={"kl_weight": 0.7})
    drawn = [(t != 0).cpu() for t in calls[-1]]
    assert len(calls) == 1 and len(drawn) == 4
    for t in calls[-1]:
        assert bool(((t == 0) | (t == float(_scale(P)))).all())
    _move_trunk_kinks_away(sd, lambda sd64: oracle(sd64, [x.double() for x in x_h], {k: v.double() for k, v in noise.items()},
                                                   {k: m.double() for k, m in zip(MASK_NAMES, drawn)}), n_s, n_p)
    module.load_state_dict(sd)
    twin = copy.deepcopy(module)   # the same parameters and BatchNorm buffers, for the injected-mask run
    trainer = _step_trainer(dev, module, case, counts_h, labels_h)
    _, _, lo = module(trainer.minibatch(rows), inference_kwargs={"noise": noise_d}, loss_kwargs={"kl_weight": 0.7})
    lo.loss.backward()
    torch.cuda.synchronize()
    assert len(calls) == 2
    keeps = [(t != 0).cpu() for t in calls[-1]]   # = drawn wherever fc2's pre-activation is positive; elsewhere both sides give 0
    for k, d in zip(keeps, drawn):
        assert not bool((k & ~d).any()), "the masks of a step depend on more than (counter, encoder, element)"
    masks = {k: m.float() for k, m in zip(MASK_NAMES, keeps)}
    want = oracle(sd, x_h, noise, masks)
    got, ref = float(lo.loss.detach()), float(want["loss"])
    tol = 2e-4 if precision == "fp32" else 2e-3
    print(f"\n{precision} B {B} H {H}: loss {got:.6f}, oracle {ref:.6f}, relative error {abs(got - ref) / abs(ref):.1e} (bound {tol:.0e})")
    assert abs(got - ref) / abs(ref) < tol, (got, ref)
    params = dict(module.named_parameters())
    if precision == "fp32":
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k in params}
        sd2 = dict(sd); sd2.update(leaves)
        oracle(sd2, x_h, noise, masks)["loss"].backward()
        gmax = max(float(v.grad.abs().max()) for v in leaves.values() if v.grad is not None)
        bad, worst = [], 0.0
        for k, q in params.items():
            ref_g = leaves[k].grad
            if ref_g is None:
                continue
            mine = torch.zeros_like(q) if q.grad is None else q.grad
            err = float((mine.cpu() - ref_g).abs().max())
            bound = 5e-3 * float(ref_g.abs().max()) + 2e-4 * gmax
            worst = max(worst, err / bound)
            if not err < bound:
                bad.append(f"{k}: abs err {err:.3e} (max |g| {float(ref_g.abs().max()):.3e})")
        print(f"worst gradient error: {worst:.3f} of its bound (5e-3 max|g| + 2e-4 gmax)")
        assert not bad, "gradients off: " + "; ".join(bad)
    # the injected-mask path of the goldens on the same state and masks
    trainer2 = _step_trainer(dev, twin, case, counts_h, labels_h)
    _, _, lo2 = twin(trainer2.minibatch(rows), inference_kwargs={"noise": noise_d, "dropout_masks": {k: m.to(dev) for k, m in masks.items()}},
                     loss_kwargs={"kl_weight": 0.7})
    lo2.loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(lo2.loss.detach(), lo.loss.detach())
    for (k, q), (_, q2) in zip(params.items(), twin.named_parameters()):
        assert (q.grad is None) == (q2.grad is None), k
        assert q.grad is None or torch.equal(q.grad, q2.grad), k


def test_consecutive_steps_draw_fresh_masks(dev, monkeypatch):
    """the step counter (advanced on the device by the optimiser's launch) keys the draw: the four masks of step t + 1 are new, and no more
    correlated with those of step t -- or with each other -- than independent draws are"""
    from spvipes_amd.module import spVIPESmodule
    case = STEP_CASES[2]
    B, G0, G1, H, n_s, n_p, cdt = case
    P = 0.1
    counts_h, labels_h, rows_h, _ = sweep_inputs(case)
    torch.manual_seed(B)
    module = spVIPESmodule({0: G0, 1: G1}, use_labels=True, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=P, precision="fp32").to(dev)
    _exact_fc2(module)
    trainer = _step_trainer(dev, module, case, counts_h, labels_h, lr=1e-6)   # (fc2 stays (0, 1) to within 1e-6 per element: h2 > 0 where kept)
    calls = _spy_on_tails(monkeypatch)
    rows = [torch.tensor(r, device=dev) for r in rows_h]
    for _ in range(2):
        trainer.step(rows, kl_weight=0.7)
    torch.cuda.synchronize()
    assert len(calls) == 2
    keep = np.stack([(t != 0).cpu().numpy().reshape(-1) for call in calls for t in call])   # [2 steps x 4 encoders, B * H]
    n = B * H
    assert np.abs(_rate_z(keep, P)).max() <= 5.0
    for i in range(4):
        assert not np.array_equal(keep[i], keep[4 + i]), f"step 2 repeated the mask of {MASK_NAMES[i]}"
    worst, (i, j) = _worst_pair(keep)
    print(f"\nworst correlation among the 8 masks of two steps: {worst * math.sqrt(n):.2f} / sqrt(n) (bound 5), masks {i} and {j}")
    assert worst <= 5.0 / math.sqrt(n), (i, j)


# ---- 4. three groups: an independent mask for every encoder ------------------------------------------------------------------------------
def test_three_group_step_draws_six_independent_masks(dev, monkeypatch):
    """tests/test_gpu_three_groups.py's three-group module with dropout: its encoder tails run as two launches (groups 0 and 1, then group 2)
    that number their problems from 0 and read the same step counter; the second launch must not repeat the first one's masks."""
    from spvipes_amd.data import MinibatchSampler, make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    P, B, H = 0.25, 256, 256
    Gs = (300, 260, 340)
    groups = [make_synthetic_group(g % 2, 1024, Gs[g], dev) for g in range(3)]
    torch.manual_seed(0)
    module = spVIPESmodule({g: Gs[g] for g in range(3)}, transport_plan="components", pair_data=False, allow_more_groups=True, n_components=10,
                           n_hidden=H, n_dimensions_shared=10, n_dimensions_private=5, dropout_rate=P, precision="bf16").to(dev)
    _exact_fc2(module)
    trainer = Trainer(module, [g.counts for g in groups], components=[g.labels for g in groups], lr=5e-3)
    module.train()
    calls = _spy_on_tails(monkeypatch)
    rows = next(iter(MinibatchSampler([1024] * 3, B, dev, seed=0).epoch()))
    trainer.step(rows, kl_weight=1.0, optimizer_step=False)
    torch.cuda.synchronize()
    h2 = [t for call in calls for t in call]
    assert [len(c) for c in calls] == [4, 2] and all(t.shape == (B, H) for t in h2)
    for t in h2:
        assert bool(((t == 0) | (t == float(_scale(P)))).all())
    names = [f"enc_{g}_{kind}" for g in range(3) for kind in ("private", "shared")]
    keep = np.stack([(t != 0).cpu().numpy().reshape(-1) for t in h2])
    n = B * H
    z = np.abs(_rate_z(keep, P))
    same = [(names[i], names[j]) for i in range(6) for j in range(i + 1, 6) if np.array_equal(keep[i], keep[j])]
    worst, (i, j) = _worst_pair(keep)
    print(f"\nthree groups: kept fraction worst {z.max():.2f} sigma (bound 5); worst pair correlation {worst * math.sqrt(n):.2f} / sqrt(n) (bound 5), "
          f"{names[i]} and {names[j]}; identical pairs: {same}")
    assert z.max() <= 5.0
    assert not same, f"encoders with IDENTICAL dropout masks: {same}"
    assert worst <= 5.0 / math.sqrt(n), (names[i], names[j])
