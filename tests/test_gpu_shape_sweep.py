"""Odd shapes through the whole HIP path against the CPU oracle on the same inputs, parameters and noise:
batch sizes and gene counts that are not multiples of any tile, wide and narrow layers, uint16 and fp32 counts,
resident (Trainer) and per-call (module X tensors) input layouts."""
import numpy as np
import pytest
import torch

from tests._step_inputs import _move_relu_kinks_away, _move_trunk_kinks_away, sweep_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()  # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


CASES = [  # B, G0, G1, H, n_s, n_p, counts dtype
    (5, 20, 20, 8, 3, 2, "u16"),
    (37, 45, 51, 16, 6, 3, "f32"),
    (100, 333, 200, 64, 25, 10, "u16"),
    (130, 1000, 777, 128, 12, 15, "u16"),
    (64, 2001, 35, 32, 31, 4, "f32"),
    (200, 129, 257, 256, 10, 5, "u16"),
    (33, 100, 90, 50, 7, 3, "u16"),         # hidden width that is a multiple of nothing
    (257, 64, 4100, 24, 31, 15, "u16"),      # the widest latents the regressor operands hold
    (70, 301, 150, 32, 8, 4, "f32frac"),   # non-integral "counts" (normalised data): the lgamma terms leave the integer table
]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}-G{c[1]}x{c[2]}-H{c[3]}-s{c[4]}p{c[5]}-{c[6]}" for c in CASES])
def test_training_step_matches_oracle(dev, case, precision):
    from oracle import spvipes_oracle as O
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.ops import GroupCounts
    from spvipes_amd.train import Trainer
    B, G0, G1, H, n_s, n_p, cdt = case
    counts_h, labels_h, rows_h, noise = sweep_inputs(case)
    torch.manual_seed(B)
    module = spVIPESmodule({0: G0, 1: G1}, use_labels=True, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=0.0, precision=precision).to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    _move_relu_kinks_away(sd, [c[r] for c, r in zip(counts_h, rows_h)])
    _move_trunk_kinks_away(sd, lambda sd64: O.forward_loss(
        sd64, [torch.tensor(c[r]).double() for c, r in zip(counts_h, rows_h)], n_dimensions_shared=n_s, n_dimensions_private=n_p,
        noise={k: v.double() for k, v in noise.items()}, mode="label", labels=[torch.tensor(l[r]) for l, r in zip(labels_h, rows_h)],
        training=True, kl_weight=0.7), n_s, n_p)
    module.load_state_dict(sd)
    to_dev = (lambda c: torch.tensor(c.astype(np.uint16).view(np.int16)).to(dev)) if cdt == "u16" else (lambda c: torch.tensor(c).to(dev))
    counts = [GroupCounts(to_dev(c), c.shape[1], 0, resident=True) for c in counts_h]
    trainer = Trainer(module, counts, labels=[torch.tensor(l, device=dev) for l in labels_h])
    module.train()
    rows = [torch.tensor(r, device=dev) for r in rows_h]
    _, _, lo = module(trainer.minibatch(rows), inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}}, loss_kwargs={"kl_weight": 0.7})
    lo.loss.backward()
    torch.cuda.synchronize()
    want = O.forward_loss(sd, [torch.tensor(c[r]) for c, r in zip(counts_h, rows_h)], n_dimensions_shared=n_s, n_dimensions_private=n_p,
                          noise=noise, mode="label", labels=[torch.tensor(l[r]) for l, r in zip(labels_h, rows_h)], training=True, kl_weight=0.7)
    got, ref = float(lo.loss.detach()), float(want["loss"])
    tol = 2e-4 if precision == "fp32" else 2e-3   # north-star: rtol 1e-3 on the ELBO in fp32; bf16 operands get 2e-3 on these tiny layers
    assert abs(got - ref) / abs(ref) < tol, (got, ref)
    if precision == "fp32":
        # gradients of a few parameters of every kind against the oracle's autograd
        params = dict(module.named_parameters())
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k in params}
        sd2 = dict(sd); sd2.update(leaves)
        out = O.forward_loss(sd2, [torch.tensor(c[r]) for c, r in zip(counts_h, rows_h)], n_dimensions_shared=n_s, n_dimensions_private=n_p,
                             noise=noise, mode="label", labels=[torch.tensor(l[r]) for l, r in zip(labels_h, rows_h)], training=True, kl_weight=0.7)
        out["loss"].backward()
        gmax = max(float(v.grad.abs().max()) for v in leaves.values() if v.grad is not None)
        bad = []
        for k, p in params.items():
            ref_g = leaves[k].grad
            if ref_g is None:
                continue
            mine = torch.zeros_like(p) if p.grad is None else p.grad
            err = float((mine.cpu() - ref_g).abs().max())
            if not err < 5e-3 * float(ref_g.abs().max()) + 2e-4 * gmax:
                bad.append(f"{k}: abs err {err:.3e} (max |g| {float(ref_g.abs().max()):.3e})")
        assert not bad, "gradients off: " + "; ".join(bad)


PLAN_CASES = [  # mode, B, G0, G1, H, n_s, n_p
    ("paired", 37, 45, 51, 16, 6, 3),
    ("paired", 130, 700, 333, 128, 12, 15),
    ("cluster", 100, 333, 200, 64, 25, 10),
    ("cluster", 67, 129, 257, 32, 10, 5),
]


@pytest.mark.parametrize("case", PLAN_CASES, ids=[f"{c[0]}-B{c[1]}-G{c[2]}x{c[3]}-H{c[4]}-s{c[5]}p{c[6]}" for c in PLAN_CASES])
def test_transport_plan_modes_match_oracle_at_odd_shapes(dev, case):
    """paired / cluster PoE through the module's own API (outer-joined X per call, dense plan handed to the constructor,
    minibatch = arbitrary rows of the data set) against the oracle on the same parameters and noise: ELBO and every
    parameter gradient, fp32."""
    from oracle import spvipes_oracle as O
    from spvipes_amd.module import spVIPESmodule
    mode, B, G0, G1, H, n_s, n_p = case
    rng = np.random.default_rng(B * 13 + G1)
    Gs = (G0, G1)
    n_cells = (B + 9, B + 23)
    counts_h = [(rng.poisson(3.0, size=(n_cells[g], Gs[g])) * (rng.random((n_cells[g], Gs[g])) < 0.35)).astype(np.float32) for g in range(2)]
    for c in counts_h:
        c[:, 0] += 1
    plan = (rng.random(n_cells) * (rng.random(n_cells) < 0.08)).astype(np.float32)
    plan[rng.integers(0, n_cells[0], 5)] = 0.0          # rows without any partner: argmax -> 0 / zero row weights
    idx_h = [rng.permutation(n_cells[g])[:B] for g in range(2)]
    comp_h = [rng.integers(0, 5, size=n_cells[0]).astype(np.float32), rng.integers(1, 6, size=n_cells[1]).astype(np.float32)]
    torch.manual_seed(B)
    module = spVIPESmodule({0: G0, 1: G1}, transport_plan=torch.tensor(plan).to(dev), pair_data=(mode == "paired"), use_labels=False,
                           n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p, dropout_rate=0.0, precision="fp32").to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    _move_relu_kinks_away(sd, [c[i] for c, i in zip(counts_h, idx_h)])
    gen = torch.Generator().manual_seed(2)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen) for g in range(2) for k, n in (("private", n_p), ("shared", n_s))}
    noise.update({f"poe_{g}": torch.randn(B, n_s, generator=gen) for g in range(2)})
    block = torch.tensor(plan[idx_h[0]][:, idx_h[1]])
    comps = [torch.tensor(comp_h[g][idx_h[g]]) for g in range(2)] if mode == "cluster" else None
    _move_trunk_kinks_away(sd, lambda sd64: O.forward_loss(
        sd64, [torch.tensor(c[i]).double() for c, i in zip(counts_h, idx_h)], n_dimensions_shared=n_s, n_dimensions_private=n_p,
        noise={k: v.double() for k, v in noise.items()}, mode=mode, plan_block=block.double(), components=comps, training=True, kl_weight=0.6), n_s, n_p)
    module.load_state_dict(sd)
    module.train()
    tensors = []
    for g in range(2):
        X = np.zeros((B, G0 + G1), np.float32)
        X[:, (0 if g == 0 else G0):(G0 if g == 0 else G0 + G1)] = counts_h[g][idx_h[g]]
        d = {"X": torch.tensor(X).to(dev), "batch": torch.zeros(B, 1, device=dev), "groups": torch.full((B, 1), float(g), device=dev),
             "indices": torch.tensor(idx_h[g], dtype=torch.float32, device=dev).unsqueeze(1)}
        if mode == "cluster":
            d["processed_transport_labels"] = torch.tensor(comp_h[g][idx_h[g]], device=dev).unsqueeze(1)
        tensors.append(d)
    _, _, lo = module(tuple(tensors), inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}}, loss_kwargs={"kl_weight": 0.6})
    lo.loss.backward()
    torch.cuda.synchronize()
    params = dict(module.named_parameters())
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k in params}
    sd2 = dict(sd); sd2.update(leaves)
    out = O.forward_loss(sd2, [torch.tensor(c[i]) for c, i in zip(counts_h, idx_h)], n_dimensions_shared=n_s, n_dimensions_private=n_p, noise=noise,
                         mode=mode, plan_block=block, components=comps, training=True, kl_weight=0.6)
    got, ref = float(lo.loss.detach()), float(out["loss"].detach())
    assert abs(got - ref) / abs(ref) < 2e-4, (got, ref)
    out["loss"].backward()
    gmax = max(float(v.grad.abs().max()) for v in leaves.values() if v.grad is not None)
    bad = []
    for k, p in params.items():
        ref_g = leaves[k].grad
        if ref_g is None:
            continue
        mine = torch.zeros_like(p) if p.grad is None else p.grad
        err = float((mine.cpu() - ref_g).abs().max())
        if not err < 5e-3 * float(ref_g.abs().max()) + 2e-4 * gmax:
            bad.append(f"{k}: abs err {err:.3e} (max |g| {float(ref_g.abs().max()):.3e})")
    assert not bad, "gradients off: " + "; ".join(bad)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [(37, 45, 51, 16, 6, 3), (130, 1000, 777, 128, 12, 15)], ids=["B37", "B130"])
def test_eval_mode_elbo_matches_oracle(dev, case, precision):
    """eval mode (BatchNorm on running statistics that a few training steps have moved, no dropout): ELBO, per-cell
    reconstruction terms and the PoE means against the oracle."""
    from oracle import spvipes_oracle as O
    from spvipes_amd.module import spVIPESmodule
    B, G0, G1, H, n_s, n_p = case
    rng = np.random.default_rng(B)
    counts_h = [(rng.poisson(3.0, size=(B, G)) * (rng.random((B, G)) < 0.35)).astype(np.float32) for G in (G0, G1)]
    for c in counts_h:
        c[:, 0] += 1
    labels_h = [rng.integers(0, 4, size=B).astype(np.float32), rng.integers(1, 6, size=B).astype(np.float32)]
    torch.manual_seed(B)
    module = spVIPESmodule({0: G0, 1: G1}, use_labels=True, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=0.1, precision=precision).to(dev)
    tensors = []
    for g in range(2):
        X = np.zeros((B, G0 + G1), np.float32)
        X[:, (0 if g == 0 else G0):(G0 if g == 0 else G0 + G1)] = counts_h[g]
        tensors.append({"X": torch.tensor(X).to(dev), "batch": torch.zeros(B, 1, device=dev), "groups": torch.full((B, 1), float(g), device=dev),
                        "indices": torch.arange(B, dtype=torch.float32, device=dev).unsqueeze(1), "labels": torch.tensor(labels_h[g], device=dev).unsqueeze(1)})
    module.train()
    for _ in range(3):   # move the running statistics of every BatchNorm away from their initial values
        module(tuple(tensors))
    module.eval()
    sd = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    gen = torch.Generator().manual_seed(4)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen) for g in range(2) for k, n in (("private", n_p), ("shared", n_s))}
    noise.update({f"poe_{g}": torch.randn(B, n_s, generator=gen) for g in range(2)})
    with torch.no_grad():
        inf, _, lo = module(tuple(tensors), inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}})
    want = O.forward_loss(sd, [torch.tensor(c) for c in counts_h], n_dimensions_shared=n_s, n_dimensions_private=n_p, noise=noise, mode="label",
                          labels=[torch.tensor(l) for l in labels_h], training=False, kl_weight=1.0)
    tol = 2e-4 if precision == "fp32" else 2e-3
    got, ref = float(lo.loss), float(want["loss"])
    assert abs(got - ref) / abs(ref) < tol, (got, ref)
    rec = list(lo.reconstruction_loss.values())
    for g in range(2):
        torch.testing.assert_close(rec[g].cpu(), want["reconstruction_loss"][g], rtol=5 * tol, atol=5 * tol * float(want["reconstruction_loss"][g].abs().max()))
        lat = dict(rtol=1e-3, atol=2e-4) if precision == "fp32" else dict(rtol=5e-2, atol=5e-2)
        torch.testing.assert_close(inf["poe_stats"][g]["logtheta_loc"].cpu(), want["poe_stats"][g]["logtheta_loc"], **lat)
