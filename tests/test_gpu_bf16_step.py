"""GPU: one whole training step in bf16 mode (Trainer -> spVIPESmodule -> EncoderFC1 on the resident f16 log1p image / encoder
tails / PoE / DecoderFused) against a float64 reference that rounds where bf16 mode rounds (tests/_bf16_reference.py), on the same
parameters, minibatch rows and noise.  Today's bf16 checks of the whole step compare with the UNROUNDED oracle: the ELBO only
(test_gpu_shape_sweep.py, 2e-3), or the gradients at 3e-2 relative L2 (test_gpu_fullsize_parity.py).  Against the rounding
reference the ELBO, per-cell reconstruction and KL terms, the private and PoE latent means and EVERY parameter gradient are held to
bounds one to two orders tighter.

Cases: the shape-sweep cases (tests/_step_inputs.py, label PoE, resident counts), C1's shape (B 128, G 2000, H 64,
10 / 5), and every golden case of tests/_golden.py LOSS_CASES (label / paired / cluster PoE, eval mode, dropout, batch
covariates) through the module's own API on the golden's inputs.

Bounds (tests/_bf16_reference.py: BOUNDS_STEP) against the worst value measured on the MI355X over all cases (metrics as in
tests/test_gpu_bf16_decoder.py):
  quantity                                   bound max / row / l2        measured max / row / l2
  ELBO                                       1.1e-6                      2.8e-7
  rec per cell                               3.2e-5 / 3.5e-5 / 3e-6      8.2e-6 / 8.8e-6 / 7.7e-7
  KL per cell                                1.2e-4 / 1.9e-4 / 4.3e-5    3.0e-5 / 4.9e-5 / 1.1e-5
  private / PoE latent means                 1.9e-4 / 3e-4 / 5.3e-5      4.8e-5 / 8.2e-5 / 1.3e-5
  encoders, mixing trunk, px_r gradients     1.5e-3 / 3e-3 / 1.3e-3      3.9e-4 / 2.0e-3 / 3.4e-4
  factor regressor and mixture gradients     6.5e-3 / 1.5e-2 / 7e-4      1.6e-3 / 3.9e-3 / 3.6e-4
The last row's row bound covers one-ulp bf16 flips in gene rows that a few cells dominate (worst: d mixture weight, B 70 / G 301;
test_bf16_reference_cpu.py::test_weight_gene_rows_carry_one_ulp_flip_noise shows the reference itself moves by up to 6e-3 there
under a 1e-6 perturbation); its l2 bound is what sees a missed dL rounding at these shapes.
Gradients that are zero by construction (biases in front of a training-mode BatchNorm) are held to the same bound relative to the
largest gradient of the step.
"""
import numpy as np
import pytest
import torch

from tests import _bf16_reference as R
from tests._golden import LOSS_CASES, Golden
from tests._step_inputs import _move_relu_kinks_away, _move_trunk_kinks_away, sweep_inputs

pytestmark = pytest.mark.gpu

SWEEP = [  # B, G0, G1, H, n_s, n_p, counts dtype (test_gpu_shape_sweep.CASES, and C1's shape last)
    (5, 20, 20, 8, 3, 2, "u16"),
    (37, 45, 51, 16, 6, 3, "f32"),
    (100, 333, 200, 64, 25, 10, "u16"),
    (130, 1000, 777, 128, 12, 15, "u16"),
    (64, 2001, 35, 32, 31, 4, "f32"),
    (200, 129, 257, 256, 10, 5, "u16"),
    (33, 100, 90, 50, 7, 3, "u16"),
    (257, 64, 4100, 24, 31, 15, "u16"),
    (70, 301, 150, 32, 8, 4, "f32frac"),
    (128, 2000, 2000, 64, 10, 5, "u16"),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def compare_step(name, inf, lo, module, ref_out, leaves, B, bounds=R.BOUNDS_STEP, training=True):
    """the metrics of one step against the reference; returns the failures"""
    bad, rep = [], {}
    bad += R.check("elbo", lo.loss.detach().cpu(), ref_out["loss"].detach(), bounds["loss"], rep)
    recs = list(lo.reconstruction_loss.values())
    for g in range(2):
        bad += R.check(f"rec{g}", recs[g].detach().cpu().reshape(-1, 1), ref_out["reconstruction_loss"][g].reshape(-1, 1), bounds["rec"], rep)
        bad += R.check(f"kl_private{g}", lo.kl_local[f"kl_divergence_groups_{g + 1}_private"].detach().cpu().reshape(-1, 1), ref_out["kl_local"][f"private_{g}"].detach().reshape(-1, 1),
                       bounds["kl"], rep)
        bad += R.check(f"kl_poe{g}", lo.kl_local[f"kl_divergence_groups_{g + 1}_poe"].detach().cpu().reshape(-1, 1), ref_out["kl_local"][f"poe_{g}"].detach().reshape(-1, 1),
                       bounds["kl"], rep)
        bad += R.check(f"private_loc{g}", inf["private_stats"][g]["logtheta_loc"].detach().cpu(), ref_out["private_stats"][g]["logtheta_loc"].detach(),
                       bounds["latent_mean"], rep)
        bad += R.check(f"poe_loc{g}", inf["poe_stats"][g]["logtheta_loc"].detach().cpu(), ref_out["poe_stats"][g]["logtheta_loc"].detach(),
                       bounds["latent_mean"], rep)
    if training:
        gmax = max(float(v.grad.abs().max()) for v in leaves.values() if v.grad is not None)
        for k, p in module.named_parameters():
            ref = leaves[k].grad
            got = (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu()
            if ref is None or float(ref.abs().max()) < 1e-9 * gmax:   # zero by construction
                e = float(got.abs().max()) / gmax
                rep["d " + k] = {"max": e, "row": e, "l2": e}
                if not e <= bounds["param"]["max"]:
                    bad.append(f"d {k}: {e:.3e} of the largest gradient (zero by construction)")
                continue
            bad += R.check("d " + k, got, ref, bounds["weight" if R.is_cell_contracted_weight(k) else "param"], rep)
    worst = {k: max(v["max"], v["row"]) for k, v in rep.items()}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"\n[bf16-step] {name} worst: " + ", ".join(f"{k} {v:.2e}" for k, v in top))
    return bad


@pytest.mark.parametrize("case", SWEEP, ids=[f"B{c[0]}-G{c[1]}x{c[2]}-H{c[3]}-s{c[4]}p{c[5]}-{c[6]}" for c in SWEEP])
def test_training_step_bf16_matches_rounding_reference(dev, case):
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.ops import GroupCounts
    from spvipes_amd.train import Trainer
    B, G0, G1, H, n_s, n_p, cdt = case
    counts_h, labels_h, rows_h, noise = sweep_inputs(case)
    torch.manual_seed(B)
    module = spVIPESmodule({0: G0, 1: G1}, use_labels=True, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=0.0, precision="bf16").to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    _move_relu_kinks_away(sd, [c[r] for c, r in zip(counts_h, rows_h)], fc1_image=True)
    c64 = [torch.tensor(c[r]).double() for c, r in zip(counts_h, rows_h)]
    labels = [torch.tensor(l[r]).double() for l, r in zip(labels_h, rows_h)]
    noise64 = {k: v.double() for k, v in noise.items()}
    kw = dict(n_dimensions_shared=n_s, n_dimensions_private=n_p, noise=noise64, mode="label", labels=labels, training=True, kl_weight=0.7)
    _move_trunk_kinks_away(sd, lambda sd64: R.forward_loss(sd64, c64, **kw), n_s, n_p)
    module.load_state_dict(sd)
    to_dev = (lambda c: torch.tensor(c.astype(np.uint16).view(np.int16)).to(dev)) if cdt == "u16" else (lambda c: torch.tensor(c).to(dev))
    counts = [GroupCounts(to_dev(c), c.shape[1], 0, resident=True) for c in counts_h]
    trainer = Trainer(module, counts, labels=[torch.tensor(l, device=dev) for l in labels_h])
    module.train()
    rows = [torch.tensor(r, device=dev) for r in rows_h]
    inf, _, lo = module(trainer.minibatch(rows), inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}}, loss_kwargs={"kl_weight": 0.7})
    lo.loss.backward()
    torch.cuda.synchronize()
    params = dict(module.named_parameters())
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items() if k in params}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    sd64.update(leaves)
    out = R.forward_loss(sd64, c64, **kw)
    out["loss"].backward()
    bad = compare_step(f"sweep B{B} G{G0}x{G1}", inf, lo, module, out, leaves, B)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("case", LOSS_CASES)
def test_golden_case_bf16_matches_rounding_reference(dev, case):
    """the golden cases' inputs through the module in bf16 mode (the golden test itself checks bf16 mode on the ELBO and the latent
    means only): ELBO, per-cell terms, latent means and, in training, every gradient against the rounding reference"""
    from tests.test_gpu_parity import _build
    g = Golden(case)
    m, tensors, noise, dm = _build(g, dev, "bf16")
    inf, _, lo = m(tensors, inference_kwargs={"noise": noise, "dropout_masks": dm}, loss_kwargs={"kl_weight": g.kl_weight})
    if g.training:
        lo.loss.backward()
    torch.cuda.synchronize()
    sd = g.state_dict(torch.float64)
    params = dict(m.named_parameters())
    leaves = {k: sd[k].clone().requires_grad_(True) for k in params}
    sd.update(leaves)
    out = R.forward_loss(sd, g.counts(torch.float64), n_dimensions_shared=g.n_s, n_dimensions_private=g.n_p, noise=g.noise(torch.float64),
                         mode=g.mode, kl_weight=g.kl_weight, training=g.training, dropout_rate=g.dropout, dropout_masks=g.dropout_masks(torch.float64),
                         **g.poe_inputs(torch.float64), **g.batch_kwargs())
    if g.training:
        out["loss"].backward()
    bad = compare_step(f"golden {case}", inf, lo, m, out, leaves, g.raw["in/counts0"].shape[0], training=g.training)
    assert not bad, "; ".join(bad)
