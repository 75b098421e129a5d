"""CPU: the bf16-mode rounding reference (tests/_bf16_reference.py) itself.

Bridge: with rounding off it is plain float64 and must reproduce oracle.spvipes_oracle.forward_loss -- loss, per-cell terms, BatchNorm
running statistics and every autograd gradient -- to 1e-10 relative, on every golden case (label / paired / cluster PoE, eval mode,
dropout, batch covariates).  Its hand-written decoder backward is thereby checked against autograd.  With rounding on it must stay
within today's bf16-mode bounds of the unrounded oracle (ELBO 2e-3: test_gpu_shape_sweep.py; gradients 6e-2 relative L2:
test_gpu_batch_covariates.py).

Sensitivity: at every shape the GPU tests use, each injected kernel defect (a zeroed last cell row of dL / tP / tS, the last partial
32-gene tile missing from the latent gradients, cell rows 128 and above missing from a weight-gradient contraction, dL not rounded
to bf16) must move at least one checked metric past twice its bound: the bounds of BOUNDS_DECODER / BOUNDS_STEP are tight enough
to see a subtly wrong kernel.

Flip noise: the gene rows of the three cell-contracted decoder weight gradients carry one-ulp bf16 rounding flips that no kernel
can avoid (the kernel's fp32 value and the float64 value straddle a rounding midpoint).  Jittering the reference's own values by
1e-6 before each bf16 rounding shows that floor and that their separate row bound sits above it; their tensor-wide l2 bound, where
single flips average out, is what sees a missed dL rounding at the whole-step shapes.
"""
import numpy as np
import pytest
import torch

from oracle import spvipes_oracle as O
from tests import _bf16_reference as R
from tests._golden import LOSS_CASES, Golden
from tests._step_inputs import sweep_inputs
from tests.test_gpu_bf16_decoder import CASES as DECODER_CASES
from tests.test_gpu_bf16_step import SWEEP


def _golden_run(gd, fn, **extra):
    sd = gd.state_dict(torch.float64)
    leaves = {k: sd[k].clone().requires_grad_(True) for k in O.param_names(sd)}
    sd.update(leaves)
    out = fn(sd, gd.counts(torch.float64), n_dimensions_shared=gd.n_s, n_dimensions_private=gd.n_p, noise=gd.noise(torch.float64), mode=gd.mode,
             kl_weight=gd.kl_weight, training=gd.training, dropout_rate=gd.dropout, dropout_masks=gd.dropout_masks(torch.float64),
             update_running_stats=True, **gd.poe_inputs(torch.float64), **gd.batch_kwargs(), **extra)
    if gd.training:
        out["loss"].backward()
    return out, {k: v.grad for k, v in leaves.items()}


def _grad_scale(grads):
    return max(float(v.abs().max()) for v in grads.values() if v is not None)


@pytest.mark.parametrize("case", LOSS_CASES)
def test_reference_without_rounding_is_the_oracle(case):
    gd = Golden(case)
    want, gw = _golden_run(gd, O.forward_loss)
    got, gg = _golden_run(gd, R.forward_loss, rounding=False)
    rel = lambda a, b, s=None: float((a - b).abs().max()) / max(float(b.abs().max()) if s is None else s, 1e-300)
    assert rel(got["loss"].detach(), want["loss"].detach()) < 1e-10
    for g in range(2):
        assert rel(got["reconstruction_loss"][g], want["reconstruction_loss"][g].detach()) < 1e-10
        for k in ("private", "poe"):
            assert rel(got["kl_local"][f"{k}_{g}"].detach(), want["kl_local"][f"{k}_{g}"].detach()) < 1e-10
        assert rel(got["poe_stats"][g]["logtheta_loc"].detach(), want["poe_stats"][g]["logtheta_loc"].detach()) < 1e-10
    ns_w, ns_g = want["new_running_stats"] or {}, got["new_running_stats"] or {}
    assert sorted(ns_w) == sorted(ns_g)
    for k in ns_w:
        assert rel(ns_g[k], ns_w[k]) < 1e-10, k
    if gd.training:
        # (biases in front of a training-mode BatchNorm have a gradient that is zero up to rounding: their scale is floored at 1e-3 of
        # the largest gradient)
        floor = 1e-3 * _grad_scale(gw)
        for k, v in gw.items():
            assert (v is None) == (gg[k] is None), k
            if v is not None:
                assert rel(gg[k], v, max(float(v.abs().max()), floor)) < 1e-10, k


@pytest.mark.parametrize("case", LOSS_CASES)
def test_rounding_reference_stays_within_bf16_bounds_of_the_oracle(case):
    gd = Golden(case)
    want, gw = _golden_run(gd, O.forward_loss)
    got, gg = _golden_run(gd, R.forward_loss, rounding=True)
    assert abs(float(got["loss"]) - float(want["loss"])) / abs(float(want["loss"])) < 2e-3
    if gd.training:
        floor = 1e-3 * _grad_scale(gw)
        for k, v in gw.items():
            if v is None:
                continue
            scale = max(float(v.norm()), floor)
            assert float((gg[k] - v).norm()) / scale < 6e-2, k


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------
def _defects_for(B):
    return [d for d in R.DEFECTS if not (d == "drop_cells_128" and B <= 128)]   # (no cell rows past 128 to drop)


def _decoder_inputs(case):
    """float64 inputs shaped like the GPU decoder test's case (random values of the same kinds)"""
    name, B, Gs, n_s, n_p, extra = case
    nb = extra.get("n_batch", 0)
    gen = torch.Generator().manual_seed(B + sum(Gs))
    rng = np.random.default_rng(B)
    a, b = n_p + nb, n_s + nb
    lat, pars, xs, libs, bufs = [], [], [], [], []
    for G in Gs:
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        lat.append((rn(B, a).requires_grad_(True), rn(B, b).requires_grad_(True)))
        n_m = 256
        par = [rn(G, a) / a ** 0.5, 1 + 0.2 * rn(G), 0.1 * rn(G), rn(G, b) / b ** 0.5, 1 + 0.2 * rn(G), 0.1 * rn(G),
               rn(n_m, a + b) / (a + b) ** 0.5, 0.1 * rn(n_m), 1 + 0.2 * rn(n_m), 0.1 * rn(n_m), rn(G, n_m + a + b) / (n_m + a + b) ** 0.5,
               0.1 * rn(G), rn(G)]
        pars.append([p.requires_grad_(True) for p in par])
        X = (rng.poisson(3.0, size=(B, G)) * (rng.random((B, G)) < 0.35)).astype(np.float32)
        X[:, 0] += 1
        x = torch.log1p(torch.tensor(X))
        xs.append(x.double())
        libs.append(torch.log(x.sum(1)).unsqueeze(1).double())
        bufs.append({k: (0.2 * rn(n), 0.5 + rn(n).abs()) for k, n in (("p", G), ("s", G), ("a", n_m))})
    return lat, pars, xs, libs, bufs


def _decoder_metrics(case, defects):
    lat, pars, xs, libs, bufs = _decoder_inputs(case)
    B = case[1]
    loss, rec, _ = R.decoder_fused(lat, pars, xs, libs, torch.full((B,), 1.0 / B, dtype=torch.float64), training=True, buffers=bufs,
                                   defects=frozenset(defects))
    loss.backward()
    out = {"loss": loss.detach()}
    for g in range(len(lat)):
        out[f"rec{g}"] = rec[g].reshape(-1, 1)
        out[f"lat{g}"] = torch.cat([lat[g][0].grad, lat[g][1].grad], 1)
        for j, p in enumerate(pars[g]):
            out[f"par{g}.{j}"] = p.grad
    return out


def _kind_decoder(key):
    if key.startswith("par"):
        return "weight" if int(key.split(".")[1]) in (0, 1, 2, 3, 4, 5, 10, 11) else "param"   # the regressors and the mixture layer
    return "loss" if key == "loss" else "rec" if key.startswith("rec") else "latent"


def _ratio(m, b):
    """the largest metric / bound ratio of one tensor"""
    bm = b if isinstance(b, dict) else {"max": b, "row": b, "l2": b}
    return max(m[k] / bm[k] for k in ("max", "row", "l2"))


@pytest.mark.parametrize("case", DECODER_CASES, ids=[c[0] for c in DECODER_CASES])
def test_decoder_bounds_see_every_injected_defect(case):
    clean = _decoder_metrics(case, ())
    for d in _defects_for(case[1]):
        bad = _decoder_metrics(case, (d,))
        ratio = 0.0
        for k, ref in clean.items():
            ratio = max(ratio, _ratio(R.metrics(bad[k], ref), R.BOUNDS_DECODER[_kind_decoder(k)]))
        assert ratio > 2.0, f"{case[0]}: defect {d} moves no checked metric past twice its bound (worst ratio {ratio:.2f})"


def _step_metrics(case, defects):
    B, G0, G1, H, n_s, n_p, cdt = case
    counts_h, labels_h, rows_h, noise = sweep_inputs(case)
    sd = O.init_state_dict([G0, G1], n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p, seed=B)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    leaves = {k: sd[k].requires_grad_(True) for k in O.param_names(sd)}
    out = R.forward_loss(sd, [torch.tensor(c[r]).double() for c, r in zip(counts_h, rows_h)], n_dimensions_shared=n_s, n_dimensions_private=n_p,
                         noise={k: v.double() for k, v in noise.items()}, mode="label", labels=[torch.tensor(l[r]).double() for l, r in zip(labels_h, rows_h)],
                         training=True, kl_weight=0.7, defects=frozenset(defects))
    out["loss"].backward()
    res = {"loss": out["loss"].detach()}
    for g in range(2):
        res[f"rec{g}"] = out["reconstruction_loss"][g].reshape(-1, 1)
    res.update({"d " + k: v.grad for k, v in leaves.items() if v.grad is not None})
    return res


def _kind_step(key):
    if key.startswith("d "):
        return "weight" if R.is_cell_contracted_weight(key[2:]) else "param"
    return "loss" if key == "loss" else "rec"


@pytest.mark.parametrize("case", SWEEP, ids=[f"B{c[0]}-G{c[1]}x{c[2]}" for c in SWEEP])
def test_step_bounds_see_every_injected_defect(case):
    clean = _step_metrics(case, ())
    gmax = max(float(v.abs().max()) for k, v in clean.items() if k.startswith("d "))
    for d in _defects_for(case[0]):
        bad = _step_metrics(case, (d,))
        ratio = 0.0
        for k, ref in clean.items():
            if k.startswith("d ") and float(ref.abs().max()) < 1e-9 * gmax:
                continue   # zero by construction
            ratio = max(ratio, _ratio(R.metrics(bad[k], ref), R.BOUNDS_STEP[_kind_step(k)]))
        assert ratio > 2.0, f"B{case[0]}: defect {d} moves no checked metric past twice its bound (worst ratio {ratio:.2f})"


def test_weight_gene_rows_carry_one_ulp_flip_noise(monkeypatch):
    """the reason BOUNDS_STEP / BOUNDS_DECODER give the cell-contracted decoder weight gradients their own row bound: two references
    whose values before each bf16 rounding differ by 1e-6 relative (less than the kernels' fp32 evaluation differs from float64)
    already disagree by more than 3e-3 in some gene row (single one-ulp flips in rows a few cells dominate), and by less than the
    row bound those gradients get"""
    bf16 = R.bf16
    noise = {"weight": {"row": 0.0, "l2": 0.0}, "param": {"row": 0.0, "l2": 0.0}}
    for case in SWEEP:
        clean = _step_metrics(case, ())
        gen = torch.Generator().manual_seed(case[0])
        monkeypatch.setattr(R, "bf16", lambda t: bf16(t * (1 + 1e-6 * torch.randn(t.shape, generator=gen, dtype=t.dtype))))
        jit = _step_metrics(case, ())
        monkeypatch.setattr(R, "bf16", bf16)
        gmax = max(float(v.abs().max()) for k, v in clean.items() if k.startswith("d "))
        for k, ref in clean.items():
            if not k.startswith("d ") or float(ref.abs().max()) < 1e-9 * gmax:
                continue
            m, kind = R.metrics(jit[k], ref), _kind_step(k)
            for q in ("row", "l2"):
                noise[kind][q] = max(noise[kind][q], m[q])
    assert noise["weight"]["row"] > 3e-3, noise
    assert noise["weight"]["row"] < R.BOUNDS_STEP["weight"]["row"], noise
