"""Inputs and kink helpers of the whole-step GPU tests (tests/test_gpu_shape_sweep.py, tests/test_gpu_bf16_step.py): the sweep's
minibatches and noise, and the parameter shifts that keep every rectifier input away from zero."""
import numpy as np
import torch


def sweep_inputs(case):
    """(counts_h, labels_h, rows_h, noise) of one shape-sweep case (B, G0, G1, H, n_s, n_p, counts dtype): B + 11 cells per group with a
    few counts beyond the lgamma table (non-integral ones for "f32frac"), labels, B random rows per group and the standard-normal draws"""
    B, G0, G1, H, n_s, n_p, cdt = case
    rng = np.random.default_rng(B * 7 + G0)
    Gs = (G0, G1)
    n_cells = B + 11
    counts_h = [(rng.poisson(3.0, size=(n_cells, G)) * (rng.random((n_cells, G)) < 0.35)).astype(np.float32) for G in Gs]
    for c in counts_h:
        c[:, 0] += 1
        c[rng.integers(0, n_cells, 4), rng.integers(0, c.shape[1], 4)] += 90.0   # a few counts beyond the lgamma table
    if cdt == "f32frac":
        counts_h = [(c * rng.uniform(0.3, 1.7, size=c.shape)).astype(np.float32) for c in counts_h]
    labels_h = [rng.integers(0, 4, size=n_cells).astype(np.float32), rng.integers(1, 6, size=n_cells).astype(np.float32)]
    rows_h = [rng.permutation(n_cells)[:B].astype(np.int32) for _ in range(2)]
    gen = torch.Generator().manual_seed(1)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen) for g in range(2) for k, n in (("private", n_p), ("shared", n_s))}
    noise.update({f"poe_{g}": torch.randn(B, n_s, generator=gen) for g in range(2)})
    return counts_h, labels_h, rows_h, noise


def _move_relu_kinks_away(sd, counts_rows, margin=1e-4, fc1_image=False):
    """Gradient checks between two fp32 implementations are ill-posed where a ReLU input is within rounding error of
    zero (one flipped (cell, unit) mask changes a whole row of a weight gradient).  Shift each hidden unit's bias by the
    smallest step that keeps every cell's fc1 / fc2 pre-activation at least `margin` away from zero (evaluated in
    float64); both implementations then load the same shifted parameters.  ``fc1_image``: evaluate fc1 on the f16 operand images
    bf16 mode contracts (tests/_bf16_reference.py) instead of the exact operands."""
    for g, c in enumerate(counts_rows):
        x = torch.log1p(torch.tensor(c, dtype=torch.float64))
        if fc1_image:
            x = torch.log1p(torch.tensor(c, dtype=torch.float32)).half().double()
        for kind in ("private", "shared"):
            h = x
            for layer in ("fc1", "fc2"):
                W, b = sd[f"encoder_{g}_{kind}.{layer}.weight"], sd[f"encoder_{g}_{kind}.{layer}.bias"]
                Wd = (W.float() * 256.0).half().double() / 256.0 if (fc1_image and layer == "fc1") else W.double()
                pre = h @ Wd.T + b.double()
                cand = torch.arange(0, 400, dtype=torch.float64) * (2.5 * margin)                  # [S] candidate shifts
                ok = ((pre.unsqueeze(0) + cand.view(-1, 1, 1)).abs() > margin).all(dim=1)             # [S, units]
                assert bool(ok.any(dim=0).all())
                shift = cand[ok.double().argmax(dim=0)]
                b += shift.float()
                h = torch.relu(pre + shift)


def _move_trunk_kinks_away(sd, forward64, n_s, n_p, margin=1e-4):
    """The same for the decoder's mixing trunk relu(BN(zcat W_a^T + b_a)): its input depends on the sampled latents, so the
    oracle is run once in float64 (``forward64(sd64) -> forward_loss output``) and each unit's BatchNorm bias is shifted
    by the smallest step that keeps every cell's pre-activation `margin` away from zero (a bias shift changes nothing
    upstream)."""
    import torch.nn.functional as F
    from oracle import spvipes_oracle as O
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    out = forward64(sd64)
    L = "fc_layers.Layer 0"
    for g in range(2):
        zp, zs = O.split_latents(out["private_stats"][g]["log_z"], out["poe_stats"][g]["logtheta_log_z"], n_s, n_p)
        zcat = torch.cat([zp, zs], dim=1)
        pre = O.batch_norm(F.linear(zcat, sd64[f"decoder_{g}.sigmoid_decoder.{L}.0.weight"], sd64[f"decoder_{g}.sigmoid_decoder.{L}.0.bias"]),
                           sd64, f"decoder_{g}.sigmoid_decoder.{L}.1", True, **O.BN_DEC).detach()
        cand = torch.arange(0, 400, dtype=torch.float64) * (2.5 * margin)
        ok = ((pre.unsqueeze(0) + cand.view(-1, 1, 1)).abs() > margin).all(dim=1)
        assert bool(ok.any(dim=0).all())
        sd[f"decoder_{g}.sigmoid_decoder.{L}.1.bias"] += cand[ok.double().argmax(dim=0)].float()
