"""TEST INFRASTRUCTURE ONLY -- a float64 restatement of ONE step in bf16 precision mode that rounds at exactly the places the HIP
kernels round, so that a bf16-mode result can be held to bounds one to two orders tighter than against the unrounded oracle.

Rounding sites (all round-to-nearest-even: f2bf / f2h in csrc/spv_common.h, the same as torch's CPU .to(bfloat16 / float16)):

  encoder fc1 (csrc/spv_fc1.h, ops.EncoderFC1)
    x image        f16(fp32 log1p(count))
    weight image   f16(W * 256) / 256                              (SPV_FC1_W_SCALE)
    dh image       f16(dpre * s) / s, s = the power of two that puts max |dpre| in [4096, 8192) -- ONE scale per group, over the
                   [B, 2H] pre-activation gradient of its private AND shared encoder (spv_enc_fc1_bwd_prep: N1 = 2H)
    bias gradient, covariate columns and every small layer (spv_linear_*): fp32, not rounded
  decoder forward (csrc/spv_decoder.h)
    y_k            hi / lo split images of the BatchNorm-folded [W'_k | c_k] and of [z_k | 1]; the product is hi*lo + lo*hi + hi*hi
    logits         f16( bf16([m | z | 1]) . bf16([W_m | b_m]) )     (the trunk kernel writes m into the bf16 image)
  likelihood (dec_nb_kernel)
    dL, tP, tS     stored as bf16, the row weight -w_b already folded in; the row sums T_p, T_s and d theta from the unrounded values
  one-pass backward (spv_dec_heads_bwd, the default bf16 route; the split-K and in-place routes compute the same products)
    corrected tile bf16( bf16(tP) - softmax * T_p )   (and the shared head), itself the MFMA operand of both contractions below
    d z (rate heads)   corrected tile . bf16(W')        (the hi plane only)
    d [W' | c]         corrected tile^T . bf16([z | 1]) (the hi plane only)
  mixture GEMMs        d W_m = bf16(dL)^T . bf16(A_m),  d A_m = bf16(dL) . bf16([W_m | b_m])
  everything downstream (fold backward, trunk, latent slicing, PoE, BatchNorm, KL): fp32, not rounded

``rounding=False`` turns every site off: the reference is then plain float64 and must agree with oracle.spvipes_oracle.forward_loss
and its autograd gradients (tests/test_bf16_reference_cpu.py).  ``defects`` injects the kernel mistakes the sensitivity test uses
(DEFECTS below) into the likelihood / backward boundary.

The bounds the GPU tests hold the kernels to live here too (BOUNDS_DECODER, BOUNDS_STEP), so that the CPU sensitivity test checks
the very numbers the GPU tests assert.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import spvipes_oracle as O

FC1_W_SCALE = 256.0
BN_EPS, BN_MOM = O.BN_DEC["eps"], O.BN_DEC["momentum"]
L = "fc_layers.Layer 0"

# the kernel mistakes the sensitivity test injects (tests/test_bf16_reference_cpu.py)
DEFECTS = ("zero_last_cell", "drop_last_gene_tile", "drop_cells_128", "unrounded_dL")

# ---- bounds (measured on the MI355X: see the tables in tests/test_gpu_bf16_decoder.py / tests/test_gpu_bf16_step.py) -------------
# metrics(): "max" tensor-wide, "row" worst gene / cell row (vectors: worst element), "l2" tensor-wide relative L2.
# "weight": the decoder gradients whose gene rows (elements, for [G] vectors) are contractions over the minibatch's cells of
# bf16-rounded operands: the factor regressors' weight, gamma and beta (the corrected tile) and the mixture weight and bias (dL).  Where the kernel's fp32 value and the float64 value
# straddle a bf16 rounding midpoint the two round one ulp (2^-8) apart; in a gene row that a few cells dominate one such flip
# moves the row by a few 1e-3 -- test_bf16_reference_cpu.py::test_weight_gene_rows_carry_one_ulp_flip_noise measures that floor on
# the reference itself.  Their rows get their own bound; their tensor-wide l2 error, where the flips average out, stays tight.
BOUNDS_DECODER = {
    "loss": 8e-7,
    "rec": {"max": 7e-6, "row": 7.9e-6, "l2": 8e-7},
    "latent": {"max": 1e-3, "row": 3e-3, "l2": 2.5e-4},      # d private_log_z, d poe_log_z
    "param": {"max": 5e-4, "row": 9.6e-4, "l2": 2.4e-4},     # d W_a, b_a, gamma_a, beta_a, px_r
    "weight": {"max": 1.9e-3, "row": 8e-3, "l2": 2.8e-4},    # d W_p, gamma_p, beta_p, W_s, gamma_s, beta_s, W_m, b_m
    "buffer": {"max": 3.6e-7, "row": 4.8e-7, "l2": 1.7e-7},  # BatchNorm running statistics after the forward pass
}
BOUNDS_STEP = {
    "loss": 1.1e-6,
    "rec": {"max": 3.2e-5, "row": 3.5e-5, "l2": 3e-6},
    "kl": {"max": 1.2e-4, "row": 1.9e-4, "l2": 4.3e-5},
    "latent_mean": {"max": 1.9e-4, "row": 3e-4, "l2": 5.3e-5},   # private and PoE logtheta_loc
    "param": {"max": 1.5e-3, "row": 3e-3, "l2": 1.3e-3},          # encoders, mixing trunk, px_r
    "weight": {"max": 6.5e-3, "row": 1.5e-2, "l2": 7e-4},         # decoder_{g}.factor_regressor_*, decoder_{g}.mixture
}


def is_cell_contracted_weight(name: str) -> bool:
    """a state_dict name of one of the "weight" gradients above"""
    return name.startswith("decoder_") and ("factor_regressor" in name or "mixture" in name)


# ---- rounding helpers -------------------------------------------------------------------------------------------------------
def bf16(t: torch.Tensor) -> torch.Tensor:
    """what a bf16 image holds of an fp32 value (float64 in, float64 out)"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def f16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def split_bf16(t: torch.Tensor):
    """the hi / lo operand planes of a split-bf16 image (split_bf16 in csrc/spv_common.h): hi = bf16(v), lo = bf16(v - hi)"""
    v = t.to(torch.float32)
    hi = v.to(torch.bfloat16)
    lo = (v - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.to(torch.float64), lo.to(torch.float64)


def split_mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a . b^T as the split-bf16 MFMAs form it: hi*lo + lo*hi + hi*hi"""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    return ah @ bl.t() + al @ bh.t() + ah @ bh.t()


def dh_scale(dpre: torch.Tensor) -> float:
    """the per-step power of two of the f16 dh image: max |dpre| lands in [4096, 8192) (csrc/spv_common.h: pow2_scale_for)"""
    amax = float(dpre.abs().max())
    return 1.0 if amax == 0.0 else 2.0 ** (13 - math.frexp(amax)[1])


# ---- metrics ------------------------------------------------------------------------------------------------------------------
def metrics(got: torch.Tensor, ref: torch.Tensor) -> Dict[str, float]:
    """{"max": max |got - ref| / max |ref|,
        "row": worst per-row relative L2 error (gene row of a [G, k] tensor, cell row of a [B, k] tensor; row norms floored at 1e-3
               of the tensor norm); a 1-D tensor is scored element by element, each element floored at the vector's RMS,
        "l2":  ||got - ref|| / ||ref|| over the whole tensor}"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.dim() == 0:
        e = float((got - ref).abs() / ref.abs().clamp(min=1e-300))
        return {"max": e, "row": e, "l2": e}
    d = got - ref
    amax = float(ref.abs().max())
    emax = float(d.abs().max()) / amax if amax > 0 else float(d.abs().max())
    l2 = float(d.norm()) / max(float(ref.norm()), 1e-300)
    if ref.dim() == 1:
        floor = max(float(ref.norm()) / ref.numel() ** 0.5, 1e-300)
        row = float((d.abs() / ref.abs().clamp(min=floor)).max())
    else:
        g2, r2 = d.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1)
        floor = max(1e-3 * float(r2.norm()), 1e-300)
        row = float((g2.norm(dim=1) / r2.norm(dim=1).clamp(min=floor)).max())
    return {"max": emax, "row": row, "l2": l2}


def check(name: str, got, ref, bound, report: Optional[dict] = None) -> list:
    """metrics of one tensor against its bound ({"max": .., "row": .., "l2": ..} or a scalar); returns the failures as strings"""
    m = metrics(torch.as_tensor(got), torch.as_tensor(ref))
    if report is not None:
        report[name] = m
    if not isinstance(bound, dict):
        bound = {"max": bound, "row": bound, "l2": bound}
    return [f"{name}: {k} {m[k]:.3e} > {bound[k]:.1e}" for k in ("max", "row", "l2") if not m[k] <= bound[k]]


# ---- encoder fc1 ----------------------------------------------------------------------------------------------------------------
class _Fc1(torch.autograd.Function):
    """x_img . W^T for BOTH encoders of a group (W = [W_private; W_shared], [2H, G]); backward: the weight gradient from the f16 dh
    image with one power-of-two scale over the whole [B, 2H] gradient (no input gradient: x is data)"""

    @staticmethod
    def forward(ctx, x_img, W, rounding: bool):
        Wr = f16(W * FC1_W_SCALE) / FC1_W_SCALE if rounding else W
        ctx.save_for_backward(x_img)
        ctx.rounding = rounding
        return x_img @ Wr.t()

    @staticmethod
    def backward(ctx, dpre):
        (x_img,) = ctx.saved_tensors
        if ctx.rounding:
            s = dh_scale(dpre)
            dpre = f16(dpre * s) / s
        return None, dpre.t() @ x_img, None


def fc1_pair(x: torch.Tensor, sd, g: int, one_hot, rounding: bool):
    """pre-activations of fc1 of encoder_{g}_private and encoder_{g}_shared: {kind: [B, H]}"""
    ws = [sd[f"encoder_{g}_{k}.fc1.weight"] for k in ("private", "shared")]
    H, G = ws[0].shape[0], x.shape[1]
    x_img = f16(x) if rounding else x
    pre = _Fc1.apply(x_img, torch.cat([w[:, :G] for w in ws], 0), rounding)
    out = {}
    for i, k in enumerate(("private", "shared")):
        p = pre[:, i * H:(i + 1) * H] + sd[f"encoder_{g}_{k}.fc1.bias"]
        if one_hot is not None:   # covariate columns: fp32 in the kernels' epilogue
            p = p + one_hot @ ws[i][:, G:].t()
        out[k] = p
    return out


def encoder_tail(sd, prefix: str, pre1, eps, training, dropout_rate=0.0, dropout_mask=None, new_stats=None):
    """oracle.encoder_forward from the fc1 pre-activation on"""
    h = F.relu(pre1)
    h = F.relu(F.linear(h, sd[prefix + ".fc2.weight"], sd[prefix + ".fc2.bias"]))
    if training and dropout_rate > 0:
        h = h * dropout_mask / (1.0 - dropout_rate)
    loc = O.batch_norm(F.linear(h, sd[prefix + ".mu_encoder.0.weight"], sd[prefix + ".mu_encoder.0.bias"]), sd, prefix + ".mu_encoder.1",
                       training, new_stats=new_stats, **O.BN_ENC)
    logvar = O.batch_norm(F.linear(h, sd[prefix + ".lvar_encoder.0.weight"], sd[prefix + ".lvar_encoder.0.bias"]), sd, prefix + ".lvar_encoder.1",
                          training, new_stats=new_stats, **O.BN_ENC)
    scale = (0.5 * logvar).exp()
    log_z = loc + scale * eps
    return {"logtheta_loc": loc, "logtheta_logvar": logvar, "logtheta_scale": scale, "log_z": log_z, "theta": F.softmax(log_z, -1)}


# ---- decoder: the regressor / logits GEMMs + likelihood boundary ------------------------------------------------------------
def _elementwise_grads(x, eta1, eta2, theta, logits, w):
    """rec_b = -sum_g log_mixture_nb and, by float64 autograd, the per-element gradients of sum_b w_b rec_b the likelihood kernel
    stores: d/d logits (dL), d/d log mu_1 (tP), d/d log mu_2 (tS), and d/d theta summed over the cells"""
    with torch.enable_grad():
        e1, e2, th, lg = (t.detach().requires_grad_(True) for t in (eta1, eta2, theta, logits))
        rec = -O.log_mixture_nb(x, e1.exp(), e2.exp(), th, lg).sum(-1)
        dL, tP, tS, dth = torch.autograd.grad((w * rec).sum(), (lg, e1, e2, th))
    return rec.detach(), dL, tP, tS, dth


class _Likelihood(torch.autograd.Function):
    """inputs: [W'_p | c_p] [G, kp+1], [W'_s | c_s] [G, ks+1], [z_p | 1] [B, kp+1], [z_s | 1] [B, ks+1], A_m = [m | z | 1] [B, KM],
    [W_m | b_m] [G, KM], px_r [G];  outputs: (sum_b w_b rec_b, rec [B]).  The hand-written backward follows the kernels' data flow
    (module docstring)."""

    @staticmethod
    def forward(ctx, Wpc, Wsc, Ap, As, Am, Wmb, px_r, x, library, w, rounding: bool, defects: frozenset):
        if rounding:
            yp, ys = split_mm(Ap, Wpc), split_mm(As, Wsc)
            logits = f16(bf16(Am) @ bf16(Wmb).t())
        else:
            yp, ys = Ap @ Wpc.t(), As @ Wsc.t()
            logits = Am @ Wmb.t()
        lp, ls = torch.logsumexp(yp, 1, keepdim=True), torch.logsumexp(ys, 1, keepdim=True)
        lib = library.reshape(-1, 1)
        theta = px_r.exp()
        rec, dL, tP, tS, dth = _elementwise_grads(x, lib - lp + yp, lib - ls + ys, theta, logits, w.reshape(-1))
        ctx.save_for_backward(Wpc, Wsc, Ap, As, Am, Wmb, theta, dL, tP, tS, dth, (yp - lp).exp(), (ys - ls).exp())
        ctx.rounding, ctx.defects = rounding, defects
        ctx.mark_non_differentiable(rec)
        return (w * rec).sum(), rec

    @staticmethod
    def backward(ctx, g, _g_rec):
        Wpc, Wsc, Ap, As, Am, Wmb, theta, dL, tP, tS, dth, smp, sms = ctx.saved_tensors
        r, dfx = ctx.rounding, ctx.defects
        B, G = dL.shape
        rnd = bf16 if r else (lambda t: t)
        Tp, Ts = tP.sum(1, keepdim=True), tS.sum(1, keepdim=True)   # row sums of the unrounded values
        dLr = dL if "unrounded_dL" in dfx else rnd(dL)
        tPr, tSr = rnd(tP), rnd(tS)
        if "zero_last_cell" in dfx:
            dLr, tPr, tSr = (t.clone() for t in (dLr, tPr, tSr))
            for t in (dLr, tPr, tSr):
                t[B - 1] = 0.0
        cP, cS = rnd(tPr - smp * Tp), rnd(tSr - sms * Ts)   # the corrected tiles
        cPz, cSz = cP, cS
        if "drop_last_gene_tile" in dfx:   # the last (partial) 32-gene tile misses the latent-gradient contraction
            cPz, cSz = cP.clone(), cS.clone()
            cPz[:, 32 * ((G - 1) // 32):] = 0.0
            cSz[:, 32 * ((G - 1) // 32):] = 0.0
        cPw = cP
        if "drop_cells_128" in dfx:         # cell rows from 128 on miss one weight-gradient contraction
            cPw = cP.clone()
            cPw[128:] = 0.0
        dAp, dAs = cPz @ rnd(Wpc), cSz @ rnd(Wsc)
        dWpc, dWsc = cPw.t() @ rnd(Ap), cS.t() @ rnd(As)
        dAm, dWmb = dLr @ rnd(Wmb), dLr.t() @ rnd(Am)
        return (g * dWpc, g * dWsc, g * dAp, g * dAs, g * dAm, g * dWmb, g * theta * dth) + (None,) * 5


def _fold(z, W, gamma, beta, training, rm, rv, new_stats, key):
    """BatchNorm1d over z W^T folded into [W' | c] (csrc/spv_decoder.h: y = z . W' + c)"""
    y = z @ W.t()
    if training:
        mean, var = y.mean(0), y.var(0, unbiased=False)
        if new_stats is not None:
            n = y.shape[0]
            new_stats[key + ".running_mean"] = (1 - BN_MOM) * rm + BN_MOM * mean.detach()
            new_stats[key + ".running_var"] = (1 - BN_MOM) * rv + BN_MOM * var.detach() * (n / max(n - 1, 1))
    else:
        mean, var = rm, rv
    s = gamma / torch.sqrt(var + BN_EPS)
    return torch.cat([W * s[:, None], (beta - mean * s)[:, None]], 1)


def decoder_group(zp, zs, zt, par, x, library, w, *, training: bool, buffers: dict, new_stats: Optional[dict] = None,
                  rounding: bool = True, defects=frozenset()):
    """one group's decoder + likelihood: (sum_b w_b rec_b, rec [B]).
    zp / zs: the inputs of the private / shared factor regressor, zt: the mixing trunk's input (= the A_m columns after m);
    par: the 13 parameters of dec_ops.decoder_params (Wp, gamma_p, beta_p, Ws, gamma_s, beta_s, Wa, ba, gamma_a, beta_a, Wm, bm, px_r);
    buffers: {"p" | "s" | "a": (running_mean, running_var)}; new_stats receives "{p,s,a}.running_{mean,var}" in training"""
    Wp, gp, bp, Ws, gs_, bs, Wa, ba, ga, bta, Wm, bm, px_r = par
    B = zp.shape[0]
    one = torch.ones(B, 1, dtype=zp.dtype)
    Wpc = _fold(zp, Wp, gp, bp, training, *buffers["p"], new_stats, "p")
    Wsc = _fold(zs, Ws, gs_, bs, training, *buffers["s"], new_stats, "s")
    pre = zt @ Wa.t() + ba
    if training:
        mean, var = pre.mean(0), pre.var(0, unbiased=False)
        if new_stats is not None:
            new_stats["a.running_mean"] = (1 - BN_MOM) * buffers["a"][0] + BN_MOM * mean.detach()
            new_stats["a.running_var"] = (1 - BN_MOM) * buffers["a"][1] + BN_MOM * var.detach() * (B / max(B - 1, 1))
    else:
        mean, var = buffers["a"]
    m = F.relu((pre - mean) / torch.sqrt(var + BN_EPS) * ga + bta)
    Am = torch.cat([m, zt, one], 1)
    Wmb = torch.cat([Wm, bm[:, None]], 1)
    return _Likelihood.apply(Wpc, Wsc, torch.cat([zp, one], 1), torch.cat([zs, one], 1), Am, Wmb, px_r, x, library, w, rounding,
                             frozenset(defects))


def decoder_fused(lat, pars, xs, libraries, w, *, training: bool, buffers, rounding: bool = True, defects=frozenset()):
    """what dec_ops.DecoderFused computes for one or two groups with n_kl = 0: (loss, [rec_g], new_stats per group).
    lat[g] = (private_log_z, poe_log_z) as the op takes them (the op's own latent slicing, oracle.split_latents, is applied here)"""
    loss, recs, stats = 0.0, [], []
    for g, (priv, poe) in enumerate(lat):
        zp, zs = O.split_latents(priv, poe, poe.shape[1], priv.shape[1])
        ns = {} if training else None
        lg, rec = decoder_group(zp, zs, torch.cat([zp, zs], 1), pars[g], xs[g], libraries[g], w, training=training, buffers=buffers[g],
                                new_stats=ns, rounding=rounding, defects=defects)
        loss = loss + lg
        recs.append(rec)
        stats.append(ns)
    return loss, recs, stats


# ---- the whole step (oracle.forward_loss with the rounding sites) -------------------------------------------------------------
def forward_loss(sd, counts: Sequence[torch.Tensor], *, n_dimensions_shared: int, n_dimensions_private: int, noise, mode: str = "label",
                 labels=None, plan_block=None, components=None, kl_weight: float = 1.0, training: bool = True, dropout_rate: float = 0.0,
                 dropout_masks=None, update_running_stats: bool = False, batch_index=None, n_batch: int = 0, rounding: bool = True,
                 defects=frozenset()) -> dict:
    """oracle.spvipes_oracle.forward_loss (same arguments, same result keys) in bf16 mode's arithmetic; run it on float64 inputs"""
    n_s, n_p = n_dimensions_shared, n_dimensions_private
    dt = counts[0].dtype
    one_hot = [None, None]
    if n_batch > 1:
        one_hot = [F.one_hot(b.flatten().long(), n_batch).to(dt) for b in batch_index]
    new_stats = {} if (training and update_running_stats) else None
    # the kernels evaluate log1p in fp32 (the x image holds f16 of that fp32 value; the likelihood uses the fp32 value itself)
    x = [torch.log1p(c.to(torch.float32)).to(dt) if rounding else torch.log(1 + c) for c in counts]
    library = [torch.log(xs.sum(1)).unsqueeze(1) for xs in x]
    private, shared = [], []
    for g in range(2):
        pre1 = fc1_pair(x[g], sd, g, one_hot[g], rounding)
        for kind, store in (("private", private), ("shared", shared)):
            dm = None if dropout_masks is None else dropout_masks.get(f"enc_{g}_{kind}")
            store.append(encoder_tail(sd, f"encoder_{g}_{kind}", pre1[kind], noise[f"enc_{g}_{kind}"], training, dropout_rate, dm, new_stats))
    if mode == "label":
        p0, p1 = O.poe_label(shared[0], shared[1], labels[0], labels[1])
        clamp = False
    elif mode == "paired":
        p0, p1 = O.poe_paired(shared[0], shared[1], plan_block)
        clamp = True
    elif mode == "cluster":
        p0, p1 = O.poe_cluster(shared[0], shared[1], plan_block, components[0], components[1])
        clamp = True
    else:
        raise ValueError(mode)
    poe = [O.poe_sample(p0, noise["poe_0"], clamp), O.poe_sample(p1, noise["poe_1"], clamp)]
    rec, kls, loss = [], {}, 0.0
    B = counts[0].shape[0]
    w = torch.full((B,), 1.0 / B, dtype=dt)
    for g in range(2):
        zp, zs = O.split_latents(private[g]["log_z"], poe[g]["logtheta_log_z"], n_s, n_p)
        zt = torch.cat([zp, zs], 1)
        if one_hot[g] is not None:   # every decoder layer sees cat(input, one_hot) (oracle.decoder_forward)
            zp, zs, zt = (torch.cat([t, one_hot[g]], 1) for t in (zp, zs, zt))
        pre = f"decoder_{g}"
        names = {"p": f"{pre}.factor_regressor_private.{L}", "s": f"{pre}.factor_regressor_shared.{L}", "a": f"{pre}.sigmoid_decoder.{L}"}
        par = [sd[names["p"] + ".0.weight"], sd[names["p"] + ".1.weight"], sd[names["p"] + ".1.bias"],
               sd[names["s"] + ".0.weight"], sd[names["s"] + ".1.weight"], sd[names["s"] + ".1.bias"],
               sd[names["a"] + ".0.weight"], sd[names["a"] + ".0.bias"], sd[names["a"] + ".1.weight"], sd[names["a"] + ".1.bias"],
               sd[f"{pre}.mixture.{L}.0.weight"], sd[f"{pre}.mixture.{L}.0.bias"], sd[f"px_r.{g}"]]
        buffers = {k: (sd[v + ".1.running_mean"], sd[v + ".1.running_var"]) for k, v in names.items()}
        ns = {} if new_stats is not None else None
        lg, r = decoder_group(zp, zs, zt, par, x[g], library[g], w, training=training, buffers=buffers, new_stats=ns,
                              rounding=rounding, defects=defects)
        if ns is not None:
            for k, v in ns.items():
                new_stats[names[k[0]] + ".1" + k[1:]] = v
        loss = loss + lg   # mean_b rec_b, differentiable through _Likelihood
        rec.append(r)
        kls[f"private_{g}"] = O.kl_normal_std(private[g]["logtheta_loc"], private[g]["logtheta_scale"])
        kls[f"poe_{g}"] = O.kl_normal_std(poe[g]["logtheta_loc"], poe[g]["logtheta_qz_scale"])
    loss = loss + torch.mean(kl_weight * kls["private_0"] + kl_weight * kls["poe_0"] + kl_weight * kls["private_1"] + kl_weight * kls["poe_1"])
    return {"loss": loss, "reconstruction_loss": rec, "kl_local": kls, "private_stats": private, "shared_stats": shared, "poe_stats": poe,
            "library": library, "new_running_stats": new_stats}
