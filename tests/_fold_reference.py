"""TEST INFRASTRUCTURE ONLY -- inputs, float64 references, derived error bounds and a numpy-float32 transcription for the decoder
preparation (csrc/spv_small.h: zsplit_*_kernel, bn_fold_fwd_kernel, bn_fold_bwd_kernel, zstats_bwd_kernel, trunk_fold_fwd_kernel,
trunk_fold_bwd_kernel, trunk_zstats_kernel).  Shared by tests/test_fold_reference_cpu.py and tests/test_gpu_decoder_prep.py.

Reference.  The UNFUSED definition in float64 torch on the CPU, on the float64 images of the fp32 inputs the kernel receives:
y = z W^T (+ b), training-mode BatchNorm1d(eps 1e-3) of y (biased variance to normalise, running variance with B / max(B - 1, 1)),
folded pair W' = gamma / sqrt(var + eps) W, c = beta - W' . zbar; eval mode takes the running statistics (trunk: mean0 = running_mean - b).
Backward = float64 AUTOGRAD of L = sum(dWeff[:, :K] * W') + sum(dWeff[:, K] * c) with the batch statistics recomputed from z inside the
graph; (d zbar | d C) are the gradients autograd leaves on the two intermediate nodes zbar (feeding the batch mean w . zbar only) and
C = (z - zbar)^T (z - zbar) / B (feeding the batch variance w^T C w).  No closed form is transcribed.

Bounds.  U = 2^-24: one fp32 rounding of v moves it by at most U |v|.  For every output the kernel's formula is evaluated a second time in
float64 with every term replaced by its absolute value (the running-error form, written A_x below) and multiplied by n U, n = the number
of roundings on the longest chain to that output, first order in U.  The statistics handed to the kernel (zsum, zz, and stat = (mean, var)
for the backward calls) are float64 values rounded once: one rounding per entry, counted below.  q4 = ceil(K / 4).  v_rsq_f32 is a 1-ulp
instruction (2 U relative, as in tests/_nb_reference.py).  A compiler that contracts a product and a sum into one fma only removes roundings.

Counts, from spv_small.h (REG = bn_fold_*_kernel, four lanes per gene; TRUNK = trunk_fold_*_kernel, one wave per row):
  zbar_k = zsum_k * (1 / B)                 the entry, 1 / B, the product                                                    3
  C_kl   = zz_kl / B - zbar_k zbar_l        first term 3, second 3 + 3 + 1 = 7, the subtraction 1: at most 8 on
                                            A_C = |zz| / B + |zbar| |zbar|^T                                                 8
  mean   = w . zbar                         REG: zbar 3, product 1, q4 adds in the lane, 2 shuffle adds                      q4 + 6
                                            TRUNK: zbar 3, product 1, 6 butterfly adds                                       10
  v_k    = sum_l C_kl w_l                   C 8, product 1, K adds                                                           K + 9
  var    = sum_k w_k v_k                    REG: v (K + 9), product 1, q4 adds, 2 shuffle adds                               K + q4 + 12
                                            TRUNK: v (K + 9), product 1, 6 butterfly adds                                    K + 16
         A_var = |w|^T A_C |w|;  the clamp max(var, 0) moves the value towards the true one (var >= 0): no term.
  inv    = gamma * rsq(var + eps)           var + eps: the sum 1, eps = fp32(1e-3) against the reference's 1e-3: 1  (2 U (var + eps));
                                            rsq halves a relative error and adds 2 U; the product 1:
                                            rel_inv = E_var / (2 (var + eps)) + 4 U
  W'_k   = w_k * inv                        rel_inv + 1;   image value hi + lo: + 2^-16 |W'| for the split
  c      = beta - mean * inv                |inv| E_mean + |mean inv| (rel_inv + 1 U) + U (|beta| + |mean inv|);  image: + 2^-16 |c|
  running_mean = (1 - m) rm + m mean        1 - m, two products, the sum: 3 U (|(1 - m) rm| + |m mean|) + m E_mean
                                            (TRUNK: mean = mean0 + b, one more sum: m U (|mean0| + |b|))
  running_var  = (1 - m) rv + m var f       f = B / max(B - 1, 1): the division (2), two products, 1 - m and its product, the sum:
                                            6 U (|(1 - m) rv| + |m var f|) + m f E_var
  eval: mean, var are the stored fp32 running statistics: E_mean = E_var = 0 (TRUNK: mean0 = running_mean - b, U (|rm| + |b|)).
Backward (stat = (mean, var) read back, one rounding each):
  rs     = rsq(var + eps)                   (U var + 2 U (var + eps)) / (2 (var + eps)) + 2 U <= 4 U;   inv = gamma rs: 5 U
  dinv   = sum_k gW_k w_k - gc mean         REG: product 1, q4 adds, 2 shuffles; gc mean: entry 1, product 1; the subtraction 1      q4 + 6
                                            TRUNK: product 1, 6 butterfly adds, the same 3                                          10
         A_dinv = |gW| . |w| + |gc mean|
  d beta = gc                               a copy: EXACT
  d gamma = dinv * rs                       rs (E_dinv + 5 U A_dinv)
  d W (eval) = gW inv,  d bias (TRUNK eval) = gc inv                                                                               6
  dmean  = -gc inv                                                                                                                6
  dvar   = dinv gamma (-1/2) rs^3           four products and three times rs (12): A_dvar = |gamma| rs^3 A_dinv / 2,
                                            E_dvar = |gamma| rs^3 E_dinv / 2 + 16 U A_dvar
  d W_k  = gW_k inv + dmean zbar_k + 2 dvar v_k     t1 = |gW inv| (6), t2 = |gc inv zbar_k| (6 + 3 + 1 = 10), t3 = 2 A_dvar A_v:
                                            6 U t1 + 10 U t2 + 2 A_v E_dvar + 2 A_dvar E_v + U t3 + 2 U (t1 + t2 + t3)
  (d zbar | d C) = sum_g (dmean_g w_g | dvar_g w_g w_g^T)   REG: the two products 2, 64 genes of a wave on the matrix pipe, 3 wave adds,
                                            ceil(nblk / 4) blocks of an interleaved group, 3 group adds                        72 + ceil(nblk / 4)
                                            TRUNK: 2, 64 rows of a block, 3 block adds                                                  69
         E_dC = |W|^T diag(E_dvar) |W| + n U A_dC,  A_dC = |W|^T diag(A_dvar) |W|;   d zbar likewise with dmean.
  d z[b][k] = dz0 + dzbar_k / B + sum_l S_kl (z_bl - zbar_l),  S = (dC + dC^T) / B
         s_k = dzbar_k / B: E_dzbar / B + 2 U A_dzbar / B;   S: (E_dC + E_dC^T) / B + 3 U A_S;   z - zbar: 4 U (|z| + |zbar|) =: 4 U A_zc
         the K + 1 adds and K products of the chain: (K + 1) U A_acc, A_acc = A_s + A_S A_zc;  the final sum with dz0: U (|dz0| + A_acc).
Statistics producer (spv_linear_wgrad as dec_ops._zstats_batch drives it): every product z_bk z_bl is rounded once and added on a chain of
at most B adds inside a wave (one slice holds at most B rows), then 3 wave adds and, past 256 rows, 16 slice adds: c = 1 + 3 + 16 = 20,
|error| <= (B + 20) U |z|^T |z|  (column sums: the same with |z|^T 1).

The cap of tests/test_fold_reference_cpu.py (each bound <= 1e-3 max|reference| on the STANDARD cases) is what keeps these bounds from
hiding a failure; the only fixed numbers here are that cap and BatchNorm's eps and momentum.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-3
SPLIT = 2.0 ** -16
MOMENTUM = 0.01
CAP = 1e-3

# ---- the grids (tests/test_gpu_decoder_prep.py runs them on the GPU, tests/test_fold_reference_cpu.py through the transcription) ------
K_NARROW = (1, 3, 4, 5, 15, 16, 17, 31, 32)
K_WIDE = (33, 47, 63, 64)
FWD_G, FWD_B = (1, 63, 64, 65, 257, 300), (2, 37, 300)
BWD_G, BWD_B = (1, 255, 256, 257, 700, 1100), (1, 2, 63, 64, 65, 130)
TRUNK_N, TRUNK_K, TRUNK_B = (1, 15, 16, 17, 64, 65, 256), (1, 31, 32, 33, 47, 48), (2, 63, 65, 130)
MIXED_BATCH = ((1, 3), (300, 31), (65, 16), (257, 1))   # (G, K): one launch, the grid sized for the largest
STATS_B = (37, 300, 1100)
KINDS_DEGENERATE = ("const_col", "equal_rows", "gamma0", "gamma_neg", "off3", "off30")


def cover(Ks, Gs, Bs):
    """(K, G, B): every (K, G) pair and every (K, B) pair -- and with them every (G, B) pair -- once, the third size rotating"""
    out = []
    for i, K in enumerate(Ks):
        for j, G in enumerate(Gs):
            out.append((K, G, Bs[(i + j) % len(Bs)]))
        for j, B in enumerate(Bs):
            out.append((K, Gs[(i + 2 * j + 1) % len(Gs)], B))
    return sorted(set(out))


def fwd_cases(wide: bool):
    return cover(K_WIDE if wide else K_NARROW, FWD_G, FWD_B)


def bwd_cases(wide: bool):
    return cover(K_WIDE if wide else K_NARROW, BWD_G, BWD_B)


def trunk_cases():
    return cover(TRUNK_K, TRUNK_N, TRUNK_B)


def f32(x: float) -> float:
    return float(np.float32(x))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_case(K: int, G: int, B: int, kind: str = "standard", trunk: bool = False, salt: int = 0) -> dict:
    """fp32 CPU tensors of one fold problem.  standard: latent column means uniform in (-1, 1), spread 1, |w| ~ 1 / sqrt(K)."""
    gen = torch.Generator().manual_seed(1000003 * K + 1009 * G + 7 * B + (1 << 20) * int(trunk) + 7919 * salt)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float64)
    mean, spread = ru(-1.0, 1.0, K), 1.0
    if kind == "off3":
        mean, spread = torch.full((K,), 3.0, dtype=torch.float64), 0.05
    elif kind == "off30":
        mean, spread = torch.full((K,), 30.0, dtype=torch.float64), 0.05
    elif kind.startswith("off:"):   # "off:<mean>:<spread>"
        mean, spread = torch.full((K,), float(kind.split(":")[1]), dtype=torch.float64), float(kind.split(":")[2])
    z = mean[None, :] + spread * rn(B, K)
    if kind == "const_col":
        z[:, K // 2] = 0.75
    elif kind == "equal_rows":
        z = z[:1].repeat(B, 1)
    gamma = ru(0.5, 1.5, G)
    if kind == "gamma0":
        gamma[::3] = 0.0
    elif kind == "gamma_neg":
        gamma = -gamma
    c = dict(K=K, G=G, B=B, kind=kind, trunk=trunk, z=z, W=rn(G, K) / math.sqrt(K), gamma=gamma, beta=rn(G), rm=0.1 * rn(G),
             rv=ru(0.5, 1.5, G), dWeff=rn(G, K + 1), dz0=rn(B, K), bias=rn(G) if trunk else None)
    return {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def stats_f32(z: torch.Tensor):
    """zsum [K], zz [K][K] of the fp32 latents: float64, rounded once"""
    zd = z.double()
    return zd.sum(0).float(), (zd.T @ zd).float()


# ---- float64 reference ----------------------------------------------------------------------------------------------------------------
def reference(c: dict, training: bool, momentum: float = MOMENTUM, use_bias: bool = True, backward: bool = False) -> dict:
    """the unfused definition (module docstring); with ``backward`` also its autograd gradients"""
    d = lambda t: t.double().clone().requires_grad_(backward)
    z, W, gamma, beta = d(c["z"]), d(c["W"]), d(c["gamma"]), d(c["beta"])
    bias = d(c["bias"]) if (c["bias"] is not None and use_bias) else None
    rm, rv = c["rm"].double(), c["rv"].double()
    B, m = z.shape[0], f32(momentum)
    b0 = bias if bias is not None else torch.zeros_like(beta)
    out = {}
    if training:
        zbar = z.mean(0)
        zc = z - z.mean(0)                         # (its own mean node: zbar below then carries the gradient of the batch mean alone)
        C = zc.T @ zc / B
        if backward:
            zbar.retain_grad(); C.retain_grad()
        mean0 = W @ zbar                           # batch mean of y = z W^T + b, less b
        var = ((W @ C) * W).sum(1)                 # its biased batch variance
        y = z @ W.T + b0
        # the statistics really are BatchNorm's: the two forms agree to float64 rounding (asserted by test_fold_reference_cpu)
        out["y_mean"], out["y_var"] = y.mean(0).detach(), y.var(0, unbiased=False).detach()
        out["rm"] = ((1 - m) * rm + m * (mean0 + b0)).detach()
        out["rv"] = ((1 - m) * rv + m * var * (B / max(B - 1, 1))).detach()
    else:
        mean0, var = rm - b0, rv
        out["rm"], out["rv"] = rm, rv
    inv = gamma / torch.sqrt(var + EPS)
    Wf = inv[:, None] * W
    cf = beta - inv * mean0
    out.update(mean0=mean0.detach(), var=var.detach(), inv=inv.detach(), Wf=Wf.detach(), cf=cf.detach())
    if backward:
        K = W.shape[1]
        g = c["dWeff"].double()
        L = (g[:, :K] * Wf).sum() + (g[:, K] * cf).sum()
        L.backward()
        zero = lambda t: torch.zeros_like(t)
        out.update(dW=W.grad, dgamma=gamma.grad, dbeta=beta.grad, dbias=(bias.grad if bias is not None and bias.grad is not None else zero(beta)))
        if training:
            out.update(dz=z.grad if z.grad is not None else zero(z), dzbar=zbar.grad if zbar.grad is not None else zero(zbar),
                       dC=C.grad if C.grad is not None else zero(C))
            out["dz_acc"] = out["dz"] + c["dz0"].double()   # what the kernel leaves: it accumulates into a non-zero d z
    return out


# ---- the counts ------------------------------------------------------------------------------------------------------------------------
def counts(K: int, trunk: bool, G: int = 1) -> dict:
    q4 = (K + 3) // 4
    nblk = (G + 255) // 256
    if trunk:
        return dict(mean=10, v=K + 9, var=K + 16, dinv=10, red=69)
    return dict(mean=q4 + 6, v=K + 9, var=K + q4 + 12, dinv=q4 + 6, red=72 + (nblk + 3) // 4)


def _absC(z: torch.Tensor):
    B = z.shape[0]
    zbar = z.mean(0)
    return zbar, (z.T @ z).abs() / B + torch.outer(zbar.abs(), zbar.abs())


def forward_bounds(c: dict, ref: dict, training: bool, momentum: float = MOMENTUM, use_bias: bool = True, image: bool = True) -> dict:
    """bounds of stat = (mean, var), the running statistics, W' and c (``image``: as hi + lo of the split-bf16 image)"""
    z, W, gamma, beta = c["z"].double(), c["W"].double(), c["gamma"].double(), c["beta"].double()
    rm, rv = c["rm"].double(), c["rv"].double()
    bias = c["bias"].double() if (c["bias"] is not None and use_bias) else None
    B, K, m = z.shape[0], W.shape[1], f32(momentum)
    n = counts(K, c["trunk"], W.shape[0])
    aW = W.abs()
    if training:
        zbar, aC = _absC(z)
        E_mean = n["mean"] * U * (aW @ zbar.abs())
        E_var = n["var"] * U * ((aW @ aC) * aW).sum(1)
        f = B / max(B - 1, 1)
        mean_full = ref["mean0"] + (bias if bias is not None else 0.0)
        E_rm = 3 * U * (((1 - m) * rm).abs() + (m * mean_full).abs()) + m * E_mean
        if bias is not None:
            E_rm = E_rm + m * U * (ref["mean0"].abs() + bias.abs())
        E_rv = 6 * U * (((1 - m) * rv).abs() + (m * ref["var"] * f).abs()) + m * f * E_var
    else:
        E_mean = U * (rm.abs() + bias.abs()) if bias is not None else torch.zeros_like(rm)
        E_var = torch.zeros_like(rv)
        E_rm, E_rv = torch.zeros_like(rm), torch.zeros_like(rv)
    var, inv, mean0 = ref["var"], ref["inv"], ref["mean0"]
    rel_inv = E_var / (2 * (var + EPS)) + 4 * U
    split = SPLIT if image else 0.0
    E_W = ref["Wf"].abs() * (rel_inv[:, None] + U + split)
    mi = (mean0 * inv).abs()
    E_c = inv.abs() * E_mean + mi * (rel_inv + U) + U * (beta.abs() + mi) + split * ref["cf"].abs()
    return dict(mean0=E_mean, var=E_var, rm=E_rm, rv=E_rv, Wf=E_W, cf=E_c)


def backward_bounds(c: dict, ref: dict, training: bool, use_bias: bool = True) -> dict:
    """bounds of dW, dgamma, dbias (trunk) and, in training mode, (d zbar | d C) and the accumulated d z; d beta is exact"""
    z, W, gamma = c["z"].double(), c["W"].double(), c["gamma"].double()
    g, dz0 = c["dWeff"].double(), c["dz0"].double()
    B, K = z.shape[0], W.shape[1]
    n = counts(K, c["trunk"], W.shape[0])
    aW, gW, gc = W.abs(), g[:, :K].abs(), g[:, K].abs()
    mean0, var = ref["mean0"], ref["var"]
    rs = 1.0 / torch.sqrt(var + EPS)
    ainv = gamma.abs() * rs
    A_dinv = (gW * aW).sum(1) + gc * mean0.abs()
    E_dinv = n["dinv"] * U * A_dinv
    out = dict(dgamma=rs * (E_dinv + 5 * U * A_dinv), dbias=6 * U * gc * ainv if not training else torch.zeros_like(gc))
    t1 = gW * ainv[:, None]
    if not training:
        out["dW"] = 6 * U * t1
        return out
    zbar, aC = _absC(z)
    E_dmean, A_dmean = 6 * U * gc * ainv, gc * ainv
    A_dvar = 0.5 * gamma.abs() * rs ** 3 * A_dinv
    E_dvar = 0.5 * gamma.abs() * rs ** 3 * E_dinv + 16 * U * A_dvar
    A_v = aW @ aC
    E_v = n["v"] * U * A_v
    t2 = A_dmean[:, None] * zbar.abs()[None, :]
    t3 = 2 * A_dvar[:, None] * A_v
    out["dW"] = 6 * U * t1 + 10 * U * t2 + 2 * A_v * E_dvar[:, None] + 2 * A_dvar[:, None] * E_v + U * t3 + 2 * U * (t1 + t2 + t3)
    A_dzbar = aW.T @ A_dmean
    E_dzbar = aW.T @ E_dmean + n["red"] * U * A_dzbar
    A_dC = aW.T @ (A_dvar[:, None] * aW)
    E_dC = aW.T @ (E_dvar[:, None] * aW) + n["red"] * U * A_dC
    out["dzbar"], out["dC"] = E_dzbar, E_dC
    A_s, E_s = A_dzbar / B, E_dzbar / B + 2 * U * A_dzbar / B
    A_S = (A_dC + A_dC.T) / B
    E_S = (E_dC + E_dC.T) / B + 3 * U * A_S
    A_zc = z.abs() + zbar.abs()[None, :]
    A_acc = A_s[None, :] + A_zc @ A_S.T
    E_acc = E_s[None, :] + A_zc @ E_S.T + 4 * U * (A_zc @ A_S.T) + (K + 1) * U * A_acc
    out["dz_acc"] = E_acc + U * (dz0.abs() + A_acc)
    return out


def stats_bounds(z: torch.Tensor):
    """(bound of zsum, bound of zz) for the statistics producer"""
    a = z.double().abs()
    B = z.shape[0]
    return (B + 20) * U * a.sum(0), (B + 20) * U * (a.T @ a)


FWD_KEYS = ("mean0", "var", "rm", "rv", "Wf", "cf")


def bwd_keys(training: bool, trunk: bool):
    return ("dW", "dgamma") + (("dbias",) if trunk else ()) + (("dzbar", "dC", "dz_acc") if training else ())


def cap_ratios(c: dict) -> dict:
    """per output, the largest bound / max|reference| over training and eval mode: from the reference alone"""
    worst = {}
    for training in (True, False):
        ref = reference(c, training, backward=True)
        bnd = dict(forward_bounds(c, ref, training, image=False), **backward_bounds(c, ref, training))
        for k in FWD_KEYS + bwd_keys(training, c["trunk"]):
            top = ref[k].abs().max().item()
            r = bnd[k].max().item() / top if top > 0.0 else (0.0 if bnd[k].max().item() == 0.0 else math.inf)
            worst[k] = max(worst.get(k, 0.0), r)
    return worst


_STANDARD = {}


def standard_case(K: int, G: int, B: int, trunk: bool = False) -> dict:
    """the standard input of a grid case.  A tensor with a single entry (K = 1 or G = 1) is one cancelling sum -- with K = 1 the layer's
    output does not even depend on the scale of w, so d W vanishes but for eps -- and a draw can land next to its zero; the bound, which
    does not cancel, then exceeds the cap.  As the cap's rule has it, the INPUT changes: the first draw (salt 0, 1, ...) whose bounds meet
    the cap is the case's input, decided from the float64 reference alone.  Batches of fewer than three cells are not held to the cap
    (with B = 2 a gene's variance is (y_1 - y_2)^2 / 4 and the smallest of G of them lies below eps: genuinely ill-conditioned)."""
    key = (K, G, B, trunk)
    if key not in _STANDARD:
        for salt in range(64):
            c = make_case(K, G, B, trunk=trunk, salt=salt)
            if B < 3 or max(cap_ratios(c).values()) <= CAP:
                break
        else:
            raise AssertionError(f"no standard input within the cap for {key}")
        _STANDARD[key] = c
    return _STANDARD[key]


# ---- bf16 images --------------------------------------------------------------------------------------------------------------------------
def split_bf16(v: torch.Tensor):
    """(hi, lo) int16 words of csrc/spv_common.h: split_bf16 for fp32 v: hi = bf16(v), lo = bf16(v - hi), round to nearest even"""
    v = v.float()
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def bf16_value(words: torch.Tensor) -> torch.Tensor:
    """float64 value of int16 bf16 words"""
    return words.contiguous().view(torch.bfloat16).double()


def bf16_ulp(hi_words: torch.Tensor) -> torch.Tensor:
    """the spacing of bf16 at the value of each word (2^(e - 7), the smallest normal's for zero and subnormals)"""
    v = bf16_value(hi_words).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 7)


def zcat_of(priv: torch.Tensor, poe: torch.Tensor) -> torch.Tensor:
    """the latent slicing: Z = cat(private_log_z, poe_log_z); z_private = Z[:, n_s : n_s + n_p], z_shared = Z[:, :n_s] (the A6 quirk)"""
    n_p, n_s = priv.shape[1], poe.shape[1]
    Z = torch.cat([priv, poe], 1)
    return torch.cat([Z[:, n_s:n_s + n_p], Z[:, :n_s]], 1)


# ---- numpy-float32 transcription of the kernels' formulas ----------------------------------------------------------------------------------
F = np.float32


def _lane4(t: np.ndarray) -> np.ndarray:
    """sum over the last axis as four lanes do: lane s adds k = s, s + 4, ... in order, then (p0 + p1) + (p2 + p3)"""
    K = t.shape[-1]
    p = []
    for s in range(4):
        a = np.zeros(t.shape[:-1], F)
        for k in range(s, K, 4):
            a = a + t[..., k]
        p.append(a)
    return (p[0] + p[1]) + (p[2] + p[3])


def _wave64(t: np.ndarray) -> np.ndarray:
    """sum over the last axis (<= 64 lanes) as a six-step butterfly"""
    v = np.zeros(t.shape[:-1] + (64,), F)
    v[..., :t.shape[-1]] = t
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., np.arange(64) ^ off]
    return v[..., 0]


def _seq(t: np.ndarray, axis: int) -> np.ndarray:
    """sum along ``axis`` in index order"""
    t = np.moveaxis(t, axis, 0)
    a = np.zeros(t.shape[1:], F)
    for i in range(t.shape[0]):
        a = a + t[i]
    return a


def _stats_lds(zsum, zz, B):
    invB = F(1.0) / F(B)
    zbar = zsum * invB
    return invB, zbar, zz * invB - np.outer(zbar, zbar).astype(F)


def emulate_forward(c: dict, zsum, zz, training: bool, momentum: float = MOMENTUM, use_bias: bool = True) -> dict:
    W, gamma, beta = (c[k].numpy().astype(F) for k in ("W", "gamma", "beta"))
    rm, rv = c["rm"].numpy().astype(F), c["rv"].numpy().astype(F)
    bias = c["bias"].numpy().astype(F) if (c["bias"] is not None and use_bias) else np.zeros_like(beta)
    B, m, eps = c["B"], F(momentum), F(EPS)
    red = _wave64 if c["trunk"] else _lane4
    if training:
        _, zbar, C = _stats_lds(zsum.numpy(), zz.numpy(), B)
        mean0 = red(W * zbar[None, :])
        v = _seq(W[:, None, :] * C[None, :, :], 2) if not c["trunk"] else _seq(W[:, :, None] * C[None, :, :], 1)
        var = np.maximum(red(W * v), F(0))
        rm = (F(1) - m) * rm + m * (mean0 + bias)
        rv = (F(1) - m) * rv + m * var * (F(B) / np.maximum(F(B) - F(1), F(1)))
    else:
        mean0, var = rm - bias, rv
    inv = gamma * (F(1) / np.sqrt(var + eps)).astype(F)
    return dict(mean0=mean0, var=var, rm=rm, rv=rv, Wf=W * inv[:, None], cf=beta - inv * mean0 if c["trunk"] else beta - mean0 * inv)


def emulate_backward(c: dict, zsum, zz, stat_mean, stat_var, training: bool) -> dict:
    W, gamma, g, z, dz0 = (c[k].numpy().astype(F) for k in ("W", "gamma", "dWeff", "z", "dz0"))
    G, K, B, trunk = c["G"], c["K"], c["B"], c["trunk"]
    mean, var = stat_mean.numpy().astype(F), stat_var.numpy().astype(F)
    red = _wave64 if trunk else _lane4
    rs = (F(1) / np.sqrt(var + F(EPS))).astype(F)
    inv = gamma * rs
    gW, gc = g[:, :K], g[:, K]
    dinv = red(gW * W) - gc * mean
    out = dict(dbeta=gc.copy(), dgamma=dinv * rs, dbias=(gc * inv if not training else np.zeros_like(gc)))
    if not training:
        out["dW"] = gW * inv[:, None]
        return out
    invB, zbar, C = _stats_lds(zsum.numpy(), zz.numpy(), B)
    dmean = -gc * inv
    dvar = dinv * gamma * F(-0.5) * rs * rs * rs
    v = _seq(W[:, None, :] * C[None, :, :], 2) if not trunk else _seq(W[:, :, None] * C[None, :, :], 1)
    out["dW"] = gW * inv[:, None] + dmean[:, None] * zbar[None, :] + F(2) * dvar[:, None] * v
    # block partials of (d zbar | d C): runs of 64 rows in order (a wave on the matrix pipe), then the fixed-order sums above them
    rows = 64
    Gq = -(-G // rows) * rows
    Wq = np.zeros((Gq, K), F); Wq[:G] = W
    dmq = np.zeros(Gq, F); dmq[:G] = dmean
    dvq = np.zeros(Gq, F); dvq[:G] = dvar
    pC = _seq(((dvq[:, None] * Wq)[:, :, None] * Wq[:, None, :]).reshape(Gq // rows, rows, K, K), 1)   # [runs][K][K]
    pM = _seq((dmq[:, None] * Wq).reshape(Gq // rows, rows, K), 1)
    part = np.concatenate([pM, pC.reshape(-1, K * K)], 1)
    if trunk:
        redv = _seq(part, 0)
    else:
        nw = -(-part.shape[0] // 4) * 4
        pw = np.zeros((nw, part.shape[1]), F); pw[:part.shape[0]] = part
        blk = pw.reshape(nw // 4, 4, -1)
        blk = ((blk[:, 0] + blk[:, 1]) + blk[:, 2]) + blk[:, 3]          # the four waves of a 256-gene block
        g4 = [np.zeros(blk.shape[1], F) for _ in range(4)]
        for k in range(blk.shape[0]):
            g4[k % 4] = g4[k % 4] + blk[k]
        redv = ((g4[0] + g4[1]) + g4[2]) + g4[3]
    out["dzbar"], out["dC"] = redv[:K], redv[K:].reshape(K, K)
    s = redv[:K] * invB
    S = (out["dC"] + out["dC"].T) * invB
    zc = z - zbar[None, :]
    acc = np.broadcast_to(s[None, :], (B, K)).astype(F)
    for l in range(K):
        acc = acc + S[None, :, l] * zc[:, l:l + 1]
    out["dz_acc"] = dz0 + acc
    return out
