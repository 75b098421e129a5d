"""TEST INFRASTRUCTURE ONLY -- inputs, a float64 reference, derived error bounds and a numpy-float32 transcription for the N-group
component Product of Experts (csrc/spv_poe_n.h: pn_stats, pn_means, pn_fuse_fwd, pn_cell_bwd, pn_comp_bwd, pn_apply_bwd) as
nn_ops.PoEComponents drives them.  Shared by tests/test_poe_n_reference_cpu.py and tests/test_gpu_poe_n.py; imported by no product file.
The arithmetic (``V``, ``fexp`` ... ``fsum_lanes``), U = 2^-24 and the two caps are those of tests/_poe_reference.py, imported, not copied.

Reference.  The definition in the header of csrc/spv_poe_n.h as float64 torch autograd on the float64 images of the fp32 inputs: the
component means of every group, prior + own posterior + the other groups' component means, the draw and the KL on scale*.clamp(min = 1e-6).
A cell whose code is not in [0, ncomp) (negative, too large, NaN) is in no component mean and receives no expert.  Gradients are AUTOGRAD of
L = sum(coef . output) over loc*, logvar*, scale*, log_z and kl of every group (theta is compared, not differentiated); a coef of None is
a gradient that nobody sends.  No closed-form backward is transcribed into the reference.

Bounds.  The six kernels' operation chain is written ONCE (``chain``) over numpy float32 (the transcription) or over the running-error
arithmetic ``V`` (rules in tests/_poe_reference.py).  Roundings per chain (those ``V`` adds up; d a latent dimension, c a component):
  pn_stats + pn_means  S_h[c] = sum of the K = count_h[c] rows (loc | logvar) of component c: per segment of per = ceil(B / 16) cells
                       one accumulator takes the cells in index order, then the 16 segment sums are added in index order (empty
                       segments add an exact zero): at most (K + 16) U sum|term|.  The count is a sum of ones: exact.
                       m_h[c] = S / max(count, 1)                                                  the division                2
  pn_fuse_fwd          inv = expf(-lv)                                                             expf                        2
                       per other group h with count_h[c] > 0, in index order: w = expf(-mlv_h[c])  expf on the mean's error    2
                       prec = (1 + inv) + w + ...    num = loc inv + mloc_h[c] w + ...             a product and a sum per expert
                       J = 1 / prec                                                                the division                2
                       loc* = num J (1);   logvar* = logf(J): e(J) / J + 2 U max(|logvar*|, 1);   scale* = sqrtf(J): e(J) / (2 scale*) + 2
                       q = max(scale*, 1e-6f)   the clamped value carries U (the constant)
                       log_z = loc* + q eps (2);  kl = sum_d 0.5 (q q + loc* loc* - 1 - logf(q q)): per term two products, three sums,
                       logf of a product; then sum32's five butterfly adds: 5 U sum_d |term_d|
                       theta = e / sum_d e, e = expf(log_z - max): the subtraction 1, expf 2, the butterfly 5, the division 2
  pn_cell_bwd          reads loc* and scale* back AS STORED (they carry their forward bounds); incoming gradients are exact, absent ones 0
                       Gl = (g_loc + g_z) + g_kl loc*;   Gs = g_scale + [live] (g_z eps + g_kl (q - 1 / q));   Gv = g_logvar + (0.5 scale*) Gs
                       J' = scale* scale*   -- NOT the forward's 1 / prec: twice the relative error of scale*, and the product   1
                       dN = Gl J' (1);   dP = -J' (Gl loc* + Gv) (3)
                       own expert: d loc = dN inv (expf 2, product 1);   d logvar = -inv (dN loc + dP) (3)
  pn_comp_bwd + pn_apply_bwd   for the target group h and component c, over the cells of the OTHER groups g (index order) with code c, when
                       count_h[c] > 0:  w = expf(-mlv_h[c]);  t_loc = dN w;  t_lv = -w (dN mloc_h[c] + dP)
                       one accumulator per segment takes group after group, cells in index order (segment seg of group g is its cells
                       [seg per_g, (seg + 1) per_g)); the 16 segment sums are added in order: e(terms) + (K + 16) U sum|term|, K the
                       number of terms;  / count_h[c] (2);  added onto the cell's own-expert gradient (1)
``live`` (scale* >= 1e-6f) is a comparison: a cell whose scale* lay within its own bound of 1e-6 could take either branch.  No such
cell exists on a committed case (the clamp margin, asserted by both test files): the clamp cells sit at scale* ~ 3e-7.
Input domain: exp(-logvar) finite in fp32; the cases go to logvar ~ -30.

The cap of tests/test_poe_n_reference_cpu.py (forward bounds <= 2e-5 max|reference|, gradient bounds <= 1e-4 max|reference| on the
STANDARD cases) keeps these bounds from hiding a failure.  The two points of the grid NS x GRID_B whose bound exceeds the cap are
held to their bound only, with the structured cases: ``OVER_CAP`` lists them with the reason.  The cap is never raised.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests._poe_reference import CAP_FWD, CAP_GRAD, F, U, V, fcat, fdiv, fexp, flog, fmaxc, fsqrt, fsum_lanes, fwhere

SEG = 16          # SPV_POE_COMP_SEG
CMAX = 64         # SPV_POE_COMP_CMAX
CLAMP = 1e-6
OUT = ("loc", "logvar", "scale", "logz", "theta", "kl")
DIFF = ("loc", "logvar", "scale", "logz", "kl")      # outputs that enter the loss
MUTATIONS = ("include_self", "absent_as_unit", "drop_gk_jl", "no_live", "apply_no_div", "skip_last_group", "seg_tail", "j_from_prec_sign")

NS = (1, 10, 25, 31, 32)
# group sizes -> ncomp.  (1, 1): 15 of 16 segments empty; (15, 16, 17): B below, at, above the segment count; (40, 33, 50): the sizes of
# tests/test_gpu_three_groups.py; (7, 9, 8, 130): four groups of very different size; (257, 33, 15): one much larger; (130, 130): two
# groups, and with n = 32 the full 64-entry LDS table beside the full 32-lane row
GRID_B = {(1, 1): 1, (15, 16, 17): 5, (40, 33, 50): 5, (7, 9, 8, 130): 7, (257, 33, 15): 12, (130, 130): 64}


def fwd_keys(c):
    return tuple(f"{k}{g}" for g in range(c["NG"]) for k in OUT)


def grad_keys(c):
    return tuple(f"{k}{g}" for g in range(c["NG"]) for k in ("dloc", "dlogvar"))


def keys(c):
    return fwd_keys(c) + grad_keys(c)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def hash_kind(kind: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(kind)) % 4093


def make_case(n: int, ncomp: int, B, kind: str = "standard", comp=None, use=None, clamp_cells: bool = False) -> dict:
    """fp32 CPU inputs of one N-group problem: loc ~ N(0, 1), logvar ~ 0.5 N(0, 1), eps ~ N(0, 1), uniform codes unless ``comp(rng, B)``
    gives them (fp32 values, any).  ``use``: the (output, group) pairs that enter the loss (default: every differentiable output of every
    group); a coef left out is None -- that gradient is not sent.  clamp_cells: every second cell has logvar ~ -30 + 0.5 N(0, 1)."""
    B = tuple(B)
    NG = len(B)
    seed = 1000003 * n + 8191 * ncomp + sum((1009 * (g + 1) + 7) * b for g, b in enumerate(B)) + (hash_kind(kind) << 8) + (3 << 20)
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    loc = [rn(b, n) for b in B]
    logvar = [0.5 * rn(b, n) for b in B]
    if clamp_cells:
        for g in range(NG):
            logvar[g][::2] = -30.0 + logvar[g][::2]
    eps = [rn(b, n) for b in B]
    coef = [{k: (rn(b) if k == "kl" else rn(b, n)) for k in DIFF} for b in B]
    if use is not None:
        for g in range(NG):
            for k in DIFF:
                if (k, g) not in use:
                    coef[g][k] = None
    codes = comp(rng, B) if comp is not None else [rng.integers(0, ncomp, size=b) for b in B]
    c = dict(NG=NG, n=n, ncomp=ncomp, B=B, kind=kind, loc=[t.float() for t in loc], logvar=[t.float() for t in logvar], eps=[t.float() for t in eps],
             comp=[torch.as_tensor(np.asarray(x, np.float32)) for x in codes],
             coef=[{k: (None if v is None else v.float()) for k, v in d.items()} for d in coef])
    assert all(t.shape == (b,) for t, b in zip(c["comp"], B)) and 2 <= NG <= 4 and 1 <= n <= 32 and 1 <= ncomp <= CMAX
    return c


def codes_of(c: dict):
    """pn_code per cell: the integral code, or -1 when the stored value is not in [0, ncomp) (negative, too large, NaN)"""
    out = []
    for t in c["comp"]:
        v = t.numpy().astype(np.float64)
        ok = (v >= 0) & (v < c["ncomp"])
        out.append(np.where(ok, np.where(ok, v, 0.0).astype(np.int64), -1))
    return out


def sub_case(c: dict, groups) -> dict:
    """the same problem with only ``groups`` of it"""
    pick = lambda k: [c[k][g] for g in groups]
    return dict(c, NG=len(groups), B=tuple(c["B"][g] for g in groups), loc=pick("loc"), logvar=pick("logvar"), eps=pick("eps"), comp=pick("comp"),
                coef=pick("coef"))


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------
def reference(c: dict) -> dict:
    """the definition of csrc/spv_poe_n.h in float64 with autograd gradients; keys ``keys(c)``"""
    NG, C = c["NG"], c["ncomp"]
    code = codes_of(c)
    idx = [torch.as_tensor(np.maximum(k, 0)) for k in code]
    ok = [torch.as_tensor(k >= 0) for k in code]
    loc = [t.double().clone().requires_grad_(True) for t in c["loc"]]
    lv = [t.double().clone().requires_grad_(True) for t in c["logvar"]]
    means = []
    for h in range(NG):
        oh = torch.nn.functional.one_hot(idx[h], C).double() * ok[h].double()[:, None]       # [B][C]; no row for a cell without a code
        cnt = oh.sum(0)
        den = cnt.clamp(min=1.0)[:, None]
        means.append(((oh.t() @ loc[h]) / den, (oh.t() @ lv[h]) / den, cnt))
    res, L = {}, 0.0
    for g in range(NG):
        inv = torch.exp(-lv[g])
        prec, num = 1.0 + inv, loc[g] * inv
        for h in range(NG):
            if h == g:
                continue
            m_loc, m_lv, cnt = means[h]
            present = ((cnt[idx[g]] > 0) & ok[g]).double()[:, None]
            w = torch.exp(-m_lv[idx[g]]) * present
            prec, num = prec + w, num + m_loc[idx[g]] * w
        jl, jv = num / prec, -torch.log(prec)
        sc = torch.exp(0.5 * jv)
        sq = sc.clamp(min=CLAMP)
        z = jl + sq * c["eps"][g].double()
        kl = (0.5 * (sq * sq + jl * jl - 1.0 - torch.log(sq * sq))).sum(1)
        outs = dict(loc=jl, logvar=jv, scale=sc, logz=z, theta=torch.softmax(z, -1), kl=kl)
        for k in OUT:
            res[f"{k}{g}"] = outs[k].detach()
        for k in DIFF:
            w = c["coef"][g][k]
            if w is not None:
                L = L + (w.double() * outs[k]).sum()
    grads = torch.autograd.grad(L, loc + lv, allow_unused=True)
    for g in range(NG):
        for name, gr, leaf in (("dloc", grads[g], loc[g]), ("dlogvar", grads[NG + g], lv[g])):
            res[f"{name}{g}"] = gr if gr is not None else torch.zeros_like(leaf)
    return res


# ---- the two-stage reductions ---------------------------------------------------------------------------------------------------------------
def _seg_sum(C: int, width: int, parts, ar: str, drop_tail: bool = False):
    """per component the sum of the rows x[b] of ``parts`` = [(code [B] (-1: no term), per, x [B][width])], as pn_stats / pn_comp_bwd and
    pn_means / pn_apply_bwd do it: a [16][C][width] table of segment accumulators takes part after part, cells in index order (cell b of
    a part belongs to segment b // per), then the 16 segment sums are added in index order.  -> (sums [C][width], K [C] terms per sum).
    bound arithmetic: the propagated errors + (K + 16) U sum|term|.  drop_tail (a mutation): the last non-empty segment's cells are lost."""
    K = np.zeros(C)
    if ar == "bound":
        v, e, a = np.zeros((C, width)), np.zeros((C, width)), np.zeros((C, width))
        for code, per, x in parts:
            sel = code >= 0
            i = code[sel]
            np.add.at(v, i, x.v[sel]); np.add.at(e, i, x.e[sel]); np.add.at(a, i, np.abs(x.v[sel])); np.add.at(K, i, 1.0)
        return V(v, e + (K + SEG)[:, None] * U * a), K
    acc = np.zeros((SEG, C, width), F)
    for code, per, x in parts:
        assert x.dtype == F
        last = (len(code) - 1) // per
        for b in range(len(code)):
            k, seg = code[b], b // per
            if k < 0 or (drop_tail and seg == last):
                continue
            acc[seg, k] += x[b]
            K[k] += 1.0
    s = np.zeros((C, width), F)
    for seg in range(SEG):
        s = s + acc[seg]
    return s, K


# ---- the kernels' chain, once ---------------------------------------------------------------------------------------------------------------
def chain(c: dict, ar: str = "f32", mut: str | None = None) -> dict:
    """csrc/spv_poe_n.h's six kernels on the case.  ar = "f32": numpy float32 arrays (the transcription; ``mut`` one of MUTATIONS breaks it
    on purpose); ar = "bound": V (values in float64 and their error bounds)."""
    assert ar in ("f32", "bound") and (mut is None or (mut in MUTATIONS and ar == "f32"))
    NG, n, C, Bs = c["NG"], c["n"], c["ncomp"], c["B"]
    code = codes_of(c)
    idx, ok = [np.maximum(k, 0) for k in code], [k >= 0 for k in code]
    per = [-(-B // SEG) for B in Bs]
    inp = (lambda t: V(t.numpy().astype(np.float64))) if ar == "bound" else (lambda t: t.numpy().astype(F))
    val = (lambda x: x.v) if ar == "bound" else (lambda x: x)
    den = (lambda k: np.maximum(k, 1.0)[:, None]) if ar == "bound" else (lambda k: np.maximum(k, 1.0).astype(F)[:, None])
    loc, lv, eps = ([inp(t) for t in c[k]] for k in ("loc", "logvar", "eps"))
    ONE, ZERO, HALF = F(1.0), F(0.0), F(0.5)
    # pn_stats, pn_means
    mloc, mlv, cnt = [], [], []
    for h in range(NG):
        S, K = _seg_sum(C, 2 * n, [(code[h], per[h], fcat(loc[h], lv[h]))], ar, drop_tail=(mut == "seg_tail"))
        m = fdiv(S, den(K))
        mloc.append(m[:, :n]); mlv.append(m[:, n:]); cnt.append(K)
    # pn_fuse_fwd
    out, keep = {}, []
    for g in range(NG):
        inv = fexp(-lv[g])
        prec, num = ONE + inv, loc[g] * inv
        for h in range(NG):
            if h == g and mut != "include_self":
                continue
            m = (ok[g] & ((cnt[h][idx[g]] > 0) | (mut == "absent_as_unit")))[:, None]
            w = fexp(-mlv[h][idx[g]])
            prec, num = fwhere(m, prec + w, prec), fwhere(m, num + mloc[h][idx[g]] * w, num)
        J = fdiv(ONE, prec)
        jl, jv, sc = num * J, flog(J), fsqrt(J)
        sq = fmaxc(sc, CLAMP)
        z = jl + sq * eps[g]
        s2 = sq * sq
        klt = HALF * (((s2 + jl * jl) - ONE) - flog(s2))
        e = fexp(z - val(z).max(1, keepdims=True))
        theta = fdiv(e, fsum_lanes(e)[:, None])
        out.update({f"loc{g}": jl, f"logvar{g}": jv, f"scale{g}": sc, f"logz{g}": z, f"theta{g}": theta, f"kl{g}": fsum_lanes(klt)})
        keep.append(dict(inv=inv, jl=jl, sc=sc, sq=sq))
    # pn_cell_bwd
    dN, dP, own = [], [], []
    for g in range(NG):
        gin = lambda name, shape: inp(torch.zeros(shape) if c["coef"][g][name] is None else c["coef"][g][name])   # (ld_or_zero)
        gl, gv, gs, gz = (gin(name, (Bs[g], n)) for name in ("loc", "logvar", "scale", "logz"))
        gk = gin("kl", (Bs[g],))[:, None]
        jl, sc, sq, inv = (keep[g][k] for k in ("jl", "sc", "sq", "inv"))
        live = np.ones_like(val(sc), bool) if mut == "no_live" else (val(sc) >= (CLAMP if ar == "bound" else F(CLAMP)))
        Gl = (gl + gz) if mut == "drop_gk_jl" else (gl + gz) + gk * jl
        Gs = gs + fwhere(live, gz * eps[g] + gk * (sq - fdiv(ONE, sq)), ZERO)
        Gv = gv + (HALF * sc) * Gs
        J = sc * sc
        n_, p_ = Gl * J, J * (Gl * jl + Gv)
        if mut != "j_from_prec_sign":
            p_ = -p_
        dN.append(n_); dP.append(p_)
        own.append(fcat(n_ * inv, -(inv * (n_ * loc[g] + p_))))
    # pn_comp_bwd, pn_apply_bwd
    for h in range(NG):
        others = [g for g in range(NG) if g != h]
        if mut == "skip_last_group":
            others = others[:-1]
        parts = []
        for g in others:
            w = fexp(-mlv[h][idx[g]])
            x = fcat(dN[g] * w, -(w * (dN[g] * mloc[h][idx[g]] + dP[g])))
            parts.append((np.where(ok[g] & (cnt[h][idx[g]] > 0), code[g], -1), per[g], x))
        S, _ = _seg_sum(C, 2 * n, parts, ar)
        add = S[idx[h]] if mut == "apply_no_div" else fdiv(S[idx[h]], den(cnt[h][idx[h]]))
        d = fwhere(ok[h][:, None], own[h] + add, own[h])
        out[f"dloc{h}"], out[f"dlogvar{h}"] = d[:, :n], d[:, n:]
    out["_scale_margin"] = None
    if ar == "bound":
        out["_scale_margin"] = min(float((np.abs(keep[g]["sc"].v - CLAMP) - keep[g]["sc"].e).min()) for g in range(NG))
    return out


def bounds(c: dict):
    """(values of the chain in float64, error bounds, clamp margin): dicts of float64 tensors keyed like ``reference``; the margin is the
    smallest |scale* - 1e-6| - bound(scale*) over the cells and must be positive"""
    r = chain(c, "bound")
    return ({k: torch.as_tensor(r[k].v) for k in keys(c)}, {k: torch.as_tensor(r[k].e) for k in keys(c)}, r["_scale_margin"])


def transcription(c: dict, mut: str | None = None) -> dict:
    r = chain(c, "f32", mut)
    out = {}
    for k in keys(c):
        assert r[k].dtype == np.float32, (k, r[k].dtype)
        out[k] = torch.as_tensor(r[k].astype(np.float64))
    return out


def cap_of(key: str) -> float:
    return CAP_GRAD if key.startswith("d") else CAP_FWD


def cap_ratios(c: dict, ref=None, bnd=None) -> dict:
    """per output bound / (cap x max|reference|): at most 1 within the cap"""
    ref = reference(c) if ref is None else ref
    bnd = bounds(c)[1] if bnd is None else bnd
    out = {}
    for k in keys(c):
        top, b = ref[k].abs().max().item(), bnd[k].max().item()
        out[k] = b / (cap_of(k) * top) if top > 0.0 else (0.0 if b == 0.0 else math.inf)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
# Points of the grid n x group sizes whose derived bound exceeds the cap: held to the bound only, with the structured cases, never by a
# raised cap.  Both have n = 1, where an output tensor is a few numbers and nothing large stands beside a small one:
#   n 1, B (1, 1)          log_z of group 0 is ONE number, loc* + q eps = -0.04 next to its zero; its bound is 2.1 x the forward cap
#   n 1, B (7, 9, 8, 130)  d logvar of group 2 (8 cells, 7 components) is the sum over up to 130 cells of group 3, as in ``lopsided``:
#                          1.95 x the gradient cap
OVER_CAP = ((1, (1, 1)), (1, (7, 9, 8, 130)))


def grid_points():
    return [(n, B) for n in NS for B in GRID_B]


def standard_grid():
    return [p for p in grid_points() if p not in OVER_CAP]


_CASES = {}


def grid_case(n: int, B) -> dict:
    key = (n, tuple(B))
    if key not in _CASES:
        _CASES[key] = make_case(n, GRID_B[tuple(B)], B)
    return _CASES[key]


def _absent(rng, B):          # 0 not in group 1, 3 not in group 2, 4 in group 1 only, 5 and 6 nowhere
    return [rng.integers(0, 4, size=B[0]), rng.integers(1, 5, size=B[1]), rng.integers(0, 3, size=B[2])]


def _disjoint(rng, B):        # group 2 shares no code with groups 0 and 1
    return [rng.integers(0, 5, size=B[0]), rng.integers(0, 5, size=B[1]), rng.integers(10, 12, size=B[2])]


BAD_CELLS = {0: (0, 5, 9, 21), 2: (1, 24)}


def _bad_codes(rng, B):       # -1, ncomp = 4, NaN, 1000.0 in groups 0 and 2
    x = [rng.integers(0, 4, size=b).astype(np.float32) for b in B]
    x[0][list(BAD_CELLS[0])] = (-1.0, 4.0, float("nan"), 1000.0)
    x[2][list(BAD_CELLS[2])] = (1000.0, float("nan"))
    return x


def _edge_code(rng, B):       # code 63 = ncomp - 1 present, code 0 absent
    return [rng.choice([63, 1, 2, 17, 62], size=b) for b in B]


KL_LOGZ3 = tuple((k, g) for g in range(3) for k in ("kl", "logz"))
STRUCTURED = {
    "absent": dict(n=10, ncomp=7, B=(40, 33, 50), comp=_absent),
    "disjoint": dict(n=10, ncomp=12, B=(40, 33, 25), comp=_disjoint),
    "bad_codes": dict(n=10, ncomp=4, B=(40, 33, 25), comp=_bad_codes),
    "clamp": dict(n=10, ncomp=5, B=(40, 33, 50), clamp_cells=True),
    "clamp-kl_logz": dict(n=31, ncomp=3, B=(17, 40), clamp_cells=True, use=(("kl", 0), ("logz", 0), ("kl", 1), ("logz", 1))),
    "partial_grads-kl_logz": dict(n=10, ncomp=5, B=(40, 33, 50), use=KL_LOGZ3),                                  # what the module sends
    "partial_grads-group1_unused": dict(n=25, ncomp=5, B=(40, 33, 50), use=tuple(u for u in KL_LOGZ3 if u[1] != 1)),
    "partial_grads-kl_logz-4": dict(n=32, ncomp=7, B=(7, 9, 8, 130), use=tuple((k, g) for g in range(4) for k in ("kl", "logz"))),
    "partial_grads-only_loc0": dict(n=10, ncomp=3, B=(17, 9, 33), use=(("loc", 0),)),
    "one_component": dict(n=10, ncomp=1, B=(9, 17, 8, 30)),
    "edge_code": dict(n=32, ncomp=64, B=(70, 45), comp=_edge_code),
    "lopsided": dict(n=10, ncomp=3, B=(300, 17, 64, 9)),     # its gradient bound exceeds the cap (few cells receive the sum over many)
}


def structured_case(name: str) -> dict:
    if name not in _CASES:
        if name in STRUCTURED:
            _CASES[name] = make_case(kind=name, **STRUCTURED[name])
        else:                                   # a grid point over the cap: "n-B0xB1x..."
            n, B = name.split("-")
            _CASES[name] = grid_case(int(n), tuple(int(b) for b in B.split("x")))
    return _CASES[name]


def structured_names():
    return sorted(STRUCTURED) + [f"{n}-{'x'.join(map(str, B))}" for (n, B) in OVER_CAP]


def two_group_uniform_plan_case(n: int = 10, B: int = 48, ncomp: int = 4) -> dict:
    """the one tie to the upstream two-group cluster PoE: both minibatches carry the SAME codes at the same positions, every component is
    present, and each group's statistics are constant inside a component (so a cell's own posterior is its group's component mean)"""
    c = make_case(n, ncomp, (B, B), kind="tie", comp=lambda rng, Bs: [np.arange(Bs[0]) % ncomp] * 2)
    k = torch.as_tensor(codes_of(c)[0])
    for g in range(2):
        for key in ("loc", "logvar"):
            c[key][g] = c[key][g][:ncomp][k].contiguous()
    return c
