"""TEST INFRASTRUCTURE ONLY -- inputs, float64 references, derived error bounds and a numpy-float32 transcription for the two-group
Product-of-Experts fusion (csrc/spv_small.h: poe_fuse_fwd_kernel, poe_fuse_bwd_kernel<AGG>, and for the cluster pairing
plan_expert_fwd_kernel / plan_expert_bwd_kernel) as nn_ops.PoELabel / PoEPaired / PoECluster drive them.  Shared by
tests/test_poe_reference_cpu.py and tests/test_gpu_poe_fuse.py; imported by no product file.

Reference.  The float64 CPU definitions of oracle/spvipes_oracle.py (poe_label, poe_paired, poe_cluster on the dense plan[idx0][:, idx1]
block, poe_sample, kl_normal_std) on the float64 images of the fp32 values the kernel receives.  kl is taken on scale*.clamp(min = 1e-6)
where the pairing clamps (paired, cluster).  Gradients are float64 AUTOGRAD of L = sum(coef . output) over loc*, logvar*, scale*, log_z
and kl of both groups (theta is not differentiable in the product, and excluded); no closed-form backward is transcribed into the
reference.  tests/_torch_poe.py is a second restatement (reference_torch_poe), cross-checked by the CPU test.

Bounds.  U = 2^-24: one fp32 rounding of v moves it by at most U |v|.  The kernel's operation chain is written ONCE (``chain``) over an
arithmetic that is either numpy float32 (the transcription) or the first-order running-error arithmetic ``V``: a float64 value and a bound
of the error that the fp32 evaluation carries at that point, every term taken in absolute value:
  a + b : e_a + e_b + U |a + b|          a * b : |a| e_b + |b| e_a + U |a b|          -a, select, gather : exact
  1 / a, a / b : the propagated error + 2 U |result|    (<= 1 ulp; the compiler's default division is correctly rounded: U)
  expf, sqrtf  : the propagated error + 2 U |result|    (1 ulp, the figure of tests/_nb_reference.py for these device functions)
  logf         : e_a / |a| + 2 U max(|result|, 1)       (as there: the result may be near zero)
A compiler that contracts a product and a sum into one fma only removes roundings.  Inputs are exact (fp32 values); the fp32 constants
0.36787944117144233f, 1e-6f, 1e-10f differ from the reference's exp(-1), 1e-6, 1e-10 by at most U relative, which is counted.

Roundings per chain (those ``V`` adds up; d a latent dimension, n <= 32 of them per cell):
  inv = expf(-lv)                     expf                                                                              2
  t = expf(-lv_o), u = loc_o t        expf 2; the product 1                                                             2, 3
          mode 1: t = 1 exact; mode 2: t = fl(exp(-1)): 1; u = 0
  J = 1 / (1 + (inv + t))             two sums on inv (2) and t (2), the division 2                                     <= 6
  loc* = (loc inv + u) J              loc inv: 2 + 1; + u (3): the sum 1; J 6; the product 1                            <= 12
  logvar* = logf(J)                   6 U relative in J = 6 U absolute, and logf: 2 U max(|logvar*|, 1)
  scale* = sqrtf(expf(logvar*))       the error of logvar* relative in expf, + 2, halved by sqrtf, + 2
          lone_passthrough (mode 2): loc*, logvar* copies (exact), scale* = expf(lv / 2): 2 (0.5 lv is exact)
  q = max(scale*, 1e-6f)              the clamped value carries U (the constant)
  log_z = loc* + q eps                q eps 1, the sum 1, on top of the errors of loc* and q
  kl  = sum_d 0.5 (q q + loc* loc* - 1 - logf(q q))    per term: two products, three running sums, logf of a product; then the five
          butterfly adds of sum32: 5 U sum_d |term_d| on top of the terms' errors
  theta = e / sum_d e, e = expf(log_z - max)           the shift is free (any m gives the same quotient): the error of log_z, the
          subtraction 1, expf 2; the sum: 5 butterfly adds; the division 2
Backward (the forward's loc*, scale* are read back as stored: they carry their forward bounds; incoming gradients are exact):
  Gl = (g_loc + g_z) + g_kl loc*                                                                                       3 + loc*
  Gs = g_scale + [live] (g_z eps + g_kl (q - 1 / q))      1 / q 2, the difference 1, two products, two sums             <= 7 + q
  Gv = g_logvar + (0.5 scale*) Gs                         the product 1, the sum 1
  dN = Gl J,  dP = -J (Gl loc* + Gv)                      J 6; products and the sum
  own expert:   d loc += dN inv,  d logvar += -inv (dN loc + dP)
  partner (mode 0):  c0 = dN t,  c1 = -t (dP + dN loc_o)
  passthrough:  d loc += Gl, d logvar += Gv
  An element of d_stats (d_expert) that receives K contributions c_k, atomics or the in-workgroup sum in any order:
          sum_k e(c_k) + K U sum_k |c_k|   (K adds, the first of them onto the zero fill).
Cluster pairing, plan_expert_fwd: per cell i with m_i stored entries inside its component
  al = sum_j w_ij s_j : product 1, m_i adds          (m_i + 1) U sum_j w_ij |s_j|
  rs = sum_j w_ij     : m_i adds                     m_i U rs;      rc = max(rs, 1e-10f)
  E = al / rc         : the two errors propagated, the division 2.   (no stored entry: al = 0, E = 0 exactly)
plan_expert_bwd: per position t with m'_t entries:  w' = w / rc (error of rc, the division 2), products 1, m'_t adds, and the final
  add onto what the fusion backward left in d_stats: (m'_t + 1) U sum_i w'_it |dE_i| + the propagated errors + U |result|.
``live`` (scale* >= 1e-6f) is a comparison: a cell whose scale* lies within its own bound of 1e-6 could legitimately take either
branch.  No such cell exists on any committed case (clamp_margin, asserted by both test files): the clamp cases sit at scale* ~ 3e-7.

The cap of tests/test_poe_reference_cpu.py (forward bounds <= 2e-5 max|reference|, gradient bounds <= 1e-4 max|reference| on the
STANDARD cases) is what keeps these bounds from hiding a failure.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import spvipes_oracle as O

U = 2.0 ** -24
F = np.float32
CAP_FWD, CAP_GRAD = 2e-5, 1e-4
CLAMP = 1e-6
EINV = 0.36787944117144233
OUT = ("loc", "logvar", "scale", "logz", "theta", "kl")
DIFF = ("loc", "logvar", "scale", "logz", "kl")      # outputs that enter the loss
FWD_KEYS = tuple(f"{k}{g}" for g in (0, 1) for k in OUT)
GRAD_KEYS = tuple(f"{k}{g}" for g in (0, 1) for k in ("dloc", "dlogvar"))
MUTATIONS = ("drop_gk_jl", "t1_mode2", "drop_second", "no_live", "no_passthrough")

# ---- the grids ----------------------------------------------------------------------------------------------------------------------------
NS = (1, 10, 25, 31, 32)
LABEL_B = ((1, 1), (7, 9), (8, 8), (9, 70), (70, 9), (130, 130), (257, 33))
PLAN_B = (1, 7, 31, 32, 33, 130)


def standard_grid(pairing: str):
    """every (n, B) pair of the pairing once"""
    Bs = LABEL_B if pairing == "label" else tuple((B, B) for B in PLAN_B)
    return [(n, B0, B1) for n in NS for (B0, B1) in Bs]


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def _sparse_rows(rng, n0, n1, per_row, lo=0.05, hi=1.0):
    p = np.zeros((n0, n1), F)
    for r in range(n0):
        cols = rng.choice(n1, size=min(per_row, n1), replace=False)
        p[r, cols] = rng.uniform(lo, hi, size=len(cols)).astype(F)
    return p


def make_case(pairing: str, n: int, B0: int, B1: int, kind: str = "standard", salt: int = 0, use=None) -> dict:
    """fp32 CPU inputs of one fusion problem.  standard: loc ~ N(0, 1), logvar ~ 0.5 N(0, 1), eps ~ N(0, 1).
    ``use``: the (output, group) pairs that enter the loss (default: every differentiable output of both groups)."""
    seed = 1000003 * n + 1009 * B0 + 7 * B1 + 7919 * salt + {"label": 0, "paired": 1, "cluster": 2}[pairing] * (1 << 20) + (hash_kind(kind) << 8)
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    Bs = (B0, B1)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float64)
    loc = [rn(B, n) for B in Bs]
    logvar = [0.5 * rn(B, n) for B in Bs]
    if kind == "clamp":
        logvar = [ru(-30.1, -29.9, B, n) for B in Bs]
    elif kind == "extreme":
        loc = [ru(-30.0, 30.0, B, n) for B in Bs]
        logvar = [ru(-8.0, 8.0, B, n) for B in Bs]
    c = dict(pairing=pairing, n=n, B=Bs, kind=kind, loc=loc, logvar=logvar, eps=[rn(B, n) for B in Bs],
             coef=[{k: (rn(B) if k == "kl" else rn(B, n)) for k in DIFF} for B in Bs])
    if use is not None:
        for g in (0, 1):
            for k in DIFF:
                if (k, g) not in use:
                    c["coef"][g][k] = None
    if pairing == "label":
        c["labels"] = _labels(kind, rng, B0, B1)
    else:
        assert B0 == B1
        c.update(_plan(pairing, kind, rng, B0))
    f = lambda t: t.float() if isinstance(t, torch.Tensor) and t.dtype == torch.float64 else t
    for k in ("loc", "logvar", "eps"):
        c[k] = [f(t) for t in c[k]]
    c["coef"] = [{k: (None if v is None else f(v)) for k, v in d.items()} for d in c["coef"]]
    return c


def hash_kind(kind: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(kind)) % 4093


def _labels(kind, rng, B0, B1):
    L = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.long)
    if kind == "codes_edge":          # codes 0 and 1023 in use
        return [L(rng.choice([0, 1023, 5], size=B0)), L(rng.choice([0, 1023, 5], size=B1))]
    if kind == "one_side_0":          # label 7 in group 0 only: mode 2 there
        return [L(rng.choice([2, 7], size=B0)), L(np.full(B1, 2))]
    if kind == "one_side_1":
        return [L(np.full(B0, 2)), L(rng.choice([2, 7], size=B1))]
    if kind == "more_on_0":           # label 4: more cells in group 0 than in group 1 (mode 1 for the surplus)
        a, b = np.full(B0, 4), np.full(B1, 9)
        a[::5] = 9
        b[:max(B1 // 4, 1)] = 4
        return [L(a), L(rng.permutation(b))]
    if kind == "more_on_1":
        a, b = np.full(B0, 9), np.full(B1, 4)
        b[::5] = 9
        a[:max(B0 // 4, 1)] = 4
        return [L(rng.permutation(a)), L(b)]
    if kind == "all_one":
        return [L(np.full(B0, 3)), L(np.full(B1, 3))]
    if kind == "each_own":
        assert B0 == B1
        return [L(rng.permutation(B0)), L(rng.permutation(B1))]
    k = 3 if kind != "extreme" else 2
    return [L(rng.integers(0, k, size=B0)), L(rng.integers(0, k, size=B1))]


def _plan(pairing, kind, rng, B):
    """dense fp32 plan [n0][n1] of the dataset, the minibatch's dataset indices, and (cluster) the component codes"""
    n0, n1 = B + 13, B + 11
    idx = [rng.permutation(n0)[:B].astype(np.int32), rng.permutation(n1)[:B].astype(np.int32)]
    comp = [rng.integers(0, 3, size=B), rng.integers(0, 3, size=B)]
    plan = _sparse_rows(rng, n0, n1, 3 if pairing == "paired" else 6)
    blk = lambda: np.zeros((n0, n1), F)
    if kind == "mostly_empty":        # a handful of stored entries inside the minibatch block: every other row / column points at cell 0
        plan = blk()
        for r in rng.choice(B, size=6, replace=False):
            plan[idx[0][r], idx[1][rng.integers(0, B)]] = F(rng.uniform(0.1, 1.0))
        out = np.setdiff1d(np.arange(n1), idx[1])
        plan[idx[0][3], out[0]] = F(2.0)     # and entries that leave the minibatch
    elif kind == "shared_ws":         # cells 0, 5, 31 of workgroup 0 and cell 32 of workgroup 1 share partner 9; the rest pair off one to one
        plan = blk()
        perm = rng.permutation(B)
        r9 = int(np.nonzero(perm == 9)[0][0])
        perm[0], perm[r9] = perm[r9], perm[0]      # (row 0 is the one whose own entry lies at 9)
        for r in range(B):
            plan[idx[0][r], idx[1][perm[r]]] = F(rng.uniform(0.1, 0.5))
        for r in (0, 5, 31, 32):
            plan[idx[0][r], idx[1][9]] = F(0.9)
    elif kind == "diagonal":
        plan = blk()
        perm = rng.permutation(B)
        for r in range(B):
            plan[idx[0][r], idx[1][perm[r]]] = F(rng.uniform(0.1, 1.0))
    elif kind == "ties":              # equal maxima in rows and columns: the first minibatch position wins
        plan = blk()
        for r in range(B):
            cols = rng.choice(B, size=3, replace=False)
            plan[idx[0][r], idx[1][cols]] = F(0.5)
            plan[idx[0][r], idx[1][rng.integers(0, B)]] = F(0.25)
    elif kind == "lone":              # component 5 in group 0 only, component 6 in group 1 only
        comp[0][::4] = 5
        comp[1][1::3] = 6
    elif kind == "unequal":           # component 0: a quarter of group 0, three quarters of group 1
        comp = [np.where(np.arange(B) % 4 == 0, 0, 1), np.where(np.arange(B) % 4 == 0, 1, 0)]
        comp = [rng.permutation(comp[0]), rng.permutation(comp[1])]
    elif kind == "empty_rows":        # one entry per dataset row: most rows have none inside their component
        plan = _sparse_rows(rng, n0, n1, 1)
    elif kind == "absent":            # a wide dataset: most stored entries name cells outside the minibatch
        n0, n1 = 3 * B + 5, 3 * B + 2
        idx = [rng.permutation(n0)[:B].astype(np.int32), rng.permutation(n1)[:B].astype(np.int32)]
        plan = _sparse_rows(rng, n0, n1, 9)
    out = dict(plan=plan, idx=[torch.as_tensor(i) for i in idx])
    if pairing == "cluster":
        out["comp"] = [torch.as_tensor(np.asarray(x), dtype=torch.long) for x in comp]
    return out


def block_of(c: dict) -> torch.Tensor:
    """plan[idx0][:, idx1], float64"""
    return torch.as_tensor(c["plan"][c["idx"][0].long().numpy()][:, c["idx"][1].long().numpy()]).double()


def clamps(c: dict) -> bool:
    return c["pairing"] != "label"


# ---- float64 references -------------------------------------------------------------------------------------------------------------------
def _finish(c: dict, leaves, outs) -> dict:
    """outs[g] = dict of the six outputs (float64, in the graph) -> values and the autograd gradients of L = sum coef . output"""
    res, L = {}, 0.0
    for g in (0, 1):
        for k in OUT:
            res[f"{k}{g}"] = outs[g][k].detach()
        for k in DIFF:
            w = c["coef"][g][k]
            if w is not None:
                L = L + (w.double() * outs[g][k]).sum()
    grads = torch.autograd.grad(L, leaves, allow_unused=True)
    for i, name in enumerate(("dloc0", "dlogvar0", "dloc1", "dlogvar1")):
        res[name] = grads[i] if grads[i] is not None else torch.zeros_like(leaves[i])
    return res


def _leaves(c):
    d = lambda t: t.double().clone().requires_grad_(True)
    return d(c["loc"][0]), d(c["logvar"][0]), d(c["loc"][1]), d(c["logvar"][1])


def reference(c: dict) -> dict:
    """the oracle's definitions; keys FWD_KEYS + GRAD_KEYS"""
    l0, v0, l1, v1 = leaves = _leaves(c)
    sh = [dict(logtheta_loc=l, logtheta_logvar=v, logtheta_scale=torch.exp(0.5 * v)) for l, v in ((l0, v0), (l1, v1))]
    if c["pairing"] == "label":
        p = O.poe_label(sh[0], sh[1], c["labels"][0], c["labels"][1])
    elif c["pairing"] == "paired":
        p = O.poe_paired(sh[0], sh[1], block_of(c))
    else:
        p = O.poe_cluster(sh[0], sh[1], block_of(c), c["comp"][0], c["comp"][1])
    outs = []
    for g in (0, 1):
        s = O.poe_sample(p[g], c["eps"][g].double(), clamps(c))
        outs.append(dict(loc=s["logtheta_loc"], logvar=s["logtheta_logvar"], scale=s["logtheta_scale"], logz=s["logtheta_log_z"],
                         theta=s["logtheta_theta"], kl=O.kl_normal_std(s["logtheta_loc"], s["logtheta_qz_scale"])))
    return _finish(c, leaves, outs)


def reference_torch_poe(c: dict) -> dict:
    """the same through tests/_torch_poe.py, in float64"""
    from tests import _torch_poe as T
    l0, v0, l1, v1 = leaves = _leaves(c)
    sh = {g: dict(logtheta_loc=l, logtheta_logvar=v, logtheta_scale=torch.exp(0.5 * v)) for g, (l, v) in enumerate(((l0, v0), (l1, v1)))}
    noise = {f"poe_{g}": c["eps"][g].double() for g in (0, 1)}
    if c["pairing"] == "label":
        p = T.label_based_poe(sh, {0: c["labels"][0], 1: c["labels"][1]}, noise)
    elif c["pairing"] == "paired":
        p = T.paired_poe(sh, block_of(c), noise)
    else:
        p = T.cluster_based_poe(sh, block_of(c), {0: c["comp"][0], 1: c["comp"][1]}, noise)
    outs = [dict(loc=p[g]["logtheta_loc"], logvar=p[g]["logtheta_logvar"], scale=p[g]["logtheta_scale"], logz=p[g]["logtheta_log_z"],
                 theta=p[g]["logtheta_theta"], kl=T.kl_normal_std(p[g]["logtheta_loc"], p[g]["logtheta_qz"].scale)) for g in (0, 1)]
    return _finish(c, leaves, outs)


def structure(c: dict) -> dict:
    """the pairing itself (no arithmetic): partner / mode per group as the oracle defines them, and for the cluster pairing the masked plan
    weights W[g][i][j] between cell i of group g and position j of the other minibatch"""
    if c["pairing"] == "label":
        pm = [O.label_partner(c["labels"][0], c["labels"][1]), O.label_partner(c["labels"][1], c["labels"][0])]
        return dict(partner=[p.numpy() for p, _ in pm], mode=[m.numpy() for _, m in pm], passthrough=False)
    blk = block_of(c)
    if c["pairing"] == "paired":
        z = lambda B: np.zeros(B, np.int64)
        return dict(partner=[torch.argmax(blk, 1).numpy(), torch.argmax(blk, 0).numpy()], mode=[z(c["B"][0]), z(c["B"][1])], passthrough=False)
    pm = [O.label_partner(c["comp"][0], c["comp"][1]), O.label_partner(c["comp"][1], c["comp"][0])]
    same = (c["comp"][0][:, None] == c["comp"][1][None, :])
    W = [torch.where(same, blk, torch.zeros_like(blk)).numpy(), torch.where(same.T, blk.T, torch.zeros_like(blk.T)).numpy()]
    return dict(partner=[p.numpy() for p, _ in pm], mode=[m.numpy() for _, m in pm], passthrough=True, W=W)


# ---- the running-error arithmetic -----------------------------------------------------------------------------------------------------------
class V:
    """value (float64) and a first-order bound of the error an fp32 evaluation carries at this point"""
    __slots__ = ("v", "e")
    __array_ufunc__ = None     # numpy operands defer to the operators below

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def lift(x):
        return x if isinstance(x, V) else V(x)

    def __neg__(self):
        return V(-self.v, self.e)

    def __add__(self, o):
        o = V.lift(o)
        v = self.v + o.v
        return V(v, self.e + o.e + U * np.abs(v))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-V.lift(o))

    def __rsub__(self, o):
        return V.lift(o) + (-self)

    def __mul__(self, o):
        o = V.lift(o)
        v = self.v * o.v
        return V(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + U * np.abs(v))

    __rmul__ = __mul__

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])


def _isv(*xs):
    return any(isinstance(x, V) for x in xs)


def fexp(x):
    if _isv(x):
        v = np.exp(x.v)
        return V(v, v * (x.e + 2 * U))
    return np.exp(np.asarray(x, np.float64)).astype(F)     # the device function as correctly rounded fp32 (within its 1 ulp)


def flog(x):
    if _isv(x):
        v = np.log(x.v)
        return V(v, x.e / np.abs(x.v) + 2 * U * np.maximum(np.abs(v), 1.0))
    return np.log(np.asarray(x, np.float64)).astype(F)


def fsqrt(x):
    if _isv(x):
        v = np.sqrt(x.v)
        return V(v, x.e / (2 * v) + 2 * U * v)
    return np.sqrt(np.asarray(x, np.float64)).astype(F)


def fdiv(a, b):
    if _isv(a, b):
        a, b = V.lift(a), V.lift(b)
        v = a.v / b.v
        return V(v, a.e / np.abs(b.v) + np.abs(v) * b.e / np.abs(b.v) + 2 * U * np.abs(v))
    return a / b


def fwhere(m, a, b):
    if _isv(a, b):
        a, b = V.lift(a), V.lift(b)
        return V(np.where(m, a.v, b.v), np.where(m, a.e, b.e))
    return np.where(m, a, b).astype(F)


def fmaxc(a, cst):
    """fmaxf(a, cst) with the fp32 constant fl(cst)"""
    if _isv(a):
        return fwhere(a.v >= cst, a, V(np.full_like(a.v, cst), U * cst))
    return np.maximum(a, F(cst))


def fcat(a, b):
    if _isv(a, b):
        a, b = V.lift(a), V.lift(b)
        return V(np.concatenate([a.v, b.v], 1), np.concatenate([a.e, b.e], 1))
    return np.concatenate([a, b], 1)


def fsum_lanes(a):
    """sum over the latent dimension by sum32's five butterfly steps (any order in the transcription)"""
    if _isv(a):
        return V(a.v.sum(1), a.e.sum(1) + 5 * U * np.abs(a.v).sum(1))
    return a.sum(1, dtype=F)


def fscatter(rows: int, width: int, parts, ar: str):
    """zero-filled [rows][width] plus every (idx, values) of ``parts``, K adds per element in any order"""
    if ar == "bound":
        v, e, a, cnt = np.zeros((rows, width)), np.zeros((rows, width)), np.zeros((rows, width)), np.zeros(rows)
        for idx, x in parts:
            np.add.at(v, idx, x.v); np.add.at(e, idx, x.e); np.add.at(a, idx, np.abs(x.v)); np.add.at(cnt, idx, 1.0)
        return V(v, e + cnt[:, None] * U * a)
    out = np.zeros((rows, width), F)
    for idx, x in parts:
        np.add.at(out, idx, x.astype(F))
    return out


def _expert_fwd(W, s, ar):
    """E = (W s) / max(rowsum W, 1e-10f) for s = (loc | logvar) [B][2n] -> (E, rc)"""
    nnz = (W > 0).sum(1).astype(np.float64)
    if ar == "bound":
        al = V(W @ s.v, W @ s.e + (nnz + 1)[:, None] * U * (W @ np.abs(s.v)))
        rs = W.sum(1)
        rc = fwhere(rs >= 1e-10, V(rs, nnz * U * rs), V(np.full_like(rs, 1e-10), U * 1e-10))
        return fdiv(al, rc[:, None]), rc
    W32 = W.astype(F)
    rc = np.maximum(W32.sum(1, dtype=F), F(1e-10))
    return (W32 @ s) / rc[:, None], rc


def _expert_bwd(W, rc, dE, ar):
    """[t] = sum_i (W[i][t] / rc[i]) dE[i]"""
    cnt = (W > 0).sum(0).astype(np.float64)
    if ar == "bound":
        w = fdiv(V(W), rc[:, None])
        a = w.v.T @ np.abs(dE.v)
        return V(w.v.T @ dE.v, w.v.T @ dE.e + w.e.T @ np.abs(dE.v) + (cnt + 1)[:, None] * U * a)
    return (W.astype(F) / rc[:, None]).T @ dE


# ---- the kernel's chain, once ---------------------------------------------------------------------------------------------------------------
def chain(c: dict, ar: str = "f32", mut: str | None = None) -> dict:
    """csrc/spv_small.h poe_fuse_fwd_kernel / poe_fuse_bwd_kernel (and plan_expert_*) on the case.  ar = "f32": numpy float32 arrays (the
    transcription; ``mut`` one of MUTATIONS breaks it on purpose); ar = "bound": V (values in float64 and their error bounds)."""
    assert mut is None or mut in MUTATIONS
    S = structure(c)
    n, Bs, clamp = c["n"], c["B"], clamps(c)
    cluster = c["pairing"] == "cluster"
    inp = (lambda t: V(t.numpy().astype(np.float64))) if ar == "bound" else (lambda t: t.numpy().astype(F))
    val = (lambda x: x.v) if ar == "bound" else (lambda x: x)
    loc, lv, eps = ([inp(t) for t in c[k]] for k in ("loc", "logvar", "eps"))
    ONE, ZERO, HALF = F(1.0), F(0.0), F(0.5)
    t2 = ONE if mut == "t1_mode2" else (V(np.float64(math.exp(-1.0)), U * math.exp(-1.0)) if ar == "bound" else F(EINV))
    if cluster:
        ex = [_expert_fwd(S["W"][g], fcat(loc[g], lv[g]), ar) for g in (0, 1)]
        sl, sv = [ex[g][0][:, :n] for g in (0, 1)], [ex[g][0][:, n:] for g in (0, 1)]
    else:
        sl, sv = loc, lv
    out, keep = {}, []
    for g in (0, 1):
        o = 1 - g
        m, pr = S["mode"][g][:, None], np.maximum(S["partner"][g], 0)
        inv = fexp(-sv[g])
        ol, t0 = sl[o][pr], fexp(-sv[o][pr])
        t = fwhere(m == 0, t0, fwhere(m == 1, ONE, t2))
        u = fwhere(m == 0, ol * t0, ZERO)
        J = fdiv(ONE, ONE + (inv + t))
        jl, jv = (sl[g] * inv + u) * J, flog(J)
        sc = fsqrt(fexp(jv))
        lone = (m == 2) & bool(S["passthrough"]) & (mut != "no_passthrough")
        jl, jv, sc = fwhere(lone, loc[g], jl), fwhere(lone, lv[g], jv), fwhere(lone, fexp(HALF * lv[g]), sc)
        sq = fmaxc(sc, CLAMP) if clamp else sc
        z = jl + sq * eps[g]
        s2 = sq * sq
        klt = HALF * (((s2 + jl * jl) - ONE) - flog(s2))
        e = fexp(z - val(z).max(1, keepdims=True))
        theta = fdiv(e, fsum_lanes(e)[:, None])
        out.update({f"loc{g}": jl, f"logvar{g}": jv, f"scale{g}": sc, f"logz{g}": z, f"theta{g}": theta, f"kl{g}": fsum_lanes(klt)})
        keep.append(dict(m=m, pr=pr, inv=inv, t=t, lo=fwhere(m == 0, ol, ZERO), J=J, jl=jl, sc=sc, sq=sq, lone=lone))
    # backward
    own_parts, self_parts = ([], []), ([], [])     # per group: contributions to d_stats / to the self expert's gradient
    for g in (0, 1):
        o, k = 1 - g, keep[g]
        gin = lambda name, shape: inp(torch.zeros(shape) if c["coef"][g][name] is None else c["coef"][g][name])   # (ld_or_zero)
        gl, gv, gs, gz = (gin(name, (Bs[g], n)) for name in ("loc", "logvar", "scale", "logz"))
        gk = gin("kl", (Bs[g],))[:, None]
        jl, sc, sq = k["jl"], k["sc"], k["sq"]
        Gl = (gl + gz) if mut == "drop_gk_jl" else (gl + gz) + gk * jl
        live = np.ones_like(val(sc), bool) if (not clamp or mut == "no_live") else (val(sc) >= (CLAMP if ar == "bound" else F(CLAMP)))
        Gs = gs + fwhere(live, gz * eps[g] + gk * (sq - fdiv(ONE, sq)), ZERO)
        Gv = gv + (HALF * sc) * Gs
        dN = Gl * k["J"]
        dP = -(k["J"] * (Gl * jl + Gv))
        s_self = fcat(dN * k["inv"], -(k["inv"] * (dN * sl[g] + dP)))
        c_oth = fcat(dN * k["t"], -(k["t"] * (dP + dN * k["lo"])))
        rows = np.arange(Bs[g])
        lone_r, m0 = k["lone"][:, 0], k["m"][:, 0] == 0
        own_parts[g].append((rows[lone_r], fcat(Gl, Gv)[lone_r]))
        self_parts[g].append((rows[~lone_r], s_self[~lone_r]))
        sel = rows[m0]
        if mut == "drop_second" and g == 0:
            seen = {}
            for b in sel:
                seen.setdefault(int(k["pr"][b]), []).append(b)
            dup = [v for v in seen.values() if len(v) > 1]
            if dup:
                sel = sel[sel != dup[0][1]]
        self_parts[o].append((k["pr"][sel], c_oth[sel]))
    for g in (0, 1):
        if cluster:
            d_exp = fscatter(Bs[g], 2 * n, self_parts[g], ar)
            d = fscatter(Bs[g], 2 * n, own_parts[g], ar) + _expert_bwd(S["W"][g], ex[g][1], d_exp, ar)
        else:
            d = fscatter(Bs[g], 2 * n, own_parts[g] + self_parts[g], ar)
        out[f"dloc{g}"], out[f"dlogvar{g}"] = d[:, :n], d[:, n:]
    out["_scale_margin"] = None
    if ar == "bound" and clamp:
        out["_scale_margin"] = min(float((np.abs(keep[g]["sc"].v - CLAMP) - keep[g]["sc"].e).min()) for g in (0, 1))
    return out


def bounds(c: dict):
    """(values of the chain in float64, error bounds, clamp margin): dicts of float64 tensors keyed like ``reference``; the margin is the
    smallest |scale* - 1e-6| - bound(scale*) over the cells of a clamping pairing (None for the label pairing) and must be positive"""
    r = chain(c, "bound")
    keys = FWD_KEYS + GRAD_KEYS
    return ({k: torch.as_tensor(r[k].v) for k in keys}, {k: torch.as_tensor(r[k].e) for k in keys}, r["_scale_margin"])


def transcription(c: dict, mut: str | None = None) -> dict:
    r = chain(c, "f32", mut)
    out = {}
    for k in FWD_KEYS + GRAD_KEYS:
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
    for k in FWD_KEYS + GRAD_KEYS:
        top, b = ref[k].abs().max().item(), bnd[k].max().item()
        out[k] = b / (cap_of(k) * top) if top > 0.0 else (0.0 if b == 0.0 else math.inf)
    return out


_STANDARD = {}


def standard_case(pairing: str, n: int, B0: int, B1: int) -> dict:
    """the standard input of a grid case.  With a single cell or a single latent dimension an output tensor is one or a few numbers, and a
    draw can land one of them next to a zero of that output (kl = 0 at loc* = 0, scale* = 1; a gradient that cancels); the bound, which does
    not cancel, then exceeds the cap relative to that value.  As the cap's rule has it, the INPUT changes: the first draw (salt 0, 1, ...)
    whose bounds meet the cap is the case's input, decided from the float64 reference alone."""
    key = (pairing, n, B0, B1)
    if key not in _STANDARD:
        for salt in range(64):
            c = make_case(pairing, n, B0, B1, salt=salt)
            if max(cap_ratios(c).values()) <= 1.0:
                break
        else:
            raise AssertionError(f"no standard input within the cap for {key}")
        c["salt"] = salt
        _STANDARD[key] = c
    return _STANDARD[key]


# ---- the structured cases (one parameter id each) -----------------------------------------------------------------------------------------
ALL = None
STRUCTURED = {
    "label-codes_edge": ("label", 10, 40, 37, "codes_edge", ALL),
    "label-one_side_0": ("label", 10, 21, 12, "one_side_0", ALL),
    "label-one_side_1": ("label", 7, 12, 21, "one_side_1", ALL),
    "label-more_on_0": ("label", 10, 40, 24, "more_on_0", ALL),
    "label-more_on_1": ("label", 25, 24, 40, "more_on_1", ALL),
    "label-all_one": ("label", 10, 40, 33, "all_one", ALL),
    "label-each_own": ("label", 32, 30, 30, "each_own", ALL),
    "paired-mostly_empty": ("paired", 10, 130, 130, "mostly_empty", ALL),
    "paired-shared_ws": ("paired", 10, 64, 64, "shared_ws", ALL),
    "paired-diagonal": ("paired", 31, 45, 45, "diagonal", ALL),
    "paired-ties": ("paired", 10, 40, 40, "ties", ALL),
    "cluster-lone": ("cluster", 10, 40, 40, "lone", ALL),
    "cluster-unequal": ("cluster", 10, 41, 41, "unequal", ALL),
    "cluster-empty_rows": ("cluster", 25, 40, 40, "empty_rows", ALL),
    "cluster-absent": ("cluster", 10, 33, 33, "absent", ALL),
    "paired-clamp": ("paired", 10, 40, 40, "clamp", ALL),
    "cluster-clamp": ("cluster", 10, 40, 40, "clamp", ALL),
    "paired-clamp-logz_kl": ("paired", 10, 40, 40, "clamp", (("logz", 0), ("kl", 0), ("logz", 1), ("kl", 1))),
    "label-extreme": ("label", 10, 40, 33, "extreme", ALL),
    "paired-extreme": ("paired", 10, 40, 40, "extreme", ALL),
    "label-only_kl0": ("label", 10, 40, 33, "standard", (("kl", 0),)),
    "label-only_logz1": ("label", 10, 40, 33, "standard", (("logz", 1),)),
    "label-only_scale": ("label", 10, 40, 33, "standard", (("scale", 0), ("scale", 1))),
    "paired-only_kl0": ("paired", 10, 70, 70, "standard", (("kl", 0),)),
    "paired-only_logz1": ("paired", 10, 70, 70, "standard", (("logz", 1),)),
    "cluster-only_kl0": ("cluster", 10, 40, 40, "standard", (("kl", 0),)),
    "cluster-only_scale": ("cluster", 10, 40, 40, "standard", (("scale", 0), ("scale", 1))),
}
_CASES = {}


def structured_case(name: str) -> dict:
    if name not in _CASES:
        pairing, n, B0, B1, kind, use = STRUCTURED[name]
        _CASES[name] = make_case(pairing, n, B0, B1, kind=kind, use=use)
    return _CASES[name]
