"""Entropic optimal transport on the device: the fused kernels spv_ot_softmin / spv_ot_topk (csrc/spv_ot.h; include/spvipes_hip.h
states the contract), the log-domain Sinkhorn driver on top of them and the sparse plan it ends in.  ``spVIPES.compute_transport_plan``
runs it on a common low-dimensional representation of the two groups; nothing of size n0 x n1 is ever stored.  ``ot_segment_lse``
(csrc/spv_ot_segments.h) gives the untruncated plan's log mass per (cell, segment of the other group's cells) from the potentials:
what ``cluster_ops`` / ``spVIPES.match_transport_clusters`` read.  ``ot_project`` (csrc/spv_ot_project.h) pushes per-cell values of one group
through the untruncated plan onto the other group's cells: ``transport_project`` / ``spVIPES.transport_project``."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _abi
from ._abi import (OT_DMAX, OT_KMAX, OT_SEG_MAX, OT_SPLIT_MAX, OT_VAL_MAX, SpvOtArgs, SpvOtProjArgs, SpvOtSegArgs, ptr,   # the limits: part of this module's interface
                   stream_ptr)
from ._scan_ops import _fill_sides, _k, _n_split, _out_pair, _rows, _sides, _workspace
from .data import plan_union_csr


def ot_tiles() -> Tuple[int, int]:
    """(queries per workgroup, candidates per LDS tile) of the partial passes"""
    lib = _abi.load()
    return int(lib.spv_ot_tile_q()), int(lib.spv_ot_tile_c())


def ot_splits(n_q: int, n_c: int) -> int:
    """Chunks of the candidates both kernels use for this shape when ``n_split`` is 0: a pure function of the shapes"""
    return int(_abi.load().spv_ot_splits(int(n_q), int(n_c)))


def ot_ws_bytes(n_q: int, k: int, n_split: int) -> int:
    """Bytes of workspace for ``n_split`` chunks (the resolved number, not 0); ``k`` = 0 asks for ot_softmin's: 0 for one chunk"""
    return int(_abi.load().spv_ot_ws_bytes(int(n_q), int(k), int(n_split)))


def _vector(t, n: int, dev, name: str) -> None:
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n
            or not t.is_contiguous()):
        raise _abi.SpvError(f"ot: {name} must be a contiguous fp32 device tensor with {n} entries")


def _common(X, Y, h, inv_eps, n_split) -> SpvOtArgs:
    """the checks and the argument fields ot_softmin and ot_topk share"""
    dev, n_q, n_c, D = _sides("ot", X, Y, ("X", "Y"))
    _vector(h, n_c, dev, "h")
    inv_eps = float(inv_eps)
    if not (0.0 < inv_eps < math.inf) or not (0.0 < float(np.float32(inv_eps)) < math.inf):
        raise ValueError(f"ot: inv_eps must be a positive finite number in fp32, got {inv_eps!r}")
    a = SpvOtArgs()
    _fill_sides(a, X, Y)
    a.h, a.inv_eps, a.n_split = (ptr(h) if n_c else ptr(X)), inv_eps, _n_split("ot", n_split)
    return a


def ot_softmin(X: torch.Tensor, Y: torch.Tensor, h: torch.Tensor, inv_eps: float, n_split: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """L[i] = log sum_j exp(t_ij), t_ij = fma(-c_ij, inv_eps, h[j]) with c_ij the squared Euclidean distance of ``knn_ops.knn`` (the
    same bits) -> fp32 [n_q].  ``X`` [n_q >= 1, D], ``Y`` [n_c >= 0, D]: fp32 device tensors with unit column stride (row strides may
    exceed D), 1 <= D <= OT_DMAX; ``h`` contiguous fp32 [n_c], -inf marks a candidate without mass.  A t that is not finite adds
    nothing; a query without a contributing candidate gets -inf.  ``n_split``: chunks of the candidates, 0 = ``ot_splits(n_q, n_c)``;
    different values agree within rounding, not bit for bit.  ``out``: a contiguous fp32 tensor [>= n_q]; a view of its first n_q
    entries is returned and nothing else is written.  Deterministic: two calls agree bit for bit."""
    a = _common(X, Y, h, inv_eps, n_split)
    dev, n_q = X.device, int(X.shape[0])
    if out is None:
        out = torch.empty(n_q, dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 1
          or out.numel() < n_q or not out.is_contiguous()):
        raise _abi.SpvError(f"ot_softmin: out must be a contiguous fp32 device tensor with at least {n_q} entries")
    ws = _workspace(ot_ws_bytes(n_q, 0, int(n_split) or ot_splits(n_q, int(Y.shape[0]))), dev)
    a.L, a.ws = ptr(out), ptr(ws)
    _abi.call("spv_ot_softmin", C.byref(a), stream_ptr())
    return out[:n_q]


def ot_topk(X: torch.Tensor, Y: torch.Tensor, h: torch.Tensor, r: torch.Tensor, inv_eps: float, k: int, n_split: int = 0,
            out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """For every row of ``X`` the ``k`` rows of ``Y`` with the largest t_ij (``ot_softmin``'s t, the same bits) -> (idx int32 [n_q, k],
    val fp32 [n_q, k], mass fp32 [n_q]), descending in t, equal t to the smaller index, a non-finite t never: val = exp(t_ij + r[i])
    is the plan entry for r = phi + log a, mass the sum of the row's val in list order; rows with fewer than k selectable candidates
    end in idx = -1 / val = 0.  ``r`` contiguous fp32 [n_q]; 1 <= k <= OT_KMAX; the rest as ``ot_softmin``.  idx is the same for every
    ``n_split``.  ``out``: (idx, val) tensors [n_q, >= k] with one common row stride and unit column stride and mass [>= n_q]; views
    are returned and nothing else is written."""
    a = _common(X, Y, h, inv_eps, n_split)
    dev, n_q = X.device, int(X.shape[0])
    _vector(r, n_q, dev, "r")
    k = _k("ot_topk", k)
    if out is None:
        idx, val, ld_out = _out_pair("ot_topk", None, "val", n_q, k, dev)
        mass = torch.empty(n_q, dtype=torch.float32, device=dev)
    else:
        idx, val, mass = out
        idx, val, ld_out = _out_pair("ot_topk", (idx, val), "val", n_q, k, dev)
        if (not isinstance(mass, torch.Tensor) or not mass.is_cuda or mass.device != dev or mass.dtype != torch.float32 or mass.dim() != 1
                or mass.numel() < n_q or not mass.is_contiguous()):
            raise _abi.SpvError(f"ot_topk: out mass must be a contiguous fp32 device tensor with at least {n_q} entries")
    ws = _workspace(ot_ws_bytes(n_q, k, int(n_split) or ot_splits(n_q, int(Y.shape[0]))), dev)
    a.k, a.r = k, ptr(r)
    a.idx, a.val, a.ld_out = ptr(idx), ptr(val), ld_out
    a.mass, a.ws = ptr(mass), ptr(ws)
    _abi.call("spv_ot_topk", C.byref(a), stream_ptr())
    return idx[:, :k], val[:, :k], mass[:n_q]


def ot_segment_splits(n_q: int, n_c: int) -> int:
    """Chunks of the candidates spv_ot_segment_lse uses for this shape when ``n_split`` is 0: a pure function of the shapes"""
    return int(_abi.load().spv_ot_segment_splits(int(n_q), int(n_c)))


def ot_segment_ws_bytes(n_q: int, n_seg: int, n_split: int) -> int:
    """Bytes of workspace for ``n_split`` chunks (the resolved number, not 0): 0 for one chunk"""
    return int(_abi.load().spv_ot_segment_ws_bytes(int(n_q), int(n_seg), int(n_split)))


def ot_segment_lse(X: torch.Tensor, Y: torch.Tensor, h: torch.Tensor, seg_ptr: torch.Tensor, inv_eps: float, n_split: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """For every row of ``X`` and every segment of the rows of ``Y``: L[i, s] = log sum_{j in segment s} exp(t_ij) with ``ot_softmin``'s
    t (the same bits) -> fp32 device tensor [n_q, n_seg].  The result is the TRANSPOSED VIEW of a segment-major buffer [n_seg, n_q] (the
    kernel's layout), so ``result[:, s]`` is contiguous and ``result[i]`` is strided.  With h = psi + log b of a Sinkhorn result,
    ``exp(L[i, s] + phi_i + log a_i)`` is the mass the untruncated plan puts between cell i and segment s.
    A t that is not finite adds nothing; a segment without a contributing candidate (an empty one included) gives -inf.
    ``X`` [n_q >= 1, D], ``Y`` [n_c >= 0, D], ``h`` [n_c], ``inv_eps``: as ``ot_softmin``.  ``seg_ptr``: contiguous int32 DEVICE tensor
    [n_seg + 1], 1 <= n_seg <= OT_SEG_MAX, ascending from 0 to n_c (segment s is rows seg_ptr[s] .. seg_ptr[s + 1] - 1 of ``Y``).  It is
    not read back for checking: other contents give unspecified values.
    ``n_split``: chunks of the candidates, 0 = ``ot_segment_splits(n_q, n_c)``.  For a fixed value two calls agree bit for bit and a row
    of the result does not depend on the other rows of ``X``; different values agree within rounding.  With one segment and the same
    explicit ``n_split`` the column equals ``ot_softmin``'s result bit for bit.
    ``out``: an fp32 device tensor [n_seg, >= n_q] with unit column stride (segment-major, as stored); the transposed view of its first
    n_q columns is returned and nothing else is written."""
    op = "ot_segment_lse"
    dev, n_q, n_c, D = _sides(op, X, Y, ("X", "Y"))
    _vector(h, n_c, dev, "h")
    inv_eps = float(inv_eps)
    if not (0.0 < inv_eps < math.inf) or not (0.0 < float(np.float32(inv_eps)) < math.inf):
        raise ValueError(f"{op}: inv_eps must be a positive finite number in fp32, got {inv_eps!r}")
    n_split = _n_split(op, n_split)
    if (not isinstance(seg_ptr, torch.Tensor) or not seg_ptr.is_cuda or seg_ptr.device != dev or seg_ptr.dtype != torch.int32 or seg_ptr.dim() != 1
            or not seg_ptr.is_contiguous()):
        raise _abi.SpvError(f"{op}: seg_ptr must be a contiguous int32 device tensor [n_seg + 1]")
    n_seg = int(seg_ptr.numel()) - 1
    if not 1 <= n_seg <= OT_SEG_MAX:
        raise ValueError(f"{op}: the number of segments must lie in [1, {OT_SEG_MAX}], got {n_seg}")
    if out is None:
        out = torch.empty((n_seg, n_q), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 2
          or out.shape[0] != n_seg or out.shape[1] < n_q or (out.shape[1] > 1 and out.stride(1) != 1) or (n_seg > 1 and out.stride(0) < n_q)):
        raise _abi.SpvError(f"{op}: out must be an fp32 device tensor [{n_seg}, >= {n_q}] with unit column stride")
    ws = _workspace(ot_segment_ws_bytes(n_q, n_seg, n_split or ot_segment_splits(n_q, n_c)), dev)
    a = SpvOtSegArgs()
    _fill_sides(a, X, Y)
    a.h, a.inv_eps = (ptr(h) if n_c else ptr(X)), inv_eps
    a.seg_ptr, a.n_seg, a.n_split = ptr(seg_ptr), n_seg, n_split
    a.L, a.ld_l, a.ws = ptr(out), (out.stride(0) if n_seg > 1 else max(n_q, int(out.shape[1]))), ptr(ws)
    _abi.call("spv_ot_segment_lse", C.byref(a), stream_ptr())
    return out[:, :n_q].t()


def ot_project_splits(n_q: int, n_c: int, n_v: int) -> int:
    """Chunks of the candidates spv_ot_project uses for this shape when ``n_split`` is 0: a pure function of the shapes"""
    return int(_abi.load().spv_ot_project_splits(int(n_q), int(n_c), int(n_v)))


def ot_project_ws_bytes(n_q: int, n_v: int, n_split: int) -> int:
    """Bytes of workspace for ``n_split`` chunks (the resolved number, not 0): 0 for one chunk"""
    return int(_abi.load().spv_ot_project_ws_bytes(int(n_q), int(n_v), int(n_split)))


def ot_project_block(D: int) -> int:
    """Value columns per column block of the kernel form that serves ``D`` columns of X / Y"""
    return int(_abi.load().spv_ot_project_block(int(D)))


def ot_project(X: torch.Tensor, Y: torch.Tensor, h: torch.Tensor, V: torch.Tensor, inv_eps: float, n_split: int = 0,
               out: Optional[torch.Tensor] = None, return_lse: bool = False):
    """For every row of ``X`` the mean of the rows of ``V`` under the weights softmax_j(t_ij), ``ot_softmin``'s t (the same bits):
    out[i, v] = sum_j exp(t_ij) V[j, v] / sum_j exp(t_ij) -> fp32 device tensor [n_q, n_v]; with ``return_lse`` (out, L) with
    L[i] = log sum_j exp(t_ij), fp32 [n_q].  The result is the TRANSPOSED VIEW of a value-major buffer [n_v, n_q] (the kernel's
    layout), so ``result[:, v]`` is contiguous and ``result[i]`` is strided.  With h = psi + log b of a Sinkhorn result this is the
    barycentric projection through the untruncated plan.
    A t that is not finite adds nothing, whatever its row of ``V`` holds; a query without a contributing candidate gets NaN in every
    column and L = -inf.  A column of ones comes back as exactly 1.
    ``X`` [n_q >= 1, D], ``Y`` [n_c >= 0, D], ``h`` [n_c], ``inv_eps``: as ``ot_softmin``.  ``V``: fp32 device tensor [n_c, n_v],
    1 <= n_v <= OT_VAL_MAX, unit column stride (the row stride may exceed n_v).
    ``n_split``: chunks of the candidates, 0 = ``ot_project_splits(n_q, n_c, n_v)``.  For a fixed value two calls agree bit for bit, a
    row of the result does not depend on the other rows of ``X`` and a column not on the other columns of ``V``; different values
    agree within rounding.  L equals ``ot_softmin``'s at the same explicit ``n_split`` bit for bit.
    ``out``: an fp32 device tensor [n_v, >= n_q] with unit column stride (value-major, as stored); the transposed view of its first
    n_q columns is returned and nothing else is written.  With ``return_lse`` a pair (out, L) is taken too, L a contiguous fp32 device
    tensor [>= n_q] of which the first n_q entries are written and returned."""
    op = "ot_project"
    dev, n_q, n_c, D = _sides(op, X, Y, ("X", "Y"))
    _vector(h, n_c, dev, "h")
    inv_eps = float(inv_eps)
    if not (0.0 < inv_eps < math.inf) or not (0.0 < float(np.float32(inv_eps)) < math.inf):
        raise ValueError(f"{op}: inv_eps must be a positive finite number in fp32, got {inv_eps!r}")
    n_split = _n_split(op, n_split)
    if (not isinstance(V, torch.Tensor) or not V.is_cuda or V.device != dev or V.dtype != torch.float32 or V.dim() != 2 or V.shape[0] != n_c
            or V.shape[1] < 1 or (n_c > 0 and V.shape[1] > 1 and V.stride(1) != 1) or (n_c > 1 and V.stride(0) < V.shape[1])):
        raise _abi.SpvError(f"{op}: V must be an fp32 device tensor [{n_c}, n_v] with unit column stride")
    n_v = int(V.shape[1])
    if n_v > OT_VAL_MAX:
        raise ValueError(f"{op}: V must have between 1 and {OT_VAL_MAX} columns, got {n_v}")
    L = None
    if isinstance(out, (tuple, list)):
        if len(out) != 2 or not return_lse:
            raise _abi.SpvError(f"{op}: out must be one tensor, or with return_lse a pair (out, L)")
        out, L = out
        if (not isinstance(L, torch.Tensor) or not L.is_cuda or L.device != dev or L.dtype != torch.float32 or L.dim() != 1 or L.numel() < n_q
                or not L.is_contiguous()):
            raise _abi.SpvError(f"{op}: out L must be a contiguous fp32 device tensor with at least {n_q} entries")
    if out is None:
        out = torch.empty((n_v, n_q), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 2
          or out.shape[0] != n_v or out.shape[1] < n_q or (out.shape[1] > 1 and out.stride(1) != 1) or (n_v > 1 and out.stride(0) < n_q)):
        raise _abi.SpvError(f"{op}: out must be an fp32 device tensor [{n_v}, >= {n_q}] with unit column stride")
    if return_lse and L is None:
        L = torch.empty(n_q, dtype=torch.float32, device=dev)
    ws = _workspace(ot_project_ws_bytes(n_q, n_v, n_split or ot_project_splits(n_q, n_c, n_v)), dev)
    a = SpvOtProjArgs()
    _fill_sides(a, X, Y)
    a.h, a.inv_eps, a.n_split = (ptr(h) if n_c else ptr(X)), inv_eps, n_split
    a.V, a.ld_v, a.n_v = (ptr(V) if n_c else None), (V.stride(0) if n_c > 1 else n_v), n_v
    a.out, a.ld_out = ptr(out), (out.stride(0) if n_v > 1 else max(n_q, int(out.shape[1])))
    a.L, a.ws = ptr(L), ptr(ws)
    _abi.call("spv_ot_project", C.byref(a), stream_ptr())
    res = out[:, :n_q].t()
    return (res, L[:n_q]) if return_lse else res


def mean_sq_cost(X0: torch.Tensor, X1: torch.Tensor) -> float:
    """The mean of |x_i - y_j|^2 over ALL pairs in closed form from the moments, in fp64: mean|x|^2 + mean|y|^2 - 2 mean(x).mean(y).
    No pairwise pass."""
    x, y = X0.detach().double(), X1.detach().double()
    return float((x * x).sum(1).mean() + (y * y).sum(1).mean() - 2.0 * torch.dot(x.mean(0), y.mean(0)))


def _marginal(w, n: int, dev, name: str) -> torch.Tensor:
    """log of a marginal as fp32 [n]: uniform by default; zeros are allowed and become -inf"""
    if w is None:
        return torch.full((n,), -math.log(n), dtype=torch.float32, device=dev)
    w = torch.as_tensor(w).detach().to(dev, torch.float64).reshape(-1)
    if w.numel() != n or not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not float(w.sum()) > 0:
        raise ValueError(f"sinkhorn: {name} must hold {n} finite non-negative weights with a positive sum")
    return torch.log(w / w.sum()).to(torch.float32)


@dataclass
class SinkhornResult:
    """``phi`` [n0], ``psi`` [n1]: the dimensionless potentials (fp32 device tensors); ``log_a`` / ``log_b`` the log marginals;
    ``inv_eps`` the scalar s the kernels saw (1 / (epsilon x cost scale)); ``cost_scale`` what the cost was divided by;
    ``n_iter`` iterations run; ``error`` the last max_i |phi_new - phi_old| read (nan if never read); ``converged``: error <= tol."""
    phi: torch.Tensor
    psi: torch.Tensor
    log_a: torch.Tensor
    log_b: torch.Tensor
    inv_eps: float
    cost_scale: float
    n_iter: int
    error: float
    converged: bool


def sinkhorn(X0: torch.Tensor, X1: torch.Tensor, epsilon: float = 0.05, scale_cost: Optional[str] = "mean", a=None, b=None,
             max_iter: int = 2000, tol: float = 1e-3, check_every: int = 10) -> SinkhornResult:
    """Log-domain Sinkhorn iterations between the rows of ``X0`` [n0, D] and ``X1`` [n1, D] (fp32 device tensors) with cost
    c_ij = |x_i - y_j|^2 and plan P_ij = a_i b_j exp(phi_i + psi_j - s c_ij).  ``scale_cost="mean"`` divides the cost by the mean of all
    c_ij (``mean_sq_cost``), ``None`` uses ``epsilon`` as given: s = 1 / (epsilon x scale).  ``a`` / ``b``: the marginals, uniform by default,
    normalised to sum 1; zeros are allowed.  One iteration is phi = -softmin(X0, X1, psi + log b), then psi = -softmin(X1, X0, phi + log a).
    Every ``check_every`` iterations the host reads max_i |phi_new - phi_old| over the cells with mass -- the largest log-deviation of
    the row marginal -- ONCE and stops at <= ``tol``; ``tol=0`` runs all ``max_iter``."""
    _rows("ot", X0, "X0"), _rows("ot", X1, "X1")
    if X0.device != X1.device or X0.shape[1] != X1.shape[1]:
        raise _abi.SpvError("sinkhorn: X0 and X1 must share a device and have the same number of columns")
    n0, n1, dev = int(X0.shape[0]), int(X1.shape[0]), X0.device
    if n0 < 1 or n1 < 1:
        raise ValueError("sinkhorn: both groups need at least one row")
    if scale_cost not in ("mean", None):
        raise ValueError(f"sinkhorn: scale_cost must be 'mean' or None, got {scale_cost!r}")
    if not (float(epsilon) > 0 and math.isfinite(float(epsilon))):
        raise ValueError(f"sinkhorn: epsilon must be a positive finite number, got {epsilon!r}")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1 or int(check_every) != check_every or int(check_every) < 1:
        raise ValueError("sinkhorn: max_iter and check_every must be positive integers")
    if not float(tol) >= 0:
        raise ValueError(f"sinkhorn: tol must be >= 0, got {tol!r}")
    scale = mean_sq_cost(X0, X1) if scale_cost == "mean" else 1.0
    if not (scale > 0 and math.isfinite(scale)):
        raise ValueError("sinkhorn: the mean cost is not a positive finite number (all points equal, or non-finite input)")
    s = float(np.float32(1.0 / (float(epsilon) * scale)))
    log_a, log_b = _marginal(a, n0, dev, "a"), _marginal(b, n1, dev, "b")
    live = torch.isfinite(log_a)
    phi, psi = torch.zeros(n0, dtype=torch.float32, device=dev), torch.zeros(n1, dtype=torch.float32, device=dev)
    L0, L1 = torch.empty_like(phi), torch.empty_like(psi)
    n_iter, err, done = 0, float("nan"), False
    for it in range(1, int(max_iter) + 1):
        ot_softmin(X0, X1, psi + log_b, s, out=L0)
        check = tol > 0 and (it % int(check_every) == 0 or it == int(max_iter))
        if check:
            delta = torch.where(live, (L0 + phi).abs(), torch.zeros_like(phi)).max()   # phi_new = -L0
        torch.neg(L0, out=phi)
        ot_softmin(X1, X0, phi + log_a, s, out=L1)
        torch.neg(L1, out=psi)
        n_iter = it
        if check:
            err = float(delta)   # the one host sync
            if err <= tol:
                done = True
                break
    return SinkhornResult(phi, psi, log_a, log_b, s, scale, n_iter, err, done)


def transport_project(res: SinkhornResult, X_q: torch.Tensor, X_c: torch.Tensor, V: torch.Tensor, side: int):
    """The barycentric projection of the value rows ``V`` [n_c, n_v] of the candidate cells ``X_c`` onto the query cells ``X_q`` through
    the UNTRUNCATED plan P = a b exp(phi + psi - s c) of the Sinkhorn result ``res``: out[i] = sum_j P_ij V[j] / sum_j P_ij
    -> (out fp32 device tensor [n_q, n_v], mass host fp64 [n_q]).  ``side``: the group of the QUERIES, 0 (``X_q`` is the X0 the
    potentials were computed on, ``X_c`` the X1) or 1 (the other way round), as ``cluster_ops.cluster_transport_log_mass``.
    mass_i = exp(L_i + r_i), r the queries' potential plus log marginal, formed in fp64 on the host: the row mass of the untruncated
    plan, equal to the cell's marginal at convergence -- a diagnostic.  ``V`` with at most OT_VAL_MAX columns: one ``ot_project`` call."""
    if side not in (0, 1):
        raise ValueError(f"side must be 0 or 1, got {side!r}")
    pot_q, pot_c = (res.phi + res.log_a, res.psi + res.log_b)[::1 if side == 0 else -1]
    if pot_c.shape[0] != X_c.shape[0] or pot_q.shape[0] != X_q.shape[0]:
        raise ValueError("transport_project: the potentials' sizes must match the two sides")
    out, L = ot_project(X_q, X_c, pot_c, V, res.inv_eps, return_lse=True)
    with np.errstate(over="ignore"):
        mass = np.exp(L.cpu().numpy().astype(np.float64) + pot_q.cpu().numpy().astype(np.float64))
    return out, mass


class TransportPlan:
    """What ``transport_plan`` returns: the sparse plan as CSR arrays on the host (``indptr`` int64 [n0 + 1], ``indices`` int32,
    ``data`` fp32; columns ascending within a row), the Sinkhorn result (``sinkhorn``: potentials and diagnostics) and the share of
    every cell's mass the truncation to k entries per pass kept: ``row_kept`` = row_mass / a [n0], ``col_kept`` = col_mass / b [n1]
    (numpy fp32; nan for a cell without mass).  ``row_mass`` / ``col_mass`` are the kernels' own sums of each pass's kept entries."""

    def __init__(self, indptr, indices, data, shape, sinkhorn_result, row_mass, col_mass, row_kept, col_kept, k):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, (int(shape[0]), int(shape[1]))
        self.sinkhorn, self.k = sinkhorn_result, int(k)
        self.row_mass, self.col_mass, self.row_kept, self.col_kept = row_mass, col_mass, row_kept, col_kept

    @property
    def nnz(self) -> int:
        return int(self.indices.shape[0])

    def to_scipy(self):
        """scipy CSR [n0, n1], fp32"""
        import scipy.sparse as sp

        return sp.csr_matrix((self.data, self.indices, self.indptr), shape=self.shape)

    def sparse_plan(self, device):
        """the device-resident form the PoE kernels walk (plan.SparsePlan)"""
        from .plan import SparsePlan

        return SparsePlan.from_scipy(self.to_scipy(), device)


def transport_plan(X0: torch.Tensor, X1: torch.Tensor, k: int = 32, **sinkhorn_kwargs) -> TransportPlan:
    """``sinkhorn``, then two ``ot_topk`` passes -- every cell of group 0 against group 1 and every cell of group 1 against group 0,
    ``k`` entries each -- and their union as one sparse plan; a pair both passes kept takes the row pass's value."""
    k = _k("transport_plan", k)
    res = sinkhorn(X0, X1, **sinkhorn_kwargs)
    rows = ot_topk(X0, X1, res.psi + res.log_b, res.phi + res.log_a, res.inv_eps, k)
    cols = ot_topk(X1, X0, res.phi + res.log_a, res.psi + res.log_b, res.inv_eps, k)
    host = [t.cpu().numpy() for t in (*rows, *cols)]
    indptr, indices, data = plan_union_csr(host[0], host[1], host[3], host[4], X0.shape[0], X1.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        row_kept = (host[2] / np.exp(res.log_a.cpu().numpy())).astype(np.float32)
        col_kept = (host[5] / np.exp(res.log_b.cpu().numpy())).astype(np.float32)
    return TransportPlan(indptr, indices, data, (X0.shape[0], X1.shape[0]), res, host[2], host[5], row_kept, col_kept, k)
