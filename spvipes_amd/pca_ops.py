"""PCA of the log-normalised observed counts on the device: the operand stage and the two skinny products spv_pca_stage /
spv_pca_project / spv_pca_back (csrc/spv_pca.h; include/spvipes_hip.h states the contract), the operator X^T X they make of one or two
groups' resident count matrices, and a block Lanczos iteration on it.  ``spVIPES.count_pca`` / ``spVIPES.pca`` build their result from
``count_pca`` below; the matrix X of log-normalised, centred, scaled values is never stored."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _abi
from ._abi import PCA_COLUMNS, SpvCsrGatherArgs, SpvPcaArgs, ptr, round_up, stream_ptr
from .count_ops import COUNT_CHUNK_ROWS, count_totals
from .data import pca_block, pca_sign_flip
from .ops import GroupCounts, SparseGroupCounts

DENSE_PIECE_ROWS = 4 * COUNT_CHUNK_ROWS   # a dense matrix is passed this many list positions at a time: the back workspace stays at 16 slabs
_WS = {}                                  # device -> the cached back workspace (uint8), grown on demand


def pca_slab() -> int:
    """List positions per slab of spv_pca_back; a piece must start on a multiple of it"""
    return int(_abi.load().spv_pca_slab())


def pca_cell_tile() -> int:
    """List positions per workgroup of spv_pca_project"""
    return int(_abi.load().spv_pca_cell_tile())


def pca_ws_bytes(G: int, n_piece: int, l: int) -> int:
    """spv_pca_ws_bytes: 4 * ceil(n_piece / slab) * round_up(G, 64) * l (0 outside the ranges)"""
    return int(_abi.load().spv_pca_ws_bytes(int(G), int(n_piece), int(l)))


def _workspace(device, need: int) -> torch.Tensor:
    ws = _WS.get(device)
    if ws is None or ws.numel() < need:
        _WS.pop(device, None)
        ws = None
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
        _WS[device] = ws
    return ws


def _check_list(fn: str, counts, rows, w):
    if not isinstance(counts, (GroupCounts, SparseGroupCounts)):
        raise _abi.SpvError(f"{fn}: counts must be a GroupCounts or a SparseGroupCounts, got {type(counts).__name__}")
    dev = counts.device
    if (not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.device != dev or rows.dtype != torch.int32 or rows.dim() != 1
            or not rows.is_contiguous() or rows.numel() < 1):
        raise _abi.SpvError(f"{fn}: rows must be a non-empty contiguous 1-d int32 tensor on the counts' device")
    if w is not None and (not isinstance(w, torch.Tensor) or w.device != dev or w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous()
                          or w.numel() != rows.numel()):
        raise _abi.SpvError(f"{fn}: w must be a contiguous 1-d float32 tensor on the counts' device with one entry per listed row ({rows.numel()})")
    lo, hi = (int(v) for v in torch.aminmax(rows))
    if lo < 0 or hi >= counts.n_cells:
        raise ValueError(f"{fn}: rows must lie in [0, {counts.n_cells}), got values from {lo} to {hi}")


def pieces(counts, rows: torch.Tensor, piece_rows: Optional[int] = None):
    """The list ``rows`` of a ``GroupCounts`` or ``SparseGroupCounts`` in slab-aligned pieces, in list order: yields
    (spv_counts struct, n_rows, pos_off, n_piece) for the kernels.  A dense matrix is addressed through the piece's row numbers; a CSR
    matrix is densified ``COUNT_CHUNK_ROWS`` listed rows at a time by spv_csr_gather (one buffer, refilled per piece: a piece must be
    consumed before the next one is asked for), as ``rank_ops._stage`` does."""
    n = int(rows.numel())
    if isinstance(counts, SparseGroupCounts):
        step = COUNT_CHUNK_ROWS
        ldx = round_up(counts.G, 8)
        buf = torch.empty((min(n, step), ldx), dtype=torch.float32 if counts.dtype == _abi.SPV_COUNT_F32 else torch.int16, device=counts.device)
        dense = GroupCounts(buf, counts.G, 0)
        for p0 in range(0, n, step):
            p1 = min(p0 + step, n)
            piece = rows[p0:p1]
            g = (SpvCsrGatherArgs * 1)()
            g[0].indptr, g[0].cols, g[0].vals, g[0].n_rows, g[0].G, g[0].dtype = ptr(counts.indptr), ptr(counts.cols), ptr(counts.vals), counts.n_cells, counts.G, counts.dtype
            g[0].B, g[0].rows, g[0].X, g[0].ldx = p1 - p0, ptr(piece), ptr(buf), ldx
            g[0].xb, g[0].ld_xb, g[0].xb_split, g[0].library = None, 0, 0, None
            _abi.call("spv_csr_gather", g, 1, stream_ptr())
            yield dense.c_struct(None), p1 - p0, p0, p1 - p0
        return
    step = int(piece_rows or DENSE_PIECE_ROWS)
    if step % pca_slab():
        raise ValueError(f"pieces: piece_rows must be a multiple of the slab ({pca_slab()}), got {step}")
    for p0 in range(0, n, step):
        p1 = min(p0 + step, n)
        yield counts.c_struct(rows[p0:p1]), counts.n_cells, p0, p1 - p0


def _args(G: int, n: int, l: int, w, mu, scale) -> SpvPcaArgs:
    a = SpvPcaArgs()
    a.G, a.n, a.l, a.w, a.mu, a.scale = int(G), int(n), int(l), ptr(w), ptr(mu), ptr(scale)
    return a


def stage_block(counts, rows: torch.Tensor, w=None, mu=None, scale=None, piece_rows: Optional[int] = None):
    """The operand itself, piece by piece: yields (pos_off, block fp32 [n_piece, G]) with block[p - pos_off, j] = x(p, j) =
    (log1p(count * w[p]) - mu[j]) * scale[j] as the kernels form it (spv_pca_stage).  The block is one buffer, refilled per piece."""
    _check_list("stage_block", counts, rows, w)
    G, n = int(counts.G), int(rows.numel())
    a = _args(G, n, 16, w, mu, scale)
    out = None
    for cs, n_rows, p0, m in pieces(counts, rows, piece_rows or COUNT_CHUNK_ROWS):
        if out is None:
            out = torch.empty((m, G), dtype=torch.float32, device=counts.device)
        a.x, a.n_rows, a.pos_off, a.n_piece, a.block, a.ld_block = cs, n_rows, p0, m, ptr(out), G
        _abi.call("spv_pca_stage", C.byref(a), stream_ptr())
        yield p0, out[:m]


def lognorm_moments(counts, rows: torch.Tensor, w: Optional[torch.Tensor] = None):
    """Per gene the sum and the sum of squares of a = log1p(count * w[p]) over the LISTED cells -> (sum fp64 [G], sum of squares fp64
    [G]) on the device.  The values are the kernels' own (spv_pca_stage with mu = 0, scale = 1), widened and reduced in torch fp64,
    ``COUNT_CHUNK_ROWS`` list positions at a time in list order -- the pattern of ``count_ops.count_square_sums``: one staged fp32 block
    and two fp64 temporaries of chunk rows x G.  A kernel of its own (two more rows of spv_count_stats) is the later home of this."""
    G = int(counts.G)
    s = torch.zeros((G,), dtype=torch.float64, device=counts.device)
    q = torch.zeros((G,), dtype=torch.float64, device=counts.device)
    for _p0, block in stage_block(counts, rows, w):
        b = block.to(torch.float64)
        s += b.sum(0)
        q += (b * b).sum(0)
    return s, q


@dataclass
class PcaGroup:
    """One group's part of the operator: its counts, the listed rows (int32 device [n_g]), the weights (fp32 device [n_g] or None), mu and
    scale (fp32 device [G_g]; scale 0 for a gene outside the pairing) and ``cols`` (int64 device [p]): joint column t is gene cols[t]"""
    counts: object
    rows: torch.Tensor
    w: Optional[torch.Tensor]
    mu: torch.Tensor
    scale: torch.Tensor
    cols: torch.Tensor


class PcaOperator:
    """X^T X of the stacked groups, X [n, p] = the listed cells of group 0, then group 1's, over the p joint columns; never stored.
    ``apply(V)`` with a joint V fp32 [p, l], l in (16, 32, 48, 64): V is scattered into each group's [G_g, l] image (zero rows for genes
    outside the pairing), project then back run per group and per piece, and the groups' paired rows of Z are added -> (Z fp64 [p, l],
    Y fp32 [n, l], the stacked projections).  Every kernel sum has a fixed order: two calls agree bit for bit."""

    def __init__(self, groups: List[PcaGroup]):
        if not groups:
            raise ValueError("PcaOperator: at least one group")
        self.groups = list(groups)
        self.p = int(groups[0].cols.numel())
        for g in self.groups:
            _check_list("PcaOperator", g.counts, g.rows, g.w)
            if int(g.cols.numel()) != self.p:
                raise ValueError("PcaOperator: every group maps the same joint columns")
        self.device = groups[0].counts.device
        self.n = sum(int(g.rows.numel()) for g in self.groups)
        self.n_apply = 0

    def project(self, V: torch.Tensor) -> torch.Tensor:
        """Y fp32 [n, l] = X V alone"""
        return self._run(V, None, None)[1]

    def apply(self, V: torch.Tensor):
        """-> (Z fp64 [p, l] = X^T (X V), Y fp32 [n, l] = X V)"""
        Z = torch.zeros((self.p, V.shape[1]), dtype=torch.float64, device=self.device)
        return self._run(V, Z, None)

    def back(self, Y: torch.Tensor) -> torch.Tensor:
        """Z fp64 [p, l] = X^T Y alone, for a contiguous fp32 device tensor Y [n, l] (the final pass never needs it apart; the
        benchmark times it)"""
        l = int(Y.shape[1]) if Y.dim() == 2 else 0
        if Y.dim() != 2 or Y.shape[0] != self.n or l not in PCA_COLUMNS or Y.dtype != torch.float32 or Y.device != self.device or not Y.is_contiguous():
            raise _abi.SpvError(f"PcaOperator: Y must be a contiguous fp32 device tensor [{self.n}, l] with l one of {PCA_COLUMNS}")
        Z = torch.zeros((self.p, l), dtype=torch.float64, device=self.device)
        return self._run(None, Z, Y)[0]

    def _run(self, V: Optional[torch.Tensor], Z: Optional[torch.Tensor], Y: Optional[torch.Tensor]):
        """project (``V`` given) and / or back (``Z`` given; onto the Y just projected, or the ``Y`` handed in) group by group"""
        if V is not None:
            l = int(V.shape[1]) if V.dim() == 2 else 0
            if V.dim() != 2 or V.shape[0] != self.p or l not in PCA_COLUMNS or V.dtype != torch.float32 or V.device != self.device:
                raise _abi.SpvError(f"PcaOperator: V must be an fp32 device tensor [{self.p}, l] with l one of {PCA_COLUMNS}")
            Y = torch.empty((self.n, l), dtype=torch.float32, device=self.device)
        else:
            l = int(Y.shape[1])
        n0 = 0
        for g in self.groups:
            G, n_g = int(g.counts.G), int(g.rows.numel())
            Yg = Y[n0:n0 + n_g]
            Zg = torch.zeros((G, l), dtype=torch.float64, device=self.device) if Z is not None else None
            a = _args(G, n_g, l, g.w, g.mu, g.scale)
            a.Y, a.ld_y = ptr(Yg), l
            if V is not None:
                Vg = torch.zeros((G, l), dtype=torch.float32, device=self.device)
                Vg.index_copy_(0, g.cols, V)
                a.V, a.ld_v = ptr(Vg), l
            if Zg is not None:
                a.Z, a.ld_z = ptr(Zg), l
            dense = isinstance(g.counts, GroupCounts)
            if dense and V is not None:   # a resident dense matrix is projected in ONE launch (a piece of 16 384 positions is one workgroup per CU); back goes by pieces
                a.x, a.n_rows, a.pos_off, a.n_piece = g.counts.c_struct(g.rows), g.counts.n_cells, 0, n_g
                _abi.call("spv_pca_project", C.byref(a), stream_ptr())
            for cs, n_rows, p0, m in (pieces(g.counts, g.rows) if (Zg is not None or not dense) else ()):
                a.x, a.n_rows, a.pos_off, a.n_piece = cs, n_rows, p0, m
                if not dense and V is not None:
                    _abi.call("spv_pca_project", C.byref(a), stream_ptr())
                if Zg is not None:
                    ws = _workspace(self.device, pca_ws_bytes(G, m, l))
                    a.ws, a.ws_bytes = ptr(ws), ws.numel()
                    _abi.call("spv_pca_back", C.byref(a), stream_ptr())
            if Z is not None:
                Z += Zg.index_select(0, g.cols)
            n0 += n_g
        self.n_apply += 1
        return Z, Y


@dataclass
class LanczosResult:
    theta: torch.Tensor       # fp64 [n_comps], descending: the Ritz values
    vectors: torch.Tensor     # fp64 [p, n_comps]: the Ritz vectors
    residuals: torch.Tensor   # fp64 [n_comps]: || Z S - Q S theta || of the last Rayleigh-Ritz step
    n_blocks: int
    n_restarts: int
    converged: bool


def _orthonormal(W: torch.Tensor) -> torch.Tensor:
    return torch.linalg.qr(W, mode="reduced")[0]


def block_lanczos(op, n_comps: int, block: Optional[int] = None, tol: float = 1e-4, max_blocks: int = 12, seed: int = 0, max_restarts: int = 4) -> LanczosResult:
    """The ``n_comps`` largest eigenpairs of ``op`` (anything with ``p``, ``device`` and ``apply(V fp32 [p, l]) -> (Z fp64 [p, l], _)``)
    by a block Lanczos iteration with full reorthogonalisation and Rayleigh-Ritz.
    Start: a seeded fp64 Gaussian [p, l] drawn on the host, orthonormalised.  Each step rounds the block to fp32 -- what the kernels
    read -- and keeps the ROUNDED block as the basis Q; Z = op.apply(block); T = Q^T Z, symmetrised; eigh(T).  For the top n_comps Ritz
    pairs (theta, S) the residual columns are Z S - Q S theta; the iteration stops when the largest residual 2-norm is at most tol *
    theta_1.  Otherwise Z's newest block is orthogonalised against the whole basis twice, QR'd, and becomes the next block.  At
    ``max_blocks`` (or when the basis would exceed p columns) it restarts from the top l Ritz vectors; after ``max_restarts`` restarts
    it returns with ``converged=False`` -- not an exception.  The small algebra is torch fp64 on the device.
    ``block``: l, one of 16, 32, 48, 64 (default min(64, round_up(n_comps + 8, 16))), n_comps <= l <= p."""
    p, dev = int(op.p), op.device
    l = pca_block(n_comps) if block is None else int(block)
    if l not in PCA_COLUMNS or not 1 <= n_comps <= l:
        raise ValueError(f"block_lanczos: block must be one of {PCA_COLUMNS} and at least n_comps ({n_comps}), got {l}")
    if l > p:
        raise ValueError(f"block_lanczos: the block ({l}) exceeds the operator's size ({p})")
    most = max(1, min(int(max_blocks), p // l))
    start = torch.from_numpy(np.random.default_rng(int(seed)).standard_normal((p, l))).to(dev)
    cur = _orthonormal(start)
    n_blocks = n_restarts = 0
    while True:
        Q = torch.empty((p, 0), dtype=torch.float64, device=dev)
        AQ = torch.empty((p, 0), dtype=torch.float64, device=dev)
        for _step in range(most):
            v32 = cur.to(torch.float32)
            Z, _Y = op.apply(v32)
            n_blocks += 1
            Q = torch.cat([Q, v32.to(torch.float64)], 1)
            AQ = torch.cat([AQ, Z], 1)
            T = Q.T @ AQ
            theta, S = torch.linalg.eigh(0.5 * (T + T.T))
            theta, S = theta.flip(0), S.flip(1)
            top = S[:, :n_comps]
            R = AQ @ top - (Q @ top) * theta[:n_comps]
            res = torch.linalg.vector_norm(R, dim=0)
            if float(res.max()) <= tol * float(theta[0]):
                return LanczosResult(theta[:n_comps], Q @ top, res, n_blocks, n_restarts, True)
            if Q.shape[1] + l > p or _step + 1 == most:
                break
            W = Z
            for _twice in range(2):
                W = W - Q @ (Q.T @ W)
            cur = _orthonormal(W)
        if n_restarts >= max_restarts:
            return LanczosResult(theta[:n_comps], Q @ top, res, n_blocks, n_restarts, False)
        n_restarts += 1
        cur = _orthonormal(Q @ S[:, :l])


def count_pca(groups, cols, n_comps: int, normalize: bool = True, target_sum: float = 1e4, scale: bool = False, tol: float = 1e-4, seed: int = 0,
              block: Optional[int] = None, max_blocks: int = 12, max_restarts: int = 4) -> dict:
    """PCA of log1p(count * target_sum / total) over the stacked listed cells of one or two groups.  ``groups``: [(counts, rows int32
    device [n_g])]; ``cols``: per group the int32 positions [p] of the joint columns among its genes (a gene selection, or the pairing).
    Weights as ``rank_genes_groups``: fp32(target_sum / the cell's total over ALL of its group's genes), 0 for a cell without counts;
    ``normalize=False``: no weight.  Moments from ``lognorm_moments``; centring by the joint mean; ``scale=True`` divides by the joint
    standard deviation (ddof 1; a gene without variance gets scale 0).  -> dict of ``scores`` (fp32 device [n, n_comps]), ``components``
    (fp64 [n_comps, p], numpy), ``mean``, ``var``, ``theta``, ``variance``, ``variance_ratio``, ``residuals``, ``n_blocks``,
    ``n_restarts``, ``converged``."""
    dev = groups[0][0].device
    p = len(cols[0])
    n = sum(int(r.numel()) for _c, r in groups)
    ws, sums, sqs = [], torch.zeros(p, dtype=torch.float64, device=dev), torch.zeros(p, dtype=torch.float64, device=dev)
    dev_cols = [torch.as_tensor(np.asarray(c), dtype=torch.int64, device=dev) for c in cols]
    for (counts, rows), dc in zip(groups, dev_cols):
        w = None
        if normalize:
            total = count_totals(counts).index_select(0, rows.long())
            w = torch.where(total > 0, target_sum / total, torch.zeros_like(total)).to(torch.float32)
        ws.append(w)
        s, q = lognorm_moments(counts, rows, w)
        sums += s.index_select(0, dc)
        sqs += q.index_select(0, dc)
    mean = sums / n
    var = torch.clamp(sqs - n * mean * mean, min=0.0) / (n - 1)
    sc = torch.where(var > 0, 1.0 / torch.sqrt(var), torch.zeros_like(var)) if scale else torch.ones_like(var)
    total_var = float((var * sc * sc).sum())
    parts = []
    for (counts, rows), dc, w in zip(groups, dev_cols, ws):
        G = int(counts.G)
        mu_g = torch.zeros(G, dtype=torch.float32, device=dev)
        sc_g = torch.zeros(G, dtype=torch.float32, device=dev)
        mu_g.index_copy_(0, dc, mean.to(torch.float32))
        sc_g.index_copy_(0, dc, sc.to(torch.float32))
        parts.append(PcaGroup(counts, rows, w, mu_g, sc_g, dc))
    op = PcaOperator(parts)
    lz = block_lanczos(op, n_comps, block=block, tol=tol, max_blocks=max_blocks, seed=seed, max_restarts=max_restarts)
    # the final pass: Ritz vectors -> sign rule -> the fp32 vectors that are returned -> their scores and their own residuals
    l = pca_block(n_comps) if block is None else int(block)
    vec = lz.vectors.cpu().numpy()
    vec = vec * pca_sign_flip(vec.T)[None, :]
    V32 = torch.zeros((p, l), dtype=torch.float32, device=dev)
    V32[:, :n_comps] = torch.from_numpy(vec).to(dev).to(torch.float32)
    Z, Y = op.apply(V32)
    U = V32[:, :n_comps].to(torch.float64)
    Zc = Z[:, :n_comps]
    theta = (U * Zc).sum(0) / (U * U).sum(0)
    residuals = torch.linalg.vector_norm(Zc - U * theta, dim=0) / torch.linalg.vector_norm(U, dim=0)
    variance = theta / (n - 1)
    return dict(scores=Y[:, :n_comps].contiguous(), components=U.T.cpu().numpy(), mean=mean.cpu().numpy(), var=var.cpu().numpy(),
                theta=theta.cpu().numpy(), variance=variance.cpu().numpy(), variance_ratio=(variance / total_var).cpu().numpy(),
                residuals=residuals.cpu().numpy(), n_blocks=lz.n_blocks, n_restarts=lz.n_restarts, converged=bool(lz.converged),
                n_apply=op.n_apply, block=l)
