"""Rank sums of the observed counts on the device: the segmented column sort spv_rank_stage / spv_rank_sums over listed rows of a
resident count matrix (csrc/spv_rank.h; include/spvipes_hip.h states the contract).  ``spVIPES.rank_genes_groups`` builds its Wilcoxon
table from them; nothing but the integer tables leaves the device."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi
from ._abi import RANK_MAX_N, RANK_MAX_SEG, SpvCsrGatherArgs, SpvRankArgs, ptr, round_up, stream_ptr
from .count_ops import COUNT_CHUNK_ROWS
from .ops import GroupCounts, SparseGroupCounts

WS_BUDGET_BYTES = 1 << 30   # what the two halves of the sort workspace may take together: rank_gene_slab cuts the gene slabs to it
_WS = {}                    # device -> the cached workspace (uint8), grown on demand


def rank_lds_capacity() -> int:
    """Non-zero keys of one gene that the LDS-resident sort holds; a gene with more takes the radix passes through the workspace"""
    return int(_abi.load().spv_rank_lds_capacity())


def rank_stage_tile() -> int:
    """List positions per workgroup of the stage"""
    return int(_abi.load().spv_rank_stage_tile())


def rank_sort_tile() -> int:
    """Entries one tile of a radix pass moves"""
    return int(_abi.load().spv_rank_sort_tile())


def rank_ws_bytes(n: int, n_sel: int) -> int:
    """spv_rank_ws_bytes: 8192 + 16 n n_sel for a list of n positions and a slab of n_sel genes (0 outside the ranges)"""
    return int(_abi.load().spv_rank_ws_bytes(int(n), int(n_sel)))


def rank_gene_slab(n: int) -> int:
    """Genes per call for a list of ``n`` positions: the most the kernel takes (spv_rank_gene_slab(), 1024) cut so that the workspace,
    16 bytes per (position, gene), stays within ``WS_BUDGET_BYTES`` -- but at least one gene.  The workspace of ``rank_sums`` is therefore
    at most 8192 + max(WS_BUDGET_BYTES, 16 n) bytes: 1 GiB + 8 KiB at the default budget for every n up to the cap 2^20."""
    return max(1, min(int(_abi.load().spv_rank_gene_slab()), WS_BUDGET_BYTES // (16 * max(int(n), 1))))


def _workspace(device, need: int) -> torch.Tensor:
    ws = _WS.get(device)
    if ws is None or ws.numel() < need:
        _WS.pop(device, None)
        ws = None   # (the old block is released before the larger one is taken)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _WS[device] = ws
    return ws


def rank_sums(counts, rows: torch.Tensor, seg: torch.Tensor, n_seg: int, w: Optional[torch.Tensor] = None, genes: Optional[torch.Tensor] = None):
    """For the LISTED cells ``rows`` (int32 device tensor [n], 1 <= n <= 2^20, any order, repeats allowed) of a ``GroupCounts`` or
    ``SparseGroupCounts``, with one segment code ``seg[p]`` (int32 device tensor [n]) per list position: -> (rank2 int64 [n_seg, n_sel],
    ties int64 [n_sel]) on the device.  Per selected gene, key[p] = fl32(float(count) * w[p]) (``w``: fp32 device tensor [n] of
    non-negative weights aligned with ``rows``; None: the count itself); rank2[k, j] is the sum over segment k's positions of TWICE the
    position's average rank among all n keys of gene j (ties share their mean rank), ties[j] the sum of t^3 - t over the runs of equal
    keys.  Integers throughout: exact, independent of any order, two calls agree bit for bit, and a ``SparseGroupCounts`` gives the bits
    of the ``GroupCounts`` of the same data.  A code outside [0, n_seg) (n_seg <= 1024) is ranked with the others but counted in no
    sum.  ``genes``: int32 device tensor [n_sel] of gene positions in [0, G), repeats allowed, None = all genes; a selected column
    equals the same column of the all-genes result.  A row outside the matrix is a ValueError raised here, before any launch.
    The genes are walked in slabs of ``rank_gene_slab(n)`` (the cached workspace stays within 8 KiB + max(WS_BUDGET_BYTES, 16 n) bytes);
    a ``SparseGroupCounts`` is densified ``COUNT_CHUNK_ROWS`` listed rows at a time (spv_csr_gather) and staged chunk by chunk, once per
    gene slab."""
    fn = "rank_sums"
    if not isinstance(counts, (GroupCounts, SparseGroupCounts)):
        raise _abi.SpvError(f"{fn}: counts must be a GroupCounts or a SparseGroupCounts, got {type(counts).__name__}")
    dev, G = counts.device, int(counts.G)

    def vec(t, dtype, what, length=None):
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous()
                or (length is not None and t.numel() != length)):
            raise _abi.SpvError(f"{fn}: {what} must be a contiguous 1-d {str(dtype).replace('torch.', '')} tensor on the counts' device"
                                + (f" with one entry per listed row ({length})" if length is not None else ""))

    vec(rows, torch.int32, "rows")
    n = int(rows.numel())
    if not 1 <= n <= RANK_MAX_N:
        raise ValueError(f"{fn}: between 1 and 2^20 listed rows, got {n}")
    vec(seg, torch.int32, "seg", n)
    if isinstance(n_seg, bool) or not isinstance(n_seg, int) or not 1 <= n_seg <= RANK_MAX_SEG:
        raise ValueError(f"{fn}: n_seg must be an integer between 1 and {RANK_MAX_SEG}, got {n_seg!r}")
    if w is not None:
        vec(w, torch.float32, "w", n)
    if genes is not None:
        vec(genes, torch.int32, "genes")
        if genes.numel() < 1:
            raise _abi.SpvError(f"{fn}: genes must not be empty")
    lo, hi = (int(v) for v in torch.aminmax(rows))
    if lo < 0 or hi >= counts.n_cells:
        raise ValueError(f"{fn}: rows must lie in [0, {counts.n_cells}), got values from {lo} to {hi}")
    if genes is not None:
        lo, hi = (int(v) for v in torch.aminmax(genes))
        if lo < 0 or hi >= G:
            raise ValueError(f"{fn}: genes must lie in [0, {G}), got values from {lo} to {hi}")
    n_sel = G if genes is None else int(genes.numel())
    slab = rank_gene_slab(n)
    ws = _workspace(dev, rank_ws_bytes(n, min(slab, n_sel)))
    rank2 = torch.empty((n_seg, n_sel), dtype=torch.int64, device=dev)
    ties = torch.empty((n_sel,), dtype=torch.int64, device=dev)
    sparse = isinstance(counts, SparseGroupCounts)
    if sparse:
        ldx = round_up(G, 8)
        buf = torch.empty((min(n, COUNT_CHUNK_ROWS), ldx), dtype=torch.float32 if counts.dtype == _abi.SPV_COUNT_F32 else torch.int16, device=dev)
        dense = GroupCounts(buf, G, 0)
    a = SpvRankArgs()
    a.G, a.n, a.n_seg, a.seg, a.w = G, n, n_seg, ptr(seg), ptr(w)
    a.ld_rank2, a.ws, a.ws_bytes = n_sel, ptr(ws), ws.numel()
    for j0 in range(0, n_sel, slab):
        m = min(slab, n_sel - j0)
        sel = None if genes is None and j0 == 0 else (genes[j0:j0 + m] if genes is not None else torch.arange(j0, j0 + m, dtype=torch.int32, device=dev))
        a.genes, a.n_sel = ptr(sel), m
        a.rank2, a.ties = rank2.data_ptr() + 8 * j0, ties.data_ptr() + 8 * j0
        if not sparse:
            a.x, a.n_rows, a.n_piece, a.pos_off, a.reset = counts.c_struct(rows), counts.n_cells, n, 0, 1
            _abi.call("spv_rank_stage", C.byref(a), stream_ptr())
        else:
            for p0 in range(0, n, COUNT_CHUNK_ROWS):
                p1 = min(p0 + COUNT_CHUNK_ROWS, n)
                piece = rows[p0:p1]
                g = (SpvCsrGatherArgs * 1)()
                g[0].indptr, g[0].cols, g[0].vals, g[0].n_rows, g[0].G, g[0].dtype = ptr(counts.indptr), ptr(counts.cols), ptr(counts.vals), counts.n_cells, G, counts.dtype
                g[0].B, g[0].rows, g[0].X, g[0].ldx = p1 - p0, ptr(piece), ptr(buf), ldx
                g[0].xb, g[0].ld_xb, g[0].xb_split, g[0].library = None, 0, 0, None
                _abi.call("spv_csr_gather", g, 1, stream_ptr())
                a.x, a.n_rows, a.n_piece, a.pos_off, a.reset = dense.c_struct(None), p1 - p0, p1 - p0, p0, int(p0 == 0)
                _abi.call("spv_rank_stage", C.byref(a), stream_ptr())
        _abi.call("spv_rank_sums", C.byref(a), stream_ptr())
    return rank2, ties
