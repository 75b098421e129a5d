"""Rank sums of the observed counts on the device: the segmented column sort spv_rank_stage / spv_rank_sums over listed rows of a
resident count matrix (csrc/spv_rank.h; include/spvipes_hip.h states the contract).  ``spVIPES.rank_genes_groups`` builds its Wilcoxon
table from them; nothing but the integer tables leaves the device.  ``rank_transform`` (spv_rank_values_stage / spv_rank_values,
csrc/spv_rank_values.h) hands every listed cell its rank back on the same sort: the block Spearman's rho is the Gram of."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi
from ._abi import RANK_MAX_N, RANK_MAX_SEG, SpvCsrGatherArgs, SpvRankArgs, SpvRankValuesArgs, ptr, round_up, stream_ptr
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


def _gather_buffer(counts, n: int):
    """None for a ``GroupCounts``; for a ``SparseGroupCounts`` the dense chunk (buffer, pitch, its GroupCounts) spv_csr_gather fills"""
    if not isinstance(counts, SparseGroupCounts):
        return None
    ldx = round_up(counts.G, 8)
    buf = torch.empty((min(n, COUNT_CHUNK_ROWS), ldx), dtype=torch.float32 if counts.dtype == _abi.SPV_COUNT_F32 else torch.int16, device=counts.device)
    return buf, ldx, GroupCounts(buf, counts.G, 0)


def _stage(entry: str, a, counts, rows: torch.Tensor, n: int, gather) -> None:
    """Stage the whole list for the gene slab ``a`` names, through ``entry`` (spv_rank_stage / spv_rank_values_stage): one call for a
    ``GroupCounts``; a ``SparseGroupCounts`` is densified ``COUNT_CHUNK_ROWS`` listed rows at a time and staged chunk by chunk"""
    if gather is None:
        a.x, a.n_rows, a.n_piece, a.pos_off, a.reset = counts.c_struct(rows), counts.n_cells, n, 0, 1
        _abi.call(entry, C.byref(a), stream_ptr())
        return
    buf, ldx, dense = gather
    for p0 in range(0, n, COUNT_CHUNK_ROWS):
        p1 = min(p0 + COUNT_CHUNK_ROWS, n)
        piece = rows[p0:p1]
        g = (SpvCsrGatherArgs * 1)()
        g[0].indptr, g[0].cols, g[0].vals, g[0].n_rows, g[0].G, g[0].dtype = ptr(counts.indptr), ptr(counts.cols), ptr(counts.vals), counts.n_cells, counts.G, counts.dtype
        g[0].B, g[0].rows, g[0].X, g[0].ldx = p1 - p0, ptr(piece), ptr(buf), ldx
        g[0].xb, g[0].ld_xb, g[0].xb_split, g[0].library = None, 0, 0, None
        _abi.call("spv_csr_gather", g, 1, stream_ptr())
        a.x, a.n_rows, a.n_piece, a.pos_off, a.reset = dense.c_struct(None), p1 - p0, p1 - p0, p0, int(p0 == 0)
        _abi.call(entry, C.byref(a), stream_ptr())


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
    gather = _gather_buffer(counts, n)
    a = SpvRankArgs()
    a.G, a.n, a.n_seg, a.seg, a.w = G, n, n_seg, ptr(seg), ptr(w)
    a.ld_rank2, a.ws, a.ws_bytes = n_sel, ptr(ws), ws.numel()
    for j0 in range(0, n_sel, slab):
        m = min(slab, n_sel - j0)
        sel = None if genes is None and j0 == 0 else (genes[j0:j0 + m] if genes is not None else torch.arange(j0, j0 + m, dtype=torch.int32, device=dev))
        a.genes, a.n_sel = ptr(sel), m
        a.rank2, a.ties = rank2.data_ptr() + 8 * j0, ties.data_ptr() + 8 * j0
        _stage("spv_rank_stage", a, counts, rows, n, gather)
        _abi.call("spv_rank_sums", C.byref(a), stream_ptr())
    return rank2, ties


def rank_values_ws_bytes(n: int, n_sel: int) -> int:
    """spv_rank_values_ws_bytes: spv_rank_ws_bytes + 4 n n_sel, rounded up to 8 (0 outside the ranges)"""
    return int(_abi.load().spv_rank_values_ws_bytes(int(n), int(n_sel)))


def rank_values_gene_slab(n: int) -> int:
    """Genes per call of ``rank_transform``: ``rank_gene_slab`` with the transform's 20 bytes per (position, gene) -- the two halves of
    the sort and the fp32 column -- so that the workspace stays within 8 KiB + max(WS_BUDGET_BYTES, 20 n) bytes"""
    return max(1, min(int(_abi.load().spv_rank_gene_slab()), WS_BUDGET_BYTES // (20 * max(int(n), 1))))


def _same_memory(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    """whether the byte ranges the two tensors span meet (strided views are taken by their whole span)"""
    def span(t):
        if t.numel() == 0:
            return 0, 0
        last = sum((d - 1) * st for d, st in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def rank_transform(counts, rows: torch.Tensor, w: Optional[torch.Tensor] = None, genes: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None, ties: bool = False):
    """The exact rank transform of the LISTED cells ``rows`` (int32 device tensor [n], 1 <= n <= 2^20, any order, repeats allowed) of a
    ``GroupCounts`` (uint16 or fp32) or ``SparseGroupCounts``: -> ``out``, an fp32 device tensor [n, n_sel] with
        out[p, j] = 2 * (average rank of key[p] among the n keys of selected gene j) - (n + 1) = L + U - n
    (L = the keys smaller than key[p], U = the smaller or equal ones), or ``(out, ties)`` with ``ties=True``: int64 [n_sel], the sum of
    t^3 - t over the runs of equal keys, ``rank_sums``' table for the same keys.  key[p] = fl32(float(count) * w[p]) as in ``rank_sums``
    (``w``: non-negative fp32 weights [n]).  Every value is an integer in [-(n - 1), n - 1], exact in fp32; a column sums to exactly 0
    and its squares to exactly (n^3 - n - ties[j]) / 3, so the Gram of the block (``gram_ops.gram_accumulate``) is Spearman's table in
    exact integers for n <= 208 063.  Two calls agree bit for bit, and a ``SparseGroupCounts`` gives the bits of the ``GroupCounts``.
    Keys must be non-negative: an fp32 matrix is checked once here (``aminmax``; a negative or NaN minimum is a ValueError), as are
    the rows and the genes -- every refusal comes before any launch.
    ``out``: None (allocated) or an fp32 device tensor [n, n_sel] with unit column stride (the row stride may exceed n_sel; what lies
    between the rows is never touched).  It may BE the matrix itself -- an in-place transform -- only for a dense fp32 ``GroupCounts``
    with ``col_off == 0`` whose G columns are the whole selection (``genes is None``) and ``rows == arange(n_cells)``: a gene slab's
    columns are staged completely before any of them is written, and no other slab reads them.  Any other overlap with the matrix is a
    ValueError.
    The genes are walked in slabs of ``rank_values_gene_slab(n)``; a ``SparseGroupCounts`` is staged ``COUNT_CHUNK_ROWS`` rows at a time."""
    fn = "rank_transform"
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
    values = counts.vals if isinstance(counts, SparseGroupCounts) else counts.X[:, counts.col_off:counts.col_off + G]
    if values.dtype == torch.float32 and values.numel():
        least = float(torch.aminmax(values).min)
        if not least >= 0.0:
            raise ValueError(f"{fn}: keys must be non-negative (their bit patterns order them); the matrix's minimum is {least}")
    if out is None:
        out = torch.empty((n, n_sel), dtype=torch.float32, device=dev)
    else:
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 2
                or tuple(out.shape) != (n, n_sel) or (n_sel > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < n_sel)):
            raise _abi.SpvError(f"{fn}: out must be an fp32 tensor [{n}, {n_sel}] with unit column stride on the counts' device")
        if isinstance(counts, GroupCounts) and _overlaps(out, counts.X):
            in_place = (counts.dtype == _abi.SPV_COUNT_F32 and counts.col_off == 0 and genes is None and n == counts.n_cells
                        and _same_memory(out, counts.X[:, :G]) and bool(torch.equal(rows, torch.arange(n, dtype=torch.int32, device=dev))))
            if not in_place:
                raise ValueError(f"{fn}: out overlaps the matrix; an in-place transform takes a dense fp32 GroupCounts with col_off 0, genes=None, "
                                 f"rows == arange(n_cells) and out = its own [n_cells, G] block")
    ld_out = max(n_sel, out.stride(0))   # (a one-row block may carry any row stride)
    slab = rank_values_gene_slab(n)
    ws = _workspace(dev, rank_values_ws_bytes(n, min(slab, n_sel)))
    tie = torch.empty((n_sel,), dtype=torch.int64, device=dev) if ties else None
    gather = _gather_buffer(counts, n)
    a = SpvRankValuesArgs()
    a.G, a.n, a.w = G, n, ptr(w)
    a.ld_out, a.nonzero, a.ws, a.ws_bytes = ld_out, None, ptr(ws), ws.numel()
    for j0 in range(0, n_sel, slab):
        m = min(slab, n_sel - j0)
        sel = None if genes is None and j0 == 0 else (genes[j0:j0 + m] if genes is not None else torch.arange(j0, j0 + m, dtype=torch.int32, device=dev))
        a.genes, a.n_sel = ptr(sel), m
        a.out, a.ties = out.data_ptr() + 4 * j0, (tie.data_ptr() + 8 * j0 if ties else None)
        _stage("spv_rank_values_stage", a, counts, rows, n, gather)
        _abi.call("spv_rank_values", C.byref(a), stream_ptr())
    return (out, tie) if ties else out
