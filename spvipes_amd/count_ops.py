"""Statistics of the observed counts on the device: the segmented column reduction spv_count_stats over listed rows of a resident
count matrix and the per-cell totals spv_count_totals / spv_csr_totals (csrc/spv_count_stats.h; include/spvipes_hip.h states the
contract).  ``spVIPES.count_statistics`` builds its table from them; nothing but the per-segment sums leaves the device."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _abi
from ._abi import SpvCountStatsArgs, SpvCsrGatherArgs, ptr, round_up, stream_ptr
from .data import count_slab_plan
from .ops import GroupCounts, SparseGroupCounts

COUNT_STATS = ("sum", "non_zeros", "weighted_sum")   # the rows of spv_count_stats' output
COUNT_CHUNK_ROWS = 4096   # a CSR matrix is densified this many listed rows at a time (whole slabs): the minibatch buffers' order of size


def count_stats_tile() -> int:
    """Genes per workgroup of the partial pass (T)"""
    return int(_abi.load().spv_count_stats_tile())


def count_stats_slab() -> int:
    """List positions per slab (S): ``count_stats`` plans its slabs with it"""
    return int(_abi.load().spv_count_stats_slab())


def count_stats_workspace(n_genes: int, seg_sizes, device) -> torch.Tensor:
    """The scratch ``count_stats`` needs for these segment sizes (fp64, overwritten by every call): one record of 3 x n_genes per slab"""
    n_slabs = count_slab_plan(seg_sizes, count_stats_slab())[0].shape[0]
    return torch.empty(max(n_slabs, 1) * len(COUNT_STATS) * int(n_genes), dtype=torch.float64, device=device)


def _counts(counts, fn: str) -> None:
    if not isinstance(counts, (GroupCounts, SparseGroupCounts)):
        raise _abi.SpvError(f"{fn}: counts must be a GroupCounts or a SparseGroupCounts, got {type(counts).__name__}")


def count_totals(counts) -> torch.Tensor:
    """total[c] = the sum over ALL of the group's genes of cell c's counts -> fp64 device vector [n_cells].  Exact for uint16 counts;
    fp32 counts are added in fp64 in one fixed order for both storages, so a ``GroupCounts`` and the ``SparseGroupCounts`` of the same
    data agree bit for bit.  Computed once per resident matrix and kept on the counts object (as ``log1p_image`` is)."""
    _counts(counts, "count_totals")
    t = getattr(counts, "_totals", None)
    if t is None:
        if counts.n_cells < 1:
            raise ValueError("count_totals: the matrix has no cells")
        t = torch.empty((counts.n_cells,), dtype=torch.float64, device=counts.device)
        if isinstance(counts, GroupCounts):
            cs = counts.c_struct(None)
            _abi.call("spv_count_totals", C.byref(cs), counts.n_cells, counts.G, ptr(t), stream_ptr())
        else:
            _abi.call("spv_csr_totals", ptr(counts.indptr), ptr(counts.cols), ptr(counts.vals), counts.dtype, counts.n_cells, counts.G, ptr(t),
                      stream_ptr())
        counts._totals = t
    return t


def _chunks(slabs: np.ndarray, limit: int):
    """consecutive slabs grouped into chunks of at most ``limit`` list positions (a longer slab is a chunk of its own): [(first, count)]"""
    out, first, rows = [], 0, 0
    for i in range(slabs.shape[0]):
        n = int(slabs[i, 1] - slabs[i, 0])
        if i > first and rows + n > limit:
            out.append((first, i - first))
            first, rows = i, 0
        rows += n
    out.append((first, slabs.shape[0] - first))
    return out


def count_square_sums(counts, rows: torch.Tensor, seg_sizes, genes: Optional[torch.Tensor] = None, row_totals: bool = False):
    """Per segment and selected gene the sum of the SQUARED observed counts over listed cells -> device tensor [n_seg, n_sel]: int64
    for uint16 counts (exact: 65535^2 * 2^31 < 2^63), fp64 for fp32 counts (squared and added in fp64, segment by segment in list
    order).  ``rows`` / ``seg_sizes`` / ``genes``: as ``count_stats`` takes them (rows sorted by segment; checked the same way).
    The second moment next to ``count_stats``' sum and non-zero tally: posterior_predictive_check's observed variance.  Not a
    kernel of its own: ONE chunked torch reduction, ``COUNT_CHUNK_ROWS`` listed rows at a time -- a gather of the chunk's rows (a
    CSR matrix is densified by spv_csr_gather first), a widening copy and a square, i.e. two temporaries of 8 bytes x chunk rows x
    n_sel, and one read of every listed row.  A fourth row of spv_count_stats is the later home of this statistic.
    ``row_totals``: also return each listed cell's total over the SELECTED genes (a repeated gene counts as often as it is listed),
    fp64 [n] aligned with ``rows``, from the same pass -> (sums, totals)."""
    fn = "count_square_sums"
    _counts(counts, fn)
    dev, G = counts.device, int(counts.G)
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous() or rows.device != dev:
        raise _abi.SpvError(f"{fn}: rows must be a contiguous 1-d int32 tensor on the counts' device")
    sizes = [int(s) for s in np.asarray(seg_sizes).ravel().tolist()]
    n, n_seg = int(rows.numel()), len(sizes)
    if n_seg < 1 or any(s < 0 for s in sizes) or sum(sizes) != n:
        raise ValueError(f"{fn}: seg_sizes must be non-negative and add up to the number of listed rows ({n}), got {sizes!r}")
    if genes is not None and (not isinstance(genes, torch.Tensor) or not genes.is_cuda or genes.device != dev or genes.dtype != torch.int32
                              or genes.dim() != 1 or genes.numel() < 1 or not genes.is_contiguous()):
        raise _abi.SpvError(f"{fn}: genes must be a non-empty contiguous 1-d int32 device tensor")
    if n:
        lo, hi = (int(v) for v in torch.aminmax(rows))
        if lo < 0 or hi >= counts.n_cells:
            raise ValueError(f"{fn}: rows must lie in [0, {counts.n_cells}), got values from {lo} to {hi}")
    if genes is not None:
        lo, hi = (int(v) for v in torch.aminmax(genes))
        if lo < 0 or hi >= G:
            raise ValueError(f"{fn}: genes must lie in [0, {G}), got values from {lo} to {hi}")
    n_sel = G if genes is None else int(genes.numel())
    is_f32 = counts.dtype == _abi.SPV_COUNT_F32
    out = torch.zeros((n_seg, n_sel), dtype=torch.float64 if is_f32 else torch.int64, device=dev)
    totals = torch.zeros((n,), dtype=torch.float64, device=dev) if row_totals else None
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sparse = isinstance(counts, SparseGroupCounts)
    if sparse and n:
        ldx = round_up(G, 8)
        buf = torch.empty((min(n, COUNT_CHUNK_ROWS), ldx), dtype=torch.float32 if is_f32 else torch.int16, device=dev)
    for p0 in range(0, n, COUNT_CHUNK_ROWS):
        p1 = min(p0 + COUNT_CHUNK_ROWS, n)
        piece = rows[p0:p1]
        if sparse:
            g = (SpvCsrGatherArgs * 1)()
            g[0].indptr, g[0].cols, g[0].vals, g[0].n_rows, g[0].G, g[0].dtype = ptr(counts.indptr), ptr(counts.cols), ptr(counts.vals), counts.n_cells, G, counts.dtype
            g[0].B, g[0].rows, g[0].X, g[0].ldx = p1 - p0, ptr(piece), ptr(buf), ldx
            g[0].xb, g[0].ld_xb, g[0].xb_split, g[0].library = None, 0, 0, None
            _abi.call("spv_csr_gather", g, 1, stream_ptr())
            x = buf[:p1 - p0, :G]
        else:
            x = counts.X.index_select(0, piece.long())[:, counts.col_off:counts.col_off + G]
        if genes is not None:
            x = x.index_select(1, genes.long())
        if is_f32:
            x = x.to(torch.float64)
        else:   # uint16 bit patterns, whichever 16-bit integer dtype stores them
            x = (x.view(torch.int16) if x.dtype != torch.int16 else x).to(torch.int64) & 0xFFFF
        if row_totals:
            totals[p0:p1] = x.sum(1).to(torch.float64)
        x = x * x
        for k in range(n_seg):   # the segments this chunk touches
            a, b = max(int(bounds[k]), p0), min(int(bounds[k + 1]), p1)
            if a < b:
                out[k] += x[a - p0:b - p0].sum(0)
    return (out, totals) if row_totals else out


def count_stats(counts, rows: torch.Tensor, seg_sizes, w: Optional[torch.Tensor] = None, genes: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per segment and selected gene the statistics of the observed counts over LISTED cells -> fp64 device tensor [n_seg, 3, n_sel]
    (a view of ``out``, or a new one): row 0 the sum of the counts, row 1 the number of listed cells with a non-zero count, row 2 the
    sum of fl64(count * w).  ``counts``: a ``GroupCounts`` or a ``SparseGroupCounts``.  ``rows``: int32 device tensor [n] of cells,
    any order, repeats allowed; its first ``seg_sizes[0]`` entries are segment 0, and so on (zeros allowed: an empty segment yields
    zeros).  A row outside the matrix is a ValueError raised here, before any launch (one min / max read-back).  ``w``: fp64 device
    tensor [n], one weight per LISTED cell (aligned with ``rows``, not with the matrix), None = 1.  ``genes``: int32 device tensor
    [n_sel] of gene positions in [0, G), repeats allowed, None = all genes; a selected column equals the same column of the
    all-genes result bit for bit.  ``ws``: ``count_stats_workspace(G, seg_sizes, device)`` or larger; ``out``: fp64 [n_seg, 3, >= n_sel]
    contiguous, columns >= n_sel are left alone.  A ``SparseGroupCounts`` is densified ``COUNT_CHUNK_ROWS`` listed rows at a time in
    whole slabs (spv_csr_gather) and reduced chunk by chunk, then merged once: bit-identical to the dense route on the same data.
    Deterministic: two calls agree bit for bit."""
    fn = "count_stats"
    _counts(counts, fn)
    dev, G = counts.device, int(counts.G)
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous() or rows.device != dev:
        raise _abi.SpvError(f"{fn}: rows must be a contiguous 1-d int32 tensor on the counts' device")
    sizes = [int(s) for s in np.asarray(seg_sizes).ravel().tolist()]
    n, n_seg = int(rows.numel()), len(sizes)
    if n_seg < 1 or any(s < 0 for s in sizes) or sum(sizes) != n:
        raise ValueError(f"{fn}: seg_sizes must be non-negative and add up to the number of listed rows ({n}), got {sizes!r}")
    if n_seg > 65535:
        raise ValueError(f"{fn}: at most 65535 segments, got {n_seg}")
    if w is not None and (not isinstance(w, torch.Tensor) or not w.is_cuda or w.device != dev or w.dtype != torch.float64 or w.dim() != 1
                          or w.numel() != n or not w.is_contiguous()):
        raise _abi.SpvError(f"{fn}: w must be a contiguous fp64 device tensor with one weight per listed row ({n})")
    if genes is not None and (not isinstance(genes, torch.Tensor) or not genes.is_cuda or genes.device != dev or genes.dtype != torch.int32
                              or genes.dim() != 1 or genes.numel() < 1 or not genes.is_contiguous()):
        raise _abi.SpvError(f"{fn}: genes must be a non-empty contiguous 1-d int32 device tensor")
    n_sel = G if genes is None else int(genes.numel())
    if n:
        lo, hi = (int(v) for v in torch.aminmax(rows))
        if lo < 0 or hi >= counts.n_cells:
            raise ValueError(f"{fn}: rows must lie in [0, {counts.n_cells}), got values from {lo} to {hi}")
    if genes is not None:
        lo, hi = (int(v) for v in torch.aminmax(genes))
        if lo < 0 or hi >= G:
            raise ValueError(f"{fn}: genes must lie in [0, {G}), got values from {lo} to {hi}")
    if out is None:
        out = torch.empty((n_seg, len(COUNT_STATS), n_sel), dtype=torch.float64, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float64 or out.dim() != 3
          or out.shape[0] != n_seg or out.shape[1] != len(COUNT_STATS) or out.shape[2] < n_sel or not out.is_contiguous()):
        raise _abi.SpvError(f"{fn}: out must be a contiguous fp64 device tensor [{n_seg}, 3, >= {n_sel}]")
    res = out[:, :, :n_sel]
    slabs, seg_slabs = count_slab_plan(sizes, count_stats_slab())
    n_slabs = int(slabs.shape[0])
    if n_slabs == 0:   # nothing is listed: every segment is empty
        res.zero_()
        return res
    need = n_slabs * len(COUNT_STATS) * G
    if ws is None:
        ws = torch.empty(need, dtype=torch.float64, device=dev)
    elif not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.device != dev or ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() < need:
        raise _abi.SpvError(f"{fn}: ws must be a contiguous fp64 device tensor of at least {need} elements (count_stats_workspace)")
    slabs_d, seg_d = torch.from_numpy(slabs).to(dev), torch.from_numpy(seg_slabs).to(dev)
    a = SpvCountStatsArgs()
    a.G, a.n, a.pos_off, a.w, a.genes, a.n_sel = G, n, 0, ptr(w), ptr(genes), n_sel
    a.slabs, a.seg_slabs, a.n_slabs, a.n_seg, a.slab_first, a.slab_count = ptr(slabs_d), ptr(seg_d), n_slabs, n_seg, 0, n_slabs
    a.out, a.ld_out, a.ws, a.ws_bytes = ptr(out), out.stride(1), ptr(ws), ws.numel() * 8
    if isinstance(counts, GroupCounts):
        a.x, a.n_rows = counts.c_struct(rows), counts.n_cells
        _abi.call("spv_count_stats", C.byref(a), stream_ptr())
        return res
    # CSR: densify whole slabs of listed rows into one buffer, reduce them at their slab offset, merge once
    chunks = _chunks(slabs, COUNT_CHUNK_ROWS)
    most = max(int(slabs[f + c - 1, 1] - slabs[f, 0]) for f, c in chunks)
    ldx = round_up(G, 8)
    buf = torch.empty((most, ldx), dtype=torch.float32 if counts.dtype == _abi.SPV_COUNT_F32 else torch.int16, device=dev)
    dense = GroupCounts(buf, G, 0)
    for first, cnt in chunks:
        p0, p1 = int(slabs[first, 0]), int(slabs[first + cnt - 1, 1])
        piece = rows[p0:p1]
        g = (SpvCsrGatherArgs * 1)()
        g[0].indptr, g[0].cols, g[0].vals, g[0].n_rows, g[0].G, g[0].dtype = ptr(counts.indptr), ptr(counts.cols), ptr(counts.vals), counts.n_cells, G, counts.dtype
        g[0].B, g[0].rows, g[0].X, g[0].ldx = p1 - p0, ptr(piece), ptr(buf), ldx
        g[0].xb, g[0].ld_xb, g[0].xb_split, g[0].library = None, 0, 0, None
        _abi.call("spv_csr_gather", g, 1, stream_ptr())
        a.x, a.n_rows, a.n, a.pos_off, a.slab_first, a.slab_count = dense.c_struct(None), p1 - p0, p1 - p0, p0, first, cnt
        _abi.call("spv_count_stats_partial", C.byref(a), stream_ptr())
    _abi.call("spv_count_stats_merge", C.byref(a), stream_ptr())
    return res
