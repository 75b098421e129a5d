"""Differential expression on the device: the pair-compare-reduce kernel spv_de_pairs over two fp32 sample banks
(csrc/spv_de.h; include/spvipes_hip.h states the contract) and the exact median of the same pairs, spv_de_median
(csrc/spv_de_median.h).  The banks are what ``spVIPES.differential_expression`` fills with ``module.expected_expression``; nothing
but the per-gene statistics leaves the device."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _abi
from ._abi import SpvDeMedianArgs, SpvDePairsArgs, ptr, stream_ptr

DE_STATS = ("lfc_mean", "lfc_std", "lfc_min", "lfc_max", "count_de", "scale1", "scale2")   # the rows of spv_de_pairs' stats array
DE_MAX_PAIRS = 1 << 24   # the exceedance count is carried as fp32 whole numbers


def de_splits(n_genes: int, n_pairs: int) -> int:
    """Pair splits spv_de_pairs uses for this shape: a lane sums at most ceil(ceil(n_pairs / splits) / 4) terms in fp32; the rest is fp64"""
    return int(_abi.load().spv_de_pairs_splits(int(n_genes), int(n_pairs)))


def de_workspace(n_genes: int, n_pairs: int, device) -> torch.Tensor:
    """The scratch ``de_pairs`` needs for this shape (fp64, overwritten by every call)"""
    return torch.empty(de_splits(n_genes, n_pairs) * len(DE_STATS) * int(n_genes), dtype=torch.float64, device=device)


def _bank(t, name: str, fn: str = "de_pairs") -> None:
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1
            or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise _abi.SpvError(f"{fn}: {name} must be a non-empty fp32 device tensor [rows, genes] with unit column stride")


def _rows(t, name: str, fn: str = "de_pairs") -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
        raise _abi.SpvError(f"{fn}: {name} must be a contiguous 1-d int32 device tensor")


def de_pairs(bank1: torch.Tensor, bank2: torch.Tensor, rows1: torch.Tensor, rows2: torch.Tensor, *, delta: float, eps: float = 0.0,
             ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Per gene the statistics of lfc = log2(max(x1 + eps, FLT_MIN)) - log2(max(x2 + eps, FLT_MIN)) over the pairs
    (bank1[rows1[m]], bank2[rows2[m]]): {"lfc_mean", "lfc_std" (population form), "lfc_min", "lfc_max", "count_de" (the number of
    pairs with |lfc| >= delta, a whole number), "scale1", "scale2" (the means of x1 and x2)} -> fp32 device vectors [n_genes], views
    of one [7, n_genes] array (``out``, or a new one).  ``bank1`` / ``bank2``: fp32 device tensors [rows, n_genes] with unit column
    stride (row strides may exceed n_genes); ``rows1`` / ``rows2``: int32 device tensors [n_pairs], 1 <= n_pairs <= 2^24 (row
    numbers outside a bank are clamped into it by the kernel).  ``ws``: ``de_workspace(n_genes, n_pairs, device)`` or larger; one is
    allocated when None.  Deterministic: two calls agree bit for bit."""
    _bank(bank1, "bank1"), _bank(bank2, "bank2"), _rows(rows1, "rows1"), _rows(rows2, "rows2")
    n_genes, n_pairs, dev = int(bank1.shape[1]), int(rows1.numel()), bank1.device
    if bank2.shape[1] != n_genes or bank2.device != dev or rows1.device != dev or rows2.device != dev:
        raise _abi.SpvError("de_pairs: the two banks must have the same number of genes, and banks and row arrays must share a device")
    if rows2.numel() != n_pairs or not 1 <= n_pairs <= DE_MAX_PAIRS:
        raise ValueError(f"de_pairs: rows1 and rows2 must hold the same number of pairs, between 1 and 2^24 (got {n_pairs} and {int(rows2.numel())})")
    if not (float(delta) >= 0.0 and float(eps) >= 0.0):
        raise ValueError(f"de_pairs: delta and eps must be non-negative numbers, got {delta!r} and {eps!r}")
    need = de_splits(n_genes, n_pairs) * len(DE_STATS) * n_genes
    if ws is None:
        ws = torch.empty(need, dtype=torch.float64, device=dev)
    elif not ws.is_cuda or ws.device != dev or ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() < need:
        raise _abi.SpvError(f"de_pairs: ws must be a contiguous fp64 device tensor of at least {need} elements (de_workspace)")
    if out is None:
        out = torch.empty((len(DE_STATS), n_genes), dtype=torch.float32, device=dev)
    elif (not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != len(DE_STATS)
          or out.shape[1] < n_genes or (out.shape[1] > 1 and out.stride(1) != 1) or out.stride(0) < n_genes):
        raise _abi.SpvError(f"de_pairs: out must be an fp32 device tensor [7, >= {n_genes}] with unit column stride")
    a = SpvDePairsArgs()
    a.bank1, a.bank2 = ptr(bank1), ptr(bank2)
    a.ld1, a.ld2 = (bank1.stride(0) if bank1.shape[0] > 1 else n_genes), (bank2.stride(0) if bank2.shape[0] > 1 else n_genes)
    a.rows1, a.rows2, a.n_rows1, a.n_rows2 = ptr(rows1), ptr(rows2), int(bank1.shape[0]), int(bank2.shape[0])
    a.n_genes, a.n_pairs, a.delta, a.eps = n_genes, n_pairs, float(delta), float(eps)
    a.stats, a.ld_stats, a.ws, a.ws_bytes = ptr(out), out.stride(0), ptr(ws), ws.numel() * 8
    _abi.call("spv_de_pairs", C.byref(a), stream_ptr())
    return {k: out[i, :n_genes] for i, k in enumerate(DE_STATS)}


DE_MEDIAN_ROWS = ("mid_lo", "mid_hi")   # the rows of spv_de_median's output array


def de_median_workspace(n_genes: int, n_pairs: int, device) -> torch.Tensor:
    """The scratch ``de_median`` needs for this shape (bytes, overwritten by every call); it grows with n_genes only"""
    return torch.empty(int(_abi.load().spv_de_median_ws_bytes(int(n_genes), int(n_pairs))), dtype=torch.uint8, device=device)


def de_median(bank1: torch.Tensor, bank2: torch.Tensor, rows1: torch.Tensor, rows2: torch.Tensor, *, eps: float = 0.0,
              ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Per gene the two middle order statistics of the lfc ``de_pairs`` reduces, over the same pairs: {"mid_lo" (rank
    (n_pairs - 1) // 2 of the ascending values), "mid_hi" (rank n_pairs // 2)} -> fp32 device vectors [n_genes], views of one
    [2, n_genes] array (``out``, or a new one); the median is their mean.  Exact: both are elements of the gene's fp32 lfc values
    (``lfc_min <= mid_lo <= mid_hi <= lfc_max``), found by a radix select that stores nothing of size n_pairs x n_genes.  Banks and
    row arrays as for ``de_pairs``.  ``ws``: ``de_median_workspace(n_genes, n_pairs, device)`` or larger; one is allocated when
    None.  Deterministic: two calls agree bit for bit."""
    fn = "de_median"
    _bank(bank1, "bank1", fn), _bank(bank2, "bank2", fn), _rows(rows1, "rows1", fn), _rows(rows2, "rows2", fn)
    n_genes, n_pairs, dev = int(bank1.shape[1]), int(rows1.numel()), bank1.device
    if bank2.shape[1] != n_genes or bank2.device != dev or rows1.device != dev or rows2.device != dev:
        raise _abi.SpvError("de_median: the two banks must have the same number of genes, and banks and row arrays must share a device")
    if rows2.numel() != n_pairs or not 1 <= n_pairs <= DE_MAX_PAIRS:
        raise ValueError(f"de_median: rows1 and rows2 must hold the same number of pairs, between 1 and 2^24 (got {n_pairs} and {int(rows2.numel())})")
    if not float(eps) >= 0.0:
        raise ValueError(f"de_median: eps must be a non-negative number, got {eps!r}")
    need = int(_abi.load().spv_de_median_ws_bytes(n_genes, n_pairs))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.device != dev or not ws.is_contiguous() or ws.numel() * ws.element_size() < need
          or ws.data_ptr() % 4):
        raise _abi.SpvError(f"de_median: ws must be a contiguous, 4-byte aligned device tensor of at least {need} bytes (de_median_workspace)")
    if out is None:
        out = torch.empty((2, n_genes), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != 2
          or out.shape[1] < n_genes or (out.shape[1] > 1 and out.stride(1) != 1) or out.stride(0) < n_genes):
        raise _abi.SpvError(f"de_median: out must be an fp32 device tensor [2, >= {n_genes}] with unit column stride")
    a = SpvDeMedianArgs()
    a.bank1, a.bank2 = ptr(bank1), ptr(bank2)
    a.ld1, a.ld2 = (bank1.stride(0) if bank1.shape[0] > 1 else n_genes), (bank2.stride(0) if bank2.shape[0] > 1 else n_genes)
    a.rows1, a.rows2, a.n_rows1, a.n_rows2 = ptr(rows1), ptr(rows2), int(bank1.shape[0]), int(bank2.shape[0])
    a.n_genes, a.n_pairs, a.eps = n_genes, n_pairs, float(eps)
    a.mid, a.ld_mid, a.ws, a.ws_bytes = ptr(out), out.stride(0), ptr(ws), ws.numel() * ws.element_size()
    _abi.call("spv_de_median", C.byref(a), stream_ptr())
    return {k: out[i, :n_genes] for i, k in enumerate(DE_MEDIAN_ROWS)}
