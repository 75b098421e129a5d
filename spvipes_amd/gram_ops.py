"""The fp64 Gram of an fp32 block on the device: spv_gram_f64 (csrc/spv_gram.h; include/spvipes_hip.h states the contract), the
reduction ``spVIPES.get_feature_correlation_matrix`` adds every decoded minibatch with.  Only the two fp64 tables it accumulates into
ever leave the device."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi
from ._abi import GRAM_MAX_N, SpvGramArgs, ptr, stream_ptr


def gram_slabs(n: int, n_use: int) -> int:
    """Row slabs spv_gram_f64 uses for ``n`` columns and ``n_use`` counted rows (a pure function of the two): with more than one, the
    partial tiles pass through the workspace and a merge launch adds them in slab order"""
    return int(_abi.load().spv_gram_slabs(int(n), int(n_use)))


def gram_workspace(n: int, n_use: int, device) -> torch.Tensor:
    """The scratch ``gram_accumulate`` needs for this shape (fp64, overwritten by every call; empty for one slab)"""
    return torch.empty(int(_abi.load().spv_gram_ws_bytes(int(n), int(n_use))) // 8, dtype=torch.float64, device=device)


def gram_accumulate(x: torch.Tensor, *, rows: Optional[torch.Tensor] = None, sums: torch.Tensor, gram: torch.Tensor,
                    ws: Optional[torch.Tensor] = None) -> None:
    """``sums[j] += sum_r x[r, j]`` and ``gram[i, j] += sum_r x[r, i] * x[r, j]`` over the counted rows r, every x widened to fp64 first
    (the products are exact; the sums run in fp64 MFMA accumulators, rows in ascending order).  ``x``: fp32 device tensor [n_rows, n]
    with unit column stride (the row stride may exceed n), 1 <= n <= 4096.  ``rows``: None (every row counts) or a contiguous int32
    device tensor of strictly ascending row numbers in [0, n_rows) (taken as checked: the kernel clamps them, it does not report
    them); rows that are not listed are never read and may hold NaN.  ``sums``: fp64 device tensor [>= n]; ``gram``: fp64 device
    tensor [n, >= n] with unit column stride, both triangles are written and columns >= n stay untouched.  Both ACCUMULATE: zero them
    once, then one pair collects a whole walk; a ``gram`` that is symmetric in bits stays so.  ``ws``: ``gram_workspace(n, n_use,
    device)`` or larger; one is allocated when None.  No counted row: nothing changes.  Deterministic: two calls agree bit for bit."""
    who = "gram_accumulate"
    if (not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < 1
            or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
        raise _abi.SpvError(f"{who}: x must be an fp32 device tensor [rows, columns >= 1] with unit column stride")
    n_rows, n, dev = int(x.shape[0]), int(x.shape[1]), x.device
    if n > GRAM_MAX_N:
        raise ValueError(f"{who}: at most {GRAM_MAX_N} columns (the table is n x n fp64), got {n}")
    if rows is not None and (not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.device != dev or rows.dtype != torch.int32 or rows.dim() != 1
                             or not rows.is_contiguous()):
        raise _abi.SpvError(f"{who}: rows must be None or a contiguous 1-d int32 tensor on x's device")
    n_use = n_rows if rows is None else int(rows.numel())
    if n_use > n_rows:
        raise ValueError(f"{who}: rows lists {n_use} rows of a block of {n_rows}: row numbers must be strictly ascending")
    if (not isinstance(sums, torch.Tensor) or not sums.is_cuda or sums.device != dev or sums.dtype != torch.float64 or sums.dim() != 1
            or sums.shape[0] < n or (sums.shape[0] > 1 and sums.stride(0) != 1)):
        raise _abi.SpvError(f"{who}: sums must be a contiguous fp64 tensor [>= {n}] on x's device")
    if (not isinstance(gram, torch.Tensor) or not gram.is_cuda or gram.device != dev or gram.dtype != torch.float64 or gram.dim() != 2
            or gram.shape[0] != n or gram.shape[1] < n or (gram.shape[1] > 1 and gram.stride(1) != 1) or (n > 1 and gram.stride(0) < n)):
        raise _abi.SpvError(f"{who}: gram must be an fp64 tensor [{n}, >= {n}] with unit column stride on x's device")
    need = int(_abi.load().spv_gram_ws_bytes(n, n_use))
    if n_use == 0:
        return   # (an empty tensor has no address to hand to the entry point, and an empty ``rows`` must not read as None)
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    elif not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.device != dev or ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() * 8 < need:
        raise _abi.SpvError(f"{who}: ws must be a contiguous fp64 tensor of at least {need // 8} elements on x's device (gram_workspace)")
    a = SpvGramArgs()
    a.x, a.ld_x, a.n_rows = ptr(x), (x.stride(0) if n_rows > 1 else n), n_rows
    a.rows, a.n_use, a.n = (None if rows is None else ptr(rows)), n_use, n
    a.sums, a.gram, a.ld_gram = ptr(sums), ptr(gram), (gram.stride(0) if n > 1 else max(int(gram.shape[1]), n))
    a.ws, a.ws_bytes = (ptr(ws) if ws.numel() else None), ws.numel() * 8
    _abi.call("spv_gram_f64", C.byref(a), stream_ptr())
