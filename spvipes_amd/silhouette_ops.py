"""Segmented distance sums on the device: the fused kernel spv_silhouette_sums (csrc/spv_silhouette.h; include/spvipes_hip.h states the
contract).  ``spVIPES.latent_silhouette`` runs it on the latents; nothing of size queries x candidates is ever stored."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi
from ._abi import SIL_SEG_MAX, SpvSilhouetteArgs, ptr, stream_ptr
from ._scan_ops import _WS, _fill_sides, _n_split, _sides, _workspace   # _WS: the benchmarks clear it


def silhouette_splits(n_q: int, n_c: int) -> int:
    """Chunks of the candidates spv_silhouette_sums uses for this shape when ``n_split`` is 0: a pure function of the shapes"""
    return int(_abi.load().spv_silhouette_splits(int(n_q), int(n_c)))


def silhouette_ws_bytes(n_q: int, n_seg: int, n_split: int) -> int:
    """Bytes of workspace for ``n_split`` chunks (the resolved number, not 0): 0 for one chunk"""
    return int(_abi.load().spv_silhouette_ws_bytes(int(n_q), int(n_seg), int(n_split)))


def segment_distance_sums(Q: torch.Tensor, C_: torch.Tensor, seg_ptr: torch.Tensor, n_split: int = 0,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """For every row of ``Q`` and every segment of the rows of ``C_`` the fp64 sum of the Euclidean distances to the segment's rows ->
    fp64 device tensor [n_q, n_seg].  The result is the TRANSPOSED VIEW of a segment-major buffer [n_seg, n_q] (the kernel's layout:
    ``result.t()`` is what is stored), so ``result[:, s]`` is contiguous and ``result[i]`` is strided.
    A distance is the correctly rounded fp32 square root of ``knn``'s squared distance (the same bits), widened to fp64; the additions run
    in ascending row order of ``C_``.  A row of ``Q`` that is also a row of ``C_`` adds exactly +0 for itself.  An empty segment gives 0;
    a non-finite row of ``C_`` makes its segment's column NaN / inf and nothing else.
    ``Q`` [n_q >= 1, D], ``C_`` [n_c >= 0, D]: fp32 device tensors with unit column stride (row strides may exceed D), 1 <= D <= KNN_DMAX.
    ``seg_ptr``: contiguous int32 DEVICE tensor [n_seg + 1], 1 <= n_seg <= SIL_SEG_MAX, ascending from 0 to n_c (segment s is rows
    seg_ptr[s] .. seg_ptr[s + 1] - 1 of ``C_``).  It is not read back for checking: other contents give unspecified sums.
    ``n_split``: chunks of the candidates, 0 = ``silhouette_splits(n_q, n_c)``.  For a fixed value two calls agree bit for bit and a row
    of the result does not depend on the other rows of ``Q``; different values may differ in the last bits of fp64.
    ``out``: an fp64 device tensor [n_seg, >= n_q] with unit column stride (segment-major, as stored); the transposed view of its first
    n_q columns is returned and nothing else is written."""
    dev, n_q, n_c, D = _sides("segment_distance_sums", Q, C_)
    n_split = _n_split("segment_distance_sums", n_split)
    if (not isinstance(seg_ptr, torch.Tensor) or not seg_ptr.is_cuda or seg_ptr.device != dev or seg_ptr.dtype != torch.int32 or seg_ptr.dim() != 1
            or not seg_ptr.is_contiguous()):
        raise _abi.SpvError("segment_distance_sums: seg_ptr must be a contiguous int32 device tensor [n_seg + 1]")
    n_seg = int(seg_ptr.numel()) - 1
    if not 1 <= n_seg <= SIL_SEG_MAX:
        raise ValueError(f"segment_distance_sums: the number of segments must lie in [1, {SIL_SEG_MAX}], got {n_seg}")
    if out is None:
        out = torch.empty((n_seg, n_q), dtype=torch.float64, device=dev)
    elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.float64 or out.dim() != 2
          or out.shape[0] != n_seg or out.shape[1] < n_q or (out.shape[1] > 1 and out.stride(1) != 1) or (n_seg > 1 and out.stride(0) < n_q)):
        raise _abi.SpvError(f"segment_distance_sums: out must be an fp64 device tensor [{n_seg}, >= {n_q}] with unit column stride")
    ws = _workspace(silhouette_ws_bytes(n_q, n_seg, n_split or silhouette_splits(n_q, n_c)), dev)
    a = SpvSilhouetteArgs()
    _fill_sides(a, Q, C_)
    a.seg_ptr, a.n_seg, a.n_split = ptr(seg_ptr), n_seg, n_split
    a.S, a.ld_s, a.ws = ptr(out), (out.stride(0) if n_seg > 1 else max(n_q, int(out.shape[1]))), ptr(ws)
    _abi.call("spv_silhouette_sums", C.byref(a), stream_ptr())
    return out[:, :n_q].t()
