"""Exact k-nearest neighbours on the device: the fused distance-and-select kernel spv_knn (csrc/spv_knn.h; include/spvipes_hip.h
states the contract).  ``spVIPES.latent_neighbors`` runs it on the latents; nothing of size queries x candidates is ever stored."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from . import _abi
from ._abi import KNN_DMAX, KNN_KMAX, KNN_SPLIT_MAX, SpvKnnArgs, ptr, stream_ptr

_WS: Dict[tuple, torch.Tensor] = {}   # (device, bytes) -> the workspace of that size; a few shapes per process
_WS_KEEP = 4


def knn_tiles() -> Tuple[int, int]:
    """(queries per workgroup, candidates per LDS tile) of the partial pass"""
    lib = _abi.load()
    return int(lib.spv_knn_tile_q()), int(lib.spv_knn_tile_c())


def knn_splits(n_q: int, n_c: int) -> int:
    """Chunks of the candidates spv_knn uses for this shape when ``n_split`` is 0: a pure function of the shapes"""
    return int(_abi.load().spv_knn_splits(int(n_q), int(n_c)))


def knn_ws_bytes(n_q: int, k: int, n_split: int) -> int:
    """Bytes of workspace for ``n_split`` chunks (the resolved number, not 0): 0 for one chunk"""
    return int(_abi.load().spv_knn_ws_bytes(int(n_q), int(k), int(n_split)))


def _workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    if nbytes == 0:
        return None
    key = (str(device), nbytes)
    ws = _WS.get(key)
    if ws is None:
        while len(_WS) >= _WS_KEEP:
            _WS.pop(next(iter(_WS)))
        ws = _WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _rows(t, name: str) -> None:
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 1
            or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise _abi.SpvError(f"knn: {name} must be an fp32 device tensor [rows, D] with unit column stride")


def knn(Q: torch.Tensor, C_: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None, n_split: int = 0,
        out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """For every row of ``Q`` the ``k`` rows of ``C_`` nearest to it -> (idx int32 [n_q, k], dist fp32 [n_q, k]), ascending in
    (dist, idx): ``dist`` is the SQUARED Euclidean distance as one fixed fp32 chain per pair, equal distances go to the smaller
    index, rows with fewer than k finite-distance candidates end in idx = -1 / dist = +inf.  ``Q`` [n_q >= 1, D], ``C_`` [n_c >= 0, D]:
    fp32 device tensors with unit column stride (row strides may exceed D), 1 <= D <= KNN_DMAX; 1 <= k <= KNN_KMAX.  ``exclude``:
    contiguous int32 device tensor [n_q], candidate exclude[i] is skipped for query i (a value outside [0, n_c) skips nothing).
    ``n_split``: chunks of the candidates, 0 = ``knn_splits(n_q, n_c)``; the result is the same bit for bit for every value.
    ``out``: (idx, dist) tensors [n_q, >= k] with one common row stride and unit column stride; views of their first k columns are
    returned and nothing else is written.  Deterministic: two calls agree bit for bit."""
    _rows(Q, "Q"), _rows(C_, "C")
    dev, n_q, n_c, D = Q.device, int(Q.shape[0]), int(C_.shape[0]), int(Q.shape[1])
    if C_.device != dev or int(C_.shape[1]) != D:
        raise _abi.SpvError("knn: Q and C must share a device and have the same number of columns")
    if n_q < 1:
        raise ValueError("knn: Q has no rows")
    if not 1 <= D <= KNN_DMAX:
        raise ValueError(f"knn: D must lie in [1, {KNN_DMAX}], got {D}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_KMAX:
        raise ValueError(f"knn: k must be an integer in [1, {KNN_KMAX}], got {k!r}")
    k = int(k)
    if isinstance(n_split, bool) or int(n_split) != n_split or not 0 <= int(n_split) <= KNN_SPLIT_MAX:
        raise ValueError(f"knn: n_split must be 0 or an integer in [1, {KNN_SPLIT_MAX}], got {n_split!r}")
    if exclude is not None and (not isinstance(exclude, torch.Tensor) or not exclude.is_cuda or exclude.device != dev or exclude.dtype != torch.int32
                                or exclude.dim() != 1 or exclude.numel() != n_q or not exclude.is_contiguous()):
        raise _abi.SpvError(f"knn: exclude must be a contiguous int32 device tensor with one entry per query ({n_q})")
    if out is None:
        idx = torch.empty((n_q, k), dtype=torch.int32, device=dev)
        dist = torch.empty((n_q, k), dtype=torch.float32, device=dev)
    else:
        idx, dist = out
        for t, dt, name in ((idx, torch.int32, "idx"), (dist, torch.float32, "dist")):
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dt or t.dim() != 2 or t.shape[0] != n_q
                    or t.shape[1] < k or (t.shape[1] > 1 and t.stride(1) != 1) or (n_q > 1 and t.stride(0) < k)):
                raise _abi.SpvError(f"knn: out {name} must be a device tensor [{n_q}, >= {k}] of {dt} with unit column stride")
        if n_q > 1 and idx.stride(0) != dist.stride(0):
            raise _abi.SpvError("knn: out idx and dist must have the same row stride")
    splits = int(n_split) or knn_splits(n_q, n_c)
    ws = _workspace(knn_ws_bytes(n_q, k, splits), dev)
    a = SpvKnnArgs()
    a.Q, a.ld_q, a.n_q = ptr(Q), (Q.stride(0) if n_q > 1 else D), n_q
    a.C, a.ld_c, a.n_c = (ptr(C_) if n_c else ptr(Q)), (C_.stride(0) if n_c > 1 else D), n_c   # an empty tensor has no address; nothing is read
    a.D, a.k, a.exclude, a.n_split = D, k, ptr(exclude), int(n_split)
    a.idx, a.dist, a.ld_out, a.ws = ptr(idx), ptr(dist), (idx.stride(0) if n_q > 1 else max(k, int(idx.shape[1]))), ptr(ws)
    _abi.call("spv_knn", C.byref(a), stream_ptr())
    return idx[:, :k], dist[:, :k]
