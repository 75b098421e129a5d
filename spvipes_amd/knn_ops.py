"""Exact k-nearest neighbours on the device: the fused distance-and-select kernel spv_knn (csrc/spv_knn.h; include/spvipes_hip.h
states the contract).  ``spVIPES.latent_neighbors`` runs it on the latents; nothing of size queries x candidates is ever stored."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _abi
from ._abi import KNN_DMAX, KNN_KMAX, KNN_PAGED_KMAX, KNN_SPLIT_MAX, SpvKnnArgs, ptr, stream_ptr  # the limits: part of this module's interface
from ._scan_ops import _WS, _fill_sides, _k, _n_split, _out_pair, _sides, _workspace   # _WS: the benchmarks clear it


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
    dev, n_q, n_c, D = _sides("knn", Q, C_)
    k, n_split = _k("knn", k), _n_split("knn", n_split)
    if exclude is not None and (not isinstance(exclude, torch.Tensor) or not exclude.is_cuda or exclude.device != dev or exclude.dtype != torch.int32
                                or exclude.dim() != 1 or exclude.numel() != n_q or not exclude.is_contiguous()):
        raise _abi.SpvError(f"knn: exclude must be a contiguous int32 device tensor with one entry per query ({n_q})")
    idx, dist, ld_out = _out_pair("knn", out, "dist", n_q, k, dev)
    ws = _workspace(knn_ws_bytes(n_q, k, n_split or knn_splits(n_q, n_c)), dev)
    a = SpvKnnArgs()
    _fill_sides(a, Q, C_)
    a.k, a.exclude, a.n_split = k, ptr(exclude), n_split
    a.idx, a.dist, a.ld_out, a.ws = ptr(idx), ptr(dist), ld_out, ptr(ws)
    _abi.call("spv_knn", C.byref(a), stream_ptr())
    return idx[:, :k], dist[:, :k]


def knn_paged_ws_bytes(n_q: int, k: int, n_split: int) -> int:
    """Bytes of workspace of ``knn_paged`` for ``n_split`` chunks (the resolved number, not 0): one page's worth, 0 for one chunk"""
    return int(_abi.load().spv_knn_paged_ws_bytes(int(n_q), int(k), int(n_split)))


def knn_paged(Q: torch.Tensor, C_: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None, n_split: int = 0,
              out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``knn`` for 1 <= k <= KNN_PAGED_KMAX (256), spv_knn_paged: columns [64 p, 64 p + 64) are one more run of ``knn``'s kernels over the
    candidates that come after the previous page's last (dist, idx) key.  Every convention is ``knn``'s -- the arguments, ``out``, the
    squared fp32 distance chain, the order (dist, idx), the fill -1 / +inf, the same bits for every ``n_split`` -- and the first
    min(k, 64) columns are what ``knn`` returns for that k, bit for bit."""
    dev, n_q, n_c, D = _sides("knn_paged", Q, C_)
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_PAGED_KMAX:
        raise ValueError(f"knn_paged: k must be an integer in [1, {KNN_PAGED_KMAX}], got {k!r}")
    k, n_split = int(k), _n_split("knn_paged", n_split)
    if exclude is not None and (not isinstance(exclude, torch.Tensor) or not exclude.is_cuda or exclude.device != dev or exclude.dtype != torch.int32
                                or exclude.dim() != 1 or exclude.numel() != n_q or not exclude.is_contiguous()):
        raise _abi.SpvError(f"knn_paged: exclude must be a contiguous int32 device tensor with one entry per query ({n_q})")
    idx, dist, ld_out = _out_pair("knn_paged", out, "dist", n_q, k, dev)
    ws = _workspace(knn_paged_ws_bytes(n_q, k, n_split or knn_splits(n_q, n_c)), dev)
    a = SpvKnnArgs()
    _fill_sides(a, Q, C_)
    a.k, a.exclude, a.n_split = k, ptr(exclude), n_split
    a.idx, a.dist, a.ld_out, a.ws = ptr(idx), ptr(dist), ld_out, ptr(ws)
    _abi.call("spv_knn_paged", C.byref(a), stream_ptr())
    return idx[:, :k], dist[:, :k]
