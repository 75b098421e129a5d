"""What the wrappers of the pair-scan kernels share (knn_ops, ot_ops, silhouette_ops; csrc/spv_pair_scan.h): the workspace cache, the
checks of the two row matrices, of ``n_split``, ``k`` and an (idx, values) output pair, and the argument fields of the two sides.  ``op``
is the name a message starts with."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _abi
from ._abi import KNN_DMAX, KNN_KMAX, KNN_SPLIT_MAX, ptr

_WS: Dict[tuple, torch.Tensor] = {}   # (device, bytes) -> the workspace of that size; a few shapes per process
_WS_KEEP = 4


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


def _rows(op: str, t, name: str) -> None:
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < 1
            or (t.shape[0] > 0 and t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):   # no rows: no strides to speak of
        raise _abi.SpvError(f"{op}: {name} must be an fp32 device tensor [rows, D] with unit column stride")


def _sides(op: str, Q, C_, names: Tuple[str, str] = ("Q", "C")) -> Tuple[torch.device, int, int, int]:
    """the checks of the queries ``Q`` [n_q >= 1, D] and the candidates ``C_`` [n_c >= 0, D] -> (device, n_q, n_c, D)"""
    _rows(op, Q, names[0]), _rows(op, C_, names[1])
    dev, n_q, n_c, D = Q.device, int(Q.shape[0]), int(C_.shape[0]), int(Q.shape[1])
    if C_.device != dev or int(C_.shape[1]) != D:
        raise _abi.SpvError(f"{op}: {names[0]} and {names[1]} must share a device and have the same number of columns")
    if n_q < 1:
        raise ValueError(f"{op}: {names[0]} has no rows")
    if not 1 <= D <= KNN_DMAX:
        raise ValueError(f"{op}: D must lie in [1, {KNN_DMAX}], got {D}")
    return dev, n_q, n_c, D


def _n_split(op: str, n_split) -> int:
    if isinstance(n_split, bool) or int(n_split) != n_split or not 0 <= int(n_split) <= KNN_SPLIT_MAX:
        raise ValueError(f"{op}: n_split must be 0 or an integer in [1, {KNN_SPLIT_MAX}], got {n_split!r}")
    return int(n_split)


def _k(op: str, k) -> int:
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= KNN_KMAX:
        raise ValueError(f"{op}: k must be an integer in [1, {KNN_KMAX}], got {k!r}")
    return int(k)


def _out_pair(op: str, pair, name: str, n_q: int, k: int, dev) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """``pair`` = (idx int32, ``name`` fp32) [n_q, >= k] with one common row stride and unit column stride, or None: new tensors
    -> (idx, values, the row stride the kernel is given)"""
    if pair is None:
        idx = torch.empty((n_q, k), dtype=torch.int32, device=dev)
        values = torch.empty((n_q, k), dtype=torch.float32, device=dev)
    else:
        idx, values = pair
        for t, dt, nm in ((idx, torch.int32, "idx"), (values, torch.float32, name)):
            if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dt or t.dim() != 2 or t.shape[0] != n_q
                    or t.shape[1] < k or (t.shape[1] > 1 and t.stride(1) != 1) or (n_q > 1 and t.stride(0) < k)):
                raise _abi.SpvError(f"{op}: out {nm} must be a device tensor [{n_q}, >= {k}] of {dt} with unit column stride")
        if n_q > 1 and idx.stride(0) != values.stride(0):
            raise _abi.SpvError(f"{op}: out idx and {name} must have the same row stride")
    return idx, values, (idx.stride(0) if n_q > 1 else max(k, int(idx.shape[1])))


def _fill_sides(a, Q, C_) -> None:
    """Q / ld_q / n_q / C / ld_c / n_c / D of an argument struct, from tensors ``_sides`` has passed"""
    n_q, n_c, D = int(Q.shape[0]), int(C_.shape[0]), int(Q.shape[1])
    a.Q, a.ld_q, a.n_q = ptr(Q), (Q.stride(0) if n_q > 1 else D), n_q
    a.C, a.ld_c, a.n_c = (ptr(C_) if n_c else ptr(Q)), (C_.stride(0) if n_c > 1 else D), n_c   # an empty tensor has no address; nothing is read
    a.D = D
