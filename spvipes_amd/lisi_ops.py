"""LISI on the device: the fused calibrate-and-Simpson kernel spv_lisi (csrc/spv_lisi.h; include/spvipes_hip.h states the contract) on the
neighbour lists of ``knn_ops.knn_paged``.  ``spVIPES.latent_lisi`` and ``spVIPES.lisi`` run the two on the latents or on any ``obsm`` key;
nothing of size cells x cells is ever stored."""
from __future__ import annotations

import ctypes as C
import math
from typing import Tuple

import torch

from . import _abi
from ._abi import LISI_KMAX, LISI_SETS_MAX, SpvLisiArgs, ptr, stream_ptr   # the limits: part of this module's interface
from ._scan_ops import _out_pair


def lisi(idx: torch.Tensor, dist: torch.Tensor, codes: torch.Tensor, perplexity: float = 30.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The local inverse Simpson index of every row -> (lisi fp64 [n_sets, n], beta fp64 [n], n_valid int32 [n], converged int32 [n]).
    ``idx`` int32 / ``dist`` fp32 [n >= 1, 1 <= k <= LISI_KMAX]: the neighbour lists as ``knn_paged`` returns them (SQUARED distances,
    ascending, -1 / +inf for an empty slot; one common row stride, unit column stride).  ``codes``: contiguous int32 device tensor
    [n_sets, n_c] (or [n_c]: one set), 1 <= n_sets <= LISI_SETS_MAX, one code per candidate row and label set; a negative code, or a
    neighbour index outside [0, n_c), counts for no label.  One calibration per row (LISI's own: beta from 1, at most 50 updates, stop at
    |H - log(perplexity)| < 1e-5) serves every label set.  A row without a finite slot gets lisi = NaN, beta = 1, n_valid = 0,
    converged = 0.  Deterministic: two calls agree bit for bit, and renaming the codes leaves every bit unchanged."""
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or not 1 <= idx.shape[1] <= LISI_KMAX or idx.shape[0] < 1:
        raise _abi.SpvError(f"lisi: idx must be an int32 device tensor [n >= 1, 1 <= k <= {LISI_KMAX}]")
    n, k, dev = int(idx.shape[0]), int(idx.shape[1]), idx.device
    idx, dist, ld = _out_pair("lisi", (idx, dist), "dist", n, k, dev)
    if isinstance(codes, torch.Tensor) and codes.dim() == 1:
        codes = codes[None, :]
    if (not isinstance(codes, torch.Tensor) or not codes.is_cuda or codes.device != dev or codes.dtype != torch.int32 or codes.dim() != 2
            or not 1 <= codes.shape[0] <= LISI_SETS_MAX or not codes.is_contiguous()):
        raise _abi.SpvError(f"lisi: codes must be a contiguous int32 device tensor [1 <= n_sets <= {LISI_SETS_MAX}, n_c]")
    if not (isinstance(perplexity, (int, float)) and not isinstance(perplexity, bool) and math.isfinite(perplexity) and perplexity >= 1):
        raise ValueError(f"lisi: perplexity must be a finite number >= 1, got {perplexity!r}")
    n_sets, n_c = int(codes.shape[0]), int(codes.shape[1])
    out = torch.empty((n_sets, n), dtype=torch.float64, device=dev)
    beta = torch.empty(n, dtype=torch.float64, device=dev)
    n_valid = torch.empty(n, dtype=torch.int32, device=dev)
    converged = torch.empty(n, dtype=torch.int32, device=dev)
    a = SpvLisiArgs()
    a.idx, a.dist, a.ld, a.n, a.k = ptr(idx), ptr(dist), ld, n, k
    a.codes, a.n_c, a.n_sets, a.perplexity = (ptr(codes) if n_c else ptr(idx)), n_c, n_sets, float(perplexity)   # an empty tensor has no address; nothing is read
    a.lisi, a.beta, a.n_valid, a.converged = ptr(out), ptr(beta), ptr(n_valid), ptr(converged)
    _abi.call("spv_lisi", C.byref(a), stream_ptr())
    return out, beta, n_valid, converged
