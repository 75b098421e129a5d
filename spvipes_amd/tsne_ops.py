"""Exact t-SNE on the device: the three kernels of csrc/spv_tsne.h (include/spvipes_hip.h states their contracts) and the driver ``tsne``
that ``spVIPES.latent_tsne`` / ``spVIPES.tsne`` run.  The repulsive half of every gradient is an all-pairs reduction on the fused pair
scan: no tree, no grid, nothing of size n x n, and bit-for-bit repeatable."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _abi
from ._abi import KNN_KMAX, TSNE_DMAX, SpvTsneRepArgs, SpvTsneUpdArgs, ptr, stream_ptr
from ._scan_ops import _fill_sides, _n_split, _sides, _workspace


def tsne_splits(n_q: int, n_c: int) -> int:
    """Chunks of the candidates spv_tsne_repulsion uses for this shape when ``n_split`` is 0: a pure function of the shapes"""
    return int(_abi.load().spv_tsne_splits(int(n_q), int(n_c)))


def tsne_ws_bytes(n_q: int, D: int, n_split: int) -> int:
    """Bytes of workspace for ``n_split`` chunks (the resolved number, not 0): 0 for one chunk"""
    return int(_abi.load().spv_tsne_ws_bytes(int(n_q), int(D), int(n_split)))


def _f64(op: str, t, name: str, shape, dev) -> None:
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape)
            or not t.is_contiguous()):
        raise _abi.SpvError(f"{op}: {name} must be a contiguous fp64 device tensor of shape {tuple(shape)}")


def repulsion(Q: torch.Tensor, C_: torch.Tensor, exclude: Optional[torch.Tensor] = None, n_split: int = 0,
              out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The all-pairs half of a t-SNE gradient -> (Zrow fp64 [n_q], F fp64 [D, n_q]): per query row of ``Q`` the sum over the rows of
    ``C_`` of w = 1 / (1 + d2) and of w^2 (q - c), every pair's value formed in fp32 as spv_tsne_repulsion's contract states and added
    in fp64 in ascending candidate order.  ``Q`` [n_q >= 1, D], ``C_`` [n_c >= 0, D]: fp32 device tensors with unit column stride,
    1 <= D <= TSNE_DMAX.  ``exclude``: contiguous int32 device tensor [n_q], candidate exclude[i] is skipped for query i.  ``n_split``:
    chunks of the candidates, 0 = ``tsne_splits(n_q, n_c)``.  ``out``: (Zrow [n_q], F [D, >= n_q] with unit column stride), fp64.
    Deterministic: two calls agree bit for bit."""
    dev, n_q, n_c, D = _sides("tsne repulsion", Q, C_)
    if D > TSNE_DMAX:
        raise ValueError(f"tsne repulsion: D must lie in [1, {TSNE_DMAX}], got {D}")
    n_split = _n_split("tsne repulsion", n_split)
    if exclude is not None and (not isinstance(exclude, torch.Tensor) or not exclude.is_cuda or exclude.device != dev or exclude.dtype != torch.int32
                                or exclude.dim() != 1 or exclude.numel() != n_q or not exclude.is_contiguous()):
        raise _abi.SpvError(f"tsne repulsion: exclude must be a contiguous int32 device tensor with one entry per query ({n_q})")
    if out is None:
        Zrow, F = torch.empty(n_q, dtype=torch.float64, device=dev), torch.empty((D, n_q), dtype=torch.float64, device=dev)
    else:
        Zrow, F = out
        _f64("tsne repulsion", Zrow, "out Zrow", (n_q,), dev)
        if (not isinstance(F, torch.Tensor) or not F.is_cuda or F.device != dev or F.dtype != torch.float64 or F.dim() != 2 or F.shape[0] != D
                or F.shape[1] < n_q or (F.shape[1] > 1 and F.stride(1) != 1) or (D > 1 and F.stride(0) < n_q)):
            raise _abi.SpvError(f"tsne repulsion: out F must be an fp64 device tensor [{D}, >= {n_q}] with unit column stride")
    ws = _workspace(tsne_ws_bytes(n_q, D, n_split or tsne_splits(n_q, n_c)), dev)
    a = SpvTsneRepArgs()
    _fill_sides(a, Q, C_)
    a.exclude, a.n_split = ptr(exclude), n_split
    a.Zrow, a.F, a.ld_f, a.ws = ptr(Zrow), ptr(F), (F.stride(0) if D > 1 else max(n_q, int(F.shape[1]))), ptr(ws)
    _abi.call("spv_tsne_repulsion", C.byref(a), stream_ptr())
    return Zrow, F[:, :n_q]


def affinities(d2: torch.Tensor, perplexity: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The perplexity calibration -> (P fp32 [n, k], beta fp64 [n]).  ``d2``: contiguous fp32 device tensor [n >= 1, 1 <= k <= KNN_KMAX],
    per row the squared distances of ``knn`` in ascending order, +inf for an empty slot.  Per row the search of scikit-learn's
    ``_binary_search_perplexity`` in fp64 on d2 - d2[:, :1]: P = exp(-beta d) / sum, an empty slot gets 0 and does not count."""
    if (not isinstance(d2, torch.Tensor) or not d2.is_cuda or d2.dtype != torch.float32 or d2.dim() != 2 or d2.shape[0] < 1
            or not 1 <= d2.shape[1] <= KNN_KMAX or not d2.is_contiguous()):
        raise _abi.SpvError(f"tsne affinities: d2 must be a contiguous fp32 device tensor [n >= 1, 1 <= k <= {KNN_KMAX}]")
    if not (isinstance(perplexity, (int, float)) and not isinstance(perplexity, bool) and math.isfinite(perplexity) and perplexity >= 1):
        raise ValueError(f"tsne affinities: perplexity must be a finite number >= 1, got {perplexity!r}")
    n, k = int(d2.shape[0]), int(d2.shape[1])
    P = torch.empty_like(d2)
    beta = torch.empty(n, dtype=torch.float64, device=d2.device)
    _abi.call("spv_tsne_affinities", ptr(d2), ptr(P), k, n, k, float(perplexity), ptr(beta), stream_ptr())
    return P, beta


def update(y_in: torch.Tensor, y_out: torch.Tensor, indptr: torch.Tensor, cols: torch.Tensor, vals: torch.Tensor, Zrow: torch.Tensor,
           F: torch.Tensor, Z: torch.Tensor, u: torch.Tensor, gain: torch.Tensor, alpha: float, momentum: float, lr: float, min_gain: float = 0.01,
           kl_row: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None) -> None:
    """The sparse half of the gradient and the step, spv_tsne_update: Z[0] = sum(Zrow) in a fixed order, then per row of the symmetric
    CSR matrix P (``indptr`` int64 [n + 1], ``cols`` int32 ascending per row, ``vals`` fp32) the attractive term, the gradient
    g = 4 (alpha A - F / Z) in fp64 and scikit-learn's step.  ``y_in`` is read, ``y_out`` written (two different contiguous fp32 tensors
    [n, D]); ``u`` and ``gain`` (fp32 [n, D]) change in place.  ``Zrow`` [n] / ``F`` [D, n]: contiguous fp64, of ``repulsion``; ``Z``: fp64
    [1].  ``kl_row`` (fp64 [n]): sum_j p_ij (log p_ij - log w_ij), so KL = kl_row.sum() + log Z.  ``grad`` (fp64 [D, n]): g."""
    op = "tsne update"
    if (not isinstance(y_in, torch.Tensor) or not y_in.is_cuda or y_in.dtype != torch.float32 or y_in.dim() != 2 or y_in.shape[0] < 1
            or not 1 <= y_in.shape[1] <= TSNE_DMAX or not y_in.is_contiguous()):
        raise _abi.SpvError(f"{op}: y_in must be a contiguous fp32 device tensor [n >= 1, 1 <= D <= {TSNE_DMAX}]")
    dev, n, D = y_in.device, int(y_in.shape[0]), int(y_in.shape[1])
    for t, name in ((y_out, "y_out"), (u, "u"), (gain, "gain")):
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != (n, D) or not t.is_contiguous()):
            raise _abi.SpvError(f"{op}: {name} must be a contiguous fp32 device tensor of y_in's shape")
    if y_out.data_ptr() == y_in.data_ptr():
        raise _abi.SpvError(f"{op}: y_out must not be y_in")
    for t, dt, name in ((indptr, torch.int64, "indptr"), (cols, torch.int32, "cols"), (vals, torch.float32, "vals")):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
            raise _abi.SpvError(f"{op}: {name} must be a contiguous device vector of {dt}")
    if indptr.numel() != n + 1 or cols.numel() != vals.numel():
        raise _abi.SpvError(f"{op}: indptr must hold n + 1 = {n + 1} entries, cols and vals one per entry of P")
    _f64(op, Zrow, "Zrow", (n,), dev), _f64(op, F, "F", (D, n), dev), _f64(op, Z, "Z", (1,), dev)
    if kl_row is not None:
        _f64(op, kl_row, "kl_row", (n,), dev)
    if grad is not None:
        _f64(op, grad, "grad", (D, n), dev)
    pad = cols.numel() == 0   # an empty tensor has no address; nothing is read
    a = SpvTsneUpdArgs()
    a.y_in, a.y_out, a.ld_y, a.n, a.D = ptr(y_in), ptr(y_out), D, n, D
    a.indptr, a.cols, a.vals = ptr(indptr), ptr(indptr if pad else cols), ptr(indptr if pad else vals)
    a.Zrow, a.F, a.ld_f, a.Z, a.u, a.gain = ptr(Zrow), ptr(F), n, ptr(Z), ptr(u), ptr(gain)
    a.alpha, a.momentum, a.lr, a.min_gain = float(alpha), float(momentum), float(lr), float(min_gain)
    a.kl_row, a.grad = ptr(kl_row), ptr(grad)
    _abi.call("spv_tsne_update", C.byref(a), stream_ptr())


@dataclass
class TsneResult:
    """What ``tsne`` returns.  ``embedding`` fp32 [n, n_components], centred; ``kl_divergence``: the KL divergence of exactly that
    embedding; ``kl_history`` float64 [m, 2]: (steps taken, KL there) every ``kl_every`` steps, the last row the final one; ``beta`` fp64
    [n]: each cell's calibrated precision; ``n_neighbors``: the neighbours per cell the affinities rest on; ``affinities``: the symmetric
    P as (indptr int64, cols int32, vals fp32), its entries summing to 1."""
    embedding: np.ndarray
    kl_divergence: float
    kl_history: np.ndarray
    beta: np.ndarray
    n_neighbors: int
    affinities: Tuple[np.ndarray, np.ndarray, np.ndarray]


def tsne(X: torch.Tensor, perplexity: float = 30.0, n_components: int = 2, n_iter: int = 1000, init="pca", seed: int = 0,
         early_exaggeration: float = 12.0, exaggeration_iter: int = 250, learning_rate="auto", momentum: Tuple[float, float] = (0.5, 0.8),
         min_gain: float = 0.01, kl_every: int = 50) -> TsneResult:
    """Exact t-SNE of the rows of ``X`` (fp32 device tensor [n, D <= KNN_DMAX], finite) with scikit-learn's exact-method schedule:
    ``early_exaggeration`` for the first ``exaggeration_iter`` steps at momentum[0], then momentum[1]; learning rate
    max(n / early_exaggeration / 4, 50) for "auto"; gains with floor ``min_gain``; ``n_iter`` steps, ALWAYS all of them: there is no early
    stop.  The affinities rest on each cell's k = min(3 perplexity, 64, n - 1) exact nearest neighbours (``knn``); scikit-learn's exact
    method uses all n - 1, its Barnes-Hut method 3 perplexity: beyond perplexity 21 the 64 neighbours the k-NN kernel can return are FEWER
    than 3 perplexity, which is why ``perplexity`` must lie in [2, k / 2] (at most 32).  The gradient is exact: the repulsive forces and
    the normaliser run over all pairs (``repulsion``), nothing is approximated by a tree or a grid.  ``init``: "pca" (fp64 principal
    axes, sign fixed, scaled to a standard deviation of 1e-4 along the first), "random" (seeded normal draws, 1e-4) or an array
    [n, n_components].  Nothing is copied to the host inside the loop: the KL divergence every ``kl_every`` steps goes into a device
    buffer that is read once at the end.  Deterministic: two calls agree bit for bit."""
    from .data import check_tsne_args, tsne_initial_layout, tsne_symmetrize
    from .knn_ops import knn
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2:
        raise _abi.SpvError("tsne: X must be an fp32 device tensor [n, D]")
    n, dev = int(X.shape[0]), X.device
    s = check_tsne_args(n, perplexity, n_components, n_iter, init, seed, early_exaggeration=early_exaggeration, exaggeration_iter=exaggeration_iter,
                        learning_rate=learning_rate, momentum=momentum, min_gain=min_gain, kl_every=kl_every)
    k, d = s["n_neighbors"], s["n_components"]
    X = X.contiguous()
    me = torch.arange(n, dtype=torch.int32, device=dev)
    idx, d2 = knn(X, X, k, exclude=me)
    P, beta = affinities(d2.contiguous(), s["perplexity"])
    indptr_h, cols_h, vals_h = tsne_symmetrize(idx.cpu().numpy(), P.cpu().numpy(), n)
    indptr, cols, vals = (torch.from_numpy(v).to(dev) for v in (indptr_h, cols_h, vals_h))
    Y0 = tsne_initial_layout(init, X.cpu().numpy() if isinstance(init, str) and init == "pca" else None, n, d, s["seed"])
    Y = [torch.from_numpy(Y0).to(dev).contiguous(), torch.empty((n, d), dtype=torch.float32, device=dev)]
    u, gain = torch.zeros((n, d), dtype=torch.float32, device=dev), torch.ones((n, d), dtype=torch.float32, device=dev)
    Zrow, F = torch.empty(n, dtype=torch.float64, device=dev), torch.empty((d, n), dtype=torch.float64, device=dev)
    Z, kl_row = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    marks = [it for it in range(s["n_iter"]) if it % s["kl_every"] == 0]
    kl_buf = torch.zeros(len(marks) + 1, dtype=torch.float64, device=dev)
    for it in range(s["n_iter"]):
        early = it < s["exaggeration_iter"]
        record = it % s["kl_every"] == 0
        repulsion(Y[0], Y[0], exclude=me, out=(Zrow, F))
        update(Y[0], Y[1], indptr, cols, vals, Zrow, F, Z, u, gain, s["early_exaggeration"] if early else 1.0, s["momentum"][0 if early else 1],
               s["learning_rate"], s["min_gain"], kl_row=kl_row if record else None)
        if record:
            kl_buf[it // s["kl_every"]] = kl_row.sum() + torch.log(Z[0])
        Y.reverse()
    # the embedding, centred in fp64, and ITS divergence: one more pass of both kernels with a step of zero
    Y64 = Y[0].double()
    Y[0] = (Y64 - Y64.mean(dim=0, keepdim=True)).float().contiguous()
    repulsion(Y[0], Y[0], exclude=me, out=(Zrow, F))
    update(Y[0], Y[1], indptr, cols, vals, Zrow, F, Z, u, gain, 1.0, 0.0, 0.0, s["min_gain"], kl_row=kl_row)
    kl_buf[len(marks)] = kl_row.sum() + torch.log(Z[0])
    kl = kl_buf.cpu().numpy()
    history = np.stack([np.asarray(marks + [s["n_iter"]], dtype=np.float64), kl], axis=1)
    return TsneResult(embedding=Y[0].cpu().numpy(), kl_divergence=float(kl[-1]), kl_history=history, beta=beta.cpu().numpy(), n_neighbors=k,
                      affinities=(indptr_h, cols_h, vals_h))
