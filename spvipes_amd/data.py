"""Device-resident data for the hot path: count matrices, minibatch sampler, synthetic generator.

Replaces the reference's host-side iterators
    data/_multi_datasplitter.py:65-98   per-group permutation split, train loader shuffle + drop_last
    dataloaders/_concat_dataloader.py:101-110  zip of per-group loaders, shorter ones cycled
    dataloaders/_ann_dataloader.py      batch sampler + AnnTorchDataset row densification
with an index sampler: the count matrices stay in HBM (uint16 when the counts are integral and
< 65536, else float32) and a minibatch is just an int32 row-index vector per group that the
kernels gather through.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _abi
from .ops import GroupCounts, SparseGroupCounts


_NEGATIVE_COUNTS = "count matrices must be non-negative (the likelihood is evaluated at log1p(count); the reference gives NaN for counts <= -1)"


def to_group_counts(X, device, prefer_u16: bool = True, col_off: int = 0, G: Optional[int] = None) -> GroupCounts:
    """Move a dense [cells, genes] count array into HBM (uint16 if lossless, else float32)."""
    if isinstance(X, torch.Tensor):
        Xn = X.detach().cpu().numpy()
    else:
        Xn = np.asarray(X)
    G = Xn.shape[1] - col_off if G is None else G
    if Xn.size and float(Xn.min()) < 0:
        raise ValueError(_NEGATIVE_COUNTS)
    if prefer_u16 and Xn.size and float(Xn.min()) >= 0 and float(Xn.max()) < 65536 and np.all(Xn == np.floor(Xn)):
        t = torch.from_numpy(np.ascontiguousarray(Xn.astype(np.uint16)).view(np.int16))
    else:
        t = torch.from_numpy(np.ascontiguousarray(Xn.astype(np.float32)))
    return GroupCounts(t.to(device), G, col_off, resident=True)


def is_sparse(X) -> bool:
    """a scipy.sparse matrix or array (or anything else with ``.tocsr()``)"""
    return hasattr(X, "tocsr") and not isinstance(X, (np.ndarray, torch.Tensor))


def csr_group_arrays(X, obs_idx, var_idx, prefer_u16: bool = True):
    """One group's counts ``X[obs_idx][:, var_idx]`` as CSR arrays without densifying them: (indptr int64 [n + 1], cols int32 (sorted
    within a row, duplicates summed), vals, dtype) with dtype / vals uint16 when every stored value is integral and < 65536, else
    float32 -- to_group_counts' rule (implicit zeros are integral and in range).  ``X``: anything with ``.tocsr()`` (scipy CSR, CSC, COO,
    ...; a CSR input is only read), or a dense array.  The group's genes may be any columns (an outer join's ``groups_var_indices``)."""
    obs_idx = np.asarray(obs_idx, dtype=np.int64).reshape(-1)
    var_idx = np.asarray(var_idx, dtype=np.int64).reshape(-1)
    n, G = len(obs_idx), len(var_idx)
    if len(np.unique(var_idx)) != G:
        raise ValueError("groups_var_indices must not repeat a gene")
    if is_sparse(X):
        M = X.tocsr()
        n_var = M.shape[1]
        ip = np.asarray(M.indptr, dtype=np.int64)
        starts, lens = ip[obs_idx], ip[obs_idx + 1] - ip[obs_idx]
        row = np.repeat(np.arange(n, dtype=np.int64), lens)
        src = np.arange(row.size, dtype=np.int64) + np.repeat(starts - (np.cumsum(lens) - lens), lens)
        gcol, vals = np.asarray(M.indices)[src], np.asarray(M.data)[src]
        del src
    else:
        D = X.detach().cpu().numpy() if isinstance(X, torch.Tensor) else np.asarray(X)
        n_var = D.shape[1]
        sub = D[obs_idx]
        row, gcol = np.nonzero(sub)
        vals = sub[row, gcol]
        del sub
    colmap = np.full(n_var, -1, dtype=np.int64)
    colmap[var_idx] = np.arange(G)
    loc = colmap[gcol]
    keep = loc >= 0
    if not keep.all():
        row, loc, vals = row[keep], loc[keep], vals[keep]
    del gcol, keep
    key = row * max(G, 1) + loc
    if key.size > 1 and not bool(np.all(key[1:] > key[:-1])):   # unsorted columns or duplicate entries: sort, sum duplicates
        order = np.argsort(key, kind="stable")
        key, vals = key[order], vals[order]
        del order
        first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
        vals = np.add.reduceat(vals, first) if first.size else vals
        key = key[first]
    row, loc = key // max(G, 1), key % max(G, 1)
    del key
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=indptr[1:])
    if vals.size and float(vals.min()) < 0:
        raise ValueError(_NEGATIVE_COUNTS)
    if prefer_u16 and n * G and (vals.size == 0 or (float(vals.max()) < 65536 and np.all(vals == np.floor(vals)))):
        return indptr, loc.astype(np.int32), vals.astype(np.uint16), _abi.SPV_COUNT_U16
    return indptr, loc.astype(np.int32), vals.astype(np.float32), _abi.SPV_COUNT_F32


def csr_to_dense(indptr, cols, vals, G: int) -> np.ndarray:
    """host densification of csr_group_arrays' output (``counts_storage="dense"`` on a sparse AnnData: one group at a time)"""
    n = len(indptr) - 1
    out = np.zeros((n, G), dtype=vals.dtype)
    out[np.repeat(np.arange(n), np.diff(indptr)), cols] = vals
    return out


def to_sparse_group_counts(X, obs_idx, var_idx, device) -> SparseGroupCounts:
    """One group of an AnnData's counts resident in HBM as CSR (csr_group_arrays, then the three arrays to the device)"""
    indptr, cols, vals, _ = csr_group_arrays(X, obs_idx, var_idx)
    return SparseGroupCounts.from_arrays(indptr, cols, vals, len(np.asarray(var_idx).reshape(-1)), device)


@dataclass
class SyntheticGroup:
    counts: GroupCounts
    labels: torch.Tensor  # float32 [n_cells] label codes (the reference carries labels as float32)


def make_synthetic_group(g: int, n_cells: int, n_genes: int, device, n_labels: int = 10, dtype: str = "u16",
                         chunk: int = 4096, shard: int = 0) -> SyntheticGroup:
    """SURVEY.md 8d synthetic counts: X[c,j] ~ NB(mean = s_c * exp(a[label(c), j]), dispersion 2) * Bernoulli(0.2),
    s_c ~ LogNormal(0, 0.25), a ~ N(0, 1), 10 labels (group 0 never has label 0, group 1 never has
    label n_labels-1 so the non-common-label branch of the PoE runs).  Small tables come from
    numpy.random.default_rng(1000 + g); the [cells, genes] draws are generated on the device with a
    torch generator seeded 1000 + g (a 5e8-entry numpy NB draw per group would dominate start-up).  ``shard`` (a rank of a
    data-parallel job) offsets both seeds by 10 per shard: ranks hold DIFFERENT cells, as a sharded data set does."""
    rng = np.random.default_rng(1000 + g + 10 * shard)
    allowed = [l for l in range(n_labels) if l != (0 if g == 0 else n_labels - 1)]
    labels = rng.choice(allowed, size=n_cells)
    a = rng.normal(size=(n_labels, n_genes)).astype(np.float32)
    s = rng.lognormal(0.0, 0.25, size=n_cells).astype(np.float32)
    gen = torch.Generator(device=device).manual_seed(1000 + g + 10 * shard)
    a_d, s_d = torch.tensor(a, device=device), torch.tensor(s, device=device)
    lab_d = torch.tensor(labels, device=device)
    out = torch.empty((n_cells, n_genes), dtype=torch.int16 if dtype == "u16" else torch.float32, device=device)
    for lo in range(0, n_cells, chunk):
        hi = min(lo + chunk, n_cells)
        mean = s_d[lo:hi, None] * torch.exp(a_d[lab_d[lo:hi]])
        lam = torch._standard_gamma(torch.full_like(mean, 2.0), generator=gen) * (mean / 2.0)  # Gamma(shape 2, mean `mean`)
        cnt = torch.poisson(lam, generator=gen)
        cnt = cnt * (torch.rand(cnt.shape, device=device, generator=gen) < 0.2)
        cnt[:, 0] += (cnt.sum(1) == 0)  # no empty cell: library = log(sum log1p(x)) must be finite
        cnt = cnt.clamp_(max=65535.0)
        out[lo:hi] = cnt.to(torch.int32).to(torch.int16) if dtype == "u16" else cnt
    return SyntheticGroup(GroupCounts(out, n_genes, 0, resident=True), torch.tensor(labels, dtype=torch.float32, device=device))


class MinibatchSampler:
    """Per-group row-index minibatches with the reference's epoch semantics.

    * split: ``np.random.RandomState(seed).permutation(group_indices)`` per group, validation rows
      first, then training rows (data/_multi_datasplitter.py:66-79; scvi ``validate_data_split``:
      n_train = ceil(train_size * n), n_val = n - n_train by default);
    * training epochs: every group reshuffled, ``drop_last=True``; the epoch has as many steps as
      the group with the most batches; a group that runs out REPLAYS the batches of its first pass
      in order (``itertools.cycle`` caches them, dataloaders/_concat_dataloader.py:108-110);
    * evaluation order: sequential, ``drop_last=False``.

    A rank of a data-parallel job keeps the contiguous shard [rank::world] of every group's
    training rows, so ranks draw disjoint minibatches."""

    def __init__(self, n_cells: Sequence[int], batch_size: int, device, seed: int = 0, train_size: float = 1.0,
                 validation_size: Optional[float] = None, rank: int = 0, world: int = 1,
                 group_indices_list: Optional[Sequence[Sequence[int]]] = None):
        self.batch_size, self.device = batch_size, device
        rs = np.random.RandomState(seed=seed)
        self.train_idx: List[np.ndarray] = []
        self.val_idx: List[np.ndarray] = []
        for g, n in enumerate(n_cells):
            idx = np.arange(n) if group_indices_list is None else np.asarray(group_indices_list[g])
            n_train = int(np.ceil(train_size * len(idx)))
            n_val = (len(idx) - n_train) if validation_size is None else int(np.floor(validation_size * len(idx)))
            perm = rs.permutation(idx)
            self.val_idx.append(perm[:n_val])
            tr = perm[n_val:n_val + n_train]
            if world > 1:
                per = len(tr) // world
                tr = tr[rank * per:(rank + 1) * per]
            self.train_idx.append(tr)
        self._train_dev = [torch.as_tensor(t, dtype=torch.int32, device=device) for t in self.train_idx]
        self._gen = torch.Generator(device=device).manual_seed(seed + 7919 * (rank + 1))
        self.batches_per_group = [len(t) // batch_size for t in self.train_idx]
        if min(self.batches_per_group) == 0:
            raise ValueError("batch_size larger than a group's training shard")
        self.steps_per_epoch = max(self.batches_per_group)

    def draw_permutations(self):
        """one fresh permutation of every group's training rows (the per-epoch reshuffle of the reference's train loaders)"""
        return [t[torch.randperm(len(t), device=self.device, generator=self._gen)] for t in self._train_dev]

    def epoch_from_permutations(self, perms):
        """The steps of one epoch given each group's visiting order: drop_last batches; the group with the most batches
        leads; a group that runs out REPLAYS the batches of its first pass in order (ConcatDataLoader wraps the shorter
        loaders in itertools.cycle, dataloaders/_concat_dataloader.py:108-110)."""
        B = self.batch_size
        for step in range(self.steps_per_epoch):
            out = []
            for g, p in enumerate(perms):
                i = step % self.batches_per_group[g]
                out.append(p[i * B:(i + 1) * B].contiguous())
            yield out

    def epoch(self):
        """Yields a list (one int32 [batch_size] row-index tensor per group) per training step."""
        yield from self.epoch_from_permutations(self.draw_permutations())

    @staticmethod
    def sequential(indices: Sequence[int], batch_size: int, device):
        idx = torch.as_tensor(np.asarray(indices), dtype=torch.int32, device=device)
        for lo in range(0, len(idx), batch_size):
            yield idx[lo:lo + batch_size].contiguous()


def latent_loader_mode(use_labels: bool, use_transport_plan: bool, pair_data: bool, drop_last: Optional[bool]):
    """(drop_last, use_cycling) as get_latent_representation decides them (model/spvipes.py:468-503): ``drop_last=None``
    means False for every PoE flavour; the cycling path is taken by the paired PoE only (a transport plan, ``pair_data``, no
    labels) and only when no batch is dropped."""
    drop_last = bool(drop_last) if drop_last is not None else False
    return drop_last, bool(use_transport_plan and pair_data and not drop_last and not use_labels)


def latent_steps(local: Sequence[Sequence[int]], batch_size: int, drop_last: bool, use_cycling: bool):
    """The (group-0 rows, group-1 rows) pairs get_latent_representation feeds to the module, in order
    (model/spvipes.py:497-523 and the cycling path :578-626): sequential batches, last partial batch kept unless
    ``drop_last``; the group with more batches leads (the first on ties) and the other one's batches are replayed
    cyclically; with ``use_cycling`` the cells are first cut into chunks of min(n0, n1) cells per group, the shorter group's
    cells wrapping around, and every chunk is batched on its own with the partial batch kept."""
    def batches(idx, dl):
        idx = np.asarray(idx)
        out = [idx[lo:lo + batch_size] for lo in range(0, len(idx), batch_size)]
        if dl and out and len(out[-1]) < batch_size:
            out.pop()
        return out

    n0, n1 = len(local[0]), len(local[1])
    if use_cycling:
        mn, mx = min(n0, n1), max(n0, n1)
        if mn == 0:
            raise ValueError("One of the groups is empty")
        a0, a1 = np.asarray(local[0]), np.asarray(local[1])
        chunks = [(a0[(s + np.arange(mn)) % n0], a1[(s + np.arange(mn)) % n1]) for s in range(0, mx, mn)]
        dl = False
    else:
        chunks, dl = [(local[0], local[1])], drop_last
    steps = []
    for c0, c1 in chunks:
        b0, b1 = batches(c0, dl), batches(c1, dl)
        if not b0 or not b1:
            continue   # (a loader without a batch ends the reference's zip() at once)
        n = max(len(b0), len(b1))   # the loader with the most batches leads, the other is replayed cyclically
        steps += [(b0[i % len(b0)], b1[i % len(b1)]) for i in range(n)]
    return steps


def walk_positions(steps, g: int, n_g: int):
    """The eval walk ``steps`` ((step, tensors, (B0, B1)), as ``_eval_minibatches`` yields them) with group g's bookkeeping -> (step, tensors, (B0, B1),
    off, pos): the step's rows are rows off .. off + B_g - 1 of the group's concatenated read-out, ``pos`` (int64) those positions, with -1 for every
    one at or beyond ``n_g`` -- the replayed rows, which a read-out cuts off and a reduction must not count twice."""
    off = 0
    for step, tensors, B in steps:
        pos = off + np.arange(B[g], dtype=np.int64)
        yield step, tensors, B, off, np.where(pos < n_g, pos, -1)
        off += B[g]


class RowBlocks:
    """Per-step blocks of a two-group read-out, copied to the host as they complete or kept on the device; ``result``: concatenated, cut at the sizes ``n``"""

    def __init__(self, n: Sequence[int], return_numpy: bool):
        self.n, self.return_numpy, self.blocks = n, return_numpy, ([], [])

    def add(self, per_group) -> None:
        for g, block in enumerate(per_group):
            self.blocks[g].append(block.cpu().numpy() if self.return_numpy else block)

    def result(self) -> dict:
        cat = np.concatenate if self.return_numpy else torch.cat
        return {g: cat(self.blocks[g])[:self.n[g]] for g in range(2)}


def format_latent_results(private0, private1, shared0, shared1, indices1, n0: int, n1: int) -> dict:
    """model/spvipes.py:628-650: per-step arrays concatenated, truncated to the group sizes; the ``*_reordered`` entries sort
    GROUP 1 ONLY by its 'indices' column (group 0 is returned as is)."""
    i1 = np.concatenate(indices1).flatten()[:n1]
    p = {0: np.concatenate(private0)[:n0], 1: np.concatenate(private1)[:n1]}
    s = {0: np.concatenate(shared0)[:n0], 1: np.concatenate(shared1)[:n1]}
    order = np.argsort(i1)
    return {"shared": s, "private": p, "shared_reordered": {0: s[0], 1: s[1][order]}, "private_reordered": {0: p[0], 1: p[1][order]}}


# ---- denoised-expression read-out (model.get_normalized_expression): host-side argument handling ------------------------------
EXPRESSION_COMPONENTS = {"mixture": 0, "private": 1, "shared": 2, "mixing": 3}   # -> ``what`` of spv_dec_expected


def expression_what(component) -> int:
    """"mixture" | "private" | "shared" | "mixing" (or the code 0..3 itself) -> the ``what`` code of spv_dec_expected"""
    if isinstance(component, str) and component in EXPRESSION_COMPONENTS:
        return EXPRESSION_COMPONENTS[component]
    if isinstance(component, (int, np.integer)) and not isinstance(component, bool) and 0 <= int(component) <= 3:
        return int(component)
    raise ValueError(f"component must be one of {sorted(EXPRESSION_COMPONENTS)}, got {component!r}")


def expression_log_library(library_size) -> Optional[float]:
    """``library_size``: "latent" -> None (the model's own library), a positive finite number L -> log L, the value the library
    vector handed to spv_dec_lse is filled with (rate = L * softmax)"""
    if isinstance(library_size, str):
        if library_size != "latent":
            raise ValueError(f"library_size must be 'latent' or a positive number, got {library_size!r}")
        return None
    try:
        L = float(library_size)
    except (TypeError, ValueError):
        raise ValueError(f"library_size must be 'latent' or a positive number, got {library_size!r}") from None
    if not (L > 0.0 and math.isfinite(L)):
        raise ValueError(f"library_size must be 'latent' or a positive number, got {library_size!r}")
    return math.log(L)


def check_expression_args(component, library_size, n_samples, use_mean: bool):
    """The argument checks of get_normalized_expression: -> (what code, log L or None, n_samples).  ``n_samples`` must be a
    positive integer and, when the posterior means are decoded (``use_mean``), 1: there is nothing to average."""
    what, log_l = expression_what(component), expression_log_library(library_size)
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or int(n_samples) < 1:
        raise ValueError(f"n_samples must be a positive integer, got {n_samples!r}")
    if use_mean and int(n_samples) > 1:
        raise ValueError("n_samples > 1 needs use_mean=False: decoding the posterior means is deterministic, there is nothing to average")
    return what, log_l, int(n_samples)


SAMPLE_MAX_SEED = (1 << 32) - 1   # the seed is the low word of the sampler's Philox key (dec_ops.sample_key)


def check_sample_args(n_samples, seed, library_size):
    """The argument checks of posterior_predictive_sample: -> (n_samples, seed, log L or None).  ``n_samples`` a positive integer,
    ``seed`` an integer in [0, 2^32), ``library_size`` "latent" or a positive number (as get_normalized_expression takes it)."""
    log_l = expression_log_library(library_size)
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or int(n_samples) < 1:
        raise ValueError(f"n_samples must be a positive integer, got {n_samples!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= SAMPLE_MAX_SEED:
        raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
    return int(n_samples), int(seed), log_l


def group_var_names(adata, n_groups: int = 2):
    """Per group the names of its own genes, as get_loadings labels them: ``adata.var_names`` cut by ``uns["groups_var_indices"]``,
    else ``uns["groups_var_names"]`` (list or dict), else None"""
    out = []
    for g in range(n_groups):
        names = None
        if getattr(adata, "var_names", None) is not None:
            names = np.asarray(adata.var_names)[np.asarray(adata.uns["groups_var_indices"][g])]
        elif adata.uns.get("groups_var_names") is not None:
            gv = adata.uns["groups_var_names"]
            names = np.asarray(gv[g] if not isinstance(gv, dict) else list(gv.values())[g])
        out.append(names)
    return out


def resolve_gene_list(gene_list, n_genes: Sequence[int], var_names=None) -> List[Optional[np.ndarray]]:
    """``gene_list`` of get_normalized_expression -> per group None (all genes in order) or an int32 array of positions within the
    group's own genes.  ``gene_list``: None, or one entry per group, each None | integer positions | gene names (looked up in
    ``var_names[g]``, the group's own names; the first occurrence of a repeated name).  Any order, repeats allowed.  Unknown names
    raise KeyError and positions outside [0, n_genes[g]) IndexError, both naming the offender."""
    ng = len(n_genes)
    if gene_list is None:
        return [None] * ng
    if isinstance(gene_list, (str, bytes)) or not hasattr(gene_list, "__len__") or len(gene_list) != ng:
        raise ValueError(f"gene_list must be None or hold one entry per group ({ng}): None, positions or names")
    out = []
    for g in range(ng):
        sel = gene_list[g] if not isinstance(gene_list, dict) else gene_list.get(g)
        if sel is None:
            out.append(None)
            continue
        if isinstance(sel, (str, bytes)):
            sel = [sel]
        arr = np.asarray(sel)
        if arr.ndim != 1 or arr.size == 0:
            raise ValueError(f"gene_list[{g}] must be a non-empty 1-d sequence of positions or names")
        if arr.dtype == bool:
            raise TypeError(f"gene_list[{g}]: boolean masks are not supported, pass positions or names")
        if np.issubdtype(arr.dtype, np.integer):
            bad = np.nonzero((arr < 0) | (arr >= n_genes[g]))[0]
            if bad.size:
                raise IndexError(f"gene_list[{g}]: position {int(arr[bad[0]])} is out of range for a group of {n_genes[g]} genes")
            out.append(arr.astype(np.int32))
            continue
        if arr.dtype.kind not in "USO":
            raise TypeError(f"gene_list[{g}] must hold integer positions or gene names, got dtype {arr.dtype}")
        names = None if var_names is None else var_names[g]
        if names is None:
            raise KeyError(f"gene_list[{g}] holds names ({arr[0]!r}, ...) but the AnnData carries neither var_names nor uns['groups_var_names']")
        first = {}
        for i, nme in enumerate(np.asarray(names).astype(str)):
            first.setdefault(nme, i)
        pos = np.empty(arr.size, np.int32)
        for i, nme in enumerate(arr.astype(str)):
            if nme not in first:
                raise KeyError(f"gene_list[{g}]: gene {nme!r} is not among the genes of group {g}")
            pos[i] = first[nme]
        out.append(pos)
    return out


# ---- differential expression (model.differential_expression): host-side argument handling, pairing and the result table ---------
DE_COLUMNS = ("proba_de", "proba_not_de", "bayes_factor", "scale1", "scale2", "lfc_mean", "lfc_std", "lfc_min", "lfc_max")
DE_MAX_PAIRS = 1 << 24   # spv_de_pairs carries the exceedance count as fp32 whole numbers


def check_de_args(n_pairs, delta, pseudocount, fdr_target, max_cells=None):
    """The argument checks of differential_expression that are its own (component / library_size / n_samples / use_mean go through
    ``check_expression_args``): -> (n_pairs, delta, pseudocount, fdr_target, max_cells) as plain numbers"""
    if isinstance(n_pairs, bool) or not isinstance(n_pairs, (int, np.integer)) or not 1 <= int(n_pairs) <= DE_MAX_PAIRS:
        raise ValueError(f"n_pairs must be an integer between 1 and 2^24, got {n_pairs!r}")

    def number(v, name, ok):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if isinstance(v, (bool, str)) or not (math.isfinite(f) and ok(f)):
            raise ValueError(f"{name} got {v!r}")
        return f

    delta = number(delta, "delta must be a non-negative number,", lambda f: f >= 0.0)
    pseudocount = number(pseudocount, "pseudocount must be a non-negative number,", lambda f: f >= 0.0)
    fdr_target = number(fdr_target, "fdr_target must lie in [0, 1],", lambda f: 0.0 <= f <= 1.0)
    if max_cells is not None and (isinstance(max_cells, bool) or not isinstance(max_cells, (int, np.integer)) or int(max_cells) < 1):
        raise ValueError(f"max_cells must be None or a positive integer, got {max_cells!r}")
    return int(n_pairs), delta, pseudocount, fdr_target, (None if max_cells is None else int(max_cells))


def check_group(group) -> int:
    """``group`` of the one-group read-outs: 0 or 1, else ValueError"""
    if group not in (0, 1):
        raise ValueError(f"group must be 0 or 1, got {group!r}")
    return int(group)


def group_cell_labels(obs, groupby, cells: np.ndarray, g: int, unique: bool = False) -> np.ndarray:
    """``groupby`` -> one label per cell of ``cells`` (= ``group_indices_list[g]``, adata row numbers): the name of a column of ``obs``
    (KeyError for an unknown one) or an array of that length (else ValueError).  ``unique``: then, ValueError for a cell listed twice."""
    if isinstance(groupby, str):
        if groupby not in obs:
            raise KeyError(f"groupby: adata.obs has no column {groupby!r}")
        cell_labels = np.asarray(obs[groupby])[cells]
    else:
        cell_labels = np.asarray(groupby).ravel()
        if cell_labels.shape[0] != len(cells):
            raise ValueError(f"groupby: an array must hold one label per cell of group_indices_list[{g}] ({len(cells)}), got {cell_labels.shape[0]}")
    if unique and len(np.unique(cells)) != len(cells):
        raise ValueError(f"group_indices_list[{g}] lists a cell more than once")
    return cell_labels


def vs_rest_frames(tables, index):
    """The frame of a one-vs-rest read-out: ``tables`` = (label, column -> array) per compared label, in order -> their frames over
    ``index`` with ``comparison`` ("<label> vs Rest"), ``group1`` (the label) and ``group2`` ("Rest") appended, concatenated."""
    import pandas as pd

    return pd.concat([pd.DataFrame(table, index=index).assign(comparison=f"{name} vs Rest", group1=name, group2="Rest") for name, table in tables])


def _first_positions(gi: np.ndarray) -> dict:
    """adata row number -> its first position within ``gi``"""
    where = {}
    for i, c in enumerate(gi.tolist()):
        where.setdefault(c, i)
    return where


def _population_positions(where: dict, idx, name: str, group: int) -> np.ndarray:
    """One population given as adata row numbers -> positions (``where``: ``_first_positions``).  ValueError for anything but integers, an
    empty population, a cell that is not in the group (naming it) and a cell listed twice."""
    arr = np.asarray(idx)
    if arr.dtype == bool or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
        raise ValueError(f"{name} must hold adata row numbers (integers), got dtype {arr.dtype}")
    arr = arr.astype(np.int64).ravel()
    if arr.size == 0:
        raise ValueError(f"{name} is empty: a population needs at least one cell")
    for c in arr.tolist():
        if c not in where:
            raise ValueError(f"{name}: cell {c} is not in group_indices_list[{group}]")
    if len(set(arr.tolist())) != arr.size:
        u, k = np.unique(arr, return_counts=True)
        raise ValueError(f"{name}: cell {int(u[k > 1][0])} is listed more than once")
    return np.array([where[c] for c in arr.tolist()], dtype=np.int64)


def de_populations(group_indices, idx1, idx2=None, group: int = 0):
    """The two populations of differential_expression as POSITIONS within ``group_indices`` (= ``group_indices_list[group]``, adata row
    numbers; position i is row i of what the read-out methods return for the group).  ``idx1`` / ``idx2``: adata row numbers;
    ``idx2=None`` takes every cell of ``group_indices`` that is not in ``idx1``.  ValueError for a cell that is not in
    ``group_indices`` (naming it), a cell listed twice, overlapping populations and an empty population."""
    gi = np.asarray(group_indices).astype(np.int64).ravel()
    where = _first_positions(gi)

    def resolve(idx, name):
        return _population_positions(where, idx, name, group)

    p1 = resolve(idx1, "idx1")
    if idx2 is None:
        rest = np.ones(len(gi), bool)
        rest[p1] = False
        rest &= np.array([where[c] == i for i, c in enumerate(gi.tolist())], dtype=bool)   # a repeated cell counts once
        p2 = np.nonzero(rest)[0].astype(np.int64)
        if p2.size == 0:
            raise ValueError(f"idx2=None leaves no cell: idx1 covers all of group_indices_list[{group}]")
        return p1, p2
    p2 = resolve(idx2, "idx2")
    both = np.intersect1d(p1, p2)
    if both.size:
        raise ValueError(f"idx1 and idx2 overlap: cell {int(gi[both[0]])} is in both populations")
    return p1, p2


def de_subsample(pos: np.ndarray, max_cells: Optional[int], seed: int) -> np.ndarray:
    """At most ``max_cells`` of a population's positions, drawn without replacement from ``default_rng(seed)``, in their original order"""
    if max_cells is None or len(pos) <= max_cells:
        return pos
    keep = np.sort(np.random.default_rng(seed).choice(len(pos), size=max_cells, replace=False))
    return pos[keep]


def de_label_populations(cell_labels, labels=None, max_cells: Optional[int] = None, seed: int = 0):
    """The bookkeeping of differential_expression_by: every label of ``cell_labels`` (one label per cell of the group, position i =
    row i of the group's read-out) against the rest.  -> (names, compared, kept, places):
      names     the label set, ``np.unique(cell_labels)`` (sorted)
      compared  the places k in ``names`` of the labels to compare, ascending: all of them, or those listed in ``labels``
                (an unknown label is a KeyError)
      kept      the positions of every cell that enters the bank, ascending: label k's cells capped by
                ``de_subsample(positions, max_cells, seed + 1 + k)``, all labels together
      places    per k in ``compared``: (p1, p2) -- where in ``kept`` the label's kept cells and the rest (the other labels' kept
                cells) are, each in position order
    Fewer than two distinct labels is a ValueError."""
    lab = np.asarray(cell_labels).ravel()
    if lab.size == 0:
        raise ValueError("groupby: the group has no cells")
    names, code = np.unique(lab, return_inverse=True)
    if len(names) < 2:
        raise ValueError(f"groupby: one label against the rest needs at least two distinct labels among the group's cells, got {names.tolist()!r}")
    if labels is None:
        compared = list(range(len(names)))
    else:
        where = {v: k for k, v in enumerate(names.tolist())}
        wanted = np.asarray(labels).ravel().tolist()
        for v in wanted:
            if v not in where:
                raise KeyError(f"labels: {v!r} is not among the labels {names.tolist()!r}")
        compared = sorted({where[v] for v in wanted})
        if not compared:
            raise ValueError("labels is empty: name at least one label to compare")
    per = [de_subsample(np.nonzero(code == k)[0].astype(np.int64), max_cells, seed + 1 + k) for k in range(len(names))]
    kept = np.sort(np.concatenate(per))
    own = np.full(lab.size, -1, dtype=np.int64)   # position -> the label whose kept cell it is
    for k, p in enumerate(per):
        own[p] = k
    own = own[kept]
    places = {k: (np.nonzero(own == k)[0].astype(np.int64), np.nonzero(own != k)[0].astype(np.int64)) for k in compared}
    return names, compared, kept, places


def de_bank_rows(index, place: np.ndarray, n_kept: int) -> np.ndarray:
    """Pair rows of ONE population -> rows of the shared bank of differential_expression_by.  Index i of a population of n_pop
    cells means draw i // n_pop, the population's (i % n_pop)-th cell in position order (the row numbering of
    differential_expression's per-population banks); that cell sits at ``place[i % n_pop]`` among the ``n_kept`` kept cells, and
    the bank's row is draw * n_kept + place.  int32."""
    i, n_pop = np.asarray(index).astype(np.int64), len(place)
    rows = (i // n_pop) * int(n_kept) + np.asarray(place)[i % n_pop]
    if rows.size and int(rows.max()) > np.iinfo(np.int32).max:
        raise ValueError("the bank has more rows than an int32 row number can address")
    return rows.astype(np.int32)


def de_pair_rows(rows_1: int, rows_2: int, n_pairs: int, seed: int = 0):
    """``n_pairs`` pairs of bank rows drawn with replacement: (r1 in [0, rows_1), r2 in [0, rows_2)) as int32 arrays, from ONE
    ``np.random.default_rng(seed)`` (r1 first, then r2)"""
    if min(int(rows_1), int(rows_2)) < 1:
        raise ValueError(f"both banks need at least one row, got {rows_1} and {rows_2}")
    if isinstance(n_pairs, bool) or not isinstance(n_pairs, (int, np.integer)) or not 1 <= int(n_pairs) <= DE_MAX_PAIRS:
        raise ValueError(f"n_pairs must be an integer between 1 and 2^24, got {n_pairs!r}")
    rng = np.random.default_rng(seed)
    r1 = rng.integers(0, int(rows_1), int(n_pairs)).astype(np.int32)
    r2 = rng.integers(0, int(rows_2), int(n_pairs)).astype(np.int32)
    return r1, r2


def de_table(stats, n_pairs: int, fdr_target: float = 0.05) -> dict:
    """The result table of differential_expression from the kernel's per-gene statistics (``stats``: mapping with "lfc_mean",
    "lfc_std", "lfc_min", "lfc_max", "count_de", "scale1", "scale2" -> arrays [n_genes]), column name -> numpy array, in column order:
    proba_de = count_de / n_pairs, proba_not_de = 1 - proba_de, bayes_factor = log(proba_de + 1e-8) - log(proba_not_de + 1e-8), the
    scales and lfc statistics as given, and ``is_de_fdr_<fdr_target>``: the largest set of genes, taken in order of decreasing
    proba_de (equal values in the order of the genes), whose mean proba_not_de -- the posterior expected false discovery rate -- is
    <= fdr_target (scvi-tools 0.20 ``differential_expression``, mode "change").  A ``stats`` that also carries "lfc_median" puts that
    column directly after ``lfc_mean`` (scvi's order); without the key the table is the one above."""
    count = np.asarray(stats["count_de"], dtype=np.float64)
    proba_de = count / float(n_pairs)
    proba_not = 1.0 - proba_de
    out = {"proba_de": proba_de, "proba_not_de": proba_not, "bayes_factor": np.log(proba_de + 1e-8) - np.log(proba_not + 1e-8)}
    for k in DE_COLUMNS[3:]:
        out[k] = np.asarray(stats[k])
        if k == "lfc_mean" and "lfc_median" in stats:
            out["lfc_median"] = np.asarray(stats["lfc_median"])
    order = np.argsort(-proba_de, kind="stable")
    fdr = np.cumsum(proba_not[order]) / (1.0 + np.arange(len(order)))
    ok = np.nonzero(fdr <= fdr_target)[0]
    is_de = np.zeros(len(order), bool)
    if ok.size:
        is_de[order[: ok[-1] + 1]] = True
    out[f"is_de_fdr_{fdr_target}"] = is_de
    return out


# ---- statistics of the observed counts (model.count_statistics): slab plan, "rest" sums and the result table ---------------------
COUNT_COLUMNS = ("raw_mean1", "raw_mean2", "non_zeros_proportion1", "non_zeros_proportion2", "raw_normalized_mean1", "raw_normalized_mean2")


def check_target_sum(target_sum) -> float:
    """``target_sum`` of count_statistics as a float: a positive finite number, else ValueError"""
    try:
        f = float(target_sum)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(target_sum, (bool, str)) or not (math.isfinite(f) and f > 0.0):
        raise ValueError(f"target_sum must be a positive finite number, got {target_sum!r}")
    return f


def count_slab_plan(seg_sizes, slab: int):
    """The slab table of spv_count_stats for a list whose first ``seg_sizes[0]`` positions are segment 0, and so on (zeros allowed):
    -> (slabs int32 [n_slabs, 3] = begin, end, segment, seg_slabs int32 [n_seg + 1]).  Every segment is cut into slabs of ``slab``
    positions, the last one shorter; no slab crosses a segment, every position lies in exactly one slab, an empty segment owns none
    (``seg_slabs[k] == seg_slabs[k + 1]``)."""
    sizes = [int(s) for s in np.asarray(seg_sizes).ravel().tolist()]
    if isinstance(slab, bool) or not isinstance(slab, (int, np.integer)) or int(slab) < 1:
        raise ValueError(f"slab must be a positive integer, got {slab!r}")
    if any(s < 0 for s in sizes):
        raise ValueError(f"seg_sizes must be non-negative, got {sizes!r}")
    if sum(sizes) > np.iinfo(np.int32).max:
        raise ValueError("the list has more positions than an int32 can address")
    slabs, seg_slabs, pos = [], [0], 0
    for k, s in enumerate(sizes):
        for b in range(pos, pos + s, int(slab)):
            slabs.append((b, min(b + int(slab), pos + s), k))
        pos += s
        seg_slabs.append(len(slabs))
    return np.asarray(slabs, dtype=np.int32).reshape(-1, 3), np.asarray(seg_slabs, dtype=np.int32)


def count_rest(stats) -> np.ndarray:
    """One-vs-rest from per-segment sums: ``stats`` fp64 [n_seg, ...] -> rest[k] = the sum of every segment but k, formed as the sum
    of the segments before k (added in ascending order) plus the sum of the segments after k (added in descending order).  Every term
    is non-negative, so nothing cancels as it would in ``total - own``; integral sums below 2^53 stay exact."""
    s = np.asarray(stats, dtype=np.float64)
    n = s.shape[0]
    before, after = np.zeros_like(s), np.zeros_like(s)
    for k in range(1, n):
        before[k] = before[k - 1] + s[k - 1]
    for k in range(n - 2, -1, -1):
        after[k] = after[k + 1] + s[k + 1]
    return before + after


def count_table(own, n_own: int, other, n_other: int) -> dict:
    """The six raw-count columns of one comparison from the kernel's sums: ``own`` / ``other`` fp64 [3, n_sel] = (sum of counts,
    number of cells with a non-zero count, sum of count * w) of the two populations of ``n_own`` / ``n_other`` cells (both positive)
    -> column name -> float64 array, in COUNT_COLUMNS order: raw_mean = S0 / n, non_zeros_proportion = S1 / n, raw_normalized_mean =
    S2 / n."""
    if int(n_own) < 1 or int(n_other) < 1:
        raise ValueError(f"both populations need at least one cell, got {n_own} and {n_other}")
    a, b = np.asarray(own, dtype=np.float64), np.asarray(other, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != 3 or b.shape != a.shape:
        raise ValueError(f"own and other must both be [3, n_sel], got {a.shape} and {b.shape}")
    n1, n2 = float(int(n_own)), float(int(n_other))
    return {"raw_mean1": a[0] / n1, "raw_mean2": b[0] / n2, "non_zeros_proportion1": a[1] / n1, "non_zeros_proportion2": b[1] / n2,
            "raw_normalized_mean1": a[2] / n1, "raw_normalized_mean2": b[2] / n2}


# ---- rank-sum test of the observed counts (model.rank_genes_groups): the result table from the kernel's integer tables -------------
RANK_COLUMNS = ("scores", "u_statistic", "auc", "pvals", "pvals_adj")


def benjamini_hochberg(pvals) -> np.ndarray:
    """Benjamini-Hochberg adjusted p-values over the finite entries of ``pvals`` (m of them): the i-th smallest becomes
    min(1, min over the i-th and every larger one of p * m / its place); a NaN stays NaN and is not counted in m"""
    p = np.asarray(pvals, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    ok = np.nonzero(np.isfinite(p))[0]
    if ok.size:
        order = ok[np.argsort(p[ok], kind="stable")]
        adj = p[order] * ok.size / (1.0 + np.arange(ok.size))
        out[order] = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    return out


def rank_test_table(rank2_k, ties, n1: int, n: int, tie_correct: bool = True) -> dict:
    """The Wilcoxon / Mann-Whitney rank-sum test of one population of ``n1`` cells against the other ``n2 = n - n1`` of a ranked list,
    per gene, from the integer tables of ``rank_ops.rank_sums``: ``rank2_k`` int64 [n_sel] = TWICE the rank sum R2 of the population
    (ties at their mean rank) and ``ties`` int64 [n_sel] = T, the sum of t^3 - t over the runs of equal keys.  In fp64, column name ->
    array, in RANK_COLUMNS order:
        u_statistic = (R2 - n1 (n1 + 1)) / 2                      the population's Mann-Whitney U
        auc         = U / (n1 n2)
        var         = n1 n2 / 12 * ((n + 1) - T / (n (n - 1)))    T = 0 with ``tie_correct=False`` (scanpy's default)
        scores      = (R2 - n1 (n + 1)) / (2 sqrt(var))           the z-score, without continuity correction
        pvals       = 2 ndtr(-|scores|) = erfc(|scores| / sqrt 2)
        pvals_adj   = ``benjamini_hochberg(pvals)`` over the selected genes
    which is ``scipy.stats.mannwhitneyu(a, b, use_continuity=False, method="asymptotic")`` in statistic and p-value.  A gene whose keys
    are all tied (var == 0) gets score 0 and p-value 1; an empty side (n1 == 0 or n1 == n) gives NaN in every column."""
    r2, T = np.asarray(rank2_k).astype(np.float64).ravel(), np.asarray(ties).astype(np.float64).ravel()
    if isinstance(n1, bool) or isinstance(n, bool) or not isinstance(n1, (int, np.integer)) or not isinstance(n, (int, np.integer)) or not 0 <= int(n1) <= int(n) or int(n) < 1:
        raise ValueError(f"n1 and n must be integers with 0 <= n1 <= n and n >= 1, got {n1!r} and {n!r}")
    if r2.shape != T.shape:
        raise ValueError(f"rank2_k and ties must have one entry per gene each, got {r2.shape} and {T.shape}")
    n1, n = int(n1), int(n)
    n2 = n - n1
    if n1 == 0 or n2 == 0:
        return {k: np.full(r2.shape, np.nan) for k in RANK_COLUMNS}
    f1, f2, fn = float(n1), float(n2), float(n)
    u = (r2 - f1 * (f1 + 1.0)) / 2.0
    var = f1 * f2 / 12.0 * ((fn + 1.0) - (T / (fn * (fn - 1.0)) if tie_correct else np.zeros_like(T)))
    flat = np.logical_not(var > 0.0)
    scores = np.where(flat, 0.0, (r2 - f1 * (fn + 1.0)) / (2.0 * np.sqrt(np.where(flat, 1.0, var))))
    pvals = torch.special.erfc(torch.from_numpy(np.abs(scores) / math.sqrt(2.0))).numpy()
    return {"scores": scores, "u_statistic": u, "auc": u / (f1 * f2), "pvals": pvals, "pvals_adj": benjamini_hochberg(pvals)}


# ---- posterior-predictive check (model.posterior_predictive_check): segment codes of a walk and the result table -----------------
PPC_STATS = ("mean", "var", "cv", "zero_fraction", "max")   # the columns ppc_table derives from a table of spv_dec_sample_stats


def check_ppc_library(library_size):
    """``library_size`` of posterior_predictive_check: "observed" -> "observed"; else what posterior_predictive_sample takes ("latent"
    or a positive finite number), returned unchanged after the same check"""
    if isinstance(library_size, str) and library_size == "observed":
        return library_size
    try:
        expression_log_library(library_size)
    except ValueError:
        raise ValueError(f"library_size must be 'latent', 'observed' or a positive number, got {library_size!r}") from None
    return library_size


def ppc_segments(cell_labels, labels=None, n_cells: Optional[int] = None, positions=None):
    """The populations of posterior_predictive_check as segment codes of a minibatch walk -> (names, sizes, seg).
    ``cell_labels``: one label per cell of the group, entry i = the cell at position i of ``group_indices_list[group]`` (row i of the
    group's read-out); None = one population "all" over ``n_cells`` cells.  ``labels``: the wanted labels, in the order the result
    lists them (an unknown label is a KeyError, a repeated one a ValueError); None = ``np.unique(cell_labels)`` (sorted).
      names  the populations, in order          sizes  how many of the group's cells each one holds
      seg    int32 code per entry of ``positions`` (walk positions: the concatenation of a group's per-step rows; None = every cell
             once, 0 .. n - 1): the place of the cell's label in ``names``, -1 for a cell of any other label, and -1 for every
             position at or beyond the group's size -- the replayed rows a read-out cuts off (``_eval_minibatches``), which would
             otherwise be counted twice."""
    if cell_labels is None:
        if labels is not None:
            raise ValueError("labels goes with groupby")
        if isinstance(n_cells, bool) or not isinstance(n_cells, (int, np.integer)) or int(n_cells) < 1:
            raise ValueError(f"n_cells must be a positive integer, got {n_cells!r}")
        n, names = int(n_cells), ["all"]
        code = np.zeros(n, dtype=np.int32)
    else:
        lab = np.asarray(cell_labels).ravel()
        n = int(lab.size)
        if n == 0:
            raise ValueError("groupby: the group has no cells")
        if n_cells is not None and int(n_cells) != n:
            raise ValueError(f"groupby: one label per cell of the group ({int(n_cells)}) is needed, got {n}")
        uniq, inv = np.unique(lab, return_inverse=True)
        known = uniq.tolist()
        names = known if labels is None else np.asarray(labels).ravel().tolist()
        if not names:
            raise ValueError("labels is empty: name at least one label")
        if len(set(names)) != len(names):
            raise ValueError(f"labels names a label more than once: {names!r}")
        where = {v: k for k, v in enumerate(known)}
        place = np.full(len(known), -1, dtype=np.int32)
        for k, v in enumerate(names):
            if v not in where:
                raise KeyError(f"labels: {v!r} is not among the labels {known!r}")
            place[where[v]] = k
        code = place[inv.ravel()]
    sizes = np.bincount(code[code >= 0], minlength=len(names)).astype(np.int64).tolist()
    if positions is None:
        return names, sizes, code
    pos = np.asarray(positions, dtype=np.int64).ravel()
    if pos.size and pos.min() < 0:
        raise ValueError("positions must not be negative")
    seg = np.full(pos.size, -1, dtype=np.int32)
    inside = pos < n
    seg[inside] = code[pos[inside]]
    return names, sizes, seg


def ppc_table(stats, counts, prefix: str = "ppc_"):
    """The per-(segment, gene) columns of posterior_predictive_check from a table of spv_dec_sample_stats -> pandas DataFrame, one row
    per (segment, column) in segment-major order, with the columns ``segment``, ``column`` and ``<prefix>`` + PPC_STATS.
    ``stats``: uint64 [n_seg, 4, n_sel] (int64 storage is read as the same bits): S = sum of x, NZ = number of x > 0, Q = sum of x^2
    modulo 2^64, M = max of x.  ``counts``: N_k = how many values segment k's entries were reduced over (cells x samples).
        mean = S / N      var = (N Q - S^2) / (N (N - 1)), NaN for N < 2      zero_fraction = (N - NZ) / N = 1 - NZ / N
        cv = sqrt(var) / mean, NaN at mean 0          (every column NaN for N < 1)
    Numerators and denominators are formed as exact Python integers and divided ONCE, so mean, var and zero_fraction are the
    correctly rounded fp64 values of the exact rationals (no cancellation between N Q and S^2 however large the counts).
    Overflow rule: where N * M^2 >= 2^64 the square sum may have wrapped; ``var`` and ``cv`` of that (segment, gene) are NaN and one
    RuntimeWarning says how many there are.  Below that bound Q < 2^64 holds, the table is exact."""
    import warnings

    import pandas as pd

    t = np.asarray(stats)
    if t.dtype == np.int64:
        t = t.view(np.uint64)
    if t.dtype != np.uint64 or t.ndim != 3 or t.shape[1] != 4:
        raise ValueError(f"stats must be a uint64 array [n_seg, 4, n_sel], got {t.dtype} {t.shape}")
    n_seg, _, n_sel = t.shape
    cnt = [int(c) for c in np.asarray(counts).ravel().tolist()]
    if len(cnt) != n_seg or any(c < 0 for c in cnt):
        raise ValueError(f"counts must hold one non-negative count per segment ({n_seg}), got {cnt!r}")
    col = {k: np.full((n_seg, n_sel), np.nan) for k in PPC_STATS}
    wrapped = 0
    for k, N in enumerate(cnt):
        if N < 1:
            continue
        S, NZ, Q, M = (t[k, j].astype(object) for j in range(4))   # Python integers from here on
        col["mean"][k] = np.asarray(S / N, dtype=np.float64)
        col["zero_fraction"][k] = np.asarray((N - NZ) / N, dtype=np.float64)
        col["max"][k] = t[k, 3].astype(np.float64)
        if N >= 2:
            safe = np.asarray(N * M * M < (1 << 64), dtype=bool)
            wrapped += int(n_sel - safe.sum())
            var = np.full(n_sel, np.nan)
            if safe.any():
                var[safe] = np.asarray((N * Q[safe] - S[safe] * S[safe]) / (N * (N - 1)), dtype=np.float64)
            col["var"][k] = var
            with np.errstate(divide="ignore", invalid="ignore"):
                col["cv"][k] = np.where(col["mean"][k] > 0, np.sqrt(var) / col["mean"][k], np.nan)
    if wrapped:
        warnings.warn(f"ppc_table: the sum of squares of {wrapped} (segment, gene) entries may have wrapped past 2^64 "
                      "(N * max^2 >= 2^64); their var and cv are NaN", RuntimeWarning, stacklevel=2)
    frame = {"segment": np.repeat(np.arange(n_seg), n_sel), "column": np.tile(np.arange(n_sel), n_seg)}
    frame.update({prefix + k: col[k].ravel() for k in PPC_STATS})
    return pd.DataFrame(frame)


def ppc_observed_columns(sums, sq, sizes):
    """The observed columns of posterior_predictive_check -> DataFrame with ``obs_`` + mean / var / cv / zero_fraction, one row per (population,
    gene), population-major, NaN where ``ppc_table`` has it.  ``sums``: fp64 [n_seg, 3, n_sel] of ``count_ops.count_stats``, ``sq``: [n_seg, n_sel] of
    ``count_ops.count_square_sums``, ``sizes``: cells per population.  Integer or whole-number sums below 2^53 go through ``ppc_table`` (exact)."""
    import pandas as pd

    n_seg, n_sel = sq.shape
    if sq.dtype == np.int64 or (np.all(sums[:, :2] == np.floor(sums[:, :2])) and np.all(sq == np.floor(sq)) and (sq.size == 0 or sq.max() < 2.0 ** 53)):
        exact = np.zeros((n_seg, 4, n_sel), dtype=np.uint64)   # whole numbers below 2^53: the exact route (no modular sum here: max row 0)
        exact[:, 0], exact[:, 1], exact[:, 2] = sums[:, 0].astype(np.uint64), sums[:, 1].astype(np.uint64), sq.astype(np.uint64)
        return ppc_table(exact, sizes, prefix="obs_")
    N = np.asarray(sizes, dtype=np.float64)[:, None]   # fractional fp32 counts: fp64 throughout
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(N > 0, sums[:, 0] / N, np.nan)
        var = np.where(N > 1, (N * sq - sums[:, 0] ** 2) / (N * (N - 1)), np.nan)
        return pd.DataFrame({"obs_mean": mean.ravel(), "obs_var": var.ravel(),
                             "obs_cv": np.where(mean > 0, np.sqrt(var) / mean, np.nan).ravel(),
                             "obs_zero_fraction": np.where(N > 0, (N - sums[:, 1]) / N, np.nan).ravel()})


def ppc_frame(names, sizes, index, obs, ppc, n_samples: int, cells, order, kept, obs_totals, ppc_totals):
    """The frame posterior_predictive_check returns: one row per (population of ``names`` / ``sizes``, gene of ``index``), population-major, with the
    columns of ``obs`` (``ppc_observed_columns``) and ``ppc`` (``ppc_table``).  ``attrs["cell_totals"]``: ``obs_total`` / ``ppc_total_mean`` per cell of
    ``cells`` (adata row numbers, the index), NaN outside every population.  ``kept``: the positions in ``cells`` of the populations' cells, ascending;
    ``order``: the same sorted by population, as ``obs_totals`` is; ``ppc_totals``: uint64 per position, summed over the ``n_samples`` samples."""
    import pandas as pd

    n_seg, n_sel = len(names), len(index)
    frame = pd.DataFrame({"population": np.repeat(np.asarray(names, dtype=object), n_sel), "gene": np.tile(np.asarray(index), n_seg),
                          "n_cells": np.repeat(np.asarray(sizes, dtype=np.int64), n_sel), "n_samples": n_samples})
    for table, prefix, stats in ((obs, "obs_", PPC_STATS[:4]), (ppc, "ppc_", PPC_STATS)):
        for c in stats:
            frame[prefix + c] = table[prefix + c].to_numpy()
    totals = np.full((2, len(cells)), np.nan)
    totals[0, order], totals[1, kept] = obs_totals, np.asarray(ppc_totals)[kept].astype(np.float64) / n_samples
    frame.attrs["cell_totals"] = pd.DataFrame({"obs_total": totals[0], "ppc_total_mean": totals[1]}, index=cells)
    return frame


# ---- expected-expression statistics (model.expression_statistics): the tile plan of a step and the result table ---------------------
EXPRESSION_STATS = ("mean", "mean_private", "mean_shared", "mixing", "private_fraction", "var", "var_private", "var_shared", "var_mixing")


def expression_tile_plan(seg, n_seg: int, tile: int = 32):
    """One minibatch's per-cell segment codes -> (perm, tile_seg, tile_n), the arrangement spv_dec_expected_stats reduces in a fixed order.
    ``seg``: one code per row of the step; a code of -1 (any negative one) or >= ``n_seg`` means the cell is not counted.
      perm      int64 row numbers, a multiple of ``tile`` long: for each segment present, in ascending order, its rows in walk order,
                the run padded to a multiple of ``tile`` by repeating the run's first row; rows that are not counted do not appear
      tile_seg  int32, one per ``tile`` rows of ``perm``: the tile's segment
      tile_n    int32, one per tile: how many of its leading rows count (``tile`` everywhere but in a run's last tile)
    A step without a counted cell gives three empty arrays: the caller skips it."""
    if isinstance(n_seg, bool) or not isinstance(n_seg, (int, np.integer)) or int(n_seg) < 1:
        raise ValueError(f"n_seg must be a positive integer, got {n_seg!r}")
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or int(tile) < 1:
        raise ValueError(f"tile must be a positive integer, got {tile!r}")
    code = np.asarray(seg).ravel()
    if code.size and not np.issubdtype(code.dtype, np.integer):
        raise TypeError("seg must hold integer segment codes")
    code, tile = code.astype(np.int64), int(tile)
    counted = (code >= 0) & (code < int(n_seg))
    perm, tile_seg, tile_n = [], [], []
    for k in np.unique(code[counted]).tolist():   # ascending
        rows = np.nonzero(code == k)[0]           # walk order
        n_tiles = -(-rows.size // tile)
        run = np.full(n_tiles * tile, rows[0], dtype=np.int64)
        run[:rows.size] = rows
        perm.append(run)
        tile_seg += [k] * n_tiles
        tile_n += [tile] * (n_tiles - 1) + [rows.size - (n_tiles - 1) * tile]
    perm = np.concatenate(perm) if perm else np.zeros(0, dtype=np.int64)
    return perm, np.asarray(tile_seg, dtype=np.int32), np.asarray(tile_n, dtype=np.int32)


def expression_stats_table(stats, counts):
    """The per-(segment, gene) columns of expression_statistics from a table of spv_dec_expected_stats -> pandas DataFrame, one row per
    (segment, column) in segment-major order, with the columns ``segment``, ``column`` and EXPRESSION_STATS, all float64.
    ``stats``: fp64 [n_seg, 8, n_sel]: rows 0..3 the sums S of the mixture mean, its private part, its shared part and the mixing
    weight, rows 4..7 the sums Q of their squares.  ``counts``: n_k = how many values segment k's entries were summed over
    (cells x samples).
        mean* / mixing = S / n, NaN for n < 1        var* = max(0, (Q - S^2 / n) / (n - 1)), NaN for n < 2
        private_fraction = S_private / S_mixture, NaN where S_mixture is 0 (and for n < 1)
    (the unbiased sample variance; the clamp removes the small negative values cancellation leaves for a constant column)."""
    import pandas as pd

    t = np.asarray(stats)
    if t.dtype != np.float64 or t.ndim != 3 or t.shape[1] != 8:
        raise ValueError(f"stats must be a float64 array [n_seg, 8, n_sel], got {t.dtype} {t.shape}")
    n_seg, _, n_sel = t.shape
    cnt = np.asarray(counts).ravel()
    if cnt.size != n_seg or (cnt.size and (not np.issubdtype(cnt.dtype, np.integer) or cnt.min() < 0)):
        raise ValueError(f"counts must hold one non-negative integer per segment ({n_seg}), got {cnt.tolist()!r}")
    n = cnt.astype(np.float64)[:, None]
    names = ("", "_private", "_shared", "_mixing")
    col = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for w, suffix in enumerate(names):
            S, Q = t[:, w], t[:, 4 + w]
            col["mixing" if w == 3 else "mean" + suffix] = np.where(n >= 1, S / n, np.nan)
            col["var" + suffix] = np.where(n >= 2, np.maximum((Q - S * S / n) / (n - 1), 0.0), np.nan)
        col["private_fraction"] = np.where((n >= 1) & (t[:, 0] != 0), t[:, 1] / t[:, 0], np.nan)
    frame = {"segment": np.repeat(np.arange(n_seg), n_sel), "column": np.tile(np.arange(n_sel), n_seg)}
    frame.update({k: col[k].ravel() for k in EXPRESSION_STATS})
    return pd.DataFrame(frame)


def expression_stats_frame(names, sizes, index, table, n_samples: int, sums=None):
    """The frame expression_statistics returns: one row per (population of ``names`` / ``sizes``, gene of ``index``), population-major, with
    ``population``, ``gene``, ``n_cells``, ``n_samples`` and the EXPRESSION_STATS columns of ``table`` (``expression_stats_table``).
    ``sums``: the fp64 table [n_seg, 8, n_sel] the columns were derived from, kept as ``attrs["sums"]``."""
    import pandas as pd

    n_seg, n_sel = len(names), len(index)
    frame = pd.DataFrame({"population": np.repeat(np.asarray(names, dtype=object), n_sel), "gene": np.tile(np.asarray(index), n_seg),
                          "n_cells": np.repeat(np.asarray(sizes, dtype=np.int64), n_sel), "n_samples": n_samples})
    for c in EXPRESSION_STATS:
        frame[c] = table[c].to_numpy()
    if sums is not None:
        frame.attrs["sums"] = np.asarray(sums)
    return frame


# ---- gene-gene correlation (model.get_feature_correlation_matrix): refusals, the counted cells and the host arithmetic -----------
CORRELATION_MAX_GENES = 4096   # SPV_GRAM_MAX_N


def check_correlation_args(correlation_type, n_sel: Optional[int] = None) -> None:
    """The refusals of ``get_feature_correlation_matrix`` that are its own, ahead of any device work: ``correlation_type`` "pearson";
    "spearman" is a NotImplementedError that names ``get_feature_spearman_matrix`` (ranks need a gene's whole column, which this
    streaming reduction never holds: Spearman is a method of its own), anything else a ValueError; more than 4096 selected genes a
    ValueError naming the table they would need."""
    if isinstance(correlation_type, str) and correlation_type == "spearman":
        raise NotImplementedError("correlation_type='spearman' is not implemented here: ranks need every value of a gene at once, and this read-out "
                                  "streams the cells through one Gram table; call get_feature_spearman_matrix (same arguments), or "
                                  "count_spearman_matrix for the observed counts")
    if not isinstance(correlation_type, str) or correlation_type != "pearson":
        raise ValueError(f"correlation_type must be 'pearson' (Spearman is get_feature_spearman_matrix, a method of its own), got {correlation_type!r}")
    if n_sel is not None and n_sel > CORRELATION_MAX_GENES:
        raise ValueError(f"{n_sel} genes selected: the fp64 table of their pairs would take n_sel^2 x 8 = {n_sel * n_sel * 8} bytes on the device; "
                         f"select at most {CORRELATION_MAX_GENES} genes (gene_list)")


def correlation_cells(group_indices, cells=None, group: int = 0) -> np.ndarray:
    """Which positions of ``group_indices`` (= ``group_indices_list[group]``) ``get_feature_correlation_matrix`` counts -> a bool mask over
    them.  ``cells``: None (every position) or adata row numbers, resolved like ``idx1`` of ``de_populations`` with its errors (named
    ``cells``): not integers, empty, a cell outside the group, a cell listed twice."""
    gi = np.asarray(group_indices).astype(np.int64).ravel()
    if cells is None:
        return np.ones(len(gi), dtype=bool)
    mask = np.zeros(len(gi), dtype=bool)
    mask[_population_positions(_first_positions(gi), cells, "cells", group)] = True
    return mask


def correlation_table(sums, gram, n) -> dict:
    """Pearson correlation from the one-pass sums of ``n`` observations, pure float64 numpy: ``sums`` S [p] = sum x_i, ``gram`` C [p, p] =
    sum x_i x_j ->
        "mean" S / n                                  "cov"  (C - S S^T / n) / (n - 1)
        "var"  the diagonal of cov, clamped at 0      "corr" cov_ij / sqrt(var_i var_j), clipped to [-1, 1]
    The diagonal of corr is exactly 1 where var > 0; corr is NaN wherever var_i or var_j is 0; mean is NaN for n < 1 and cov, var
    and corr for n < 2.  A symmetric C gives symmetric tables in bits (a * b is b * a).
    Limit of the one-pass formula ("Limits"): C - S S^T / n is the difference of two numbers of size n mean^2, each
    known to about n 2^-53 of itself, so a gene's variance -- and every correlation with it -- is lost once its relative spread
    std / |mean| falls below about 2 sqrt(n 2^-53) (4e-6 for a million cells).  Such a gene comes out with var 0 and NaN correlations
    or with noise; it is not diagnosed."""
    S, Cm = np.asarray(sums), np.asarray(gram)
    if S.dtype != np.float64 or S.ndim != 1 or Cm.dtype != np.float64 or Cm.shape != (S.shape[0], S.shape[0]):
        raise ValueError(f"sums must be a float64 vector [p] and gram a float64 matrix [p, p], got {S.dtype} {S.shape} and {Cm.dtype} {Cm.shape}")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 0:
        raise ValueError(f"n must be a non-negative integer, got {n!r}")
    n, p = int(n), S.shape[0]
    nan_v, nan_m = np.full(p, np.nan), np.full((p, p), np.nan)
    if n < 1:
        return {"mean": nan_v, "cov": nan_m, "var": nan_v.copy(), "corr": nan_m.copy()}
    mean = S / n
    if n < 2:
        return {"mean": mean, "cov": nan_m, "var": nan_v, "corr": nan_m.copy()}
    cov = (Cm - np.outer(S, S) / n) / (n - 1)
    var = np.maximum(np.diagonal(cov), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(var)
        corr = np.clip(cov / np.outer(sd, sd), -1.0, 1.0)   # (the product of the roots: var_i var_j may leave fp64's range)
    dead = var <= 0.0
    corr[dead, :] = np.nan
    corr[:, dead] = np.nan
    live = np.nonzero(~dead)[0]
    corr[live, live] = 1.0
    return {"mean": mean, "cov": cov, "var": var, "corr": corr}


# ---- Spearman correlation (model.get_feature_spearman_matrix / count_spearman_matrix): the table of the rank block's Gram ----------
SPEARMAN_EXACT_ROWS = 208063   # the largest n with n^3 < 2^53 (208063^3 = 9 007 091 372 906 047 < 2^53 = 9 007 199 254 740 992 < 208064^3)
SPEARMAN_MAX_ROWS = 1 << 20    # SPV_RANK_MAX_N
SPEARMAN_GRAM_ROWS = 16384     # rows of the rank block one spv_gram_f64 call adds


def spearman_table(gram, n) -> dict:
    """Spearman's rho from the Gram of the rank block (``rank_ops.rank_transform`` then ``gram_ops.gram_accumulate``): ``gram`` C [p, p]
    float64 with C_ij = sum over the n rows of c_i c_j, c = 2 * average rank - (n + 1).  Every column of the block sums to exactly 0,
    so the sums are not read: -> ``correlation_table(zeros, C, n)`` ("mean" 0, "cov" C / (n - 1), "var", "corr" = rho: NaN in the row
    and column of a constant gene -- its whole column is 0 --, exactly 1 on the rest of the diagonal, symmetric in bits for a symmetric
    C) plus "tie_term" = n^3 - n - 3 diag(C), the sum of t^3 - t over every gene's runs of equal values (0 for a gene without ties).
    Exactness (``SPEARMAN_EXACT_ROWS`` = 208 063): |c| <= n - 1, so every product and every partial sum of a Gram element is an
    integer of magnitude at most n (n - 1)^2 < n^3, and n^3 < 2^53 holds up to n = 208 063 (208063^3 < 2^53 < 208064^3): up to there
    C is the exact integer whatever the order of addition, and "tie_term" is exact as well (3 diag(C) <= n^3 - n).  Beyond it C carries
    fp64 summation error like any Gram."""
    Cm = np.asarray(gram)
    if Cm.dtype != np.float64 or Cm.ndim != 2 or Cm.shape[0] != Cm.shape[1]:
        raise ValueError(f"gram must be a square float64 matrix [p, p], got {Cm.dtype} {Cm.shape}")
    table = correlation_table(np.zeros(Cm.shape[0], dtype=np.float64), Cm, n)
    n = int(n)
    table["tie_term"] = float(n) ** 3 - float(n) - 3.0 * np.diagonal(Cm)
    return table


def check_spearman_shape(n_rows: int, n_sel: int, who: str) -> None:
    """The limits of the Spearman read-outs, ahead of any device work: at most 4096 genes (the fp64 table) and 2^20 ranked rows"""
    if n_sel > CORRELATION_MAX_GENES:
        raise ValueError(f"{who}: {n_sel} genes selected: the fp64 table of their pairs would take n_sel^2 x 8 = {n_sel * n_sel * 8} bytes on the "
                         f"device; select at most {CORRELATION_MAX_GENES} genes (gene_list)")
    if n_rows < 1:
        raise ValueError(f"{who}: no cell to rank")
    if n_rows > SPEARMAN_MAX_ROWS:
        raise ValueError(f"{who}: {n_rows} rows (cells x n_samples) to rank; a column sort holds at most 2^20 = {SPEARMAN_MAX_ROWS}")


# ---- neighbours in latent space (model.latent_neighbors / transfer_labels): host-side argument handling and the label vote ------
NEIGHBOR_SETS = (0, 1, "both")


def check_neighbor_args(k, query, target, latent: str):
    """The refusals of ``latent_neighbors``, ahead of any device work -> (k, query groups, target groups, exclude self?): ``k`` an integer in
    [1, KNN_KMAX]; ``query`` / ``target`` 0, 1 or "both" (group 0's cells, then group 1's); ``latent`` "shared" or "private", the latter
    only within ONE group (the two groups' private spaces are not comparable).  Self-exclusion applies when every query cell is also a
    target cell."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _abi.KNN_KMAX:
        raise ValueError(f"k must be an integer in [1, {_abi.KNN_KMAX}], got {k!r}")
    if latent not in ("shared", "private"):
        raise ValueError(f"latent must be 'shared' or 'private', got {latent!r}")
    sets = []
    for name, v in (("query", query), ("target", target)):
        if isinstance(v, bool) or not (v == "both" if isinstance(v, str) else isinstance(v, (int, np.integer)) and v in (0, 1)):
            raise ValueError(f"{name} must be 0, 1 or 'both', got {v!r}")
        sets.append((0, 1) if isinstance(v, str) else (int(v),))
    if latent == "private" and (sets[0] != sets[1] or len(sets[0]) != 1):
        raise ValueError("latent='private' needs query == target, one group: the private spaces of the two groups are not comparable")
    return int(k), sets[0], sets[1], set(sets[0]) <= set(sets[1])


def neighbor_self_positions(query_groups, target_groups, sizes) -> np.ndarray:
    """Each query cell's own position in the target cells' order (query set contained in the target set), int32 [n_query]"""
    start, off = {}, 0
    for g in target_groups:
        start[g], off = off, off + int(sizes[g])
    return np.concatenate([start[g] + np.arange(int(sizes[g]), dtype=np.int32) for g in query_groups]).astype(np.int32)


def vote_labels(indices, codes, n_labels: int):
    """Majority vote of the neighbours' labels -> (predicted int64 [n], confidence fp64 [n], n_neighbors int64 [n]).  ``indices``
    [n, k]: positions into ``codes`` (one integer label code in [0, n_labels) per source cell), -1 = no neighbour, ignored.  Uniform
    weights; ties go to the smallest code; ``confidence`` is the share of the cell's valid neighbours that voted for the winner.  A
    cell without a valid neighbour gets predicted = -1, confidence = nan."""
    idx = np.asarray(indices)
    codes = np.asarray(codes).ravel()
    if idx.ndim != 2:
        raise ValueError(f"indices must be a 2-d array [cells, k], got {idx.ndim} dimensions")
    if n_labels < 1 or (codes.size and (codes.min() < 0 or codes.max() >= n_labels)):
        raise ValueError(f"codes must lie in [0, n_labels = {n_labels})")
    valid = idx >= 0
    if (idx[valid] >= codes.shape[0]).any() or (idx < -1).any():
        raise ValueError(f"indices must be -1 or lie in [0, {codes.shape[0]})")
    n = idx.shape[0]
    votes = np.zeros((n, int(n_labels)), dtype=np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], idx.shape)
    np.add.at(votes, (rows[valid], codes[idx[valid]].astype(np.int64)), 1)
    n_valid = valid.sum(1).astype(np.int64)
    predicted = votes.argmax(1).astype(np.int64)   # the first maximum: the smallest code on ties
    with np.errstate(invalid="ignore", divide="ignore"):
        confidence = votes[np.arange(n), predicted] / n_valid.astype(np.float64)
    predicted[n_valid == 0] = -1
    confidence[n_valid == 0] = np.nan
    return predicted, confidence, n_valid


def transfer_frame(names, categories, predicted, confidence, n_valid):
    """The frame transfer_labels returns: indexed by the target cells' names; ``predicted`` (the label, None without a valid neighbour),
    ``confidence``, ``n_neighbors``"""
    import pandas as pd

    cats = np.asarray(categories, dtype=object)
    lab = np.empty(len(predicted), dtype=object)
    ok = np.asarray(predicted) >= 0
    lab[ok] = cats[np.asarray(predicted)[ok]]
    lab[~ok] = None
    return pd.DataFrame({"predicted": lab, "confidence": np.asarray(confidence, dtype=np.float64), "n_neighbors": np.asarray(n_valid, dtype=np.int64)},
                        index=pd.Index(np.asarray(names)))


# ---- transport plans from two top-k passes (ot_ops.transport_plan / model.compute_transport_plan): host-side assembly and refusals ------
def plan_union_csr(idx_rows, val_rows, idx_cols, val_cols, n0: int, n1: int):
    """The sparse plan [n0, n1] whose support is the union of two top-k passes -> CSR (indptr int64 [n0 + 1], indices int32, data fp32),
    columns ascending within a row.  ``idx_rows`` / ``val_rows`` [n0, k]: per cell i of group 0 its kept cells j of group 1 (-1 = empty
    slot) and the entries P_ij; ``idx_cols`` / ``val_cols`` [n1, k]: per cell j of group 1 its kept cells i of group 0 and P_ij.  A pair
    both passes kept takes the ROW pass's value (the two differ by rounding order only)."""
    idx_rows, idx_cols = np.asarray(idx_rows), np.asarray(idx_cols)
    val_rows, val_cols = np.asarray(val_rows, dtype=np.float32), np.asarray(val_cols, dtype=np.float32)
    n0, n1 = int(n0), int(n1)
    if idx_rows.ndim != 2 or idx_rows.shape[0] != n0 or val_rows.shape != idx_rows.shape:
        raise ValueError(f"plan_union_csr: the row pass must be two arrays [{n0}, k]")
    if idx_cols.ndim != 2 or idx_cols.shape[0] != n1 or val_cols.shape != idx_cols.shape:
        raise ValueError(f"plan_union_csr: the column pass must be two arrays [{n1}, k]")
    if (idx_rows < -1).any() or (idx_rows >= n1).any() or (idx_cols < -1).any() or (idx_cols >= n0).any():
        raise ValueError("plan_union_csr: indices must be -1 or lie inside the other group")
    keep_r, keep_c = idx_rows >= 0, idx_cols >= 0
    i_r = np.broadcast_to(np.arange(n0, dtype=np.int64)[:, None], idx_rows.shape)[keep_r]
    j_c = np.broadcast_to(np.arange(n1, dtype=np.int64)[:, None], idx_cols.shape)[keep_c]
    key_r = i_r * n1 + idx_rows[keep_r].astype(np.int64)
    key_c = idx_cols[keep_c].astype(np.int64) * n1 + j_c
    keys = np.concatenate([key_r, key_c])
    vals = np.concatenate([val_rows[keep_r], val_cols[keep_c]])
    uniq, first = np.unique(keys, return_index=True)   # `first`: the row pass's entry where both kept the pair
    indptr = np.zeros(n0 + 1, dtype=np.int64)
    np.add.at(indptr, uniq // max(n1, 1) + 1, 1)
    return np.cumsum(indptr), (uniq % max(n1, 1)).astype(np.int32), vals[first].astype(np.float32)


def check_transport_args(rep, obs_idx, k):
    """The refusals of ``compute_transport_plan`` ahead of any device work -> (X0, X1 float32 C-contiguous [n_g, D], k): ``rep``
    [n_obs, D] with 1 <= D <= OT_DMAX, finite; ``obs_idx`` the two groups' row positions; ``k`` an integer in [1, OT_KMAX]."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _abi.OT_KMAX:
        raise ValueError(f"k must be an integer in [1, {_abi.OT_KMAX}], got {k!r}")
    rep = np.asarray(rep)
    if rep.ndim != 2 or not np.issubdtype(rep.dtype, np.number):
        raise ValueError(f"use_rep must be a numeric array [n_obs, D], got shape {rep.shape}")
    if not 1 <= rep.shape[1] <= _abi.OT_DMAX:
        raise ValueError(f"use_rep must have between 1 and {_abi.OT_DMAX} columns, got {rep.shape[1]}")
    if len(obs_idx) != 2:
        raise ValueError("a transport plan couples exactly two groups")
    parts = []
    for g, rows in enumerate(obs_idx):
        rows = np.asarray(rows)
        if rows.size < 1 or rows.min() < 0 or rows.max() >= rep.shape[0]:
            raise ValueError(f"group {g}: its rows must be non-empty and lie inside use_rep's {rep.shape[0]} rows")
        part = np.ascontiguousarray(rep[rows], dtype=np.float32)
        if not np.isfinite(part).all():
            raise ValueError(f"group {g}: use_rep holds non-finite values")
        parts.append(part)
    return parts[0], parts[1], int(k)


# ---- exact t-SNE (tsne_ops.tsne / model.latent_tsne / model.tsne): refusals, the symmetric affinities as CSR, the initial layout ------
TSNE_SCHEDULE = ("early_exaggeration", "exaggeration_iter", "learning_rate", "momentum", "min_gain", "kl_every")


def tsne_neighbors(perplexity: float, n: int) -> int:
    """k = min(3 perplexity, KNN_KMAX, n - 1): the neighbours per cell the affinities rest on"""
    return max(0, min(int(3 * perplexity), _abi.KNN_KMAX, int(n) - 1))


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)


def check_tsne_args(n: int, perplexity=30.0, n_components=2, n_iter=1000, init="pca", seed=0, early_exaggeration=12.0, exaggeration_iter=250,
                    learning_rate="auto", momentum=(0.5, 0.8), min_gain=0.01, kl_every=50) -> dict:
    """The refusals of ``tsne`` / ``latent_tsne``, ahead of any device work -> the resolved settings, with ``n_neighbors`` =
    ``tsne_neighbors(perplexity, n)`` and ``learning_rate`` = max(n / early_exaggeration / 4, 50) for "auto".  ``perplexity`` must lie in
    [2, n_neighbors / 2]: the k-NN kernel returns at most 64 neighbours, so at most 32."""
    n = int(n)
    if not _number(perplexity) or perplexity < 2:
        raise ValueError(f"perplexity must be a number >= 2, got {perplexity!r}")
    k = tsne_neighbors(perplexity, n)
    if perplexity > k / 2:
        raise ValueError(f"perplexity must lie in [2, {k / 2:g}] for {n} cells: the affinities rest on k = min(3 perplexity, {_abi.KNN_KMAX}, n - 1) = {k} "
                         f"neighbours and need k >= 2 perplexity, got {perplexity!r}")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= int(n_components) <= _abi.TSNE_DMAX:
        raise ValueError(f"n_components must be an integer in [1, {_abi.TSNE_DMAX}], got {n_components!r}")
    for name, v, low in (("n_iter", n_iter, 1), ("exaggeration_iter", exaggeration_iter, 0), ("kl_every", kl_every, 1), ("seed", seed, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < low:
            raise ValueError(f"{name} must be an integer >= {low}, got {v!r}")
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError(f"init must be 'pca', 'random' or an array [n, n_components], got {init!r}")
    else:
        a = np.asarray(init)
        if a.shape != (n, int(n_components)) or not np.issubdtype(a.dtype, np.number) or not np.isfinite(a).all():
            raise ValueError(f"init: an array must be finite and of shape ({n}, {int(n_components)}), got shape {a.shape}")
    if not _number(early_exaggeration) or early_exaggeration < 1:
        raise ValueError(f"early_exaggeration must be a number >= 1, got {early_exaggeration!r}")
    if not (isinstance(learning_rate, str) and learning_rate == "auto") and (not _number(learning_rate) or learning_rate <= 0):
        raise ValueError(f"learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
    if (not isinstance(momentum, (tuple, list)) or len(momentum) != 2 or not all(_number(m) and 0 <= m < 1 for m in momentum)):
        raise ValueError(f"momentum must be two numbers in [0, 1): before and after the early exaggeration, got {momentum!r}")
    if not _number(min_gain) or min_gain <= 0:
        raise ValueError(f"min_gain must be a positive number, got {min_gain!r}")
    lr = max(n / float(early_exaggeration) / 4.0, 50.0) if isinstance(learning_rate, str) else float(learning_rate)
    return {"perplexity": float(perplexity), "n_neighbors": k, "n_components": int(n_components), "n_iter": int(n_iter), "seed": int(seed),
            "early_exaggeration": float(early_exaggeration), "exaggeration_iter": int(exaggeration_iter), "learning_rate": lr,
            "momentum": (float(momentum[0]), float(momentum[1])), "min_gain": float(min_gain), "kl_every": int(kl_every)}


def check_tsne_schedule(schedule: dict) -> dict:
    """``**schedule`` of ``latent_tsne`` / ``spVIPES.tsne``: only the names of ``TSNE_SCHEDULE``"""
    unknown = sorted(set(schedule) - set(TSNE_SCHEDULE))
    if unknown:
        raise ValueError(f"unknown schedule argument(s) {unknown}: the schedule takes {list(TSNE_SCHEDULE)}")
    return dict(schedule)


def check_tsne_rep(rep, n_obs: Optional[int] = None) -> np.ndarray:
    """``use_rep`` of ``spVIPES.tsne`` -> float32 C-contiguous [n_obs, D], 1 <= D <= KNN_DMAX, finite"""
    rep = np.asarray(rep)
    if rep.ndim != 2 or not np.issubdtype(rep.dtype, np.number):
        raise ValueError(f"use_rep must be a numeric array [n_obs, D], got shape {rep.shape}")
    if n_obs is not None and rep.shape[0] != n_obs:
        raise ValueError(f"use_rep must have one row per cell ({n_obs}), got {rep.shape[0]}")
    if not 1 <= rep.shape[1] <= _abi.KNN_DMAX:
        raise ValueError(f"use_rep must have between 1 and {_abi.KNN_DMAX} columns, got {rep.shape[1]}")
    rep = np.ascontiguousarray(rep, dtype=np.float32)
    if not np.isfinite(rep).all():
        raise ValueError("use_rep holds non-finite values")
    return rep


def tsne_symmetrize(idx, P, n: int):
    """The joint affinities P = (P_cond + P_cond^T) / 2n as CSR (indptr int64 [n + 1], cols int32 ascending within a row, vals fp32) from
    the conditional ones: ``idx`` int [n, k] each cell's neighbours (-1 = empty slot), ``P`` [n, k] their conditional affinities.  A pair
    either cell lists is an entry; the sums are formed in fp64 and rounded once.  With rows of ``P`` summing to 1 the entries sum to 1."""
    idx, P, n = np.asarray(idx), np.asarray(P, dtype=np.float64), int(n)
    if idx.ndim != 2 or idx.shape[0] != n or P.shape != idx.shape:
        raise ValueError(f"tsne_symmetrize: idx and P must be two arrays [{n}, k]")
    if (idx < -1).any() or (idx >= n).any():
        raise ValueError("tsne_symmetrize: indices must be -1 or lie in [0, n)")
    keep = idx >= 0
    i = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], idx.shape)[keep]
    j = idx[keep].astype(np.int64)
    keys = np.concatenate([i * n + j, j * n + i])
    uniq, inverse = np.unique(keys, return_inverse=True)
    vals = np.bincount(inverse.ravel(), weights=np.concatenate([P[keep], P[keep]]), minlength=len(uniq)) / (2.0 * n)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(indptr, uniq // max(n, 1) + 1, 1)
    return np.cumsum(indptr), (uniq % max(n, 1)).astype(np.int32), vals.astype(np.float32)


def tsne_pca_layout(X, n_components: int) -> np.ndarray:
    """The "pca" initial layout, float32 [n, n_components]: the rows of ``X`` centred and projected, in fp64, on the eigenvectors of their
    covariance with the largest eigenvalues, each eigenvector's sign fixed so that its entry of largest magnitude (the first on ties) is
    positive, the whole scaled so that the first column's standard deviation is 1e-4 (scikit-learn's scaling).  When X has fewer columns
    than ``n_components`` the missing ones are zero."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0, keepdims=True)
    vals, vecs = np.linalg.eigh(Xc.T @ Xc / max(X.shape[0] - 1, 1))
    V = vecs[:, np.argsort(-vals, kind="stable")[:n_components]]
    lead = np.abs(V).argmax(axis=0)
    V = V * np.where(V[lead, np.arange(V.shape[1])] < 0, -1.0, 1.0)[None, :]
    Y = np.zeros((X.shape[0], n_components), dtype=np.float64)
    Y[:, :V.shape[1]] = Xc @ V
    sd = Y[:, 0].std()
    return (Y / sd * 1e-4 if sd > 0 else Y).astype(np.float32)


def tsne_initial_layout(init, X, n: int, n_components: int, seed: int) -> np.ndarray:
    """float32 C-contiguous [n, n_components]: ``tsne_pca_layout(X)``, seeded normal draws scaled by 1e-4, or the given array"""
    if isinstance(init, str) and init == "pca":
        return np.ascontiguousarray(tsne_pca_layout(X, n_components))
    if isinstance(init, str):
        return np.ascontiguousarray((np.random.default_rng(seed).standard_normal((n, n_components)) * 1e-4).astype(np.float32))
    return np.ascontiguousarray(np.asarray(init), dtype=np.float32)


def tsne_frame(names, group_of_cell, result, perplexity: float):
    """The frame ``latent_tsne`` returns: one row per cell, indexed by ``names``, with ``group`` and ``tsne_1`` .. ``tsne_n``; ``attrs``
    holds ``kl_divergence``, ``kl_history``, ``perplexity`` and ``n_neighbors``."""
    import pandas as pd

    cols = {"group": np.asarray(group_of_cell).astype(np.int64)}
    for t in range(result.embedding.shape[1]):
        cols[f"tsne_{t + 1}"] = result.embedding[:, t]
    frame = pd.DataFrame(cols, index=pd.Index(np.asarray(names)))
    frame.attrs.update(kl_divergence=result.kl_divergence, kl_history=result.kl_history, perplexity=float(perplexity), n_neighbors=result.n_neighbors)
    return frame


# ---- silhouette widths in latent space (model.latent_silhouette / integration_scores): host-side arrangement, the per-cell values from
# the kernel's exact sums, and the scores -- pure numpy ------
SILHOUETTE_MAX_LABELS = _abi.SIL_SEG_MAX // 2   # two segments (group 0, group 1) per label


def check_silhouette_args(cells, latent: str):
    """The refusals of ``latent_silhouette``, ahead of any device work -> the groups of ``cells``: 0, 1 or "both" (group 0's cells, then
    group 1's); ``latent`` "shared" or "private", the latter only with ONE group (the two groups' private spaces are not comparable)."""
    if latent not in ("shared", "private"):
        raise ValueError(f"latent must be 'shared' or 'private', got {latent!r}")
    if isinstance(cells, bool) or not (cells == "both" if isinstance(cells, str) else isinstance(cells, (int, np.integer)) and cells in (0, 1)):
        raise ValueError(f"cells must be 0, 1 or 'both', got {cells!r}")
    groups = (0, 1) if isinstance(cells, str) else (int(cells),)
    if latent == "private" and len(groups) != 1:
        raise ValueError("latent='private' needs cells 0 or 1: the private spaces of the two groups are not comparable")
    return groups


def silhouette_segments(label_codes, group_of_cell, n_labels: int):
    """The arrangement of the cells by (label, group) the kernel's candidates need -> (perm int64 [n]: the cells in segment order, each
    segment's cells in their given order; seg_ptr int32 [2 * n_labels + 1]; sizes int64 [2 * n_labels]).  Segment 2 * t + g holds the
    cells of label code t in group g: group 0 then group 1 within each label; a segment without a cell is empty, not left out."""
    codes, grp = np.asarray(label_codes).ravel().astype(np.int64), np.asarray(group_of_cell).ravel().astype(np.int64)
    n_labels = int(n_labels)
    if codes.shape != grp.shape:
        raise ValueError(f"one label code and one group per cell, got {codes.shape[0]} and {grp.shape[0]}")
    if not 1 <= n_labels <= SILHOUETTE_MAX_LABELS:
        raise ValueError(f"the number of labels must lie in [1, {SILHOUETTE_MAX_LABELS}], got {n_labels}")
    if codes.size and (codes.min() < 0 or codes.max() >= n_labels):
        raise ValueError(f"label codes must lie in [0, n_labels = {n_labels})")
    if grp.size and (grp.min() < 0 or grp.max() > 1):
        raise ValueError("group_of_cell must hold 0 or 1")
    seg = 2 * codes + grp
    perm = np.argsort(seg, kind="stable").astype(np.int64)
    sizes = np.bincount(seg, minlength=2 * n_labels).astype(np.int64)
    seg_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return perm, seg_ptr, sizes


def _silhouette_width(a, b, single):
    """(b - a) / max(a, b), 0 where ``single`` (the cell is alone in its cluster) or max(a, b) = 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.maximum(a, b)
        s = (b - a) / m
    s = np.where(m == 0, 0.0, s)
    return np.where(single, 0.0, s)


def silhouette_table(S, sizes, label_codes, group_of_cell) -> dict:
    """The per-cell silhouette values, in fp64, from the exact distance sums.  ``S`` [n, 2 * n_labels]: cell i's summed distance to
    the cells of each (label, group) segment, ``sizes`` the segments' cell counts (``silhouette_segments``' order), ``label_codes`` /
    ``group_of_cell`` [n] the cells' own.  Returns arrays [n]:
      a, b, silhouette_label   the label silhouette (sklearn's ``silhouette_samples``): with n_t the cells of the cell's label t in both
                               groups, a = S_t / (n_t - 1) (its own distance is +0), b = min over the labels u != t that have cells of
                               S_u / n_u, s = (b - a) / max(a, b); s = 0 and a = NaN for the only cell of a label; s = 0 where
                               max(a, b) = 0; b = s = NaN when no other label has a cell
      nearest_label            the code u that gives b, the smallest on ties; -1 when there is none
      silhouette_group         the same width inside the cell's label with its own group g as the cluster and the other group as the
                               neighbour: a = S_{t,g} / (n_{t,g} - 1), b = S_{t,1-g} / n_{t,1-g}; 0 for the only cell of (t, g); NaN for a
                               label that has cells in one group only"""
    S = np.asarray(S, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.int64).ravel()
    codes, grp = np.asarray(label_codes).ravel().astype(np.int64), np.asarray(group_of_cell).ravel().astype(np.int64)
    n, L = codes.shape[0], sizes.shape[0] // 2
    if S.shape != (n, 2 * L) or sizes.shape[0] != 2 * L or grp.shape[0] != n:
        raise ValueError(f"S must be [cells, 2 * n_labels] = [{n}, {2 * L}], got {S.shape}")
    rows = np.arange(n)
    S_lab, n_lab = S[:, 0::2] + S[:, 1::2], sizes[0::2] + sizes[1::2]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = S_lab[rows, codes] / (n_lab[codes] - 1).astype(np.float64)
        mean_to = S_lab / n_lab.astype(np.float64)[None, :]
    a = np.where(n_lab[codes] == 1, np.nan, a)
    mean_to = np.where((n_lab > 0)[None, :], mean_to, np.inf)
    mean_to[rows, codes] = np.inf
    nearest = mean_to.argmin(axis=1) if L else np.zeros(n, dtype=np.int64)
    b = mean_to[rows, nearest] if n else np.zeros(0)
    none = ~(b < np.inf) & ~np.isnan(b)
    b = np.where(none, np.nan, b)
    nearest = np.where(none, -1, nearest).astype(np.int64)
    s = _silhouette_width(a, b, n_lab[codes] == 1)
    s = np.where(none, np.nan, s)

    n_own, n_oth = sizes[2 * codes + grp], sizes[2 * codes + 1 - grp]
    with np.errstate(invalid="ignore", divide="ignore"):
        a_g = S[rows, 2 * codes + grp] / (n_own - 1).astype(np.float64)
        b_g = S[rows, 2 * codes + 1 - grp] / n_oth.astype(np.float64)
    s_g = _silhouette_width(a_g, b_g, n_own == 1)
    s_g = np.where(n_oth > 0, s_g, np.nan)
    return {"a": a, "b": b, "silhouette_label": s, "nearest_label": nearest, "silhouette_group": s_g}


def silhouette_scores(table: dict, sizes, label_codes) -> dict:
    """scIB's two scores and their per-label parts from ``silhouette_table``'s columns ->
    {"label_asw": (mean_i s_i + 1) / 2 over all cells; "group_asw": the mean, over the labels with cells in both groups, of
    mean_i (1 - |s_g,i|) over the label's cells (NaN without such a label); "label_mean" / "group_mean" [n_labels]: each label's mean
    label silhouette and its 1 - |s_g| mean (NaN for a label without cells / not in both groups)}"""
    sizes = np.asarray(sizes, dtype=np.int64).ravel()
    codes = np.asarray(label_codes).ravel().astype(np.int64)
    L = sizes.shape[0] // 2
    s, s_g = np.asarray(table["silhouette_label"], dtype=np.float64), np.asarray(table["silhouette_group"], dtype=np.float64)
    label_mean, group_mean = np.full(L, np.nan), np.full(L, np.nan)
    for t in range(L):
        own = codes == t
        if own.any():
            label_mean[t] = s[own].mean()
            if sizes[2 * t] > 0 and sizes[2 * t + 1] > 0:
                group_mean[t] = (1.0 - np.abs(s_g[own])).mean()
    both = ~np.isnan(group_mean)
    return {"label_asw": float((s.mean() + 1.0) / 2.0) if s.size else float("nan"),
            "group_asw": float(group_mean[both].mean()) if both.any() else float("nan"), "label_mean": label_mean, "group_mean": group_mean}


def silhouette_frame(names, group_of_cell, categories, label_codes, sizes, table: dict):
    """The frame ``latent_silhouette`` returns: one row per cell, indexed by ``names``, with ``group``, ``label``, ``silhouette_label``,
    ``a``, ``b``, ``nearest_label`` (None when there is no other label), ``silhouette_group``; ``attrs`` holds ``label_asw``,
    ``group_asw`` and ``per_label``: indexed by the labels, ``n_group0`` / ``n_group1`` (cells), ``silhouette_label`` (its cells' mean) and
    ``group_mixing`` (their 1 - |silhouette_group| mean)."""
    import pandas as pd

    cats = np.asarray(categories, dtype=object)
    codes = np.asarray(label_codes).ravel().astype(np.int64)
    sizes = np.asarray(sizes, dtype=np.int64).ravel()
    near = np.empty(len(codes), dtype=object)
    ok = np.asarray(table["nearest_label"]) >= 0
    near[ok] = cats[np.asarray(table["nearest_label"])[ok]]
    near[~ok] = None
    frame = pd.DataFrame({"group": np.asarray(group_of_cell).astype(np.int64), "label": cats[codes], "silhouette_label": table["silhouette_label"],
                          "a": table["a"], "b": table["b"], "nearest_label": near, "silhouette_group": table["silhouette_group"]},
                         index=pd.Index(np.asarray(names)))
    sc = silhouette_scores(table, sizes, codes)
    frame.attrs["label_asw"], frame.attrs["group_asw"] = sc["label_asw"], sc["group_asw"]
    frame.attrs["per_label"] = pd.DataFrame({"n_group0": sizes[0::2], "n_group1": sizes[1::2], "silhouette_label": sc["label_mean"],
                                             "group_mixing": sc["group_mean"]}, index=pd.Index(cats))
    return frame


def silhouette_query_blocks(n: int, row_bytes: int, cap_bytes: int):
    """[(first, end)] blocks of the n query cells such that a block x ``row_bytes`` (what one query costs in table and workspace) stays
    within ``cap_bytes``; at least one cell per block"""
    rows = max(1, int(cap_bytes) // max(1, int(row_bytes)))
    return [(b, min(b + rows, int(n))) for b in range(0, int(n), rows)]


# ---- LISI in latent space (model.latent_lisi / spVIPES.lisi): the refusals, the frames and scIB's scaling -- pure numpy ------
def lisi_neighbors(perplexity: float, n: int) -> int:
    """k = min(int(3 perplexity) - 1, n - 1): the neighbours per cell LISI rests on, the cell itself left out (89 at perplexity 30)"""
    return min(int(3 * perplexity) - 1, int(n) - 1)


def check_lisi_args(n: int, perplexity=30.0) -> int:
    """The refusals of ``latent_lisi`` / ``spVIPES.lisi`` about the perplexity, ahead of any device work -> k = ``lisi_neighbors``:
    ``perplexity`` a finite number >= 1 that gives 1 <= k <= 256 (the most the paged k-NN returns) for ``n`` cells"""
    if not _number(perplexity) or not np.isfinite(perplexity) or perplexity < 1:
        raise ValueError(f"perplexity must be a finite number >= 1, got {perplexity!r}")
    k = lisi_neighbors(perplexity, n)
    if not 1 <= k <= _abi.KNN_PAGED_KMAX:
        raise ValueError(f"perplexity {perplexity!r} and {int(n)} cells give k = min(int(3 perplexity) - 1, n - 1) = {k} neighbours per cell: "
                         f"k must lie in [1, {_abi.KNN_PAGED_KMAX}]")
    return k


def _nanmedian(v) -> float:
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(np.median(v)) if v.size else float("nan")


def lisi_scaled(median: float, n: int, kind: str) -> float:
    """scIB's scaling of a median LISI to [0, 1], larger is better: ``kind`` "ilisi": (median - 1) / (n - 1) over n groups; "clisi":
    (n - median) / (n - 1) over n labels; NaN for n < 2"""
    if kind not in ("ilisi", "clisi"):
        raise ValueError(f"kind must be 'ilisi' or 'clisi', got {kind!r}")
    if int(n) < 2:
        return float("nan")
    return float((median - 1.0) / (n - 1.0) if kind == "ilisi" else (n - median) / (n - 1.0))


def lisi_frame(names, group_of_cell, categories, label_codes, ilisi, clisi, n_valid, converged, perplexity: float, k: int):
    """The frame ``latent_lisi`` returns: one row per cell, indexed by ``names``, with ``group``, ``label`` (None without labels),
    ``ilisi`` (``None``: the selection holds one group, a NaN column), ``clisi`` (left out when ``clisi`` is None), ``n_neighbors`` and
    ``converged``.  ``attrs``: ``ilisi_median`` / ``clisi_median`` (nan-medians), ``ilisi_scaled`` = (median - 1) / (n_groups - 1) and
    ``clisi_scaled`` = (n_labels - median) / (n_labels - 1) (scIB's scaling; NaN with one group / one label; the clisi entries are left
    out without labels), ``per_label`` (indexed by the labels: ``n_group0`` / ``n_group1`` cells, median ``ilisi``, median ``clisi``;
    None without labels), ``perplexity``, ``n_neighbors`` (= k) and ``n_unconverged``."""
    import pandas as pd

    grp = np.asarray(group_of_cell).ravel().astype(np.int64)
    n = grp.shape[0]
    n_groups = len(np.unique(grp))
    il = np.full(n, np.nan) if ilisi is None or n_groups < 2 else np.asarray(ilisi, dtype=np.float64).ravel()
    n_valid, converged = np.asarray(n_valid).ravel().astype(np.int64), np.asarray(converged).ravel().astype(bool)
    if il.shape[0] != n or n_valid.shape[0] != n or converged.shape[0] != n:
        raise ValueError(f"one value per cell ({n}) of ilisi, n_valid and converged")
    cols = {"group": grp}
    if clisi is None:
        cols["label"] = np.full(n, None, dtype=object)
    else:
        cats, codes = np.asarray(categories, dtype=object), np.asarray(label_codes).ravel().astype(np.int64)
        cl = np.asarray(clisi, dtype=np.float64).ravel()
        if codes.shape[0] != n or cl.shape[0] != n:
            raise ValueError(f"one value per cell ({n}) of the label codes and clisi")
        cols["label"] = cats[codes]
    cols["ilisi"] = il
    if clisi is not None:
        cols["clisi"] = cl
    cols["n_neighbors"], cols["converged"] = n_valid, converged
    frame = pd.DataFrame(cols, index=pd.Index(np.asarray(names)))
    frame.attrs["ilisi_median"] = _nanmedian(il)
    frame.attrs["ilisi_scaled"] = lisi_scaled(frame.attrs["ilisi_median"], n_groups, "ilisi")
    frame.attrs["per_label"] = None
    if clisi is not None:
        frame.attrs["clisi_median"] = _nanmedian(cl)
        frame.attrs["clisi_scaled"] = lisi_scaled(frame.attrs["clisi_median"], len(cats), "clisi")
        frame.attrs["per_label"] = pd.DataFrame({"n_group0": [int(((codes == t) & (grp == 0)).sum()) for t in range(len(cats))],
                                                 "n_group1": [int(((codes == t) & (grp == 1)).sum()) for t in range(len(cats))],
                                                 "ilisi": [_nanmedian(il[codes == t]) for t in range(len(cats))],
                                                 "clisi": [_nanmedian(cl[codes == t]) for t in range(len(cats))]}, index=pd.Index(cats))
    frame.attrs.update(perplexity=float(perplexity), n_neighbors=int(k), n_unconverged=int((~converged).sum()))
    return frame


def check_lisi_keys(obs, keys, n_obs: int):
    """``keys`` of ``spVIPES.lisi`` -> [(key, categories, codes int32 [n_obs])]: one or more column names of ``obs`` (KeyError for an
    unknown one, ValueError for none, a repeated one or a column of another length)"""
    keys = [keys] if isinstance(keys, str) else list(keys)
    if not keys or not all(isinstance(key, str) for key in keys) or len(set(keys)) != len(keys):
        raise ValueError(f"keys must be one or more distinct obs column names, got {keys!r}")
    out = []
    for key in keys:
        if key not in obs:
            raise KeyError(f"keys: adata.obs has no column {key!r}")
        col = np.asarray(obs[key]).ravel()
        if col.shape[0] != int(n_obs):
            raise ValueError(f"obs[{key!r}] must hold one entry per cell ({int(n_obs)}), got {col.shape[0]}")
        cats, codes = np.unique(col, return_inverse=True)
        out.append((key, cats, codes.astype(np.int32)))
    return out


def lisi_rep_frame(names, keyed, lisi, n_valid, converged, perplexity: float, k: int):
    """The frame ``spVIPES.lisi`` returns: one row per cell, indexed by ``names``, a ``lisi_<key>`` column per entry of ``keyed``
    (``check_lisi_keys``; ``lisi`` [len(keyed), n_obs]), ``n_neighbors`` and ``converged``.  ``attrs``: ``lisi_<key>_median`` (nan-median)
    and ``n_<key>`` (its distinct values) per key, ``perplexity``, ``n_neighbors`` (= k) and ``n_unconverged``."""
    import pandas as pd

    lisi = np.asarray(lisi, dtype=np.float64)
    converged = np.asarray(converged).ravel().astype(bool)
    if lisi.ndim != 2 or lisi.shape[0] != len(keyed):
        raise ValueError(f"lisi must be [keys, cells] = [{len(keyed)}, n], got {lisi.shape}")
    cols = {f"lisi_{key}": lisi[t] for t, (key, _cats, _codes) in enumerate(keyed)}
    cols["n_neighbors"], cols["converged"] = np.asarray(n_valid).ravel().astype(np.int64), converged
    frame = pd.DataFrame(cols, index=pd.Index(np.asarray(names)))
    for t, (key, cats, _codes) in enumerate(keyed):
        frame.attrs[f"lisi_{key}_median"], frame.attrs[f"n_{key}"] = _nanmedian(lisi[t]), len(cats)
    frame.attrs.update(perplexity=float(perplexity), n_neighbors=int(k), n_unconverged=int((~converged).sum()))
    return frame


# ---- cluster matching across the two groups from a transport plan (model.match_transport_clusters): k-means seeding, the entropy
# criterion that chooses a clustering, the block scores and the Hungarian matching that names the clusters -- pure numpy / scipy ------
def kmeans_pp_init(X, K: int, seed: int) -> np.ndarray:
    """k-means++ seeding on the host in fp64 -> ``K`` DISTINCT rows of ``X`` [n, D] (in X's dtype), a function of (X, K, seed) alone.
    The first row is drawn uniformly, every further one with probability proportional to its squared distance to the nearest row
    chosen so far: a row equal to a chosen one has probability 0.  Fewer than K distinct rows: ValueError."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError(f"kmeans_pp_init: X must be an array [n >= 1, D], got shape {X.shape}")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= X.shape[0]:
        raise ValueError(f"kmeans_pp_init: K must be an integer in [1, n = {X.shape[0]}], got {K!r}")
    rng = np.random.default_rng(int(seed))
    X64 = X.astype(np.float64)
    chosen = [int(rng.integers(X.shape[0]))]
    d2 = ((X64 - X64[chosen[0]]) ** 2).sum(1)
    for _ in range(int(K) - 1):
        cum = np.cumsum(d2)
        if not cum[-1] > 0:
            raise ValueError(f"kmeans_pp_init: X holds fewer than K = {K} distinct rows")
        pick = min(int(np.searchsorted(cum, rng.random() * cum[-1], side="right")), X.shape[0] - 1)
        while d2[pick] == 0:   # the draw landed on the end of the cumulative sum's range: the last row with weight
            pick -= 1
        chosen.append(pick)
        d2 = np.minimum(d2, ((X64 - X64[pick]) ** 2).sum(1))
    return X[np.array(chosen)].copy()


def kmeans_update(X64: np.ndarray, labels: np.ndarray, d2: np.ndarray, K: int) -> np.ndarray:
    """The centroid step of ``cluster_ops.kmeans`` -> fp32 [K, D]: per cluster the fp64 sum of its cells' rows in ascending cell order
    (``np.bincount`` with weights), divided by the count, rounded to fp32.  A cluster without a cell takes the ROW of the cell with the
    largest current squared distance ``d2`` (the smaller index on ties); several such clusters, in ascending order, take the largest,
    the next largest, ...: a cell serves once.  The cell stays in its old cluster's mean; the next assignment moves it."""
    counts = np.bincount(labels, minlength=K)
    sums = np.stack([np.bincount(labels, weights=X64[:, t], minlength=K) for t in range(X64.shape[1])], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cent = (sums / counts[:, None]).astype(np.float32)
    left = np.asarray(d2, dtype=np.float64).copy()
    for c in np.flatnonzero(counts == 0):
        cell = int(np.argmax(left))
        cent[c] = X64[cell].astype(np.float32)
        left[cell] = -np.inf
    return cent


def cluster_segments(labels, K: int):
    """The arrangement of one group's cells by cluster the segment kernel's candidates need -> (perm int64 [n]: the cells in cluster
    order, each cluster's cells in their given order (a stable sort); seg_ptr int32 [K + 1]; sizes int64 [K])"""
    labels = np.asarray(labels).ravel().astype(np.int64)
    K = int(K)
    if not 1 <= K <= _abi.OT_SEG_MAX:
        raise ValueError(f"the number of clusters must lie in [1, {_abi.OT_SEG_MAX}], got {K}")
    if labels.size and (labels.min() < 0 or labels.max() >= K):
        raise ValueError(f"cluster labels must lie in [0, K = {K})")
    sizes = np.bincount(labels, minlength=K).astype(np.int64)
    return np.argsort(labels, kind="stable").astype(np.int64), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), sizes


def cluster_entropy_score(logT) -> float:
    """The reference's criterion for a clustering of one group (process_transport_plan, model/spvipes.py:55-67) from the LOG masses
    ``logT`` [K, n_other] (log of the plan's mass between cluster c and cell i of the other group): every cluster's row normalised over
    the other group's cells, its natural-log entropy, and MINUS the mean over the clusters -- higher is better.  All in fp64 through
    the row's maximum, so nothing underflows: H = log Z - sum_i p_i (l_i - m) / Z with p_i = exp(l_i - m), Z = sum_i p_i.  A cluster
    without any mass (every entry -inf; the reference divides 0 by 0 there) counts as the uniform distribution, ln(n_other): the least
    informative a cluster can be, so a clustering gains nothing from having one."""
    logT = np.asarray(logT, dtype=np.float64)
    if logT.ndim != 2 or logT.shape[0] < 1 or logT.shape[1] < 1 or np.isnan(logT).any() or np.isposinf(logT).any():
        raise ValueError("cluster_entropy_score: logT must be an array [K >= 1, n >= 1] of finite values or -inf")
    m = logT.max(1)
    live = np.isfinite(m)
    H = np.full(logT.shape[0], np.log(logT.shape[1]))
    if live.any():
        d = logT[live] - m[live, None]   # <= 0, -inf where there is no mass
        p = np.exp(d)
        Z = p.sum(1)
        H[live] = np.log(Z) - np.where(p > 0, p * np.where(p > 0, d, 0.0), 0.0).sum(1) / Z
    return float(-H.mean())


def cluster_pair_scores(logT1, labels0, sizes1, K0: Optional[int] = None):
    """The plan's mass between the clusters of the two groups -> (M fp64 [K0, K1], score fp64 [K0, K1]).  ``logT1`` [K1, n0]: the log
    mass between cluster c1 of group 1 and cell i of group 0; ``labels0`` [n0]: the cells' clusters in group 0; ``sizes1`` [K1]: the
    cells per cluster of group 1.  M[c0, c1] = the fp64 sum over the cells i of c0, in ascending order, of exp(logT1[c1, i]);
    score = M / (n_c0 n_c1), the MEAN plan entry of the block (0 for a block with an empty side)."""
    logT1 = np.asarray(logT1, dtype=np.float64)
    labels0 = np.asarray(labels0).ravel().astype(np.int64)
    sizes1 = np.asarray(sizes1).ravel().astype(np.int64)
    if logT1.ndim != 2 or logT1.shape[1] != labels0.shape[0] or sizes1.shape[0] != logT1.shape[0]:
        raise ValueError("cluster_pair_scores: logT1 must be [K1, n0] with one label per column and one size per row")
    K0 = int(labels0.max()) + 1 if K0 is None else int(K0)
    if labels0.size and (labels0.min() < 0 or labels0.max() >= K0):
        raise ValueError(f"cluster_pair_scores: labels0 must lie in [0, K0 = {K0})")
    T = np.exp(logT1)
    M = np.stack([np.bincount(labels0, weights=T[c1], minlength=K0) for c1 in range(T.shape[0])], axis=1)
    cells = np.bincount(labels0, minlength=K0)[:, None] * sizes1[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return M, np.where(cells > 0, M / cells, 0.0)


def match_cluster_labels(score) -> dict:
    """Names for the clusters of both groups from the block scores ``score`` [K0, K1] (higher = more plan mass per pair of cells):
    ``scipy.optimize.linear_sum_assignment(-score)``, the matched pairs named ``Cluster_0 ..`` in ``row_ind`` order (model/spvipes.py
    :126-135), then every unmatched cluster -- there are |K0 - K1| -- its OWN further ``Cluster_m``, ascending in (group, cluster)
    order.  -> {"names": ([K0 names], [K1 names]), "row_ind", "col_ind"}.  Deterministic: a function of ``score`` alone."""
    from scipy.optimize import linear_sum_assignment

    score = np.asarray(score, dtype=np.float64)
    if score.ndim != 2 or score.shape[0] < 1 or score.shape[1] < 1 or not np.isfinite(score).all():
        raise ValueError("match_cluster_labels: score must be a finite array [K0 >= 1, K1 >= 1]")
    row_ind, col_ind = linear_sum_assignment(-score)
    names = ([None] * score.shape[0], [None] * score.shape[1])
    for m, (r, c) in enumerate(zip(row_ind, col_ind)):
        names[0][int(r)] = names[1][int(c)] = f"Cluster_{m}"
    m = len(row_ind)
    for g in range(2):
        for c in range(len(names[g])):
            if names[g][c] is None:
                names[g][c] = f"Cluster_{m}"
                m += 1
    return {"names": names, "row_ind": np.asarray(row_ind, dtype=np.int64), "col_ind": np.asarray(col_ind, dtype=np.int64)}


def cluster_tables_from_matrix(plan, labels0, K0: int, labels1, K1: int):
    """The two tables of log masses from a plain matrix plan [n0, n1] (dense array or scipy sparse), on the host in fp64 by products
    with one-hot cluster matrices -> (logT0 [K0, n1]: cluster of group 0 x cell of group 1; logT1 [K1, n0]: cluster of group 1 x cell
    of group 0); a zero mass becomes -inf.  NaN entries count as 0, as the reference's ``nan_to_num`` (:44)."""
    import scipy.sparse as sp

    labels0, labels1 = np.asarray(labels0).ravel().astype(np.int64), np.asarray(labels1).ravel().astype(np.int64)
    n0, n1 = labels0.shape[0], labels1.shape[0]
    if tuple(plan.shape) != (n0, n1):
        raise ValueError(f"the plan must be [n0, n1] = [{n0}, {n1}], got {tuple(plan.shape)}")
    one0 = sp.csr_matrix((np.ones(n0), (labels0, np.arange(n0))), shape=(int(K0), n0))   # [K0, n0]
    one1 = sp.csr_matrix((np.ones(n1), (np.arange(n1), labels1)), shape=(n1, int(K1)))   # [n1, K1]
    if sp.issparse(plan):
        P = plan.astype(np.float64).tocsr()
        P.data = np.nan_to_num(P.data, nan=0.0)
        T0, T1 = np.asarray((one0 @ P).todense()), np.asarray((P @ one1).todense()).T
    else:
        P = np.nan_to_num(np.asarray(plan, dtype=np.float64), nan=0.0)
        T0, T1 = np.asarray(one0 @ P), np.asarray((one1.T @ P.T))
    if (T0 < 0).any() or (T1 < 0).any() or not np.isfinite(T0).all():
        raise ValueError("the plan must hold finite non-negative entries")
    with np.errstate(divide="ignore"):
        return np.log(T0), np.log(T1)


@dataclass
class ClusterMatching:
    """What ``match_transport_clusters`` returns and, as a dict without ``labels``, writes to ``uns["cluster_matching"]``:
    ``n_clusters`` (K0, K1) chosen; ``candidates``: the K swept, or None; ``criterion``: per group {K: cluster_entropy_score};
    ``mass`` / ``score`` fp64 [K0, K1]: the plan's mass per block and the mean entry per block; ``row_ind`` / ``col_ind``: the
    assignment (cluster row_ind[m] of group 0 with cluster col_ind[m] of group 1 is ``Cluster_m``); ``names``: per group the new name
    of every cluster; ``cluster_values``: per group what a cluster is called in ``group_cluster_labels`` (k-means index or the
    ``cluster_key`` value); ``labels``: per group the cells' cluster index int64 [n_g]."""
    n_clusters: tuple
    candidates: Optional[tuple]
    criterion: list
    mass: np.ndarray
    score: np.ndarray
    row_ind: np.ndarray
    col_ind: np.ndarray
    names: tuple
    labels: list
    cluster_values: list

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k in ("n_clusters", "candidates", "criterion", "mass", "score", "row_ind", "col_ind", "names", "cluster_values")}


def check_match_clusters_args(adata, rep, plan, n_clusters, cluster_key, n_init, seed):
    """The refusals of ``match_transport_clusters`` ahead of any device work and of anything written -> (obs_idx, candidates: a tuple
    of K per group or None with ``cluster_key``, swept: whether the criterion chooses).  ``rep``: the representation [n_obs, D] or
    None (not needed with a matrix plan and ``cluster_key``)."""
    if "groups_obs_indices" not in adata.uns:
        raise ValueError("adata.uns['groups_obs_indices'] missing: build the AnnData with prepare_adatas (or the same schema)")
    obs_idx = [np.asarray(v) for v in adata.uns["groups_obs_indices"]]
    if len(obs_idx) != 2:
        raise ValueError("cluster matching couples exactly two groups")
    if any(len(v) < 1 for v in obs_idx):
        raise ValueError("both groups need at least one cell")
    if plan is not None and tuple(getattr(plan, "shape", ())) != (len(obs_idx[0]), len(obs_idx[1])):
        raise ValueError(f"plan must be a TransportPlan or a matrix [n0, n1] = [{len(obs_idx[0])}, {len(obs_idx[1])}], "
                         f"got shape {tuple(getattr(plan, 'shape', ()))}")
    for name, v in (("n_init", n_init), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or (name == "n_init" and int(v) < 1) or int(v) < 0:
            raise ValueError(f"{name} must be a {'positive' if name == 'n_init' else 'non-negative'} integer, got {v!r}")
    if cluster_key is not None:
        if cluster_key not in adata.obs:
            raise KeyError(f"cluster_key '{cluster_key}' not found in adata.obs")
        col = np.asarray(adata.obs[cluster_key])
        for g, rows in enumerate(obs_idx):
            if len(np.unique(col[rows])) > _abi.OT_SEG_MAX:
                raise ValueError(f"group {g}: cluster_key holds more than {_abi.OT_SEG_MAX} clusters")
        return obs_idx, None, False
    if rep is None:
        raise ValueError("use_rep is needed unless cluster_key names the clusters")
    swept = not isinstance(n_clusters, (int, np.integer))
    try:
        cand = tuple(n_clusters) if swept else (n_clusters,)
    except TypeError:
        cand = ()
    if not cand or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= int(c) <= _abi.OT_SEG_MAX for c in cand):
        raise ValueError(f"n_clusters must be an integer or a non-empty sequence of integers in [1, {_abi.OT_SEG_MAX}], got {n_clusters!r}")
    cand = tuple(int(c) for c in cand)
    for g, rows in enumerate(obs_idx):
        if not any(c <= len(rows) for c in cand):
            raise ValueError(f"group {g}: every candidate of n_clusters exceeds its {len(rows)} cells")
    return obs_idx, cand, swept


# ---- barycentric projection through the transport plan (model.transport_project): the refusals, the one-hot encoding of a label
# column and the frame a label projection comes back as -- pure numpy / pandas ------
def one_hot_labels(col):
    """An ``obs`` column's values for some cells -> (categories: the sorted distinct values, one-hot float32 [n, n_categories])"""
    cats, inv = np.unique(np.asarray(col), return_inverse=True)
    hot = np.zeros((len(inv), len(cats)), dtype=np.float32)
    hot[np.arange(len(inv)), inv] = 1.0
    return cats, hot


def label_projection_frame(probs, categories, index):
    """The projection of one-hot labels [n, n_categories] -> pandas DataFrame indexed by ``index``: one probability column per category
    (named str(category)), ``predicted`` (the category with the largest probability, the FIRST one on ties; None for a row of NaN: a
    cell the plan gives no mass) and ``confidence`` (that probability)."""
    import pandas as pd

    probs = np.asarray(probs)
    categories = np.asarray(categories)
    if probs.ndim != 2 or probs.shape[1] != len(categories) or len(index) != probs.shape[0]:
        raise ValueError("label_projection_frame: probs must be [len(index), len(categories)]")
    frame = pd.DataFrame(probs, index=index, columns=[str(c) for c in categories])
    none = np.isnan(probs).any(1)
    best = np.argmax(np.where(none[:, None], 0.0, probs), axis=1)   # argmax: the first of equal entries
    predicted = categories[best].astype(object)
    predicted[none] = None
    frame["predicted"] = predicted
    frame["confidence"] = np.where(none, np.nan, probs[np.arange(len(best)), best])
    return frame


def check_transport_project_args(adata, rep, plan, values, onto, key_added):
    """The refusals of ``transport_project`` ahead of any device work and of anything written -> (obs_idx, X0, X1 float32 [n_g, D],
    V float32 C-contiguous [n_other, n_v], categories or None).  ``rep``: the representation [n_obs, D]; ``values``: an array
    [n_other, n_v] or [n_obs, n_v], a key of ``obsm`` or the name of an ``obs`` column (then ``categories`` are its distinct values
    among the other group's cells and V their one-hot encoding)."""
    if "groups_obs_indices" not in adata.uns:
        raise ValueError("adata.uns['groups_obs_indices'] missing: build the AnnData with prepare_adatas (or the same schema)")
    obs_idx = [np.asarray(v) for v in adata.uns["groups_obs_indices"]]
    if len(obs_idx) != 2:
        raise ValueError("a transport plan couples exactly two groups")
    if isinstance(onto, bool) or not isinstance(onto, (int, np.integer)) or int(onto) not in (0, 1):
        raise ValueError(f"onto must be 0 or 1, the group whose cells receive the projection, got {onto!r}")
    if key_added is not None and not isinstance(key_added, str):
        raise ValueError(f"key_added must be a string or None, got {key_added!r}")
    if not hasattr(plan, "sinkhorn"):
        raise TypeError("plan must be the TransportPlan of compute_transport_plan: a plain matrix has no potentials, and the projection "
                        "reads the untruncated plan from them.  The host route for a matrix is plan.to_scipy() @ values (or plan @ values), "
                        "divided by the row sums")
    n = (len(obs_idx[0]), len(obs_idx[1]))
    if tuple(plan.shape) != n:
        raise ValueError(f"plan couples {tuple(plan.shape)} cells, the groups hold {n}")
    X0, X1, _ = check_transport_args(rep, obs_idx, 1)
    other = obs_idx[1 - int(onto)]
    categories = None
    if isinstance(values, str):
        obsm = getattr(adata, "obsm", None)
        if obsm is not None and values in obsm:
            values = obsm[values]
        elif values in adata.obs:
            categories, values = one_hot_labels(np.asarray(adata.obs[values])[other])
        else:
            raise KeyError(f"values '{values}' is neither a key of adata.obsm nor a column of adata.obs")
    V = np.asarray(values)
    if V.ndim != 2 or V.shape[1] < 1 or not (np.issubdtype(V.dtype, np.number) or V.dtype == bool):
        raise ValueError(f"values must be a numeric array [n_other, n_v] or [n_obs, n_v] with n_v >= 1, got shape {V.shape}")
    if V.shape[0] == adata.n_obs:
        V = V[other]
    elif V.shape[0] != len(other):
        raise ValueError(f"values must have one row per cell of group {1 - int(onto)} ({len(other)}) or per cell of adata ({adata.n_obs}), "
                         f"got {V.shape[0]}")
    with np.errstate(over="ignore"):
        V = np.ascontiguousarray(V, dtype=np.float32)
    if not np.isfinite(V).all():
        raise ValueError("values holds non-finite entries (after the conversion to float32)")
    return obs_idx, X0, X1, V, categories


# ---- PCA of the log-normalised counts (model.count_pca / spVIPES.pca): the resident counts, the pairing, the argument checks, the sign rule ----
PCA_MAX_COMPS = 56       # n_comps, at most: the block is min(64, round_up(n_comps + 8, 16)) columns and the kernels take 64
PCA_MIN_GENES = 16       # paired genes, at least: the smallest block the kernels take


def resident_group_counts(X, obs_idx, var_idx, device, counts_storage: str = "auto"):
    """The per-group count matrices resident in HBM, as the model's constructor keeps them: rows = the group's cells (obs order),
    columns = its own genes.  ``counts_storage``: "dense", "sparse" (CSR) or "auto" (CSR for a scipy.sparse ``X``, else dense); a
    scipy.sparse input is never densified as a whole (csr_group_arrays works on its stored entries)."""
    sparse_in = is_sparse(X)
    if (counts_storage == "sparse") or (counts_storage == "auto" and sparse_in):
        return [to_sparse_group_counts(X, obs_idx[g], var_idx[g], device) for g in range(2)]
    if sparse_in:   # "dense" storage of a sparse input: one group's slice at a time
        return [to_group_counts(csr_to_dense(*csr_group_arrays(X, obs_idx[g], var_idx[g])[:3], len(var_idx[g])), device) for g in range(2)]
    X = np.asarray(X)
    return [to_group_counts(X[obs_idx[g]][:, var_idx[g]], device) for g in range(2)]


def check_pca_args(n_comps, tol=1e-4, seed=0, n_cells: Optional[int] = None, n_genes: Optional[int] = None):
    """The argument checks of count_pca -> (n_comps, tol, seed) as plain numbers; every refusal is a ValueError with the limit in it"""
    if isinstance(n_comps, bool) or not isinstance(n_comps, (int, np.integer)) or not 1 <= int(n_comps) <= PCA_MAX_COMPS:
        raise ValueError(f"n_comps must be an integer between 1 and {PCA_MAX_COMPS}, got {n_comps!r}")
    try:
        t = float(tol)
    except (TypeError, ValueError):
        t = float("nan")
    if isinstance(tol, (bool, str)) or not (math.isfinite(t) and 0.0 < t < 1.0):
        raise ValueError(f"tol must be a number in (0, 1), got {tol!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= SAMPLE_MAX_SEED:
        raise ValueError(f"seed must be an integer in [0, 2^32), got {seed!r}")
    n_comps = int(n_comps)
    if n_cells is not None and n_cells < 2:
        raise ValueError(f"count_pca needs at least 2 cells, got {n_cells}")
    if n_genes is not None and n_genes < PCA_MIN_GENES:
        raise ValueError(f"count_pca needs at least {PCA_MIN_GENES} genes (the smallest block of the kernels), got {n_genes}")
    for what, m in (("cells", n_cells), ("genes", n_genes)):
        if m is not None and n_comps >= m:
            raise ValueError(f"n_comps must be smaller than the number of {what} ({m}), got {n_comps}")
    if n_genes is not None and (n_comps + 15) // 16 * 16 > n_genes:
        raise ValueError(f"n_comps={n_comps} needs an iteration block of {(n_comps + 15) // 16 * 16} columns (a multiple of 16), and a block cannot "
                         f"be wider than the number of genes ({n_genes}): at most n_comps={n_genes // 16 * 16} with these genes")
    return n_comps, t, int(seed)


def pca_block(n_comps: int, n_genes: Optional[int] = None) -> int:
    """The block of block_lanczos: min(64, round_up(n_comps + 8, 16)) by default; with fewer genes than that, the largest multiple of
    16 the genes allow (a block cannot be wider than the operator).  It is at least round_up(n_comps, 16) wherever ``check_pca_args``
    has accepted (n_comps, n_genes)."""
    b = min(64, (int(n_comps) + 8 + 15) // 16 * 16)
    return b if n_genes is None else min(b, int(n_genes) // 16 * 16)


def pca_group_keys(uns, n_groups: int = 2):
    """the group keys of ``uns["groups_mapping"]`` (prepare_adatas: {position: key}; a list is taken as it is), or None"""
    gm = uns.get("groups_mapping") if hasattr(uns, "get") else None
    if gm is None:
        return None
    if isinstance(gm, dict):
        keys = [gm[k] if k in gm else list(gm.values())[k] for k in range(n_groups)] if len(gm) >= n_groups else None
    else:
        keys = list(gm)[:n_groups] if len(gm) >= n_groups else None
    return None if keys is None else [str(k) for k in keys]


def pca_pair_genes(names, keys=None, gene_list=None, n_genes=None):
    """The PAIRED genes of the joint PCA -> (pos0 int32 [p], pos1 int32 [p], labels [p]): column t of the joint matrix is gene pos0[t]
    of group 0 and gene pos1[t] of group 1.
    Default: every group's names (``group_var_names``) lose the prefix ``"<group key>_"`` that prepare_adatas adds (``keys``: the
    group keys, None = nothing is stripped; a name without the prefix stays as it is); the pairing keeps the names BOTH groups have, in
    group 0's order (the first occurrence of a repeated name).  ``gene_list=[names0, names1]`` (names or positions, as
    ``resolve_gene_list`` takes them) pairs BY POSITION: equal lengths, no repeats.  Without names and without ``gene_list`` there is
    nothing to pair by: a ValueError that says so -- nothing is guessed."""
    if gene_list is not None:
        sel = resolve_gene_list(gene_list, n_genes, names)
        if sel[0] is None or sel[1] is None:
            raise ValueError("gene_list of the joint PCA must name BOTH groups' genes: [names0, names1], paired by position")
        if len(sel[0]) != len(sel[1]):
            raise ValueError(f"gene_list pairs by position: the two lists must have equal length, got {len(sel[0])} and {len(sel[1])}")
        for g in range(2):
            if len(np.unique(sel[g])) != len(sel[g]):
                raise ValueError(f"gene_list[{g}] repeats a gene: a paired gene is one column of the joint matrix")
        labels = np.asarray(names[0])[sel[0]] if names is not None and names[0] is not None else np.asarray(sel[0])
        return sel[0].astype(np.int32), sel[1].astype(np.int32), labels
    if names is None or names[0] is None or names[1] is None:
        raise ValueError("the joint PCA pairs the groups' genes by name, and this AnnData carries neither var_names nor uns['groups_var_names']: "
                         "pass gene_list=[names0, names1] (positions paired by position), or group=g for one group's own PCA")
    stripped = []
    for g in range(2):
        pre = None if keys is None else keys[g] + "_"
        stripped.append([s[len(pre):] if pre and s.startswith(pre) else s for s in np.asarray(names[g]).astype(str)])
    first1 = {}
    for i, s in enumerate(stripped[1]):
        first1.setdefault(s, i)
    pos0, pos1, labels, seen = [], [], [], set()
    for i, s in enumerate(stripped[0]):
        if s in first1 and s not in seen:
            seen.add(s)
            pos0.append(i), pos1.append(first1[s]), labels.append(s)
    if not pos0:
        raise ValueError("the two groups share no gene name (after the '<group key>_' prefixes are stripped): pass gene_list=[names0, names1]")
    return np.asarray(pos0, np.int32), np.asarray(pos1, np.int32), np.asarray(labels)


def pca_sign_flip(components: np.ndarray) -> np.ndarray:
    """The sign rule of count_pca: +1 / -1 per component (row of ``components`` [n_comps, p]) such that its largest |loading| becomes
    positive; ties go to the smaller gene index; an all-zero row keeps +1"""
    c = np.asarray(components, np.float64)
    at = np.argmax(np.abs(c), axis=1)   # (the first of equal maxima)
    lead = c[np.arange(c.shape[0]), at]
    return np.where(lead < 0, -1.0, 1.0)


@dataclass
class PcaResult:
    """What count_pca returns.  ``scores`` fp32 [cells, n_comps]; ``components`` fp64 [n_comps, p] (the fp32 vectors the scores were
    made with); ``genes``: per group the paired names (positions without names), or the one group's; ``mean`` / ``var`` fp64 [p] of the
    log-normalised values (ddof 1); ``variance`` = theta / (n - 1); ``variance_ratio`` against the total variance from the moments;
    ``residuals``: || X^T X v - theta v || of the returned vectors; ``n_blocks`` / ``n_restarts`` / ``converged``: the iteration's
    record; ``obs``: the adata rows of the scores' rows"""
    scores: np.ndarray
    components: np.ndarray
    genes: list
    mean: np.ndarray
    var: np.ndarray
    variance: np.ndarray
    variance_ratio: np.ndarray
    residuals: np.ndarray
    n_blocks: int
    n_restarts: int
    converged: bool
    obs: np.ndarray
    theta: Optional[np.ndarray] = None
    params: Optional[dict] = None


def pca_plan(adata, n_genes, obs_idx, group_indices_list, n_comps=50, group=None, gene_list=None, normalize=True, target_sum=1e4, scale=False,
             tol=1e-4, seed=0) -> dict:
    """Everything count_pca decides on the host, every refusal included, ahead of any device work -> dict of ``groups`` (the group
    numbers whose cells are stacked), ``cols`` (per such group the int32 positions of the joint columns among its genes), ``genes``
    (per such group the columns' names, positions without names), ``rows`` (per such group the rows of its resident matrix),
    ``obs`` (the adata rows of the stacked cells), ``params``.  ``n_genes``: the groups' gene counts; ``obs_idx``: their adata rows."""
    target_sum = check_target_sum(target_sum)
    for what, v in (("normalize", normalize), ("scale", scale)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{what} must be True or False, got {v!r}")
    names = group_var_names(adata)
    if group is None:
        gs = [0, 1]
        pos0, pos1, _labels = pca_pair_genes(names, pca_group_keys(adata.uns), gene_list, n_genes)
        cols = [pos0, pos1]
    else:
        g = check_group(group)
        gs = [g]
        sel = resolve_gene_list(gene_list, n_genes, names)[g]
        if sel is None:
            sel = np.arange(n_genes[g], dtype=np.int32)
        elif len(np.unique(sel)) != len(sel):
            raise ValueError(f"gene_list[{g}] repeats a gene: a gene is one column of the PCA")
        cols = [np.asarray(sel, np.int32)]
    if not hasattr(group_indices_list, "__len__") or len(group_indices_list) != 2:
        raise ValueError("group_indices_list must hold one list of adata row numbers per group (2)")
    rows, obs = [], []
    for g in gs:
        listed = np.asarray(group_indices_list[g]).astype(np.int64).ravel()
        if listed.size and (listed.min() < 0 or listed.max() >= adata.n_obs):
            raise ValueError(f"group_indices_list[{g}] must hold adata row numbers in [0, {adata.n_obs})")
        pos = np.full(adata.n_obs, -1, dtype=np.int64)
        pos[np.asarray(obs_idx[g])] = np.arange(len(obs_idx[g]))
        loc = pos[listed]
        if (loc < 0).any():
            raise ValueError(f"group_indices_list[{g}] contains cells that do not belong to group {g}")
        rows.append(loc.astype(np.int32))
        obs.append(listed)
    if any(len(r) == 0 for r in rows):
        raise ValueError("count_pca: every group that takes part needs at least one listed cell")
    n_comps, tol, seed = check_pca_args(n_comps, tol, seed, n_cells=sum(len(r) for r in rows), n_genes=len(cols[0]))
    genes = [np.asarray(c) if names[g] is None else np.asarray(names[g])[c] for g, c in zip(gs, cols)]
    params = dict(n_comps=n_comps, group=group, normalize=bool(normalize), target_sum=target_sum, scale=bool(scale), tol=tol, seed=seed,
                  block=pca_block(n_comps, len(cols[0])), n_genes=len(cols[0]))
    return dict(groups=gs, cols=cols, genes=genes, rows=rows, obs=np.concatenate(obs), params=params)


def check_pca_adata(adata, layer=None, counts_storage="auto", key_added="X_pca", kwargs=None):
    """The refusals of spVIPES.pca that concern the AnnData and its own arguments -> the count matrix (``adata.X`` or the layer)"""
    for k in ("groups_var_indices", "groups_obs_indices"):
        if k not in adata.uns:
            raise ValueError(f"adata.uns['{k}'] missing: build the AnnData with prepare_adatas (or the same schema)")
    if counts_storage not in ("auto", "dense", "sparse"):
        raise ValueError(f"counts_storage must be 'auto', 'dense' or 'sparse', got {counts_storage!r}")
    if not isinstance(key_added, str) or not key_added:
        raise ValueError(f"key_added must be a non-empty string, got {key_added!r}")
    allowed = ("gene_list", "normalize", "target_sum", "scale", "tol", "seed")
    for k in (kwargs or {}):
        if k not in allowed:
            raise ValueError(f"spVIPES.pca takes the keyword arguments {allowed} of count_pca (the joint PCA over every cell), got {k!r}")
    if layer is not None:
        layers = getattr(adata, "layers", None)
        if layers is None or layer not in layers:
            raise KeyError(f"layer '{layer}' not found in adata.layers")
        return layers[layer]
    return adata.X
