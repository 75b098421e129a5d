"""scvi-tools-style user surface of the MI355X hot path: ``setup_anndata`` / ``train`` /
``get_latent_representation`` / ``get_loadings`` / ``save(dir)`` / ``load(dir, adata=...)``.

Mirrors /root/reference/src/spVIPES/model/spvipes.py (class ``spVIPES``: ctor :216-283,
``setup_anndata`` :285-422, ``get_latent_representation`` :424-650, ``get_loadings`` :652-677) and
model/base/training_mixin.py (``train`` :19-123).  anndata / scvi-tools / Lightning are not part of
this build: the AnnData object is duck-typed (``.X`` dense array or scipy.sparse matrix, ``.obs`` mapping of columns,
``.uns`` dict, ``.n_obs``) and ``prepare_adatas``' output schema is the input contract --
``uns["groups_lengths" | "groups_var_indices" | "groups_obs_indices" | ...]``, ``obs["groups"]``,
``obs["indices"]`` (data/prepare_adatas.py:97-132).

``process_transport_plan`` (:26-162, scanpy Leiden + Hungarian matching) has its counterpart in ``match_transport_clusters``:
k-means (or the user's own clusters) in place of Leiden, the plan's cluster masses from a fused kernel, the same matching; it writes
the ``obs["processed_transport_labels"]`` that cluster matching reads.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _abi
from .data import (check_tsne_args, check_tsne_rep, check_tsne_schedule, tsne_frame, MinibatchSampler, RowBlocks, check_de_args, check_neighbor_args, check_transport_args, neighbor_self_positions, transfer_frame, vote_labels, check_expression_args, check_group, check_ppc_library, check_sample_args, check_target_sum, count_rest, count_table,
                   de_bank_rows, de_label_populations, de_pair_rows, de_populations, de_subsample, de_table, expression_stats_frame, expression_stats_table, expression_tile_plan, format_latent_results, group_cell_labels, group_var_names, is_sparse,
                   latent_loader_mode, latent_steps, ppc_frame, ppc_observed_columns, ppc_segments, ppc_table, resolve_gene_list, vs_rest_frames, walk_positions,
                   ClusterMatching, check_match_clusters_args, cluster_entropy_score, cluster_pair_scores, cluster_tables_from_matrix, match_cluster_labels,
                   check_transport_project_args, label_projection_frame,
                   SILHOUETTE_MAX_LABELS, check_silhouette_args, silhouette_frame, silhouette_query_blocks, silhouette_segments, silhouette_table,
                   check_lisi_args, check_lisi_keys, lisi_frame, lisi_rep_frame,
                   check_correlation_args, correlation_cells, correlation_table)
from .data import PcaResult, check_pca_adata, pca_plan, resident_group_counts
from .data import SPEARMAN_EXACT_ROWS, SPEARMAN_GRAM_ROWS, check_spearman_shape, spearman_table
from .module import spVIPESmodule
from .plan import SparsePlan
from .train import Trainer, default_max_epochs

_SETUP_KEY = "_spvipes_amd_setup"


def _codes(column) -> np.ndarray:
    """Categorical codes the way scvi's CategoricalObsField produces them (sorted unique values)."""
    arr = np.asarray(column)
    _, inv = np.unique(arr, return_inverse=True)
    return inv.astype(np.float32)


def _run_count_pca(counts, plan: dict, device) -> PcaResult:
    """the device half of count_pca / pca: ``plan`` is ``data.pca_plan``'s"""
    from .pca_ops import count_pca
    q = plan["params"]
    groups = [(counts[g], torch.as_tensor(r, dtype=torch.int32, device=device)) for g, r in zip(plan["groups"], plan["rows"])]
    out = count_pca(groups, plan["cols"], q["n_comps"], normalize=q["normalize"], target_sum=q["target_sum"], scale=q["scale"], tol=q["tol"],
                    seed=q["seed"], block=q["block"])
    return PcaResult(scores=out["scores"].cpu().numpy(), components=out["components"], genes=plan["genes"], mean=out["mean"], var=out["var"],
                     variance=out["variance"], variance_ratio=out["variance_ratio"], residuals=out["residuals"], n_blocks=out["n_blocks"],
                     n_restarts=out["n_restarts"], converged=out["converged"], obs=plan["obs"], theta=out["theta"], params=q)


class spVIPES:
    """Shared-private VAE with Product-of-Experts integration, HIP-accelerated.  Constructor arguments as
    the reference (:216-224); ``precision`` ("bf16" | "fp32"), ``device`` and ``counts_storage`` are this build's additions.
    ``counts_storage``: how the count matrices stay in HBM -- "dense" (uint16 / float32 cells x genes), "sparse" (CSR; every step
    densifies only its minibatch, bit-identical results) or "auto" (CSR for a scipy.sparse ``adata.X`` / layer, else dense)."""

    def __init__(self, adata, n_hidden: int = 128, n_dimensions_shared: int = 25, n_dimensions_private: int = 10,
                 dropout_rate: float = 0.1, precision: str = "bf16", device: Optional[str] = None, counts_storage: str = "auto",
                 **model_kwargs):
        if _SETUP_KEY not in adata.uns:
            raise ValueError("Please run `spVIPES.setup_anndata(adata, groups_key=...)` before creating the model")
        if counts_storage not in ("auto", "dense", "sparse"):
            raise ValueError(f"counts_storage must be 'auto', 'dense' or 'sparse', got {counts_storage!r}")
        if not torch.cuda.is_available():
            raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
        _abi.load()
        self.adata = adata
        self.device = torch.device(device or "cuda:0")
        self.n_dimensions_private, self.n_dimensions_shared = n_dimensions_private, n_dimensions_shared
        setup = adata.uns[_SETUP_KEY]
        self._setup = setup
        groups_lengths = adata.uns["groups_lengths"]
        var_idx = [np.asarray(v) for v in adata.uns["groups_var_indices"]]
        self.obs_idx = [np.asarray(v) for v in adata.uns["groups_obs_indices"]]
        plan_key = setup.get("transport_plan_key")
        transport_plan = None
        if plan_key:
            if adata.uns.get(plan_key) is None:
                raise ValueError(f"Transport plan not found in adata.uns['{plan_key}']")
            transport_plan = adata.uns[plan_key]
            if not (is_sparse(transport_plan) or isinstance(transport_plan, SparsePlan)):   # a sparse plan goes to the module as it is, never densified
                transport_plan = torch.tensor(np.asarray(transport_plan), dtype=torch.float32, device=self.device)
        pair_data = "processed_transport_labels" not in adata.obs  # :249
        use_labels = setup.get("label_key") is not None  # :251
        # batch covariates (setup_anndata(batch_key=...): CategoricalObsField(BATCH_KEY), :358; n_batch = its number of categories, :230):
        # integer codes over the WHOLE AnnData; without a batch_key scvi registers one dummy category, i.e. no covariate column
        batch_codes = _codes(adata.obs[setup["batch_key"]]) if setup.get("batch_key") else None
        n_batch = int(batch_codes.max()) + 1 if batch_codes is not None and len(batch_codes) else 1
        # the decoder kernels' operand layout: the narrow one wherever it fits (every shape the narrow layout takes builds exactly that),
        # the wide one for more covariate categories; kept in init_params_ below, so load() rebuilds the same layout
        model_kwargs.setdefault("decoder_slots", "auto")
        self.module = spVIPESmodule(
            groups_lengths=groups_lengths, groups_obs_names=adata.uns.get("groups_obs_names"),
            groups_var_names=adata.uns.get("groups_var_names"), groups_var_indices=var_idx, groups_obs_indices=self.obs_idx,
            transport_plan=transport_plan, pair_data=pair_data, use_labels=use_labels,
            n_labels=(len(np.unique(np.asarray(adata.obs[setup["label_key"]]))) if use_labels else None), n_batch=n_batch,
            n_hidden=n_hidden, n_dimensions_shared=n_dimensions_shared, n_dimensions_private=n_dimensions_private,
            dropout_rate=dropout_rate, precision=precision, **model_kwargs,
        ).to(self.device)
        # resident per-group count matrices: rows = the group's cells (obs order), columns = its own genes (data.resident_group_counts,
        # which spVIPES.pca shares)
        X = adata.X if setup.get("layer") is None else adata.layers[setup["layer"]]
        self.counts = resident_group_counts(X, self.obs_idx, var_idx, self.device, counts_storage)
        obs = adata.obs
        self._labels = [torch.tensor(_codes(obs[setup["label_key"]])[self.obs_idx[g]], device=self.device) for g in range(2)] if use_labels else None
        self._components = ([torch.tensor(_codes(obs["processed_transport_labels"])[self.obs_idx[g]], device=self.device) for g in range(2)]
                            if (transport_plan is not None and not pair_data) else None)
        self._plan_indices = [torch.tensor(np.asarray(obs["indices"])[self.obs_idx[g]].astype(np.float32), device=self.device) for g in range(2)]
        self._batch = ([torch.tensor(np.asarray(batch_codes)[self.obs_idx[g]].astype(np.int32), device=self.device) for g in range(2)]
                       if n_batch > 1 else None)
        self.is_trained_ = False
        self.history: Dict[str, List[float]] = {}
        # what load() re-creates the model from (scvi's BaseModelClass keeps the same record: _get_init_params(locals()), :281)
        self.init_params_ = dict(n_hidden=n_hidden, n_dimensions_shared=n_dimensions_shared, n_dimensions_private=n_dimensions_private,
                                 dropout_rate=dropout_rate, precision=precision, device=str(self.device), counts_storage=counts_storage,
                                 **model_kwargs)

    # ------------------------------------------------------------------------------------------
    @classmethod
    def setup_anndata(cls, adata, groups_key: str, match_clusters: bool = False, transport_plan_key: Optional[str] = None,
                      label_key: Optional[str] = None, batch_key: Optional[str] = None, layer: Optional[str] = None, **kwargs) -> None:
        """Registers the fields the model reads (:355-422).  Same arguments, priorities and errors."""
        if batch_key is not None and batch_key not in adata.obs:
            raise KeyError(f"batch_key '{batch_key}' not found in adata.obs")
        if groups_key not in adata.obs:
            raise KeyError(f"groups_key '{groups_key}' not found in adata.obs")
        if transport_plan_key is not None:
            if transport_plan_key not in adata.uns:
                raise ValueError(f"Transport plan key '{transport_plan_key}' not found in adata.uns")
            adata.uns["transport_plan"] = adata.uns[transport_plan_key]
            if match_clusters and "processed_transport_labels" not in adata.obs:
                raise NotImplementedError(
                    "match_clusters=True needs obs['processed_transport_labels']: run spVIPES.match_transport_clusters(adata, ...) "
                    "first (the counterpart of the reference's process_transport_plan), or write the column yourself")
            if "indices" not in adata.obs:
                raise ValueError("'indices' must be present in adata.obs when using a transport plan")
        if label_key is not None and label_key not in adata.obs:
            raise KeyError(f"label_key '{label_key}' not found in adata.obs")
        for k in ("groups_lengths", "groups_var_indices", "groups_obs_indices"):
            if k not in adata.uns:
                raise ValueError(f"adata.uns['{k}'] missing: build the AnnData with prepare_adatas (or the same schema)")
        adata.uns[_SETUP_KEY] = {"groups_key": groups_key, "match_clusters": match_clusters, "transport_plan_key": transport_plan_key,
                                 "label_key": label_key, "batch_key": batch_key, "layer": layer}

    @classmethod
    def compute_transport_plan(cls, adata, use_rep, k: int = 32, key_added: str = "transport_plan", device: Optional[str] = None,
                               **sinkhorn_kwargs):
        """The optimal-transport plan between the two groups' cells that the paired and cluster-matched PoE modes read, from a
        low-dimensional representation both groups share (PCA, or this model's own shared latents from a label-free run): entropic OT
        with squared Euclidean cost by log-domain Sinkhorn iterations, truncated to each cell's ``k`` largest entries in either
        direction (``ot_ops.transport_plan``).  No n0 x n1 matrix exists at any time; needs no model and no training.
        ``use_rep``: a key of ``adata.obsm`` or an array [n_obs, D], 1 <= D <= 64; rows are split by ``adata.uns["groups_obs_indices"]``.
        Writes the scipy CSR plan [n0, n1] (fp32) to ``adata.uns[key_added]`` and, where absent, ``obs["indices"]`` (each cell's position
        within its group); then ``setup_anndata(..., transport_plan_key=key_added)`` takes it.  ``sinkhorn_kwargs``: ``epsilon``,
        ``scale_cost``, ``a``, ``b``, ``max_iter``, ``tol``, ``check_every`` of ``ot_ops.sinkhorn``.  Returns the ``TransportPlan``: the
        potentials, the iteration count and error, and ``row_kept`` / ``col_kept``, the share of each cell's mass the truncation kept."""
        if "groups_obs_indices" not in adata.uns:
            raise ValueError("adata.uns['groups_obs_indices'] missing: build the AnnData with prepare_adatas (or the same schema)")
        if isinstance(use_rep, str):
            obsm = getattr(adata, "obsm", None)
            if obsm is None or use_rep not in obsm:
                raise KeyError(f"use_rep '{use_rep}' not found in adata.obsm")
            use_rep = obsm[use_rep]
        obs_idx = [np.asarray(v) for v in adata.uns["groups_obs_indices"]]
        rep = np.asarray(use_rep)
        if rep.ndim == 2 and rep.shape[0] != adata.n_obs:
            raise ValueError(f"use_rep must have one row per cell ({adata.n_obs}), got {rep.shape[0]}")
        X0, X1, k = check_transport_args(rep, obs_idx, k)
        if not torch.cuda.is_available():
            raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
        from .ot_ops import transport_plan
        dev = torch.device(device or "cuda:0")
        result = transport_plan(torch.from_numpy(X0).to(dev), torch.from_numpy(X1).to(dev), k=k, **sinkhorn_kwargs)
        adata.uns[key_added] = result.to_scipy()
        if "indices" not in adata.obs:
            pos = np.zeros(adata.n_obs, dtype=np.int32)
            for rows in obs_idx:
                pos[rows] = np.arange(len(rows), dtype=np.int32)
            adata.obs["indices"] = pos
        return result

    @classmethod
    def tsne(cls, adata, use_rep, key_added: str = "X_tsne", device: Optional[str] = None, perplexity: float = 30.0, n_components: int = 2,
             n_iter: int = 1000, init="pca", seed: int = 0, **schedule):
        """An exact t-SNE layout of a low-dimensional representation (PCA, or this model's latents written to ``obsm``), for looking at
        it: ``tsne_ops.tsne`` on all cells of ``adata``; needs no model and no training.  ``use_rep``: a key of
        ``adata.obsm`` or an array [n_obs, D], 1 <= D <= 64, finite.  Writes the fp32 layout [n_obs, n_components] to
        ``adata.obsm[key_added]`` and returns the ``TsneResult`` (``embedding``, ``kl_divergence``, ``kl_history``, ``beta``,
        ``n_neighbors``, ``affinities``).  ``perplexity`` in [2, 32]: the affinities rest on min(3 perplexity, 64, n - 1) exact neighbours.
        ``n_iter`` steps are always all taken (no early stop).  ``schedule``: ``early_exaggeration``, ``exaggeration_iter``,
        ``learning_rate``, ``momentum``, ``min_gain``, ``kl_every`` of ``tsne_ops.tsne``.  Deterministic: two calls agree bit for bit."""
        if isinstance(use_rep, str):
            obsm = getattr(adata, "obsm", None)
            if obsm is None or use_rep not in obsm:
                raise KeyError(f"use_rep '{use_rep}' not found in adata.obsm")
            use_rep = obsm[use_rep]
        rep = check_tsne_rep(use_rep, getattr(adata, "n_obs", None))
        schedule = check_tsne_schedule(schedule)
        check_tsne_args(rep.shape[0], perplexity, n_components, n_iter, init, seed, **schedule)
        if not torch.cuda.is_available():
            raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
        from .tsne_ops import tsne
        dev = torch.device(device or "cuda:0")
        result = tsne(torch.from_numpy(rep).to(dev), perplexity=perplexity, n_components=n_components, n_iter=n_iter, init=init, seed=seed, **schedule)
        adata.obsm[key_added] = result.embedding
        return result

    @classmethod
    def lisi(cls, adata, use_rep, keys, perplexity: float = 30, device: Optional[str] = None):
        """The LISI score of every cell of ``adata`` on any low-dimensional representation, for one or more ``obs`` columns: how a user sets
        the shared latent (written to ``obsm``) against the ``X_pca`` they started from.  Needs no model and no training; the paged exact
        k-NN and the fused kernel of ``latent_lisi``.  ``use_rep``: a key of ``adata.obsm`` or an array
        [n_obs, D], 1 <= D <= 64, finite.  ``keys``: an ``obs`` column name or several.  Returns a DataFrame indexed by ``obs_names`` (row
        numbers without any) with a ``lisi_<key>`` column per key, ``n_neighbors`` and ``converged``; ``attrs``: ``lisi_<key>_median``
        and ``n_<key>`` per key, ``perplexity``, ``n_neighbors`` (k = min(int(3 perplexity) - 1, n_obs - 1), which must lie in [1, 256])
        and ``n_unconverged``.  Deterministic: two calls agree bit for bit."""
        if isinstance(use_rep, str):
            obsm = getattr(adata, "obsm", None)
            if obsm is None or use_rep not in obsm:
                raise KeyError(f"use_rep '{use_rep}' not found in adata.obsm")
            use_rep = obsm[use_rep]
        rep = check_tsne_rep(use_rep, getattr(adata, "n_obs", None))
        n = rep.shape[0]
        k = check_lisi_args(n, perplexity)
        keyed = check_lisi_keys(adata.obs, keys, n)
        if not torch.cuda.is_available():
            raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
        from .knn_ops import knn_paged
        from .lisi_ops import LISI_SETS_MAX, lisi
        dev = torch.device(device or "cuda:0")
        X = torch.from_numpy(rep).to(dev)
        idx, d2 = knn_paged(X, X, k, exclude=torch.arange(n, dtype=torch.int32, device=dev))
        parts = []
        for t0 in range(0, len(keyed), LISI_SETS_MAX):   # the calibration is a function of the row alone: every call repeats its bits
            codes = torch.as_tensor(np.stack([c for _key, _cats, c in keyed[t0:t0 + LISI_SETS_MAX]]), device=dev)
            out, _beta, n_valid, converged = lisi(idx, d2, codes, perplexity)
            parts.append(out.cpu().numpy())
        names = getattr(adata, "obs_names", None)
        return lisi_rep_frame(np.arange(n) if names is None else np.asarray(names), keyed, np.concatenate(parts), n_valid.cpu().numpy(),
                              converged.cpu().numpy(), perplexity, k)

    @classmethod
    def pca(cls, adata, n_comps: int = 50, key_added: str = "X_pca", layer: Optional[str] = None, counts_storage: str = "auto",
            device: Optional[str] = None, **kwargs):
        """The ``X_pca`` that ``compute_transport_plan``, ``match_transport_clusters``, ``transport_project``, ``tsne`` and ``lisi`` take
        as ``use_rep``, made here from the raw counts: the joint PCA of ``count_pca`` (``group=None``: the paired genes of both groups,
        log-normalised) over EVERY cell of ``adata``.  Needs no model and no training.  The count matrices become resident the way the
        constructor keeps them (``layer``: a key of ``adata.layers``, None = ``adata.X``; ``counts_storage``: "auto" | "dense" |
        "sparse").  ``kwargs``: ``gene_list``, ``normalize``, ``target_sum``, ``scale``, ``tol``, ``seed`` of ``count_pca``.
        Writes the fp32 scores [n_obs, n_comps] to ``adata.obsm[key_added]``, rows in adata order (a cell of neither group gets NaN),
        and ``adata.uns["pca"] = {"variance", "variance_ratio", "params"}``; returns the ``PcaResult``.  Every refusal comes ahead of
        any device work, as a ValueError or KeyError with the limit in the message."""
        X = check_pca_adata(adata, layer, counts_storage, key_added, kwargs)
        var_idx = [np.asarray(v) for v in adata.uns["groups_var_indices"]]
        obs_idx = [np.asarray(v) for v in adata.uns["groups_obs_indices"]]
        plan = pca_plan(adata, [len(v) for v in var_idx], obs_idx, obs_idx, n_comps=n_comps, group=None, **kwargs)
        if not torch.cuda.is_available():
            raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
        dev = torch.device(device or "cuda:0")
        counts = resident_group_counts(X, obs_idx, var_idx, dev, counts_storage)
        result = _run_count_pca(counts, plan, dev)
        out = np.full((adata.n_obs, result.scores.shape[1]), np.nan, dtype=np.float32)
        out[result.obs] = result.scores
        if getattr(adata, "obsm", None) is None:
            adata.obsm = {}
        adata.obsm[key_added] = out
        adata.uns["pca"] = {"variance": result.variance, "variance_ratio": result.variance_ratio, "params": dict(result.params)}
        return result

    @classmethod
    def match_transport_clusters(cls, adata, use_rep=None, plan=None, n_clusters=(4, 6, 8, 12, 16, 24, 32), cluster_key: Optional[str] = None,
                                 n_init: int = 4, seed: int = 0, device: Optional[str] = None):
        """The labels the cluster-matched PoE mode reads (``setup_anndata(..., match_clusters=True)``), derived as the reference's
        ``process_transport_plan`` derives them: clusters per group, chosen by the plan's entropy criterion, matched across the groups
        by the Hungarian algorithm on the plan's mass between them.  No scanpy and no n0 x n1 matrix.
        ``use_rep``: a key of ``adata.obsm`` or an array [n_obs, D], 1 <= D <= 64, as ``compute_transport_plan``.
        ``plan``: the ``TransportPlan`` of ``compute_transport_plan`` -- the masses then come from its Sinkhorn potentials, i.e. from the
        UNTRUNCATED plan, by the fused kernel (``ot_ops.ot_segment_lse``); the potentials mean something only on the representation
        they were computed on, so pass the same ``use_rep`` (only the two row counts can be checked) --, or a plain matrix [n0, n1]
        (dense array or scipy sparse), whose cluster sums are taken on the host in fp64, or None: ``compute_transport_plan(adata,
        use_rep)`` runs first and writes the plan as usual.
        ``n_clusters``: an int fixes K for both groups; a sequence is swept per group (candidates above the group's size are dropped)
        and each group takes the K with the highest ``data.cluster_entropy_score``, the first on ties.  Clusters are k-means on
        ``use_rep`` (``cluster_ops.kmeans_best`` with ``n_init`` seedings from ``seed``).  ``cluster_key``: an ``obs`` column with the
        user's own per-cell clusters (Leiden run elsewhere, say) instead: no k-means, no sweep; a cluster is (group, value).  With a
        matrix plan as well no device is needed, nor ``use_rep``.
        Clusters are matched on score = block mass / (cells x cells), the MEAN plan entry of a block (the reference takes the median).
        Writes ``obs["group_cluster_labels"]`` ("<group index>_<cluster>"), ``obs["processed_transport_labels"]`` ("Cluster_m": matched
        pairs share a name, in ``row_ind`` order; every unmatched cluster gets its own) and ``uns["cluster_matching"]``: a dict with
        ``n_clusters`` (K0, K1), ``candidates``, ``criterion`` (per group {K: score}), ``mass`` and ``score`` [K0, K1], ``row_ind`` /
        ``col_ind`` and ``names`` (per group the clusters' new names).  Returns a ``data.ClusterMatching`` with the same contents and
        the per-group labels.  Argument faults are refused before any device work and before anything is written."""
        rep = None
        if use_rep is not None:
            if isinstance(use_rep, str):
                obsm = getattr(adata, "obsm", None)
                if obsm is None or use_rep not in obsm:
                    raise KeyError(f"use_rep '{use_rep}' not found in adata.obsm")
                rep = np.asarray(obsm[use_rep])
            else:
                rep = np.asarray(use_rep)
            if rep.ndim == 2 and rep.shape[0] != adata.n_obs:
                raise ValueError(f"use_rep must have one row per cell ({adata.n_obs}), got {rep.shape[0]}")
        obs_idx, cand, swept = check_match_clusters_args(adata, rep, plan, n_clusters, cluster_key, n_init, seed)
        matrix_plan = plan is not None and not hasattr(plan, "sinkhorn")
        Xd = None
        if not (matrix_plan and cluster_key is not None):
            if rep is None:
                raise ValueError("use_rep is needed: the plan's potentials are read on the representation they were computed on")
            X0, X1, _ = check_transport_args(rep, obs_idx, 1)
            if not torch.cuda.is_available():
                raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
            dev = torch.device(device or "cuda:0")
            Xd = [torch.from_numpy(X0).to(dev), torch.from_numpy(X1).to(dev)]
            if plan is None:
                plan = cls.compute_transport_plan(adata, rep, device=device)

        def table(g, labels, K):
            """log mass [K, n_other] between the clusters of group g and the cells of the other group"""
            from .cluster_ops import cluster_transport_log_mass
            return cluster_transport_log_mass(plan.sinkhorn, Xd[1 - g], Xd[g], labels, 1 - g, K)

        labels, values, tables, criterion = [None, None], [None, None], [None, None], [{}, {}]
        if cluster_key is not None:
            col = np.asarray(adata.obs[cluster_key])
            for g in range(2):
                values[g], labels[g] = np.unique(col[obs_idx[g]], return_inverse=True)
                labels[g] = labels[g].astype(np.int64)
            if matrix_plan:
                tables = list(cluster_tables_from_matrix(plan, labels[0], len(values[0]), labels[1], len(values[1])))
            else:
                tables = [table(g, labels[g], len(values[g])) for g in range(2)]
            for g in range(2):
                criterion[g][len(values[g])] = cluster_entropy_score(tables[g])
        else:
            from .cluster_ops import kmeans_best
            for g in range(2):
                best = None
                for K in (c for c in cand if c <= len(obs_idx[g])):
                    lab = kmeans_best(Xd[g], K, n_init, seed).labels
                    if matrix_plan:
                        other = np.zeros(len(obs_idx[1 - g]), dtype=np.int64)
                        tab = cluster_tables_from_matrix(plan, *((lab, K, other, 1) if g == 0 else (other, 1, lab, K)))[g]
                    else:
                        tab = table(g, lab, K)
                    criterion[g][K] = cluster_entropy_score(tab)
                    if best is None or criterion[g][K] > criterion[g][best]:
                        best, labels[g], tables[g] = K, lab, tab
                values[g] = np.arange(best)
        K0, K1 = len(values[0]), len(values[1])
        mass, score = cluster_pair_scores(tables[1], labels[0], np.bincount(labels[1], minlength=K1), K0)
        match = match_cluster_labels(score)
        group_cluster = np.full(adata.n_obs, "", dtype=object)
        processed = np.full(adata.n_obs, "", dtype=object)
        for g in range(2):
            group_cluster[obs_idx[g]] = np.array([f"{g}_{v}" for v in values[g]], dtype=object)[labels[g]]
            processed[obs_idx[g]] = np.array(match["names"][g], dtype=object)[labels[g]]
        result = ClusterMatching(n_clusters=(K0, K1), candidates=cand if swept else None, criterion=criterion, mass=mass, score=score,
                                 row_ind=match["row_ind"], col_ind=match["col_ind"], names=match["names"], labels=labels,
                                 cluster_values=[list(values[0]), list(values[1])])
        adata.obs["group_cluster_labels"] = group_cluster.astype(str)
        adata.obs["processed_transport_labels"] = processed.astype(str)
        adata.uns["cluster_matching"] = result.as_dict()
        return result

    @classmethod
    def transport_project(cls, adata, use_rep, plan, values, onto: int = 0, key_added: Optional[str] = None, device: Optional[str] = None):
        """Push per-cell values of one group through the transport plan onto the other group's cells (the barycentric projection, the
        ``push`` / ``pull`` of OT tool kits): for every cell i of group ``onto`` the plan-weighted mean sum_j P_ij V[j] / sum_j P_ij of
        the OTHER group's values.  The weights are the UNTRUNCATED plan, read from the Sinkhorn potentials by one fused kernel
        (``ot_ops.ot_project``): no n0 x n1 matrix, none of the stored plan's truncation to k entries per cell.
        Needs no model and no training.
        ``use_rep``: a key of ``adata.obsm`` or an array [n_obs, D], 1 <= D <= 64 -- the representation ``plan`` was computed on (the
        potentials mean something only there; only the two row counts can be checked).  ``plan``: the ``TransportPlan`` of
        ``compute_transport_plan``; a plain matrix is refused (it has no potentials: ``plan.to_scipy() @ values`` is the host route).
        ``values`` describes the other group's cells: an array [n_other, n_v] or [n_obs, n_v] (the other group's rows are then taken
        by ``uns["groups_obs_indices"]``), or a key of ``obsm`` -- coordinates give each cell's image in the other group's space,
        log-expression of marker genes gives cross-group imputation --, or the name of an ``obs`` column: OT label transfer.  All
        values must be finite; more than ``ot_ops.OT_VAL_MAX`` columns are walked in slices (a column's result does not depend on
        the slicing).
        Returns an ndarray fp32 [n_onto, n_v]; for an ``obs`` column a DataFrame indexed by the receiving cells' ``obs_names`` (their
        row numbers where ``adata`` has none): one probability column per category among the other group's cells, ``predicted`` (the
        most probable category, the first on ties) and ``confidence`` (its probability).  With ``key_added`` the array (the
        probabilities) is also written to ``obsm[key_added]`` [n_obs, n_v], NaN in the other group's rows.  Argument faults are refused
        before any device work and before anything is written."""
        rep = use_rep
        if isinstance(use_rep, str):
            obsm = getattr(adata, "obsm", None)
            if obsm is None or use_rep not in obsm:
                raise KeyError(f"use_rep '{use_rep}' not found in adata.obsm")
            rep = obsm[use_rep]
        rep = np.asarray(rep)
        if rep.ndim == 2 and rep.shape[0] != adata.n_obs:
            raise ValueError(f"use_rep must have one row per cell ({adata.n_obs}), got {rep.shape[0]}")
        obs_idx, X0, X1, V, categories = check_transport_project_args(adata, rep, plan, values, onto, key_added)
        if key_added is not None and getattr(adata, "obsm", None) is None:
            raise ValueError("key_added needs adata.obsm")
        if not torch.cuda.is_available():
            raise _abi.SpvError("spvipes_amd needs an MI355X: there is no CPU fallback for the hot path")
        from .ot_ops import OT_VAL_MAX
        from .ot_ops import transport_project as project
        dev, onto = torch.device(device or "cuda:0"), int(onto)
        Xd = [torch.from_numpy(X0).to(dev), torch.from_numpy(X1).to(dev)]
        Vd = torch.from_numpy(V).to(dev)
        out = np.empty((len(obs_idx[onto]), V.shape[1]), dtype=np.float32)
        for v0 in range(0, V.shape[1], OT_VAL_MAX):
            out[:, v0:v0 + OT_VAL_MAX] = project(plan.sinkhorn, Xd[onto], Xd[1 - onto], Vd[:, v0:v0 + OT_VAL_MAX], onto)[0].cpu().numpy()
        if key_added is not None:
            full = np.full((adata.n_obs, V.shape[1]), np.nan, dtype=np.float32)
            full[obs_idx[onto]] = out
            adata.obsm[key_added] = full
        if categories is None:
            return out
        names = getattr(adata, "obs_names", None)
        return label_projection_frame(out, categories, np.asarray(names)[obs_idx[onto]] if names is not None else obs_idx[onto])

    # ------------------------------------------------------------------------------------------
    def _local_rows(self, g: int, indices: Sequence[int]) -> np.ndarray:
        """adata row numbers -> rows of group g's resident matrix."""
        pos = np.full(self.adata.n_obs, -1, dtype=np.int64)
        pos[self.obs_idx[g]] = np.arange(len(self.obs_idx[g]))
        loc = pos[np.asarray(indices)]
        if (loc < 0).any():
            raise ValueError(f"group_indices_list[{g}] contains cells that do not belong to group {g}")
        return loc

    def _minibatch(self, rows: Sequence[torch.Tensor]):
        out = []
        for g, r in enumerate(rows):
            rl = r.long()
            d = {"counts": self.counts[g], "rows": r, "indices": self._plan_indices[g][rl].unsqueeze(1), "groups": None, "batch": None}
            if self._batch is not None:
                d["batch"] = self._batch[g][rl].unsqueeze(1)
            if self._labels is not None:
                d["labels"] = self._labels[g][rl].unsqueeze(1)
            if self._components is not None:
                d["processed_transport_labels"] = self._components[g][rl].unsqueeze(1)
            out.append(d)
        return tuple(out)

    def train(self, group_indices_list: List[List[int]], batch_size: Optional[int] = 128, max_epochs: Optional[int] = None,
              use_gpu=None, train_size: float = 0.9, validation_size: Optional[float] = None, early_stopping: bool = False,
              plan_kwargs: Optional[dict] = None, n_steps_kl_warmup: Optional[int] = None, n_epochs_kl_warmup: Optional[int] = 400,
              seed: int = 0, **trainer_kwargs) -> None:
        """training_mixin.py:19-123, same signature.  ``validation_size`` / ``train_size`` hold cells out exactly as
        MultiGroupDataSplitter does; ``early_stopping`` monitors ``elbo_validation`` with scvi-tools' defaults (patience 45;
        ``early_stopping_patience`` / ``early_stopping_min_delta`` / ``check_val_every_n_epoch`` in ``trainer_kwargs`` as for
        scvi's Trainer).  ``use_gpu`` is accepted and ignored (the path only runs on the GPU).  Inside an initialised
        ``torch.distributed`` job every rank trains on its own shard of the training cells from identical
        initial weights (rank 0's are broadcast)."""
        import torch.distributed as dist

        if max_epochs is None:
            max_epochs = default_max_epochs(self.adata.n_obs)
        plan_kwargs = dict(plan_kwargs or {})
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        local = [self._local_rows(g, group_indices_list[g]) for g in range(2)]
        sampler = MinibatchSampler([len(l) for l in local], batch_size, self.device, seed=seed, train_size=train_size,
                                   validation_size=validation_size, group_indices_list=local, rank=rank, world=world)
        trainer = Trainer(self.module, self.counts, lr=plan_kwargs.get("lr", 1e-3), eps=plan_kwargs.get("eps", 0.01),
                          weight_decay=plan_kwargs.get("weight_decay", 1e-6), n_epochs_kl_warmup=n_epochs_kl_warmup,
                          n_steps_kl_warmup=n_steps_kl_warmup, batch_codes=self._batch)
        if world > 1:
            dist.broadcast(trainer.fp.flat, src=0)
            trainer.parameters_changed()
        trainer.minibatch = self._minibatch  # labels / components / plan indices of this AnnData
        self.trainer_, self.sampler_ = trainer, sampler
        self.history = trainer.fit(sampler, max_epochs, log_every=trainer_kwargs.get("log_every", 1), use_graph=trainer_kwargs.get("use_graph", True),
                                   early_stopping=bool(trainer_kwargs.get("early_stopping", early_stopping)),
                                   early_stopping_patience=trainer_kwargs.get("early_stopping_patience", 45),
                                   early_stopping_min_delta=trainer_kwargs.get("early_stopping_min_delta", 0.0),
                                   check_val_every_n_epoch=trainer_kwargs.get("check_val_every_n_epoch"))
        self.is_trained_ = True

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def get_latent_representation(self, group_indices_list: List[List[int]], adata=None, indices=None, normalized: bool = False,
                                  give_mean: bool = True, mc_samples: int = 5000, batch_size: Optional[int] = None,
                                  drop_last: Optional[bool] = None, _noise=None) -> dict:
        """model/spvipes.py:424-650.  {"shared","private","shared_reordered","private_reordered"} -> {0: ndarray, 1: ndarray}, one row
        per cell of ``group_indices_list[g]``.

        ``normalized=False``: the SAMPLED ``log_z`` (as the reference does).
        ``normalized=True, give_mean=False``: the softmaxed embedding, each cell's topic proportions (:448-454) -- ``softmax`` of the
          very ``log_z`` that ``normalized=False`` returns, i.e. the ``theta`` the inference kernels write next to it; same keys,
          shapes and row order.
        ``normalized=True, give_mean=True`` (the Monte-Carlo mean of the logistic-normal over ``mc_samples`` draws, :555-564) is not
          built: NotImplementedError, raised before any device work.  ``mc_samples`` is otherwise unused.
        ``_noise`` (tests only): callable (step, B0, B1) -> dict of injected standard-normal draws for module.inference."""
        if normalized and give_mean:
            raise NotImplementedError("normalized=True with give_mean=True (the Monte-Carlo mean of the logistic-normal) is not built; "
                                      "give_mean=False returns softmax(log_z)")
        n1, n2 = (len(g) for g in group_indices_list)
        res = {k: [] for k in ("s0", "s1", "p0", "p1", "i1")}
        private_key, shared_key = ("theta", "logtheta_theta") if normalized else ("log_z", "logtheta_log_z")
        for step, tensors, (B0, B1) in self._eval_minibatches(group_indices_list, batch_size, drop_last):
            out = self._infer(tensors, _noise, step, B0, B1)
            res["s0"].append(out["poe_stats"][0][shared_key].cpu().numpy())
            res["s1"].append(out["poe_stats"][1][shared_key].cpu().numpy())
            res["p0"].append(out["private_stats"][0][private_key].cpu().numpy())
            res["p1"].append(out["private_stats"][1][private_key].cpu().numpy())
            res["i1"].append(tensors[1]["indices"].cpu().numpy())
        return format_latent_results(res["p0"], res["p1"], res["s0"], res["s1"], res["i1"], n1, n2)

    def _eval_minibatches(self, group_indices_list, batch_size: Optional[int], drop_last: Optional[bool]):
        """The minibatch pairs the read-out methods walk, in order, with the module in eval mode (its mode is restored when the
        walk ends): (step, per-group minibatch tensors, (B0, B1)) for every step of ``latent_steps`` under ``latent_loader_mode``
        (model/spvipes.py:468-523, the cycling path of the paired PoE :578-626).  Concatenating a group's per-step rows and cutting
        at the group's size gives one row per cell of ``group_indices_list[g]``, in its order."""
        batch_size = batch_size or 128
        local = [self._local_rows(g, group_indices_list[g]) for g in range(2)]
        drop_last, use_cycling = latent_loader_mode(self.module.use_labels, self.module.use_transport_plan, self.module.pair_data, drop_last)   # :468-503
        was_training = self.module.training
        self.module.eval()
        try:
            for step, (r0, r1) in enumerate(latent_steps(local, batch_size, drop_last, use_cycling)):
                rows = [torch.as_tensor(r, dtype=torch.int32, device=self.device) for r in (r0, r1)]
                yield step, self._minibatch(rows), (len(r0), len(r1))
        finally:
            self.module.train(was_training)

    def _infer(self, tensors, _noise, draw: int, B0: int, B1: int):
        kw = {} if _noise is None else {"noise": _noise(draw, B0, B1)}
        return self.module.inference(**self.module._get_inference_input(tensors), **kw)

    def _draws(self, step: int, tensors, B, n_samples: int, _noise):
        """(sample, inference outputs) for the ``n_samples`` draws of one step of the walk.  The draw index ``step * n_samples + sample``
        is what ``_noise`` is asked for: every read-out walking the same minibatches sees the same latents draw for draw."""
        for smp in range(n_samples):
            yield smp, self._infer(tensors, _noise, step * n_samples + smp, B[0], B[1])

    def _genes(self, g: int, gene_list, own: bool = False):
        """-> (positions or None, their device copy or None, how many, the index of a result table) for group g's part of a gene
        selection.  ``gene_list``: one entry per group as ``resolve_gene_list`` takes it, or with ``own`` group g's entry alone."""
        if own and gene_list is not None:
            gene_list = [gene_list if k == g else None for k in range(2)]
        n_genes = [int(self.module.input_dims[k]) for k in range(2)]
        names = group_var_names(self.adata)
        sel = resolve_gene_list(gene_list, n_genes, names)[g]
        dev_sel = None if sel is None else torch.as_tensor(sel, dtype=torch.int32, device=self.device)
        n_sel = n_genes[g] if sel is None else len(sel)
        index = (np.arange(n_sel) if sel is None else np.asarray(sel)) if names[g] is None else (np.asarray(names[g]) if sel is None else np.asarray(names[g])[sel])
        return sel, dev_sel, n_sel, index

    @torch.no_grad()
    def get_normalized_expression(self, group_indices_list: List[List[int]], gene_list=None, library_size="latent", component: str = "mixture",
                                  n_samples: int = 1, use_mean: bool = True, batch_size: Optional[int] = None, return_numpy: bool = True,
                                  _noise=None) -> dict:
        """The expression the decoder predicts for every cell (scvi-tools' ``get_normalized_expression``): {0: [n_cells_0, n_sel_0],
        1: [n_cells_1, n_sel_1]}, row i of group g being the cell row i of ``get_latent_representation(...)["shared"][g]`` describes
        (the same minibatch walk).  The decoder is an NB mixture whose component 1 is driven by the private factors and component 2
        by the shared ones (spVIPESmodule.py:751-759, nn/networks.py:314-325); with pi = sigmoid(mixing logits)

        ``component``: "mixture" the mixture's mean pi * rate_private + (1 - pi) * rate_shared | "private" pi * rate_private |
        "shared" (1 - pi) * rate_shared | "mixing" pi itself.
        ``gene_list``: None, or one entry per group: None (all the group's genes) | integer positions within the group's own genes |
        gene names (``adata.var_names`` / ``uns["groups_var_names"]``, as ``get_loadings`` labels them); any order, repeats allowed;
        unknown names raise KeyError, positions out of range IndexError.  Only the selected genes are computed and stored.
        ``library_size``: "latent" -- the model's own exp(library); the library the encoder sees is the log of the summed LOG1P
        counts, so this scale lives in the log1p domain, not in raw counts -- or a positive number L
        (every cell's rates then sum to L over the group's genes).
        ``use_mean``: decode the posterior means (deterministic: two calls agree bit for bit); else decode sampled latents and
        average ``n_samples`` draws on the device.  ``n_samples > 1`` with ``use_mean`` is a ValueError.
        ``return_numpy``: each step's block is copied to the host as it completes (device memory holds one [batch, n_sel] block per
        group); False returns device tensors.  A full [n_cells, G] result returned as numpy is bounded by that copy, not by the kernel.
        Each cell is decoded with its own batch covariate.  ``_noise`` (tests only): callable (draw, B0, B1) -> injected standard-normal
        draws for module.inference, draw = step * n_samples + sample."""
        _what, _log_l, n_samples = check_expression_args(component, library_size, n_samples, use_mean)
        blocks = RowBlocks([len(g) for g in group_indices_list], return_numpy)
        dev_sel = [self._genes(g, gene_list)[1] for g in range(2)]
        for step, tensors, B in self._eval_minibatches(group_indices_list, batch_size, None):
            blk = [None, None]
            for smp, out in self._draws(step, tensors, B, n_samples, _noise):
                for g in range(2):
                    blk[g] = self.module.expected_expression(out, g, genes=dev_sel[g], what=component, library_size=library_size, use_mean=use_mean,
                                                             out=blk[g], alpha=1.0 / n_samples, accumulate=smp > 0)
            blocks.add(blk)
        return blocks.result()

    @torch.no_grad()
    def posterior_predictive_sample(self, group_indices_list: List[List[int]], n_samples: int = 1, gene_list=None, library_size="latent", seed: int = 0,
                                    batch_size: Optional[int] = None, return_numpy: bool = True, _noise=None) -> dict:
        """Counts drawn from the model for every cell (scvi-tools' ``posterior_predictive_sample``): {0: int32 [n_cells_0, n_sel_0],
        1: int32 [n_cells_1, n_sel_1]}, or [n_cells, n_sel, n_samples] (scvi-tools' layout) for ``n_samples > 1``; row i of group g
        is the cell row i of ``get_latent_representation(...)["shared"][g]`` describes (the same minibatch walk).  Every sample runs
        the encoders with freshly sampled latents (posterior predictive) and then draws, per cell and gene, from the decoder's NB
        mixture (spVIPESmodule.py:751-759): c ~ Bernoulli(pi), lam ~ Gamma(theta, mu_c / theta), x ~ Poisson(lam), with
        mu_1 = rate_private, mu_2 = rate_shared, pi = sigmoid(mixing logits), theta = exp(px_r) -- decode and draw in one HIP kernel.

        ``gene_list`` / ``library_size``: as ``get_normalized_expression`` takes them.  "latent" is the model's own exp(library); the
        library the encoder sees is the log of the summed LOG1P counts, so counts drawn at this scale
        live in the log1p domain, not in raw counts; pass a positive number L for rates that sum to L over the group's genes.
        ``seed`` (0 .. 2^32 - 1) keys the count draws: the draw of (cell, gene, sample) depends on the seed, the cell's adata row
        number, the gene's position within the group and the sample index only, not on ``batch_size``, the gene selection or the
        device.  The latents' noise is the module's own (torch's generator) unless ``_noise`` injects it, so two calls agree bit for
        bit only with the same seed AND the same latent noise.
        ``return_numpy``: each step's block is copied to the host as it completes; False returns device tensors.
        ``_noise`` (tests only): callable (draw, B0, B1) -> injected standard-normal draws, draw = step * n_samples + sample."""
        from .dec_ops import sample_key

        n_samples, seed, _log_l = check_sample_args(n_samples, seed, library_size)
        blocks = RowBlocks([len(g) for g in group_indices_list], return_numpy)
        _sel, dev_sel, n_sel, _index = zip(*[self._genes(g, gene_list) for g in range(2)])
        obs = [torch.as_tensor(np.asarray(self.obs_idx[g]), dtype=torch.int32, device=self.device) for g in range(2)]
        key = sample_key(seed)
        for step, tensors, B in self._eval_minibatches(group_indices_list, batch_size, None):
            blk = [torch.empty((B[g], n_sel[g], n_samples), dtype=torch.int32, device=self.device) for g in range(2)]
            ids = [obs[g][tensors[g]["rows"].long()].contiguous() for g in range(2)]
            for smp, out in self._draws(step, tensors, B, n_samples, _noise):
                for g in range(2):
                    self.module.sample_counts(out, g, genes=dev_sel[g], library_size=library_size, key=key, sample=smp, cell_ids=ids[g],
                                              out=blk[g][:, :, smp])
            blocks.add(blk if n_samples > 1 else [b[:, :, 0] for b in blk])
        return blocks.result()

    @torch.no_grad()
    def differential_expression(self, group_indices_list: List[List[int]], group: int, idx1, idx2=None, gene_list=None, component: str = "mixture",
                                library_size=1.0, n_samples: int = 1, use_mean: bool = False, n_pairs: int = 10_000, delta: float = 0.25,
                                pseudocount: float = 0.0, fdr_target: float = 0.05, max_cells: Optional[int] = None, seed: int = 0,
                                batch_size: Optional[int] = None, _noise=None, _pair_rows=None):
        """Which genes differ between two sets of cells of ONE group (scvi-tools 0.20 ``differential_expression``, mode "change"):
        a pandas DataFrame, one row per selected gene in selection order, indexed by the genes' names as ``get_loadings`` labels
        them (their positions when the AnnData has none), with the columns

            proba_de       the share of pairs with |lfc| >= ``delta``,  lfc = log2(x1 + pseudocount) - log2(x2 + pseudocount)
            proba_not_de   1 - proba_de           bayes_factor   log(proba_de + 1e-8) - log(proba_not_de + 1e-8)
            scale1, scale2 the mean decoded expression of the two populations over the pairs
            lfc_mean, lfc_std (population form), lfc_min, lfc_max
            is_de_fdr_<fdr_target>   the largest set of genes, by decreasing proba_de, whose mean proba_not_de is <= fdr_target

        ``lfc_median`` is not a column of this table: it needs a per-gene selection over the pairs, not a streaming reduction, and so
        a kernel of its own; ``differential_expression_median`` is this method with that column.
        ``idx1`` / ``idx2``: adata row numbers of cells of ``group_indices_list[group]``; ``idx2=None`` = every other cell of it.  A cell
        outside it, overlapping or empty populations are ValueErrors.  ``gene_list``: None | positions | names of THIS group's genes.
        How it is computed: the minibatches are walked exactly as ``get_normalized_expression`` walks them (a cell's latents depend on its
        minibatch partners, so a cell's decoded row IS the row that method returns for it; steps without a population cell are
        skipped), each of ``n_samples`` draws is decoded with ``component`` / ``library_size`` (1.0: normalised scales, what scvi-tools
        compares) into a device-resident fp32 bank per population, ``n_pairs`` pairs of bank rows are drawn with replacement from
        ``default_rng(seed)``, and ONE fused HIP kernel (spv_de_pairs) compares and reduces them: only the per-gene table leaves the
        device.  Bank memory is (n_1 + n_2) * n_samples * n_sel * 4 bytes; ``max_cells`` caps each population by a seeded subsample
        before the walk.  ``use_mean=True`` (needs ``n_samples == 1``) compares decoded posterior means and is deterministic.
        ``_noise`` (tests only): as in ``get_normalized_expression``; ``_pair_rows`` (tests only): (r1, r2) bank rows instead of drawn ones."""
        return self.differential_expression_median(group_indices_list, group, idx1, idx2, gene_list, component, library_size, n_samples, use_mean, n_pairs,
                                                   delta, pseudocount, fdr_target, max_cells, seed, batch_size, False, _noise, _pair_rows)

    @torch.no_grad()
    def differential_expression_median(self, group_indices_list: List[List[int]], group: int, idx1, idx2=None, gene_list=None, component: str = "mixture",
                                       library_size=1.0, n_samples: int = 1, use_mean: bool = False, n_pairs: int = 10_000, delta: float = 0.25,
                                       pseudocount: float = 0.0, fdr_target: float = 0.05, max_cells: Optional[int] = None, seed: int = 0,
                                       batch_size: Optional[int] = None, lfc_median: bool = True, _noise=None, _pair_rows=None):
        """``differential_expression`` (same arguments, same banks, same pairs, every column of its table bit for bit) with scvi-tools'
        column ``lfc_median`` directly after ``lfc_mean``: the exact median of the pairs' fp32 lfc values, 0.5 * (mid_lo + mid_hi) of
        the two middle order statistics in float64.  They come from a second HIP kernel (spv_de_median, a radix select in four gather
        passes) on the banks the first one read; ``lfc_min <= lfc_median <= lfc_max`` holds exactly.  ``lfc_median=False`` launches
        nothing more and returns ``differential_expression``'s frame."""
        import pandas as pd

        _what, _log_l, n_samples = check_expression_args(component, library_size, n_samples, use_mean)
        n_pairs, delta, pseudocount, fdr_target, max_cells = check_de_args(n_pairs, delta, pseudocount, fdr_target, max_cells)
        g = check_group(group)
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        pops = de_populations(group_indices_list[g], idx1, idx2, group=g)
        pops = [de_subsample(p, max_cells, seed + 1 + k) for k, p in enumerate(pops)]
        banks = self._de_banks(group_indices_list, g, pops, dev_sel, n_sel, component, library_size, n_samples, use_mean, batch_size, _noise)
        r1, r2 = de_pair_rows(banks[0].shape[0], banks[1].shape[0], n_pairs, seed) if _pair_rows is None else (np.asarray(r).astype(np.int32) for r in _pair_rows)
        return pd.DataFrame(self._de_compare(banks[0], banks[1], r1, r2, delta, pseudocount, fdr_target, bool(lfc_median)), index=index)

    def _de_banks(self, group_indices_list, g: int, pops, dev_sel, n_sel: int, component, library_size, n_samples: int, use_mean: bool, batch_size, _noise):
        """One device-resident fp32 bank [len(p) * n_samples, n_sel] per population p of ``pops`` (positions within
        ``group_indices_list[g]``): row draw * len(p) + i holds draw ``draw`` of the decoded expression of the population's i-th cell.
        ONE walk of the eval minibatches fills them all; steps without a population cell are skipped."""
        n_g = len(group_indices_list[g])
        slot = [np.full(n_g, -1, dtype=np.int64) for _ in pops]   # position within group_indices_list[g] -> the cell's place in its population (-1: not in it)
        for s, p in zip(slot, pops):
            s[p] = np.arange(len(p))
        banks = [torch.empty((len(p) * n_samples, n_sel), dtype=torch.float32, device=self.device) for p in pops]
        blk = None
        for step, tensors, B, _off, pos in walk_positions(self._eval_minibatches(group_indices_list, batch_size, None), g, n_g):
            moves = []
            for k in range(len(pops)):
                sl = np.where(pos >= 0, slot[k][pos], -1)   # a cut row (pos -1) belongs to no population
                src = np.nonzero(sl >= 0)[0]
                if src.size:
                    moves.append((k, torch.as_tensor(src, device=self.device), torch.as_tensor(sl[src], device=self.device)))
            if not moves:
                continue   # eval mode: steps are independent of each other
            for smp, out in self._draws(step, tensors, B, n_samples, _noise):
                if blk is None or blk.shape[0] < B[g]:
                    blk = torch.empty((B[g], n_sel), dtype=torch.float32, device=self.device)
                rows = self.module.expected_expression(out, g, genes=dev_sel, what=component, library_size=library_size, use_mean=use_mean, out=blk)
                for k, src, dst in moves:
                    banks[k].index_copy_(0, dst + smp * len(pops[k]), rows.index_select(0, src))
        return banks

    def _de_compare(self, bank1, bank2, r1, r2, delta: float, pseudocount: float, fdr_target: float, lfc_median: bool) -> dict:
        """The result table (column -> array) of one comparison: spv_de_pairs, and spv_de_median when asked, on the same banks and pair rows"""
        from .de_ops import de_median, de_pairs

        t1, t2 = torch.as_tensor(r1, device=self.device), torch.as_tensor(r2, device=self.device)
        stats = {k: v.cpu().numpy() for k, v in de_pairs(bank1, bank2, t1, t2, delta=delta, eps=pseudocount).items()}
        if lfc_median:
            mid = de_median(bank1, bank2, t1, t2, eps=pseudocount)
            stats["lfc_median"] = 0.5 * (mid["mid_lo"].cpu().numpy().astype(np.float64) + mid["mid_hi"].cpu().numpy().astype(np.float64))
        return de_table(stats, len(r1), fdr_target)

    @torch.no_grad()
    def differential_expression_by(self, group_indices_list: List[List[int]], group: int, groupby, labels=None, gene_list=None, component: str = "mixture",
                                   library_size=1.0, n_samples: int = 1, use_mean: bool = False, n_pairs: int = 10_000, delta: float = 0.25,
                                   pseudocount: float = 0.0, fdr_target: float = 0.05, max_cells: Optional[int] = None, seed: int = 0,
                                   batch_size: Optional[int] = None, lfc_median: bool = True, _noise=None):
        """One label against the rest, for every label of a column (scvi-tools' ``differential_expression(groupby=...)``): the
        tables of ``differential_expression_median`` for label k's cells against every other cell of ``group_indices_list[group]``,
        concatenated in label order, with the columns ``comparison`` ("<label> vs Rest"), ``group1`` (the label) and ``group2``
        ("Rest") appended; the index repeats the gene names once per label, ``is_de_fdr_*`` is computed per comparison.

        ``groupby``: the name of an ``adata.obs`` column, or an array with one label per cell of ``group_indices_list[group]``.  The
        label set is ``np.unique`` of those labels (sorted); ``labels`` restricts which of them are compared (KeyError for an unknown
        one); fewer than two distinct labels is a ValueError.  ``max_cells`` caps EACH label's cells (``de_subsample`` with seed
        ``seed + 1 + k``, k = the label's place in the sorted set); "rest" is the other labels' kept cells.  Label k's pairs are
        ``de_pair_rows(n_label * n_samples, n_rest * n_samples, n_pairs, seed + k)``.
        How it is computed: the eval minibatches are walked ONCE and every kept cell is decoded ONCE per draw into one device bank
        (row = draw * n_kept + the cell's place among the kept cells in position order); every comparison then runs the two kernels
        with that bank on both sides and its own pair rows.  With ``max_cells=None`` label k's block equals
        ``differential_expression_median(group_indices_list, group, idx1=<the label's cells in position order>, idx2=None,
        seed=seed + k, ...)`` bit for bit, which decodes the whole group again for every label.  The other arguments are
        ``differential_expression``'s."""
        _what, _log_l, n_samples = check_expression_args(component, library_size, n_samples, use_mean)
        n_pairs, delta, pseudocount, fdr_target, max_cells = check_de_args(n_pairs, delta, pseudocount, fdr_target, max_cells)
        g = check_group(group)
        cells = np.asarray(group_indices_list[g]).astype(np.int64).ravel()
        cell_labels = group_cell_labels(self.adata.obs, groupby, cells, g, unique=True)
        names, compared, kept, places = de_label_populations(cell_labels, labels, max_cells, seed)
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        bank, = self._de_banks(group_indices_list, g, [kept], dev_sel, n_sel, component, library_size, n_samples, use_mean, batch_size, _noise)
        tables = []
        for k in compared:
            p1, p2 = places[k]
            r1, r2 = de_pair_rows(len(p1) * n_samples, len(p2) * n_samples, n_pairs, seed + k)
            tables.append((names[k], self._de_compare(bank, bank, de_bank_rows(r1, p1, len(kept)), de_bank_rows(r2, p2, len(kept)), delta, pseudocount, fdr_target, bool(lfc_median))))
        return vs_rest_frames(tables, index)

    @torch.no_grad()
    def count_statistics(self, group_indices_list: List[List[int]], group: int, idx1=None, idx2=None, groupby=None, labels=None, gene_list=None,
                         target_sum: float = 1e4):
        """The raw-count columns of scvi-tools' differential-expression tables (``all_stats=True``), from the OBSERVED counts of ONE
        group: a pandas DataFrame of float64 columns

            raw_mean1, raw_mean2                          the mean count of the gene over the population's cells
            non_zeros_proportion1, non_zeros_proportion2  the share of the population's cells with a non-zero count
            raw_normalized_mean1, raw_normalized_mean2    the mean of count * target_sum / (the cell's total count)

        It needs no trained model and decodes nothing.  Exactly one of ``idx1`` / ``groupby`` selects the mode (else ValueError):
        ``idx1`` (with ``idx2``, None = every other cell of ``group_indices_list[group]``): the two populations of
        ``differential_expression``, resolved by the same rules with the same errors; the frame has that method's index and gene order
        for the same ``gene_list``.  ``groupby`` (with ``labels``): every label against every other cell of the group, as
        ``differential_expression_by`` compares them -- the same label set, the same ``labels`` restriction (KeyError for an unknown
        one), blocks concatenated in label order with ``comparison`` / ``group1`` / ``group2`` appended, rows exactly in that method's
        order for the same ``groupby`` / ``labels`` / ``gene_list``, so ``pd.concat([de, stats[list(data.COUNT_COLUMNS)]], axis=1)`` lines up.
        There is no ``max_cells``: the statistics always cover the full populations.  A cell's total runs over ALL of the group's
        genes whatever ``gene_list`` selects; a cell without counts gets the weight 0 (scvi-tools would divide by zero).
        ``target_sum``: a positive finite number.
        How it is computed: the cells' rows, sorted by population, go through ONE segmented reduction on the device
        (spv_count_stats: integer sums of the uint16 counts, fp64 elsewhere, a fixed order throughout) with the per-cell totals of
        spv_count_totals / spv_csr_totals, kept on the resident matrix; "rest" is the sum of the other labels' sums.  Dense and sparse
        ``counts_storage`` give the same frame bit for bit."""
        import pandas as pd

        from .count_ops import count_stats, count_totals

        target_sum = check_target_sum(target_sum)
        if (idx1 is None) == (groupby is None):
            raise ValueError("count_statistics: give exactly one of idx1 (two populations) and groupby (every label against the rest)")
        g = check_group(group)
        cells = np.asarray(group_indices_list[g]).astype(np.int64).ravel()
        if groupby is None:
            if labels is not None:
                raise ValueError("count_statistics: labels goes with groupby")
            p1, p2 = de_populations(cells, idx1, idx2, group=g)
            order, sizes = np.concatenate([p1, p2]), [len(p1), len(p2)]
        else:
            if idx2 is not None:
                raise ValueError("count_statistics: idx2 goes with idx1")
            cell_labels = group_cell_labels(self.adata.obs, groupby, cells, g, unique=True)
            names, compared, _kept, _places = de_label_populations(cell_labels, labels, None, 0)
            code = np.unique(cell_labels, return_inverse=True)[1].ravel()
            order, sizes = np.argsort(code, kind="stable"), np.bincount(code, minlength=len(names)).tolist()
        _sel, dev_sel, _n_sel, index = self._genes(g, gene_list, own=True)
        rows = torch.as_tensor(self._local_rows(g, cells[order]).astype(np.int32), device=self.device)
        total = count_totals(self.counts[g]).index_select(0, rows.long())
        w = torch.where(total > 0, target_sum / total, torch.zeros_like(total))
        sums = count_stats(self.counts[g], rows, sizes, w=w, genes=dev_sel).cpu().numpy()
        if groupby is None:
            return pd.DataFrame(count_table(sums[0], sizes[0], sums[1], sizes[1]), index=index)
        rest, n_all = count_rest(sums), int(sum(sizes))
        return vs_rest_frames(((names[k], count_table(sums[k], sizes[k], rest[k], n_all - sizes[k])) for k in compared), index)

    @torch.no_grad()
    def rank_genes_groups(self, group_indices_list: List[List[int]], group: int, idx1=None, idx2=None, groupby=None, labels=None, gene_list=None,
                          target_sum: float = 1e4, normalize: bool = True, tie_correct: bool = True):
        """The Wilcoxon / Mann-Whitney rank-sum test on the OBSERVED counts of ONE group (scanpy's
        ``rank_genes_groups(method="wilcoxon")``): a pandas DataFrame of float64 columns per gene (``data.rank_test_table``)

            scores        the z-score of the population's rank sum (ties at their mean rank, no continuity correction)
            u_statistic   the population's Mann-Whitney U          auc   U / (n1 n2)
            pvals         two-sided, from the normal approximation   pvals_adj   Benjamini-Hochberg over the selected genes

        It needs no trained model and decodes nothing.  Exactly one of ``idx1`` / ``groupby`` selects the mode, and the populations,
        labels, ``gene_list`` and ``target_sum`` are resolved exactly as ``count_statistics`` resolves them, with the same errors; the
        frame's index, row order and ``comparison`` / ``group1`` / ``group2`` columns are that method's for the same arguments, so
        ``pd.concat`` with its frame and with the DE frame lines up.  ``groupby``: ONE sort of all the group's cells per gene serves every
        label; "rest" is every other cell of the group.  ``idx1`` (with ``idx2``): only the two populations are listed and ranked.
        ``normalize=True`` ranks count * fp32(target_sum / the cell's total over ALL of the group's genes) (a cell without counts gets
        the weight 0); log1p is monotone, so these are the ranks of scanpy's log-normalised data.  ``normalize=False`` ranks the raw
        counts (``target_sum`` is still checked).  ``tie_correct``: the variance's tie term (scanpy's default is False).  At most 2^20
        ranked cells and 1024 labels.
        ``attrs``: ``n_cells`` (population -> its cells), ``rank2`` (int64 [n_populations, n_sel]: twice each population's rank sum),
        ``ties`` (int64 [n_sel]: the sum of t^3 - t over the runs of equal keys) and ``populations`` (the rows of ``rank2``).
        How it is computed: spv_rank_stage appends every gene's non-zero keys to its column, spv_rank_sums sorts the columns (a
        segmented column sort) and walks the tie runs; every device output is an integer, so dense and sparse ``counts_storage`` give
        the same frame bit for bit and two calls agree bit for bit."""
        import pandas as pd

        from .count_ops import count_totals
        from .data import rank_test_table
        from .rank_ops import rank_sums

        target_sum = check_target_sum(target_sum)
        if (idx1 is None) == (groupby is None):
            raise ValueError("rank_genes_groups: give exactly one of idx1 (two populations) and groupby (every label against the rest)")
        g = check_group(group)
        cells = np.asarray(group_indices_list[g]).astype(np.int64).ravel()
        if groupby is None:
            if labels is not None:
                raise ValueError("rank_genes_groups: labels goes with groupby")
            p1, p2 = de_populations(cells, idx1, idx2, group=g)
            listed, code = np.concatenate([p1, p2]), np.concatenate([np.zeros(len(p1), np.int32), np.ones(len(p2), np.int32)])
            names, compared = np.array(["idx1", "idx2"]), [0]
        else:
            if idx2 is not None:
                raise ValueError("rank_genes_groups: idx2 goes with idx1")
            cell_labels = group_cell_labels(self.adata.obs, groupby, cells, g, unique=True)
            names, compared, _kept, _places = de_label_populations(cell_labels, labels, None, 0)
            listed, code = np.arange(len(cells)), np.unique(cell_labels, return_inverse=True)[1].ravel().astype(np.int32)
        n, n_seg = len(listed), len(names)
        if n > _abi.RANK_MAX_N or n_seg > _abi.RANK_MAX_SEG:
            raise ValueError(f"rank_genes_groups: at most 2^20 ranked cells and {_abi.RANK_MAX_SEG} labels, got {n} and {n_seg}")
        sizes = np.bincount(code, minlength=n_seg).tolist()
        _sel, dev_sel, _n_sel, index = self._genes(g, gene_list, own=True)
        rows = torch.as_tensor(self._local_rows(g, cells[listed]).astype(np.int32), device=self.device)
        w = None
        if normalize:
            total = count_totals(self.counts[g]).index_select(0, rows.long())
            w = torch.where(total > 0, target_sum / total, torch.zeros_like(total)).to(torch.float32)
        rank2, ties = (t.cpu().numpy() for t in rank_sums(self.counts[g], rows, torch.as_tensor(code, device=self.device), n_seg, w=w, genes=dev_sel))
        if groupby is None:
            frame = pd.DataFrame(rank_test_table(rank2[0], ties, sizes[0], n, bool(tie_correct)), index=index)
        else:
            frame = vs_rest_frames(((names[k], rank_test_table(rank2[k], ties, sizes[k], n, bool(tie_correct))) for k in compared), index)
        frame.attrs.update(n_cells={names[k]: sizes[k] for k in range(n_seg)}, rank2=rank2, ties=ties, populations=list(names.tolist()))
        return frame

    @torch.no_grad()
    def posterior_predictive_check(self, group_indices_list: List[List[int]], group: int, n_samples: int = 25, groupby=None, labels=None,
                                   gene_list=None, library_size="latent", seed: int = 0, batch_size: Optional[int] = None, _noise=None):
        """A posterior-predictive check of ONE group's count model that never leaves the device (scvi-tools'
        ``criticism.PosteriorPredictiveCheck``: per-gene mean, variance / CV and zero fraction of sampled against observed counts):
        a pandas DataFrame with one row per (population, selected gene) and the columns

            population, gene, n_cells, n_samples
            obs_mean, obs_var, obs_cv, obs_zero_fraction                  the OBSERVED counts of the population's cells
            ppc_mean, ppc_var, ppc_cv, ppc_zero_fraction, ppc_max         the n_cells * n_samples counts DRAWN for them

        (var: the unbiased sample variance, NaN for fewer than two values; cv = sqrt(var) / mean, NaN at mean 0.)
        ``attrs["cell_totals"]`` holds a frame with ``obs_total`` and ``ppc_total_mean`` (the cell's drawn total averaged over the
        samples) per cell of ``group_indices_list[group]``, in ``get_latent_representation``'s row order, indexed by the adata row
        numbers; a cell outside every population has NaN in both.  Sampled totals run over the SELECTED genes (a repeated gene counts as
        often as it is listed), and the observed totals run over the same selection here -- unlike ``count_statistics``, whose
        normalisation weight always uses the total over all of the group's genes.

        The drawn counts are those of ``posterior_predictive_sample(group_indices_list, n_samples, gene_list, library_size, seed,
        batch_size)`` for this group, integer for integer (same minibatch walk, ``draw = step * n_samples + sample``, same key and cell
        ids), but the [n_cells, n_sel, n_samples] cube is never stored: one fused HIP kernel (spv_dec_sample_stats) decodes, draws and
        adds every minibatch into one 64-bit integer table per (population, gene) and one total per cell; only those leave the device.
        ``groupby``: None -- one population "all" -- or the name of an ``adata.obs`` column or an array with one label per cell of
        ``group_indices_list[group]``: each label is a population, in ``labels`` order (default: the sorted unique labels; an unknown
        label is a KeyError); cells of other labels are left out.  ``gene_list``: None or this group's selection, as
        ``differential_expression`` takes it.  ``library_size``: "latent" and a positive number mean what they mean for
        ``posterior_predictive_sample``; "observed" gives each cell the log of its observed total over ALL of the group's genes as its
        library, so its draws are on the raw-count scale of that cell (a cell without counts gets rate 0 and draws 0).
        The sampled columns are exact: integer sums, divided once (``data.ppc_table``, which also states the overflow rule for the
        sum of squares).  The observed second moment is one chunked pass over the resident counts (``count_ops.count_square_sums``).
        Dense and CSR ``counts_storage`` give the same frame.  ``_noise`` (tests only): as ``posterior_predictive_sample`` takes it."""
        from .count_ops import count_square_sums, count_stats, count_totals
        from .dec_ops import sample_key

        library_size = check_ppc_library(library_size)
        observed = isinstance(library_size, str) and library_size == "observed"
        n_samples, seed, _log_l = check_sample_args(n_samples, seed, "latent" if observed else library_size)
        g = check_group(group)
        cells = np.asarray(group_indices_list[g]).astype(np.int64).ravel()
        n_g = len(cells)
        cell_labels = None if groupby is None else group_cell_labels(self.adata.obs, groupby, cells, g)
        names, sizes, code = ppc_segments(cell_labels, labels, n_cells=n_g)
        n_seg = len(names)
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        obs_ids = torch.as_tensor(np.asarray(self.obs_idx[g]), dtype=torch.int32, device=self.device)
        key = sample_key(seed)
        stats = torch.zeros((n_seg, 4, n_sel), dtype=torch.int64, device=self.device)   # (uint64 bits)
        totals = torch.zeros((n_g + (batch_size or 128),), dtype=torch.int64, device=self.device)   # walk positions; the tail is never counted
        obs_all = count_totals(self.counts[g]) if observed else None
        for step, tensors, B, off, pos in walk_positions(self._eval_minibatches(group_indices_list, batch_size, None), g, n_g):
            seg = np.where(pos >= 0, code[pos], -1)   # a cut row (pos -1) is in no population
            if not (seg >= 0).any():
                continue   # nothing of this step is counted (eval mode: steps are independent of each other)
            rows = tensors[g]["rows"].long()
            ids = obs_ids[rows].contiguous()
            seg_d = torch.as_tensor(seg, dtype=torch.int32, device=self.device)
            lib = torch.log(obs_all.index_select(0, rows)).to(torch.float32).contiguous() if observed else None
            for smp, out in self._draws(step, tensors, B, n_samples, _noise):
                self.module.sample_count_stats(out, g, genes=dev_sel, library_size="latent" if observed else library_size, library=lib, key=key,
                                               sample=smp, cell_ids=ids, seg=seg_d, n_seg=n_seg, stats=stats, cell_total=totals[off:off + B[g]])
        ppc = ppc_table(stats.cpu().numpy().view(np.uint64), [sizes[k] * n_samples for k in range(n_seg)], prefix="ppc_")
        # the observed side: the populations' cells sorted by population, one segmented reduction + one chunked pass for the squares
        kept = np.nonzero(code >= 0)[0]
        order = kept[np.argsort(code[kept], kind="stable")]
        rows = torch.as_tensor(self._local_rows(g, cells[order]).astype(np.int32), device=self.device)
        sums = count_stats(self.counts[g], rows, sizes, genes=dev_sel).cpu().numpy()
        sq, tot = count_square_sums(self.counts[g], rows, sizes, genes=dev_sel, row_totals=True)
        obs = ppc_observed_columns(sums, sq.cpu().numpy(), sizes)
        return ppc_frame(names, sizes, index, obs, ppc, n_samples, cells, order, kept, tot.cpu().numpy(), totals[:n_g].cpu().numpy().view(np.uint64))

    @torch.no_grad()
    def expression_statistics(self, group_indices_list: List[List[int]], group: int, groupby=None, labels=None, gene_list=None, library_size="latent",
                              n_samples: int = 1, use_mean: bool = True, batch_size: Optional[int] = None, _noise=None):
        """What the model EXPECTS per population and gene of ONE group, split into its private and its shared part (the third read-out
        next to ``count_statistics``, what was observed, and ``posterior_predictive_check``, what the model draws): a pandas DataFrame
        with one row per (population, selected gene) and the columns

            population, gene, n_cells, n_samples
            mean, mean_private, mean_shared, mixing      the means over the population's cells of the four ``component`` values of
                                                         ``get_normalized_expression``: the NB mixture's mean pi * rate_private +
                                                         (1 - pi) * rate_shared, its two terms, and pi itself
            private_fraction                             sum of the private part / sum of the mixture mean (NaN where that is 0)
            var, var_private, var_shared, var_mixing     their unbiased sample variances over the same values (NaN for fewer than two)

        ``attrs["sums"]`` holds the fp64 table [populations, 8, n_sel] the columns are derived from (``data.expression_stats_table``):
        the sums of the four values and the sums of their squares.

        The summed values are the very fp32 numbers ``get_normalized_expression(group_indices_list, gene_list, library_size, component,
        n_samples=1, use_mean, batch_size)`` returns for those cells (same minibatch walk, same kernel front end), but no [n_cells,
        n_sel] matrix is stored or copied: one fused HIP entry point (spv_dec_expected_stats) decodes every minibatch and adds it into
        ONE fp64 table [populations, 8, n_sel]; only that table leaves the device.
        ``groupby`` / ``labels``: ``posterior_predictive_check``'s rules and errors -- None is one population "all", else the name of
        an ``adata.obs`` column or one label per cell of ``group_indices_list[group]``; the populations come in ``labels`` order
        (default: sorted unique labels; an unknown label is a KeyError); a cell outside every population is left out.
        ``gene_list``: None or this group's selection, as ``differential_expression`` takes it.
        ``library_size``: "latent" or a positive number, as ``get_normalized_expression`` means them, or "observed", as
        ``posterior_predictive_check`` means it: each cell decodes at the log of its observed total over ALL of the group's genes, so
        ``mean`` is on the raw-count scale of ``count_statistics``' ``raw_mean``.
        ``use_mean`` / ``n_samples``: ``get_normalized_expression``'s rules.  With sampled latents every draw adds its values to the
        table (``draw = step * n_samples + sample``): the statistics then run over n_cells * n_samples values.
        Cost of the arrangement: within a step the cells are sorted by population and each population's run is padded to a multiple of
        32 rows, so up to 31 padded rows are decoded per population present in a step; a ``batch_size`` well above 32 x the number of
        labels keeps that overhead small.
        Reproducibility: there are no floating-point atomics and every order of addition is fixed, so two calls with the same arguments
        agree bit for bit.  A different ``batch_size`` changes the order of summation (last bits) and, under a label PoE, which
        minibatch mates a cell is fused with (its values).  ``_noise`` (tests only): as ``get_normalized_expression`` takes it."""
        from .count_ops import count_totals

        library_size = check_ppc_library(library_size)
        observed = isinstance(library_size, str) and library_size == "observed"
        _what, _log_l, n_samples = check_expression_args("mixture", "latent" if observed else library_size, n_samples, use_mean)
        g = check_group(group)
        cells = np.asarray(group_indices_list[g]).astype(np.int64).ravel()
        n_g = len(cells)
        cell_labels = None if groupby is None else group_cell_labels(self.adata.obs, groupby, cells, g)
        names, sizes, code = ppc_segments(cell_labels, labels, n_cells=n_g)
        n_seg = len(names)
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        stats = torch.zeros((n_seg, 8, n_sel), dtype=torch.float64, device=self.device)
        obs_all = count_totals(self.counts[g]) if observed else None
        for step, tensors, B, _off, pos in walk_positions(self._eval_minibatches(group_indices_list, batch_size, None), g, n_g):
            seg = np.where(pos >= 0, code[pos], -1)   # a cut row (pos -1) is in no population
            perm, tile_seg, tile_n = expression_tile_plan(seg, n_seg)
            if not perm.size:
                continue   # nothing of this step is counted (eval mode: steps are independent of each other)
            plan = [torch.as_tensor(t, device=self.device) for t in (perm, tile_seg, tile_n)]
            lib = torch.log(obs_all.index_select(0, tensors[g]["rows"].long())).to(torch.float32).contiguous() if observed else None
            for _smp, out in self._draws(step, tensors, B, n_samples, _noise):
                self.module.expression_stats(out, g, genes=dev_sel, library_size="latent" if observed else library_size, library=lib, use_mean=use_mean,
                                             perm=plan[0], tile_seg=plan[1], tile_n=plan[2], n_seg=n_seg, stats=stats)
        sums = stats.cpu().numpy()
        table = expression_stats_table(sums, [sizes[k] * n_samples for k in range(n_seg)])
        return expression_stats_frame(names, sizes, index, table, n_samples, sums=sums)

    @torch.no_grad()
    def get_feature_correlation_matrix(self, group_indices_list: List[List[int]], group: int, gene_list=None, cells=None, component: str = "mixture",
                                       library_size="latent", n_samples: int = 1, use_mean: bool = True, correlation_type: str = "pearson",
                                       batch_size: Optional[int] = None, _noise=None):
        """Which genes of ONE group the model moves together (scvi-tools' ``get_feature_correlation_matrix``): the Pearson correlation
        of the decoded expression over the cells, a pandas DataFrame [n_sel, n_sel] labelled on both axes by the selected genes' names
        as ``get_loadings`` labels them (their positions when the AnnData has none).  ``component`` separates the question the way
        ``get_normalized_expression`` separates the values: "mixture" correlates the mixture's mean, "private" / "shared" the part of
        it the private / the shared factors drive, "mixing" the mixing weight.

        ``attrs``: ``mean`` and ``var`` (unbiased) of every selected gene, ``n_cells``, ``n_samples`` and ``sums`` = {"S": [n_sel],
        "C": [n_sel, n_sel]}, the fp64 tables sum x_i and sum x_i x_j everything is derived from (``data.correlation_table``: cov =
        (C - S S^T / n) / (n - 1) with n = n_cells * n_samples; a gene without variance has NaN in its row and column, the diagonal is
        exactly 1 elsewhere; the one-pass formula loses a gene whose relative spread is below about 2 sqrt(n 2^-53)).

        The correlated values are the very fp32 numbers ``get_normalized_expression(group_indices_list, gene_list, library_size,
        component, n_samples=1, use_mean, batch_size)`` returns for those cells (same minibatch walk, same kernel), but no [n_cells,
        n_sel] matrix is stored or copied: per step ONE [batch, n_sel] fp32 block is decoded on the device (``module.
        expected_expression``, reused from step to step) and ONE HIP entry point (spv_gram_f64, an fp64 MFMA kernel) adds its counted
        rows into the two tables.  Every product of two fp32 values is exact in fp64, so the tables carry summation error only.  Only
        S and C leave the device.
        ``gene_list``: None or this group's selection, as ``differential_expression`` takes it; at most 4096 genes (the table is
        n_sel^2 x 8 bytes).  ``cells``: None (all of ``group_indices_list[group]``) or adata row numbers of cells of it, resolved like
        ``idx1`` of ``differential_expression`` with its errors; ALL cells are still walked -- a cell's latents depend on its minibatch
        mates -- and only steps without a counted cell are skipped.  ``library_size`` / ``use_mean`` / ``n_samples``:
        ``get_normalized_expression``'s rules; with sampled latents every draw adds its block (``draw = step * n_samples + sample``),
        so the correlation runs over n_cells * n_samples rows, scvi-tools' flattening.  ``correlation_type``: "pearson"; "spearman"
        is a NotImplementedError (ranks need a gene's whole column).
        Reproducibility: no floating-point atomics, every order of addition fixed: two calls with the same arguments agree bit for
        bit, and the frame is symmetric in bits.  ``_noise`` (tests only): as ``get_normalized_expression`` takes it."""
        import pandas as pd

        from .gram_ops import gram_accumulate, gram_workspace

        check_correlation_args(correlation_type)
        _what, _log_l, n_samples = check_expression_args(component, library_size, n_samples, use_mean)
        g = check_group(group)
        counted = correlation_cells(group_indices_list[g], cells, group=g)
        n_g = len(counted)
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        check_correlation_args(correlation_type, n_sel)
        S = torch.zeros(n_sel, dtype=torch.float64, device=self.device)
        Cm = torch.zeros((n_sel, n_sel), dtype=torch.float64, device=self.device)
        blk = ws = None
        for step, tensors, B, _off, pos in walk_positions(self._eval_minibatches(group_indices_list, batch_size, None), g, n_g):
            use = np.nonzero((pos >= 0) & counted[np.maximum(pos, 0)])[0]   # a cut row (pos -1) is never counted
            if not use.size:
                continue   # eval mode: steps are independent of each other
            rows = None if use.size == B[g] else torch.as_tensor(use.astype(np.int32), device=self.device)
            if blk is None or blk.shape[0] < B[g]:
                blk = torch.empty((B[g], n_sel), dtype=torch.float32, device=self.device)
                ws = gram_workspace(n_sel, B[g], self.device)   # the largest a step of this walk can need: it grows with the counted rows
            for _smp, out in self._draws(step, tensors, B, n_samples, _noise):
                x = self.module.expected_expression(out, g, genes=dev_sel, what=component, library_size=library_size, use_mean=use_mean, out=blk)
                gram_accumulate(x, rows=rows, sums=S, gram=Cm, ws=ws)
        n_cells = int(counted.sum())
        sums = {"S": S.cpu().numpy(), "C": Cm.cpu().numpy()}
        table = correlation_table(sums["S"], sums["C"], n_cells * n_samples)
        frame = pd.DataFrame(table["corr"], index=index, columns=index)
        frame.attrs.update(mean=table["mean"], var=table["var"], n_cells=n_cells, n_samples=n_samples, sums=sums)
        return frame

    def _spearman_frame(self, block: torch.Tensor, ties: torch.Tensor, index, n_cells: int, n_samples: int):
        """The shared tail of the two Spearman read-outs.  ``block``: the fp32 device tensor [rows, n_sel] of rank-transformed values
        (every column sums to 0), ``ties`` the transform's int64 [n_sel] -> the frame of ``data.spearman_table`` over the block's Gram,
        added up ``SPEARMAN_GRAM_ROWS`` rows at a time."""
        import pandas as pd

        from .gram_ops import gram_accumulate, gram_workspace

        n, n_sel = int(block.shape[0]), int(block.shape[1])
        S = torch.zeros(n_sel, dtype=torch.float64, device=self.device)
        Cm = torch.zeros((n_sel, n_sel), dtype=torch.float64, device=self.device)
        ws = gram_workspace(n_sel, min(n, SPEARMAN_GRAM_ROWS), self.device)   # the largest a chunk can need: it grows with the counted rows
        for r0 in range(0, n, SPEARMAN_GRAM_ROWS):
            gram_accumulate(block[r0:r0 + SPEARMAN_GRAM_ROWS], sums=S, gram=Cm, ws=ws)
        sums = {"S": S.cpu().numpy(), "C": Cm.cpu().numpy()}
        table = spearman_table(sums["C"], n)
        frame = pd.DataFrame(table["corr"], index=index, columns=index)
        frame.attrs.update(n_cells=n_cells, n_samples=n_samples, exact=n <= SPEARMAN_EXACT_ROWS, ties=ties.cpu().numpy(), sums=sums)
        return frame

    @torch.no_grad()
    def get_feature_spearman_matrix(self, group_indices_list: List[List[int]], group: int, gene_list=None, cells=None, component: str = "mixture",
                                    library_size="latent", n_samples: int = 1, use_mean: bool = True, batch_size: Optional[int] = None, _noise=None):
        """Spearman's rank correlation of the decoded expression of ONE group's genes over the cells (scvi-tools'
        ``get_feature_correlation_matrix(correlation_type="spearman")``): a pandas DataFrame [n_sel, n_sel] labelled on both axes by the
        selected genes, the Pearson correlation of the genes' average ranks.  Arguments, checks and errors are exactly those of
        ``get_feature_correlation_matrix`` (without ``correlation_type``), and the ranked values are the very fp32 numbers
        ``get_normalized_expression`` returns for the same arguments: same minibatch walk, same kernel.

        How it is computed: every step's counted rows of the decoded [batch, n_sel] block are copied on the device into ONE fp32 block
        [n_cells * n_samples, n_sel] (with sampled latents, draw ``sample`` of the counted cell at rank i among the counted cells is row
        ``sample * n_cells + i``: the correlation runs over n_cells * n_samples rows, scvi-tools' flattening).  ``rank_ops.
        rank_transform`` then replaces every column IN PLACE by 2 * average rank - (rows + 1) (spv_rank_values: the column sort of
        ``rank_genes_groups``, exact integers), and spv_gram_f64 adds the block's Gram up in row chunks.
        ``attrs``: ``n_cells``, ``n_samples``, ``exact`` (rows <= 208 063: every sum is then an exact integer whatever the order of
        addition, ``data.spearman_table``), ``ties`` (int64 [n_sel]: the sum of t^3 - t over each gene's runs of equal values, 0 for
        a gene without ties) and ``sums`` = {"S": [n_sel], "C": [n_sel, n_sel]} straight from the kernel -- S is exactly 0.  A gene
        whose values are all equal has NaN in its row and column; the diagonal is exactly 1 elsewhere; the frame is symmetric in bits
        and two calls agree bit for bit.
        Limits, each a ValueError ahead of any device work: at most 4096 genes and at most 2^20 rows (cells * n_samples).
        Device memory, in bytes: the block 4 * rows * n_sel; the sort's workspace at most 8192 + max(``rank_ops.WS_BUDGET_BYTES``,
        20 * rows) (1 GiB by default: the genes are walked in slabs that fit); the table 8 * n_sel^2 (plus n_sel * 8 for S and one
        decoded [batch, n_sel] block)."""
        _what, _log_l, n_samples = check_expression_args(component, library_size, n_samples, use_mean)
        g = check_group(group)
        counted = correlation_cells(group_indices_list[g], cells, group=g)
        n_g, n_cells = len(counted), int(counted.sum())
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        check_spearman_shape(n_cells * n_samples, n_sel, "get_feature_spearman_matrix")
        from .ops import GroupCounts
        from .rank_ops import rank_transform

        place = np.cumsum(counted) - 1   # position in the group's read-out -> row among the counted cells
        block = torch.empty((n_cells * n_samples, n_sel), dtype=torch.float32, device=self.device)
        blk = None
        for step, tensors, B, _off, pos in walk_positions(self._eval_minibatches(group_indices_list, batch_size, None), g, n_g):
            use = np.nonzero((pos >= 0) & counted[np.maximum(pos, 0)])[0]   # a cut row (pos -1) is never counted
            if not use.size:
                continue   # eval mode: steps are independent of each other
            src = torch.as_tensor(use, device=self.device)
            dst = torch.as_tensor(place[pos[use]], device=self.device)
            if blk is None or blk.shape[0] < B[g]:
                blk = torch.empty((B[g], n_sel), dtype=torch.float32, device=self.device)
            for smp, out in self._draws(step, tensors, B, n_samples, _noise):
                x = self.module.expected_expression(out, g, genes=dev_sel, what=component, library_size=library_size, use_mean=use_mean, out=blk)
                block.index_copy_(0, dst + smp * n_cells, x.index_select(0, src))
        rows = torch.arange(block.shape[0], dtype=torch.int32, device=self.device)
        _block, ties = rank_transform(GroupCounts(block, n_sel, 0), rows, out=block, ties=True)
        return self._spearman_frame(block, ties, index, n_cells, n_samples)

    @torch.no_grad()
    def count_spearman_matrix(self, group_indices_list: List[List[int]], group: int, gene_list=None, cells=None, normalize: bool = True,
                              target_sum: float = 1e4):
        """Spearman's rank correlation of the OBSERVED counts of ONE group's genes over the cells: the frame of
        ``get_feature_spearman_matrix`` -- same labels, same ``attrs`` (``n_samples`` is 1) -- for the data itself.  It needs no
        trained model and decodes nothing: the companion of ``count_statistics`` and ``rank_genes_groups``.
        The ranked keys are ``rank_genes_groups``': ``normalize=True`` ranks count * fp32(target_sum / the cell's total over ALL of the
        group's genes) (a cell without counts gets the weight 0; log1p is monotone, so these are the ranks of log-normalised data),
        ``normalize=False`` the raw counts (``target_sum`` is still checked).  ``gene_list``: this group's selection, as
        ``rank_genes_groups`` takes it; ``cells``: None (all of ``group_indices_list[group]``) or adata row numbers of cells of it,
        resolved like ``cells`` of ``get_feature_correlation_matrix`` with its errors; the rows are ranked in the group's order.
        Single-cell counts are mostly zeros: all zero keys of a gene form one run at the bottom that is never stored or sorted
        (spv_rank_values_stage), which is what this method is fast for.  Every device output is an integer, so dense and sparse
        ``counts_storage`` give the same frame bit for bit and two calls agree bit for bit.
        Limits, each a ValueError ahead of any device work: at most 4096 genes and 2^20 cells.  Device memory, in bytes: the rank
        block 4 * cells * n_sel, the sort's workspace at most 8192 + max(``rank_ops.WS_BUDGET_BYTES``, 20 * cells), the table 8 * n_sel^2."""
        from .count_ops import count_totals
        from .rank_ops import rank_transform

        target_sum = check_target_sum(target_sum)
        g = check_group(group)
        counted = correlation_cells(group_indices_list[g], cells, group=g)
        listed = np.asarray(group_indices_list[g]).astype(np.int64).ravel()[counted]
        _sel, dev_sel, n_sel, index = self._genes(g, gene_list, own=True)
        check_spearman_shape(len(listed), n_sel, "count_spearman_matrix")
        rows = torch.as_tensor(self._local_rows(g, listed).astype(np.int32), device=self.device)
        w = None
        if normalize:
            total = count_totals(self.counts[g]).index_select(0, rows.long())
            w = torch.where(total > 0, target_sum / total, torch.zeros_like(total)).to(torch.float32)
        block, ties = rank_transform(self.counts[g], rows, w=w, genes=dev_sel, ties=True)
        return self._spearman_frame(block, ties, index, len(listed), 1)

    @torch.no_grad()
    def count_pca(self, group_indices_list: List[List[int]], n_comps: int = 50, group: Optional[int] = None, gene_list=None, normalize: bool = True,
                  target_sum: float = 1e4, scale: bool = False, tol: float = 1e-4, seed: int = 0) -> PcaResult:
        """Principal components of the log-normalised OBSERVED counts: scanpy's normalize_total -> log1p -> pca on the resident count
        matrices, which never leave the device and are never expanded -- the matrix of log-normalised values is made in registers
        inside two fused fp32 MFMA kernels (``pca_ops``).  It needs no trained model and decodes nothing: the
        companion of ``count_statistics``, ``rank_genes_groups`` and ``count_spearman_matrix``, with their weights -- count *
        fp32(target_sum / the cell's total over ALL of its group's genes), a cell without counts gets the weight 0;
        ``normalize=False`` takes log1p of the raw counts (``target_sum`` is still checked).
        ``group=None``: the JOINT PCA both groups share, which is what ``compute_transport_plan`` wants.  Rows are group 0's listed cells,
        then group 1's; columns are PAIRED genes.  By default the pairing strips the ``"<group key>_"`` prefix that prepare_adatas adds
        (keys: ``uns["groups_mapping"]``, names: ``var_names`` / ``uns["groups_var_names"]``) and keeps the names both groups have, in
        group 0's order; ``gene_list=[names0, names1]`` pairs by position (equal lengths, no repeats).  Without names and without
        ``gene_list`` it is a ValueError -- nothing is guessed.  ``group=g``: one group's own PCA over its genes (or ``gene_list[g]``).
        ``scale=True`` divides every gene by its standard deviation (ddof 1; a gene without variance gets the scale 0).  There is no
        clipping: scanpy's ``max_value`` is not built.
        The eigenpairs come from a block Lanczos iteration (``pca_ops.block_lanczos``) with the block min(64, round_up(n_comps + 8, 16), 16 * (genes // 16));
        it stops when every residual || X^T X v - theta v || is at most ``tol`` * theta_1.  Not reaching that is reported
        (``converged=False``), not raised.  The reported ``residuals`` are those of the fp32 vectors actually returned, whose largest
        |loading| is positive (ties: the smaller gene index).  Deterministic in ``seed``.
        Limits, each a ValueError ahead of any device work: 1 <= n_comps <= 56, n_comps below the number of cells and of genes, at
        least 16 genes, at least 2 cells, and round_up(n_comps, 16) <= the number of genes (the iteration's block is a multiple of 16
        and cannot be wider than the operator; with fewer genes than the default block it shrinks to the largest multiple that fits).  Device memory beyond the counts: the scores and one block of 4 * cells * 64 bytes each, the
        basis of at most 2 * 12 * 64 * 8 * genes bytes, and a workspace of at most 16 * round_up(genes, 64) * 256 bytes."""
        n_genes = [int(self.module.input_dims[k]) for k in range(2)]
        plan = pca_plan(self.adata, n_genes, self.obs_idx, group_indices_list, n_comps=n_comps, group=group, gene_list=gene_list,
                        normalize=normalize, target_sum=target_sum, scale=scale, tol=tol, seed=seed)
        return _run_count_pca(self.counts, plan, self.device)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _latents_on_device(self, group_indices_list, latent: str = "shared", give_mean: bool = True, batch_size: Optional[int] = None, _noise=None) -> dict:
        """{0: fp32 device tensor [n_cells_0, n_latent], 1: ...}: the ``latent`` ("shared" | "private") embedding of every cell of
        ``group_indices_list[g]``, from the minibatch walk of ``get_latent_representation``, never copied to the host.  ``give_mean``: the
        posterior means (``logtheta_loc``; deterministic), else the sampled ``log_z`` / ``logtheta_log_z`` -- what
        ``get_latent_representation(normalized=False)`` returns under the same ``_noise``."""
        stats, key = ("poe_stats", "logtheta_loc" if give_mean else "logtheta_log_z") if latent == "shared" else ("private_stats", "logtheta_loc" if give_mean else "log_z")
        blocks = RowBlocks([len(g) for g in group_indices_list], False)
        for step, tensors, (B0, B1) in self._eval_minibatches(group_indices_list, batch_size, None):
            out = self._infer(tensors, _noise, step, B0, B1)
            blocks.add([out[stats][g][key].float() for g in range(2)])
        return {g: z.contiguous() for g, z in blocks.result().items()}

    @torch.no_grad()
    def latent_neighbors(self, group_indices_list: List[List[int]], k: int = 15, query=0, target=1, latent: str = "shared", give_mean: bool = True,
                         include_self: bool = False, batch_size: Optional[int] = None, return_numpy: bool = True, _noise=None) -> dict:
        """Each query cell's ``k`` nearest target cells in latent space, exact (the fused kernel spv_knn: no queries x targets matrix
        exists at any time) -> {"indices" int32 [n_query, k]: positions into the target cells' order, ascending in
        (distance, position), -1 where fewer than k exist; "distances" fp32 [n_query, k]: Euclidean (the square root of the kernel's
        values; inf next to a -1); "query_obs" / "target_obs": the adata row numbers of the query and target cells, so
        ``target_obs[indices]`` are adata rows}.
        ``query`` / ``target``: 0, 1 or "both" (group 0's cells of ``group_indices_list``, then group 1's).  ``latent``: "shared" or
        "private"; "private" only within one group (query == target, not "both": the groups' private spaces are not comparable).
        ``give_mean``: neighbours among the posterior means (deterministic: two calls agree bit for bit), else among one sampled embedding,
        the rows of ``get_latent_representation(normalized=False)``.  When every query cell is also a target cell its own row is left
        out, unless ``include_self``.  ``return_numpy=False`` keeps the two arrays on the device.  ``_noise`` (tests only): as
        ``get_latent_representation`` takes it."""
        k, q_groups, t_groups, contained = check_neighbor_args(k, query, target, latent)
        from .knn_ops import knn
        z = self._latents_on_device(group_indices_list, latent, give_mean, batch_size, _noise)
        Q, T = (z[gs[0]] if len(gs) == 1 else torch.cat([z[g] for g in gs]) for gs in (q_groups, t_groups))
        sizes = [int(z[g].shape[0]) for g in range(2)]
        exclude = None
        if contained and not include_self:
            exclude = torch.as_tensor(neighbor_self_positions(q_groups, t_groups, sizes), device=self.device)
        if Q.shape[0] < 1:
            raise ValueError("latent_neighbors: the query set is empty")
        idx, d2 = knn(Q, T, k, exclude=exclude)
        dist = torch.sqrt(d2)
        obs = [np.concatenate([np.asarray(group_indices_list[g], dtype=np.int64) for g in gs]) for gs in (q_groups, t_groups)]
        return {"indices": idx.cpu().numpy() if return_numpy else idx, "distances": dist.cpu().numpy() if return_numpy else dist,
                "query_obs": obs[0], "target_obs": obs[1]}

    def transfer_labels(self, group_indices_list: List[List[int]], source=1, target=0, labels="cell_type", k: int = 15, **neighbor_kwargs):
        """Labels for the ``target`` group's cells by a vote of their ``k`` nearest ``source`` cells in latent space
        (``latent_neighbors(query=target, target=source, k=k, **neighbor_kwargs)``; ``data.vote_labels``: uniform weights, ties to the
        label that sorts first) -> DataFrame indexed by the target cells' ``obs_names`` (their adata row numbers without any) with
        ``predicted`` (None for a cell without a valid neighbour), ``confidence`` (the share of the cell's valid neighbours that voted for
        it) and ``n_neighbors`` (the valid ones).  ``source`` / ``target``: 0 or 1.  ``labels``: an ``obs`` column, or an array with one
        entry per source cell."""
        src, tgt = check_group(source), check_group(target)
        check_neighbor_args(k, tgt, src, neighbor_kwargs.get("latent", "shared"))
        if "query" in neighbor_kwargs or "target" in neighbor_kwargs or "return_numpy" in neighbor_kwargs:
            raise ValueError("transfer_labels sets query, target and return_numpy itself")
        cells = np.asarray(group_indices_list[src], dtype=np.int64)
        cats, codes = np.unique(group_cell_labels(self.adata.obs, labels, cells, src), return_inverse=True)
        nb = self.latent_neighbors(group_indices_list, k=k, query=tgt, target=src, **neighbor_kwargs)
        predicted, confidence, n_valid = vote_labels(nb["indices"], codes, len(cats))
        names = getattr(self.adata, "obs_names", None)
        return transfer_frame(nb["query_obs"] if names is None else np.asarray(names)[nb["query_obs"]], cats, predicted, confidence, n_valid)

    _SILHOUETTE_TABLE_BYTES = 256 << 20   # cap on the fp64 [cells of a query block, segments] table of one kernel call plus its workspace: a memory condition, not a measurement

    @torch.no_grad()
    def latent_silhouette(self, group_indices_list: List[List[int]], labels="cell_type", cells="both", latent: str = "shared", give_mean: bool = True,
                          batch_size: Optional[int] = None, _noise=None):
        """The exact silhouette width of every cell of ``cells`` in latent space, by label and by group within its label (scIB's
        ``silhouette`` and ``silhouette_batch``), from the fused kernel spv_silhouette_sums: no cells x cells matrix exists at any time and
        nothing is subsampled.  Returns a DataFrame with one row per cell, in ``group_indices_list`` order (group
        0's cells, then group 1's), indexed by ``obs_names`` (the adata row numbers without any):
            group, label          the cell's group and label
            a, b                  its mean Euclidean distance to the other cells of its label, and to the cells of the nearest other label
            silhouette_label      (b - a) / max(a, b): ``sklearn.metrics.silhouette_samples``, 0 for the only cell of a label (a is NaN
                                  there) and where max(a, b) = 0; NaN, like b, when the selection has one label only
            nearest_label         the label that gives b, the one that sorts first on ties
            silhouette_group      the same width inside the cell's label, its own group against the other group; 0 for the only cell of
                                  its (label, group); NaN for a label with cells in one group only, so for every cell when ``cells``
                                  is 0 or 1
        ``attrs``: ``label_asw`` = (mean silhouette_label + 1) / 2; ``group_asw`` = the mean, over the labels present in both groups, of
        the label's mean 1 - |silhouette_group| (NaN without such a label); ``per_label``: a frame per label with its cells in each group
        (``n_group0`` / ``n_group1``), its mean ``silhouette_label`` and its ``group_mixing`` (the 1 - |silhouette_group| mean).
        ``labels``: an ``obs`` column, or an array with one entry per cell of the selection; at most 128 distinct labels.
        ``cells``: 0, 1 or "both".  ``latent``: "shared" or "private", "private" only with ``cells`` 0 or 1.  ``give_mean``: the
        posterior means (deterministic: two calls agree bit for bit), else one sampled embedding, the rows of
        ``get_latent_representation(normalized=False)``.  Non-finite latents are a ValueError.  ``_noise`` (tests only): as
        ``get_latent_representation`` takes it.
        The distances are the ones ``latent_neighbors`` reports, bit for bit; each is widened to fp64 and summed per (label, group) in a
        fixed order, and every value of the frame is computed from those sums in fp64 on the host: only the [cells, 2 x labels] table of
        sums leaves the device.  Very many cells go through the kernel in blocks of query cells whose table, with the kernel's workspace,
        stays within 256 MiB; a cell's sums do not depend on the other cells of its block, so the blocking does not change a bit."""
        groups = check_silhouette_args(cells, latent)
        from .silhouette_ops import segment_distance_sums, silhouette_splits
        obs_rows = np.concatenate([np.asarray(group_indices_list[g], dtype=np.int64).ravel() for g in groups])
        group_of_cell = np.concatenate([np.full(len(group_indices_list[g]), g, dtype=np.int64) for g in groups])
        n = len(obs_rows)
        if n < 1:
            raise ValueError("latent_silhouette: the selection has no cells")
        if not isinstance(labels, str) and np.asarray(labels).ravel().shape[0] != n:
            raise ValueError(f"labels: an array must hold one label per cell of the selection ({n}), got {np.asarray(labels).ravel().shape[0]}")
        cats, codes = np.unique(group_cell_labels(self.adata.obs, labels, obs_rows, groups[0]), return_inverse=True)
        if len(cats) > SILHOUETTE_MAX_LABELS:
            raise ValueError(f"latent_silhouette takes at most {SILHOUETTE_MAX_LABELS} distinct labels, got {len(cats)}")
        perm, seg_ptr, sizes = silhouette_segments(codes, group_of_cell, len(cats))
        z = self._latents_on_device(group_indices_list, latent, give_mean, batch_size, _noise)
        X = z[groups[0]] if len(groups) == 1 else torch.cat([z[g] for g in groups])
        if not bool(torch.isfinite(X).all()):
            raise ValueError("latent_silhouette: the latents hold non-finite values")
        cand = X.index_select(0, torch.as_tensor(perm, device=self.device))
        ptr_dev = torch.as_tensor(seg_ptr, device=self.device)
        n_seg = len(sizes)
        n_split = silhouette_splits(n, n)   # ONE chunk count, from the whole selection, for every query block: the sums must not depend on the blocking
        row_bytes = 8 * n_seg * (1 + (n_split if n_split > 1 else 0))   # a query's row of the table and of every chunk's slab of the workspace
        S = np.empty((n, n_seg), dtype=np.float64)
        for b0, b1 in silhouette_query_blocks(n, row_bytes, self._SILHOUETTE_TABLE_BYTES):
            S[b0:b1] = segment_distance_sums(X[b0:b1], cand, ptr_dev, n_split=n_split).cpu().numpy()
        names = getattr(self.adata, "obs_names", None)
        return silhouette_frame(obs_rows if names is None else np.asarray(names)[obs_rows], group_of_cell, cats, codes, sizes,
                                silhouette_table(S, sizes, codes, group_of_cell))

    @torch.no_grad()
    def latent_tsne(self, group_indices_list: List[List[int]], cells="both", latent: str = "shared", give_mean: bool = True, perplexity: float = 30.0,
                    n_components: int = 2, n_iter: int = 1000, init="pca", seed: int = 0, batch_size: Optional[int] = None, _noise=None, **schedule):
        """An exact t-SNE layout of the cells of ``cells`` in latent space, for looking at the embedding: ``tsne_ops.tsne`` on the very rows
        ``latent_neighbors`` sees, which never leave the device.  The repulsive half of every gradient runs over
        all pairs on the fused pair scan: no tree or grid approximation, no cells x cells matrix, and two calls agree bit for bit.
        Returns a DataFrame with one row per cell, in ``group_indices_list`` order (group 0's cells, then group 1's), indexed by
        ``obs_names`` (the adata row numbers without any): ``group`` and ``tsne_1`` .. ``tsne_n`` (fp32, centred).  ``attrs``:
        ``kl_divergence`` (of the returned layout), ``kl_history`` ([steps taken, KL] every ``kl_every`` steps), ``perplexity``,
        ``n_neighbors``.
        ``cells``: 0, 1 or "both".  ``latent``: "shared" or "private", "private" only with ``cells`` 0 or 1.  ``give_mean``: the posterior
        means, else one sampled embedding.  ``perplexity`` in [2, 32]: the affinities rest on each cell's min(3 perplexity, 64, n - 1)
        exact nearest neighbours, the most the k-NN kernel returns, where scikit-learn's exact method uses all others.  ``n_components``
        in [1, 4].  ``n_iter`` steps are always all taken: there is no early stop.  ``init``: "pca", "random" (``seed``) or an array.
        ``schedule``: ``early_exaggeration`` (12), ``exaggeration_iter`` (250), ``learning_rate`` ("auto"), ``momentum`` ((0.5, 0.8)),
        ``min_gain`` (0.01), ``kl_every`` (50): scikit-learn's exact-method defaults.  Non-finite latents are a ValueError.  ``_noise``
        (tests only): as ``get_latent_representation`` takes it."""
        groups = check_silhouette_args(cells, latent)
        schedule = check_tsne_schedule(schedule)
        obs_rows = np.concatenate([np.asarray(group_indices_list[g], dtype=np.int64).ravel() for g in groups])
        group_of_cell = np.concatenate([np.full(len(group_indices_list[g]), g, dtype=np.int64) for g in groups])
        check_tsne_args(len(obs_rows), perplexity, n_components, n_iter, init, seed, **schedule)
        from .tsne_ops import tsne
        z = self._latents_on_device(group_indices_list, latent, give_mean, batch_size, _noise)
        X = z[groups[0]] if len(groups) == 1 else torch.cat([z[g] for g in groups])
        if not bool(torch.isfinite(X).all()):
            raise ValueError("latent_tsne: the latents hold non-finite values")
        result = tsne(X, perplexity=perplexity, n_components=n_components, n_iter=n_iter, init=init, seed=seed, **schedule)
        names = getattr(self.adata, "obs_names", None)
        return tsne_frame(obs_rows if names is None else np.asarray(names)[obs_rows], group_of_cell, result, perplexity)

    @torch.no_grad()
    def latent_lisi(self, group_indices_list: List[List[int]], labels="cell_type", cells="both", latent: str = "shared", give_mean: bool = True,
                    perplexity: float = 30, batch_size: Optional[int] = None, _noise=None):
        """The LISI scores (Korsunsky et al., the Harmony paper) of every cell of ``cells`` in latent space: the effective number of groups
        (iLISI) and of labels (cLISI) in the cell's perplexity-weighted neighbourhood, from the paged exact k-NN spv_knn_paged and the
        fused kernel spv_lisi, which calibrates each cell once for both.  No cells x cells matrix exists at any
        time and nothing is subsampled.  Returns a DataFrame with one row per cell, in ``group_indices_list`` order (group 0's cells, then
        group 1's), indexed by ``obs_names`` (the adata row numbers without any):
            group, label          the cell's group and label (label None with ``labels=None``)
            ilisi                 LISI over group membership, in [1, 2]; NaN when ``cells`` is 0 or 1
            clisi                 LISI over the labels, in [1, number of labels]; left out with ``labels=None``
            n_neighbors           the neighbours that counted; converged: False where the 50 updates of the search ran out
        Neighbours: k = min(int(3 perplexity) - 1, n - 1) per cell, itself left out: 89 at the standard perplexity 30.  ``perplexity`` must
        give 1 <= k <= 256, else ValueError before any device work.
        ``attrs``: ``ilisi_median`` / ``clisi_median`` (nan-medians); ``ilisi_scaled`` = (median - 1) / (n_groups - 1) and ``clisi_scaled``
        = (n_labels - median) / (n_labels - 1), scIB's scaling to [0, 1], larger is better, NaN with one group / one label; ``per_label``:
        a frame per label with its cells in each group and its median ``ilisi`` and ``clisi``; ``perplexity``, ``n_neighbors`` (k),
        ``n_unconverged``.
        ``labels`` / ``cells`` / ``latent`` / ``give_mean`` / ``batch_size`` / ``_noise``: as ``latent_silhouette`` takes them (any number
        of distinct labels).  Non-finite latents are a ValueError.  The distances are the ones ``latent_neighbors`` reports, bit for bit;
        every order of addition is fixed, so with ``give_mean`` two calls agree bit for bit."""
        groups = check_silhouette_args(cells, latent)
        obs_rows = np.concatenate([np.asarray(group_indices_list[g], dtype=np.int64).ravel() for g in groups])
        group_of_cell = np.concatenate([np.full(len(group_indices_list[g]), g, dtype=np.int64) for g in groups])
        n = len(obs_rows)
        if n < 1:
            raise ValueError("latent_lisi: the selection has no cells")
        k = check_lisi_args(n, perplexity)
        cats = codes = None
        if labels is not None:
            if not isinstance(labels, str) and np.asarray(labels).ravel().shape[0] != n:
                raise ValueError(f"labels: an array must hold one label per cell of the selection ({n}), got {np.asarray(labels).ravel().shape[0]}")
            cats, codes = np.unique(group_cell_labels(self.adata.obs, labels, obs_rows, groups[0]), return_inverse=True)
        from .knn_ops import knn_paged
        from .lisi_ops import lisi
        z = self._latents_on_device(group_indices_list, latent, give_mean, batch_size, _noise)
        X = z[groups[0]] if len(groups) == 1 else torch.cat([z[g] for g in groups])
        if not bool(torch.isfinite(X).all()):
            raise ValueError("latent_lisi: the latents hold non-finite values")
        idx, d2 = knn_paged(X, X, k, exclude=torch.arange(n, dtype=torch.int32, device=self.device))
        sets = [group_of_cell] + ([] if codes is None else [codes])
        out, _beta, n_valid, converged = lisi(idx, d2, torch.as_tensor(np.stack(sets).astype(np.int32), device=self.device), perplexity)
        out = out.cpu().numpy()
        names = getattr(self.adata, "obs_names", None)
        return lisi_frame(obs_rows if names is None else np.asarray(names)[obs_rows], group_of_cell, cats, codes, out[0] if len(groups) > 1 else None,
                          None if codes is None else out[1], n_valid.cpu().numpy(), converged.cpu().numpy(), perplexity, k)

    def integration_scores(self, group_indices_list: List[List[int]], labels="cell_type", **kwargs) -> dict:
        """How well the two groups are integrated in latent space, scIB's two silhouette scores from ONE ``latent_silhouette`` call
        (``kwargs`` go to it) -> {"label_asw": do the labels stay apart, in [0, 1], larger is better; "group_asw": do the groups mix
        within each label, in [0, 1], larger is better, NaN when no label has cells in both groups; "per_label": the frame of the parts}."""
        check_silhouette_args(kwargs.get("cells", "both"), kwargs.get("latent", "shared"))
        attrs = self.latent_silhouette(group_indices_list, labels=labels, **kwargs).attrs
        return {"label_asw": attrs["label_asw"], "group_asw": attrs["group_asw"], "per_label": attrs["per_label"]}

    def get_loadings(self) -> dict:
        """:652-677: per-gene weights of the linear decoder, {(group, "private" | "shared"): DataFrame [genes, latent dims]}
        with the reference's column names ``Z_private_{n}`` / ``Z_shared_{n}`` and the group's own var_names as the index
        (``adata.var_names``, or ``adata.uns["groups_var_names"]``; a plain RangeIndex when the duck-typed input has neither)."""
        import pandas as pd

        out = {}
        all_names = group_var_names(self.adata, len(self.module.input_dims))
        for i in range(len(self.module.input_dims)):
            names = all_names[i]
            cols = {"private": [f"Z_private_{n}" for n in range(self.module.n_dimensions_private)],
                    "shared": [f"Z_shared_{n}" for n in range(self.module.n_dimensions_shared)]}
            for t in ("private", "shared"):
                out[(i, t)] = pd.DataFrame(self.module.get_loadings(i, t), index=names, columns=cols[t])
        return out

    # ------------------------------------------------------------------------------------------
    def save(self, dir_path: str, prefix: Optional[str] = None, overwrite: bool = False, save_anndata: bool = False, **anndata_write_kwargs) -> None:
        """``spvipes.save("spvipes_model")`` (docs/notebooks/Tutorial.ipynb:487; inherited scvi-tools 0.20.0 ``BaseModelClass.save``):
        creates ``dir_path`` (an existing one is an error unless ``overwrite``) and writes ``{prefix}model.pt`` =
        ``{"model_state_dict", "var_names", "attr_dict"}``.  The state_dict carries the reference's parameter names (BatchNorm
        buffers included), so the file's weights load into the reference module and back; ``attr_dict`` holds the constructor
        arguments (``init_params_``), the ``setup_anndata`` arguments, ``is_trained_`` and the training history."""
        import os

        if os.path.exists(dir_path) and not overwrite:
            raise ValueError(f"{dir_path} already exists. Please provide an unexisting directory for saving.")
        if save_anndata:
            raise NotImplementedError("save_anndata=True needs anndata's writer, which is outside this build: keep the AnnData yourself and pass it to load()")
        os.makedirs(dir_path, exist_ok=True)
        var_names = getattr(self.adata, "var_names", None)
        attr = {"init_params_": dict(self.init_params_), "setup_args_": dict(self._setup), "is_trained_": bool(self.is_trained_),
                "history_": {k: list(v) for k, v in self.history.items()}}
        torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in self.module.state_dict().items()},
                    "var_names": None if var_names is None else np.asarray(var_names).astype(str), "attr_dict": attr},
                   os.path.join(dir_path, f"{prefix or ''}model.pt"))

    @classmethod
    def load(cls, dir_path: str, adata=None, use_gpu=None, prefix: Optional[str] = None, backup_url: Optional[str] = None,
             device: Optional[str] = None) -> "spVIPES":
        """``spVIPES.load("spvipes_model", adata=adata)`` (Tutorial.ipynb:538; scvi-tools ``BaseModelClass.load``): rebuilds the
        model from the saved constructor arguments on ``adata`` (registering it with the saved ``setup_anndata`` arguments when
        it has not been set up), loads the state_dict, leaves the module in eval mode.  ``adata`` is required (the AnnData is
        never written by this build); ``use_gpu`` is accepted and ignored, ``backup_url`` is not supported (no network)."""
        import os
        import warnings

        path = os.path.join(dir_path, f"{prefix or ''}model.pt")
        if not os.path.exists(path):
            raise ValueError(f"Failed to load model file at {path}. If attempting to load a saved model from <v0.15.0, please use the util function `convert_legacy_save` to convert to an updated format.")
        if adata is None:
            raise ValueError("Save path contains no saved anndata and no adata was passed.")
        blob = torch.load(path, map_location="cpu", weights_only=False)
        attr = blob["attr_dict"]
        if _SETUP_KEY not in adata.uns:
            cls.setup_anndata(adata, **attr["setup_args_"])
        saved_names, names = blob.get("var_names"), getattr(adata, "var_names", None)
        if saved_names is not None and names is not None and not np.array_equal(np.asarray(names).astype(str), saved_names):
            warnings.warn("var_names for adata passed in does not match var_names of adata used to train the model. "
                          "For valid results, the vars need to be the same and in the same order as the adata used to train the model.")
        init = dict(attr["init_params_"])
        if device is not None:
            init["device"] = device
        model = cls(adata, **init)
        model.module.load_state_dict(blob["model_state_dict"])
        model.module.eval()
        model.is_trained_ = bool(attr["is_trained_"])
        model.history = {k: list(v) for k, v in attr.get("history_", {}).items()}
        return model
