#!/usr/bin/env python3
"""Cost of the differential-expression reduction on device-resident sample banks (two fp32 banks of 4096 rows, 10 000 pairs, delta
0.25), at 10 000 / 1 000 / 64 genes, timed with device events after warm-up, in alternating rounds in one process:

    (a) the torch route on the same banks: two index_selects, log2, subtract, abs() >= delta, mean / std / amin / amax, two more means
    (b) de_ops.de_pairs                                                       -- one fused gather-compare-reduce kernel + its combine

    python tools/bench_de.py [--steps 20] [--warmup 5] [--rounds 3]
    python tools/bench_de.py --only kernel --genes 10000        # one path alone, e.g. under rocprofv3 --kernel-trace --stats

``--what median`` times the exact median of the same pairs under the same protocol:

    (a) the torch route on the same banks: two index_selects, log2, subtract, sort along the pairs, the two middle rows
        (torch.quantile refuses inputs this large)
    (b) de_ops.de_median                                                      -- a radix select: four gather passes + their bin picks

``--what by_label`` records, on one small trained model, one differential_expression_by call against the loop of
differential_expression_median calls it replaces (host clock around a device synchronise; ms per call; for the record, no threshold).

Prints one JSON line per gene count."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

FLT_MIN = float(np.finfo(np.float32).tiny)


def _timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]))


def run(n_genes: int, steps: int, warmup: int, rounds: int, only: str, rows: int = 4096, n_pairs: int = 10_000, delta: float = 0.25) -> dict:
    from spvipes_amd import de_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    b1, b2 = (torch.exp2(-13.0 + 3.0 * torch.randn(rows, n_genes, generator=gen)).to(dev) for _ in range(2))
    rng = np.random.default_rng(0)
    r1, r2 = (torch.as_tensor(rng.integers(0, rows, n_pairs).astype(np.int32), device=dev) for _ in range(2))
    l1, l2 = r1.long(), r2.long()
    ws, out = de_ops.de_workspace(n_genes, n_pairs, dev), torch.empty(7, n_genes, device=dev)

    def torch_route():
        x1, x2 = b1.index_select(0, l1), b2.index_select(0, l2)
        d = torch.log2(x1.clamp_min(FLT_MIN)) - torch.log2(x2.clamp_min(FLT_MIN))
        return {"lfc_mean": d.mean(0), "lfc_std": d.std(0, unbiased=False), "lfc_min": d.amin(0), "lfc_max": d.amax(0),
                "count_de": (d.abs() >= delta).sum(0).float(), "scale1": x1.mean(0), "scale2": x2.mean(0)}

    def kernel():
        return de_ops.de_pairs(b1, b2, r1, r2, delta=delta, eps=0.0, ws=ws, out=out)

    paths = {}
    if only in ("all", "torch"):
        paths["torch_route"] = torch_route
    if only in ("all", "kernel"):
        paths["de_pairs"] = kernel
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    res = {"n_genes": n_genes, "bank_rows": rows, "n_pairs": n_pairs, "steps": steps, "warmup": warmup, "rounds": rounds,
           "gathered_MB": round(2 * n_pairs * n_genes * 4 / 1e6, 1),
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        res["speedup"] = round(res["ms"]["torch_route"] / res["ms"]["de_pairs"], 3)
        a, b = torch_route(), kernel()
        res["max_abs_difference_of_the_two_paths"] = {k: float((a[k] - b[k]).abs().max()) for k in a}
    return res


def run_median(n_genes: int, steps: int, warmup: int, rounds: int, only: str, rows: int = 4096, n_pairs: int = 10_000) -> dict:
    from spvipes_amd import de_ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    b1, b2 = (torch.exp2(-13.0 + 3.0 * torch.randn(rows, n_genes, generator=gen)).to(dev) for _ in range(2))
    rng = np.random.default_rng(0)
    r1, r2 = (torch.as_tensor(rng.integers(0, rows, n_pairs).astype(np.int32), device=dev) for _ in range(2))
    l1, l2 = r1.long(), r2.long()
    ws, out = de_ops.de_median_workspace(n_genes, n_pairs, dev), torch.empty(2, n_genes, device=dev)

    def torch_route():
        d = torch.log2(b1.index_select(0, l1).clamp_min(FLT_MIN)) - torch.log2(b2.index_select(0, l2).clamp_min(FLT_MIN))
        s = d.sort(0).values
        return {"mid_lo": s[(n_pairs - 1) // 2], "mid_hi": s[n_pairs // 2]}

    def kernel():
        return de_ops.de_median(b1, b2, r1, r2, eps=0.0, ws=ws, out=out)

    paths = {}
    if only in ("all", "torch"):
        paths["torch_route"] = torch_route
    if only in ("all", "kernel"):
        paths["de_median"] = kernel
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    res = {"what": "median", "n_genes": n_genes, "bank_rows": rows, "n_pairs": n_pairs, "steps": steps, "warmup": warmup, "rounds": rounds,
           "gather_passes": 4, "gathered_MB_per_pass": round(2 * n_pairs * n_genes * 4 / 1e6, 1),
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        res["speedup"] = round(res["ms"]["torch_route"] / res["ms"]["de_median"], 3)
        a, b = torch_route(), kernel()
        res["max_abs_difference_of_the_two_paths"] = {k: float((a[k] - b[k]).abs().max()) for k in a}
    return res


class _Adata:
    """the fields of prepare_adatas' output that the model reads"""

    def __init__(self, X, obs, uns):
        self.X, self.obs, self.uns, self.layers = X, obs, uns, {}
        self.n_obs, self.n_vars = X.shape


def run_by_label(n_cells: int = 2000, n_genes: int = 2000, n_labels: int = 8, repeats: int = 3) -> dict:
    import time

    from spvipes_amd.model import spVIPES
    rng = np.random.default_rng(0)
    X = np.zeros((2 * n_cells, 2 * n_genes), np.float32)
    for g in range(2):
        X[g * n_cells:(g + 1) * n_cells, g * n_genes:(g + 1) * n_genes] = rng.poisson(2.0, (n_cells, n_genes)) * (rng.random((n_cells, n_genes)) < 0.3)
    obs = {"groups": np.array(["a"] * n_cells + ["b"] * n_cells), "indices": np.concatenate([np.arange(n_cells)] * 2).astype(np.int32),
           "cell_type": rng.integers(0, n_labels, 2 * n_cells)}
    uns = {"groups_lengths": {0: n_genes, 1: n_genes}, "groups_var_indices": [np.arange(n_genes), n_genes + np.arange(n_genes)],
           "groups_obs_indices": [np.arange(n_cells), n_cells + np.arange(n_cells)], "groups_obs_names": None, "groups_var_names": None}
    ad = _Adata(X, obs, uns)
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10, precision="bf16")
    gi = [list(uns["groups_obs_indices"][0]), list(uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=512, max_epochs=1, train_size=1.0)
    cells, lab = np.asarray(gi[0]), np.asarray(obs["cell_type"])[:n_cells]
    names = np.unique(lab)

    def by():
        return model.differential_expression_by(gi, 0, "cell_type", batch_size=512, seed=0)

    def loop():
        return [model.differential_expression_median(gi, 0, cells[lab == v], None, batch_size=512, seed=k) for k, v in enumerate(names.tolist())]

    ms = {"by_label": [], "loop_of_single_calls": []}
    for fn in (by, loop):
        fn()   # warm-up
    for _ in range(repeats):
        for k, fn in (("by_label", by), ("loop_of_single_calls", loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {"what": "by_label", "cells_per_group": n_cells, "genes_per_group": n_genes, "labels": int(len(names)), "n_pairs": 10_000,
            "ms": {k: round(float(np.median(v)), 2) for k, v in ms.items()}, "ms_repeats": {k: [round(x, 2) for x in v] for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["pairs", "median", "by_label"], default="pairs")
    ap.add_argument("--genes", nargs="+", type=int, default=[10_000, 1_000, 64])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "torch", "kernel"], default="all")
    a = ap.parse_args()
    if a.what == "by_label":
        print(json.dumps(run_by_label()), flush=True)
        return
    for n in a.genes:
        print(json.dumps((run if a.what == "pairs" else run_median)(n, a.steps, a.warmup, a.rounds, a.only)), flush=True)


if __name__ == "__main__":
    main()
