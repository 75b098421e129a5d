#!/usr/bin/env python3
"""Cost of the raw-count statistics of spVIPES.count_statistics on one resident count matrix (C2's shape: 50 000 cells x 10 000
genes, uint16, make_synthetic_group's density; 20 labels of unequal size, every cell listed once, rows sorted by label, weights
target_sum / total), timed with device events after warm-up, in alternating rounds in one process:

    (a) the torch route on the same matrix, per label and in chunks of 4096 rows: index_select, mask the uint16 bit patterns to
        int32, widen to fp64, .sum(0), (x != 0).sum(0), (x * w[:, None]).sum(0)
    (b) count_ops.count_stats on the dense matrix          -- one fused partial pass + its merge
    (c) count_ops.count_stats on the CSR form of the matrix -- spv_csr_gather per chunk of whole slabs, partial pass per chunk, one merge

    python tools/bench_count_stats.py [--steps 10] [--warmup 3] [--rounds 3] [--cells 50000] [--genes 10000] [--labels 20]
    python tools/bench_count_stats.py --only kernel        # one route alone, e.g. under rocprofv3 --kernel-trace --stats
    python tools/bench_count_stats.py --slab 512           # plan the slabs with another length than the library reports (A/B)

Prints one JSON line: the three medians (ms), the achieved bytes/s of (b) and (c) counted as n * G * 2 matrix bytes per call, and
whether (a) and (b) agree (integer rows exactly)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


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


def run(cells: int, genes: int, n_labels: int, steps: int, warmup: int, rounds: int, only: str, slab: int = 0, chunk: int = 4096,
        target_sum: float = 1e4) -> dict:
    from spvipes_amd import count_ops
    if slab:   # the kernels take any slab length up to 32768 from the table; count_stats plans with count_stats_slab()
        count_ops.count_stats_slab = lambda: int(slab)
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.ops import SparseGroupCounts

    dev = torch.device("cuda:0")
    counts = make_synthetic_group(0, cells, genes, dev).counts
    assert counts.X.dtype == torch.int16, "the benchmark shape is a uint16 matrix"
    rng = np.random.default_rng(0)
    share = np.arange(1, n_labels + 1, dtype=np.float64)
    lab = rng.choice(n_labels, size=cells, p=share / share.sum())           # unequal label sizes, 1 : n_labels
    order = np.argsort(lab, kind="stable")
    sizes = np.bincount(lab, minlength=n_labels).tolist()
    rows = torch.as_tensor(order.astype(np.int32), device=dev)
    total = count_ops.count_totals(counts).index_select(0, rows.long())
    w = torch.where(total > 0, target_sum / total, torch.zeros_like(total))
    ws, out = count_ops.count_stats_workspace(genes, sizes, dev), torch.empty((n_labels, 3, genes), dtype=torch.float64, device=dev)
    sparse = SparseGroupCounts.from_dense(counts) if only in ("all", "sparse") else None
    out_sparse = torch.empty_like(out)
    long_rows, c0 = rows.long(), counts.col_off

    def torch_route():
        res, pos = torch.zeros((n_labels, 3, genes), dtype=torch.float64, device=dev), 0
        for k, s in enumerate(sizes):
            for lo in range(pos, pos + s, chunk):
                hi = min(lo + chunk, pos + s)
                x = (counts.X.index_select(0, long_rows[lo:hi])[:, c0:c0 + genes].to(torch.int32) & 0xFFFF).to(torch.float64)
                res[k, 0] += x.sum(0)
                res[k, 1] += (x != 0).sum(0)
                res[k, 2] += (x * w[lo:hi, None]).sum(0)
            pos += s
        return res

    def kernel_route():
        return count_ops.count_stats(counts, rows, sizes, w=w, ws=ws, out=out)

    def sparse_route():
        return count_ops.count_stats(sparse, rows, sizes, w=w, ws=ws, out=out_sparse)

    routes = {"torch": torch_route, "kernel": kernel_route, "sparse": sparse_route}
    names = list(routes) if only == "all" else [only]
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            ms[n].append(_timed(routes[n], steps, warmup))
    res = {"cells": cells, "genes": genes, "labels": n_labels, "label_sizes_min_max": [min(sizes), max(sizes)], "steps": steps, "warmup": warmup,
           "rounds": rounds, "tile": count_ops.count_stats_tile(), "slab": count_ops.count_stats_slab(),
           "density": float((counts.X != 0).float().mean())}
    for n in names:
        res[f"{n}_ms_median"] = float(np.median(ms[n]))
        res[f"{n}_ms_rounds"] = ms[n]
        if n != "torch":
            res[f"{n}_bytes_per_s"] = cells * genes * 2 / (res[f"{n}_ms_median"] * 1e-3)
    if only == "all":
        a, b, c = torch_route(), kernel_route().clone(), sparse_route()
        res["kernel_equals_torch_integer_rows"] = bool(torch.equal(a[:, :2], b[:, :2]))
        res["kernel_vs_torch_weighted_max_rel"] = float(((a[:, 2] - b[:, 2]).abs() / b[:, 2].clamp_min(1e-300)).max())
        res["sparse_equals_dense_bit_for_bit"] = bool(torch.equal(b, c))
        res["kernel_over_torch"] = res["kernel_ms_median"] / res["torch_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--slab", type=int, default=0)
    ap.add_argument("--only", default="all", choices=["all", "torch", "kernel", "sparse"])
    a = ap.parse_args()
    print(json.dumps(run(a.cells, a.genes, a.labels, a.steps, a.warmup, a.rounds, a.only, a.slab)), flush=True)


if __name__ == "__main__":
    main()
