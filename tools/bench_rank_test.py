#!/usr/bin/env python3
"""Cost of the rank sums behind spVIPES.rank_genes_groups on one resident count matrix (50 000 cells x 10 000 genes, uint16, 20 labels
of unequal size, every cell listed once in matrix order, weights fp32(target_sum / total)), timed with device events after warm-up, in
alternating rounds in one process:

    (a) the torch route on the same matrix, per chunk of ``--chunk`` genes: gather the columns, normalise (one fp32 multiply),
        torch.sort(dim=0), searchsorted left / right for L / U, index_add_ of L + U + 1 by label in int64; the ties from the sorted keys
    (b) rank_ops.rank_sums on the dense matrix          -- spv_rank_stage + spv_rank_sums per gene slab
    (c) rank_ops.rank_sums on the CSR form of the matrix -- spv_csr_gather + spv_rank_stage per chunk of rows, per gene slab

at ``--density`` (about 10 % non-zeros) and, with --dense-case, once more on a matrix that is non-zero in EVERY cell (every column takes
the radix passes through global memory).

    python tools/bench_rank_test.py [--steps 10] [--warmup 2] [--rounds 3] [--cells 50000] [--genes 10000] [--labels 20] [--dense-case]
    python tools/bench_rank_test.py --raw                # rank the raw counts (weight 1): a handful of distinct keys per gene, long tie runs
    python tools/bench_rank_test.py --budget-mib 256     # cut the gene slabs to a smaller workspace (A/B of rank_ops.WS_BUDGET_BYTES)
    python tools/bench_rank_test.py --only kernel        # one route alone, e.g. under rocprofv3 --kernel-trace --stats

Prints one JSON line per matrix: the medians (ms), the peak device memory each route allocated beyond the matrix (bytes), the share of
columns on each sort path, and whether (a), (b) and (c) agree (integers: exactly)."""
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


def _peak(fn) -> int:
    """bytes the route allocates at its peak, beyond what is resident before it starts"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def make_matrix(cells: int, genes: int, density: float, dev, seed: int = 0) -> torch.Tensor:
    """uint16 bit patterns [cells, genes]: a share ``density`` of non-zero counts 1 + geometric-ish (heavy at 1, 2, 3), made on the device"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    X = torch.empty((cells, genes), dtype=torch.int16, device=dev)
    for lo in range(0, cells, 4096):
        hi = min(lo + 4096, cells)
        u = torch.rand((hi - lo, genes), device=dev, generator=gen)
        c = 1 + torch.floor(-torch.log(torch.rand((hi - lo, genes), device=dev, generator=gen).clamp_min(1e-7)) * 2.0)
        X[lo:hi] = torch.where(u < density, c, torch.zeros_like(c)).to(torch.int16)
    return X


def run(cells: int, genes: int, n_labels: int, density: float, steps: int, warmup: int, rounds: int, only: str, chunk: int, target_sum: float = 1e4,
        raw: bool = False, budget_mib: int = 0) -> dict:
    from spvipes_amd import count_ops, rank_ops
    if budget_mib:   # cut the gene slabs to another workspace budget than rank_ops' default (A/B)
        rank_ops.WS_BUDGET_BYTES = budget_mib << 20
    from spvipes_amd.ops import GroupCounts, SparseGroupCounts

    dev = torch.device("cuda:0")
    counts = GroupCounts(make_matrix(cells, genes, density, dev), genes, 0)
    rng = np.random.default_rng(0)
    share = np.arange(1, n_labels + 1, dtype=np.float64)
    seg = torch.as_tensor(rng.choice(n_labels, size=cells, p=share / share.sum()).astype(np.int32), device=dev)   # unequal label sizes, 1 : n_labels
    rows = torch.arange(cells, dtype=torch.int32, device=dev)
    total = count_ops.count_totals(counts)
    w = torch.ones_like(total, dtype=torch.float32) if raw else torch.where(total > 0, target_sum / total, torch.zeros_like(total)).to(torch.float32)
    sparse = SparseGroupCounts.from_dense(counts) if only in ("all", "sparse") and density < 0.5 else None
    seg_long = seg.long()

    def torch_route():
        rank2 = torch.zeros((n_labels, genes), dtype=torch.int64, device=dev)
        ties = torch.empty((genes,), dtype=torch.int64, device=dev)
        for g0 in range(0, genes, chunk):
            g1 = min(g0 + chunk, genes)
            x = ((counts.X[:, g0:g1].to(torch.int32) & 0xFFFF).to(torch.float32) * w[:, None]).T.contiguous()   # [genes, n]: the keys
            s = torch.sort(x, dim=1).values
            lo, hi = torch.searchsorted(s, x, right=False), torch.searchsorted(s, x, right=True)
            rank2[:, g0:g1].index_add_(0, seg_long, (lo + hi + 1).T)
            t = hi - lo   # every entry of a run of t carries t: the sum of t^2 - 1 over the entries is the sum of t^3 - t over the runs
            ties[g0:g1] = (t * t - 1).sum(1)
        return rank2, ties

    def kernel_route():
        return rank_ops.rank_sums(counts, rows, seg, n_labels, w=w)

    def sparse_route():
        return rank_ops.rank_sums(sparse, rows, seg, n_labels, w=w)

    routes = {"torch": torch_route, "kernel": kernel_route}
    if sparse is not None:
        routes["sparse"] = sparse_route
    names = list(routes) if only == "all" else [only]
    nnz = (counts.X != 0).sum(0)
    cap = rank_ops.rank_lds_capacity()
    res = {"keys": "raw counts" if raw else "normalised", "cells": cells, "genes": genes, "labels": n_labels, "density": float(nnz.sum()) / (cells * genes),
           "steps": steps, "warmup": warmup, "rounds": rounds,
           "torch_gene_chunk": chunk, "gene_slab": rank_ops.rank_gene_slab(cells), "lds_capacity": cap,
           "columns_on_the_radix_path": int(((nnz > cap)).sum()), "workspace_bytes": rank_ops.rank_ws_bytes(cells, min(rank_ops.rank_gene_slab(cells), genes)),
           "matrix_bytes": cells * genes * 2}
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            ms[n].append(_timed(routes[n], steps, warmup))
    for n in names:
        res[f"{n}_ms_median"] = float(np.median(ms[n]))
        res[f"{n}_ms_rounds"] = ms[n]
    for n in names:
        rank_ops._WS.clear()   # the cached workspace counts as a fused route's memory, each time
        res[f"{n}_peak_bytes"] = _peak(routes[n])
    if only == "all":
        a, b = torch_route(), kernel_route()
        res["kernel_equals_torch"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        if sparse is not None:
            c = sparse_route()
            res["sparse_equals_dense_bit_for_bit"] = bool(torch.equal(b[0], c[0]) and torch.equal(b[1], c[1]))
        res["kernel_over_torch"] = res["kernel_ms_median"] / res["torch_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--density", type=float, default=0.10)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--dense-case", action="store_true", help="also measure a matrix that is non-zero in every cell (fused against torch)")
    ap.add_argument("--raw", action="store_true", help="rank the raw counts (weight 1: heavy ties) instead of the normalised ones")
    ap.add_argument("--budget-mib", type=int, default=0, help="workspace budget of rank_ops in MiB (0: its default)")
    ap.add_argument("--only", default="all", choices=["all", "torch", "kernel", "sparse"])
    a = ap.parse_args()
    print(json.dumps(run(a.cells, a.genes, a.labels, a.density, a.steps, a.warmup, a.rounds, a.only, a.chunk, raw=a.raw, budget_mib=a.budget_mib)), flush=True)
    if a.dense_case:
        torch.cuda.empty_cache()
        print(json.dumps(run(a.cells, a.genes, a.labels, 1.0, a.steps, a.warmup, a.rounds, a.only, a.chunk, raw=a.raw, budget_mib=a.budget_mib)), flush=True)


if __name__ == "__main__":
    main()
