#!/usr/bin/env python3
"""Cost of the exact rank transform and of Spearman's table built on it (rank_ops.rank_transform, then gram_ops.gram_accumulate in row
chunks), at ``--cells`` (50 000) x 512 / 2048 / 4096 genes, timed with device events after warm-up, in alternating rounds in one process:

    (a) the torch route on the same data, per chunk of ``--chunk`` genes: the keys, torch.sort(dim=0), searchsorted left / right for
        L / U, c = L + U - n as fp64; then ONE fp64 matmul c.T @ c
    (b) rank_transform alone                -- spv_rank_values_stage + spv_rank_values per gene slab
    (c) rank_transform + gram_accumulate    -- the whole of (a) on the fused route

for two inputs: a uint16 count matrix with about 10 % non-zeros ranked with weights fp32(target_sum / total) (the case of
count_spearman_matrix: the zero run is never sorted), and an all-positive fp32 block ranked IN PLACE (the case of
get_feature_spearman_matrix: every column takes the radix passes).

    python tools/bench_spearman.py [--steps 5] [--warmup 1] [--rounds 3] [--cells 50000] [--genes 512 2048 4096] [--chunk 256]
    python tools/bench_spearman.py --only kernel     # the fused routes alone, e.g. under rocprofv3 --kernel-trace --stats

Prints one JSON line per (input, genes): the medians (ms), the peak device memory each route allocated beyond the input (bytes), and
whether the two routes' tables agree (integers: exactly)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from bench_rank_test import _peak, _timed, make_matrix

GRAM_ROWS = 16384


def run(kind: str, cells: int, genes: int, steps: int, warmup: int, rounds: int, only: str, chunk: int, target_sum: float = 1e4) -> dict:
    from spvipes_amd import count_ops, gram_ops, rank_ops
    from spvipes_amd.ops import GroupCounts

    dev = torch.device("cuda:0")
    rows = torch.arange(cells, dtype=torch.int32, device=dev)
    if kind == "u16-10pct":
        counts = GroupCounts(make_matrix(cells, genes, 0.10, dev), genes, 0)
        total = count_ops.count_totals(counts)
        w = torch.where(total > 0, target_sum / total, torch.zeros_like(total)).to(torch.float32)
        keys = lambda g0, g1: (counts.X[:, g0:g1].to(torch.int32) & 0xFFFF).to(torch.float32) * w[:, None]   # noqa: E731
        source = None
    else:
        gen = torch.Generator(device=dev).manual_seed(1)
        source = torch.rand((cells, genes), device=dev, generator=gen) + 0.01   # all positive, (nearly) all distinct
        w = None
        keys = lambda g0, g1: source[:, g0:g1]   # noqa: E731
    block = torch.empty((cells, genes), dtype=torch.float32, device=dev)
    S = torch.zeros(genes, dtype=torch.float64, device=dev)
    Cm = torch.zeros((genes, genes), dtype=torch.float64, device=dev)
    ws = gram_ops.gram_workspace(genes, min(cells, GRAM_ROWS), dev)

    def torch_route():
        c = torch.empty((cells, genes), dtype=torch.float64, device=dev)
        for g0 in range(0, genes, chunk):
            g1 = min(g0 + chunk, genes)
            x = keys(g0, g1).T.contiguous()   # [genes, n]
            s = torch.sort(x, dim=1).values
            c[:, g0:g1] = (torch.searchsorted(s, x, right=False) + torch.searchsorted(s, x, right=True) - cells).T.to(torch.float64)
        return c.T @ c

    def transform():
        if source is None:
            return rank_ops.rank_transform(counts, rows, w=w, out=block)
        block.copy_(source)   # (the in-place transform consumes its input: the copy is part of this route's time, 4 n n_sel bytes each way)
        return rank_ops.rank_transform(GroupCounts(block, genes, 0), rows, out=block)

    def fused():
        b = transform()
        S.zero_()
        Cm.zero_()
        for r0 in range(0, cells, GRAM_ROWS):
            gram_ops.gram_accumulate(b[r0:r0 + GRAM_ROWS], sums=S, gram=Cm, ws=ws)
        return Cm

    routes = {"torch": torch_route, "transform": transform, "fused": fused}
    names = list(routes) if only == "all" else ["transform", "fused"]
    res = {"input": kind, "cells": cells, "genes": genes, "steps": steps, "warmup": warmup, "rounds": rounds, "torch_gene_chunk": chunk,
           "gene_slab": rank_ops.rank_values_gene_slab(cells), "workspace_bytes": rank_ops.rank_values_ws_bytes(cells, min(rank_ops.rank_values_gene_slab(cells), genes)),
           "block_bytes": cells * genes * 4, "table_bytes": genes * genes * 8}
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            ms[n].append(_timed(routes[n], steps, warmup))
    for n in names:
        res[f"{n}_ms_median"] = float(np.median(ms[n]))
        res[f"{n}_ms_rounds"] = ms[n]
    for n in names:
        rank_ops._WS.clear()   # the cached workspace counts as a fused route's memory, each time
        torch.cuda.empty_cache()
        res[f"{n}_peak_bytes"] = _peak(routes[n])
    if only == "all":
        a, b = torch_route(), fused()
        res["fused_equals_torch"] = bool(torch.equal(a, b))
        res["sums_are_zero"] = bool((S == 0).all())
        res["fused_over_torch"] = res["fused_ms_median"] / res["torch_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--inputs", nargs="+", default=["u16-10pct", "f32-positive"], choices=["u16-10pct", "f32-positive"])
    ap.add_argument("--only", default="all", choices=["all", "kernel"])
    a = ap.parse_args()
    for kind in a.inputs:
        for genes in a.genes:
            print(json.dumps(run(kind, a.cells, genes, a.steps, a.warmup, a.rounds, a.only, a.chunk)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
