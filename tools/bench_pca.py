#!/usr/bin/env python3
"""Cost of count_pca's pieces at 2 x 50 000 cells x 10 000 genes (uint16 counts, about 10 % non-zeros, eight planted cell clusters per
group), l = 64, timed with device events after warm-up, in alternating rounds in one process (tools/bench_gene_correlation.py's protocol):

    (a) project alone: Y = X V over both groups (spv_pca_project; X is made in registers from the 2-byte counts)
    (a') back alone on a Y projected once: Z = X^T Y (spv_pca_back and its merge)
    (b) one operator application: project then back, Z = X^T (X V)
    (c) the whole count_pca(n_comps=50): weights, moments, the block Lanczos iteration, the final pass (the median of `rounds` SINGLE calls
        after one untimed call; every other path is a median of `rounds` medians of `steps` calls after `warmup`)
    (d) the torch route on a STAGED block: X is written out once in fp32 (its cost is quoted apart), then Y = X @ V and Z = X.T @ Y
    (e) torch.pca_lowrank(q=64, niter=2) on that block

    python tools/bench_pca.py [--cells 50000] [--genes 10000] [--paired 10000 2000] [--steps 5] [--warmup 2] [--rounds 3]

Prints one JSON line per number of paired genes with the medians, the ratios (d) / (b) whichever way they fall, the rate of (a) and (a')
in fp32 flop per second (2 n G l each: every kernel walks ALL G genes of a group, a gene outside the pairing has scale
0), the iteration's record, the operator's slack against an fp64 operator on a staged block of 4096 cells, and the peak device memory
each route adds over the resident counts."""
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


def make_counts(n: int, G: int, seed: int, dev, clusters: int = 8):
    """uint16 counts [n, G] on the device (int16 bit patterns): cell c of cluster k holds gene j with probability 0.1 f[k, j], f a
    Gamma(2) profile of mean 1 per cluster, and then 1 + Poisson(1) counts"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    torch.manual_seed(seed)
    prof = torch.distributions.Gamma(2.0, 2.0).sample((clusters, G)).to(dev).clamp_(max=8.0) * 0.1
    X = torch.empty((n, G), dtype=torch.int16, device=dev)
    for c0 in range(0, n, 5000):
        m = min(5000, n - c0)
        k = torch.randint(0, clusters, (m,), generator=gen, device=dev)
        hit = torch.rand((m, G), generator=gen, device=dev) < prof[k]
        X[c0:c0 + m] = (hit * (1 + torch.poisson(torch.ones((m, G), device=dev), generator=gen))).to(torch.int16)
    return X


def _peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def run(n: int, G: int, paired: int, steps: int, warmup: int, rounds: int, counts) -> dict:
    from spvipes_amd import pca_ops
    from spvipes_amd.count_ops import count_totals
    dev = counts[0].device
    l = 64
    cols = [np.arange(paired, dtype=np.int32)] * 2
    rows = [torch.arange(n, dtype=torch.int32, device=dev) for _ in range(2)]
    groups = [(counts[g], rows[g]) for g in range(2)]
    # the operator as count_pca builds it
    ws, sums, sqs = [], 0, 0
    dc = torch.arange(paired, dtype=torch.int64, device=dev)
    for g in range(2):
        total = count_totals(counts[g])
        w = torch.where(total > 0, 1e4 / total, torch.zeros_like(total)).to(torch.float32)
        ws.append(w)
        s, q = pca_ops.lognorm_moments(counts[g], rows[g], w)
        sums, sqs = sums + s[:paired], sqs + q[:paired]
    mean = (sums / (2 * n)).to(torch.float32)
    parts = []
    for g in range(2):
        mu, sc = torch.zeros(G, dtype=torch.float32, device=dev), torch.zeros(G, dtype=torch.float32, device=dev)
        mu[:paired], sc[:paired] = mean, 1.0
        parts.append(pca_ops.PcaGroup(counts[g], rows[g], ws[g], mu, sc, dc))
    op = pca_ops.PcaOperator(parts)
    V = torch.linalg.qr(torch.randn((paired, l), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1)))[0].to(torch.float32)

    def stage():
        X = torch.empty((2 * n, paired), dtype=torch.float32, device=dev)
        for g in range(2):
            for p0, b in pca_ops.stage_block(counts[g], rows[g], ws[g], parts[g].mu, parts[g].scale):
                X[g * n + p0:g * n + p0 + b.shape[0]] = b[:, :paired]
        return X

    state = {"Y": op.project(V)}
    paths = {"project": lambda: op.project(V), "back": lambda: op.back(state["Y"]), "apply": lambda: op.apply(V),
             "torch_matmul_both_ways": lambda: state["X"].t() @ (state["X"] @ V), "torch_project": lambda: state["X"] @ V,
             "stage_block_once": stage, "pca_lowrank_q64_niter2": lambda: torch.pca_lowrank(state["X"], q=64, center=False, niter=2)}
    (_z, peak_apply) = _peak(lambda: op.apply(V), dev)
    state["X"], peak_stage = _peak(stage, dev)
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # every path under the same protocol: medians of `steps` calls after `warmup`, in alternating rounds
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    _lr, peak_lowrank = _peak(lambda: torch.pca_lowrank(state["X"], q=64, center=False, niter=2), dev)
    # the two routes' operators against each other
    Zk, Yk = op.apply(V)
    Zt = (state["X"].t() @ (state["X"] @ V)).to(torch.float64)
    diff = float(torch.linalg.matrix_norm(Zk - Zt) / torch.linalg.matrix_norm(Zk))
    # the operator's slack against an fp64 operator on a staged block of 4096 cells of group 0
    m4 = min(4096, n)
    sub = pca_ops.PcaOperator([pca_ops.PcaGroup(counts[0], rows[0][:m4].contiguous(), ws[0][:m4].contiguous(), parts[0].mu, parts[0].scale, dc)])
    Zs, _ys = sub.apply(V)
    X64 = state["X"][:m4].to(torch.float64)
    Z64 = X64.t() @ (X64 @ V.to(torch.float64))
    slack = float(torch.linalg.matrix_norm(Zs - Z64, 2) / torch.linalg.matrix_norm(Z64, 2))
    del X64, Z64
    state.clear()
    torch.cuda.empty_cache()
    out, peak_pca = _peak(lambda: pca_ops.count_pca(groups, cols, 50), dev)
    torch.cuda.synchronize()
    ms["count_pca_50"] = [_timed(lambda: pca_ops.count_pca(groups, cols, 50), 1, 0) for _ in range(rounds)]   # `rounds` single calls after the one above
    m = {k: round(float(np.median(v)), 3) for k, v in ms.items()}
    flop = 2.0 * 2 * n * G * l
    res = {"cells": [n, n], "G": G, "paired": paired, "l": l, "steps": steps, "warmup": warmup, "rounds": rounds, "ms": m,
           "ms_rounds": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "project_Tflop_per_s": round(flop / (m["project"] * 1e-3) / 1e12, 2),
           "back_Tflop_per_s": round(flop / (m["back"] * 1e-3) / 1e12, 2),
           "torch_both_ways_over_apply": round(m["torch_matmul_both_ways"] / m["apply"], 3),
           "torch_project_over_project": round(m["torch_project"] / m["project"], 3),
           "routes_relative_difference": diff, "operator_slack_vs_fp64_4096_cells": slack,
           "count_pca": {"n_blocks": out["n_blocks"], "n_restarts": out["n_restarts"], "converged": out["converged"], "n_apply": out["n_apply"],
                         "worst_residual_over_theta1": float(np.max(out["residuals"]) / out["theta"][0]),
                         "variance_ratio_sum": float(np.sum(out["variance_ratio"]))},
           "peak_MiB_over_resident_counts": {"apply": peak_apply, "staged_block": peak_stage, "pca_lowrank_on_the_block": peak_lowrank, "count_pca": peak_pca}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=10000)
    ap.add_argument("--paired", nargs="+", type=int, default=[10000, 2000])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from spvipes_amd.ops import GroupCounts
    dev = torch.device("cuda:0")
    counts = [GroupCounts(make_counts(a.cells, a.genes, 10 + g, dev), a.genes, 0) for g in range(2)]
    for p in a.paired:
        print(json.dumps(run(a.cells, a.genes, min(p, a.genes), a.steps, a.warmup, a.rounds, counts)), flush=True)


if __name__ == "__main__":
    main()
