#!/usr/bin/env python3
"""Cost of the segmented distance sums of spVIPES.latent_silhouette (silhouette_ops.segment_distance_sums -> spv_silhouette_sums) against
two torch routes on the same device tensors, timed with device events after warm-up, in alternating rounds in one process:

    (a) torch64: per chunk of queries ``torch.cdist(q, C)`` and, per segment, the fp64 sum of its slice of columns
    (b) torch32: per chunk of queries ``torch.cdist(q, C)`` and ONE fp32 matmul with the segments' one-hot matrix [n_c, n_seg]
    (c) kernel:  the fused kernel, nothing of size queries x candidates stored
    Both torch routes size their chunk so that ONE chunk x n_c fp32 temporary stays within --budget-mib.

    python tools/bench_silhouette.py [--steps 5] [--warmup 2] [--rounds 3] [--cells 50000 100000] [--budget-mib 1024]
    python tools/bench_silhouette.py --only kernel        # one route alone, e.g. under rocprofv3 --kernel-trace --stats
    python tools/bench_silhouette.py --only kernel --n-splits 3 14   # the fused kernel's automatic chunk count against forced ones, alternating

Shapes: cells x cells standard-normal rows (the queries ARE the candidates, as in latent_silhouette), D 10 / 25 / 35, 20 labels x 2
groups = 40 segments of unequal sizes.  Prints one JSON line per shape: the three medians (ms), each route's addition to the device's peak
allocated memory during one call (outputs included), the kernel's rate in (subtract, fma) pairs per second with the time the fp32
vector peak would need for the D-term chains alone (157.3 TFLOP/s = 78.6e12 lane instructions per second, two instructions per term;
the root, the convert and the fp64 add come on top), and the largest relative difference of the sums between the routes (the torch
routes' distances come from another formula; torch32 also adds in fp32)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

VALU_LANE_OPS_PER_S = 157.3e12 / 2
N_LABELS = 20


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


def _peak_added(fn) -> int:
    """bytes the call adds to the peak of allocated device memory (its result included)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return int(peak - base)


def run(cells: int, D: int, steps: int, warmup: int, rounds: int, only: str, budget_mib: int, n_splits=(0,)) -> dict:
    from spvipes_amd import silhouette_ops
    from spvipes_amd.data import silhouette_segments
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(D * 100 + cells % 97)
    rng = np.random.default_rng(D)
    codes, groups = rng.choice(N_LABELS, cells, p=np.arange(1, N_LABELS + 1) / (N_LABELS * (N_LABELS + 1) / 2)), rng.integers(0, 2, cells)
    perm, seg_ptr, sizes = silhouette_segments(codes, groups, N_LABELS)
    n_seg = len(sizes)
    Q = torch.randn(cells, D, generator=g).to(dev)
    C = Q.index_select(0, torch.as_tensor(perm, device=dev))
    ptr_dev = torch.as_tensor(seg_ptr, device=dev)
    onehot = torch.zeros((cells, n_seg), device=dev)
    onehot[torch.arange(cells, device=dev), torch.as_tensor(np.repeat(np.arange(n_seg), sizes), device=dev)] = 1.0
    chunk = max(1, (budget_mib << 20) // (cells * 4))
    bounds = [(int(seg_ptr[s]), int(seg_ptr[s + 1])) for s in range(n_seg)]

    def torch64_route():
        S = torch.empty((cells, n_seg), dtype=torch.float64, device=dev)
        for lo in range(0, cells, chunk):
            d = torch.cdist(Q[lo:lo + chunk], C)
            for s, (b0, b1) in enumerate(bounds):
                S[lo:lo + chunk, s] = d[:, b0:b1].sum(dim=1, dtype=torch.float64)
        return S

    def torch32_route():
        S = torch.empty((cells, n_seg), dtype=torch.float32, device=dev)
        for lo in range(0, cells, chunk):
            S[lo:lo + chunk] = torch.cdist(Q[lo:lo + chunk], C) @ onehot
        return S

    def kernel_route():
        return silhouette_ops.segment_distance_sums(Q, C, ptr_dev)

    routes = {"torch64": torch64_route, "torch32": torch32_route, "kernel": kernel_route}
    forced = {f"kernel_split{v}": (lambda v=v: silhouette_ops.segment_distance_sums(Q, C, ptr_dev, n_split=v)) for v in n_splits if v}
    routes.update(forced)
    names = (["torch64", "torch32", "kernel"] if only == "all" else [only]) + list(forced)
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            ms[n].append(_timed(routes[n], steps, warmup))
    splits = silhouette_ops.silhouette_splits(cells, cells)
    res = {"cells": cells, "D": D, "n_seg": n_seg, "steps": steps, "warmup": warmup, "rounds": rounds, "n_split": splits, "torch_chunk_rows": chunk,
           "budget_mib": budget_mib}
    for n in names:
        res[f"{n}_ms_median"] = float(np.median(ms[n]))
        res[f"{n}_ms_rounds"] = ms[n]
    if "kernel" in names:
        silhouette_ops._WS.clear()   # count the workspace as part of the call
        res["kernel_peak_added_bytes"] = _peak_added(kernel_route)
        res["kernel_ws_bytes"], res["kernel_out_bytes"] = silhouette_ops.silhouette_ws_bytes(cells, n_seg, splits), cells * n_seg * 8
        res["kernel_pair_terms_per_s"] = cells * cells * D / (res["kernel_ms_median"] * 1e-3)
        res["valu_bound_ms"] = cells * cells * D * 2 / VALU_LANE_OPS_PER_S * 1e3
        res["kernel_share_of_valu_bound"] = res["valu_bound_ms"] / res["kernel_ms_median"]
    for n in ("torch64", "torch32"):
        if n in names:
            res[f"{n}_peak_added_bytes"] = _peak_added(routes[n])
    if "torch64" in names or "torch32" in names:
        res["torch_chunk_temp_bytes"] = min(chunk, cells) * cells * 4
    if only == "all":
        k = kernel_route()
        for n in ("torch64", "torch32"):
            t = routes[n]().double()
            res[f"max_rel_difference_{n}_vs_kernel"] = float(((t - k).abs() / k.clamp_min(1e-300)).max())
            res[f"kernel_over_{n}"] = res["kernel_ms_median"] / res[f"{n}_ms_median"]
            del t
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=int, nargs="+", default=[50000, 100000])
    ap.add_argument("--budget-mib", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[10, 25, 35])
    ap.add_argument("--only", default="all", choices=["all", "torch64", "torch32", "kernel"])
    ap.add_argument("--n-splits", type=int, nargs="+", default=[0], help="further chunk counts to time the fused kernel under (routes kernel_split<n>)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_silhouette needs the GPU: there is no CPU timing of a GPU kernel")
    for cells in a.cells:
        for D in a.dims:
            print(json.dumps(run(cells, D, a.steps, a.warmup, a.rounds, a.only, a.budget_mib, tuple(a.n_splits))), flush=True)


if __name__ == "__main__":
    main()
