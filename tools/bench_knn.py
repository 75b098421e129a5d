#!/usr/bin/env python3
"""Cost of the exact k-nearest-neighbour search of spVIPES.latent_neighbors (knn_ops.knn -> spv_knn) against the torch route on the same
device tensors, timed with device events after warm-up, in alternating rounds in one process:

    (a) torch: per chunk of queries ``torch.cdist(q, C) ** 2`` and ``.topk(k, largest=False)``; the chunk is sized so that ONE
        chunk x n_c fp32 temporary stays within --budget-mib (the route holds two of them at a time: cdist's result and its square)
    (b) knn_ops.knn: the fused kernel, nothing of size queries x candidates stored

    python tools/bench_knn.py [--steps 10] [--warmup 2] [--rounds 3] [--cells 50000] [--budget-mib 1024]
    python tools/bench_knn.py --only kernel        # one route alone, e.g. under rocprofv3 --kernel-trace --stats

Shapes: cells x cells standard-normal rows, D 25 and 35, k 15 and 50.  Prints one JSON line per shape: the two medians (ms), each
route's addition to the device's peak allocated memory during one call (outputs included), the kernel's rate in (subtract, fma) pairs
per second with the time the fp32 vector peak would need for the D-term chains (157.3 TFLOP/s = 78.6e12 lane instructions per second,
two instructions per term), and how many rows of the two routes name the same neighbours (the torch route's distances come from
another formula, so near-ties may swap)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

VALU_LANE_OPS_PER_S = 157.3e12 / 2


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


def run(cells: int, D: int, k: int, steps: int, warmup: int, rounds: int, only: str, budget_mib: int) -> dict:
    from spvipes_amd import knn_ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(D * 100 + k)
    Q, C = (torch.randn(cells, D, generator=g).to(dev) for _ in range(2))
    chunk = max(1, (budget_mib << 20) // (cells * 4))

    def torch_route():
        idx, dist = torch.empty((cells, k), dtype=torch.int64, device=dev), torch.empty((cells, k), dtype=torch.float32, device=dev)
        for lo in range(0, cells, chunk):
            d, i = (torch.cdist(Q[lo:lo + chunk], C) ** 2).topk(k, dim=1, largest=False, sorted=True)
            idx[lo:lo + chunk], dist[lo:lo + chunk] = i, d
        return idx, dist

    def kernel_route():
        return knn_ops.knn(Q, C, k)

    routes = {"torch": torch_route, "kernel": kernel_route}
    names = list(routes) if only == "all" else [only]
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            ms[n].append(_timed(routes[n], steps, warmup))
    splits = knn_ops.knn_splits(cells, cells)
    res = {"cells": cells, "D": D, "k": k, "steps": steps, "warmup": warmup, "rounds": rounds, "tiles": list(knn_ops.knn_tiles()), "n_split": splits,
           "torch_chunk_rows": chunk, "budget_mib": budget_mib}
    for n in names:
        res[f"{n}_ms_median"] = float(np.median(ms[n]))
        res[f"{n}_ms_rounds"] = ms[n]
    if "kernel" in names:
        knn_ops._WS.clear()   # count the workspace as part of the call
        res["kernel_peak_added_bytes"] = _peak_added(kernel_route)
        res["kernel_ws_bytes"], res["kernel_out_bytes"] = knn_ops.knn_ws_bytes(cells, k, splits), cells * k * 8
        res["kernel_pair_terms_per_s"] = cells * cells * D / (res["kernel_ms_median"] * 1e-3)
        res["valu_bound_ms"] = cells * cells * D * 2 / VALU_LANE_OPS_PER_S * 1e3
        res["kernel_share_of_valu_bound"] = res["valu_bound_ms"] / res["kernel_ms_median"]
    if "torch" in names:
        res["torch_peak_added_bytes"] = _peak_added(torch_route)
        res["torch_chunk_temp_bytes"] = min(chunk, cells) * cells * 4
    if only == "all":
        (ti, td), (ki, kd) = torch_route(), kernel_route()
        res["rows_with_the_same_neighbours"] = float((ti.int() == ki).all(1).float().mean())
        res["max_rel_distance_difference"] = float(((td - kd).abs() / kd.clamp_min(1e-30)).max())
        res["kernel_over_torch"] = res["kernel_ms_median"] / res["torch_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--budget-mib", type=int, default=1024)
    ap.add_argument("--dims", type=int, nargs="+", default=[25, 35])
    ap.add_argument("--ks", type=int, nargs="+", default=[15, 50])
    ap.add_argument("--only", default="all", choices=["all", "torch", "kernel"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knn needs the GPU: there is no CPU timing of a GPU kernel")
    for D in a.dims:
        for k in a.ks:
            print(json.dumps(run(a.cells, D, k, a.steps, a.warmup, a.rounds, a.only, a.budget_mib)), flush=True)


if __name__ == "__main__":
    main()
