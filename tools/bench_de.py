#!/usr/bin/env python3
"""Cost of the differential-expression reduction on device-resident sample banks (two fp32 banks of 4096 rows, 10 000 pairs, delta
0.25), at 10 000 / 1 000 / 64 genes, timed with device events after warm-up, in alternating rounds in one process:

    (a) the torch route on the same banks: two index_selects, log2, subtract, abs() >= delta, mean / std / amin / amax, two more means
    (b) de_ops.de_pairs                                                       -- one fused gather-compare-reduce kernel + its combine

    python tools/bench_de.py [--steps 20] [--warmup 5] [--rounds 3]
    python tools/bench_de.py --only kernel --genes 10000        # one path alone, e.g. under rocprofv3 --kernel-trace --stats

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", nargs="+", type=int, default=[10_000, 1_000, 64])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "torch", "kernel"], default="all")
    a = ap.parse_args()
    for n in a.genes:
        print(json.dumps(run(n, a.steps, a.warmup, a.rounds, a.only)), flush=True)


if __name__ == "__main__":
    main()
