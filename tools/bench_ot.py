#!/usr/bin/env python3
"""Times the fused optimal-transport kernels against the torch route on the same inputs, with device events, and reads both routes'
additions to the device's peak memory (DESIGN.md section 20 holds the numbers).

  fused:  one spv_ot_softmin half-step; one spv_ot_topk pass (k entries per query).  Nothing of size n x n exists.
  torch:  the cost matrix ``torch.cdist(X, Y) ** 2`` materialised ONCE (timed on its own: a Sinkhorn run pays it once), then per
          half-step ``torch.logsumexp(h - s * C, dim=1)`` and for the plan ``topk`` of the same expression in chunks of the queries.

Per shape the two routes alternate, ``--rounds`` times; each figure is the median over the rounds of (a timed window of ``--reps`` calls
between two events) / reps, and the spread (min .. max over the rounds) is printed next to it.  Every shape is warmed up first.
The VALU figure is what the half-step needs by count -- 2 DP + 12 vector instructions per pair and lane (DP = D padded to 16 / 32 / 64:
a subtract and an fma per dimension, then t, the test, the difference, the exp argument, exp, the update) -- over the time, next to the
39.3 T lane-instructions/s of 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz (unpacked fp32).

    python tools/bench_ot.py [--cells 25000 50000] [--dims 10 25 50] [--k 32] [--reps 5] [--rounds 3] [--skip-torch-above N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

VALU_PEAK = 256 * 4 * 16 * 2.4e9   # lane-instructions per second, unpacked fp32


def clouds(n, D, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = 3.0 * torch.randn(8, D, generator=g)
    return [(centres[torch.randint(0, 8, (n,), generator=g)] + torch.randn(n, D, generator=g)).to(dev) for _ in range(2)]


def timed(fn, reps):
    """milliseconds per call of a window of ``reps`` calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_added(fn):
    """bytes a call adds to the device's peak allocation (allocator statistics: torch's own tensors, the workspace included)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[25000, 50000])
    ap.add_argument("--dims", type=int, nargs="+", default=[10, 25, 50])
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4096, help="queries per topk chunk of the torch route")
    ap.add_argument("--skip-torch-above", type=int, default=10 ** 9, help="no torch route beyond this many cells per group")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ot: needs the MI355X (there is nothing to time on a CPU)")
    from spvipes_amd import knn_ops
    from spvipes_amd.ot_ops import mean_sq_cost, ot_softmin, ot_splits, ot_topk
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))
    for n in a.cells:
        for D in a.dims:
            X, Y = clouds(n, D, 1000 + D, dev)
            s = float(np.float32(1.0 / (0.05 * mean_sq_cost(X, Y))))
            h = torch.full((n,), -float(np.log(n)), device=dev)
            r = torch.zeros(n, device=dev)
            L = torch.empty(n, device=dev)
            with_torch = n <= a.skip_torch_above
            fused_half = lambda: ot_softmin(X, Y, h, s, out=L)
            fused_topk = lambda: ot_topk(X, Y, h, r, s, a.k)
            torch_cost = lambda: torch.cdist(X, Y) ** 2
            rec = {"cells": n, "D": D, "k": a.k, "n_split": ot_splits(n, n), "inv_eps": s}
            C = None
            if with_torch:
                rec["torch_cost_peak_bytes"] = peak_added(torch_cost)
                C = torch_cost()
            torch_half = lambda: torch.logsumexp(h[None, :] - s * C, dim=1)
            torch_topk = lambda: [torch.topk(h[None, :] - s * C[q:q + a.chunk], a.k, dim=1) for q in range(0, n, a.chunk)]
            fused_half(), fused_topk()   # warm-up of every timed form at this shape
            if with_torch:
                torch_half(), torch_topk(), torch_cost()
                # the two routes agree: same potentials up to the cost's rounding (cdist forms |x|^2 + |y|^2 - 2 x.y)
                rec["max_abs_L_difference"] = float((fused_half() - torch_half()).abs().max())
            torch.cuda.synchronize()
            t = {key: [] for key in ("fused_half", "fused_topk", "torch_half", "torch_topk", "torch_cost")}
            for _ in range(a.rounds):
                t["fused_half"].append(timed(fused_half, a.reps))
                if with_torch:
                    t["torch_half"].append(timed(torch_half, a.reps))
                t["fused_topk"].append(timed(fused_topk, a.reps))
                if with_torch:
                    t["torch_topk"].append(timed(torch_topk, a.reps))
                    t["torch_cost"].append(timed(torch_cost, 1))
            for key, v in t.items():
                if v:
                    rec[key + "_ms"], rec[key + "_ms_min_max"] = med(v), [min(v), max(v)]
            knn_ops._WS.clear()
            rec["fused_half_peak_bytes"] = peak_added(lambda: ot_softmin(X, Y, h, s))
            knn_ops._WS.clear()
            rec["fused_topk_peak_bytes"] = peak_added(fused_topk)
            if with_torch:
                rec["torch_half_peak_bytes"] = peak_added(torch_half) + C.numel() * 4   # the matrix itself stays allocated across half-steps
                rec["torch_topk_peak_bytes"] = peak_added(torch_topk) + C.numel() * 4
            DP = 16 if D <= 16 else 32 if D <= 32 else 64
            rec["fused_half_valu_share"] = float(n) * n * (2 * DP + 12) / (rec["fused_half_ms"] * 1e-3) / VALU_PEAK
            print(json.dumps(rec), flush=True)
            del C


if __name__ == "__main__":
    main()
