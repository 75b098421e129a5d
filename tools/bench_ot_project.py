#!/usr/bin/env python3
"""Times the fused barycentric projection (spv_ot_project) against a Sinkhorn half-step and a torch route on the same inputs, with
device events, and reads every route's addition to the device's peak memory (DESIGN.md section 23 holds the numbers).

  fused:   one ot_project call: the plan-weighted mean of n_v value columns for every query.  Nothing of size n x n exists.  In the
           same run and at the same shape one ot_softmin half-step, the yardstick the issue's estimate (1.3 to 1.5 half-steps for one
           column block at DP 32) is held against.
  torch:   the cost matrix ``torch.cdist(X, Y) ** 2`` materialised ONCE beforehand (not timed), then in chunks of the queries
           ``torch.softmax(h - s * C[q:q + chunk], dim=1) @ V``.

Per shape the routes alternate, ``--rounds`` times; each figure is the median over the rounds of (a timed window of ``--reps`` calls
between two events) / reps, and the spread (min .. max over the rounds) is printed next to it.  Every shape is warmed up first.
``--values``: the numbers of value columns; 0 stands for one column block of the kernel form that serves D.

    python tools/bench_ot_project.py [--cells 25000 50000] [--dims 10 25 50] [--values 1 0 64] [--reps 5] [--rounds 3] [--skip-torch-above N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tools.bench_ot import clouds, peak_added, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[25000, 50000])
    ap.add_argument("--dims", type=int, nargs="+", default=[10, 25, 50])
    ap.add_argument("--values", type=int, nargs="+", default=[1, 0, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4096, help="queries per chunk of the torch route")
    ap.add_argument("--skip-torch-above", type=int, default=10 ** 9, help="no torch route beyond this many cells per group")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ot_project: needs the MI355X (there is nothing to time on a CPU)")
    from spvipes_amd import knn_ops
    from spvipes_amd.ot_ops import mean_sq_cost, ot_project, ot_project_block, ot_project_splits, ot_softmin, ot_splits
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))
    for n in a.cells:
        for D in a.dims:
            X, Y = clouds(n, D, 1000 + D, dev)
            s = float(np.float32(1.0 / (0.05 * mean_sq_cost(X, Y))))
            h = torch.full((n,), -float(np.log(n)), device=dev)
            L1 = torch.empty(n, device=dev)
            with_torch = n <= a.skip_torch_above
            C = (torch.cdist(X, Y) ** 2) if with_torch else None
            for n_v in [v or ot_project_block(D) for v in a.values]:
                V = torch.randn((n, n_v), generator=torch.Generator(device="cpu").manual_seed(n_v)).to(dev)
                out = torch.empty((n_v, n), device=dev)
                fused = lambda: ot_project(X, Y, h, V, s, out=out)
                half = lambda: ot_softmin(X, Y, h, s, out=L1)
                route = lambda: [torch.softmax(h[None, :] - s * C[q:q + a.chunk], dim=1) @ V for q in range(0, n, a.chunk)]
                rec = {"cells": n, "D": D, "n_v": n_v, "block": ot_project_block(D), "n_split": ot_project_splits(n, n, n_v), "softmin_n_split": ot_splits(n, n),
                       "inv_eps": s}
                fused(), half()   # warm-up of every timed form at this shape
                if with_torch:
                    route()
                    # the routes agree up to the cost's rounding (cdist forms |x|^2 + |y|^2 - 2 x.y)
                    rec["max_abs_difference"] = float((fused() - torch.cat(route(), dim=0)).abs().max())
                torch.cuda.synchronize()
                t = {key: [] for key in ("fused", "softmin_half", "torch")}
                for _ in range(a.rounds):
                    t["fused"].append(timed(fused, a.reps))
                    t["softmin_half"].append(timed(half, a.reps))
                    if with_torch:
                        t["torch"].append(timed(route, a.reps))
                for key, v in t.items():
                    if v:
                        rec[key + "_ms"], rec[key + "_ms_min_max"] = med(v), [min(v), max(v)]
                rec["fused_over_half_step"] = rec["fused_ms"] / rec["softmin_half_ms"]
                if with_torch:
                    rec["fused_over_torch"] = rec["fused_ms"] / rec["torch_ms"]
                knn_ops._WS.clear()
                rec["fused_peak_bytes"] = peak_added(lambda: ot_project(X, Y, h, V, s))
                if with_torch:
                    rec["torch_cost_bytes"] = C.numel() * 4   # the matrix itself stays allocated across the calls
                    rec["torch_peak_bytes"] = peak_added(route) + C.numel() * 4
                print(json.dumps(rec), flush=True)
            del C


if __name__ == "__main__":
    main()
