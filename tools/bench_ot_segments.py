#!/usr/bin/env python3
"""Times the fused segmented log-sum-exp (spv_ot_segment_lse) against two torch routes on the same inputs, with device events, and
reads every route's addition to the device's peak memory (DESIGN.md section 22 holds the numbers).

  fused:    one ot_segment_lse call: the log mass of every (query, segment).  Nothing of size n x n exists.  In the same run and at
            the same shape one ot_softmin half-step, the yardstick "about one half-step" is held against.
  slices:   the cost matrix ``torch.cdist(X, Y) ** 2`` materialised ONCE (timed on its own), then per segment
            ``torch.logsumexp(h[a:b] - s * C[:, a:b], dim=1)``.
  one-hot:  the same matrix; in chunks of the queries x = h - s * C[q:q + chunk], its row maximum m, ``exp(x - m) @ onehot``
            [n, n_seg] and log(.) + m.

Per shape the routes alternate, ``--rounds`` times; each figure is the median over the rounds of (a timed window of ``--reps`` calls
between two events) / reps, and the spread (min .. max over the rounds) is printed next to it.  Every shape is warmed up first.
Segments are of equal size (the last takes the remainder).

    python tools/bench_ot_segments.py [--cells 25000 50000] [--dims 10 25 50] [--segments 8 32] [--reps 5] [--rounds 3] [--skip-torch-above N]"""
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
    ap.add_argument("--segments", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4096, help="queries per chunk of the one-hot route")
    ap.add_argument("--skip-torch-above", type=int, default=10 ** 9, help="no torch routes beyond this many cells per group")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ot_segments: needs the MI355X (there is nothing to time on a CPU)")
    from spvipes_amd import knn_ops
    from spvipes_amd.ot_ops import mean_sq_cost, ot_segment_lse, ot_segment_splits, ot_softmin, ot_splits
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
            for n_seg in a.segments:
                cuts = [min(k * (n // n_seg), n) for k in range(n_seg)] + [n]
                seg_ptr = torch.tensor(cuts, dtype=torch.int32, device=dev)
                out = torch.empty((n_seg, n), device=dev)
                onehot = torch.zeros((n, n_seg), device=dev)
                for k in range(n_seg):
                    onehot[cuts[k]:cuts[k + 1], k] = 1.0
                fused = lambda: ot_segment_lse(X, Y, h, seg_ptr, s, out=out)
                half = lambda: ot_softmin(X, Y, h, s, out=L1)
                slices = lambda: [torch.logsumexp(h[None, cuts[k]:cuts[k + 1]] - s * C[:, cuts[k]:cuts[k + 1]], dim=1) for k in range(n_seg)]

                def one_hot():
                    parts = []
                    for q in range(0, n, a.chunk):
                        x = h[None, :] - s * C[q:q + a.chunk]
                        m = x.max(dim=1, keepdim=True).values
                        parts.append(torch.log(torch.exp(x - m) @ onehot) + m)
                    return parts
                rec = {"cells": n, "D": D, "n_seg": n_seg, "n_split": ot_segment_splits(n, n), "softmin_n_split": ot_splits(n, n), "inv_eps": s}
                fused(), half()   # warm-up of every timed form at this shape
                if with_torch:
                    slices(), one_hot()
                    # the routes agree up to the cost's rounding (cdist forms |x|^2 + |y|^2 - 2 x.y)
                    rec["max_abs_L_difference_slices"] = float((fused() - torch.stack(slices(), dim=1)).abs().max())
                    rec["max_abs_L_difference_one_hot"] = float((fused() - torch.cat(one_hot(), dim=0)).abs().max())
                torch.cuda.synchronize()
                t = {key: [] for key in ("fused", "softmin_half", "torch_slices", "torch_one_hot")}
                for _ in range(a.rounds):
                    t["fused"].append(timed(fused, a.reps))
                    t["softmin_half"].append(timed(half, a.reps))
                    if with_torch:
                        t["torch_slices"].append(timed(slices, a.reps))
                        t["torch_one_hot"].append(timed(one_hot, a.reps))
                for key, v in t.items():
                    if v:
                        rec[key + "_ms"], rec[key + "_ms_min_max"] = med(v), [min(v), max(v)]
                rec["fused_over_half_step"] = rec["fused_ms"] / rec["softmin_half_ms"]
                knn_ops._WS.clear()
                rec["fused_peak_bytes"] = peak_added(lambda: ot_segment_lse(X, Y, h, seg_ptr, s))
                if with_torch:
                    rec["torch_cost_bytes"] = C.numel() * 4   # the matrix itself stays allocated across the calls
                    rec["torch_slices_peak_bytes"] = peak_added(slices) + C.numel() * 4
                    rec["torch_one_hot_peak_bytes"] = peak_added(one_hot) + C.numel() * 4
                print(json.dumps(rec), flush=True)
            del C


if __name__ == "__main__":
    main()
