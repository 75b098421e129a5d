#!/usr/bin/env python3
"""Times one iteration of the exact t-SNE (spv_tsne_repulsion, spv_tsne_update) against a Sinkhorn half-step and a chunked torch route on
the same layout, with device events, reads every route's addition to the device's peak memory, and times a whole layout (DESIGN.md
section 24 holds the numbers).

  fused:   repulsion at the automatic chunk count (partial pass and merge pass), repulsion in one chunk (one launch, no merge),
           update (the sum of Zrow and the sparse half with the step), and the two entry points together: one iteration.
           The affinities are real ones: k-NN, calibration and symmetrisation of a D = 10 cloud, perplexity 30.
  half:    one ot_softmin half-step at D = 10 on the cloud the layout belongs to, in the same run: the yardstick.
  torch:   in chunks of the queries ``torch.cdist`` on the 2-D points, elementwise ops and row sums for Zrow and F.
  layout:  ``tsne_ops.tsne`` with its defaults (1000 steps), wall clock, for the sizes of ``--layout``.

Per size the routes alternate, ``--rounds`` times; each figure is the median over the rounds of (a timed window of ``--reps`` calls
between two events) / reps, and the spread (min .. max over the rounds) is printed next to it.  Every size is warmed up first.

    python tools/bench_tsne.py [--cells 25000 50000 100000] [--layout 25000 50000] [--reps 5] [--rounds 3] [--chunk 2048]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from tools.bench_ot import clouds, peak_added, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[25000, 50000, 100000])
    ap.add_argument("--layout", type=int, nargs="*", default=[25000, 50000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=2048, help="queries per chunk of the torch route")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tsne: needs the MI355X (there is nothing to time on a CPU)")
    from spvipes_amd import knn_ops
    from spvipes_amd.data import tsne_symmetrize
    from spvipes_amd.knn_ops import knn
    from spvipes_amd.ot_ops import mean_sq_cost, ot_softmin
    from spvipes_amd.tsne_ops import affinities, repulsion, tsne, tsne_splits, update
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))
    for n in a.cells:
        X, X2 = clouds(n, 10, 1010, dev)
        me = torch.arange(n, dtype=torch.int32, device=dev)
        idx, d2 = knn(X, X, 64, exclude=me)
        P, _beta = affinities(d2.contiguous(), 30.0)
        indptr, cols, vals = (torch.from_numpy(v).to(dev) for v in tsne_symmetrize(idx.cpu().numpy(), P.cpu().numpy(), n))
        Y = (torch.randn((n, 2), generator=torch.Generator(device="cpu").manual_seed(n)) * 20).to(dev)   # a layout of the size a finished one has
        Y1, u, gain = torch.empty_like(Y), torch.zeros_like(Y), torch.ones_like(Y)
        Zrow, F = torch.empty(n, dtype=torch.float64, device=dev), torch.empty((2, n), dtype=torch.float64, device=dev)
        Z, kl = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
        s = float(np.float32(1.0 / (0.05 * mean_sq_cost(X, X2))))
        h, L1 = torch.full((n,), -float(np.log(n)), device=dev), torch.empty(n, device=dev)
        rep = lambda: repulsion(Y, Y, exclude=me, out=(Zrow, F))
        rep1 = lambda: repulsion(Y, Y, exclude=me, n_split=1, out=(Zrow, F))
        upd = lambda: update(Y, Y1, indptr, cols, vals, Zrow, F, Z, u, gain, 1.0, 0.8, 200.0)
        upd_kl = lambda: update(Y, Y1, indptr, cols, vals, Zrow, F, Z, u, gain, 1.0, 0.8, 200.0, kl_row=kl)
        both = lambda: (rep(), upd())
        half = lambda: ot_softmin(X, X2, h, s, out=L1)

        def route():
            zs, fs = [], []
            for q in range(0, n, a.chunk):
                w = 1.0 / (1.0 + torch.cdist(Y[q:q + a.chunk], Y) ** 2)
                zs.append(w.sum(dim=1) - 1.0)   # the self pair
                w = w * w
                fs.append(torch.stack([(w * (Y[q:q + a.chunk, t, None] - Y[None, :, t])).sum(dim=1) for t in range(2)]))
            return torch.cat(zs), torch.cat(fs, dim=1)

        rec = {"cells": n, "n_split": tsne_splits(n, n), "nnz": int(cols.numel())}
        rep(), rep1(), upd(), half()
        zt, ft = route()
        rep()
        rec["max_rel_difference_Z"] = float(((Zrow - zt.double()).abs() / Zrow).max())   # the torch route is fp32 throughout
        torch.cuda.synchronize()
        t = {key: [] for key in ("repulsion", "repulsion_one_chunk", "update", "update_with_kl", "iteration", "softmin_half", "torch")}
        for _ in range(a.rounds):
            for key, fn in (("repulsion", rep), ("repulsion_one_chunk", rep1), ("update", upd), ("update_with_kl", upd_kl), ("iteration", both),
                            ("softmin_half", half), ("torch", route)):
                t[key].append(timed(fn, a.reps))
        for key, v in t.items():
            rec[key + "_ms"], rec[key + "_ms_min_max"] = med(v), [min(v), max(v)]
        rec["iteration_over_half_step"] = rec["iteration_ms"] / rec["softmin_half_ms"]
        rec["update_share"] = rec["update_ms"] / rec["iteration_ms"]
        rec["repulsion_over_torch"] = rec["repulsion_ms"] / rec["torch_ms"]
        knn_ops._WS.clear()
        rec["fused_peak_bytes"] = peak_added(lambda: repulsion(Y, Y, exclude=me))
        rec["torch_peak_bytes"] = peak_added(route)
        print(json.dumps(rec), flush=True)
    for n in a.layout:
        X, _ = clouds(n, 10, 1010, dev)
        tsne(X, n_iter=5)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = tsne(X)
        torch.cuda.synchronize()
        print(json.dumps({"layout_cells": n, "n_iter": 1000, "seconds": time.perf_counter() - t0, "kl_divergence": r.kl_divergence,
                          "kl_at_250": float(r.kl_history[5, 1])}), flush=True)


if __name__ == "__main__":
    main()
