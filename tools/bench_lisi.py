#!/usr/bin/env python3
"""Cost of the LISI read-out of spVIPES.latent_lisi / spVIPES.lisi (knn_ops.knn_paged -> spv_knn_paged, lisi_ops.lisi -> spv_lisi)
against the torch route on the same device tensor, timed with device events after warm-up, in alternating rounds in one process:

    (a) torch: per chunk of cells ``torch.cdist(x, X) ** 2``, the cell's own column set to +inf, ``.topk(k, largest=False)``; the chunk is
        sized so that ONE chunk x cells fp32 temporary stays within --budget-mib (the route holds two at a time: cdist's result and its
        square).  The neighbours only: the route has no Simpson step of its own, so its time is a LOWER bound of a torch-only LISI
    (b) the pages: knn_paged with the cell itself excluded, nothing of size cells x cells stored
    (c) the Simpson kernel on (b)'s lists, two label sets (2 groups, 12 labels)
    (d) the whole call: (b) + (c) and the two small code tensors, as ``spVIPES.lisi`` runs them

    python tools/bench_lisi.py [--steps 5] [--warmup 1] [--rounds 3] [--cells 25000 50000] [--dims 10 25 35] [--perplexity 30]
    python tools/bench_lisi.py --only pages        # one route alone, e.g. under rocprofv3 --kernel-trace --stats

Prints one JSON line per shape: the medians (ms), each route's addition to the device's peak allocated memory during one call (outputs
and workspace included), and how many rows of the two routes name the same neighbours (the torch route's distances come from another
formula, so near-ties may swap).  Then one line per D with ``knn_paged`` at k = 64 against ``knn`` at k = 64 on the largest shape: one page
is the same two launches."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tools.bench_knn import _peak_added, _timed


def run(cells: int, D: int, perplexity: float, steps: int, warmup: int, rounds: int, only: str, budget_mib: int) -> dict:
    from spvipes_amd import knn_ops
    from spvipes_amd.data import check_lisi_args
    from spvipes_amd.lisi_ops import lisi
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(D * 100 + cells)
    X = torch.randn(cells, D, generator=g).to(dev)
    k = check_lisi_args(cells, perplexity)
    me = torch.arange(cells, dtype=torch.int32, device=dev)
    host_codes = np.stack([np.arange(cells) % 2, np.arange(cells) % 12]).astype(np.int32)
    codes = torch.from_numpy(host_codes).to(dev)
    chunk = max(1, (budget_mib << 20) // (cells * 4))

    def torch_route():
        idx, dist = torch.empty((cells, k), dtype=torch.int64, device=dev), torch.empty((cells, k), dtype=torch.float32, device=dev)
        for lo in range(0, cells, chunk):
            d = torch.cdist(X[lo:lo + chunk], X) ** 2
            d[torch.arange(d.shape[0], device=dev), torch.arange(lo, lo + d.shape[0], device=dev)] = float("inf")
            d, i = d.topk(k, dim=1, largest=False, sorted=True)
            idx[lo:lo + chunk], dist[lo:lo + chunk] = i, d
        return idx, dist

    def pages():
        return knn_ops.knn_paged(X, X, k, exclude=me)

    lists = pages()

    def simpson():
        return lisi(lists[0], lists[1], codes, perplexity)

    def whole():
        idx, d2 = knn_ops.knn_paged(X, X, k, exclude=torch.arange(cells, dtype=torch.int32, device=dev))
        return lisi(idx, d2, torch.from_numpy(host_codes).to(dev), perplexity)

    routes = {"torch": torch_route, "pages": pages, "simpson": simpson, "whole": whole}
    names = list(routes) if only == "all" else [only]
    ms = {n: [] for n in names}
    for _ in range(rounds):
        for n in names:
            ms[n].append(_timed(routes[n], steps, warmup))
    splits = knn_ops.knn_splits(cells, cells)
    res = {"cells": cells, "D": D, "perplexity": perplexity, "k": k, "pages": (k + 63) // 64, "steps": steps, "warmup": warmup, "rounds": rounds,
           "n_split": splits, "torch_chunk_rows": chunk, "budget_mib": budget_mib}
    for n in names:
        res[f"{n}_ms_median"] = float(np.median(ms[n]))
        res[f"{n}_ms_rounds"] = ms[n]
    for n in names:
        knn_ops._WS.clear()   # count the workspace as part of the call
        res[f"{n}_peak_added_bytes"] = _peak_added(routes[n])
    if "pages" in names:
        res["pages_ws_bytes"], res["pages_out_bytes"] = knn_ops.knn_paged_ws_bytes(cells, k, splits), cells * k * 8
    if only == "all":
        (ti, td), (ki, kd) = torch_route(), pages()
        res["rows_with_the_same_neighbours"] = float((ti.int() == ki).all(1).float().mean())
        res["whole_over_torch_neighbours"] = res["whole_ms_median"] / res["torch_ms_median"]
        out, _beta, _nv, conv = simpson()
        res["ilisi_median"], res["clisi_median"], res["n_unconverged"] = float(out[0].median()), float(out[1].median()), int((conv == 0).sum())
    return res


def run_page_zero(cells: int, D: int, steps: int, warmup: int, rounds: int) -> dict:
    """knn_paged at k = 64 (one page) against knn at k = 64: the same kernels, alternating rounds"""
    from spvipes_amd import knn_ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(D)
    X = torch.randn(cells, D, generator=g).to(dev)
    routes = {"knn_k64": lambda: knn_ops.knn(X, X, 64), "knn_paged_k64": lambda: knn_ops.knn_paged(X, X, 64)}
    ms = {n: [] for n in routes}
    for _ in range(rounds):
        for n in routes:
            ms[n].append(_timed(routes[n], steps, warmup))
    a, b = routes["knn_k64"](), routes["knn_paged_k64"]()
    res = {"cells": cells, "D": D, "k": 64, "same_bits": bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))}
    for n in routes:
        res[f"{n}_ms_median"], res[f"{n}_ms_rounds"] = float(np.median(ms[n])), ms[n]
    res["paged_over_knn"] = res["knn_paged_k64_ms_median"] / res["knn_k64_ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cells", type=int, nargs="+", default=[25000, 50000])
    ap.add_argument("--dims", type=int, nargs="+", default=[10, 25, 35])
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--budget-mib", type=int, default=1024)
    ap.add_argument("--only", default="all", choices=["all", "torch", "pages", "simpson", "whole"])
    ap.add_argument("--no-page-zero", action="store_true", help="skip the knn_paged / knn comparison at k = 64")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lisi needs the GPU: there is no CPU timing of a GPU kernel")
    for cells in a.cells:
        for D in a.dims:
            print(json.dumps(run(cells, D, a.perplexity, a.steps, a.warmup, a.rounds, a.only, a.budget_mib)), flush=True)
    if not a.no_page_zero and a.only == "all":
        for D in a.dims:
            print(json.dumps(run_page_zero(max(a.cells), D, a.steps, a.warmup, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
