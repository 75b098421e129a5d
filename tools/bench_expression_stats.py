#!/usr/bin/env python3
"""Cost of one minibatch of expression_statistics at C2's step shape (4096 cells x 10 000 genes, 25 / 10 latents, one group), bf16 and
fp32 modes, with 1 population and with 20 labels drawn at random per cell, timed with device events after warm-up, in alternating
rounds in one process (tools/bench_ppc.py's protocol):

    (a) expected_expression alone: ONE decode of one value into an fp32 [B, G] block (spv_dec_expected), for scale
    (b) the torch route: four expected_expression calls (mixture, private, shared, mixing) into fp32 blocks, each widened to fp64 and
        reduced -- sum and sum of squares per label, by ``sum(0)`` for one population and by ``index_add_`` for 20
    (c) expected_expression_stats with the step's tile plan made on the host as the method makes it (data.expression_tile_plan, three
        small uploads, the gather of the latents by ``perm``), then decode and reduce in spv_dec_expected_stats; no [B, G] array exists
    (d) the same with the plan and the gathered latents prepared once: the entry point alone

    python tools/bench_expression_stats.py [--steps 20] [--warmup 5] [--rounds 3] [--precision bf16 fp32] [--segments 1 20]
    python tools/bench_expression_stats.py --only fused --precision bf16 --segments 20     # one path alone, e.g. under a kernel trace

All paths run the same operand preparation; the times include it.  Prints one JSON line per (precision, segments) with the medians,
(b) / (c), (d) / (a) -- what the reduction stage costs on top of one decode -- the largest relative difference between the two routes'
tables, the padded rows of the plan, and the peak device memory each of (b) and (c) adds over the baseline."""
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


def run(precision: str, n_seg: int, steps: int, warmup: int, rounds: int, only: str, B: int = 4096, G: int = 10000) -> dict:
    from spvipes_amd import dec_ops
    from spvipes_amd.data import expression_tile_plan
    from spvipes_amd.module import spVIPESmodule
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    module = spVIPESmodule({0: G, 1: G}, use_labels=True, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10, precision=precision).to(dev)
    module.eval()
    gen = torch.Generator().manual_seed(1)
    z_p, z_s = torch.randn(B, 10, generator=gen).to(dev), torch.randn(B, 25, generator=gen).to(dev)
    lib = (9.0 + 0.3 * torch.randn(B, generator=gen)).to(dev)   # ~8 000 counts per cell (tools/bench_sample.py's state)
    with torch.no_grad():
        module.px_r[0].copy_(torch.linspace(-2.0, 3.0, G)[torch.randperm(G, generator=gen)].to(dev))
    dec, px_r, ws, ns = module.decoders[0], module.px_r[0], module._workspace(0, dev), module.nsplit
    seg_host = torch.randint(0, n_seg, (B,), generator=gen).numpy()   # cells in arbitrary label order
    seg = torch.as_tensor(seg_host, device=dev)

    def fresh():
        return torch.zeros((n_seg, 8, G), dtype=torch.float64, device=dev)

    state = {"torch": fresh(), "fused": fresh(), "block": None}

    def block():
        if state["block"] is None:
            state["block"] = torch.empty(B, G, dtype=torch.float32, device=dev)
        return state["block"]

    def expected_alone():
        return dec_ops.expected_expression(dec, px_r, z_p, z_s, lib, False, ns, ws, what=0, out=block())

    def torch_route():
        stats = state["torch"]
        for w in range(4):
            x = dec_ops.expected_expression(dec, px_r, z_p, z_s, lib, False, ns, ws, what=w, out=block()).double()
            if n_seg == 1:
                stats[0, w] += x.sum(0)
                stats[0, 4 + w] += (x * x).sum(0)
            else:
                stats[:, w].index_add_(0, seg, x)
                stats[:, 4 + w].index_add_(0, seg, x * x)

    def plan():
        perm, tile_seg, tile_n = expression_tile_plan(seg_host, n_seg)
        perm, tile_seg, tile_n = (torch.as_tensor(t, device=dev) for t in (perm, tile_seg, tile_n))
        take = lambda t: t.index_select(0, perm).contiguous()
        return take(z_p), take(z_s), take(lib), tile_seg, tile_n

    def fused(planned=None):
        f, s, l, tile_seg, tile_n = planned or plan()
        dec_ops.expected_expression_stats(dec, px_r, f, s, l, False, ns, ws, tile_seg=tile_seg, tile_n=tile_n, n_seg=n_seg, stats=state["fused"], batch_rows=B)

    ready = plan()
    paths = {}
    if only == "all":
        paths["expected_expression_alone"] = expected_alone
    if only in ("all", "torch"):
        paths["torch_route"] = torch_route
    if only in ("all", "fused"):
        paths["fused_with_host_plan"] = fused
        paths["fused_entry_point_alone"] = lambda: fused(ready)
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    rows = int(ready[0].shape[0])
    res = {"precision": precision, "n_seg": n_seg, "B": B, "G": G, "steps": steps, "warmup": warmup, "rounds": rounds,
           "rows_decoded": rows, "padded_rows": rows - B, "cell_tiles": rows // 32,
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        m = res["ms"]
        res["torch_over_fused"] = round(m["torch_route"] / m["fused_with_host_plan"], 3)
        res["fused_alone_over_expected_alone"] = round(m["fused_entry_point_alone"] / m["expected_expression_alone"], 3)
        # one step through both routes, from zeroed tables: how far the tables are apart, and what each route adds to the device's peak
        peak = {}
        for name, fn in (("torch", torch_route), ("fused", fused)):
            state["block"] = None
            ws._buf.pop(next((k for k in ws._buf if k[0] == "mat_xstats"), None), None)   # the fused route's partial sums count as its own
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            state[name] = fresh()
            fn()
            torch.cuda.synchronize()
            peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        res["peak_MiB_over_baseline"] = peak
        a, b = state["torch"], state["fused"]
        res["max_relative_difference"] = float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())
        res["mean_expression"] = float(b[:, 0].sum()) / (B * G)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--segments", nargs="+", type=int, default=[1, 20])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "torch", "fused"], default="all")
    a = ap.parse_args()
    for p in a.precision:
        for k in a.segments:
            print(json.dumps(run(p, k, a.steps, a.warmup, a.rounds, a.only)), flush=True)


if __name__ == "__main__":
    main()
