#!/usr/bin/env python3
"""Cost of one sample of the posterior-predictive check at C2's step shape (4096 cells x 10 000 genes, 25 / 10 latents, one group), bf16
and fp32 modes, with 1 and 20 populations, timed with device events after warm-up, in alternating rounds in one process:

    (a) sample_counts alone: decode and draw into one int32 [B, G] block (spv_dec_sample), for scale
    (b) the two-step route: sample_counts into the int32 block, then torch reductions of it -- sum, ``> 0``, the square in int64, max
        (per label by index_add_ / scatter_reduce_ when there are 20 populations) and the row sums
    (c) sample_count_stats: decode, draw and reduce in one fused kernel (spv_dec_sample_stats); no [B, G] array exists

    python tools/bench_ppc.py [--steps 20] [--warmup 5] [--rounds 3] [--precision bf16 fp32] [--segments 1 20]
    python tools/bench_ppc.py --only fused --precision bf16 --segments 20     # one path alone, e.g. under rocprofv3 --kernel-trace --stats

All paths run the same operand preparation; the times include it.  Prints one JSON line per (precision, segments) with the three
medians, (b) / (c), (c) / (a) -- what the atomics cost on top of the sampler -- whether both routes produced the same tables, and the
peak device memory each of (b) and (c) adds while it accumulates ``--samples`` (25) samples into its tables."""
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


def run(precision: str, n_seg: int, steps: int, warmup: int, rounds: int, only: str, samples: int, B: int = 4096, G: int = 10000) -> dict:
    from spvipes_amd import dec_ops
    from spvipes_amd.module import spVIPESmodule
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    module = spVIPESmodule({0: G, 1: G}, use_labels=True, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10, precision=precision).to(dev)
    module.eval()
    gen = torch.Generator().manual_seed(1)
    z_p, z_s = torch.randn(B, 10, generator=gen).to(dev), torch.randn(B, 25, generator=gen).to(dev)
    lib = (9.0 + 0.3 * torch.randn(B, generator=gen)).to(dev)   # ~8 000 counts per cell, 0.85 per element (tools/bench_sample.py's state)
    with torch.no_grad():
        module.px_r[0].copy_(torch.linspace(-2.0, 3.0, G)[torch.randperm(G, generator=gen)].to(dev))
    dec, px_r, ws, ns = module.decoders[0], module.px_r[0], module._workspace(0, dev), module.nsplit
    seg = torch.randint(0, n_seg, (B,), generator=gen).to(dev)   # cells in arbitrary label order: a 32-cell tile holds many labels
    seg32 = seg.int().contiguous()
    step = [0]

    def fresh():
        return torch.zeros((n_seg, 4, G), dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)

    state = {"two_step": fresh(), "fused": fresh(), "block": None}

    def block():
        if state["block"] is None:
            state["block"] = torch.empty(B, G, dtype=torch.int32, device=dev)
        return state["block"]

    def sample_only():
        step[0] += 1
        return dec_ops.sample_counts(dec, px_r, z_p, z_s, lib, False, ns, ws, key=1, sample=step[0], out=block())

    def two_step(sample=None):
        if sample is None:
            step[0] += 1
            sample = step[0]
        stats, total = state["two_step"]
        x = dec_ops.sample_counts(dec, px_r, z_p, z_s, lib, False, ns, ws, key=1, sample=sample, out=block())
        x64 = x.long()
        if n_seg == 1:
            stats[0, 0] += x64.sum(0)
            stats[0, 1] += (x > 0).sum(0)
            stats[0, 2] += (x64 * x64).sum(0)
            stats[0, 3] = torch.maximum(stats[0, 3], x64.amax(0))
        else:
            stats[:, 0].index_add_(0, seg, x64)
            stats[:, 1].index_add_(0, seg, (x > 0).long())
            stats[:, 2].index_add_(0, seg, x64 * x64)
            stats[:, 3].scatter_reduce_(0, seg[:, None].expand(B, G), x64, "amax", include_self=True)
        total += x64.sum(1)

    def fused(sample=None):
        if sample is None:
            step[0] += 1
            sample = step[0]
        stats, total = state["fused"]
        dec_ops.sample_count_stats(dec, px_r, z_p, z_s, lib, False, ns, ws, key=1, sample=sample, seg=seg32 if n_seg > 1 else None, n_seg=n_seg,
                                   stats=stats, cell_total=total)

    paths = {}
    if only == "all":
        paths["sample_counts_alone"] = sample_only
    if only in ("all", "two_step"):
        paths["two_step_route"] = two_step
    if only in ("all", "fused"):
        paths["fused_sample_count_stats"] = fused
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    res = {"precision": precision, "n_seg": n_seg, "B": B, "G": G, "steps": steps, "warmup": warmup, "rounds": rounds,
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        m = res["ms"]
        res["two_step_over_fused"] = round(m["two_step_route"] / m["fused_sample_count_stats"], 3)
        res["fused_over_sample_alone"] = round(m["fused_sample_count_stats"] / m["sample_counts_alone"], 3)
        # the same samples through both routes, from zeroed tables: equal tables, and what each route adds to the device's peak
        peak = {}
        for name, fn in (("two_step", two_step), ("fused", fused)):
            state["block"] = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            state[name] = fresh()
            for s in range(samples):
                fn(sample=s)
            torch.cuda.synchronize()
            peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        res["samples"] = samples
        res["peak_MiB_over_baseline"] = peak
        res["cube_MiB_if_stored"] = round(B * G * samples * 4 / 2 ** 20, 1)
        res["tables_equal"] = bool(torch.equal(state["two_step"][0], state["fused"][0]) and torch.equal(state["two_step"][1], state["fused"][1]))
        res["mean_count"] = float(state["fused"][0][:, 0].sum()) / (B * G * samples)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--segments", nargs="+", type=int, default=[1, 20])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--only", choices=["all", "two_step", "fused"], default="all")
    a = ap.parse_args()
    for p in a.precision:
        for k in a.segments:
            print(json.dumps(run(p, k, a.steps, a.warmup, a.rounds, a.only, a.samples)), flush=True)


if __name__ == "__main__":
    main()
