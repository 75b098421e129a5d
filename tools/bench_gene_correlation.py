#!/usr/bin/env python3
"""Cost of one minibatch of get_feature_correlation_matrix at C2's step shape (4096 cells of a 10 000-gene group, 25 / 10 latents), bf16 and
fp32 modes, 64 / 512 / 2048 selected genes, timed with device events after warm-up, in alternating rounds in one process
(tools/bench_ppc.py's protocol):

    (a) expected_expression alone: ONE decode of the selection into an fp32 [B, n_sel] block (spv_dec_expected), for scale
    (b) the torch route: that decode, the block widened to fp64, then C += X.T @ X (the vendor dgemm) and S += X.sum(0)
    (b') its reduction alone on a block decoded once: widen, dgemm, column sums, the two adds;  (b'') the dgemm alone on a block
        widened once (``C.addmm_(X.T, X)``)
    (c) that decode and gram_accumulate (spv_gram_f64, the fp64 MFMA kernel) on the fp32 block: no fp64 copy of the block exists
    (d) gram_accumulate alone on a block decoded once

    python tools/bench_gene_correlation.py [--steps 20] [--warmup 5] [--rounds 3] [--precision bf16 fp32] [--genes 64 512 2048]
    python tools/bench_gene_correlation.py --only gram --precision bf16 --genes 2048     # one path alone, e.g. under a kernel trace

Prints one JSON line per (precision, n_sel) with the medians, (b) / (c), (b') / (d) and (b'') / (d) -- the margin to quote is (d) against the
dgemm part of (b) in the same run, whichever way it falls --, the rate of (d) in fp64 multiply-adds per second counting the FULL table
(what the dgemm computes; the kernel computes the upper triangle and mirrors it), the slab count and workspace of the shape, the largest
relative difference between the two routes' tables, and the peak device memory each of (b) and (c) adds over the baseline."""
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


def run(precision: str, n_sel: int, steps: int, warmup: int, rounds: int, only: str, B: int = 4096, G: int = 10000) -> dict:
    from spvipes_amd import dec_ops
    from spvipes_amd.gram_ops import gram_accumulate, gram_slabs, gram_workspace
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
    genes = torch.randperm(G, generator=gen)[:n_sel].sort().values.to(torch.int32).to(dev)

    def fresh():
        return torch.zeros(n_sel, dtype=torch.float64, device=dev), torch.zeros((n_sel, n_sel), dtype=torch.float64, device=dev)

    state = {"torch": fresh(), "gram": fresh(), "block": None, "gws": None}

    def block():
        if state["block"] is None:
            state["block"] = torch.empty(B, n_sel, dtype=torch.float32, device=dev)
        return state["block"]

    def decode():
        return dec_ops.expected_expression(dec, px_r, z_p, z_s, lib, False, ns, ws, genes=genes, what=0, out=block())

    def torch_reduce(x):
        S, Cm = state["torch"]
        xd = x.double()
        Cm += xd.t() @ xd
        S += xd.sum(0)

    def gram_reduce(x):
        if state["gws"] is None:
            state["gws"] = gram_workspace(n_sel, B, dev)
        S, Cm = state["gram"]
        gram_accumulate(x, sums=S, gram=Cm, ws=state["gws"])

    ready = decode().clone()
    ready64 = ready.double()
    paths = {}
    if only == "all":
        paths["expected_expression_alone"] = decode
    if only in ("all", "torch"):
        paths["torch_route"] = lambda: torch_reduce(decode())
        paths["torch_reduction_alone"] = lambda: torch_reduce(ready)
        paths["torch_dgemm_alone"] = lambda: state["torch"][1].addmm_(ready64.t(), ready64)
    if only in ("all", "gram"):
        paths["gram_route"] = lambda: gram_reduce(decode())
        paths["gram_accumulate_alone"] = lambda: gram_reduce(ready)
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    res = {"precision": precision, "n_sel": n_sel, "B": B, "G": G, "steps": steps, "warmup": warmup, "rounds": rounds,
           "slabs": gram_slabs(n_sel, B), "workspace_MiB": round(gram_workspace(n_sel, B, "meta").numel() * 8 / 2 ** 20, 2),
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        m = res["ms"]
        res["torch_route_over_gram_route"] = round(m["torch_route"] / m["gram_route"], 3)
        res["torch_reduction_over_gram_alone"] = round(m["torch_reduction_alone"] / m["gram_accumulate_alone"], 3)
        res["torch_dgemm_over_gram_alone"] = round(m["torch_dgemm_alone"] / m["gram_accumulate_alone"], 3)
        res["gram_alone_full_table_Tfma_per_s"] = round(B * n_sel * n_sel / (m["gram_accumulate_alone"] * 1e-3) / 1e12, 3)
        res["dgemm_alone_Tfma_per_s"] = round(B * n_sel * n_sel / (m["torch_dgemm_alone"] * 1e-3) / 1e12, 3)
        # one step through both routes, from zeroed tables: how far the tables are apart, and what each route adds to the device's peak
        peak = {}
        for name, fn in (("torch", lambda: torch_reduce(decode())), ("gram", lambda: gram_reduce(decode()))):
            state["block"] = state["gws"] = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            state[name] = fresh()
            fn()
            torch.cuda.synchronize()
            peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        res["peak_MiB_over_baseline"] = peak
        (sa, ca), (sb, cb) = state["torch"], state["gram"]
        res["max_relative_difference"] = {"S": float(((sa - sb).abs() / sb.abs().clamp_min(1e-300)).max()), "C": float(((ca - cb).abs() / cb.abs().clamp_min(1e-300)).max())}
        res["gram_is_symmetric_in_bits"] = bool(torch.equal(cb, cb.t()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--genes", nargs="+", type=int, default=[64, 512, 2048])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "torch", "gram"], default="all")
    a = ap.parse_args()
    for p in a.precision:
        for k in a.genes:
            print(json.dumps(run(p, k, a.steps, a.warmup, a.rounds, a.only)), flush=True)


if __name__ == "__main__":
    main()
