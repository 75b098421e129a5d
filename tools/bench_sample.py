#!/usr/bin/env python3
"""Cost of one posterior-predictive count draw at C2's step shape (4096 cells x 10 000 genes, 25 / 10 latents, one group), bf16 and fp32
modes, timed with device events after warm-up, in alternating rounds in one process:

    (a) the torch route on the same decoder state: three expected_expression calls ("private", "shared", "mixing": three fp32 [B, G]
        arrays), then torch.bernoulli, torch._standard_gamma and torch.poisson with the element-wise passes between them
    (b) sample_counts: decode and draw in one fused kernel (spv_dec_sample), one int32 [B, G] array
    (c) expected_expression("mixture") alone: the operand preparation plus one decode-and-store pass, for scale

    python tools/bench_sample.py [--steps 20] [--warmup 5] [--rounds 3] [--precision bf16 fp32]
    python tools/bench_sample.py --only fused --precision bf16      # one path alone, e.g. under rocprofv3 --kernel-trace --stats

All paths run the same operand preparation (latent slicing, BatchNorm fold, mixing trunk, operand images, softmax statistics over all
genes); the times include it.  Prints one JSON line per precision mode, with the means of both routes' counts as a sanity figure."""
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


def run(precision: str, steps: int, warmup: int, rounds: int, only: str, B: int = 4096, G: int = 10000) -> dict:
    from spvipes_amd import dec_ops
    from spvipes_amd.module import spVIPESmodule
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    module = spVIPESmodule({0: G, 1: G}, use_labels=True, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10, precision=precision).to(dev)
    module.eval()
    gen = torch.Generator().manual_seed(1)
    z_p, z_s = torch.randn(B, 10, generator=gen).to(dev), torch.randn(B, 25, generator=gen).to(dev)
    lib = (9.0 + 0.3 * torch.randn(B, generator=gen)).to(dev)   # ~8 000 counts per cell, 0.85 per element: most draws run the inversion, the Gamma's tail reaches PTRS
    with torch.no_grad():
        module.px_r[0].copy_(torch.linspace(-2.0, 3.0, G)[torch.randperm(G, generator=gen)].to(dev))
    dec, px_r, ws, ns = module.decoders[0], module.px_r[0], module._workspace(0, dev), module.nsplit
    theta = torch.exp(px_r.detach().float())
    counts = torch.empty(B, G, dtype=torch.int32, device=dev)
    arrays = [torch.empty(B, G, device=dev) for _ in range(4)]
    step = [0]

    def torch_route():
        part_p, part_s, pi = (dec_ops.expected_expression(dec, px_r, z_p, z_s, lib, False, ns, ws, what=w, out=arrays[i])
                              for i, w in enumerate(("private", "shared", "mixing")))
        c = torch.bernoulli(pi)
        mu = torch.where(c > 0, part_p / pi, part_s / (1 - pi))
        lam = (torch._standard_gamma(theta.expand(B, G)) * (mu / theta)).clamp_(max=1e8)
        return torch.poisson(lam).to(torch.int32)

    def fused():
        step[0] += 1
        return dec_ops.sample_counts(dec, px_r, z_p, z_s, lib, False, ns, ws, key=1, sample=step[0], out=counts)

    def expected():
        return dec_ops.expected_expression(dec, px_r, z_p, z_s, lib, False, ns, ws, out=arrays[3])

    paths = {}
    if only in ("all", "torch"):
        paths["torch_route"] = torch_route
    if only in ("all", "fused"):
        paths["fused_sample_counts"] = fused
    if only == "all":
        paths["expected_mixture_for_scale"] = expected
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    res = {"precision": precision, "B": B, "G": G, "steps": steps, "warmup": warmup, "rounds": rounds,
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        res["torch_over_fused"] = round(res["ms"]["torch_route"] / res["ms"]["fused_sample_counts"], 3)
        res["mean_count"] = {"torch_route": float(torch_route().double().mean()), "fused": float(fused().double().mean()),
                             "model": float(expected().double().mean())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "torch", "fused"], default="all")
    a = ap.parse_args()
    for p in a.precision:
        print(json.dumps(run(p, a.steps, a.warmup, a.rounds, a.only)), flush=True)


if __name__ == "__main__":
    main()
