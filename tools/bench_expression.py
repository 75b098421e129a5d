#!/usr/bin/env python3
"""Cost of the denoised-expression read-out at C2's step shape (4096 cells x 10 000 genes, 25 / 10 latents, one group), bf16 and
fp32 modes, timed with device events after warm-up, in alternating rounds in one process:

    (a) materialize_decoder + the torch combine sigmoid(l) * rate_p + (1 - sigmoid(l)) * rate_s   -- the way to this array
        before spv_dec_expected existed (five fp32 [B, G] arrays, a tiled logits array, three torch passes)
    (b) expected_expression for all genes, for 1 000 genes and for 64 genes                      -- one fused kernel, one array

    python tools/bench_expression.py [--steps 20] [--warmup 5] [--rounds 3] [--precision bf16 fp32]
    python tools/bench_expression.py --only expected --precision bf16      # one path alone, e.g. under rocprofv3 --kernel-trace --stats

Both paths run the same operand preparation (latent slicing, BatchNorm fold, mixing trunk, operand images, softmax statistics over
all genes); the times include it.  Prints one JSON line per precision mode."""
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
    lib = (7.0 + 0.3 * torch.randn(B, generator=gen)).to(dev)
    dec, px_r, ws, ns = module.decoders[0], module.px_r[0], module._workspace(0, dev), module.nsplit
    rng = np.random.default_rng(0)
    sel = {n: torch.tensor(rng.permutation(G)[:n], dtype=torch.int32, device=dev) for n in (1000, 64)}
    out = {n: torch.empty(B, n, device=dev) for n in (G, 1000, 64)}

    def parent():
        m = dec_ops.materialize_decoder(dec, px_r, z_p, z_s, lib, False, ns, ws)
        s = torch.sigmoid(m["px_mixing"])
        return s * m["px_rate_private"] + (1 - s) * m["px_rate_shared"]

    def fused(n):
        return lambda: dec_ops.expected_expression(dec, px_r, z_p, z_s, lib, False, ns, ws, genes=(None if n == G else sel[n]), out=out[n])

    paths = {}
    if only in ("all", "parent"):
        paths["materialize_plus_combine"] = parent
    if only in ("all", "expected"):
        paths.update({f"expected_{n}_genes": fused(n) for n in (G, 1000, 64)})
    ms = {k: [] for k in paths}
    for _ in range(rounds):   # alternating rounds: the paths see the same clocks and neighbours
        for k, fn in paths.items():
            ms[k].append(_timed(fn, steps, warmup))
    res = {"precision": precision, "B": B, "G": G, "steps": steps, "warmup": warmup, "rounds": rounds,
           "ms": {k: round(float(np.median(v)), 4) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if only == "all":
        res["speedup_all_genes"] = round(res["ms"]["materialize_plus_combine"] / res["ms"][f"expected_{G}_genes"], 3)
        d = (parent() - fused(G)()).abs().max()
        res["max_abs_difference_of_the_two_paths"] = float(d)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "parent", "expected"], default="all")
    a = ap.parse_args()
    for p in a.precision:
        print(json.dumps(run(p, a.steps, a.warmup, a.rounds, a.only)), flush=True)


if __name__ == "__main__":
    main()
