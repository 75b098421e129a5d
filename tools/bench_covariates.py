#!/usr/bin/env python3
"""Cost of the decoder's wide operand layout: trainer steps at C2's shape (2 groups x 4096 cells per step, 10 000 genes, 25 / 10 latents,
bf16, hipGraph replay) with n_batch 3 (narrow layout) and n_batch 12 (wide layout), timed with device events after warm-up.

    python tools/bench_covariates.py [--nb 3 12] [--steps 20] [--warmup 5]

Prints one JSON line per n_batch.  Kernel times: run one n_batch at a time under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def run(nb: int, steps: int, warmup: int, B: int = 4096, G: int = 10000, cells: int = 16384) -> dict:
    from spvipes_amd.data import MinibatchSampler, make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    groups = [make_synthetic_group(g, cells, G, dev) for g in range(2)]
    codes = [torch.tensor(rng.integers(0, nb, size=cells), dtype=torch.int32, device=dev) for _ in range(2)]
    module = spVIPESmodule({0: G, 1: G}, use_labels=True, n_batch=nb, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10,
                           dropout_rate=0.1, precision="bf16", decoder_slots="auto").to(dev)
    module.train()
    trainer = Trainer(module, [g.counts for g in groups], labels=[g.labels for g in groups], batch_codes=codes, lr=1e-3)
    sampler = MinibatchSampler([cells, cells], B, dev, seed=1)
    batches = []
    while len(batches) < steps + warmup:
        batches += list(sampler.epoch())
    trainer.capture(batches[0], warmup=1)
    for r in batches[:warmup]:
        trainer.step(r, kl_weight=1.0)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i, r in enumerate(batches[warmup:warmup + steps]):
        trainer.step(r, kl_weight=1.0)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return {"n_batch": nb, "layout": "wide" if module.dec_slots.kslots else "narrow", "ms_per_step": sum(ms) / steps,
            "ms_per_step_median": float(np.median(ms)), "steps": steps, "warmup": warmup, "B": B, "G": G}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[3, 12])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for nb in a.nb:
        print(json.dumps(run(nb, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
