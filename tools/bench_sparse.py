#!/usr/bin/env python3
"""Cost of CSR-resident counts (ops.SparseGroupCounts: the minibatch densified per step by spv_csr_gather) against the dense-resident
path: trainer steps at C2's shape (2 groups x 4096 cells per step, 10 000 genes, 25 / 10 latents, bf16, hipGraph replay), timed with
device events after warm-up, on the same synthetic data (make_synthetic_group; the sparse storage is built from it on the device with
SparseGroupCounts.from_dense).  Storages alternate over --rounds.

    python tools/bench_sparse.py [--storage dense sparse] [--steps 20] [--warmup 5] [--rounds 2]

Prints one JSON line per storage and round: ms per step, the measured density and the HBM the counts hold (dense: matrix + f16
log1p image; sparse: CSR arrays; the [B][ld] minibatch buffers of the sparse path are reported apart).  Kernel time of the gather:
run one storage under rocprofv3 --kernel-trace --stats (``--storage sparse --rounds 1``)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def _setup(B: int, G: int, cells: int):
    from spvipes_amd.data import make_synthetic_group
    dev = torch.device("cuda:0")
    return dev, [make_synthetic_group(g, cells, G, dev) for g in range(2)]


def run(storage: str, dev, groups, steps: int, warmup: int, B: int, G: int, cells: int) -> dict:
    from spvipes_amd._abi import round_up
    from spvipes_amd.data import MinibatchSampler
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.ops import SparseGroupCounts
    from spvipes_amd.train import Trainer
    if storage == "sparse":
        counts = [SparseGroupCounts.from_dense(g.counts) for g in groups]
        nnz = sum(c.nnz for c in counts)
        held = sum(c.nbytes for c in counts)
        minibatch = 2 * B * (round_up(G, 8) * 2 + round_up(round_up(G, 96), 128) * 2 + 4)
    else:
        counts = [g.counts for g in groups]
        nnz = sum(int((c.X != 0).sum()) for c in counts)
        held = sum(c.X.numel() * 2 + sum(t.numel() * t.element_size() for t in c.log1p_image()) for c in counts)
        minibatch = 0
    torch.manual_seed(0)
    module = spVIPESmodule({0: G, 1: G}, use_labels=True, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10,
                           dropout_rate=0.1, precision="bf16").to(dev)
    module.train()
    trainer = Trainer(module, counts, labels=[g.labels for g in groups], lr=1e-3)
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
    return {"storage": storage, "ms_per_step": sum(ms) / steps, "ms_per_step_median": float(np.median(ms)), "density": nnz / (2 * cells * G),
            "counts_hbm_bytes": held, "minibatch_buffer_bytes": minibatch, "steps": steps, "warmup": warmup, "B": B, "G": G, "cells": cells,
            "loss_last": float(trainer._static_lo.loss) if trainer.graph is not None else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--storage", nargs="+", default=["dense", "sparse"], choices=["dense", "sparse"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cells", type=int, default=16384)
    a = ap.parse_args()
    B, G = 4096, 10000
    dev, groups = _setup(B, G, a.cells)
    for rnd in range(a.rounds):
        for s in a.storage:
            out = run(s, dev, groups, a.steps, a.warmup, B, G, a.cells)
            out["round"] = rnd
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
