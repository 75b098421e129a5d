#!/usr/bin/env python3
"""Record every argument block the package hands to its C ABI during one eager training step or one round of read-outs.

    python tools/abi_trace.py ROW OUT.jsonl [--root DIR] [--record-only] [--env NAME=VALUE ...] [--eval]

``spvipes_amd._abi.call`` is replaced by a spy that writes one JSON line per call: the entry-point name and every argument.  A ctypes
structure is walked through its ``_fields_`` (nested structures, arrays and non-null structure pointers included) and given as
field name -> value.  Device addresses would differ from process to process, so every ``c_void_p`` field and every positional integer
>= 2^40 (device addresses and stream handles) is replaced by [k, offset]: k numbers the allocations (the caching allocator's live
block that holds the address; the bare value for what lies in none, such as a stream handle) in order of first appearance in the whole
trace, offset is the distance from the block's start.  Null stays null.  Two processes that fill equal blocks, aliasing and interior
offsets included, write equal traces; `diff` of the traces of two trees is the check that a change of the host code left every launch's
arguments alone.

ROW is one of ROWS below; each runs at B = 128 and then at B = 200 cells per group, G = (300, 280), H = 32, 10 shared / 5 private
dimensions, 512 cells.  ``--root DIR`` imports ``spvipes_amd`` from DIR (a checkout of another commit) instead of this tree.
``--record-only``: the spy returns without calling the library, so nothing of the project's is launched -- for the switch rows
(``--env SPV_TRUNK_FOLD=0`` ...), which reach fills no default step runs.  ``--eval`` traces the training rows in eval() mode, backward
pass included."""
import argparse
import bisect
import ctypes as C
import json
import os
import sys

ROWS = ("label_bf16", "label_fp32", "paired", "cluster", "three_groups", "narrow_nb3", "wide_nb12", "readouts",
        "readouts_fp32", "readouts_wide", "readouts_stats")
GS, H, N_S, N_P, CELLS = (300, 280), 32, 10, 5, 512


class Tracer:
    def __init__(self, out, record_only: bool):
        self.out, self.record_only, self.ids, self.blocks = out, record_only, {}, []

    def _live_blocks(self):
        import torch
        blocks = []
        for seg in torch.cuda.memory_snapshot():
            addr = seg["address"]
            for b in seg["blocks"]:
                a = b.get("address", addr)
                if b["state"] != "inactive":
                    blocks.append((a, b["size"]))
                addr = a + b["size"]
        blocks.sort()
        return blocks

    def pointer(self, v):
        if not v:
            return None
        v = int(v)
        i = bisect.bisect_right(self.blocks, (v, float("inf"))) - 1
        base = self.blocks[i][0] if i >= 0 and v < self.blocks[i][0] + self.blocks[i][1] else v
        return [self.ids.setdefault(base, len(self.ids)), v - base]

    def value(self, ctype, v):
        if ctype is C.c_void_p:
            return self.pointer(v)
        if isinstance(ctype, type) and issubclass(ctype, C.Structure):
            return self.struct(v)
        if isinstance(ctype, type) and issubclass(ctype, C.Array):
            return [self.value(ctype._type_, v[i]) for i in range(ctype._length_)]
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
            return self.value(ctype._type_, v.contents) if v else None
        return v

    def struct(self, s):
        return {name: self.value(ctype, getattr(s, name)) for name, ctype, *_ in s._fields_}

    def argument(self, a):
        a = getattr(a, "_obj", a)   # C.byref(x)
        if isinstance(a, (C.Structure, C.Array, C._Pointer)):
            return self.value(type(a), a)
        if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 40:
            return self.pointer(a)
        return a

    def install(self):
        from spvipes_amd import _abi
        real = _abi.call

        def spy(name, *args):
            self.blocks = self._live_blocks()
            self.out.write(json.dumps({"call": name, "args": [self.argument(a) for a in args]}) + "\n")
            if not self.record_only:
                real(name, *args)

        _abi.call = spy


def _noise(torch, B, groups, seed):
    gen = torch.Generator().manual_seed(seed)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen) for g in range(groups) for k, n in (("private", N_P), ("shared", N_S))}
    noise.update({f"poe_{g}": torch.randn(B, N_S, generator=gen) for g in range(groups)})
    return noise


def training_row(row: str, B: int, dev, evaluate: bool):
    """one eager forward + loss + backward of the row's module"""
    import numpy as np
    import torch
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    kw = dict(n_hidden=H, n_dimensions_shared=N_S, n_dimensions_private=N_P, dropout_rate=0.0, precision="fp32" if row == "label_fp32" else "bf16")
    NG = 3 if row == "three_groups" else 2
    Gs = GS + (260,) if NG == 3 else GS
    groups = [make_synthetic_group(g % 2, CELLS, Gs[g], dev) for g in range(NG)]
    counts, labels = [g.counts for g in groups], [g.labels for g in groups]
    dims = {g: Gs[g] for g in range(NG)}
    if row in ("label_bf16", "label_fp32"):
        trainer = Trainer(spVIPESmodule(dims, use_labels=True, **kw).to(dev), counts, labels=labels)
    elif row in ("narrow_nb3", "wide_nb12"):
        nb = 3 if row == "narrow_nb3" else 12
        codes = [torch.tensor(rng.integers(0, nb, size=CELLS), dtype=torch.int32, device=dev) for _ in range(2)]
        module = spVIPESmodule(dims, use_labels=True, n_batch=nb, decoder_slots="narrow" if nb == 3 else "auto", **kw).to(dev)
        trainer = Trainer(module, counts, labels=labels, batch_codes=codes)
    elif row == "three_groups":
        module = spVIPESmodule(dims, transport_plan="components", pair_data=False, allow_more_groups=True, n_components=10, **kw).to(dev)
        trainer = Trainer(module, counts, components=labels)
    else:
        import scipy.sparse as sp
        i, j, v = np.repeat(np.arange(CELLS), 3), rng.integers(0, CELLS, size=3 * CELLS), rng.random(3 * CELLS).astype(np.float32) + 0.1
        plan = sp.coo_matrix((v, (i, j)), shape=(CELLS, CELLS)).tocsr()
        module = spVIPESmodule(dims, use_labels=False, transport_plan=plan, pair_data=(row == "paired"), **kw).to(dev)
        trainer = Trainer(module, counts, components=labels if row == "cluster" else None)
    trainer.module.train(not evaluate)
    rows = [torch.tensor(rng.permutation(CELLS)[:B], dtype=torch.int32, device=dev) for _ in range(NG)]
    trainer._forward_backward(rows, torch.full((), 1.0, device=dev), noise={k: v.to(dev) for k, v in _noise(torch, B, NG, 1).items()})


def readout_row(row: str, B: int, dev):
    """the module's read-outs of one minibatch, in eval() and in train() mode: materialised ``generative`` outputs, expected_expression,
    sample_counts, sample_count_stats.  "readouts": bf16, narrow layout; "readouts_fp32": precision="fp32"; "readouts_wide": n_batch = 12,
    decoder_slots="auto", with batch codes; "readouts_stats": expression_stats over a two-segment tile plan (eval() only)"""
    import numpy as np
    import torch
    from spvipes_amd.data import expression_tile_plan, make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    groups = [make_synthetic_group(g, CELLS, GS[g], dev) for g in range(2)]
    wide = dict(n_batch=12, decoder_slots="auto") if row == "readouts_wide" else {}
    module = spVIPESmodule({0: GS[0], 1: GS[1]}, use_labels=True, n_hidden=H, n_dimensions_shared=N_S, n_dimensions_private=N_P, dropout_rate=0.0,
                           precision="fp32" if row == "readouts_fp32" else "bf16", **wide).to(dev)
    rows = [torch.tensor(rng.permutation(CELLS)[:B], dtype=torch.int32, device=dev) for _ in range(2)]
    batch = [torch.tensor(rng.integers(0, 12, size=B), dtype=torch.int32, device=dev) if wide else None for _ in range(2)]
    tensors = tuple({"counts": groups[g].counts, "rows": rows[g], "indices": rows[g].float().unsqueeze(1), "groups": None, "batch": batch[g],
                     "labels": groups[g].labels[rows[g].long()].unsqueeze(1)} for g in range(2))
    noise = {k: v.to(dev) for k, v in _noise(torch, B, 2, 1).items()}
    genes = np.arange(3, 200)
    if row == "readouts_stats":
        module.eval()
        with torch.no_grad():
            inf, _ = module(tensors, inference_kwargs={"noise": noise}, compute_loss=False)
            for g in range(2):
                perm, tile_seg, tile_n = (torch.as_tensor(a, device=dev) for a in expression_tile_plan(rng.integers(0, 2, size=B), 2))
                module.expression_stats(inf, g, genes=genes, perm=perm, tile_seg=tile_seg, tile_n=tile_n, n_seg=2,
                                        stats=torch.zeros(2, 8, len(genes), dtype=torch.float64, device=dev))
        return
    for training in (False, True):
        module.train(training)
        with torch.no_grad():
            inf, gen = module(tensors, inference_kwargs={"noise": noise}, compute_loss=False)
            for g in range(2):
                gen["private_poe"][str(g)]["px_rate_private"]   # (materialises the group's arrays)
                module.expected_expression(inf, g)
                module.expected_expression(inf, g, genes=genes, what="private", library_size=1e4)
                module.sample_counts(inf, g, genes=genes, key=7, sample=2)
                stats = torch.zeros(1, 4, len(genes), dtype=torch.int64, device=dev)
                module.sample_count_stats(inf, g, genes=genes, key=7, sample=2, stats=stats, cell_total=torch.zeros(B, dtype=torch.int64, device=dev))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("row", choices=ROWS)
    ap.add_argument("out")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--record-only", action="store_true")
    ap.add_argument("--env", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--batch", type=int, nargs="*", default=[128, 200])
    a = ap.parse_args()
    for kv in a.env:   # (the switches are read when the package is imported)
        name, _, val = kv.partition("=")
        os.environ[name] = val
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import spvipes_amd
    assert os.path.abspath(spvipes_amd.__file__).startswith(os.path.abspath(a.root) + os.sep), spvipes_amd.__file__
    dev = torch.device("cuda:0")
    with open(a.out, "w") as f:
        tracer = Tracer(f, a.record_only)
        tracer.install()
        for B in a.batch:
            readout_row(a.row, B, dev) if a.row.startswith("readouts") else training_row(a.row, B, dev, a.eval)
            torch.cuda.synchronize()
            f.write(json.dumps({"end_of": a.row, "B": B}) + "\n")
    print(f"{a.row}: trace of {a.root} written to {a.out}", flush=True)


if __name__ == "__main__":
    main()
