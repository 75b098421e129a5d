"""GPU: the likelihood kernel's chunk pipeline (csrc/spv_decoder.h: dec_nb_body -- a peeled first chunk, a two-chunk ping / pong loop,
a single-chunk tail) through spv_dec_nb_fwd, under partitions the planner never picks.

What an element of dL / tP / tS is does not depend on where its gene falls in the pipeline (first chunk, loop, tail) nor on which cell
tile of a workgroup its cell is in, so the three gradient arrays (both planes in split mode) are compared BIT FOR BIT across
    nb_genes_per_split in {32, 96, 160}  x  nb_cell_tiles in {1, 3},
and dtheta_part (whose rows are per workgroup) bit for bit between the runs with equal nb_cell_tiles.
Shapes: B = 80 (padded to 128: with 3 cell tiles per workgroup the only workgroup is a trailing partial one, and 48 cells are padding);
G = 203 (the kernel walks 208 = 13 chunks: the last non-empty split has 1 chunk at 32 and at 96, 3 at 160 -- the peeled chunk alone, odd
and even counts, the tail, the g + 4 > G column path -- and at 32 the eighth split is padding only); G = 10 (one chunk in all).  The
inputs are tests/_nb_reference.edge_case: counts >= 64 and, in fp32 storage, non-integral ones (the off-table fix-up branch).
Modes: u16 at an aligned column offset, u16 at an odd one, fp32 counts  x  {bf16 words + f16 logits, split words + fp32 logits}.

The partial sums: per cell, the totals of rec_part over the splits against the float64 reference under the bounds of
tests/test_gpu_nb_edges.py (fp32 mode: _nb_reference.nb_bounds "rec", full edge case; bf16 mode: the rounding-aware reference under
_bf16_reference.BOUNDS_DECODER "rec", mild edge case), for every partition, and once in eval form (TRAIN = false).  nb_bounds does not
hand out the per-element bounds of tP / tS, so the totals of tp_part / ts_part are held to the kernel's own stored arrays, which the
edges test holds to float64 through every gradient they produce: a total is the fp32 sum, in the kernel's order, of the values whose
roundings the array stores, so |total - sum_g stored| <= (r + (G / 4 + 8 + S) U) sum_g |stored| with r the storage rounding (2^-8 for a
bf16 word, 2^-17 for a hi + lo pair: 2^-18 each), G / 4 + 8 the lane's additions and shuffles, S the splits added on the host, U = 2^-24."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _bf16_reference as BR
from tests import _hip_harness as H
from tests import _nb_reference as R
from tests.test_gpu_nb_edges import NAMES, VARIANTS, _bf16_rounding_reference, _counts

pytestmark = pytest.mark.gpu

B = 80
PARTITIONS = [(per, nct) for per in (32, 96, 160) for nct in (1, 3)]
U = 2.0 ** -24
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _case(G, storage, variant):
    """inputs and float64 reference, once per (G, count values, variant); G = 10 is the first ten genes of the G = 203 case (edge_case
    plants counts at genes 16..35)"""
    key = (G, "f32" if storage == "f32" else "u16", variant)
    if key not in _CASES:
        X, t, lib, w, regime = R.edge_case(B, 203, key[1], **VARIANTS[variant])
        if G != 203:
            X = np.ascontiguousarray(X[:, :G])
            t = {k: (v[:G].clone() if k in ("Wp", "cp", "Ws", "cs", "Wm", "bm", "px_r") else v) for k, v in t.items()}
            lib = torch.log(torch.log1p(torch.tensor(X)).sum(1))
        assert (X >= 64).any() and (key[1] != "f32" or (X != np.floor(X)).any())
        ref = R.nb_reference(X, t, lib, w)
        _CASES[key] = dict(X=X, t=t, lib=lib, w=w, ref=ref)
    return _CASES[key]


def _untile(words, Bp, Gp):
    """[Bp][Gp] float64 values of a gradient array in accumulator-tile order (int16 bf16 words [planes * Bp][Gp]; split mode: hi + lo)"""
    def plane(a):
        v = (a.astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        v = v.reshape(Bp // 32, Gp // 32, 2, 2, 2, 32, 4)   # cell tile, gene tile, chunk of the tile, gq >> 1, gq & 1, cell row, j
        return v.transpose(0, 5, 1, 2, 3, 4, 6).reshape(Bp, Gp)
    flat = words.reshape(-1, Bp * Gp)
    return sum(plane(flat[i]) for i in range(flat.shape[0]))


def _runs(dev, G, storage, nsplit, variant):
    """every partition's outputs (train form) and one eval-form rec, on one set of operands prepared by the harness"""
    from spvipes_amd import _abi, ops
    from spvipes_amd._abi import SpvDecParams, ptr, stream_ptr
    c = _case(G, storage, variant)
    counts = _counts(dev, c["X"], G, storage)
    dparams = [c["t"][k].clone().to(dev).requires_grad_(True) for k in NAMES]
    ws = ops.Workspace(dev)
    loss, _ = H.DecoderNBLoss.apply(counts, None, B, *dparams, c["lib"].to(dev), c["w"].to(dev), nsplit, True, ws)
    P0 = loss.grad_fn.P   # the harness's parameter block: operands, tables, lse -- everything but the partition and the outputs
    Bp, Gp, planes = P0.Bp, P0.Gp, (2 if nsplit == 3 else 1)
    assert (Bp, Gp) == (128, 256)
    out, keep = {}, []
    for per, nct in PARTITIONS:
        nbs = -(-Gp // per)
        z = lambda *s, dt=torch.float32: torch.full(s, float("nan") if dt == torch.float32 else 0, dtype=dt, device=dev)
        bufs = dict(rec_part=z(nbs, Bp), tp_part=z(nbs, Bp), ts_part=z(nbs, Bp), dtheta_part=torch.zeros(Bp // 64, Gp, device=dev),
                    dL=z(planes * Bp, Gp, dt=torch.int16), tP=z(planes * Bp, Gp, dt=torch.int16), tS=z(planes * Bp, Gp, dt=torch.int16))
        P = SpvDecParams.from_buffer_copy(P0)
        P.nb_splits, P.nb_genes_per_split, P.nb_cell_tiles = nbs, per, nct
        for k, v in bufs.items():
            setattr(P, k, ptr(v))
        _abi.call("spv_dec_nb_fwd", C.byref(P), 1, stream_ptr())
        keep.append(bufs)
        if (per, nct) == (96, 3):   # eval form: rec only, the gradient buffers must stay as the train launch left them
            rec_eval = torch.full((nbs, Bp), float("nan"), device=dev)
            before = {k: bufs[k].clone() for k in ("dL", "tP", "tS", "dtheta_part")}
            P.rec_part = ptr(rec_eval)
            _abi.call("spv_dec_nb_fwd", C.byref(P), 0, stream_ptr())
            torch.cuda.synchronize()
            assert all(torch.equal(before[k], bufs[k]) for k in before), "the eval launch wrote a training output"
            out["eval_rec"] = rec_eval.cpu().double().sum(0)
        torch.cuda.synchronize()
        out[(per, nct)] = {k: v.cpu().numpy() for k, v in bufs.items()}
    return out, (Bp, Gp, planes)


MODES = [(storage, nsplit) for storage in ("u16", "u16_odd", "f32") for nsplit in (1, 3)]


@pytest.mark.parametrize("G", [203, 10])
@pytest.mark.parametrize("storage,nsplit", MODES)
def test_partitions_agree_bit_for_bit_and_totals_hold(dev, G, storage, nsplit):
    variant = "full" if nsplit == 3 else "mild"
    c = _case(G, storage, variant)
    out, (Bp, Gp, planes) = _runs(dev, G, storage, nsplit, variant)
    first = out[PARTITIONS[0]]
    fails = []
    for part in PARTITIONS[1:]:
        for k in ("dL", "tP", "tS"):
            if not np.array_equal(first[k], out[part][k]):
                fails.append(f"{k} differs between partitions {PARTITIONS[0]} and {part}: {int((first[k] != out[part][k]).sum())} words")
    for nct in (1, 3):   # rows of dtheta_part are per workgroup: comparable between equal cell tilings only
        ref_d = out[(32, nct)]["dtheta_part"]
        for per in (96, 160):
            if not np.array_equal(ref_d.view(np.uint32), out[(per, nct)]["dtheta_part"].view(np.uint32)):
                fails.append(f"dtheta_part differs between partitions (32, {nct}) and ({per}, {nct})")
    # ---- the arrays are not trivially equal: written where they must be, zero where nothing is to be written ----
    tP, tS, dL = (_untile(first[k], Bp, Gp) for k in ("tP", "tS", "dL"))
    if not (np.abs(dL[:B, :G]).max() > 0 and np.abs(tP[:B, :G]).max() > 0 and np.isfinite(dL).all() and np.isfinite(tP).all() and np.isfinite(tS).all()):
        fails.append("gradient arrays empty or not finite")
    if np.abs(dL[B:]).max() != 0 or np.abs(dL[:, G:]).max() != 0 or np.abs(tP[B:]).max() != 0 or np.abs(tP[:, G:]).max() != 0:
        fails.append("gradient words of padding cells / genes are not zero")
    # ---- per-cell totals of the partial sums ----
    if nsplit == 3:
        bound = R.nb_bounds(c["X"], c["t"], c["w"], c["ref"], integral=storage != "f32")["rec"]
        want_rec = c["ref"]["rec"]
    else:
        key = ("bf16ref", G, storage == "f32")
        if key not in _CASES:
            _CASES[key] = _bf16_rounding_reference(c["X"], c["t"], c["lib"], c["w"])
        want_rec = _CASES[key][1]
    recs = {part: torch.tensor(out[part]["rec_part"]).double().sum(0) for part in PARTITIONS}
    recs["eval"] = out["eval_rec"]
    for part, rec in recs.items():
        if not (rec[B:] == 0).all():
            fails.append(f"rec of padding cells not zero at {part}")
        if nsplit == 3:
            ratio = ((rec[:B] - want_rec).abs() / bound).max()
            print(f"G={G} {storage} fp32 mode {part}: rec err/bound {float(ratio):.3f}")
            if not float(ratio) <= 1.0:
                fails.append(f"rec at {part}: err/bound {float(ratio):.3f}")
        else:
            fails += [f"{part}: {f}" for f in BR.check(f"rec {part}", rec[:B], want_rec, BR.BOUNDS_DECODER["rec"], {})]
    store = 2.0 ** -17 if nsplit == 3 else 2.0 ** -8
    for part in PARTITIONS:
        nbs = out[part]["rec_part"].shape[0]
        for name, arr in (("tp_part", tP), ("ts_part", tS)):
            tot = out[part][name].astype(np.float64).sum(0)
            err = np.abs(tot - arr.sum(1))
            lim = (store + (G / 4 + 8 + nbs) * U) * np.abs(arr).sum(1) + Gp * R.FLT_MIN   # (a word or a lo plane below the smallest normal is flushed)
            print(f"G={G} {storage} nsplit={nsplit} {part} {name}: largest err/bound {float((err / lim).max()):.3f}")
            if not (err <= lim).all():
                fails.append(f"{name} totals at {part}: err/bound {float((err / lim).max()):.3f}")
    assert not fails, fails
