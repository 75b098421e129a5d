"""GPU: the shipped decoder op (dec_ops.DecoderFused) alone, in bf16 mode, against a float64 reference of the SAME operation -- one
that rounds to bf16 / f16 at exactly the places the kernels do (tests/_bf16_reference.py).  Only fp32 accumulation order and rare
one-ulp rounding flips separate the two, so the bounds sit one to two orders below the bf16-vs-unrounded bounds of
test_gpu_fullsize_parity.py (3e-2 relative L2 / 8e-2 max) and would catch a dropped cell, a dropped gene tile or a missed rounding.

Inputs: decoders and px_r of an spVIPESmodule (BatchNorm affine parameters moved off 1 / 0), random latent leaves, resident uint16
counts gathered by row index, w = 1 / B, no KL vectors.  Checked: the loss, both per-cell reconstruction vectors, d private_log_z,
d poe_log_z, all 13 parameter gradients per group and the BatchNorm running buffers after the forward pass (eval mode: unchanged).

Bounds (tests/_bf16_reference.py: BOUNDS_DECODER) against the worst value measured on the MI355X over all cases, both DEC_PAIR modes
(metrics: max = tensor-wide max error / max |ref|, row = worst gene / cell row or vector element, l2 = tensor-wide relative L2):
  quantity                                   bound max / row / l2        measured max / row / l2
  loss                                       8e-7                        2.0e-7
  rec (per cell)                             7e-6 / 7.9e-6 / 8e-7        1.8e-6 / 2.0e-6 / 2.2e-7
  d private / poe latents                    1e-3 / 3e-3 / 2.5e-4        2.7e-4 / 1.0e-3 / 6.5e-5
  d W_a, b_a, gamma_a, beta_a, px_r          5e-4 / 9.6e-4 / 2.4e-4      1.3e-4 / 2.4e-4 / 6.1e-5
  d W_p, gamma_p, beta_p, W_s, .., W_m, b_m  1.9e-3 / 8e-3 / 2.8e-4      4.9e-4 / 2.1e-3 / 7.0e-5
  BatchNorm running buffers                  3.6e-7 / 4.8e-7 / 1.7e-7    9.2e-8 / 1.2e-7 / 4.3e-8
The regressor and mixture gradients get their own row bound: their gene rows are contractions over the cells of bf16-rounded
operands and carry one-ulp rounding flips (tests/_bf16_reference.py, "weight").
Routes (asserted per case): every narrow case runs spv_dec_heads_bwd (fused_heads) with heads_dma set; the wide case runs the
in-place softmax fix and the split-K GEMMs.  With DEC_PAIR = "1" the two groups' launches are single pair grids (the *_grouped entry
points, recorded per call); with "0" none is launched.  (Every bf16 shape pads genes to 256, so the 320-column GEMMs and the logits
GEMM take their LDS-DMA kernels at all of these shapes: the cases differ in shape, not in that choice.)
Gradients that are zero by construction (the trunk bias in front of its training-mode BatchNorm) are held to the same bound
relative to the largest parameter gradient of the group.
"""
import numpy as np
import pytest
import torch

from tests import _bf16_reference as R

pytestmark = pytest.mark.gpu

KMP = 320
WEIGHT_KIND = ("Wp", "gamma_p", "beta_p", "Ws", "gamma_s", "beta_s", "Wm", "bm")   # gradients held to BOUNDS_DECODER["weight"]

# id, B, genes per group, n_shared, n_private, extra
CASES = [
    ("ragged-tiny", 37, (45, 51), 6, 3, {}),
    ("tile-edges", 129, (257, 1030), 25, 10, {}),
    ("widest-narrow", 300, (2001, 777), 31, 15, {}),
    ("large", 1030, (3001, 2050), 25, 10, {}),
    ("wide-12-categories", 200, (700, 333), 25, 10, {"n_batch": 12}),
    ("eval", 129, (257, 1030), 25, 10, {"eval": True}),
    ("single-group", 300, (2001,), 31, 15, {}),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _move_trunk_kinks_away(zt, Wa, ba, gamma, beta, training, rm, rv, margin=1e-4):
    """shift each trunk unit's BatchNorm bias so that no cell's rectifier input lies within ``margin`` of zero (evaluated in float64):
    a flipped mask would move a whole gradient row and say nothing about the kernels"""
    pre = zt @ Wa.t() + ba
    mean, var = (pre.mean(0), pre.var(0, unbiased=False)) if training else (rm, rv)
    y = (pre - mean) / torch.sqrt(var + R.BN_EPS) * gamma + beta
    cand = torch.arange(0, 400, dtype=torch.float64) * (2.5 * margin)
    ok = ((y.unsqueeze(0) + cand.view(-1, 1, 1)).abs() > margin).all(dim=1)
    assert bool(ok.any(dim=0).all())
    return beta + cand[ok.double().argmax(dim=0)]


def _run_case(dev, case, monkeypatch, pair):
    from spvipes_amd import _abi, dec_ops, ops
    from spvipes_amd.module import CovariateColumns, spVIPESmodule
    name, B, Gs, n_s, n_p, extra = case
    NG = len(Gs)
    training = not extra.get("eval", False)
    nb = extra.get("n_batch", 0)
    monkeypatch.setattr(ops, "DEC_PAIR", pair)
    seen = []
    init = dec_ops._DecoderBwd.__init__

    def record(self, *a, **k):
        init(self, *a, **k)
        seen.append(self)
    monkeypatch.setattr(dec_ops._DecoderBwd, "__init__", record)
    launched = set()
    call = _abi.call

    def call_rec(name, *a):
        launched.add(name)
        return call(name, *a)
    monkeypatch.setattr(_abi, "call", call_rec)

    rng = np.random.default_rng(B * 31 + sum(Gs))
    gen = torch.Generator().manual_seed(B + sum(Gs))
    torch.manual_seed(B)
    G2 = (Gs[0], Gs[-1])
    module = spVIPESmodule({0: G2[0], 1: G2[1]}, use_labels=True, n_hidden=32, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           precision="bf16", n_batch=nb, decoder_slots="wide" if nb else "narrow").to(dev)
    module.train(training)
    n_cells = B + 13
    lat, pars, xs, libs, counts, rows, decs = [], [], [], [], [], [], []
    for g in range(NG):
        G = Gs[g]
        X = (rng.poisson(3.0, size=(n_cells, G)) * (rng.random((n_cells, G)) < 0.35)).astype(np.float32)
        X[:, 0] += 1
        X[rng.integers(0, n_cells, 6), rng.integers(0, G, 6)] += 90.0   # a few counts beyond the lgamma table
        r = rng.permutation(n_cells)[:B].astype(np.int32)
        counts.append(ops.GroupCounts(torch.tensor(X.astype(np.uint16).view(np.int16)).to(dev), G, 0, resident=True))
        rows.append(torch.tensor(r, device=dev))
        x32 = torch.log1p(torch.tensor(X[r]))
        xs.append(x32.double())
        libs.append(torch.log(x32.sum(1)).unsqueeze(1))
        dec = module.decoders[g]
        decs.append(dec)
        with torch.no_grad():
            for bn in (dec.factor_regressor_private.bn, dec.factor_regressor_shared.bn, dec.sigmoid_decoder.bn):
                bn.weight.copy_(torch.empty_like(bn.weight).uniform_(0.5, 1.5))
                bn.bias.copy_(torch.randn(bn.bias.shape, device=dev) * 0.1)
                bn.running_mean.copy_(torch.randn(bn.running_mean.shape, device=dev) * 0.2)
                bn.running_var.copy_(torch.empty_like(bn.running_var).uniform_(0.5, 2.0))
        par = [t.detach().clone() for t in dec_ops.decoder_params(dec, module.px_r[g])]
        priv, poe = torch.randn(B, n_p, generator=gen), torch.randn(B, n_s, generator=gen)
        if nb:   # covariates: as spVIPESmodule._decoder_operands hands them to the op
            oh = torch.nn.functional.one_hot(torch.tensor(rng.integers(0, nb, B)), nb).float()
            Z = torch.cat([priv, poe], 1)
            Zx = torch.cat([Z[:, :n_s], oh, Z[:, n_s:], oh], 1)
            priv, poe = Zx[:, :n_p + nb].contiguous(), Zx[:, n_p + nb:].contiguous()
            n_m = par[6].shape[0]
            par[6] = CovariateColumns.apply(par[6], n_p, n_p + n_s).detach()
            par[10] = CovariateColumns.apply(par[10], n_m + n_p, n_m + n_p + n_s).detach()
        # keep every trunk rectifier input away from zero
        p64 = [t.cpu().double() for t in par]
        zp, zs = R.O.split_latents(priv.double(), poe.double(), poe.shape[1], priv.shape[1])
        bn = dec.sigmoid_decoder.bn
        p64[9] = _move_trunk_kinks_away(torch.cat([zp, zs], 1), p64[6], p64[7], p64[8], p64[9], training,
                                        bn.running_mean.cpu().double(), bn.running_var.cpu().double())
        par[9] = p64[9].float().to(dev)
        lat.append((priv, poe))
        pars.append(par)
    buffers = [{k: (m.bn.running_mean.detach().cpu().double().clone(), m.bn.running_var.detach().cpu().double().clone())
                for k, m in (("p", d.factor_regressor_private), ("s", d.factor_regressor_shared), ("a", d.sigmoid_decoder))} for d in decs]
    # ---- the op ------------------------------------------------------------------------------------------------------------------
    Bp = -(-B // 128) * 128
    w_pad = torch.zeros(Bp, device=dev)
    w_pad[:B] = 1.0 / B
    leaves = []
    for g in range(NG):
        leaves += [lat[g][0].to(dev).requires_grad_(training), lat[g][1].to(dev).requires_grad_(training)]
    pleaves = [t.clone().requires_grad_(training) for g in range(NG) for t in pars[g]]
    klw = torch.zeros((), device=dev)
    ws = [ops.Workspace(dev) for _ in range(NG)]
    with torch.set_grad_enabled(training):
        res = dec_ops.DecoderFused.apply(counts, rows, B, decs, [l.to(dev) for l in libs], w_pad, training, module.nsplit, ws, klw, 0,
                                         *leaves, *pleaves)
    torch.cuda.synchronize()
    bufs_after = [{k: (m.bn.running_mean.detach().cpu().double(), m.bn.running_var.detach().cpu().double())
                   for k, m in (("p", d.factor_regressor_private), ("s", d.factor_regressor_shared), ("a", d.sigmoid_decoder))} for d in decs]
    if training:
        res[0].backward()
        torch.cuda.synchronize()
    # ---- the reference -------------------------------------------------------------------------------------------------------------
    rl = [tuple(t.detach().cpu().double().requires_grad_(training) for t in pair_) for pair_ in lat]
    rp = [[t.detach().cpu().double().requires_grad_(training) for t in par] for par in pars]
    loss_r, rec_r, stats_r = R.decoder_fused(rl, rp, xs, [l.double() for l in libs], torch.full((B,), 1.0 / B, dtype=torch.float64),
                                            training=training, buffers=buffers)
    if training:
        loss_r.backward()
    # ---- compare -------------------------------------------------------------------------------------------------------------------
    bd, bad, rep = R.BOUNDS_DECODER, [], {}
    bad += R.check("loss", res[0].detach().cpu(), loss_r.detach(), bd["loss"], rep)
    for g in range(NG):
        bad += R.check(f"rec{g}", res[2 + g].cpu().reshape(-1, 1), rec_r[g].reshape(-1, 1), bd["rec"], rep)
        for k in ("p", "s", "a"):
            for j, nm in enumerate(("running_mean", "running_var")):
                if training:
                    bad += R.check(f"bn{g}.{k}.{nm}", bufs_after[g][k][j], stats_r[g][f"{k}.{nm}"], bd["buffer"], rep)
                elif not torch.equal(bufs_after[g][k][j], buffers[g][k][j]):
                    bad.append(f"eval mode moved bn{g}.{k}.{nm}")
        if not training:
            continue
        for j, nm in enumerate(("d_private_log_z", "d_poe_log_z")):
            bad += R.check(f"{nm}{g}", leaves[2 * g + j].grad.cpu(), rl[g][j].grad, bd["latent"], rep)
        gmax = max(float(t.grad.abs().max()) for t in rp[g])
        for j, nm in enumerate(("Wp", "gamma_p", "beta_p", "Ws", "gamma_s", "beta_s", "Wa", "ba", "gamma_a", "beta_a", "Wm", "bm", "px_r")):
            ref = rp[g][j].grad
            got = pleaves[g * 13 + j].grad.cpu()
            if float(ref.abs().max()) < 1e-9 * gmax:   # zero by construction: hold it to the bound relative to the group's gradients
                got, ref = got / gmax, ref * 0.0
                e = float(got.abs().max())
                rep[f"d{nm}{g}"] = {"max": e, "row": e, "l2": e}
                if not e <= bd["param"]["max"]:
                    bad.append(f"d{nm}{g}: {e:.3e} of the largest gradient (zero by construction)")
                continue
            bad += R.check(f"d{nm}{g}", got, ref, bd["weight" if nm in WEIGHT_KIND else "param"], rep)
    # ---- routes --------------------------------------------------------------------------------------------------------------------
    routes = []
    for st in seen:
        routes.append(dict(fused_heads=st.fused_heads, heads_dma=st.heads_dma, wide=bool(st.sl.kslots)))
    grouped = sorted(n for n in launched if n.endswith("_grouped") and n.startswith(("spv_dec_", "spv_gemm_bf16")))
    worst = {k: max(v["max"], v["row"]) for k, v in rep.items()}
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f"\n[bf16-decoder] {name} pair={pair} routes={routes} grouped={grouped} worst: " + ", ".join(f"{k} {v:.2e}" for k, v in top))
    return bad, routes, grouped, training, nb


@pytest.mark.parametrize("pair", ["0", "1"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_decoder_bf16_matches_rounding_reference(dev, case, pair, monkeypatch):
    bad, routes, grouped, training, nb = _run_case(dev, case, monkeypatch, pair)
    assert not bad, f"{case[0]} (DEC_PAIR={pair}): " + "; ".join(bad)
    # the backward route each case exercises (a change to route selection must not silently drop this coverage)
    if training:
        assert len(routes) == len(case[2]), routes
        for r in routes:
            if nb:
                assert r == dict(fused_heads=False, heads_dma=False, wide=True), r
            else:
                assert r == dict(fused_heads=True, heads_dma=True, wide=False), r
    else:
        assert routes == []
    # DEC_PAIR = "1" with two groups: one grid per kernel for both groups, forward and (narrow layout) backward; "0": none
    if pair == "1" and len(case[2]) == 2:
        want = {"spv_dec_tables_grouped", "spv_dec_logits_grouped", "spv_dec_lse_grouped", "spv_dec_nb_fwd_grouped"}
        if training and not nb:
            want |= {"spv_dec_heads_bwd_grouped", "spv_gemm_bf16_grouped"}
        assert want <= set(grouped), grouped
    else:
        assert grouped == [], grouped
