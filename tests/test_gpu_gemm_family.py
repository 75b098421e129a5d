"""The decoder's MFMA GEMM entry points, route by route, against exact float64 products (tests/_gemm_reference.py), at the C ABI where
the routes are chosen: spv_gemm_bf16 (A: 320-column LDS-DMA kernels, C: narrow 128 x 32, D: register-staged 64 x 320), spv_gemm_bf16_fix
(B), spv_gemm_bf16_grouped (E), spv_dec_heads_wgrad (F), spv_dec_logits and spv_dec_logits_grouped (G).

Tier 1 (lattice operands: every partial sum representable) must come back EQUAL to the reference -- per slab, for the summed destination,
for the tiled output; a failure names the first wrong element, its slab and the K tile whose terms account for the difference.  Tier 2
(N(0, 1) operands) must stay inside 2 U n S (+ the f16 rounding) and reports error / bound.  Every case also asserts the route it names,
that no NaN came in from the guards around the operands, that the canary frame around every output is intact, and that a second call gives
the same bits.  tests/test_gemm_reference_cpu.py shows what these comparisons catch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _gemm_reference as R

pytestmark = pytest.mark.gpu

RATIOS = {}   # (route, tier) -> [cases, worst error / bound]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _up(words, dev):
    return None if words is None else torch.from_numpy(np.ascontiguousarray(words).view(np.int16)).to(dev)


def _canaries(shape, dev, dtype=torch.float32):
    return torch.full(shape, R.CANARY, dtype=dtype, device=dev)


def _judge(case, o, runs):
    """runs: the output buffers of two identical calls"""
    first, second = runs
    for buf, g in first.items():
        assert not np.isnan(g.astype(np.float64)).any(), f"{case.name}: {buf}: a NaN came in from a guard (or an operand's padding was not what the header promises)"
        assert g.tobytes() == second[buf].tobytes(), f"{case.name}: {buf}: a second call gives other bits"
    if case.tier == 1:
        assert o.exact, f"{case.name}: the lattice is not exact: this case may not be held to equality"
    fails, ratio = R.compare(case, o, first)
    key = (case.name[0], case.tier)
    n, worst = RATIOS.get(key, (0, 0.0))
    RATIOS[key] = (n + 1, max(worst, ratio))
    if case.tier == 2:
        print(f"{case.name}: error / bound {ratio:.3g}")
    assert not fails, "; ".join(fails)


# ---- spv_gemm_bf16 / _fix ---------------------------------------------------------------------------------------------------------------------
class _Gemm:
    """one case's device operands and the argument list of spv_gemm_bf16"""

    def __init__(self, case, dev):
        from spvipes_amd._abi import ptr
        self.case, self.o = case, R.build(case)
        o = self.o
        self.keep = [_up(w, dev) for w in (o.A_hi, o.A_lo, o.B_hi, o.B_lo)]
        a_hi, a_lo, b_hi, b_lo = self.keep
        boff = 2 * case.b_off
        self.ptrs = (ptr(a_hi), ptr(a_lo), ptr(b_hi) + boff, None if b_lo is None else ptr(b_lo) + boff)
        self.slab_stride = (case.M + 1) * case.ldc
        self.dev = dev

    def assert_route(self):
        from spvipes_amd import _abi
        c, o = self.case, self.o
        uses = _abi.load().spv_gemm_bf16_uses_dma(c.a_kmajor, c.M, c.N, c.K, c.nsplit, o.a_tiles, c.ldb)
        aligned = all(p is None or p % 16 == 0 for p in self.ptrs)
        took = ("dma4s" if c.nsplit == 3 else "dma4") if (uses == 1 and aligned) else ("narrow" if c.N <= 32 else "wide")   # spv_gemm_bf16_fix + gemm_dispatch
        if took != c.kernel:
            pytest.fail(f"{c.name}: the dispatch takes '{took}', the case is meant for '{c.kernel}'")
        if c.a_tiled != (o.a_tiles > 0):
            pytest.fail(f"{c.name}: a_tiles {o.a_tiles} does not select the {'tiled' if c.a_tiled else 'plain'} A staging")

    def args(self, Cbuf):
        from spvipes_amd._abi import ptr
        c, o = self.case, self.o
        a_hi, a_lo, b_hi, b_lo = self.ptrs
        return (c.a_kmajor, a_hi, a_lo, o.lda, b_hi, b_lo, c.ldb, ptr(Cbuf), c.ldc, c.M, c.N, c.K, c.nsplit, c.splits, self.slab_stride, o.a_tiles)

    def run(self, counters=None, alpha=None):
        from spvipes_amd import _abi
        from spvipes_amd._abi import ptr, stream_ptr
        c = self.case
        out = {"C": _canaries((c.splits, c.M + 1, c.ldc), self.dev)}
        if c.fix is None:
            _abi.call("spv_gemm_bf16", *self.args(out["C"]), stream_ptr())
        else:
            n0, c1, n1 = c.fix
            out["d0"] = _canaries((c.M + 1, n0 + 3), self.dev)
            if n1:
                out["d1"] = _canaries((c.M + 1, n1 + 1), self.dev)
            fx = _abi.SpvGemmFixup()
            fx.counters, fx.alpha = ptr(counters), (None if alpha is None else ptr(alpha))
            fx.dst0, fx.ld0, fx.n0 = ptr(out["d0"]), n0 + 3, n0
            fx.dst1, fx.ld1, fx.c1, fx.n1 = (ptr(out["d1"]) if n1 else None), n1 + 1, c1, n1
            _abi.call("spv_gemm_bf16_fix", *self.args(out["C"]), C.byref(fx), stream_ptr())
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", R.route_a_cases() + R.route_c_cases() + R.route_d_cases(), ids=lambda c: c.name)
def test_gemm_slabs(dev, case):
    g = _Gemm(case, dev)
    g.assert_route()
    _judge(case, g.o, [g.run(), g.run()])


@pytest.mark.parametrize("case", R.route_b_cases(), ids=lambda c: c.name)
def test_gemm_fixup(dev, case):
    g = _Gemm(case, dev)
    g.assert_route()
    counters = torch.zeros(R.round_up(case.M, 128) // 128, dtype=torch.int32, device=dev)
    alpha = None if case.alpha == "none" else torch.tensor(case.alpha_value, dtype=torch.float32, device=dev)
    runs = []
    for _ in range(2):    # the same counters twice: the call must leave them zero
        runs.append(g.run(counters, alpha))
        assert int(counters.abs().sum()) == 0, f"{case.name}: the fix-up left its counters at {counters.tolist()}"
    _judge(case, g.o, runs)


def _pair_plan(n, is_pair):
    """pairs_then_rest of spv_abi.hip: pairs from the front while they pair, the rest one by one"""
    plan, i = [], 0
    while i + 1 < n and is_pair(i):
        plan.append("pair")
        i += 2
    return tuple(plan + ["single"] * (n - i))


@pytest.mark.parametrize("name,cases,launches", R.grouped_gemm_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_gemm_grouped(dev, name, cases, launches):
    from spvipes_amd import _abi
    from spvipes_amd._abi import ptr, stream_ptr
    gs = [_Gemm(c, dev) for c in cases]
    for g in gs:
        g.assert_route()

    def is_pair(i):   # gemm_pair_ok of both + the same direction
        return all(g.case.nsplit == 1 and g.case.kernel == "dma4" for g in gs[i:i + 2]) and gs[i].case.a_kmajor == gs[i + 1].case.a_kmajor
    if _pair_plan(len(gs), is_pair) != launches:
        pytest.fail(f"{name}: the groups go out as {_pair_plan(len(gs), is_pair)}, the case is meant for {launches}")
    runs = []
    for _ in range(2):
        outs = [_canaries((g.case.splits, g.case.M + 1, g.case.ldc), dev) for g in gs]
        arr = (_abi.SpvGemmArgs * len(gs))()
        for a, g, out in zip(arr, gs, outs):
            (a.a_kmajor, a.A_hi, a.A_lo, a.lda, a.B_hi, a.B_lo, a.ldb, a.C, a.ldc, a.M, a.N, a.K, a.nsplit, a.splits, a.slab_stride, a.a_tiles) = g.args(out)
        _abi.call("spv_gemm_bf16_grouped", arr, len(gs), stream_ptr())
        torch.cuda.synchronize()
        runs.append([{"C": out.cpu().numpy()} for out in outs])
    for i, g in enumerate(gs):
        _judge(g.case, g.o, [runs[0][i], runs[1][i]])


# ---- spv_dec_heads_wgrad ------------------------------------------------------------------------------------------------------------------------
def _heads_call(case, o, dev, a_tiles=None):
    from spvipes_amd import _abi
    from spvipes_amd._abi import ptr, stream_ptr
    tP, tS, aps = (_up(w, dev) for w in (o.tP_w, o.tS_w, o.aps_w))
    out = {"P": _canaries((case.splits * case.G * 16 + R.HEADS_TAIL,), dev), "S": _canaries((case.splits * case.G * 32 + R.HEADS_TAIL,), dev)}
    _abi.call("spv_dec_heads_wgrad", ptr(tP), ptr(tS), o.a_tiles if a_tiles is None else a_tiles, ptr(aps), case.G, case.Bp, case.splits,
              ptr(out["P"]), ptr(out["S"]), stream_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", R.heads_cases(), ids=lambda c: c.name)
def test_heads_wgrad(dev, case):
    o = R.build(case)
    _judge(case, o, [_heads_call(case, o, dev), _heads_call(case, o, dev)])


@pytest.mark.parametrize("G", [1, 128, 129, 300])
def test_heads_wgrad_takes_exactly_the_tiles_it_reads(dev, G):
    """a_tiles = round_up(G, 128) / 32 is accepted (and right: the cases above with a_extra 0); one tile fewer is refused with the text that says so"""
    from spvipes_amd import _abi
    case = R.HeadsCase(1, G, 64, 1)
    o = R.build(case)
    assert o.a_tiles == R.round_up(G, 128) // 32
    with pytest.raises(_abi.SpvError, match=r"spv_dec_heads_wgrad: Bp must be a multiple of 64 and the tile arrays must cover round_up\(G, 128\) genes"):
        _heads_call(case, o, dev, a_tiles=o.a_tiles - 1)
    _judge(case, o, [_heads_call(case, o, dev), _heads_call(case, o, dev)])


# ---- spv_dec_logits -----------------------------------------------------------------------------------------------------------------------------
class _Logits:
    def __init__(self, case, dev):
        from spvipes_amd._abi import ptr
        self.case, self.o, self.dev = case, R.build(case), dev
        self.keep = [_up(w, dev) for w in (self.o.Am_hi, self.o.Am_lo, self.o.Wm_hi, self.o.Wm_lo)]
        self.ptrs = tuple(ptr(t) for t in self.keep)

    def assert_route(self):
        c = self.case
        am, _, wm, _ = self.ptrs
        dma = c.nsplit == 1 and not c.out_f32 and c.Gp % 256 == 0 and c.Bp % 128 == 0 and am % 16 == 0 and wm % 16 == 0       # spv_dec_logits
        took = "dma" if dma else "g128x128s3" if c.nsplit == 3 else "g256x128" if c.Gp % 256 == 0 else "g128x128"
        if took != c.kernel:
            pytest.fail(f"{c.name}: the dispatch takes '{took}', the case is meant for '{c.kernel}'")

    def out(self):
        c = self.case
        return _canaries((c.Bp * c.Gp + R.LOGITS_TAIL,), self.dev, torch.float32 if c.out_f32 else torch.float16)

    def run(self):
        from spvipes_amd import _abi
        from spvipes_amd._abi import ptr, stream_ptr
        c, out = self.case, self.out()
        _abi.call("spv_dec_logits", *self.ptrs, c.K, c.Bp, c.Gp, c.nsplit, ptr(out), c.out_f32, stream_ptr())
        torch.cuda.synchronize()
        return {"out": out.cpu().numpy()}


@pytest.mark.parametrize("case", R.logits_cases(), ids=lambda c: c.name)
def test_logits(dev, case):
    g = _Logits(case, dev)
    g.assert_route()
    _judge(case, g.o, [g.run(), g.run()])


@pytest.mark.parametrize("name,cases,launches", R.grouped_logits_cases(), ids=lambda v: v if isinstance(v, str) else None)
def test_logits_grouped(dev, name, cases, launches):
    from spvipes_amd import _abi
    from spvipes_amd._abi import ptr, stream_ptr
    gs = [_Logits(c, dev) for c in cases]
    for g in gs:
        g.assert_route()
    plan = _pair_plan(len(gs), lambda i: all(g.case.kernel == "dma" for g in gs[i:i + 2]))      # logits_dma_ok of both
    if plan != launches:
        pytest.fail(f"{name}: the groups go out as {plan}, the case is meant for {launches}")
    runs = []
    for _ in range(2):
        outs = [g.out() for g in gs]
        arr = (_abi.SpvDecGroup * len(gs))()
        for a, g, out in zip(arr, gs, outs):
            a.p.Bp, a.p.Gp, a.p.logits, a.p.logits_f32, a.p.n_gene_tiles = g.case.Bp, g.case.Gp, ptr(out), g.case.out_f32, g.case.Gp // 32
            a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo = g.ptrs
            a.K, a.nsplit = g.case.K, g.case.nsplit
        _abi.call("spv_dec_logits_grouped", arr, len(gs), stream_ptr())
        torch.cuda.synchronize()
        runs.append([{"out": out.cpu().numpy()} for out in outs])
    for i, g in enumerate(gs):
        _judge(g.case, g.o, [runs[0][i], runs[1][i]])


def test_report_ratios():
    """(last in the file) cases and worst error / bound per route and tier, for the lab notes"""
    for (route, tier), (n, worst) in sorted(RATIOS.items()):
        print(f"route {route} tier {tier}: {n} cases, worst error / bound {worst:.3g}")
    assert all(worst == 0.0 for (_, tier), (_, worst) in RATIOS.items() if tier == 1)
    assert all(worst <= 1.0 for (_, tier), (_, worst) in RATIOS.items() if tier == 2)
