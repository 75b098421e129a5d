"""GPU: the fused decode-draw-reduce kernel -- spv_dec_sample_stats through dec_ops.sample_count_stats, on the harness of
tests/test_gpu_posterior_predictive.py.  The yardstick is a numpy uint64 reduction of ``dec_ops.sample_counts``' output for the same
operands, key, sample and cell ids: every entry of ``stats`` and ``cell_total`` must be EQUAL (integer sums do not depend on the order of
addition).  Every test here needs the feature and fails without it.

Shapes: B in {1, 31, 33, 70} (one partial workgroup ... three workgroups, the last partial), 83 genes (three 32-gene tiles, the last
partial) and selections of 1, 31, 33 and 83 of them, one shuffled with a repeat, one ``genes=None``; bf16, fp32 and the wide layout.
Sentinels: the tables start at 7 everywhere (the max row at 0 where a value is expected), so whatever must stay untouched -- padding
columns, rows of a segment without cells, totals of skipped cells -- still reads 7, and accumulation onto a non-zero start is checked
everywhere else.  One larger case (4096 cells x 2100 genes) is the smallest at which a wave walks more than one tile: the grid gives
a wave a second tile only once there are more than 2048 / (B / 32) * 4 tiles."""
import warnings

import numpy as np
import pytest
import torch

from tests.test_gpu_posterior_predictive import _synthetic_module

pytestmark = pytest.mark.gpu

B, GS, G1, SENT = 70, (70, 83), 83, 7
U64 = 1 << 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


class _Case:
    pass


def _make_case(dev, precision, nb, Bn=B, Gs=GS, seed=3):
    """an eval-mode module, one inference output, and group 1's decoder operands (eval-mode BatchNorm: every row is its own
    computation, so the first ``b`` rows of the operands are a minibatch of their own)"""
    c = _Case()
    c.module, noise, tensors = _synthetic_module(dev, precision, Bn, Gs, 25 if nb else 10, 10 if nb else 5, nb, seed=seed)
    with torch.no_grad():
        inf = c.module.inference(**c.module._get_inference_input(tensors), noise={k: v.to(dev) for k, v in noise.items()})
    g = 1
    c.first, c.second, c.par = c.module._decoder_operands(g, inf["private_stats"][g]["log_z"].detach(), inf["poe_stats"][g]["logtheta_log_z"].detach())
    gl = torch.Generator().manual_seed(17)
    c.lib = (np.log(300.0) + np.log(10.0) * torch.rand(Bn, generator=gl)).float().to(dev)   # libraries over a factor of 10
    c.g, c.dev, c.G = g, dev, Gs[g]
    return c


@pytest.fixture(scope="module", params=[("fp32", 0), ("bf16", 0), ("fp32", 12)], ids=lambda p: f"{p[0]}-nb{p[1]}")
def case(request, dev):
    c = _make_case(dev, *request.param)
    assert c.module.dec_slots.kslots == (1 if request.param[1] == 12 else 0)
    return c


def _op(c, fn, b, **kw):
    from spvipes_amd import dec_ops
    m, g = c.module, c.g
    return getattr(dec_ops, fn)(m.decoders[g], m.px_r[g], c.first[:b].contiguous(), c.second[:b].contiguous(), c.lib[:b].contiguous(), False, m.nsplit,
                                m._workspace(g, c.dev), par=c.par, **kw)


def _reduce(x, seg, n_seg):
    """the yardstick: x int32 [b, n] -> (stats uint64 [n_seg, 4, n] with wrap-around squares, counted mask [b], totals uint64 [b])"""
    b, n = x.shape
    x64 = x.astype(np.uint64)
    seg = np.zeros(b, dtype=np.int64) if seg is None else np.asarray(seg, dtype=np.int64)
    counted = (seg >= 0) & (seg < n_seg)
    stats = np.zeros((n_seg, 4, n), dtype=np.uint64)
    for k in range(n_seg):
        rows = x64[counted & (seg == k)]
        if rows.shape[0]:
            stats[k, 0], stats[k, 1], stats[k, 2], stats[k, 3] = rows.sum(0), (rows > 0).sum(0), (rows * rows).sum(0), rows.max(0)
    return stats, counted, x64.sum(1)


def _tables(dev, n_seg, n, b, present, pad=5):
    """tables that start at the sentinel, the max row at 0 wherever a value is expected -> (stats, cell_total) int64 device tensors"""
    stats = torch.full((n_seg, 4, n + pad), SENT, dtype=torch.int64, device=dev)
    for k in present:
        stats[k, 3, :n] = 0
    return stats, torch.full((b + 3,), SENT, dtype=torch.int64, device=dev)


def _expect(stats0, total0, red, n):
    """what the tables must hold after ONE or more reductions were accumulated onto the starting values"""
    want, wtot = stats0.cpu().numpy().view(np.uint64).copy(), total0.cpu().numpy().view(np.uint64).copy()
    for st, counted, tot in red:
        want[:, :3, :n] += st[:, :3]   # (uint64: wraps as the device does)
        want[:, 3, :n] = np.maximum(want[:, 3, :n], st[:, 3])
        wtot[:len(tot)][counted] += tot[counted]
    return want, wtot


def _check(c, b, genes, seg, n_seg, key=11, sample=2, ids=None):
    n = c.G if genes is None else len(genes)
    seg_np = None if seg is None else np.asarray(seg)
    x = _op(c, "sample_counts", b, genes=genes, key=key, sample=sample, cell_ids=ids).cpu().numpy()
    assert x.shape == (b, n)
    red = _reduce(x, seg_np, n_seg)
    present = [k for k in range(n_seg) if (red[0][k, 0] > 0).any() or (seg_np is None and k == 0) or (seg_np is not None and (seg_np == k).any())]
    stats, total = _tables(c.dev, n_seg, n, b, present)
    want, wtot = _expect(stats, total, [red], n)
    seg_d = None if seg is None else torch.as_tensor(seg_np, dtype=torch.int32, device=c.dev)
    got = _op(c, "sample_count_stats", b, genes=genes, key=key, sample=sample, cell_ids=ids, seg=seg_d, n_seg=n_seg, stats=stats, cell_total=total)
    assert got.data_ptr() == stats.data_ptr()
    np.testing.assert_array_equal(stats.cpu().numpy().view(np.uint64), want)
    np.testing.assert_array_equal(total.cpu().numpy().view(np.uint64), wtot)
    return x, red


def _selections():
    rng = np.random.default_rng(5)
    shuffled = rng.permutation(G1)[:40]
    shuffled[-1] = shuffled[33] = shuffled[2]   # a repeated gene, across two tiles
    return {"one": np.array([57]), "31": np.arange(31) + 20, "33": np.arange(33)[::-1].copy() + 50, "83": np.arange(G1), "shuffled": shuffled, "none": None}


@pytest.mark.parametrize("b", [1, 31, 33, 70])
def test_tables_equal_the_reduction_of_the_stored_draws(case, b):
    """every shape x every selection x every kind of segment vector: exact equality, sentinels included"""
    rng = np.random.default_rng(b)
    skip = np.arange(b) % 3
    skip[rng.random(b) < 0.3] = -1
    skip[rng.random(b) < 0.1] = 9      # a code the table has no rows for: skipped like a negative one
    if b > 1:
        skip[0], skip[1] = -1, 0       # (for certain: a skipped cell and a counted one)
    segs = {"none": (None, 1), "interleaved": (np.arange(b) % 3, 3), "absent-label": (np.arange(b) % 3 + 2 * (np.arange(b) % 3 == 2), 5), "skipped": (skip, 3)}
    ids = (torch.arange(b, device=case.dev) * 3 + 1000).int()
    drawn = 0
    for sname, genes in _selections().items():
        for gname, (seg, n_seg) in segs.items():
            x, (st, counted, tot) = _check(case, b, genes, seg, n_seg, ids=ids)
            drawn += int(x.sum())
            if gname == "absent-label":
                assert not st[2].any() and not st[3].any()   # labels 2 and 3 have no cells: their rows kept the sentinel (checked in _check)
            if gname == "skipped" and b > 1:
                assert not counted.all() and counted.any()
            if sname == "shuffled":
                np.testing.assert_array_equal(x[:, -1], x[:, 2])   # a repeated gene fills its own column with the same draws
    assert drawn > 0


def test_two_samples_accumulate_and_a_split_batch_equals_the_single_call(case):
    c, n_seg = case, 3
    seg = (np.arange(B) * 7 % 5 % 3).astype(np.int32)
    seg[[4, 41, 69]] = -1
    genes = _selections()["shuffled"]
    n = len(genes)
    ids = (torch.arange(B, device=c.dev) + 500).int()
    seg_d = torch.as_tensor(seg, device=c.dev)
    # two samples into one table
    red = [_reduce(_op(c, "sample_counts", B, genes=genes, key=5, sample=s, cell_ids=ids).cpu().numpy(), seg, n_seg) for s in (0, 1)]
    assert not np.array_equal(red[0][0], red[1][0])
    stats, total = _tables(c.dev, n_seg, n, B, range(n_seg))
    want, wtot = _expect(stats, total, red, n)
    for s in (0, 1):
        _op(c, "sample_count_stats", B, genes=genes, key=5, sample=s, cell_ids=ids, seg=seg_d, n_seg=n_seg, stats=stats, cell_total=total)
    np.testing.assert_array_equal(stats.cpu().numpy().view(np.uint64), want)
    np.testing.assert_array_equal(total.cpu().numpy().view(np.uint64), wtot)
    # B = 70 as 40 + 30 rows, the cell ids carrying the original numbers: the same tables as the single call of sample 0
    from spvipes_amd import dec_ops
    m, g = c.module, c.g
    single, stot = _tables(c.dev, n_seg, n, B, range(n_seg))
    _op(c, "sample_count_stats", B, genes=genes, key=5, sample=0, cell_ids=ids, seg=seg_d, n_seg=n_seg, stats=single, cell_total=stot)
    split, ptot = _tables(c.dev, n_seg, n, B, range(n_seg))
    for lo, hi in ((0, 40), (40, 70)):
        dec_ops.sample_count_stats(m.decoders[g], m.px_r[g], c.first[lo:hi].contiguous(), c.second[lo:hi].contiguous(), c.lib[lo:hi].contiguous(), False,
                                   m.nsplit, m._workspace(g, c.dev), par=c.par, genes=genes, key=5, sample=0, cell_ids=ids[lo:hi].contiguous(),
                                   seg=seg_d[lo:hi].contiguous(), n_seg=n_seg, stats=split, cell_total=ptot[lo:hi])
    assert torch.equal(split, single) and torch.equal(ptot[:B], stot[:B])
    np.testing.assert_array_equal(single.cpu().numpy().view(np.uint64), _expect(*_tables(c.dev, n_seg, n, B, range(n_seg)), red[:1], n)[0])
    # without cell ids the row number names the cell: other draws for the second part, the same for the first
    a, _ = _tables(c.dev, n_seg, n, B, range(n_seg))
    b_, _ = _tables(c.dev, n_seg, n, B, range(n_seg))
    _op(c, "sample_count_stats", 40, genes=genes, key=5, sample=0, cell_ids=None, seg=seg_d, n_seg=n_seg, stats=a)
    _op(c, "sample_count_stats", 40, genes=genes, key=5, sample=0, cell_ids=torch.arange(40, device=c.dev).int(), seg=seg_d, n_seg=n_seg, stats=b_)
    assert torch.equal(a, b_)


def test_two_identical_calls_agree_bit_for_bit(case):
    """no floating-point atomics are involved: the order in which the workgroups arrive cannot show"""
    seg = torch.as_tensor((np.arange(B) % 3).astype(np.int32), device=case.dev)
    out = []
    for _ in range(2):
        stats = torch.zeros((3, 4, G1), dtype=torch.int64, device=case.dev)
        total = torch.zeros(B, dtype=torch.int64, device=case.dev)
        _op(case, "sample_count_stats", B, key=99, sample=7, seg=seg, n_seg=3, stats=stats, cell_total=total)
        out.append((stats, total))
    assert int(out[0][0].sum()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    if hasattr(torch, "uint64"):   # a torch.uint64 table is taken as well: the same bits
        stats = torch.zeros((3, 4, G1), dtype=torch.uint64, device=case.dev)
        _op(case, "sample_count_stats", B, key=99, sample=7, seg=seg, n_seg=3, stats=stats)
        assert torch.equal(stats.view(torch.int64), out[0][0])


def test_the_square_sum_wraps_modulo_2_64_and_ppc_table_says_so(case):
    """library_size = 1e12: the rates hit the sampler's 1e8 clamp, a draw is ~1e8 and its square ~1e16; 30 samples of 70 cells put 2100
    of them into one entry, 2.1e19 > 2^64 = 1.8e19.  Row 2 equals numpy's uint64 wrap-around sum, row 3 the max, and ppc_table reports
    NaN variances with its warning."""
    from spvipes_amd.data import ppc_table
    c, n_samples = case, 30
    stats = torch.zeros((1, 4, G1), dtype=torch.int64, device=c.dev)
    total = torch.zeros(B, dtype=torch.int64, device=c.dev)
    want = np.zeros((1, 4, G1), dtype=np.uint64)
    exact_sq = np.zeros(G1, dtype=object)
    wtot = np.zeros(B, dtype=np.uint64)
    for s in range(n_samples):
        x = _op(c, "sample_counts", B, library_size=1e12, key=3, sample=s).cpu().numpy()
        st, _, tot = _reduce(x, None, 1)
        want[:, :3] += st[:, :3]
        want[:, 3] = np.maximum(want[:, 3], st[:, 3])
        wtot += tot
        exact_sq += (x.astype(object) ** 2).sum(0)
        _op(c, "sample_count_stats", B, library_size=1e12, key=3, sample=s, stats=stats, cell_total=total)
    wrapped = np.array([v >= U64 for v in exact_sq])
    assert wrapped.sum() >= 10 and int(want[0, 3].max()) >= 10 ** 8   # the case does what it is here for
    got = stats.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0, 2], np.array([v % U64 for v in exact_sq], dtype=np.uint64))
    np.testing.assert_array_equal(total.cpu().numpy().view(np.uint64), wtot)
    N = B * n_samples
    flagged = np.array([N * int(m) ** 2 >= U64 for m in got[0, 3]])
    assert (flagged | ~wrapped).all()   # the rule covers every entry that did wrap
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        df = ppc_table(got, [N])
    mine = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(mine) == 1 and f"{int(flagged.sum())} (segment, gene)" in str(mine[0].message)
    assert np.isnan(df["ppc_var"].to_numpy()[flagged]).all() and np.isfinite(df["ppc_var"].to_numpy()[~flagged]).all()
    np.testing.assert_array_equal(df["ppc_max"].to_numpy(), got[0, 3].astype(np.float64))


def test_a_wave_that_walks_several_tiles(dev):
    """4096 cells x 2100 genes, bf16: 128 workgroup columns leave 16 gene slices of 4 waves for 66 tiles, so waves take a second tile --
    the tile buffers are reused and a lane's cell total runs across tiles.  20 interleaved labels, as the benchmark has them."""
    Bn, Gn, n_seg = 4096, 2100, 20
    c = _make_case(dev, "bf16", 0, Bn=Bn, Gs=(70, Gn), seed=4)
    seg = (np.arange(Bn) * 13 % n_seg).astype(np.int32)
    seg[::97] = -1
    x = _op(c, "sample_counts", Bn, key=8, sample=1).cpu().numpy()
    st, counted, tot = _reduce(x, seg, n_seg)
    stats = torch.zeros((n_seg, 4, Gn), dtype=torch.int64, device=dev)
    total = torch.full((Bn,), SENT, dtype=torch.int64, device=dev)
    _op(c, "sample_count_stats", Bn, key=8, sample=1, seg=torch.as_tensor(seg, device=dev), n_seg=n_seg, stats=stats, cell_total=total)
    np.testing.assert_array_equal(stats.cpu().numpy().view(np.uint64), st)
    np.testing.assert_array_equal(total.cpu().numpy().view(np.uint64), np.where(counted, tot + np.uint64(SENT), np.uint64(SENT)))


def test_abi_argument_errors_are_reported(case):
    from spvipes_amd import _abi
    c = case
    stats = torch.zeros((2, 4, G1), dtype=torch.int64, device=c.dev)
    for bad in (dict(stats=stats[:1]), dict(stats=stats.float()), dict(stats=stats[:, :, :50]), dict(stats=stats, n_seg=2, seg=torch.zeros(B, device=c.dev)),
                dict(stats=stats, cell_total=torch.zeros(B - 1, dtype=torch.int64, device=c.dev)), dict(stats=stats, cell_ids=torch.zeros(B, device=c.dev))):
        kw = dict(dict(n_seg=2), **bad)
        with pytest.raises(_abi.SpvError, match="sample_count_stats"):
            _op(c, "sample_count_stats", B, **kw)
    with pytest.raises(IndexError, match=str(G1)):
        _op(c, "sample_count_stats", B, genes=[0, G1], stats=stats, n_seg=2)
    with pytest.raises(_abi.SpvError, match="library override"):
        _op(c, "sample_count_stats", B, stats=stats, n_seg=2, log_library=torch.zeros(B - 1, device=c.dev))
    assert not bool(stats.any())   # nothing was launched
