"""GPU: differential expression -- spv_de_pairs through de_ops.de_pairs and spVIPES.differential_expression -- against float64 numpy
statistics computed HERE from the bank contents on the host and the same pair rows, never from the code under test.

Bounds (derived from the number formats and the documented reduction, not from observed errors).  With U = 2^-24 (half an fp32 ulp,
relative), L = the largest |log2(max(x + eps, FLT_MIN))| over the two banks (<= 40 by construction of the random part; the planted
column next to FLT_MIN raises it to 126), u = 1 = the error of the kernel's log2 in fp32 ulps -- it is the hardware's V_LOG_F32, which
AMD's CDNA ISA reference guides specify as "1 ULP accuracy", the figure the HIP math API documentation lists for ``__log2f`` too --
and one ulp of a value v being at most 2 U |v|:

  per term   |lfc32 - lfc64| <= tol = 2 * (u * 2 U * L)      the two logarithms (the issue's 2 * u * 40, in absolute units)
                                     + U * 2 L                the rounding of their difference, |lfc| <= 2 L
                                     + 2 * U / ln 2           the rounding of x + eps, seen through log2
  lfc_min / lfc_max : tol (they are one term each).
  lfc_mean : tol + (n_c + 2) U R + U |mean|.  A lane adds at most n_c = ceil(ceil(n_pairs / S) / 4) deviations t = lfc - K (K = its chunk's
             first lfc, |t| <= R = max - min of the column, widened by 2 tol) sequentially in fp32, S = spv_de_pairs_splits(...): error
             <= n_c U per unit of sum |t|, plus U per t for forming it; everything above the lane is fp64; U |mean| is the final rounding.
  lfc_std  : tol + min(sqrt(V), V / std) + U std,  V = 5 (n_c + 2) U R^2:  shifting every term by at most tol moves a standard deviation
             by at most tol; the lane's sum of t^2 (n_c + 1 roundings of non-negative terms) and its s^2 / n (2 n_c, by Cauchy-Schwarz)
             are off by at most 3 (n_c + 2) U n R^2 together, and Chan's cross terms take the chunk means with their n_c U R error twice:
             2 n_c U R^2 more per unit of n.  A variance off by V moves the std by at most sqrt(V), and by at most V / std.
             (A plain fp32 sum(x^2) - sum(x)^2 at lfc = 20 would be off by n_pairs U 400 ~ 0.24 in the variance of a column whose
             variance is 1e-4; the planted column makes the bound 6e-5 on a std of 1e-2.)
  scale1/2 : relative min(n_pairs, n_c + 2) U (positive terms, sequential fp32 in the lane, fp64 above, one final rounding).
  counts   : an element is undecided when | |lfc64| - delta | <= tol; per gene the kernel's count must lie in [sure, sure + undecided].
             The undecided share of every input is asserted <= 1e-3 from the float64 reference alone, before the kernel is looked at.

The gene-subset identity of the issue is not tested: the number of pair splits S depends on n_genes (that is how the grid fills the chip
at 64 genes as well as at 10 000), so a gene's chunk boundaries, and with them its last bits, depend on the selection's size."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLT_MIN = float(np.finfo(np.float32).tiny)
LOG2_ULPS = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


# ---- inputs and the float64 reference --------------------------------------------------------------------------------------------
def _bank(rng, rows, ng, ld, planted, which):
    """fp32 [rows, ld] (columns >= ng hold NaN: they must never be read into a result): exp2 of normals clipped to |log2 x| <= 40"""
    b = np.full((rows, ld), np.nan, np.float32)
    b[:, :ng] = np.exp2(np.clip(rng.normal(0.0, 12.0, (rows, ng)), -40.0, 40.0)).astype(np.float32)
    if planted and ng >= 8:
        b[:, 0] = (3.5, 0.75)[which]                                                  # constant columns: lfc = log2(3.5 / 0.75)
        b[:, 1] = 0.3                                                                  # the same constant on both sides: lfc = 0
        b[:, 2] = np.exp2((10.0, -10.0)[which] + rng.normal(0.0, 1e-2 / math.sqrt(2.0), rows)).astype(np.float32)   # lfc = 20 +- 1e-2
        b[:, 3] = (FLT_MIN * (1.0 + 3.0 * rng.random(rows))).astype(np.float32)        # tiny, never subnormal
        assert (b[:, 3] >= FLT_MIN).all()
    return b


def _tol(b1, b2, ng, eps):
    e = float(np.float32(eps))
    L = max(float(np.abs(np.log2(np.maximum(b[:, :ng].astype(np.float64) + e, FLT_MIN))).max()) for b in (b1, b2))
    return 2 * LOG2_ULPS * 2 * U * L + U * 2 * L + 2 * U / math.log(2.0), L


def _reference(b1, b2, r1, r2, ng, eps, delta, tol, cols=None):
    """float64 statistics per gene, plus the sure / undecided exceedance counts at ``tol``; columns in blocks to bound host memory"""
    e = float(np.float32(eps))
    i1, i2 = np.clip(r1, 0, b1.shape[0] - 1), np.clip(r2, 0, b2.shape[0] - 1)
    out = {k: np.empty(ng) for k in ("lfc_mean", "lfc_std", "lfc_min", "lfc_max", "scale1", "scale2", "sure", "undecided")}
    step = max(1, min(ng, (1 << 23) // len(r1)))
    for c0 in range(0, ng, step):
        c = slice(c0, min(ng, c0 + step))
        x1, x2 = b1[i1, c].astype(np.float64), b2[i2, c].astype(np.float64)
        d = np.log2(np.maximum(x1 + e, FLT_MIN)) - np.log2(np.maximum(x2 + e, FLT_MIN))
        out["lfc_mean"][c], out["lfc_std"][c], out["lfc_min"][c], out["lfc_max"][c] = d.mean(0), d.std(0), d.min(0), d.max(0)
        out["scale1"][c], out["scale2"][c] = x1.mean(0), x2.mean(0)
        a = np.abs(d)
        out["sure"][c], out["undecided"][c] = (a > delta + tol).sum(0), (np.abs(a - delta) <= tol).sum(0)
    return out


def _check(got, ref, n_pairs, n_c, tol, ctx):
    """``got``: name -> float64 host arrays of the kernel's seven statistics; prints every figure before it asserts"""
    R = ref["lfc_max"] - ref["lfc_min"] + 2 * tol
    V = 5 * (n_c + 2) * U * R * R
    with np.errstate(divide="ignore", invalid="ignore"):
        v_std = np.where(ref["lfc_std"] > 0, np.minimum(np.sqrt(V), V / ref["lfc_std"]), np.sqrt(V))
    bounds = {"lfc_min": tol + 0 * R, "lfc_max": tol + 0 * R, "lfc_mean": tol + (n_c + 2) * U * R + U * np.abs(ref["lfc_mean"]),
              "lfc_std": tol + v_std + U * ref["lfc_std"],
              "scale1": min(n_pairs, n_c + 2) * U * ref["scale1"], "scale2": min(n_pairs, n_c + 2) * U * ref["scale2"]}
    worst = {}
    for k, b in bounds.items():
        assert np.isfinite(got[k]).all(), f"{ctx} {k}: non-finite values"
        err = np.abs(got[k] - ref[k])
        worst[k] = float((err - b).max())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.nanmax(np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))))
        print(f"{ctx} {k}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    lo, hi = ref["sure"], ref["sure"] + ref["undecided"]
    outside = int(((got["count_de"] < lo) | (got["count_de"] > hi)).sum())
    print(f"{ctx} count_de: {outside} genes outside [sure, sure + undecided]; undecided elements {int(ref['undecided'].sum())}")
    for k, w in worst.items():
        assert w <= 0.0, f"{ctx} {k}: outside the bound by {w:.3e}"
    assert (got["count_de"] == np.round(got["count_de"])).all() and outside == 0, f"{ctx}: {outside} genes' counts outside the decided range"


def _host(stats):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in stats.items()}


def _n_c(ng, n_pairs):
    from spvipes_amd.de_ops import de_splits
    return -(-(-(-n_pairs // de_splits(ng, n_pairs))) // 4)


def _run_case(dev, rows_1, rows_2, ng, n_pairs, ld1, ld2, eps, delta=0.25, seed=0, banks=None):
    from spvipes_amd.de_ops import de_pairs, de_workspace
    rng = np.random.default_rng(seed)
    b1, b2 = banks if banks is not None else (_bank(rng, rows_1, ng, ld1, True, 0), _bank(rng, rows_2, ng, ld2, True, 1))
    r1, r2 = rng.integers(0, rows_1, n_pairs).astype(np.int32), rng.integers(0, rows_2, n_pairs).astype(np.int32)
    ctx = f"[{rows_1} x {rows_2} rows, {ng} genes, {n_pairs} pairs, eps {eps:g}]"
    tol, L = _tol(b1, b2, ng, eps)
    ref = _reference(b1, b2, r1, r2, ng, eps, delta, tol)
    share = float(ref["undecided"].sum()) / (ng * n_pairs)
    print(f"{ctx} L = {L:.1f}, tol = {tol:.3e}, undecided share {share:.3e}")
    assert share <= 1e-3   # from the reference alone
    d1, d2 = torch.from_numpy(b1).to(dev)[:, :ng], torch.from_numpy(b2).to(dev)[:, :ng]   # row stride ld, ng columns
    stats = de_pairs(d1, d2, torch.from_numpy(r1).to(dev), torch.from_numpy(r2).to(dev), delta=delta, eps=eps, ws=de_workspace(ng, n_pairs, dev))
    got = _host(stats)
    _check(got, ref, n_pairs, _n_c(ng, n_pairs), tol, ctx)
    return got, ref, (b1, b2, r1, r2)


# ---- 1. kernel vs float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4096, 4096, 10_000, 10_000, 10_016, 10_000, 0.0), (37, 5000, 10_003, 777, 10_003, 10_048, 1e-6),
                                   (1, 1, 1, 1, 1, 5, 0.0), (4096, 64, 64, 1 << 20, 64, 72, 1e-6), (300, 200, 1000, 10_000, 1000, 1000, 0.0)],
                         ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_kernel_against_float64(dev, shape):
    rows_1, rows_2, ng, n_pairs, ld1, ld2, eps = shape
    got, ref, _ = _run_case(dev, rows_1, rows_2, ng, n_pairs, ld1, ld2, eps)
    if ng >= 8:
        for col in (0, 1):   # constant columns: no spread at all, exactly
            assert got["lfc_std"][col] == 0.0 and got["lfc_min"][col] == got["lfc_max"][col] == got["lfc_mean"][col]
        if eps == 0.0:
            assert got["lfc_mean"][1] == 0.0 and got["count_de"][1] == 0.0 and got["count_de"][0] == n_pairs
        assert abs(ref["lfc_mean"][2] - 20.0) < 1e-2 and 5e-3 < ref["lfc_std"][2] < 2e-2   # the planted column is what it claims to be
        print(f"planted lfc 20 +- 1e-2 column: std {got['lfc_std'][2]:.6e} against {ref['lfc_std'][2]:.6e}")


def test_counts_on_the_issue_input(dev):
    """banks exp2(normal(-13, 3)) as fp32 [4096, 2000], 10 000 seeded pairs, delta 0.25"""
    rng = np.random.default_rng(7)
    banks = tuple(np.exp2(rng.normal(-13.0, 3.0, (4096, 2000))).astype(np.float32) for _ in range(2))
    _run_case(dev, 4096, 4096, 2000, 10_000, 2000, 2000, 0.0, delta=0.25, seed=8, banks=banks)


def test_powers_of_two_are_exact(dev):
    """banks of powers of two, eps 0, delta 0.5: every lfc is a whole number, so counts, min, max and mean equal the float64 values"""
    from spvipes_amd.de_ops import de_pairs
    rng = np.random.default_rng(11)
    ng, n_pairs = 777, 4096
    b1, b2 = (np.exp2(rng.integers(-40, 41, (500, ng)).astype(np.float64)).astype(np.float32) for _ in range(2))
    r1, r2 = rng.integers(0, 500, n_pairs).astype(np.int32), rng.integers(0, 500, n_pairs).astype(np.int32)
    d = np.log2(b1[r1].astype(np.float64)) - np.log2(b2[r2].astype(np.float64))
    assert (d == np.round(d)).all()
    got = _host(de_pairs(*(torch.from_numpy(a).to(dev) for a in (b1, b2, r1, r2)), delta=0.5, eps=0.0))
    np.testing.assert_array_equal(got["count_de"], (np.abs(d) >= 0.5).sum(0))
    np.testing.assert_array_equal(got["lfc_min"], d.min(0))
    np.testing.assert_array_equal(got["lfc_max"], d.max(0))
    np.testing.assert_array_equal(got["lfc_mean"], d.sum(0) / n_pairs)   # whole sums over 2^12: representable in fp32
    np.testing.assert_allclose(got["lfc_std"], d.std(0), rtol=4 * U, atol=0)   # fp64 throughout (the deviations are whole numbers), one rounding


# ---- 2. identities ----------------------------------------------------------------------------------------------------------------
def test_identities(dev):
    from spvipes_amd.de_ops import de_pairs
    rng = np.random.default_rng(21)
    ng, n_pairs = 1500, 5000
    b1, b2 = _bank(rng, 700, ng, ng + 4, True, 0), _bank(rng, 90, ng, ng, True, 1)
    r1, r2 = rng.integers(0, 700, n_pairs).astype(np.int32), rng.integers(0, 90, n_pairs).astype(np.int32)
    d1, d2 = torch.from_numpy(b1).to(dev)[:, :ng], torch.from_numpy(b2).to(dev)
    t1, t2 = torch.from_numpy(r1).to(dev), torch.from_numpy(r2).to(dev)
    a = de_pairs(d1, d2, t1, t2, delta=0.25, eps=1e-6)
    b = de_pairs(d1, d2, t1, t2, delta=0.25, eps=1e-6)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two calls differ"
    assert bool(torch.isfinite(torch.stack(list(a.values()))).all())   # the NaN padding beyond n_genes was never read
    s = de_pairs(d2, d1, t2, t1, delta=0.25, eps=1e-6)   # swapped: every lfc changes sign, nothing else
    assert torch.equal(s["lfc_mean"], -a["lfc_mean"]) and torch.equal(s["lfc_std"], a["lfc_std"]) and torch.equal(s["count_de"], a["count_de"])
    assert torch.equal(s["lfc_min"], -a["lfc_max"]) and torch.equal(s["lfc_max"], -a["lfc_min"])
    assert torch.equal(s["scale1"], a["scale2"]) and torch.equal(s["scale2"], a["scale1"])
    # row numbers outside a bank are clamped into it: -5 behaves as 0, n_rows + 5 as n_rows - 1
    wild1, wild2 = r1.copy(), r2.copy()
    lo, hi = np.nonzero(r1 == 0)[0], np.nonzero(r2 == 89)[0]
    assert lo.size and hi.size
    wild1[lo], wild2[hi] = -5, 89 + 6
    wild1[np.nonzero(r1 == 699)[0]] = 699 + 6
    c = de_pairs(d1, d2, torch.from_numpy(wild1).to(dev), torch.from_numpy(wild2).to(dev), delta=0.25, eps=1e-6)
    for k in a:
        assert torch.equal(a[k], c[k]), f"{k}: clamped row numbers change the result"
    # a caller's output array with a wider row stride: same numbers, columns beyond n_genes untouched
    out = torch.full((7, ng + 9), -7.0, device=dev)
    o = de_pairs(d1, d2, t1, t2, delta=0.25, eps=1e-6, out=out)
    for k in a:
        assert torch.equal(a[k], o[k])
    assert bool((out[:, ng:] == -7.0).all())


def test_argument_errors_are_reported(dev):
    import ctypes as C
    from spvipes_amd import _abi
    from spvipes_amd.de_ops import de_pairs, de_workspace
    bank = torch.ones(8, 100, device=dev)
    rows = torch.zeros(50, dtype=torch.int32, device=dev)
    stats, ws = torch.empty(7, 100, device=dev), de_workspace(100, 50, dev)

    def args(**kw):
        a = _abi.SpvDePairsArgs()
        a.bank1, a.bank2, a.ld1, a.ld2, a.rows1, a.rows2, a.n_rows1, a.n_rows2 = bank.data_ptr(), bank.data_ptr(), 100, 100, rows.data_ptr(), rows.data_ptr(), 8, 8
        a.n_genes, a.n_pairs, a.delta, a.eps, a.stats, a.ld_stats, a.ws, a.ws_bytes = 100, 50, 0.25, 0.0, stats.data_ptr(), 100, ws.data_ptr(), ws.numel() * 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    _abi.call("spv_de_pairs", C.byref(args()), _abi.stream_ptr())   # the good call
    for bad in (dict(bank1=None), dict(bank2=None), dict(rows1=None), dict(rows2=None), dict(stats=None), dict(ws=None), dict(n_pairs=0), dict(n_pairs=-3),
                dict(n_pairs=(1 << 24) + 1), dict(ld1=99), dict(ld2=99), dict(ld_stats=99), dict(n_genes=0), dict(n_rows1=0), dict(ws_bytes=ws.numel() * 8 - 8),
                dict(delta=-1.0), dict(eps=float("nan"))):
        with pytest.raises(_abi.SpvError, match="spv_de_pairs"):
            _abi.call("spv_de_pairs", C.byref(args(**bad)), _abi.stream_ptr())
    torch.cuda.synchronize()
    with pytest.raises(_abi.SpvError):
        de_pairs(bank.double(), bank, rows, rows, delta=0.25)
    with pytest.raises(_abi.SpvError):
        de_pairs(bank.t(), bank.t(), rows, rows, delta=0.25)   # column stride != 1
    with pytest.raises(_abi.SpvError):
        de_pairs(bank, bank, rows.long(), rows, delta=0.25)
    with pytest.raises(_abi.SpvError):
        de_pairs(bank, bank[:, :50], rows, rows, delta=0.25)
    with pytest.raises(_abi.SpvError):
        de_pairs(bank, bank, rows, rows, delta=0.25, ws=ws[:-1])
    with pytest.raises(ValueError):
        de_pairs(bank, bank, rows, rows[:10], delta=0.25)
    with pytest.raises(ValueError):
        de_pairs(bank, bank, rows, rows, delta=-0.25)


# ---- 3. user API -------------------------------------------------------------------------------------------------------------------
def _noise_fn(dev, n_s=10, n_p=5):
    def noise(draw, b0, b1):
        g = torch.Generator(device="cpu").manual_seed(1000 + draw)
        mk = lambda b, n: torch.randn(b, n, generator=g).to(dev)
        return {"enc_0_private": mk(b0, n_p), "enc_0_shared": mk(b0, n_s), "enc_1_private": mk(b1, n_p), "enc_1_shared": mk(b1, n_s),
                "poe_0": mk(b0, n_s), "poe_1": mk(b1, n_s)}
    return noise


def _frame_check(df, bank1, bank2, r1, r2, delta, eps, fdr_target, ctx):
    """the DataFrame against float64 statistics of the given host banks (fp32 arrays) and pair rows"""
    from spvipes_amd.data import DE_COLUMNS
    ng, n_pairs = bank1.shape[1], len(r1)
    assert list(df.columns) == list(DE_COLUMNS) + [f"is_de_fdr_{fdr_target}"] and len(df) == ng
    tol, _L = _tol(bank1, bank2, ng, eps)
    ref = _reference(bank1, bank2, r1, r2, ng, eps, delta, tol)
    got = {k: df[k].to_numpy().astype(np.float64) for k in ("lfc_mean", "lfc_std", "lfc_min", "lfc_max", "scale1", "scale2")}
    got["count_de"] = df["proba_de"].to_numpy() * n_pairs
    assert np.abs(got["count_de"] - np.round(got["count_de"])).max() < 1e-6
    got["count_de"] = np.round(got["count_de"])
    _check(got, ref, n_pairs, _n_c(ng, n_pairs), tol, ctx)
    p = df["proba_de"].to_numpy()
    np.testing.assert_array_equal(df["proba_not_de"].to_numpy(), 1.0 - p)
    np.testing.assert_allclose(df["bayes_factor"].to_numpy(), np.log(p + 1e-8) - np.log(1.0 - p + 1e-8), rtol=0, atol=1e-12)
    order = np.argsort(-p, kind="stable")
    fdr = np.cumsum((1.0 - p)[order]) / (1.0 + np.arange(ng))
    want = np.zeros(ng, bool)
    want[order[: int((fdr <= fdr_target).sum())]] = True
    np.testing.assert_array_equal(df[f"is_de_fdr_{fdr_target}"].to_numpy(), want)


@pytest.mark.parametrize("config,precision", [("label", "fp32"), ("paired", "bf16"), ("batch_key", "fp32"), ("sparse", "bf16")])
def test_differential_expression(dev, tmp_path, config, precision):
    from spvipes_amd.data import de_subsample
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    def adata():
        ad = make_duck(n=(96, 70) if config == "paired" else (300, 260), seed=2, with_plan=(config == "paired"))   # n0 != n1, ragged last batches
        ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
        if config == "batch_key":
            ad.obs["donor"] = np.random.default_rng(4).choice(np.array(["d1", "d2", "d3"]), size=ad.n_obs)
        return ad

    ad = adata()
    kw = {"transport_plan_key": "plan"} if config == "paired" else {"label_key": "cell_type"}
    if config == "batch_key":
        kw["batch_key"] = "donor"
    spVIPES.setup_anndata(ad, groups_key="groups", **kw)
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=precision,
                    counts_storage=("sparse" if config == "sparse" else "auto"))   # CSR-resident counts, densified per minibatch
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    bs = 64 if config != "paired" else 32
    g = 1 if config in ("paired", "sparse") else 0
    G, off = (96, 80)[g], (0, 96)[g]
    cells = np.asarray(gi[g])
    rng = np.random.default_rng(5)
    idx1 = cells[rng.permutation(len(cells))[: len(cells) // 3]]           # adata rows, in no particular order
    rest = np.setdiff1d(cells, idx1)
    idx2 = rest[rng.permutation(len(rest))[: len(rest) // 2]]
    pos = np.array([5, 0, G - 1, 5, 17, 33, 2, 70])
    names = [f"gene{off + i}" for i in pos]
    where = {c: i for i, c in enumerate(cells.tolist())}
    p1, p2 = (np.array([where[c] for c in idx.tolist()]) for idx in (idx1, idx2))
    n_pairs = 3000
    r1, r2 = rng.integers(0, len(p1), n_pairs).astype(np.int32), rng.integers(0, len(p2), n_pairs).astype(np.int32)
    gl = [None, None]
    gl[g] = pos

    # (a) posterior means: the banks are the public read-out's rows
    model.module.train()   # the call must put the module into eval mode and restore this
    df = model.differential_expression(gi, g, idx1, idx2, gene_list=pos, use_mean=True, batch_size=bs, _pair_rows=(r1, r2))
    assert model.module.training
    ne = model.get_normalized_expression(gi, gene_list=gl, library_size=1.0, batch_size=bs)[g]
    assert df.index.tolist() == names
    _frame_check(df, ne[p1], ne[p2], r1, r2, 0.25, 0.0, 0.05, f"[{config} {precision} use_mean]")
    by_name = model.differential_expression(gi, g, idx1, idx2, gene_list=names, use_mean=True, batch_size=bs, _pair_rows=(r1, r2))
    assert by_name.equals(df)
    again = model.differential_expression(gi, g, idx1, idx2, gene_list=pos, use_mean=True, batch_size=bs, _pair_rows=(r1, r2))
    assert again.equals(df)

    # (b) all genes, idx2=None (every other cell), drawn pairs, a pseudocount and another delta / target; max_cells
    model.module.eval()
    full = model.get_normalized_expression(gi, library_size=1.0, batch_size=bs)[g]
    others = np.array([i for i in range(len(cells)) if i not in set(p1.tolist())])
    d2 = model.differential_expression(gi, g, idx1, use_mean=True, n_pairs=2000, delta=0.1, pseudocount=1e-6, fdr_target=0.2, seed=3, batch_size=bs)
    assert not model.module.training and d2.index.tolist() == [f"gene{off + i}" for i in range(G)]
    q = np.random.default_rng(3)
    q1, q2 = q.integers(0, len(p1), 2000).astype(np.int32), q.integers(0, len(others), 2000).astype(np.int32)
    _frame_check(d2, full[p1], full[others], q1, q2, 0.1, 1e-6, 0.2, f"[{config} {precision} idx2=None]")
    d3 = model.differential_expression(gi, g, idx1, idx2, gene_list=pos, use_mean=True, max_cells=20, seed=9, batch_size=bs, _pair_rows=(r1 % 20, r2 % 20))
    s1, s2 = de_subsample(p1, 20, 10), de_subsample(p2, 20, 11)   # population k is subsampled with seed + 1 + k
    assert len(s1) == len(s2) == 20
    _frame_check(d3, ne[s1], ne[s2], r1 % 20, r2 % 20, 0.25, 0.0, 0.05, f"[{config} {precision} max_cells]")

    # (c) sampled latents, three draws, injected noise: banks assembled here from module.expected_expression per draw
    nf, ns = _noise_fn(dev), 3
    blocks = [[] for _ in range(ns)]
    for step, tensors, (B0, B1) in model._eval_minibatches(gi, bs, None):
        for smp in range(ns):
            with torch.no_grad():
                inf = model._infer(tensors, nf, step * ns + smp, B0, B1)
            blocks[smp].append(model.module.expected_expression(inf, g, genes=pos, library_size=1.0).cpu().numpy())
    draws = [np.concatenate(b)[: len(cells)] for b in blocks]
    bank1, bank2 = np.concatenate([d[p1] for d in draws]), np.concatenate([d[p2] for d in draws])   # row = draw * n_k + place in idx_k
    assert not np.array_equal(draws[0], draws[1])
    t1, t2 = rng.integers(0, len(bank1), n_pairs).astype(np.int32), rng.integers(0, len(bank2), n_pairs).astype(np.int32)
    d4 = model.differential_expression(gi, g, idx1, idx2, gene_list=pos, n_samples=ns, batch_size=bs, _noise=nf, _pair_rows=(t1, t2))
    _frame_check(d4, bank1, bank2, t1, t2, 0.25, 0.0, 0.05, f"[{config} {precision} n_samples=3]")

    # (d) errors
    other = gi[1 - g][0]
    with pytest.raises(ValueError, match=f"cell {other} "):
        model.differential_expression(gi, g, [int(idx1[0]), other], use_mean=True)
    with pytest.raises(ValueError, match="overlap"):
        model.differential_expression(gi, g, idx1, idx1[:3], use_mean=True)
    with pytest.raises(ValueError, match="empty"):
        model.differential_expression(gi, g, [], use_mean=True)
    with pytest.raises(ValueError, match="use_mean"):
        model.differential_expression(gi, g, idx1, n_samples=2, use_mean=True)
    with pytest.raises(ValueError, match="n_pairs"):
        model.differential_expression(gi, g, idx1, n_pairs=0)
    with pytest.raises(ValueError, match="group"):
        model.differential_expression(gi, 2, idx1)
    with pytest.raises(KeyError):
        model.differential_expression(gi, g, idx1, gene_list=[f"gene{(96, 0)[g]}"])   # a gene of the other group

    # (e) a model restored by save / load gives the same table bit for bit
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=adata())
    tab = back.differential_expression(gi, g, idx1, idx2, gene_list=names, use_mean=True, batch_size=bs, _pair_rows=(r1, r2))
    assert not back.module.training and tab.equals(df)


def test_planted_effect_is_found(dev):
    """half of group 0's cells carry counts with 50 genes multiplied by 8: those genes must look more different than the others
    (direction only: no threshold on the value)"""
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    ad = make_duck(n=(300, 260), seed=6)
    ad.X[:150, :50] *= 8
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32")
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=64, max_epochs=40, train_size=1.0, seed=0)
    df = model.differential_expression(gi, 0, list(range(150)), n_samples=2, n_pairs=5000, seed=1)
    assert df.index.tolist() == list(range(96))   # no names: positions
    planted, rest = float(df["proba_de"].to_numpy()[:50].mean()), float(df["proba_de"].to_numpy()[50:].mean())
    print(f"mean proba_de: planted genes {planted:.3f}, the other genes {rest:.3f}; mean lfc {df['lfc_mean'].to_numpy()[:50].mean():.3f} / {df['lfc_mean'].to_numpy()[50:].mean():.3f}")
    assert planted > rest
