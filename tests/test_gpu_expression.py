"""GPU: the denoised-expression read-out -- spv_dec_expected through dec_ops.expected_expression, spVIPESmodule.expected_expression
and spVIPES.get_normalized_expression -- against the reference's recorded decoder outputs (goldens), the CPU oracle at
kernel-relevant shapes, its own identities, and the user API on the duck AnnData.

The comparison bound (tests 1, 2, 3c-bf16) is derived from the bounds the project already holds the three ingredients to
(test_gpu_parity.py: rates (rtol_r, atol_r) = fp32 (2e-4, 1e-7), bf16 (3e-2, 1e-5); logits (rtol_l, atol_l) = fp32 (2e-4, 2e-4),
bf16 (2e-2, 3e-2)) with |d sigmoid| <= |d logit| / 4:
    |out - m| <= rtol_r * m + atol_r + 0.25 * (atol_l + rtol_l * |l|) * |rp - rs|          m = s * rp + (1 - s) * rs, s = sigmoid(l)
the two parts: m -> the part, |rp - rs| -> rp resp. rs;   pi: |out - s| <= 0.25 * (atol_l + rtol_l * |l|).   No element is excluded."""
import functools

import numpy as np
import pytest
import torch

from tests._golden import LOSS_CASES, Golden

pytestmark = pytest.mark.gpu

WIDE_CASES = ["wide/label_train_batch12", "wide/label_eval_batch14", "wide/paired_train_batch20", "wide/label_train_batch12_c1dims"]
RATE_TOL = {"fp32": (2e-4, 1e-7), "bf16": (3e-2, 1e-5)}
LOGIT_TOL = {"fp32": (2e-4, 2e-4), "bf16": (2e-2, 3e-2)}
WHATS = ("mixture", "private", "shared", "mixing")
EPS = 2.0 ** -24   # half an ulp of fp32, relative


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _reference_values(rp, rs, l):
    """float64 (m, part_p, part_s, pi) from reference rates and logits"""
    rp, rs, l = rp.double(), rs.double(), l.double()
    s = torch.sigmoid(l)
    return {"mixture": s * rp + (1 - s) * rs, "private": s * rp, "shared": (1 - s) * rs, "mixing": s}


def _bounds(rp, rs, l, precision):
    (rr, ar), (rl, al) = RATE_TOL[precision], LOGIT_TOL[precision]
    rp, rs, l = rp.double(), rs.double(), l.double()
    ref = _reference_values(rp, rs, l)
    dl = 0.25 * (al + rl * l.abs())
    return ref, {"mixture": rr * ref["mixture"] + ar + dl * (rp - rs).abs(), "private": rr * ref["private"] + ar + dl * rp,
                 "shared": rr * ref["shared"] + ar + dl * rs, "mixing": dl}


def _assert_within(out, ref, bound, what, ctx):
    err = (out.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"{ctx} {what}: max err {float(err.max()):.3e}, max err/bound {float((err / bound).max()):.3f}")
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    assert worst <= 0.0, f"{ctx} {what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst excess {worst:.3e}"


# ---- 1. against the reference's own numbers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", LOSS_CASES + WIDE_CASES)
def test_expected_expression_matches_reference_goldens(dev, case, precision, monkeypatch):
    from spvipes_amd import module as M
    from tests import test_gpu_parity as T
    if case in WIDE_CASES:   # modules that pick their decoder layout (the wide one for these shapes), as test_gpu_wide_covariates.py builds them
        monkeypatch.setattr(M, "spVIPESmodule", functools.partial(M.spVIPESmodule, decoder_slots="auto"))
    g = Golden(case)
    m, tensors, noise, dm = T._build(g, dev, precision)
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k}
    with torch.no_grad():
        inf = m.inference(**m._get_inference_input(tensors), noise=noise, dropout_masks=dm)
    before_dec = {k: v.clone() for k, v in m.state_dict().items() if "running" in k and "decoder" in k}
    for grp in range(2):
        ref, bound = _bounds(g.t(f"out/dec_{grp}/rate_private"), g.t(f"out/dec_{grp}/rate_shared"), g.t(f"out/dec_{grp}/mix_logits"), precision)
        for code, what in enumerate(WHATS):
            out = m.expected_expression(inf, grp, what=(what if code % 2 else code)).cpu()   # names and codes both reach the kernel
            _assert_within(out, ref[what], bound[what], what, f"{case} {precision} group {grp}")
    torch.cuda.synchronize()
    after = m.state_dict()
    for k, v in before_dec.items():
        assert torch.equal(after[k], v), f"the read-out moved {k}"
    assert m.training == g.training and set(before) == {k for k in after if "running" in k}


# ---- 2. at kernel-relevant shapes against the oracle ---------------------------------------------------------------------------
SHAPES = [  # cells, G0, G1, n_s, n_p, n_batch
    (512, 2000, 10003, 25, 10, 0),
    (512, 10000, 2000, 10, 5, 3),
    (4096, 10000, 2000, 25, 10, 12),
    (4096, 10003, 2000, 10, 5, 0),
    (4096, 2000, 10000, 25, 10, 3),
]


def _synthetic_module(dev, precision, B, Gs, n_s, n_p, nb, H=128, seed=0, cells=None):
    """an eval-mode module with moved BatchNorm statistics on synthetic resident counts + one minibatch of B arbitrary rows"""
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    cells = cells or B + 64
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    groups = [make_synthetic_group(g, cells, Gs[g], dev) for g in range(2)]
    module = spVIPESmodule({0: Gs[0], 1: Gs[1]}, use_labels=True, n_batch=max(nb, 1), n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=0.0, precision=precision, decoder_slots="auto").to(dev)
    gen = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        for k, v in module.state_dict().items():   # running statistics a trained model would hold
            if k.endswith("running_mean"):
                v.copy_((0.05 * torch.randn(v.shape, generator=gen)).to(dev))
            elif k.endswith("running_var"):
                v.copy_((0.75 + 0.5 * torch.rand(v.shape, generator=gen)).to(dev))
    module.eval()
    rows = [torch.tensor(rng.permutation(cells)[:B], dtype=torch.int32, device=dev) for _ in range(2)]
    codes = [torch.tensor(rng.integers(0, nb, size=cells), dtype=torch.int32, device=dev) for _ in range(2)] if nb > 1 else None
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen) for g in range(2) for k, n in (("private", n_p), ("shared", n_s))}
    noise.update({f"poe_{g}": torch.randn(B, n_s, generator=gen) for g in range(2)})
    tensors = tuple({"counts": groups[g].counts, "rows": rows[g], "indices": rows[g].float().unsqueeze(1), "groups": None,
                     "batch": None if codes is None else codes[g][rows[g].long()].unsqueeze(1),
                     "labels": groups[g].labels[rows[g].long()].unsqueeze(1)} for g in range(2))
    return module, groups, rows, codes, noise, tensors


@functools.lru_cache(maxsize=1)
def _oracle_decoder(shape):
    """the oracle's float64 decoder outputs of a SHAPES case (the module's initial state depends on the seed alone, not on the
    precision mode: both precisions are compared with one oracle run)"""
    from oracle import spvipes_oracle as O
    B, G0, G1, n_s, n_p, nb = shape
    dev = torch.device("cuda:0")
    module, groups, rows, codes, noise, _ = _synthetic_module(dev, "fp32", B, (G0, G1), n_s, n_p, nb)
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in module.state_dict().items()}
    counts = [torch.from_numpy(groups[g].counts.X[rows[g].long()].cpu().numpy().view(np.uint16).astype(np.float64)) for g in range(2)]
    kw = {} if nb <= 1 else {"n_batch": nb, "batch_index": [codes[g].cpu()[rows[g].cpu().long()] for g in range(2)]}
    with torch.no_grad():
        out = O.forward_loss(sd, counts, n_dimensions_shared=n_s, n_dimensions_private=n_p, noise={k: v.double() for k, v in noise.items()},
                             mode="label", labels=[groups[g].labels.cpu()[rows[g].cpu().long()] for g in range(2)], training=False, **kw)
    return out["decoder"]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{s[0]}-G{s[1]}x{s[2]}-s{s[3]}p{s[4]}-nb{s[5]}" for s in SHAPES])
def test_expected_expression_matches_oracle_at_size(dev, shape, precision):
    B, G0, G1, n_s, n_p, nb = shape
    want = _oracle_decoder(shape)
    module, _groups, _rows, _codes, noise, tensors = _synthetic_module(dev, precision, B, (G0, G1), n_s, n_p, nb)
    assert module.dec_slots.kslots == (1 if nb == 12 and n_s == 25 else 0)
    with torch.no_grad():
        inf = module.inference(**module._get_inference_input(tensors), noise={k: v.to(dev) for k, v in noise.items()})
    for grp in range(2):
        ref, bound = _bounds(*[t.to(dev) for t in want[grp]], precision)
        for what in WHATS:
            out = module.expected_expression(inf, grp, what=what)
            assert out.shape == (B, (G0, G1)[grp])
            _assert_within(out, ref[what], bound[what], what, f"{shape} {precision} group {grp}")


# ---- 3. identities -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("fp32", 0), ("bf16", 0), ("fp32", 12), ("bf16", 12)], ids=lambda p: f"{p[0]}-nb{p[1]}")
def ident(request, dev):
    """B = 200 (Bp = 256 > B), G = 1003 / 517 (multiples of nothing), narrow (no covariates) and wide (12 categories) layouts"""
    precision, nb = request.param
    module, _g, _r, _c, noise, tensors = _synthetic_module(dev, precision, 200, (1003, 517), 25, 10, nb, H=64, seed=3)
    with torch.no_grad():
        inf, gen = module(tensors, inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}}, compute_loss=False)
    mat = []
    for grp in range(2):
        e = gen["private_poe"][str(grp)]
        mat.append((e["px_rate_private"].clone(), e["px_rate_shared"].clone(), e["px"].mixture_logits.clone()))
    return precision, module, inf, mat, tensors, noise


def test_subset_equals_the_columns_of_the_all_genes_output_bit_for_bit(ident, dev):
    _p, module, inf, _mat, _t, _n = ident
    rng = np.random.default_rng(11)
    for grp in range(2):
        G = module.input_dims[grp]
        for what in WHATS:
            full = module.expected_expression(inf, grp, what=what)
            assert full.shape == (200, G)
            for n in (1, 31, 33, 257):
                sel = rng.integers(0, G, size=n)
                if n > 1:
                    sel[-1] = sel[0]   # a repeat for certain
                for genes in (sel, torch.tensor(sel, dtype=torch.int32, device=dev)):   # host list (checked) and device list
                    sub = module.expected_expression(inf, grp, what=what, genes=genes)
                    assert sub.shape == (200, n)
                    assert torch.equal(sub, full[:, torch.as_tensor(sel, device=dev).long()]), (grp, what, n)
    with pytest.raises(IndexError, match=str(module.input_dims[0])):
        module.expected_expression(inf, 0, genes=[0, module.input_dims[0]])


def test_parts_add_up_and_the_mean_is_a_convex_combination(ident):
    """The kernel forms the mean as ONE fp32 addition of the two rounded parts, so part 1 + part 2 (added in fp32 here) may differ
    from it by at most 1 ulp (stated bound; equality is expected); a convex combination of the two rates with weights that are each
    rounded to fp32 (pi + (1 - pi) within 1 +- 2^-23) and three more roundings stays within [min, max] * (1 -+ 4 * 2^-23)."""
    _p, module, inf, mat, _t, _n = ident
    for grp in range(2):
        w0, w1, w2 = (module.expected_expression(inf, grp, what=w) for w in (0, 1, 2))
        assert bool(((w1 + w2 - w0).abs() <= 2 * EPS * w0.abs()).all())
        rp, rs, _l = mat[grp]
        lo, hi = torch.minimum(rp, rs), torch.maximum(rp, rs)
        assert bool((w0 >= lo * (1 - 8 * EPS)).all()) and bool((w0 <= hi * (1 + 8 * EPS)).all())
        pi = module.expected_expression(inf, grp, what=3)
        assert bool(((pi >= 0) & (pi <= 1)).all())


def test_mean_agrees_with_the_materialised_arrays(ident):
    """fp32 mode: the rates are the same numbers and the logits the same fp32 accumulations as spv_dec_materialize's, so the only
    difference to the mixture formed from its arrays in float64 is the kernel's own combine: exp2(-|l| log2 e) (argument rounding
    |l| 2^-24 relative, the hardware exponential and reciprocal ~1 ulp each), two products and one sum, every term <= max(rp, rs):
    |out - m| <= (8 + |l|) * 2^-23 * max(rp, rs).  bf16 mode: the materialised logits have passed through f16 storage, the fused
    ones have not: the bound of test 1."""
    precision, module, inf, mat, _t, _n = ident
    for grp in range(2):
        rp, rs, l = mat[grp]
        out = module.expected_expression(inf, grp, what=0)
        if precision == "fp32":
            ref = _reference_values(rp, rs, l)["mixture"]
            bound = (8 + l.double().abs()) * 2 * EPS * torch.maximum(rp, rs).double()
        else:
            ref, bound = _bounds(rp, rs, l, precision)
            ref, bound = ref["mixture"], bound["mixture"]
        _assert_within(out, ref, bound, "mixture", f"vs materialize {precision} group {grp}")


def test_fixed_library_size_scales_the_output(ident):
    """library_size = L only moves a_k = log L - lse_k (rate = exp(y + a_k)), so the result is L times the library_size = 1 result up
    to rounding: a_k and the exponent's argument y + a_k are each rounded to fp32 once per call (four roundings in the comparison,
    each <= 2^-24 of a magnitude that stays below 16 here: lse_k ~ ln G ~ 7, ln L ~ 7, |y| of these decoders < 3), an absolute
    error of the argument being a relative one of the rate; plus ~8 ulps for the exponentials, log L and the products:
    relative bound (4 * 16 + 8) * 2^-24 on each part, and their sum (+ one addition) on the mean."""
    _p, module, inf, _mat, _t, _n = ident
    L, rtol = 1000.0, 72 * EPS
    for grp in range(2):
        one = [module.expected_expression(inf, grp, what=w, library_size=1).double() for w in range(4)]
        big = [module.expected_expression(inf, grp, what=w, library_size=L).double() for w in range(4)]
        assert torch.equal(one[3], big[3])   # the mixing weight does not see the library
        for k in (1, 2):
            assert bool(((big[k] - L * one[k]).abs() <= rtol * big[k]).all()), (grp, k)
        assert bool(((big[0] - L * one[0]).abs() <= (rtol + 2 * EPS) * big[0]).all()), grp
        latent = module.expected_expression(inf, grp, what=0).double()   # the model's own library: another scale per cell
        scale = latent.sum(1) / one[0].sum(1)
        assert bool(((latent - scale[:, None] * one[0]).abs() <= 1e-4 * latent).all())
    with pytest.raises(ValueError):
        module.expected_expression(inf, 0, library_size=0.0)
    with pytest.raises(ValueError):
        module.expected_expression(inf, 0, what="mean")


def test_padding_of_the_output_array_is_never_written(ident, dev):
    _p, module, inf, _mat, _t, _n = ident
    sel = np.arange(40, 40 + 77)
    for grp in range(2):
        want = module.expected_expression(inf, grp, genes=sel)
        buf = torch.full((256, 77 + 9), -7.25, device=dev)
        got = module.expected_expression(inf, grp, genes=sel, out=buf)
        assert got.data_ptr() == buf.data_ptr() and got.shape == (200, 77)
        assert torch.equal(buf[:200, :77], want)
        assert bool((buf[200:] == -7.25).all()) and bool((buf[:, 77:] == -7.25).all())
        wide = torch.full((200, 2048), -7.25, device=dev)   # all genes into a wider array
        module.expected_expression(inf, grp, out=wide)
        G = module.input_dims[grp]
        assert torch.equal(wide[:, :G], module.expected_expression(inf, grp)) and bool((wide[:, G:] == -7.25).all())


def test_accumulate_averages_draws_on_the_device(ident, dev):
    """out = sum_i fl(alpha * v_i) accumulated in fp32, alpha = fl(1 / n): against the float64 mean of n single calls the error is
    the rounding of alpha (2^-24 relative), one rounding per product or fused multiply-add and per addition: <= (2 n + 2) * 2^-24
    of sum_i |alpha v_i| = the mean itself (all values are positive)."""
    _p, module, _inf, _mat, tensors, noise = ident
    n = 3
    infs = []
    for i in range(n):
        gen = torch.Generator().manual_seed(100 + i)
        nz = {k: torch.randn(v.shape, generator=gen).to(dev) for k, v in noise.items()}
        with torch.no_grad():
            inf = module.inference(**module._get_inference_input(tensors), noise=nz)
        singles = [module.expected_expression(inf, g, genes=np.arange(3, 300)).double() for g in range(2)]
        infs.append((inf, singles))
        if i == 0:
            acc = [module.expected_expression(inf, g, genes=np.arange(3, 300), alpha=1.0 / n) for g in range(2)]
        else:
            for g in range(2):
                module.expected_expression(inf, g, genes=np.arange(3, 300), out=acc[g], alpha=1.0 / n, accumulate=True)
    for g in range(2):
        mean = sum(s[g] for _, s in infs) / n
        assert bool(((acc[g].double() - mean).abs() <= (2 * n + 2) * EPS * mean).all())
        assert not torch.equal(infs[0][1][g], infs[1][1][g])   # the draws differ
    with pytest.raises(ValueError):
        module.expected_expression(infs[0][0], 0, accumulate=True)


def test_abi_argument_errors_are_reported(ident, dev):
    """spv_dec_expected returns the ABI's negative status with a message for arguments it cannot take"""
    import ctypes as C
    from spvipes_amd import _abi, dec_ops
    _p, module, inf, _mat, _t, _n = ident
    lib = inf["library"][0]
    first, second, par = module._decoder_operands(0, inf["private_stats"][0]["log_z"], inf["poe_stats"][0]["logtheta_log_z"])
    o = dec_ops._prepare_decoder(module.decoders[0], module.px_r[0], first, second, lib, False, module.nsplit, module._workspace(0, dev), par, logits=False)
    out = torch.empty(200, 8, device=dev)

    def args(**kw):
        a = _abi.SpvDecExpectedArgs()
        a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo, a.K, a.nsplit = _abi.ptr(o.Am[0]), _abi.ptr(o.Am[1]), _abi.ptr(o.Wm[0]), _abi.ptr(o.Wm[1]), 320, module.nsplit
        a.genes, a.n_genes, a.what, a.out, a.ld_out, a.alpha, a.accumulate = None, 8, 0, _abi.ptr(out), 8, 1.0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    _abi.call("spv_dec_expected", C.byref(o.p), C.byref(args()), _abi.stream_ptr())   # the good call
    for bad in (dict(what=4), dict(what=-1), dict(n_genes=0), dict(n_genes=module.input_dims[0] + 1), dict(ld_out=7), dict(K=300), dict(K=352),
                dict(nsplit=2), dict(out=None), dict(Wm_hi=None)):
        with pytest.raises(_abi.SpvError, match="spv_dec_expected"):
            _abi.call("spv_dec_expected", C.byref(o.p), C.byref(args(**bad)), _abi.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_narrower_operand_width_gives_the_same_bits(dev, precision):
    """K < 320 takes the kernel's rolled logits loop (dec_ops always packs 320 columns: the unrolled one).  No batch covariates, 10 shared
    and 5 private dimensions: the mixture input is 256 + 5 + 10 + 1 = 272 columns wide, so columns 288..319 of every operand image
    hold zero bits (asserted: the 320-wide contraction relies on that padding), and a call with K = 288 on contiguous 288-column
    copies adds the same products in the same step order less exact zeros: equal bit for bit.  B = 200, G = 1003 / 517; 45 selected
    genes are two tiles, the second partial."""
    import ctypes as C
    from spvipes_amd import _abi, dec_ops
    module, _g, _r, _c, noise, tensors = _synthetic_module(dev, precision, 200, (1003, 517), 10, 5, 0, H=64, seed=3)
    with torch.no_grad():
        inf = module.inference(**module._get_inference_input(tensors), noise={k: v.to(dev) for k, v in noise.items()})
    for grp in range(2):
        first, second, par = module._decoder_operands(grp, inf["private_stats"][grp]["log_z"], inf["poe_stats"][grp]["logtheta_log_z"])
        o = dec_ops._prepare_decoder(module.decoders[grp], module.px_r[grp], first, second, inf["library"][grp], False, module.nsplit,
                                     module._workspace(grp, dev), par, logits=False)
        wide = [*o.Am, *o.Wm]
        assert [t is not None for t in wide] == [True, precision == "fp32"] * 2
        for t in wide:
            assert t is None or (t.dtype == torch.int16 and t.shape[1] == 320 and not bool(t[:, 288:].any()))
        narrow = [None if t is None else t[:, :288].contiguous() for t in wide]
        sel = torch.tensor(np.random.default_rng(5).integers(0, module.input_dims[grp], size=45), dtype=torch.int32, device=dev)

        def run(images, K, what):
            out = torch.full((200, 45), -7.25, device=dev)
            a = _abi.SpvDecExpectedArgs()
            a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo, a.K, a.nsplit = *[_abi.ptr(t) for t in images], K, module.nsplit
            a.genes, a.n_genes, a.what, a.out, a.ld_out, a.alpha, a.accumulate = _abi.ptr(sel), 45, what, _abi.ptr(out), 45, 1.0, 0
            _abi.call("spv_dec_expected", C.byref(o.p), C.byref(a), _abi.stream_ptr())
            return out

        for what in range(4):
            want = run(wide, 320, what)
            assert bool((want >= 0).all()) and torch.equal(run(narrow, 288, what), want), (grp, what)


# ---- 4. user API ---------------------------------------------------------------------------------------------------------------
def _noise_fn(dev, n_s=10, n_p=5):
    def noise(draw, b0, b1):
        g = torch.Generator(device="cpu").manual_seed(1000 + draw)
        mk = lambda b, n: torch.randn(b, n, generator=g).to(dev)
        return {"enc_0_private": mk(b0, n_p), "enc_0_shared": mk(b0, n_s), "enc_1_private": mk(b1, n_p), "enc_1_shared": mk(b1, n_s),
                "poe_0": mk(b0, n_s), "poe_1": mk(b1, n_s)}
    return noise


@pytest.mark.parametrize("config", ["label", "paired", "batch_key", "sparse"])
def test_get_normalized_expression(dev, tmp_path, config):
    from spvipes_amd import dec_ops
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
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision="fp32",
                    counts_storage=("sparse" if config == "sparse" else "auto"))
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)   # moves parameters and BatchNorm running statistics
    bs = 64 if config != "paired" else 32
    n, G = [len(g) for g in gi], [96, 80]
    model.module.train()   # the call must put the module into eval mode and restore this
    buffers = {k: v.clone() for k, v in model.module.state_dict().items() if "running" in k or "num_batches" in k}

    full = model.get_normalized_expression(gi, batch_size=bs)
    assert model.module.training
    for k, v in model.module.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), f"{k} changed"
    for g in range(2):
        assert isinstance(full[g], np.ndarray) and full[g].dtype == np.float32 and full[g].shape == (n[g], G[g])
        assert np.isfinite(full[g]).all() and (full[g] >= 0).all()
    again = model.get_normalized_expression(gi, batch_size=bs)
    for g in range(2):
        np.testing.assert_array_equal(full[g], again[g])   # posterior means: deterministic

    # gene lists: positions == names == the columns of the all-genes result; per-group mix with None
    pos = [np.array([5, 0, 95, 5, 17]), np.array([79, 3])]
    names = [[f"gene{i}" for i in pos[0]], [f"gene{96 + i}" for i in pos[1]]]
    by_pos = model.get_normalized_expression(gi, gene_list=pos, batch_size=bs)
    by_name = model.get_normalized_expression(gi, gene_list=names, batch_size=bs)
    mixed = model.get_normalized_expression(gi, gene_list=[None, names[1]], batch_size=bs, return_numpy=False)
    for g in range(2):
        assert by_pos[g].shape == (n[g], len(pos[g]))
        np.testing.assert_array_equal(by_pos[g], by_name[g])
        np.testing.assert_array_equal(by_pos[g], full[g][:, pos[g]])
    assert mixed[0].is_cuda and mixed[0].shape == (n[0], G[0]) and mixed[1].shape == (n[1], 2)
    np.testing.assert_array_equal(mixed[0].cpu().numpy(), full[0])
    np.testing.assert_array_equal(mixed[1].cpu().numpy(), by_pos[1])
    with pytest.raises(KeyError, match="gene96"):
        model.get_normalized_expression(gi, gene_list=[["gene96"], None])   # a gene of the other group
    with pytest.raises(IndexError, match="80"):
        model.get_normalized_expression(gi, gene_list=[None, [80]])
    with pytest.raises(ValueError):
        model.get_normalized_expression(gi, n_samples=2)
    with pytest.raises(ValueError):
        model.get_normalized_expression(gi, component="rate")
    with pytest.raises(ValueError):
        model.get_normalized_expression(gi, library_size=-1.0)

    # rows: re-decode batch by batch through the module and compare exactly
    model.module.eval()
    for comp in ("mixture", "shared"):
        got = model.get_normalized_expression(gi, gene_list=pos, component=comp, batch_size=bs)
        blocks = {0: [], 1: []}
        for step, tensors, (B0, B1) in model._eval_minibatches(gi, bs, None):
            with torch.no_grad():
                inf = model._infer(tensors, None, step, B0, B1)
            for g in range(2):
                blocks[g].append(model.module.expected_expression(inf, g, genes=pos[g], what=comp, use_mean=True).cpu().numpy())
        for g in range(2):
            np.testing.assert_array_equal(got[g], np.concatenate(blocks[g])[:n[g]])
    # ... and independently of the walking code: decode the per-cell latents get_latent_representation returns (same injected
    # draws) in ONE batch per group with a fixed library size.  Eval-mode BatchNorm makes every row its own computation; only the
    # order of the softmax denominator's partial sums depends on the batch size, so the comparison is to 1e-5, which no
    # misplaced row survives.
    if config != "batch_key":
        nf = _noise_fn(dev)
        smp = model.get_normalized_expression(gi, use_mean=False, library_size=50.0, batch_size=bs, _noise=nf)
        lat = model.get_latent_representation(gi, batch_size=bs, _noise=nf)
        for g in range(2):
            z_p, z_s = (torch.tensor(lat[k][g], device=dev) for k in ("private", "shared"))
            one = dec_ops.expected_expression(model.module.decoders[g], model.module.px_r[g], z_p, z_s, torch.zeros(n[g], device=dev), False,
                                              model.module.nsplit, model.module._workspace(g, dev), library_size=50.0)
            np.testing.assert_allclose(smp[g], one.cpu().numpy(), rtol=1e-5, atol=1e-9)
            assert not np.allclose(smp[g][:-1], smp[g][1:], rtol=1e-3)   # rows differ: the check above can see a shift

    # n_samples: the device-side average of injected draws equals the mean of single-draw calls
    nf = _noise_fn(dev)
    avg = model.get_normalized_expression(gi, gene_list=pos, use_mean=False, n_samples=3, batch_size=bs, _noise=nf)
    singles = [model.get_normalized_expression(gi, gene_list=pos, use_mean=False, batch_size=bs, _noise=(lambda d, b0, b1, s=s: nf(3 * d + s, b0, b1)))
               for s in range(3)]
    for g in range(2):
        mean = sum(s[g].astype(np.float64) for s in singles) / 3
        assert (np.abs(avg[g] - mean) <= 8 * EPS * mean).all()
        assert not np.array_equal(singles[0][g], singles[1][g])

    # a model restored by save / load gives the same numbers
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=adata())
    again = back.get_normalized_expression(gi, gene_list=names, batch_size=bs)
    assert not back.module.training
    for g in range(2):
        np.testing.assert_array_equal(again[g], by_pos[g])
