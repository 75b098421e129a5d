"""GPU: posterior-predictive counts -- spv_dec_sample through dec_ops.sample_counts, spVIPESmodule.sample_counts and
spVIPES.posterior_predictive_sample: the structure of the output bit for bit, its moments against the project's own expected-expression
read-outs (float64), and the user API on the duck AnnData.  Every test here needs the feature and fails without it.

Shapes: B = 70 cells (three 32-cell workgroups, the last one partial), G = 70 / 83 genes and a 45-gene selection with repeats (partial
32-gene tiles), bf16 and fp32 modes, and one wide-layout case (12 batch categories, 25 shared dimensions: KW = 2).  The libraries spread
over a factor of 10 between cells and px_r over [-2, 3] between genes, so a transposed or shifted tile changes the moments."""
import math

import numpy as np
import pytest
import torch

from tests import _nb_sampling_check as S

pytestmark = pytest.mark.gpu

B, GS, NSEL, NS = 70, (70, 83), 45, 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _synthetic_module(dev, precision, Bn, Gs, n_s, n_p, nb, H=64, seed=3):
    """an eval-mode module with moved BatchNorm statistics on synthetic resident counts + one minibatch of Bn arbitrary rows (the helper
    of tests/test_gpu_expression.py), with px_r spread over [-2, 3]"""
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    cells = Bn + 64
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
        for g in range(2):
            module.px_r[g].copy_(torch.linspace(-2.0, 3.0, Gs[g])[torch.randperm(Gs[g], generator=gen)].to(dev))
    module.eval()
    rows = [torch.tensor(rng.permutation(cells)[:Bn], dtype=torch.int32, device=dev) for _ in range(2)]
    codes = [torch.tensor(rng.integers(0, nb, size=cells), dtype=torch.int32, device=dev) for _ in range(2)] if nb > 1 else None
    noise = {f"enc_{g}_{k}": torch.randn(Bn, n, generator=gen) for g in range(2) for k, n in (("private", n_p), ("shared", n_s))}
    noise.update({f"poe_{g}": torch.randn(Bn, n_s, generator=gen) for g in range(2)})
    tensors = tuple({"counts": groups[g].counts, "rows": rows[g], "indices": rows[g].float().unsqueeze(1), "groups": None,
                     "batch": None if codes is None else codes[g][rows[g].long()].unsqueeze(1),
                     "labels": groups[g].labels[rows[g].long()].unsqueeze(1)} for g in range(2))
    return module, noise, tensors


class _Case:
    pass


@pytest.fixture(scope="module", params=[("fp32", 0), ("bf16", 0), ("fp32", 12)], ids=lambda p: f"{p[0]}-nb{p[1]}")
def case(request, dev):
    """the module, one inference output whose libraries are replaced by log-uniform values over a factor of 10, the 45-gene selections,
    and -- computed ONCE, from the existing expected_expression read-outs in float64 -- every element's rates, pi, theta, mean and variance"""
    precision, nb = request.param
    c = _Case()
    c.precision, c.wide = precision, nb == 12
    c.module, noise, tensors = _synthetic_module(dev, precision, B, GS, 25 if nb else 10, 10 if nb else 5, nb)
    assert c.module.dec_slots.kslots == (1 if c.wide else 0)
    with torch.no_grad():
        c.inf, _gen = c.module(tensors, inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}}, compute_loss=False)
    gl = torch.Generator().manual_seed(17)
    c.inf = dict(c.inf)
    c.inf["library"] = {g: (math.log(300.0) + math.log(10.0) * torch.rand(B, 1, generator=gl)).to(dev) for g in range(2)}
    rng = np.random.default_rng(5)
    c.sel = []
    for g in range(2):
        s = rng.integers(0, GS[g], size=NSEL)
        s[-1], s[7] = s[0], s[0]   # repeats for certain, one of them in the partial second tile
        c.sel.append(s)
    c.par = []
    for g in range(2):
        part_p, part_s, pi = (c.module.expected_expression(c.inf, g, what=w).double().cpu().numpy() for w in ("private", "shared", "mixing"))
        assert 0.05 <= pi.min() and pi.max() <= 0.95, (pi.min(), pi.max())
        theta = torch.exp(c.module.px_r[g].detach().double()).cpu().numpy()[None, :]
        mp, ms = part_p / pi, part_s / (1.0 - pi)
        m = part_p + part_s
        second = pi * (mp + mp * mp * (1.0 + 1.0 / theta)) + (1.0 - pi) * (ms + ms * ms * (1.0 + 1.0 / theta))
        c.par.append(dict(mp=mp, ms=ms, pi=pi, theta=np.broadcast_to(theta, m.shape), m=m, v=second - m * m))
        lib = c.inf["library"][g].flatten()
        assert float(lib.max() - lib.min()) > math.log(8.0)
    return c


def _ids(dev, n=B, off=0):
    return (torch.arange(n, device=dev) + off).int()


# ---- structure, bit for bit ----------------------------------------------------------------------------------------------------------
def test_subset_and_repeated_genes_equal_the_columns_of_the_all_genes_output(case, dev):
    m = case.module
    for g in range(2):
        full = m.sample_counts(case.inf, g, key=21, sample=3)
        assert full.shape == (B, GS[g]) and full.dtype == torch.int32 and int(full.min()) >= 0 and int(full.max()) > 0
        assert torch.equal(full, m.sample_counts(case.inf, g, key=21, sample=3))                       # repeat calls are identical
        assert torch.equal(full, m.sample_counts(case.inf, g, key=21, sample=3, cell_ids=_ids(dev)))   # null cell_ids = the row number
        assert not torch.equal(full, m.sample_counts(case.inf, g, key=21, sample=4))
        assert not torch.equal(full, m.sample_counts(case.inf, g, key=22, sample=3))
        assert not torch.equal(full, m.sample_counts(case.inf, g, key=21, sample=3, cell_ids=_ids(dev, off=B)))
        sel = case.sel[g]
        for genes in (sel, torch.tensor(sel, dtype=torch.int32, device=dev)):   # host list (checked) and device list
            sub = m.sample_counts(case.inf, g, key=21, sample=3, genes=genes)
            assert sub.shape == (B, NSEL)
            assert torch.equal(sub, full[:, torch.as_tensor(sel, device=dev).long()])
            assert torch.equal(sub[:, 0], sub[:, -1]) and torch.equal(sub[:, 0], sub[:, 7])
        one = m.sample_counts(case.inf, g, key=21, sample=3, genes=[int(sel[3])])
        assert torch.equal(one[:, 0], full[:, int(sel[3])])
    with pytest.raises(IndexError, match=str(GS[0])):
        m.sample_counts(case.inf, 0, genes=[0, GS[0]])
    with pytest.raises(ValueError):
        m.sample_counts(case.inf, 0, sample=-1)
    with pytest.raises(ValueError):
        m.sample_counts(case.inf, 0, key=1 << 64)
    with pytest.raises(ValueError):
        m.sample_counts(case.inf, 0, library_size=0.0)


def test_padding_and_the_elements_between_the_gene_strides_are_never_written(case, dev):
    m, SENT = case.module, -77
    for g in range(2):
        sel = case.sel[g]
        want = m.sample_counts(case.inf, g, key=8, sample=1, genes=sel)
        buf = torch.full((96, NSEL + 9), SENT, dtype=torch.int32, device=dev)
        got = m.sample_counts(case.inf, g, key=8, sample=1, genes=sel, out=buf)
        assert got.data_ptr() == buf.data_ptr() and got.shape == (B, NSEL)
        assert torch.equal(buf[:B, :NSEL], want)
        assert bool((buf[B:] == SENT).all()) and bool((buf[:, NSEL:] == SENT).all())
        cube = torch.full((B + 2, NSEL + 1, 3), SENT, dtype=torch.int32, device=dev)   # [B][n][S] filled at sample 1 only
        m.sample_counts(case.inf, g, key=8, sample=1, genes=sel, out=cube[:, :, 1])
        assert torch.equal(cube[:B, :NSEL, 1], want)
        assert bool((cube[:, :, 0] == SENT).all()) and bool((cube[:, :, 2] == SENT).all())
        assert bool((cube[B:] == SENT).all()) and bool((cube[:, NSEL:] == SENT).all())
        with pytest.raises(Exception, match="sample_counts"):
            m.sample_counts(case.inf, g, genes=sel, out=torch.empty(B, NSEL, device=dev))   # an fp32 array


def test_filling_a_sample_cube_in_place_equals_separate_calls(case, dev):
    m, n_s = case.module, 5
    for g in range(2):
        cube = torch.empty((B, GS[g], n_s), dtype=torch.int32, device=dev)
        for s in range(n_s):
            m.sample_counts(case.inf, g, key=4, sample=s, out=cube[:, :, s])
        for s in range(n_s):
            assert torch.equal(cube[:, :, s], m.sample_counts(case.inf, g, key=4, sample=s)), (g, s)
        assert not torch.equal(cube[:, :, 0], cube[:, :, 1])


def test_draws_equal_the_elementwise_sampler_on_the_materialised_parameters(dev):
    """fp32 mode: the rates spv_dec_materialize writes are the numbers the fused kernels form, its logits the same fp32 accumulations, and
    theta the same exp(px_r): spv_nbmix_sample on those arrays, gene id = column, gives spv_dec_sample's counts bit for bit.  (Not stated
    for bf16 mode: there the materialised logits have passed through f16 storage, the fused ones have not.)"""
    from spvipes_amd.dec_ops import nbmix_sample
    for nb in (0, 12):
        module, noise, tensors = _synthetic_module(dev, "fp32", B, GS, 25 if nb else 10, 10 if nb else 5, nb)
        with torch.no_grad():
            inf, gen = module(tensors, inference_kwargs={"noise": {k: v.to(dev) for k, v in noise.items()}}, compute_loss=False)
        for g in range(2):
            e = gen["private_poe"][str(g)]
            rp, rs, lg = (t.float().contiguous() for t in (e["px_rate_private"], e["px_rate_shared"], e["px"].mixture_logits))
            theta = torch.exp(module.px_r[g].detach().float()).contiguous()
            ids = _ids(dev, off=1000)
            want = nbmix_sample(rp, rs, lg, theta, key=77, sample=2, cell_ids=ids)
            got = module.sample_counts(inf, g, key=77, sample=2, cell_ids=ids)
            assert torch.equal(got, want), (nb, g, int((got != want).sum()))


# ---- moments ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cubes(case, dev):
    """S = 256 samples of the fixed latents per group: only the count draw varies.  int64 [B, G, S] on the host."""
    out = []
    for g in range(2):
        cube = torch.empty((B, GS[g], NS), dtype=torch.int32, device=dev)
        for s in range(NS):
            case.module.sample_counts(case.inf, g, key=0xC0FFEE, sample=s, cell_ids=_ids(dev, off=500), out=cube[:, :, s])
        out.append(cube.cpu().numpy().astype(np.int64))
    return out


def test_sums_of_the_draws_are_within_six_sigma_of_the_model_means(case, cubes):
    """x(b, g, s) are independent with mean m(b, g) and variance v(b, g) (float64, from the expected-expression read-outs and exp(px_r)):
    |sum (x - m)| <= 6 sqrt(sum v) pooled over everything, per gene over cells and samples, and per cell over genes and samples."""
    for g in range(2):
        m, v = case.par[g]["m"], case.par[g]["v"]
        d = cubes[g].sum(2) - NS * m          # [B, G]: sums over the samples
        var = NS * v
        pooled = abs(d.sum()) / (6.0 * math.sqrt(var.sum()))
        per_gene = np.abs(d.sum(0)) / (6.0 * np.sqrt(var.sum(0)))
        per_cell = np.abs(d.sum(1)) / (6.0 * np.sqrt(var.sum(1)))
        print(f"group {g}: pooled {pooled:.3f}, worst gene {per_gene.max():.3f}, worst cell {per_cell.max():.3f} (each must be <= 1)")
        assert pooled <= 1.0
        assert per_gene.max() <= 1.0, int(per_gene.argmax())
        assert per_cell.max() <= 1.0, int(per_cell.argmax())


def test_pooled_variance_of_the_draws_on_a_gene_subset(case, cubes):
    """sum over cells, 16 genes and samples of ((x - m)^2 - v) has variance S * sum (mu4 - v^2), mu4 the fourth central moment from the
    element's pmf table (which also reproduces m and v): |sum| <= 6 sqrt of it."""
    for g in range(2):
        genes = np.arange(3, GS[g], GS[g] // 16)[:16]
        P = case.par[g]
        tot, var = 0.0, 0.0
        for b in range(B):
            for j in genes:
                p = S.pmf_table(P["mp"][b, j], P["ms"][b, j], P["theta"][b, j], P["pi"][b, j])
                m, v, mu4 = S.moments(p)
                assert abs(m - P["m"][b, j]) <= 1e-7 * m and abs(v - P["v"][b, j]) <= 1e-6 * v
                x = cubes[g][b, j].astype(np.float64)
                tot += float(((x - m) ** 2 - v).sum())
                var += NS * (mu4 - v * v)
        ratio = abs(tot) / (6.0 * math.sqrt(var))
        print(f"group {g}: pooled variance ratio {ratio:.3f} (must be <= 1)")
        assert ratio <= 1.0


# ---- the operand width ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_narrower_operand_width_gives_the_same_draws(dev, precision):
    """K < 320 takes the kernel's rolled logits loop (dec_ops always packs 320 columns: the unrolled one).  No batch covariates, 10 shared
    and 5 private dimensions: the mixture input is 256 + 5 + 10 + 1 = 272 columns wide, so columns 288..319 of every operand image
    hold zero bits (asserted: the 320-wide contraction relies on that padding), and a call with K = 288 on contiguous 288-column
    copies adds the same products in the same step order less exact zeros: the same logits, so the same draws.  B = 200, G = 1003 /
    517; 45 selected genes are two tiles, the second partial."""
    import ctypes as C
    from spvipes_amd import _abi, dec_ops
    Bn, Gs = 200, (1003, 517)
    module, noise, tensors = _synthetic_module(dev, precision, Bn, Gs, 10, 5, 0)
    with torch.no_grad():
        inf = module.inference(**module._get_inference_input(tensors), noise={k: v.to(dev) for k, v in noise.items()})
    for g in range(2):
        first, second, par = module._decoder_operands(g, inf["private_stats"][g]["log_z"], inf["poe_stats"][g]["logtheta_log_z"])
        o = dec_ops._prepare_decoder(module.decoders[g], module.px_r[g], first, second, inf["library"][g], False, module.nsplit,
                                     module._workspace(g, dev), par, logits=False)
        wide = [*o.Am, *o.Wm]
        assert [t is not None for t in wide] == [True, precision == "fp32"] * 2
        for t in wide:
            assert t is None or (t.dtype == torch.int16 and t.shape[1] == 320 and not bool(t[:, 288:].any()))
        narrow = [None if t is None else t[:, :288].contiguous() for t in wide]
        sel = torch.tensor(np.random.default_rng(5).integers(0, Gs[g], size=NSEL), dtype=torch.int32, device=dev)
        theta = torch.exp(module.px_r[g].detach().float()).contiguous()

        def run(images, K):
            out = torch.full((Bn, NSEL), -77, dtype=torch.int32, device=dev)
            a = _abi.SpvDecSampleArgs()
            a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo, a.K, a.nsplit = *[_abi.ptr(t) for t in images], K, module.nsplit
            a.genes, a.n_genes, a.ld_gene, a.theta, a.cell_ids, a.key, a.sample = _abi.ptr(sel), NSEL, 1, _abi.ptr(theta), None, 0x5EED, 2
            a.out, a.ld_out = _abi.ptr(out), NSEL
            _abi.call("spv_dec_sample", C.byref(o.p), C.byref(a), _abi.stream_ptr())
            return out

        want = run(wide, 320)
        assert int(want.min()) >= 0 and int(want.max()) > 0 and torch.equal(run(narrow, 288), want), g


# ---- the ABI's argument errors -------------------------------------------------------------------------------------------------------
def test_abi_argument_errors_are_reported(case, dev):
    import ctypes as C
    from spvipes_amd import _abi, dec_ops
    module, inf = case.module, case.inf
    lib = inf["library"][0]
    first, second, par = module._decoder_operands(0, inf["private_stats"][0]["log_z"], inf["poe_stats"][0]["logtheta_log_z"])
    o = dec_ops._prepare_decoder(module.decoders[0], module.px_r[0], first, second, lib, False, module.nsplit, module._workspace(0, dev), par, logits=False)
    out = torch.empty(B, 8, dtype=torch.int32, device=dev)
    theta = torch.exp(module.px_r[0].detach().float()).contiguous()

    def args(**kw):
        a = _abi.SpvDecSampleArgs()
        a.Am_hi, a.Am_lo, a.Wm_hi, a.Wm_lo, a.K, a.nsplit = _abi.ptr(o.Am[0]), _abi.ptr(o.Am[1]), _abi.ptr(o.Wm[0]), _abi.ptr(o.Wm[1]), 320, module.nsplit
        a.genes, a.n_genes, a.ld_gene, a.theta, a.cell_ids, a.key, a.sample, a.out, a.ld_out = None, 8, 1, _abi.ptr(theta), None, 1, 0, _abi.ptr(out), 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    _abi.call("spv_dec_sample", C.byref(o.p), C.byref(args()), _abi.stream_ptr())   # the good call
    for bad in (dict(n_genes=0), dict(n_genes=GS[0] + 1), dict(ld_out=7), dict(ld_gene=0), dict(ld_gene=2), dict(K=300), dict(K=352), dict(nsplit=2),
                dict(out=None), dict(Wm_hi=None), dict(theta=None)):
        with pytest.raises(_abi.SpvError, match="spv_dec_sample"):
            _abi.call("spv_dec_sample", C.byref(o.p), C.byref(args(**bad)), _abi.stream_ptr())
    torch.cuda.synchronize()


# ---- user API --------------------------------------------------------------------------------------------------------------------------
def _noise_fn(dev, n_s=10, n_p=5):
    def noise(draw, b0, b1):
        g = torch.Generator(device="cpu").manual_seed(1000 + draw)
        mk = lambda b, n: torch.randn(b, n, generator=g).to(dev)
        return {"enc_0_private": mk(b0, n_p), "enc_0_shared": mk(b0, n_s), "enc_1_private": mk(b1, n_p), "enc_1_shared": mk(b1, n_s),
                "poe_0": mk(b0, n_s), "poe_1": mk(b1, n_s)}
    return noise


@pytest.mark.parametrize("config", ["label-fp32", "paired-bf16"])
def test_posterior_predictive_sample(dev, tmp_path, config):
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    paired = config.startswith("paired")

    def adata():
        ad = make_duck(n=(96, 70) if paired else (150, 110), seed=2, with_plan=paired)   # n0 != n1, ragged last batches
        ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
        return ad

    ad = adata()
    spVIPES.setup_anndata(ad, groups_key="groups", **({"transport_plan_key": "plan"} if paired else {"label_key": "cell_type"}))
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=config.split("-")[1])
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    bs, n, G, nf = 32, [len(g) for g in gi], [96, 80], _noise_fn(dev)
    model.module.train()   # the call must put the module into eval mode and restore this

    full = model.posterior_predictive_sample(gi, batch_size=bs, seed=3, _noise=nf)
    assert model.module.training
    lat = model.get_latent_representation(gi, batch_size=bs, _noise=nf)
    for g in range(2):
        assert isinstance(full[g], np.ndarray) and full[g].dtype == np.int32 and full[g].shape == (n[g], G[g])
        assert full[g].shape[0] == lat["shared"][g].shape[0] and full[g].min() >= 0 and full[g].max() > 0
    again = model.posterior_predictive_sample(gi, batch_size=bs, seed=3, _noise=nf)
    other = model.posterior_predictive_sample(gi, batch_size=bs, seed=4, _noise=nf)
    for g in range(2):
        np.testing.assert_array_equal(full[g], again[g])   # same seed, same injected latents
        assert not np.array_equal(full[g], other[g])

    # gene lists and the 3-d layout; sample 0 of a 3-sample call is the 1-sample call on the same latents
    pos = [np.array([5, 0, 95, 5, 17]), np.array([79, 3])]
    names = [[f"gene{i}" for i in pos[0]], [f"gene{96 + i}" for i in pos[1]]]
    by_pos = model.posterior_predictive_sample(gi, gene_list=pos, batch_size=bs, seed=3, _noise=nf)
    by_name = model.posterior_predictive_sample(gi, gene_list=names, batch_size=bs, seed=3, _noise=nf, return_numpy=False)
    three = model.posterior_predictive_sample(gi, n_samples=3, gene_list=pos, batch_size=bs, seed=3, _noise=(lambda d, b0, b1: nf(d // 3, b0, b1) if d % 3 == 0 else nf(5000 + d, b0, b1)))
    for g in range(2):
        np.testing.assert_array_equal(by_pos[g], full[g][:, pos[g]])
        assert by_name[g].is_cuda and by_name[g].dtype == torch.int32
        np.testing.assert_array_equal(by_name[g].cpu().numpy(), by_pos[g])
        assert three[g].shape == (n[g], len(pos[g]), 3) and three[g].dtype == np.int32
        np.testing.assert_array_equal(three[g][:, :, 0], by_pos[g])
        assert not np.array_equal(three[g][:, :, 1], three[g][:, :, 2])
    with pytest.raises(KeyError, match="gene96"):
        model.posterior_predictive_sample(gi, gene_list=[["gene96"], None])
    with pytest.raises(ValueError):
        model.posterior_predictive_sample(gi, n_samples=0)

    # rows: re-walk the minibatches through the module with the adata row numbers as cell ids and compare exactly
    from spvipes_amd.dec_ops import sample_key
    model.module.eval()
    blocks = {0: [], 1: []}
    for step, tensors, (B0, B1) in model._eval_minibatches(gi, bs, None):
        with torch.no_grad():
            inf = model._infer(tensors, nf, step, B0, B1)
        for g in range(2):
            ids = torch.as_tensor(np.asarray(ad.uns["groups_obs_indices"][g]), device=dev)[tensors[g]["rows"].long()].int()
            blocks[g].append(model.module.sample_counts(inf, g, genes=pos[g], key=sample_key(3), sample=0, cell_ids=ids).cpu().numpy())
    for g in range(2):
        np.testing.assert_array_equal(by_pos[g], np.concatenate(blocks[g])[:n[g]])

    # ... and independently of the walking code: decode the per-cell latents get_latent_representation returns (same injected draws) in ONE
    # batch per group, rows in the order of ``gi``, cell ids = the adata rows of ``gi``, at a fixed library size.  Eval-mode BatchNorm makes
    # every row its own computation and pi, theta and the Gamma draw do not see the batch; only the order of the softmax denominator's
    # partial sums depends on the batch size, which moves a rate by at most delta = 1e-5 relative (the bound test_gpu_expression.py holds
    # the same two routes to).  The inversion's CDF boundaries move by delta * lam * pmf(k), so an element's count differs with probability
    # <= delta * lam; the rates sum to 50 over 96 / 80 genes (mean lam 0.6, lam >= 10 is rare), i.e. < 1e-5 per element and < 0.2 expected
    # over a group's elements: at most 5 in all (Poisson(0.2) exceeds 5 with probability 1e-10) and 2 in a row, while two different cells' rows
    # differ in far more than 2 places, so no misplaced row survives.
    from spvipes_amd import dec_ops
    fixed_lib = model.posterior_predictive_sample(gi, library_size=50.0, batch_size=bs, seed=3, _noise=nf)
    for g in range(2):
        z_p, z_s = (torch.tensor(lat[k][g], device=dev) for k in ("private", "shared"))
        one = dec_ops.sample_counts(model.module.decoders[g], model.module.px_r[g], z_p, z_s, torch.zeros(n[g], device=dev), False, model.module.nsplit,
                                    model.module._workspace(g, dev), library_size=50.0, key=sample_key(3), sample=0,
                                    cell_ids=torch.tensor(np.asarray(gi[g]), dtype=torch.int32, device=dev)).cpu().numpy()
        differ = fixed_lib[g] != one
        print(f"{config} group {g}: {int(differ.sum())} of {differ.size} counts differ from the one-batch decode, worst row {int(differ.sum(1).max())}")
        assert differ.sum() <= 5 and differ.sum(1).max() <= 2
        assert (fixed_lib[g][:-1] != fixed_lib[g][1:]).sum(1).min() > 2   # neighbouring rows differ: the check above can see a shift

    # zero fractions of a 64-sample draw of 2 genes against the model's own P(x = 0), latents held fixed over the samples:
    # P0 = pi (theta / (theta + mu_p))^theta + (1 - pi) (theta / (theta + mu_s))^theta per (cell, gene); the number of zeros over cells and
    # samples is a sum of independent Bernoulli(P0): |zeros - 64 sum P0| <= 6 sqrt(64 sum P0 (1 - P0))
    two = [np.array([0, 41]), np.array([0, 33])]
    fixed = lambda d, b0, b1: nf(d // 64, b0, b1)
    x = model.posterior_predictive_sample(gi, n_samples=64, gene_list=two, batch_size=bs, seed=9, _noise=fixed)
    comp = {w: model.get_normalized_expression(gi, gene_list=two, component=w, use_mean=False, batch_size=bs, _noise=nf) for w in ("private", "shared", "mixing")}
    for g in range(2):
        pi = comp["mixing"][g].astype(np.float64)
        mp, ms = comp["private"][g] / pi, comp["shared"][g] / (1.0 - pi)
        th = np.exp(model.module.px_r[g].detach().double().cpu().numpy())[two[g]][None, :]
        p0 = pi * (th / (th + mp)) ** th + (1.0 - pi) * (th / (th + ms)) ** th
        zeros = (x[g] == 0).sum()
        ratio = abs(zeros - 64.0 * p0.sum()) / (6.0 * math.sqrt(64.0 * (p0 * (1.0 - p0)).sum()))
        print(f"{config} group {g}: zero fraction {zeros / x[g].size:.4f}, model {p0.mean():.4f}, ratio {ratio:.3f}")
        assert x[g].shape == (n[g], 2, 64) and ratio <= 1.0

    # a model restored by save / load draws the same counts
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=adata())
    again = back.posterior_predictive_sample(gi, gene_list=names, batch_size=bs, seed=3, _noise=nf)
    assert not back.module.training
    for g in range(2):
        np.testing.assert_array_equal(again[g], by_pos[g])
