"""GPU: the wide decoder operand layout (spVIPESmodule(decoder_slots="wide" | "auto"): regressor K slots 32 / 64, operand images
[.][96]), which takes more batch-covariate categories than the narrow 16 / 32 slots (n_batch <= 14 at 25 / 10 latents, where the
narrow layout stops at 5).  The training path against the oracle in both precision modes (at n_batch 12 the mixing trunk's input
is wider than spv_trunk_fold's 48 columns: the unfused trunk path runs with covariates), pair grids against per-group launches,
graph replay against eager steps, and the user API."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _setup(dev, precision, B, Gs, H, n_s, n_p, nb, cells=1024, seed=0, slots="wide", overlap=None):
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.train import Trainer
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    groups = [make_synthetic_group(g, cells, Gs[g], dev) for g in range(2)]
    codes = [torch.tensor(rng.integers(0, nb, size=cells), dtype=torch.int32, device=dev) for _ in range(2)]
    module = spVIPESmodule({0: Gs[0], 1: Gs[1]}, use_labels=True, n_batch=nb, n_hidden=H, n_dimensions_shared=n_s, n_dimensions_private=n_p,
                           dropout_rate=0.0, precision=precision, decoder_slots=slots).to(dev)
    with torch.no_grad():   # covariate weights large enough to matter
        for g in range(2):
            for kind in ("private", "shared"):
                module.encoders[g][kind].fc1.weight[:, Gs[g]:].normal_(0.0, 0.3)
    module.train()
    trainer = Trainer(module, [g.counts for g in groups], labels=[g.labels for g in groups], batch_codes=codes, lr=1e-3, overlap_allreduce=overlap)
    rows = [torch.tensor(rng.permutation(cells)[:B], dtype=torch.int32, device=dev) for _ in range(2)]
    gen = torch.Generator().manual_seed(seed + 1)
    noise = {f"enc_{g}_{k}": torch.randn(B, n, generator=gen) for g in range(2) for k, n in (("private", n_p), ("shared", n_s))}
    noise.update({f"poe_{g}": torch.randn(B, n_s, generator=gen) for g in range(2)})
    return module, trainer, groups, codes, rows, noise


def _oracle(module, groups, codes, rows, noise, n_s, n_p, nb, kl_weight, dtype=torch.float64):
    from oracle import spvipes_oracle as O
    sd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in module.state_dict().items()}
    for k in O.param_names(sd):
        sd[k].requires_grad_(True)
    counts = [torch.from_numpy(groups[g].counts.X[rows[g].long()].cpu().numpy().view(np.uint16).astype(np.float64)).to(dtype) for g in range(2)]
    out = O.forward_loss(sd, counts, n_dimensions_shared=n_s, n_dimensions_private=n_p, noise={k: v.to(dtype) for k, v in noise.items()},
                         mode="label", labels=[groups[g].labels.cpu()[rows[g].cpu().long()] for g in range(2)], training=True, kl_weight=kl_weight,
                         n_batch=nb, batch_index=[codes[g].cpu()[rows[g].cpu().long()] for g in range(2)])
    out["loss"].backward()
    return sd, out


def _check_step(dev, precision, B, Gs, H, n_s, n_p, nb, seed=0):
    module, trainer, groups, codes, rows, noise = _setup(dev, precision, B, Gs, H, n_s, n_p, nb, seed=seed)
    assert module.dec_slots.kslots == 1
    trainer.fp.grad.fill_(float("nan"))   # every gradient element, covariate columns included, must be overwritten by the step
    lo = trainer._forward_backward(rows, torch.full((), 0.7, device=dev), noise={k: v.to(dev) for k, v in noise.items()})
    inf, _gen = trainer.last_outputs
    torch.cuda.synchronize()
    sd, want = _oracle(module, groups, codes, rows, noise, n_s, n_p, nb, 0.7)
    for k, p in module.named_parameters():
        assert bool(torch.isfinite(p.grad).all()), f"gradient of {k} was not (fully) written"
    ltol, lat_tol, gtol = (2e-5, 2e-4, 5e-3) if precision == "fp32" else (1e-3, 5e-3, 6e-2)
    assert abs(float(lo.loss.detach()) - float(want["loss"].detach())) / abs(float(want["loss"].detach())) < ltol
    for g in range(2):
        for key in ("private_stats", "shared_stats"):
            a, b = inf[key][g]["logtheta_loc"].detach().cpu().double(), want[key][g]["logtheta_loc"].detach()
            assert float((a - b).abs().max()) < lat_tol * max(1.0, float(b.abs().max())), (key, g)
    gmax = max(float(sd[k].grad.abs().max()) for k, _ in module.named_parameters() if sd[k].grad is not None)
    for k, p in module.named_parameters():
        ref = sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])
        mine = p.grad.detach().cpu().double()
        if precision == "fp32":
            err = float((mine - ref).abs().max())
            assert err < gtol * float(ref.abs().max()) + gtol * 2e-2 * gmax, f"{precision} grad {k}: {err:.3e} (max {float(ref.abs().max()):.3e})"
        else:
            err, nrm = float((mine - ref).norm()), float(ref.norm())
            assert err < 8e-2 * nrm + 1e-3 * gmax, f"{precision} grad {k}: L2 err {err:.3e} of {nrm:.3e}"
    for g in range(2):   # the covariate columns of the regressors carry signal
        for reg in (module.decoders[g].factor_regressor_private, module.decoders[g].factor_regressor_shared):
            assert float(reg.linear.weight.grad[:, -nb:].abs().max()) > 0


@pytest.mark.parametrize("precision,B,Gs,H,n_s,n_p,nb,seed", [
    ("fp32", 96, (130, 111), 16, 25, 10, 12, 0),     # small step: pair grids, single-tile splits
    # LDS-DMA shapes.  (Seed 0 draws data with one encoder ReLU pre-activation at 9e-7 of its layer's largest: fp32 mode's split-bf16 fc1
    # puts it on the other side of the kink, and that unit's weight-gradient row -- a different, equally valid subgradient -- differs from
    # the float64 oracle's by 13 % of the gradient's max.  The narrow layout gives the same bits there: it is not a decoder matter.)
    ("fp32", 256, (700, 650), 128, 25, 10, 12, 1),
    ("bf16", 256, (700, 650), 128, 25, 10, 12, 0),
    ("fp32", 256, (700, 650), 128, 25, 10, 14, 0),   # exactly at the mixture GEMM's 320 columns
    ("bf16", 256, (700, 650), 128, 6, 3, 20, 0),     # only the private regressor needs the wide slots
])
def test_wide_training_step_matches_the_oracle(dev, precision, B, Gs, H, n_s, n_p, nb, seed):
    _check_step(dev, precision, B, Gs, H, n_s, n_p, nb, seed=seed)


def test_wide_large_step_matches_the_oracle(dev):
    """the likelihood kernel's real gene splits and the BatchNorm fold at K > 32 (25 + 12 shared columns)"""
    _check_step(dev, "fp32", 1024, (10000, 9000), 128, 25, 10, 12, seed=2)


def _run_steps(dev, precision, mode, monkeypatch, use_graph=False, steps=3):
    from spvipes_amd import ops
    from spvipes_amd.data import MinibatchSampler
    monkeypatch.setattr(ops, "DEC_PAIR", mode)
    B, cells = 128, 512
    module, trainer, groups, codes, rows, noise = _setup(dev, precision, B, (300, 280), 32, 25, 10, 12, cells=cells, seed=5)
    sampler = MinibatchSampler([cells, cells], B, dev, seed=1)
    batches = [r for r in sampler.epoch()][:steps]
    if use_graph:
        trainer.capture(batches[0], warmup=1)
    losses = [float(trainer.step(r, kl_weight=1.0).loss.detach()) for r in batches]
    torch.cuda.synchronize()
    return losses, trainer.fp.flat.clone()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_wide_pair_grids_give_the_bits_of_the_per_group_launches(dev, precision, monkeypatch):
    (la, fa), (lb, fb) = (_run_steps(dev, precision, m, monkeypatch) for m in ("0", "1"))
    assert la == lb
    assert bool((fa == fb).all())


def test_wide_graph_replay_equals_eager_steps(dev, monkeypatch):
    from spvipes_amd import ops
    (la, fa), (lb, fb) = (_run_steps(dev, "bf16", ops.DEC_PAIR, monkeypatch, use_graph=g, steps=4) for g in (False, True))
    assert la == lb
    assert bool((fa == fb).all())


def test_user_api_with_twelve_categories(dev, tmp_path):
    """setup_anndata(batch_key=...) with 12 categories: the user-facing model picks the wide layout itself (decoder_slots="auto"),
    trains, and save / load rebuild the same layout and the same latents"""
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck
    ad = make_duck()
    rng = np.random.default_rng(4)
    ad.obs["donor"] = rng.choice(np.array([f"d{i}" for i in range(12)]), size=ad.n_obs)
    spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type", batch_key="donor")
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=25, n_dimensions_private=10, precision="fp32")
    assert model.module.n_batch == 12 and model.module.dec_slots.kslots == 1
    assert model.init_params_["decoder_slots"] == "auto"
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=64, max_epochs=6, train_size=1.0, n_epochs_kl_warmup=None, plan_kwargs={"lr": 5e-3})
    h = model.history["train_loss"]
    assert len(h) == 6 and all(np.isfinite(h)) and h[-1] < h[0], h

    def latents(m):
        noise = lambda step, b0, b1: {**{f"enc_{g}_{k}": torch.randn(b, n, generator=torch.Generator().manual_seed(7 * step + g)).to(dev)
                                         for g, b in ((0, b0), (1, b1)) for k, n in (("private", 10), ("shared", 25))},
                                      **{f"poe_{g}": torch.randn(b, 25, generator=torch.Generator().manual_seed(99 + step + g)).to(dev) for g, b in ((0, b0), (1, b1))}}
        return m.get_latent_representation(gi, batch_size=64, _noise=noise)

    a = latents(model)
    model.save(str(tmp_path / "m"))
    m2 = spVIPES.load(str(tmp_path / "m"), ad)
    assert m2.module.dec_slots.kslots == 1
    b = latents(m2)
    for kind in ("shared", "private"):
        for g in range(2):
            np.testing.assert_array_equal(a[kind][g], b[kind][g])


@pytest.mark.parametrize("graph", [False, True])
def test_wide_split_backward_overwrites_and_equals_the_single_pass(dev, graph):
    """the split backward pass of a data-parallel job (see test_gpu_batch_covariates.py) in the wide layout: NaN-filled buffer, every
    element overwritten and equal to the one-pass step's gradient"""
    from spvipes_amd.data import MinibatchSampler

    def run(overlap, use_graph):
        module, trainer, groups, codes, rows, noise = _setup(dev, "bf16", 256, (640, 600), 128, 25, 10, 12, cells=1024, seed=7, overlap=overlap)
        assert trainer.overlap == overlap and module.dec_slots.kslots == 1
        rows = next(iter(MinibatchSampler([1024, 1024], 256, dev, seed=2).epoch()))
        if use_graph:
            trainer.capture(rows, warmup=1)
        trainer.fp.grad.fill_(float("nan"))
        trainer.step(rows, kl_weight=0.7, optimizer_step=False)
        torch.cuda.synchronize()
        bad = [(n_, int(torch.isnan(p.grad).sum())) for n_, p in module.named_parameters() if p.grad is not None and bool(torch.isnan(p.grad).any())]
        assert not bad, bad
        return trainer.fp.grad.clone(), {n_: p.grad.clone() for n_, p in module.named_parameters()}

    flat_one, by_name_one = run(False, False)
    flat_split, by_name_split = run(True, graph)
    for n_ in by_name_one:
        assert torch.equal(by_name_one[n_], by_name_split[n_]), n_
    assert torch.equal(torch.nan_to_num(flat_one), torch.nan_to_num(flat_split))


@pytest.mark.parametrize("nb,slots,want", [(3, "narrow", 0), (3, "auto", 0), (12, "auto", 1)])
def test_decoder_fills_the_kslots_fields_it_launches_with(dev, monkeypatch, nb, slots, want):
    """the spv_dec_params / spv_zsplit_args / spv_fold_batch structures the decoder op actually passes carry the module's layout
    (0 for every narrow module)"""
    from spvipes_amd import _abi, ops
    monkeypatch.setattr(ops, "DEC_PAIR", "0")   # (per-group launches: the structures go out one by one)
    real, seen = _abi.call, {}

    def spy(name, *args):
        for a in args:
            obj = getattr(a, "_obj", a)
            if isinstance(obj, (_abi.SpvDecParams, _abi.SpvZsplitArgs, _abi.SpvFoldBatch)):
                seen.setdefault(type(obj).__name__, set()).add(int(obj.kslots))
        return real(name, *args)

    monkeypatch.setattr(_abi, "call", spy)
    module, trainer, groups, codes, rows, noise = _setup(dev, "bf16", 128, (300, 280), 32, 25, 10, nb, cells=512, slots=slots)
    trainer._forward_backward(rows, torch.full((), 1.0, device=dev), noise={k: v.to(dev) for k, v in noise.items()})
    torch.cuda.synchronize()
    assert seen == {"SpvDecParams": {want}, "SpvZsplitArgs": {want}, "SpvFoldBatch": {want}}, seen


# ---- the reference's own runs of wide-layout shapes (tests/golden/wide/*.npz, tests/golden/make_wide_goldens.py) -----------------
WIDE_CASES = ["wide/label_train_batch12", "wide/label_eval_batch14", "wide/paired_train_batch20", "wide/label_train_batch12_c1dims"]


def _auto_modules(monkeypatch):
    """test_gpu_parity's fixture builder, with modules that pick their decoder layout ("auto": the wide one for these shapes)"""
    import functools
    from spvipes_amd import module as M
    monkeypatch.setattr(M, "spVIPESmodule", functools.partial(M.spVIPESmodule, decoder_slots="auto"))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", WIDE_CASES)
def test_module_matches_wide_reference_goldens(dev, case, precision, monkeypatch):
    """test_gpu_parity.py's golden checks (loss, latents, and in fp32 mode reconstruction, KL, every gradient, BatchNorm statistics),
    plus, in bf16 mode, reconstruction, KL and gradients at 16-bit-operand tolerances"""
    from tests import test_gpu_parity as T
    from tests._golden import Golden
    _auto_modules(monkeypatch)
    T.test_module_matches_reference_goldens(dev, case, precision)
    if precision != "bf16":
        return
    g = Golden(case)
    m, tensors, noise, dm = T._build(g, dev, precision)
    assert m.dec_slots.kslots == 1
    _inf, _gen, lo = m(tensors, inference_kwargs={"noise": noise, "dropout_masks": dm}, loss_kwargs={"kl_weight": g.kl_weight})
    lo.loss.backward()
    torch.cuda.synchronize()
    names = ["reconst_loss_groups_1_poe", "reconst_loss_groups_2_poe"]
    for grp in range(2):
        torch.testing.assert_close(lo.reconstruction_loss[names[grp]].detach().cpu(), g.t(f"out/rec_{grp}"), rtol=5e-3, atol=5e-2)
    torch.testing.assert_close(lo.kl_local["kl_divergence_groups_1_poe"].detach().cpu(), g.t("out/kl_poe_0"), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lo.kl_local["kl_divergence_groups_2_private"].detach().cpu(), g.t("out/kl_private_1"), rtol=2e-2, atol=2e-2)
    ref_g = g.grads()
    gmax = max(float(v.abs().max()) for v in ref_g.values())
    for k, p in m.named_parameters():   # relative L2 per parameter (the bf16 measure of test_gpu_fullsize_parity.py)
        mine = (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().double()
        ref = ref_g[k].double()
        err, nrm = float((mine - ref).norm()), float(ref.norm())
        assert err < 8e-2 * nrm + 2e-3 * gmax, f"{case} bf16 grad {k}: L2 err {err:.3e} of {nrm:.3e}"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("case", WIDE_CASES)
def test_generative_outputs_match_wide_reference_goldens(dev, case, precision, monkeypatch):
    """the materialising path (spv_dec_materialize, the fold in both BatchNorm modes) in the wide layout"""
    from tests import test_gpu_parity as T
    _auto_modules(monkeypatch)
    T.test_generative_outputs_match_reference_goldens(dev, case, precision)
