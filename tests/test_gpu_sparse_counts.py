"""GPU: counts resident as CSR (ops.SparseGroupCounts), densified per minibatch by spv_csr_gather.  The kernel writes exactly the
bytes the dense-resident path hands the downstream kernels (counts, the log1p images of spv_prepare_log1p / _split, the library),
so training and embedding on CSR storage must be BIT-identical to the dense path: the kernel against the prepare entries, trainer
steps in both precisions at large (LDS-DMA) and small (pair-grid) shapes, with and without covariates, label and paired PoE, eager
and graph replay, the user API on a scipy.sparse AnnData, and the HBM the sparse storage holds."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _random_counts(dev, n, G, kind, seed):
    """[n][G] counts with empty rows, one fully dense row and (u16) values up to 65535, or fractional fp32 values"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    keep = torch.rand((n, G), device=dev, generator=gen) < 0.07
    if kind == "u16":
        v = torch.randint(1, 40, (n, G), device=dev, generator=gen).float()
        v[torch.rand((n, G), device=dev, generator=gen) < 0.002] = 65535.0
    else:
        v = torch.rand((n, G), device=dev, generator=gen) * 30.0 + 0.01
    X = torch.where(keep, v, torch.zeros_like(v))
    X[1] = 0.0                # empty rows
    X[n // 2] = 0.0
    X[2] = v[2]               # a fully dense row
    from spvipes_amd.ops import GroupCounts
    t = X.to(torch.int32).to(torch.int16) if kind == "u16" else X
    return GroupCounts(t.contiguous(), G, 0, resident=True)


def _gather(items, dev):
    """items: [(SparseGroupCounts, rows, split)] -> per item (X [B][ldx], image, library) from ONE spv_csr_gather call"""
    from spvipes_amd import _abi
    from spvipes_amd._abi import round_up
    args = (_abi.SpvCsrGatherArgs * len(items))()
    outs = []
    for a, (sc, rows, split) in zip(args, items):
        B, G = rows.numel(), sc.G
        ldx = round_up(G, 8)
        ldh = round_up(round_up(G, 96), 128)
        X = torch.full((B, ldx), -1, dtype=torch.float32 if sc.dtype == _abi.SPV_COUNT_F32 else torch.int16, device=dev)   # (poisoned)
        xb = torch.full((B, 2 * ldh if split else ldh), -1, dtype=torch.int16, device=dev)
        lib = torch.full((B,), float("nan"), device=dev)
        a.indptr, a.cols, a.vals, a.n_rows, a.G, a.dtype, a.B = sc.indptr.data_ptr(), sc.cols.data_ptr(), sc.vals.data_ptr(), sc.n_cells, G, sc.dtype, B
        a.rows, a.X, a.ldx, a.xb, a.ld_xb, a.xb_split, a.library = rows.data_ptr(), X.data_ptr(), ldx, xb.data_ptr(), xb.shape[1], split, lib.data_ptr()
        outs.append((X, xb, lib))
    _abi.call("spv_csr_gather", args, len(items), _abi.stream_ptr())
    torch.cuda.synchronize()
    return outs


def _check_against_dense(gc, sc, rows, split, X, xb, lib):
    G = gc.G
    r = rows.long()
    assert torch.equal(X[:, :G], gc.X[r][:, :G])
    assert bool((X[:, G:] == 0).all())
    want_xb, want_lib = gc.log1p_image_split() if split else gc.log1p_image()
    assert torch.equal(xb, want_xb[r]), "log1p image differs (padding included)"
    assert torch.equal(lib.view(torch.int32), want_lib[r].view(torch.int32)), "library differs"


@pytest.mark.parametrize("G", [1, 95, 2000, 10_000, 20_003])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_gather_matches_the_dense_prepare_entries_bitwise(dev, G, kind):
    from spvipes_amd.ops import SparseGroupCounts
    n = 64 if G >= 10_000 else 300
    gc = _random_counts(dev, n, G, kind, seed=G)
    sc = SparseGroupCounts.from_dense(gc)
    assert sc.nnz < n * G
    rng = np.random.default_rng(G)
    rows = torch.tensor(np.concatenate([[1, 2, n // 2, 2, n - 1], rng.integers(0, n, 40)]).astype(np.int32), device=dev)   # repeated, unordered
    for split in (0, 1):
        (X, xb, lib), = _gather([(sc, rows, split)], dev)
        _check_against_dense(gc, sc, rows, split, X, xb, lib)


def test_two_groups_of_different_shape_in_one_call(dev):
    from spvipes_amd.ops import SparseGroupCounts
    gcs = [_random_counts(dev, 200, 9000, "u16", 1), _random_counts(dev, 150, 130, "f32", 2)]
    scs = [SparseGroupCounts.from_dense(g) for g in gcs]
    rows = [torch.randint(0, 200, (77,), dtype=torch.int32, device=dev), torch.randint(0, 150, (190,), dtype=torch.int32, device=dev)]
    outs = _gather([(scs[0], rows[0], 0), (scs[1], rows[1], 1)], dev)
    for g, split in ((0, 0), (1, 1)):
        _check_against_dense(gcs[g], scs[g], rows[g], split, *outs[g])


def test_gather_rejects_bad_arguments(dev):
    from spvipes_amd import _abi
    from spvipes_amd.ops import SparseGroupCounts
    sc = SparseGroupCounts.from_dense(_random_counts(dev, 20, 50, "u16", 3))
    rows = torch.arange(4, dtype=torch.int32, device=dev)
    X = torch.zeros((4, 56), dtype=torch.int16, device=dev)
    xb = torch.zeros((4, 128), dtype=torch.int16, device=dev)
    lib = torch.zeros(4, device=dev)

    def call(**kw):
        a = _abi.SpvCsrGatherArgs(indptr=sc.indptr.data_ptr(), cols=sc.cols.data_ptr(), vals=sc.vals.data_ptr(), n_rows=20, G=50,
                                  dtype=_abi.SPV_COUNT_U16, B=4, rows=rows.data_ptr(), X=X.data_ptr(), ldx=56, xb=xb.data_ptr(), ld_xb=128,
                                  xb_split=0, library=lib.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return _abi.load().spv_csr_gather(C.byref(a), 1, None)

    assert call() == 0
    torch.cuda.synchronize()
    for bad in (dict(indptr=None), dict(rows=None), dict(X=None), dict(G=0), dict(B=0), dict(n_rows=0), dict(ldx=48), dict(ldx=52),
                dict(dtype=7), dict(ld_xb=40), dict(ld_xb=130), dict(xb_split=1, ld_xb=64), dict(library=None)):
        assert call(**bad) == -1, bad   # SPV_ERR_ARG


# ------------------------------------------------------------------------------------------------------------------------------------
# trainer steps: sparse == dense, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (precision, B, (G0, G1), H, n_batch, mode, decoder_slots)
    "large_bf16_label": ("bf16", 1024, (4500, 5000), 128, 1, "label", "narrow"),
    "large_fp32_label_cov": ("fp32", 1024, (4500, 5000), 128, 3, "label", "narrow"),
    "c1_bf16_label": ("bf16", 128, (2000, 2000), 64, 1, "label", "narrow"),
    "c1_fp32_paired": ("fp32", 128, (2000, 2000), 64, 1, "paired", "narrow"),
    "c1_bf16_wide_cov": ("bf16", 128, (2000, 1800), 64, 12, "label", "wide"),
    "large_bf16_paired_cov": ("bf16", 1024, (5000, 4200), 128, 4, "paired", "narrow"),
}


def _trainers(dev, case, cells=2048):
    from spvipes_amd.data import make_synthetic_group
    from spvipes_amd.module import spVIPESmodule
    from spvipes_amd.ops import SparseGroupCounts
    from spvipes_amd.train import Trainer
    precision, B, Gs, H, nb, mode, slots = CASES[case]
    groups = [make_synthetic_group(g, cells, Gs[g], dev) for g in range(2)]
    rng = np.random.default_rng(11)
    codes = [torch.tensor(rng.integers(0, nb, cells), dtype=torch.int32, device=dev) for _ in range(2)] if nb > 1 else None
    plan = torch.tensor((rng.random((cells, cells)) * (rng.random((cells, cells)) < 0.01)).astype(np.float32), device=dev) if mode == "paired" else None
    out = []
    for storage in ("dense", "sparse"):
        counts = [g.counts if storage == "dense" else SparseGroupCounts.from_dense(g.counts) for g in groups]
        torch.manual_seed(0)   # same initial parameters and generator key
        kw = dict(use_labels=True) if mode == "label" else dict(use_labels=False, transport_plan=plan, pair_data=True)
        module = spVIPESmodule({0: Gs[0], 1: Gs[1]}, n_batch=nb, n_hidden=H, n_dimensions_shared=25, n_dimensions_private=10,
                               precision=precision, decoder_slots=slots, **kw).to(dev)
        module.train()
        trainer = Trainer(module, counts, labels=[g.labels for g in groups] if mode == "label" else None, batch_codes=codes)
        out.append((module, trainer))
    batches = [[torch.tensor(rng.permutation(cells)[:B].astype(np.int32), device=dev) for _ in range(2)] for _ in range(4)]
    return out, batches


def _grads_by_name(module, trainer, grad):
    base = trainer.fp.flat.data_ptr()
    out = {}
    for name, p in module.named_parameters():
        off = (p.data_ptr() - base) // 4
        out[name] = grad[off:off + p.numel()]
    return out


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_training_steps_on_csr_storage_are_bit_identical(dev, case, use_graph):
    """label PoE: three steps, every loss, gradient, parameter and buffer bit for bit.  Paired PoE: its backward scatters into the
    partners' rows with atomics (many cells share an arg-max partner), so the encoders' gradients already differ in the last bits
    between two runs of the DENSE path; there the first step's loss and the decoders' gradients must agree bit for bit and every other
    gradient to the accuracy the atomics leave (relative norm of the difference over all of them; a near-cancelling bias gradient
    can differ in its leading digits between two dense runs)."""
    paired = CASES[case][5] == "paired"
    runs, batches = _trainers(dev, case)
    results = []
    n_steps = 1 if paired else 3
    for module, trainer in runs:
        torch.manual_seed(5)   # (the paired PoE draws its noise from torch's generator: the same stream for both runs)
        trainer._ensure_images()
        if use_graph:
            keep = {k: b.clone() for k, b in module.named_buffers()}
            trainer.capture(batches[3])
            with torch.no_grad():
                for k, b in module.named_buffers():
                    b.copy_(keep[k])
            assert trainer.graph is not None
        losses = []
        for i in range(n_steps):
            lo = trainer.step(batches[i], kl_weight=0.5 + 0.25 * i)
            torch.cuda.synchronize()
            losses.append(lo.loss.detach().clone())
        results.append((losses, trainer.fp.flat.clone(), trainer.fp.grad.clone(), {k: b.clone() for k, b in module.named_buffers()}))
    (l_d, p_d, g_d, b_d), (l_s, p_s, g_s, b_s) = results
    for i in range(n_steps):
        assert torch.equal(l_d[i].view(torch.int32), l_s[i].view(torch.int32)), (i, float(l_d[i]), float(l_s[i]))
    assert bool(torch.isfinite(p_d).all()) and bool(torch.isfinite(g_d).all())
    for k in b_d:
        assert torch.equal(b_d[k], b_s[k]), k
    if not paired:
        assert torch.equal(g_d.view(torch.int32), g_s.view(torch.int32)), "gradients differ"
        assert torch.equal(p_d.view(torch.int32), p_s.view(torch.int32)), "parameters differ"
        return
    gd, gs = _grads_by_name(runs[0][0], runs[0][1], g_d), _grads_by_name(runs[1][0], runs[1][1], g_s)
    dec = [n for n in gd if n.startswith("decoder")]
    assert dec
    for name in dec:
        assert torch.equal(gd[name].view(torch.int32), gs[name].view(torch.int32)), f"decoder gradient {name} differs"
    rest_d = torch.cat([gd[n] for n in gd if n not in dec])
    rest_s = torch.cat([gs[n] for n in gs if n not in dec])
    rel = float((rest_s - rest_d).norm()) / float(rest_d.norm())
    assert rel < 1e-2, f"encoder / dispersion gradients: relative difference {rel:.2e}"


# ------------------------------------------------------------------------------------------------------------------------------------
# user API
# ------------------------------------------------------------------------------------------------------------------------------------
def _sparse_duck(mode, seed=0):
    """a _duck-style AnnData whose groups' genes are interleaved columns of an outer-joined matrix"""
    import scipy.sparse as sp

    from tests._duck import make_duck
    n = (300, 300) if mode == "paired" else (300, 260)
    ad = make_duck(n=n, seed=seed, with_plan=(mode == "paired"))
    X = ad.X
    nv = X.shape[1]
    perm = np.random.default_rng(seed + 1).permutation(nv)    # scatter the columns: non-contiguous gene sets per group
    Xp = np.zeros_like(X)
    Xp[:, perm] = X
    ad.X = Xp
    ad.uns["groups_var_indices"] = [np.sort(perm[v]) for v in ad.uns["groups_var_indices"]]
    # (sorted columns keep each group's gene ORDER equal between the two layouts: compare against the same dense AnnData)
    dense = make_duck(n=n, seed=seed, with_plan=(mode == "paired"))
    dense.X = Xp.copy()
    dense.uns["groups_var_indices"] = [v.copy() for v in ad.uns["groups_var_indices"]]
    ad.X = sp.csr_matrix(Xp)
    return ad, dense


def _fit_and_embed(ad, mode, **kw):
    from spvipes_amd.model import spVIPES
    if mode == "label":
        spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type", **({"layer": kw.pop("layer")} if "layer" in kw else {}))
    else:
        spVIPES.setup_anndata(ad, groups_key="groups", transport_plan_key="plan", **({"layer": kw.pop("layer")} if "layer" in kw else {}))
    torch.manual_seed(3)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=6, n_dimensions_private=3, **kw)
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=64, max_epochs=2, train_size=0.9)
    return model, model.get_latent_representation(gi, batch_size=64), gi


def _same_latents(a, b):
    for k in ("shared", "private", "shared_reordered", "private_reordered"):
        for g in (0, 1):
            assert np.array_equal(a[k][g].view(np.int32), b[k][g].view(np.int32)), (k, g)


def _close_latents(a, b):
    for k in ("shared", "private", "shared_reordered", "private_reordered"):
        for g in (0, 1):
            np.testing.assert_allclose(a[k][g], b[k][g], rtol=1e-3, atol=1e-4, err_msg=f"{k}[{g}]")


@pytest.mark.parametrize("mode", ["label", "paired"])
def test_model_on_a_scipy_sparse_anndata_matches_dense_input(dev, mode, tmp_path):
    from spvipes_amd.model import spVIPES
    from spvipes_amd.ops import GroupCounts, SparseGroupCounts
    ad, dense = _sparse_duck(mode)
    m_s, z_s, gi = _fit_and_embed(ad, mode)
    m_d, z_d, _ = _fit_and_embed(dense, mode)
    assert all(isinstance(c, SparseGroupCounts) for c in m_s.counts) and all(isinstance(c, GroupCounts) for c in m_d.counts)
    assert m_s.init_params_["counts_storage"] == "auto"
    same = _same_latents if mode == "label" else _close_latents   # (paired: the PoE backward's atomics, see the trainer test)
    same(z_s, z_d)
    if mode == "label":
        for k, v in m_d.module.state_dict().items():
            assert torch.equal(v, m_s.module.state_dict()[k]), k
        assert m_s.history == m_d.history
    # save / load on the sparse AnnData rebuilds CSR storage and the same embedding (noise injected: log_z is a sample)
    m_s.save(str(tmp_path / "m"))
    back = spVIPES.load(str(tmp_path / "m"), adata=ad)
    assert back.init_params_["counts_storage"] == "auto"
    assert all(isinstance(c, SparseGroupCounts) for c in back.counts)
    zeros = lambda step, b0, b1: {**{f"enc_{g}_{k}": torch.zeros(b, d, device=dev) for g, b in ((0, b0), (1, b1)) for k, d in (("private", 3), ("shared", 6))},
                                  **{f"poe_{g}": torch.zeros(b, 6, device=dev) for g, b in ((0, b0), (1, b1))}}
    _same_latents(back.get_latent_representation(gi, batch_size=64, _noise=zeros), m_s.get_latent_representation(gi, batch_size=64, _noise=zeros))
    # the same parameters give the same embedding from either storage
    m_d.module.load_state_dict(m_s.module.state_dict())
    _same_latents(m_d.get_latent_representation(gi, batch_size=64, _noise=zeros), m_s.get_latent_representation(gi, batch_size=64, _noise=zeros))


def test_sparse_layer_and_storage_choices(dev):
    import scipy.sparse as sp

    from spvipes_amd.ops import GroupCounts, SparseGroupCounts
    ad, dense = _sparse_duck("label", seed=4)
    _, z_ref, _ = _fit_and_embed(dense, "label")
    # a sparse layer (X itself holds something else)
    lay, _ = _sparse_duck("label", seed=4)
    lay.layers["counts"] = lay.X
    lay.X = sp.csr_matrix(lay.X.shape, dtype=np.float32)
    m, z, _ = _fit_and_embed(lay, "label", layer="counts")
    assert all(isinstance(c, SparseGroupCounts) for c in m.counts)
    _same_latents(z, z_ref)
    # CSR storage of dense input, dense storage of sparse input
    d2, _ = _sparse_duck("label", seed=4)
    d2.X = d2.X.toarray()
    m, z, _ = _fit_and_embed(d2, "label", counts_storage="sparse")
    assert all(isinstance(c, SparseGroupCounts) for c in m.counts)
    _same_latents(z, z_ref)
    s2, _ = _sparse_duck("label", seed=4)
    m, z, _ = _fit_and_embed(s2, "label", counts_storage="dense")
    assert all(isinstance(c, GroupCounts) for c in m.counts)
    _same_latents(z, z_ref)


def test_sparse_storage_memory(dev):
    """two groups of 10 000 cells x 8 000 genes at 5 % density: construction and a training epoch on CSR storage take the CSR arrays and
    the [B][ld] minibatch buffers where the dense path holds its uint16 matrices and f16 images (2 x 10 000 x 8 000 x 4 B = 640 MB);
    everything else (parameters, optimiser state, step workspaces) is the same for both and is measured on the dense run"""
    import gc

    import scipy.sparse as sp

    from spvipes_amd._abi import round_up
    from spvipes_amd.model import spVIPES
    from spvipes_amd.ops import GroupCounts, SparseGroupCounts
    from tests._duck import DuckAnnData
    n, G, dens, B = 10_000, 8_000, 0.05, 256
    rng = np.random.default_rng(0)
    blocks = [sp.random(n, G, density=dens, format="csr", random_state=g, data_rvs=lambda k: rng.integers(1, 30, k)).astype(np.float32)
              for g in range(2)]
    X = sp.block_diag(blocks, format="csr")
    obs = {"groups": np.array(["a"] * n + ["b"] * n), "indices": np.concatenate([np.arange(n), np.arange(n)]).astype(np.int32),
           "cell_type": rng.integers(0, 4, 2 * n)}
    uns = {"groups_lengths": {0: G, 1: G}, "groups_var_indices": [np.arange(G), G + np.arange(G)],
           "groups_obs_indices": [np.arange(n), n + np.arange(n)], "groups_obs_names": None, "groups_var_names": None}
    gi = [list(range(n)), list(range(n, 2 * n))]
    peaks, counts_bytes = {}, {}
    for storage in ("auto", "dense"):
        ad = DuckAnnData(X, dict(obs), dict(uns))
        spVIPES.setup_anndata(ad, groups_key="groups", label_key="cell_type")
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        model = spVIPES(ad, n_hidden=128, n_dimensions_shared=25, n_dimensions_private=10, counts_storage=storage)
        model.train(gi, batch_size=B, max_epochs=1, train_size=1.0, use_graph=False)
        torch.cuda.synchronize()
        peaks[storage] = torch.cuda.max_memory_allocated() - base
        if storage == "auto":
            assert all(isinstance(c, SparseGroupCounts) for c in model.counts)
            assert sum(c.nnz for c in model.counts) == X.nnz
            counts_bytes[storage] = sum(c.nbytes for c in model.counts)
            assert counts_bytes[storage] <= X.nnz * 6 + 2 * (n + 1) * 8
        else:
            assert all(isinstance(c, GroupCounts) for c in model.counts)
            counts_bytes[storage] = sum(c.X.numel() * 2 + sum(t.numel() * t.element_size() for t in c.log1p_image()) for c in model.counts)
        del model, ad
    ld = round_up(round_up(G, 96), 128)
    minibatch = 2 * B * (round_up(G, 8) * 2 + ld * 2 + 4)    # counts + f16 image + library per group
    bound = peaks["dense"] - counts_bytes["dense"] + counts_bytes["auto"] + minibatch + 4 * 2**20
    assert counts_bytes["dense"] >= 640e6
    assert peaks["auto"] <= bound, f"CSR storage peak {peaks['auto'] / 2**20:.0f} MB, bound {bound / 2**20:.0f} MB (dense {peaks['dense'] / 2**20:.0f} MB)"
    assert peaks["auto"] < peaks["dense"] - 500e6
