"""GPU: the user API around the exact lfc median -- ``spVIPES.differential_expression_median`` (differential_expression with the
column lfc_median) and ``spVIPES.differential_expression_by`` (every label of a column against the rest, from ONE decode walk).

The median is held to the float64 median of the host banks the public read-out returns, within the per-term bound ``tol`` of
tests/test_gpu_de.py restated in tests/test_gpu_de_median.py (an order statistic is 1-Lipschitz in the sup norm; the mean of two of
them is too).  Everything else is equality bit for bit: with the other columns of the frame without the median, and of every label's
block with the single two-population call it replaces.

``differential_expression`` itself keeps its parameter list (tests/test_de_host_cpu.py pins it), so the switch ``lfc_median`` lives on
``differential_expression_median``, which takes the same arguments."""
import numpy as np
import pytest
import torch

from tests.test_gpu_de_median import _tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _noise_fn(dev, n_s=10, n_p=5):
    def noise(draw, b0, b1):
        g = torch.Generator(device="cpu").manual_seed(1000 + draw)
        mk = lambda b, n: torch.randn(b, n, generator=g).to(dev)
        return {"enc_0_private": mk(b0, n_p), "enc_0_shared": mk(b0, n_s), "enc_1_private": mk(b1, n_p), "enc_1_shared": mk(b1, n_s),
                "poe_0": mk(b0, n_s), "poe_1": mk(b1, n_s)}
    return noise


def _same_frames(a, b, cols, ctx):
    for c in cols:
        x, y = a[c].to_numpy(), b[c].to_numpy()
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8) if x.dtype != bool else x, y.view(np.uint8) if y.dtype != bool else y), f"{ctx}: column {c} differs"


@pytest.mark.parametrize("config,precision", [("label", "fp32"), ("label", "bf16"), ("paired", "fp32"), ("paired", "bf16")])
def test_median_and_by_label(dev, tmp_path, config, precision):
    from spvipes_amd.data import DE_COLUMNS
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    def adata():
        ad = make_duck(n=(96, 70) if config == "paired" else (300, 260), seed=2, with_plan=(config == "paired"))
        ad.var_names = np.array([f"gene{i}" for i in range(ad.n_vars)])
        return ad

    ad = adata()
    kw = {"transport_plan_key": "plan"} if config == "paired" else {"label_key": "cell_type"}
    spVIPES.setup_anndata(ad, groups_key="groups", **kw)
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=10, n_dimensions_private=5, precision=precision)
    gi = [list(ad.uns["groups_obs_indices"][0]), list(ad.uns["groups_obs_indices"][1])]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)
    bs = 64 if config != "paired" else 32
    g = 1 if config == "paired" else 0
    G, off = (96, 80)[g], (0, 96)[g]
    cells = np.asarray(gi[g])
    ctx = f"[{config} {precision}]"

    # ---- (a) the lfc_median column of the two-population call ----------------------------------------------------------------
    rng = np.random.default_rng(5)
    idx1 = cells[rng.permutation(len(cells))[: len(cells) // 3]]
    rest = np.setdiff1d(cells, idx1)
    idx2 = rest[rng.permutation(len(rest))[: len(rest) // 2]]
    pos = np.array([5, 0, G - 1, 5, 17, 33, 2, 70])
    where = {c: i for i, c in enumerate(cells.tolist())}
    p1, p2 = (np.array([where[c] for c in idx.tolist()]) for idx in (idx1, idx2))
    n_pairs = 3000   # even: the two middle elements differ
    r1, r2 = rng.integers(0, len(p1), n_pairs).astype(np.int32), rng.integers(0, len(p2), n_pairs).astype(np.int32)
    gl = [None, None]
    gl[g] = pos
    model.module.train()   # the call must put the module into eval mode and restore this
    med = model.differential_expression_median(gi, g, idx1, idx2, gene_list=pos, use_mean=True, batch_size=bs, _pair_rows=(r1, r2))
    assert model.module.training
    plain = model.differential_expression(gi, g, idx1, idx2, gene_list=pos, use_mean=True, batch_size=bs, _pair_rows=(r1, r2))
    off_ = model.differential_expression_median(gi, g, idx1, idx2, gene_list=pos, use_mean=True, batch_size=bs, lfc_median=False, _pair_rows=(r1, r2))
    assert list(plain.columns) == list(DE_COLUMNS) + ["is_de_fdr_0.05"] and list(off_.columns) == list(plain.columns)
    cols = list(DE_COLUMNS)
    cols.insert(cols.index("lfc_mean") + 1, "lfc_median")
    assert list(med.columns) == cols + ["is_de_fdr_0.05"] and med.index.tolist() == plain.index.tolist() == [f"gene{off + i}" for i in pos]
    _same_frames(med, plain, plain.columns, ctx)   # every other column, bit for bit
    _same_frames(off_, plain, plain.columns, ctx)
    ne = model.get_normalized_expression(gi, gene_list=gl, library_size=1.0, batch_size=bs)[g]
    bank1, bank2 = ne[p1], ne[p2]
    tol, _L = _tol(bank1, bank2, len(pos), 0.0)
    d = np.log2(np.maximum(bank1[r1].astype(np.float64), np.finfo(np.float32).tiny)) - np.log2(np.maximum(bank2[r2].astype(np.float64), np.finfo(np.float32).tiny))
    want = np.median(d, axis=0)
    got = med["lfc_median"].to_numpy()
    assert got.dtype == np.float64
    err = np.abs(got - want)
    print(f"{ctx} lfc_median: max err {float(err.max()):.3e}, max err / bound {float(err.max()) / tol:.3f} (tol {tol:.3e})")
    assert float(err.max()) <= tol
    assert (med["lfc_min"].to_numpy().astype(np.float64) <= got).all() and (got <= med["lfc_max"].to_numpy().astype(np.float64)).all()

    # ---- (b) every label against the rest ------------------------------------------------------------------------------------
    model.module.eval()
    lab = np.asarray(ad.obs["cell_type"])[cells]
    names = np.unique(lab)
    assert len(names) >= 3
    seed, kwargs = 4, dict(gene_list=pos, use_mean=True, n_pairs=2000, delta=0.1, batch_size=bs)
    by = model.differential_expression_by(gi, g, "cell_type", seed=seed, **kwargs)
    assert not model.module.training
    numeric = cols + ["is_de_fdr_0.05"]
    assert list(by.columns) == numeric + ["comparison", "group1", "group2"] and len(by) == len(names) * len(pos)
    singles = []
    for k, v in enumerate(names.tolist()):
        block = by.iloc[k * len(pos): (k + 1) * len(pos)]
        one = model.differential_expression_median(gi, g, cells[lab == v], None, seed=seed + k, **kwargs)
        singles.append(one)
        _same_frames(block, one, numeric, f"{ctx} label {v}")
        assert block.index.tolist() == one.index.tolist()
        assert (block["comparison"] == f"{v} vs Rest").all() and (block["group1"] == v).all() and (block["group2"] == "Rest").all()
    only = model.differential_expression_by(gi, g, "cell_type", labels=[names[1]], seed=seed, **kwargs)
    assert len(only) == len(pos) and only.equals(by.iloc[len(pos): 2 * len(pos)])
    assert model.differential_expression_by(gi, g, lab, seed=seed, **kwargs).equals(by)   # an array instead of the column's name
    no_med = model.differential_expression_by(gi, g, "cell_type", seed=seed, lfc_median=False, **kwargs)
    assert list(no_med.columns) == [c for c in by.columns if c != "lfc_median"] and no_med.equals(by.drop(columns="lfc_median"))
    # sampled latents, two draws, injected noise
    nf = _noise_fn(dev)
    kw2 = dict(gene_list=pos, n_samples=2, n_pairs=2000, batch_size=bs, _noise=nf)
    by2 = model.differential_expression_by(gi, g, "cell_type", seed=seed, **kw2)
    for k, v in enumerate(names.tolist()):
        one = model.differential_expression_median(gi, g, cells[lab == v], None, seed=seed + k, **kw2)
        _same_frames(by2.iloc[k * len(pos): (k + 1) * len(pos)], one, numeric, f"{ctx} n_samples=2 label {v}")
    assert not by2["lfc_mean"].equals(by["lfc_mean"])

    # ---- (c) module mode, errors, save / load --------------------------------------------------------------------------------
    model.module.train()
    model.differential_expression_by(gi, g, "cell_type", labels=[names[0]], seed=seed, **kwargs)
    assert model.module.training
    model.module.eval()
    with pytest.raises(ValueError, match="two distinct labels"):
        model.differential_expression_by(gi, g, np.zeros(len(cells), int), **kwargs)
    with pytest.raises(KeyError, match="nope"):
        model.differential_expression_by(gi, g, "cell_type", labels=["nope"], **kwargs)
    with pytest.raises(KeyError, match="no_such_column"):
        model.differential_expression_by(gi, g, "no_such_column", **kwargs)
    with pytest.raises(ValueError, match="one label per cell"):
        model.differential_expression_by(gi, g, lab[:-1], **kwargs)
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=adata())
    assert back.differential_expression_by(gi, g, "cell_type", seed=seed, **kwargs).equals(by)
    assert not back.module.training
