"""GPU: the normalised latents of spVIPES.get_latent_representation(normalized=True, give_mean=False) on the duck AnnData: the
``theta`` the inference kernels write, held to softmax (float64 numpy) of the ``log_z`` that normalized=False returns under the
same injected draws.

The elementwise bound ``softmax_bound(n)``, from fp32 arithmetic on given fp32 inputs (the reference softmaxes the same fp32
``log_z`` in float64):
  a. d = z - max: the common shift cancels in a softmax, what remains is the rounding of the difference, 2^-24 |d|; then the product
     d * log2(e) with the constant's own representation error: two more, 3 * 2^-24 |d| in all (an absolute error of the exponent is a
     relative error of the exponential).
  b. the hardware exponential (v_exp_f32): 1 ulp = 2^-23 relative.
     So the computed exponential is e^d (1 + rho), |rho| <= 2^-23 + 3 * 2^-24 |d|, and a softmax term p_j moves by at most
     p_j (|rho_j| + sum_k p_k |rho_k|).  p_j |d_j| <= |d| e^d <= 1 / e < ln n for n >= 2 and sum_k p_k |d_k| = H(p) - ln(sum_k e^{d_k})
     <= ln n (the entropy of n outcomes; the sum of the exponentials is >= 1): both parts are <= A = 2^-23 + 3 * 2^-24 ln(max(n, 2)),
     the term moves by <= 2 A p_j.
  c. the row sum: n positive terms, (n - 1) 2^-24 relative in any order; its reciprocal and the product (1 ulp and one
     multiplication; a correctly written division is within 2.5 ulp, which covers both): 2.5 * 2^-23.
  softmax_bound(n) = 2 A + ((n - 1) + 5) * 2^-24, with p_j <= 1:  1.2e-6 at n = 5, 1.6e-6 at n = 10."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
N_S, N_P = 10, 5


def softmax_bound(n):
    a = 2.0 ** -23 + 3 * U * math.log(max(n, 2))
    return 2 * a + ((n - 1) + 5) * U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _softmax64(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def _noise_fn(dev):
    def noise(draw, b0, b1):
        g = torch.Generator(device="cpu").manual_seed(1000 + draw)
        mk = lambda b, n: torch.randn(b, n, generator=g).to(dev)
        return {"enc_0_private": mk(b0, N_P), "enc_0_shared": mk(b0, N_S), "enc_1_private": mk(b1, N_P), "enc_1_shared": mk(b1, N_S),
                "poe_0": mk(b0, N_S), "poe_1": mk(b1, N_S)}
    return noise


@pytest.mark.parametrize("config,precision", [("label", "fp32"), ("paired", "bf16")])
def test_get_latent_representation_normalized_sample(dev, tmp_path, config, precision):
    from spvipes_amd.model import spVIPES
    from tests._duck import make_duck

    def adata():
        return make_duck(n=(96, 70) if config == "paired" else (300, 260), seed=2, with_plan=(config == "paired"))   # n0 != n1, ragged last batches

    ad = adata()
    kw = {"transport_plan_key": "plan"} if config == "paired" else {"label_key": "cell_type"}
    spVIPES.setup_anndata(ad, groups_key="groups", **kw)
    torch.manual_seed(0)
    model = spVIPES(ad, n_hidden=32, n_dimensions_shared=N_S, n_dimensions_private=N_P, precision=precision)
    gi = [list(ad.uns["groups_obs_indices"][0]), list(np.random.default_rng(3).permutation(ad.uns["groups_obs_indices"][1]))]
    model.train(gi, batch_size=32, max_epochs=2, train_size=1.0)   # a few steps: moves parameters and BatchNorm running statistics
    bs = 64 if config != "paired" else 32
    n, dims = [len(g) for g in gi], {"private": N_P, "shared": N_S}
    model.module.train()   # every call must put the module into eval mode and restore this
    nf = _noise_fn(dev)

    # the softmax of the very log_z that normalized=False returns
    plain = model.get_latent_representation(gi, batch_size=bs, _noise=nf)
    theta = model.get_latent_representation(gi, batch_size=bs, normalized=True, give_mean=False, _noise=nf)
    assert model.module.training
    assert set(theta) == set(plain) == {"shared", "private", "shared_reordered", "private_reordered"}
    for k in plain:
        kind = k.split("_")[0]
        for g in range(2):
            assert theta[k][g].shape == plain[k][g].shape == (n[g], dims[kind]) and theta[k][g].dtype == np.float32
            err = np.abs(theta[k][g] - _softmax64(plain[k][g].astype(np.float64)))
            print(f"{config} {k} group {g}: max err {err.max():.3e}, bound {softmax_bound(dims[kind]):.3e}")
            assert err.max() <= softmax_bound(dims[kind]), (k, g, err.max())
            assert (np.abs(theta[k][g].astype(np.float64).sum(1) - 1.0) <= dims[kind] * 2.0 ** -23 + softmax_bound(dims[kind])).all()
    # *_reordered: group 0 as is, group 1 sorted by its 'indices' column
    order = np.argsort(np.asarray(ad.obs["indices"])[np.asarray(gi[1])])
    assert not np.array_equal(order, np.arange(n[1]))
    for kind in dims:
        np.testing.assert_array_equal(theta[f"{kind}_reordered"][0], theta[kind][0])
        np.testing.assert_array_equal(theta[f"{kind}_reordered"][1], theta[kind][1][order])
    # the same injected draws: the same bits
    again = model.get_latent_representation(gi, batch_size=bs, normalized=True, give_mean=False, _noise=nf)
    for k in theta:
        for g in range(2):
            np.testing.assert_array_equal(theta[k][g], again[k][g])
    # the Monte-Carlo mean is not built, and says so before it touches the module
    with pytest.raises(NotImplementedError, match="give_mean"):
        model.get_latent_representation(gi, batch_size=bs, normalized=True)
    assert model.module.training

    # a model restored by save / load gives the same numbers
    d = str(tmp_path / "model")
    model.save(d)
    back = spVIPES.load(d, adata=adata())
    restored = back.get_latent_representation(gi, batch_size=bs, normalized=True, give_mean=False, _noise=nf)
    for k in theta:
        for g in range(2):
            np.testing.assert_array_equal(restored[k][g], theta[k][g])
