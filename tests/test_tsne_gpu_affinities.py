"""GPU: spv_tsne_affinities (spvipes_amd.tsne_ops.affinities) against the float64 search of tests/_tsne_reference.py: rows sum to 1 within
fp32 rounding, the float64 entropy of a returned row is within 2e-5 of log(perplexity) wherever the reference converges within its 100
steps, and P is the softmax of the returned beta.  Rows with empty slots (+inf), a row of equal distances (the entropy is log k whatever
beta: the search runs out), a row with one neighbour, a row without any.  Every test here imports the new function and fails without it."""
import numpy as np
import pytest
import torch

from tests import _tsne_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()
    return torch.device("cuda:0")


def _rows(n, k, seed):
    rng = np.random.default_rng([seed, n, k])
    d2 = np.sort(rng.gamma(2.0, 2.0, (n, k)).astype(np.float32) + np.float32(3.0), axis=1)
    if n >= 8:
        d2[1, k // 2:] = np.inf      # idx = -1 slots
        d2[2, :] = 1.5               # equal distances
        d2[3, :] = np.inf            # no neighbour at all
        d2[4, 1:] = np.inf           # one neighbour
        d2[5, k - 1] = np.inf
        d2[6] = d2[6] * np.float32(1e-4)   # a tight neighbourhood: beta far above 1
        d2[7] = d2[7] * np.float32(1e4)    # a wide one: beta far below 1
    return d2


@pytest.mark.parametrize("n", [1, 130, 300])
@pytest.mark.parametrize("k,perplexity", [(5, 2.0), (60, 20.0), (64, 30.0)])
def test_affinities(dev, n, k, perplexity):
    from spvipes_amd.tsne_ops import affinities
    d2 = _rows(n, k, 11)
    P, beta = affinities(torch.from_numpy(d2).to(dev), perplexity)
    P2, beta2 = affinities(torch.from_numpy(d2).to(dev), perplexity)
    assert torch.equal(P, P2) and torch.equal(beta, beta2), "two calls agree bit for bit"
    P, beta = P.cpu().numpy(), beta.cpu().numpy()
    assert P.dtype == np.float32 and P.shape == (n, k) and beta.dtype == np.float64 and beta.shape == (n,)
    Pr, br, conv = R.affinities_ref(d2, perplexity)
    finite = np.isfinite(d2)
    some = finite[:, 0]
    assert (P[~finite] == 0).all() and (P[finite] >= 0).all() and (beta[~some] == 1.0).all()
    # each entry is one fp32 rounding of e / S: k of them sum to 1 within k 2^-24 (and the fp64 sum's own 2^-53s)
    assert (np.abs(P[some].astype(np.float64).sum(axis=1) - 1.0) <= (k + 1) * R.U).all()
    H = np.array([R.entropy_of(P[i]) for i in range(n)])
    assert conv[some].mean() > 0.9 or n == 1, "the reference converges on the ordinary rows"
    assert (np.abs(H[conv] - np.log(perplexity)) <= 2e-5).all(), np.abs(H[conv] - np.log(perplexity)).max()
    # P is the softmax of the RETURNED beta: float64 from d2 and beta, one fp32 rounding, and the device's exp against numpy's (2^-50)
    with np.errstate(invalid="ignore"):
        d = np.where(finite, d2.astype(np.float64) - d2[:, :1].astype(np.float64), np.inf)
        e = np.where(finite, np.exp(-beta[:, None] * np.where(finite, d, 0.0)), 0.0)
    want = e[some] / e[some].sum(axis=1, keepdims=True)
    assert (np.abs(P[some] - want) <= (R.U + 2.0 ** -40) * want + 2.0 ** -149).all()
    # and the search took the reference's path: the same beta up to the last bits of the entropies it compared
    assert np.allclose(beta[conv], br[conv], rtol=1e-6)
    if n >= 8:
        assert not conv[2] and np.allclose(P[2], 1.0 / k, rtol=1e-6) and P[4, 0] == 1.0 and beta[6] > 100 and beta[7] < 0.01


def test_refusals(dev):
    from spvipes_amd import _abi
    from spvipes_amd.tsne_ops import affinities
    with pytest.raises(_abi.SpvError, match="d2"):
        affinities(torch.zeros((4, 65), dtype=torch.float32, device=dev), 5.0)
    with pytest.raises(ValueError, match="perplexity"):
        affinities(torch.zeros((4, 6), dtype=torch.float32, device=dev), 0.5)
