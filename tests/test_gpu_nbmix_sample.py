"""GPU: the count sampler on its own -- spv_nbmix_sample (csrc/spv_dec_sample.h: nbmix_draw over given parameters) against the NB
mixture's float64 pmf (tests/_nb_sampling_check.py: DKW distance, mean and variance, all derived bounds), its exact cases, the
addressing of its random stream and its argument errors.  Every test here needs the entry point and fails without it."""
import math

import numpy as np
import pytest
import torch

from tests import _nb_sampling_check as S

pytestmark = pytest.mark.gpu

FLT_TINY = float(np.finfo(np.float32).tiny)
FLT_DENORM = float(np.float32(1e-45))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from spvipes_amd import _abi
    _abi.load()   # raises if libspvipes_hip.so is missing: no fallback
    return torch.device("cuda:0")


def _columns(dev, cols, R):
    """constant parameter columns: cols = [(theta, m1, m2, logit)] -> contiguous fp32 [R, G] arrays + theta [G]"""
    c = np.asarray(cols, np.float32)
    full = lambda v: torch.tensor(v, device=dev).expand(R, len(cols)).contiguous()
    return full(c[:, 1]), full(c[:, 2]), full(c[:, 3]), torch.tensor(c[:, 0], device=dev)


def _draw(dev, cols, R, **kw):
    from spvipes_amd.dec_ops import nbmix_sample
    rp, rs, lg, th = _columns(dev, cols, R)
    return nbmix_sample(rp, rs, lg, th, **kw)


def _logit(pi):
    return math.inf if pi >= 1.0 else -math.inf if pi <= 0.0 else math.log(pi / (1.0 - pi))


def _f32(v):
    return float(np.float32(v))


def _tail_bound(mu, theta, tail=1e-12):
    """the smallest k with P(NB(mu, theta) > k) < tail, from the pmf summed from far out (the pmf decays geometrically there: with the
    last term below 1e-40 the mass beyond the table is below 1e-30)"""
    K = S.table_extent(mu, mu, theta) * 8
    p = S.nb_pmf(np.arange(K + 1, dtype=np.float64), mu, theta)
    assert p[-1] < 1e-40
    above = np.concatenate([np.cumsum(p[::-1])[::-1][1:], [0.0]])   # above[k] = P(X > k)
    return int(np.argmax(above < tail))


# ---- distribution --------------------------------------------------------------------------------------------------------------------
def test_every_grid_point_passes_the_distribution_mean_and_variance_bounds(dev):
    """R = 65 536 rows x 144 columns in ONE launch, one grid point per column.  The table of a column is evaluated at the fp32 values the
    kernel is handed (theta, both rates, and pi = sigmoid of the fp32 logit), in float64."""
    cols = [(th, m1, m2, _logit(pi)) for (th, m1, m2, pi) in S.GRID]
    x = _draw(dev, cols, S.N_DRAWS, key=0x1234ABCD5678, sample=0).cpu().numpy()
    assert x.shape == (S.N_DRAWS, 144) and x.dtype == np.int32 and x.min() >= 0
    worst, bad = np.zeros(3), []
    for j, (th, m1, m2, pi) in enumerate(S.GRID):
        lg = _f32(_logit(pi))
        p = S.pmf_table(_f32(m1), _f32(m2), _f32(th), 1.0 / (1.0 + math.exp(-lg)) if math.isfinite(lg) else pi)
        r = S.check(x[:, j], p)
        worst = np.maximum(worst, r)
        if max(r) > 1.0:
            bad.append(((th, m1, m2, pi), r))
    print("worst ratios (distribution, mean, variance):", worst)
    assert not bad, bad


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------
def test_a_saturated_logit_selects_one_component(dev):
    """logit = +40: pi rounds to 1 in fp32 and every uniform is < 1, so every draw comes from rate_p; -40: pi = 4e-18 is below the
    smallest uniform (2^-24), every draw comes from rate_s.  The other rate is 1e6: one draw from it would sit near 1e6, the chosen
    rate's law puts less than 1e-12 above the bound (131 072 draws: 1.3e-7 in all)."""
    R = 16384
    for theta, mu in ((3.0, 5.0), (0.3, 40.0)):
        bound = _tail_bound(mu, theta)
        x = _draw(dev, [(theta, mu, 1e6, 40.0)] * 4 + [(theta, 1e6, mu, -40.0)] * 4, R, key=7)
        assert x.shape == (R, 8) and int(x.min()) >= 0
        assert int(x.max()) <= bound < 1e5, (theta, mu, int(x.max()), bound)
        assert int(x.max()) > mu   # (and it is not a column of zeros)


def test_zero_and_tiny_rates_give_zeros_and_no_draw_is_negative(dev):
    R = 4096
    cols = [(th, m, m, lg) for th in (1e-3, 1.0, 1e4) for m in (0.0, FLT_DENORM, FLT_TINY) for lg in (-3.0, 0.0, 3.0)]
    x = _draw(dev, cols, R, key=3)
    assert int(x.abs().max()) == 0
    # a selected rate or a theta that is NaN, zero or negative gives 0 -- not Poisson(1e8), which a clamp that drops the NaN would draw
    nan = float("nan")
    cols = [(th, m, m, lg) for th in (1e-3, 1.0, 1e4) for m in (nan, -1.0, -3e38) for lg in (-3.0, 0.0, 3.0)]
    cols += [(th, m, m, 0.0) for th in (nan, 0.0, -1.0, -3e38) for m in (0.5, 12.0, 3e38)]
    assert int(_draw(dev, cols, R, key=5).abs().max()) == 0
    # one unusable rate of two: the draws that select it are 0, the others come from the usable rate (saturated logits select for certain)
    x = _draw(dev, [(3.0, nan, 5.0, 40.0), (3.0, nan, 5.0, -40.0), (3.0, 5.0, -1.0, -40.0), (3.0, 5.0, -1.0, 40.0)], R, key=6)
    assert int(x[:, 0].max()) == 0 and int(x[:, 2].max()) == 0
    assert 0 < int(x[:, 1].max()) <= _tail_bound(5.0, 3.0) and 0 < int(x[:, 3].max()) <= _tail_bound(5.0, 3.0)
    # the other end: rates and dispersions far outside a trained model's -- never a negative count, never above the clamp's reach
    cols = [(th, m1, m2, 0.0) for th in (1e-3, 0.05, 1.0, 1e6) for (m1, m2) in ((1e6, 1e9), (3e38, 1.0), (-1.0, 2.0), (nan, 1.0))]
    x = _draw(dev, cols, R, key=4)
    assert int(x.min()) >= 0 and int(x.max()) <= 100_100_000   # lam is clamped at 1e8: Poisson(1e8) stays below 1e8 + 10 sigma = 1e8 + 1e5
    big = _draw(dev, [(1.0, 3e38, 3e38, 0.0)], R, key=4)   # a usable, enormous rate IS clamped, not zeroed: Poisson(1e8) within 10 sigma
    assert int(big.min()) >= 99_900_000 and int(big.max()) <= 100_100_000


def test_a_tiny_theta_gives_mostly_zeros_and_a_finite_maximum(dev):
    """theta = 1e-3, mu = 10: P(x = 0) = (theta / (theta + mu))^theta = 0.99083; the zero fraction of N draws is within the DKW bound of
    it.  lam is clamped at 1e8, so no draw exceeds 1e8 + 10 sqrt(1e8)."""
    theta, mu, R, G = _f32(1e-3), 10.0, 16384, 8
    x = _draw(dev, [(theta, mu, mu, 0.0)] * G, R, key=11).cpu().numpy()
    p0 = (theta / (theta + mu)) ** theta
    zero = float((x == 0).mean())
    print(f"zero fraction {zero:.5f}, P(x = 0) = {p0:.5f}")
    assert abs(zero - p0) <= S.dkw_eps(R * G) and p0 > 0.99
    assert 0 <= x.min() and x.max() <= 100_100_000 and x.max() > 0


# ---- the stream ----------------------------------------------------------------------------------------------------------------------
STREAM_COLS = [(3.0, 12.0, 80.0, 0.0)] * 61 + [(0.3, 0.5, 5.0, 1.0), (30.0, 300.0, 3000.0, -1.0), (1.0, 5.0, 9.5, 0.5)]   # G = 64


def test_same_key_and_sample_repeat_and_other_keys_or_samples_are_independent(dev):
    """Two independent draws of one law agree with probability q = sum_k p_k^2; over n elements the number of agreements is
    Binomial(n, q): at most n q + 6 sqrt(n q (1 - q)).  Counted on the 61 columns that share one parameter set."""
    R = 200
    a = _draw(dev, STREAM_COLS, R, key=99, sample=5)
    assert torch.equal(a, _draw(dev, STREAM_COLS, R, key=99, sample=5))
    p = S.pmf_table(12.0, 80.0, 3.0, 0.5)
    q, n = float((p * p).sum()), R * 61
    limit = n * q + 6.0 * math.sqrt(n * q * (1.0 - q))
    for kw in (dict(key=100, sample=5), dict(key=99, sample=6), dict(key=99 + (1 << 32), sample=5), dict(key=99, sample=5 + (1 << 31))):
        b = _draw(dev, STREAM_COLS, R, **kw)
        same = int((a[:, :61] == b[:, :61]).sum())
        print(kw, "agreements", same, "expected", n * q, "limit", limit)
        assert same <= limit, (kw, same, limit)
        assert not torch.equal(a[:, 61:], b[:, 61:])


def test_cell_ids_name_the_rows_and_a_launch_extent_does_not_matter(dev):
    R = 200
    base = _draw(dev, STREAM_COLS, R, key=5, sample=1)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(0)).to(dev)
    got = _draw(dev, STREAM_COLS, R, key=5, sample=1, cell_ids=perm.int())
    assert torch.equal(got, base[perm])
    assert not torch.equal(got, base)
    shifted = _draw(dev, STREAM_COLS, R, key=5, sample=1, cell_ids=(torch.arange(R, device=dev) + 1000).int())
    assert not torch.equal(shifted, base)
    assert torch.equal(_draw(dev, STREAM_COLS, 70, key=5, sample=1), base[:70])
    # a column's draws depend on its gene id (= its column) and its own parameters, not on its neighbours: drop the last column
    assert torch.equal(_draw(dev, STREAM_COLS[:40], R, key=5, sample=1), base[:, :40])


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_entry_point(dev):
    from spvipes_amd import _abi
    R, G = 8, 4
    rp, rs, lg, th = _columns(dev, [(1.0, 2.0, 3.0, 0.0)] * G, R)
    out = torch.full((R, G), -9, dtype=torch.int32, device=dev)
    ptr = _abi.ptr
    good = dict(rate_p=ptr(rp), rate_s=ptr(rs), logit=ptr(lg), ld_in=G, theta=ptr(th), R=R, G=G, cell_ids=None, key=1, sample=0, out=ptr(out), ld_out=G)
    call = lambda **kw: _abi.call("spv_nbmix_sample", *{**good, **kw}.values(), _abi.stream_ptr())
    call()
    assert int(out.min()) >= 0
    call(R=0)   # nothing to do is not an error
    for bad in (dict(rate_p=None), dict(rate_s=None), dict(logit=None), dict(theta=None), dict(out=None), dict(G=0), dict(R=-1), dict(ld_in=G - 1), dict(ld_out=G - 1)):
        with pytest.raises(_abi.SpvError, match="spv_nbmix_sample"):
            call(**bad)
    torch.cuda.synchronize()
