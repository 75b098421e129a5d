"""TEST INFRASTRUCTURE ONLY -- the yardstick the count sampler (csrc/spv_dec_sample.h: nbmix_draw) is held to: the NB mixture's pmf in
float64 and three derived acceptance bounds for a sample of it.  Shared by tests/test_sample_host_cpu.py, tests/test_gpu_nbmix_sample.py
and tests/test_gpu_posterior_predictive.py.  numpy, float64 (log-gamma through torch.lgamma on the CPU: numpy has none).

The law.  x ~ pi NB(m1, theta) + (1 - pi) NB(m2, theta), NB(mu, theta) the Gamma-Poisson mixture with mean mu and variance
mu + mu^2 / theta:  log pmf(k) = lgamma(k + theta) - lgamma(theta) - lgamma(k + 1) + theta log(theta / (theta + mu)) + k log(mu / (theta + mu)).

``pmf_table`` tabulates it on 0 .. K, K = max over both components of (mu + 40 sqrt(mu + mu^2 / theta) + 200).  For theta >= 0.3 the
mass beyond that K is below 1e-11.  For theta = 0.05 it is not (a Gamma of shape 0.05 still has 9e-7 beyond 9 scale units, which is
where 40 standard deviations end), and a table cut there would both reject correct draws and understate the fourth moment; K is
therefore doubled until the mass beyond it IS below 1e-11.  The bounds below then hold as derived.

``check(x, p)`` -> three ratios, each of which must be <= 1 for a sample x of size N from the tabulated law:
  distribution  sup |F_N - F| / eps,  eps = sqrt(ln(2 / alpha) / (2 N)), alpha = 1e-9: the Dvoretzky-Kiefer-Wolfowitz inequality with
                Massart's constant, P(sup |F_N - F| > eps) <= 2 exp(-2 N eps^2) = alpha; distribution-free, valid for discrete laws
  mean          |mean - m| / (6 sqrt(v / N))
  variance      |var - v| / (6 sqrt((mu4 - v^2) / N))       (var = the mean squared deviation from the sample mean)
with m, v, mu4 the table's mean, variance and fourth central moment.  A draw outside 0 .. K is a failure (ratio = inf).
Derived bounds, not measured ones."""
from __future__ import annotations

import math

import numpy as np
import torch

ALPHA = 1e-9
TAIL = 1e-11
N_DRAWS = 65536
THETAS = (0.05, 0.3, 1.0, 3.0, 30.0, 1e4)
RATES = ((1e-3, 0.5), (0.5, 5.0), (5.0, 9.5), (12.0, 80.0), (300.0, 3000.0), (1e4, 2.0))
PIS = (0.0, 0.1, 0.5, 1.0)
GRID = tuple((th, m1, m2, pi) for th in THETAS for (m1, m2) in RATES for pi in PIS)   # 144 points


def _lgamma(a: np.ndarray) -> np.ndarray:
    return torch.lgamma(torch.from_numpy(np.ascontiguousarray(a, np.float64))).numpy()


def nb_pmf(k: np.ndarray, mu: float, theta: float) -> np.ndarray:
    if mu <= 0.0:
        return (k == 0).astype(np.float64)
    lg = _lgamma(k + theta) - math.lgamma(theta) - _lgamma(k + 1.0) + theta * math.log(theta / (theta + mu)) + k * math.log(mu / (theta + mu))
    return np.exp(lg)


def table_extent(m1: float, m2: float, theta: float) -> int:
    return int(math.ceil(max(mu + 40.0 * math.sqrt(mu + mu * mu / theta) + 200.0 for mu in (m1, m2))))


def pmf_table(m1: float, m2: float, theta: float, pi: float) -> np.ndarray:
    """the mixture's pmf on 0 .. K (see the module docstring for K); p.sum() >= 1 - 1e-11"""
    K = table_extent(m1, m2, theta)
    while True:
        k = np.arange(K + 1, dtype=np.float64)
        p = np.zeros(K + 1)
        if pi > 0.0:
            p += pi * nb_pmf(k, m1, theta)
        if pi < 1.0:
            p += (1.0 - pi) * nb_pmf(k, m2, theta)
        if 1.0 - p.sum() < TAIL:
            return p
        K *= 2


def moments(p: np.ndarray):
    k = np.arange(p.size, dtype=np.float64)
    m = float((k * p).sum())
    d = k - m
    return m, float((d * d * p).sum()), float((d ** 4 * p).sum())


def dkw_eps(n: int, alpha: float = ALPHA) -> float:
    return math.sqrt(math.log(2.0 / alpha) / (2.0 * n))


def check(x: np.ndarray, p: np.ndarray):
    """-> (distribution, mean, variance) ratios of the sample x against the table p; each must be <= 1"""
    x = np.asarray(x).reshape(-1)
    n = x.size
    if x.min() < 0 or x.max() >= p.size:
        return (math.inf, math.inf, math.inf)
    F = np.cumsum(p)
    Fn = np.cumsum(np.bincount(x.astype(np.int64), minlength=p.size)) / n
    m, v, mu4 = moments(p)
    xs = x.astype(np.float64)
    mean = xs.mean()
    var = ((xs - mean) ** 2).mean()
    r_mean = abs(mean - m) / (6.0 * math.sqrt(v / n)) if v > 0 else (0.0 if mean == m else math.inf)
    r_var = abs(var - v) / (6.0 * math.sqrt((mu4 - v * v) / n)) if mu4 > v * v else (0.0 if var == v else math.inf)
    return (float(np.abs(Fn - F).max()) / dkw_eps(n), r_mean, r_var)


def numpy_draws(rng, m1: float, m2: float, theta: float, pi: float, n: int = N_DRAWS) -> np.ndarray:
    """the reference route: Bernoulli, Gamma(theta, mu / theta), Poisson with numpy's own samplers"""
    mu = np.where(rng.random(n) < pi, m1, m2)
    return rng.poisson(np.minimum(rng.gamma(theta, mu / theta), 1e8))
