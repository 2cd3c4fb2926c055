"""The noise statistics of tests/_noise_stats.py on numpy's own float64 draws:
a correct sampler passes every condition at the n the GPU test uses, and a
sampler whose variance is 1% too large fails -- so the helper is neither too
tight nor vacuous before it judges smcdet_sample_image (test_gpu_noise.py)."""
import numpy as np
import pytest

from tests import _noise_stats as NS

N_DRAWS = 1 << 20
POISSON_RATES = [0.05, 1.0, 9.99, 10.0, 10.01, 30.0, 1e3, 5e4, 3e5, 1e6]


def test_normal_draws_pass():
    g = np.random.default_rng(20261019)
    a, b = g.normal(size=N_DRAWS), g.normal(size=N_DRAWS)
    rep = NS.normal_report(a, b)
    NS.show("normal", rep)
    assert set(rep) == {"mean", "variance", "skewness", "excess_kurtosis", "autocorr_lag1",
                        "autocorr_lag64", "ks", "cross_seed_corr"}
    assert NS.failures(rep) == []


def test_normal_variance_inflated_fails():
    g = np.random.default_rng(20261020)
    rep = NS.normal_report(np.sqrt(1.01) * g.normal(size=N_DRAWS))
    NS.show("normal x1.01", rep)
    bad = NS.failures(rep)
    assert any(b.startswith("variance") for b in bad), rep
    assert rep["variance"][1] > NS.Z_MAX


def test_normal_correlated_fails():
    """Serial and cross-seed correlation of 1% are seen too."""
    g = np.random.default_rng(20261021)
    a = g.normal(size=N_DRAWS)
    ar = a.copy()
    ar[1:] += 0.01 * a[:-1]
    ar /= np.sqrt(1.0001)
    rep = NS.normal_report(ar, 0.01 * ar + g.normal(size=N_DRAWS))
    bad = " ".join(NS.failures(rep))
    assert "autocorr_lag1:" in bad and "cross_seed_corr" in bad and "autocorr_lag64" not in bad


@pytest.mark.parametrize("lam", POISSON_RATES)
def test_poisson_draws_pass(lam):
    g = np.random.default_rng([20261022, int(lam * 100)])
    rep = NS.poisson_report(g.poisson(lam, N_DRAWS), lam)
    NS.show(f"poisson {lam:g}", rep)
    assert ("chi2" in rep) == (lam <= 30)
    assert NS.failures(rep) == []


@pytest.mark.parametrize("lam", [30.0, 1e3, 1e6])
def test_poisson_variance_inflated_fails(lam):
    """Poisson(lam * G), G gamma with mean 1 and variance 0.01 / lam: integer
    draws of mean lam and variance 1.01 lam."""
    g = np.random.default_rng([20261023, int(lam)])
    shape = lam / 0.01
    k = g.poisson(lam * g.gamma(shape, 1.0 / shape, N_DRAWS))
    rep = NS.poisson_report(k, lam)
    NS.show(f"poisson {lam:g} x1.01", rep)
    assert any(b.startswith("variance") for b in NS.failures(rep)), rep
    assert abs(rep["mean"][1]) <= NS.Z_MAX


def test_poisson_skew_se_against_simulation():
    """The delta-method standard error of the sample skewness against its
    spread over repeated small samples (and 6 / n in the Normal limit)."""
    g = np.random.default_rng(20261024)
    n, reps = 4096, 2000
    for lam in (0.05, 1.0, 30.0):
        k = g.poisson(lam, (reps, n)).astype(np.float64)
        d = k - k.mean(1, keepdims=True)
        sk = (d ** 3).mean(1) / (d ** 2).mean(1) ** 1.5
        assert abs(sk.std() / NS.poisson_skew_se(lam, n) - 1) < 0.1, lam
    assert abs(NS.poisson_skew_se(1e9, n) / np.sqrt(6.0 / n) - 1) < 1e-3


def test_chi2_pools_to_expected_counts():
    g = np.random.default_rng(20261025)
    p, bins = NS.poisson_chi2(g.poisson(0.05, N_DRAWS), 0.05)
    assert bins == 4 and p >= NS.P_MIN      # n pmf(3) = 20.8, n pmf(4) = 0.26: k >= 3 pooled
