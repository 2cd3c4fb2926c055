"""Statistics that judge a noise sampler's draws against its law
(tests/test_gpu_noise.py: smcdet_sample_image; tests/test_noise_stats_host.py
shows on numpy draws that they pass a correct sampler and fail one whose
variance is 1% too large).

A report is a dict name -> ("z", value) or ("p", value): a z-score is a
statistic minus its expectation over its standard error under the law, a
p-value that of a goodness-of-fit test.  failures() lists the entries outside
|z| <= Z_MAX or p >= P_MIN.  With n = 2^20 draws a 1% variance error is a
z of about 7.
"""
import numpy as np
from scipy import stats

Z_MAX = 4.5
P_MIN = 1e-5


def _central(x, order):
    d = x - x.mean()
    return [float((d ** k).mean()) for k in range(2, order + 1)]


def _autocorr(d, lag):
    return float((d[:-lag] * d[lag:]).mean() / (d * d).mean())


def normal_report(z, other=None):
    """z: residuals that should be iid N(0, 1); other: the residuals of a
    second seed at the same positions (their correlation should vanish)."""
    z = np.asarray(z, np.float64).ravel()
    n = z.size
    m2, m3, m4 = _central(z, 4)
    d = z - z.mean()
    rep = {
        "mean": ("z", float(z.mean()) * np.sqrt(n)),
        "variance": ("z", (m2 - 1.0) / np.sqrt(2.0 / n)),
        "skewness": ("z", m3 / m2 ** 1.5 / np.sqrt(6.0 / n)),
        "excess_kurtosis": ("z", (m4 / m2 ** 2 - 3.0) / np.sqrt(24.0 / n)),
        "autocorr_lag1": ("z", _autocorr(d, 1) * np.sqrt(n)),
        "autocorr_lag64": ("z", _autocorr(d, 64) * np.sqrt(n)),
        "ks": ("p", float(stats.kstest(z, "norm").pvalue)),
    }
    if other is not None:
        o = np.asarray(other, np.float64).ravel()
        rep["cross_seed_corr"] = ("z", float(np.corrcoef(z, o)[0, 1]) * np.sqrt(n))
    return rep


def poisson_skew_se(lam, n):
    """Standard error of the sample skewness m3 / m2^1.5 of n Poisson(lam)
    draws: the delta-method variance (Kendall & Stuart, vol. 1, 10.27)
      n var = (4 u2^2 u6 - 12 u2 u3 u5 - 24 u2^3 u4 + 9 u3^2 u4 + 35 u2^2 u3^2
               + 36 u2^5) / (4 u2^5)
    with the Poisson central moments u2 = u3 = lam, u4 = lam + 3 lam^2,
    u5 = lam + 10 lam^2, u6 = lam + 25 lam^2 + 15 lam^3 (6 for a Normal)."""
    u2 = u3 = lam
    u4 = lam + 3 * lam ** 2
    u5 = lam + 10 * lam ** 2
    u6 = lam + 25 * lam ** 2 + 15 * lam ** 3
    nv = (4 * u2 ** 2 * u6 - 12 * u2 * u3 * u5 - 24 * u2 ** 3 * u4 + 9 * u3 ** 2 * u4
          + 35 * u2 ** 2 * u3 ** 2 + 36 * u2 ** 5) / (4 * u2 ** 5)
    return float(np.sqrt(nv / n))


def poisson_chi2(k, lam, min_expected=10.0):
    """Pearson chi^2 of the counts of k against the exact Poisson(lam) pmf; the
    two tails are pooled into the outermost bins whose expected count reaches
    min_expected.  Returns (p-value, number of bins)."""
    k = np.asarray(k).astype(np.int64).ravel()
    n = k.size
    kmax = int(max(k.max(), lam + 20 * np.sqrt(lam) + 20))
    exp = n * stats.poisson.pmf(np.arange(kmax + 1), lam)
    ok = np.nonzero(exp >= min_expected)[0]
    lo, hi = int(ok[0]), int(ok[-1])
    obs = np.bincount(np.clip(k, lo, hi) - lo, minlength=hi - lo + 1).astype(np.float64)
    e = exp[lo:hi + 1].copy()
    e[0] += n * stats.poisson.cdf(lo - 1, lam)
    e[-1] += n * stats.poisson.sf(hi, lam)
    chi2 = float(((obs - e) ** 2 / e).sum())
    return float(stats.chi2.sf(chi2, e.size - 1)), int(e.size)


def poisson_report(k, lam, chi2_max_lam=30.0):
    """k: draws that should be iid Poisson(lam)."""
    k = np.asarray(k, np.float64).ravel()
    n = k.size
    m2, m3 = _central(k, 3)
    rep = {
        "mean": ("z", (float(k.mean()) - lam) / np.sqrt(lam / n)),
        "variance": ("z", (m2 - lam) / (lam * np.sqrt(2.0 / n + 1.0 / (lam * n)))),
        "skewness": ("z", (m3 / m2 ** 1.5 - lam ** -0.5) / poisson_skew_se(lam, n)),
    }
    if lam <= chi2_max_lam:
        rep["chi2"] = ("p", poisson_chi2(k, lam)[0])
    return rep


def failures(rep, z_max=Z_MAX, p_min=P_MIN):
    bad = []
    for name, (kind, v) in rep.items():
        if not np.isfinite(v) or (abs(v) > z_max if kind == "z" else v < p_min):
            bad.append(f"{name}: {kind} = {v:.4g}")
    return bad


def show(label, rep):
    print(label, "  ".join(f"{k} {kind}={v:.3g}" for k, (kind, v) in rep.items()))
