"""Float64 numpy oracle of smcdet_amd.predictive (smcdet_posterior_image and
the derived fields of PosteriorImage), on top of oracle.smc_oracle.render_rate.

Layouts as the oracle's: rate [nH,nW,H,W,N], weights [nH,nW,N] (None:
uniform), image [nH,nW,H,W]."""
import numpy as np

from oracle import smc_oracle as O


def noise_var(model, rate):
    """v(rate): noise_additive + noise_multiplicative * rate (M71), rate (Poisson)."""
    if hasattr(model, "noise_multiplicative"):
        return np.float64(model.noise_additive) + np.float64(model.noise_multiplicative) * rate
    return rate


def eta(model):
    """dv/drate."""
    return float(getattr(model, "noise_multiplicative", 1.0))


def normalised(weights, shape):
    if weights is None:
        return np.full(shape, 1.0 / shape[-1])
    w = np.asarray(weights, np.float64)
    return w / w.sum(-1, keepdims=True)


def moments(rate, weights=None):
    """Weighted mean, population variance and root mean square of the rate over
    catalogs: each [nH,nW,H,W]."""
    rate = np.asarray(rate, np.float64)
    w = normalised(weights, rate.shape[:2] + rate.shape[-1:])[:, :, None, None, :]
    mean = (w * rate).sum(-1)
    var = (w * (rate - mean[..., None]) ** 2).sum(-1)
    rms = np.sqrt((w * rate ** 2).sum(-1))
    return mean, var, rms


def chi2(model, image, rate):
    """sum_p (x - rate)^2 / v(rate) per catalog: [nH,nW,N]."""
    rate = np.asarray(rate, np.float64)
    x = np.asarray(image, np.float64)[..., None]
    return ((x - rate) ** 2 / noise_var(model, rate)).sum((2, 3))


def chi2_sensitivity(model, image, rate):
    """sum_p (|2 (x - rate) / v| + eta (x - rate)^2 / v^2) * rate per catalog:
    |d chi2 / d log rate| summed over pixels, the factor of a relative error
    in every rate."""
    rate = np.asarray(rate, np.float64)
    x = np.asarray(image, np.float64)[..., None]
    v = noise_var(model, rate)
    return ((np.abs(2 * (x - rate) / v) + eta(model) * (x - rate) ** 2 / v ** 2) * rate).sum((2, 3))


def p_value(stat_rep, stat_obs, weights=None):
    """Weighted share of catalogs with stat_rep >= stat_obs (ties count)."""
    hit = np.asarray(stat_rep, np.float64) >= np.asarray(stat_obs, np.float64)
    return (normalised(weights, hit.shape) * hit).sum(-1)


def posterior_image(model, locs, fluxes, weights=None, image=None):
    """Everything that does not depend on the replicate noise."""
    rate = O.render_rate(locs, fluxes, model)
    mean, var, rms = moments(rate, weights)
    out = dict(rate=rate, mean=mean, rate_var=var, rms=rms, noise_var=noise_var(model, mean))
    out["pred_var"] = out["rate_var"] + out["noise_var"]
    if image is not None:
        x = np.asarray(image, np.float64)
        out["residual"] = x - mean
        out["z"] = out["residual"] / np.sqrt(out["pred_var"])
        out["flux_obs"] = x.sum((-2, -1))
        out["chi2"] = chi2(model, image, rate)
        out["chi2_sens"] = chi2_sensitivity(model, image, rate)
    return out
