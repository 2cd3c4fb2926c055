"""smcdet_amd — MI355X (gfx950) native SMC star-detection sampler.

Drop-in for the hot path of timwhite0/smcdet: the modules `sampler`,
`kernel`, `images`, `prior`, `distributions`, `metrics` keep the reference's classes
and signatures; the per-particle work runs as hand-written HIP kernels behind
the C ABI in include/smcdet_hip.h (libsmcdet_hip.so, loaded by ctypes).
`condense` (not in the reference) turns a run's catalogs into one list of
detections per tile; `predictive` (not in the reference either) gives the
posterior mean / variance image and posterior-predictive checks of a run;
`calibration` (the reference's results notebooks, by hand) gives count
posteriors, interval coverage, quantile bands and bootstrap bands;
`convergence` (not in the reference) gives split-R-hat, effective sample sizes
and Monte Carlo standard errors of MCMC chains; `extract` (the scripts'
run_sep.py baseline, without sep) is a classical multi-threshold source
extractor with the grid search of its hyperparameters for F1; `fit` (the
reference's m71.ipynb, "Optimize image model parameters") fits the M71 image
model's parameters to calibration fields with a fixed catalog; `photometry`
(not in the reference) is forced PSF photometry: the joint flux solve at fixed
positions with Cramér–Rao errors, for `extract`'s detections and for condensed
posterior detections; `psffind` (not in the reference) is the PSF-fitting
detector around it: the matched-filter significance map of the residual, its
peaks, leave-one-out recentring, and the grid search of its settings for F1.
"""
import importlib
import sys

from . import _hip  # noqa: F401

__version__ = "0.1.0"

_DROP_IN = ("sampler", "kernel", "images", "prior", "distributions", "aggregate",
            "metrics", "condense", "predictive", "calibration", "convergence", "extract",
            "fit", "photometry", "psffind")


def install_as_smcdet():
    """Registers this package under the reference's module names (`smcdet`,
    `smcdet.sampler`, ...) so that an unmodified driver doing
    `from smcdet.sampler import SMCsampler` runs on the HIP path."""
    pkg = sys.modules[__name__]
    sys.modules["smcdet"] = pkg
    for name in _DROP_IN:
        sys.modules[f"smcdet.{name}"] = importlib.import_module(f"{__name__}.{name}")
    return pkg
