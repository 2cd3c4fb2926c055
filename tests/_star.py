"""StarPrior (Normal fluxes) test helpers: the fixtures' parameters
(tests/golden/make_star_golden.py), product- and oracle-side constructors, and
the float64 Normal log prior the oracle's MH sweep is run with."""
import contextlib
from dataclasses import dataclass

import numpy as np

from tests._params import golden, tiles_of

# experiments/jsm2024 (normalfluxes_*): StarPrior(1300, 250), Poisson
# ImageModel(psf_stdev=1.0, background=300); kernel flux bounds mean +- 5 stdev
# (the reference's proposal asserts every current flux inside its bounds)
STAR = dict(flux_mean=1300.0, flux_stdev=250.0, pad=2, psf_radius=8, psf_stdev=1.0,
            background=300.0, fluxes_min=50.0, fluxes_max=2550.0)


def _f32(x):
    return float(np.float32(x))


@dataclass
class NormalPriorP:
    """smcdet/prior.py:125-154 (StarPrior) over PointProcessPrior :8-75, in the
    shape of the oracle's prior parameter objects."""
    min_objects: int
    max_objects: int
    H: int
    W: int
    pad: float
    flux_mean: float
    flux_stdev: float

    @property
    def loc_low(self):
        return _f32(-self.pad)

    @property
    def loc_high(self):
        return (_f32(self.H + self.pad), _f32(self.W + self.pad))


def normal_log_prior(counts, locs, fluxes, prior, dtype=np.float64):
    """StarPrior.log_prob (prior.py:151-154 -> :67-75): DiscreteUniform count,
    uniform locations and Normal(mean, stdev) fluxes over the first `count`
    sources; a flux of 0 is not replaced."""
    counts = np.asarray(counts, dtype=dtype)
    locs = np.asarray(locs, dtype=dtype)
    fluxes = np.asarray(fluxes, dtype=dtype)
    S = locs.shape[-2]
    mask = np.arange(S)[None] < counts[..., None]
    k = prior.max_objects - prior.min_objects + 1
    insup = (counts >= prior.min_objects) & (counts <= prior.max_objects)
    lp = np.where(insup, dtype(np.log(np.float32(1.0 / k))), -np.inf)
    lo = np.asarray(prior.loc_low, dtype=dtype)
    hi = np.array(prior.loc_high, dtype=dtype)
    with np.errstate(divide="ignore"):
        lu = np.where((locs >= lo) & (locs < hi), -np.log(hi - lo), -np.inf)
    # (x * mask with x = -inf in a masked slot would be nan: where() instead)
    lp = lp + np.where(mask, lu.sum(-1), 0.0).sum(-1)
    mu, sd = dtype(_f32(prior.flux_mean)), dtype(_f32(prior.flux_stdev))
    lf = -((fluxes - mu) ** 2) / (2 * sd * sd) - np.log(sd) - 0.5 * np.log(2 * np.pi)
    return lp + np.where(mask, lf, 0.0).sum(-1)


@contextlib.contextmanager
def oracle_with_normal_prior():
    """For its duration oracle.smc_oracle.log_prior handles a NormalPriorP and
    delegates every other prior (log_target looks log_prior up at call time)."""
    from oracle import smc_oracle as O
    orig = O.log_prior

    def log_prior(counts, locs, fluxes, prior, dtype=np.float64):
        if isinstance(prior, NormalPriorP):
            return normal_log_prior(counts, locs, fluxes, prior, dtype)
        return orig(counts, locs, fluxes, prior, dtype)

    O.log_prior = log_prior
    try:
        yield O
    finally:
        O.log_prior = orig


# ---- oracle-side constructors ---------------------------------------------------
def o_star_model(H):
    from oracle import smc_oracle as O
    return O.BasicModel(H, H, STAR["background"], STAR["psf_radius"], STAR["psf_stdev"])


def o_star_prior(H, smin, smax):
    return NormalPriorP(smin, smax, H, H, STAR["pad"], STAR["flux_mean"], STAR["flux_stdev"])


def o_star_mh(K, locs_stdev=0.25, fluxes_stdev=100):
    from oracle import smc_oracle as O
    return O.MHParams(K, locs_stdev, fluxes_stdev, STAR["fluxes_min"], STAR["fluxes_max"])


# fixture name -> (tile_dim, smin, smax, K)
STAR_MH_FIXTURES = {"star_mh_16x16": (16, 1, 3, 20), "star_mh_tiles": (8, 2, 2, 10)}


def star_mh_fixture_setup(name):
    td, smin, smax, K = STAR_MH_FIXTURES[name]
    return td, o_star_model(td), o_star_prior(td, smin, smax), o_star_mh(K)


def oracle_mh_trace(d, name):
    """(locs, fluxes, acc, log alpha, decisions) of the float64 oracle's MH
    sweep on a star_mh_* fixture's recorded draws."""
    td, model, prior, mh = star_mh_fixture_setup(name)
    t = tiles_of(d["image"], td)
    tau = np.full(t.shape[:2], float(d["tau"]))
    with oracle_with_normal_prior() as O:
        return O.mh_sweep(t, d["counts"], d["locs0"], d["fluxes0"], tau, prior, model, mh,
                          d["comp"], d["uloc"], d["uflux"], d["uacc"], trace=True)


def decision_margin(d, loga):
    with np.errstate(all="ignore"):
        m = np.abs(np.log(np.asarray(d["uacc"], dtype=np.float64)) - np.minimum(loga, 0))
    return float(np.where(np.isfinite(m), m, np.inf).min())


def decisions_pinned(d, name, min_margin):
    """True if the float64 oracle reproduces every recorded decision of the
    fixture with |log U - log alpha| >= min_margin."""
    _, _, _, loga, acc = oracle_mh_trace(d, name)
    m = decision_margin(d, loga)
    same = np.array_equal(acc, np.asarray(d["accept"]).astype(bool))
    print(name, "min margin %.2e" % m, "decisions equal", same)
    return bool(same and m >= min_margin)


# ---- product-side constructors (smcdet_amd) -------------------------------------
def p_star_model(H):
    from smcdet_amd.images import ImageModel
    return ImageModel(image_height=H, image_width=H, psf_radius=STAR["psf_radius"],
                      psf_stdev=STAR["psf_stdev"], background=STAR["background"])


def p_star_prior(H, smin, smax, **kw):
    from smcdet_amd.prior import StarPrior
    return StarPrior(min_objects=smin, max_objects=smax, image_height=H, image_width=H,
                     flux_mean=STAR["flux_mean"], flux_stdev=STAR["flux_stdev"], pad=STAR["pad"],
                     **kw)


def p_star_mh(K, locs_stdev=0.25, fluxes_stdev=100, **kw):
    from smcdet_amd.kernel import SingleComponentMH
    return SingleComponentMH(K, locs_stdev, fluxes_stdev, STAR["fluxes_min"], STAR["fluxes_max"],
                             **kw)


def p_star_mala(K, locs_step=0.25, fluxes_step=100):
    from smcdet_amd.kernel import SingleComponentMALA
    return SingleComponentMALA(K, locs_step, fluxes_step, STAR["fluxes_min"], STAR["fluxes_max"])


def p_star_mh_fixture_setup(name, **kw):
    td, smin, smax, K = STAR_MH_FIXTURES[name]
    return td, p_star_model(td), p_star_prior(td, smin, smax), p_star_mh(K, **kw)


def star_golden(name):
    return golden(name)
