"""Forced PSF photometry without a device: the float64 oracle against a closed
form, the calibration of its Cramér–Rao errors over noise replicates, and the
refusals of the Python layer and of the C ABI (all before any device work)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _photometry_oracle as O
import smcdet_amd
from _params import M71, p_basic_model, p_m71_model
from smcdet_amd import _hip, extract, photometry

MODEL = O.model_of(p_m71_model(8))


def test_exported_and_listed():
    assert "photometry" in smcdet_amd._DROP_IN
    name = "smcdet_forced_photometry"
    assert name in _hip.EXPORTS and name in _hip._OUTS
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "smcdet_hip.h")).read()
    assert name in header
    assert int(re.search(r"#define SMCDET_PHOT_MAX_SOURCES (\d+)", header).group(1)) == \
        _hip.PHOT_MAX_SOURCES == 32
    assert int(re.search(r"#define SMCDET_PHOT_MAX_ITER (\d+)", header).group(1)) == \
        _hip.PHOT_MAX_ITER == 16
    assert any(p.endswith("photometry_kernel.hip") for p in _hip.SOURCES)


def test_oracle_matches_the_closed_form():
    """One isolated source, the background fixed, one iteration:
    f = sum w phi (x - B) / (g sum w phi^2), to rounding."""
    m = MODEL
    rng = np.random.default_rng(7)
    loc = np.array([[3.7, 4.2]], np.float32)
    x = O.noisy(m, O.render(m, loc, [50.0]), rng)
    r = O.solve_one(m, x, 1, loc, n_iter=1)
    phi = O.columns(m, loc)[:, 0]
    xd = x.astype(np.float64).reshape(-1)
    w = 1.0 / (m.na + m.nm * np.maximum(xd, m.background / 4))
    f = np.sum(w * phi * (xd - m.background)) / (m.g * np.sum(w * phi * phi))
    assert abs(r["fluxes"][0] - f) <= 1e-13 * abs(f)
    assert r["n_free"] == 1 and r["status"] == 0 and r["n_pixels"] == 64
    assert 30.0 < f < 70.0


def test_oracle_captured_fraction():
    """The figures the module's docstring quotes: an 8x8 tile captures 0.909 of
    a star at its centre and 0.556 of one at (1, 1)."""
    for loc, frac in (((4.0, 4.0), 0.909), ((1.0, 1.0), 0.556)):
        assert abs(O.columns(MODEL, [loc]).sum() - frac) < 2e-3


@pytest.mark.parametrize("name", list(O.CONFIGS))
def test_oracle_errors_are_calibrated(name):
    """400 noise replicates per configuration: per source the mean of
    z = (f_hat - f) / flux_err within +-0.2 (about four standard errors of a
    mean of 400) and its standard deviation within [0.85, 1.15]."""
    m = MODEL
    locs, fluxes = O.CONFIGS[name]
    locs = np.asarray(locs, np.float32)
    rate = O.render(m, locs, fluxes)
    rng = np.random.default_rng(20240 + list(O.CONFIGS).index(name))
    z = np.empty((400, len(fluxes)))
    for i in range(400):
        r = O.solve_one(m, O.noisy(m, rate, rng), len(fluxes), locs)
        assert r["status"] == 0
        z[i] = (r["fluxes"] - np.asarray(fluxes)) / r["flux_err"]
    mean, sd = z.mean(0), z.std(0, ddof=1)
    print(f"{name}: mean z {np.round(mean, 3)}, sd z {np.round(sd, 3)}")
    assert np.all(np.abs(mean) <= 0.2), mean
    assert np.all((sd >= 0.85) & (sd <= 1.15)), sd


def test_oracle_skips_drops_and_refuses_singular_problems():
    m = MODEL
    x = O.noisy(m, O.render(m, [(3.5, 3.5)], [40.0]), np.random.default_rng(3))
    nan = float("nan")
    r = O.solve_one(m, x, 3, [(3.5, 3.5), (nan, 2.0), (-20.0, 3.0), (1.0, 1.0)])
    assert r["status"] == 1 and r["n_free"] == 1
    assert np.isfinite(r["fluxes"][0]) and r["fluxes"][1] == 0 and np.isnan(r["fluxes"][2])
    assert r["fluxes"][3] == 0 and np.isnan(r["flux_err"][1:]).all()
    for second in ((3.5, 3.5), (3.5, 3.5001)):
        r = O.solve_one(m, x, 2, [(3.5, 3.5), second])
        assert r["status"] == 2 and np.isnan(r["fluxes"]).all() and np.isnan(r["chi2"])
        # (the pair 1e-4 px apart has a squared pivot of 3e-9, inside the band the GPU
        # tests keep clear of; identical positions are clear of it)
        assert O.pivots_clear_of_threshold(r["pivots"]) == (second == (3.5, 3.5))
    r = O.solve_one(m, x, 2, [(3.5, 3.5), (3.5, 3.8)])
    assert r["status"] == 0 and min(r["pivots"]) > 1e-3


# ---- the Python layer: every refusal comes before anything touches a device -------
IMG = torch.zeros(2, 8, 8)
COUNTS = torch.ones(2, dtype=torch.int32)
LOCS = torch.full((2, 4, 2), 3.5)


def call(**kw):
    a = dict(images=IMG, counts=COUNTS, locs=LOCS, ImageModel=p_m71_model(8))
    a.update(kw)
    return photometry.forced_photometry(**a)


@pytest.mark.parametrize("kw, match", [
    (dict(locs=torch.zeros(2, 33, 2)), "33 position slots"),
    (dict(images=torch.zeros(2, 25, 41), ImageModel=p_m71_model(8)), "1025 pixels"),
    (dict(n_iter=0), "n_iter"),
    (dict(n_iter=17), "n_iter"),
    (dict(locs=torch.zeros(2, 4)), "locs must be"),
    (dict(locs=torch.zeros(2, 1, 1, 4, 2)), "locs must be"),
    (dict(locs=torch.zeros(2, 4, 3)), "locs must be"),
    (dict(locs=torch.zeros(3, 4, 2)), "do not go with"),
    (dict(counts=torch.ones(2, 2, dtype=torch.int32)), "counts"),
    (dict(ImageModel=p_m71_model(16)), "image model is 16x16"),
    (dict(background=0.0), "background"),
    (dict(background=torch.tensor([100.0, -1.0])), "background"),
])
def test_python_validation(kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)


def test_python_type_errors_and_host_tensors():
    with pytest.raises(TypeError, match="int"):
        call(n_iter=4.0)
    with pytest.raises(TypeError, match="image model"):
        call(ImageModel=object())
    with pytest.raises(TypeError, match="int32 or int64"):
        call(counts=torch.ones(2))
    with pytest.raises(RuntimeError, match="HIP device"):
        call()  # valid arguments, host tensors: refused, there is no CPU path
    with pytest.raises(TypeError, match="Extraction"):
        photometry.photometry_of((COUNTS, LOCS), IMG, p_m71_model(8))


def test_tune_refusals():
    args = (IMG, 0.0, 1.0, torch.zeros(2), torch.zeros(2, 1, 2), torch.zeros(2, 1), [1.5])
    with pytest.raises(ValueError, match="needs image_model"):
        extract.tune(*args, flux="psf")
    with pytest.raises(ValueError, match="'isophotal' or 'psf'"):
        extract.tune(*args, flux="aperture")
    with pytest.raises(ValueError, match="image model is 16x16"):
        extract.tune(*args, flux="psf", image_model=p_m71_model(16))
    with pytest.raises(ValueError, match="max_detections = 33"):
        extract.tune(*args, flux="psf", image_model=p_m71_model(8), max_detections=33)
    with pytest.raises(ValueError, match="only with flux='psf'"):
        extract.tune(*args, image_model=p_m71_model(8))
    # valid arguments reach the device check, with or without the new argument
    with pytest.raises(RuntimeError, match="HIP device"):
        extract.tune(*args, flux="psf", image_model=p_m71_model(8))
    with pytest.raises(RuntimeError, match="HIP device"):
        extract.tune(*args, flux="isophotal")


# ---- the C ABI's refusals (placeholder pointers, never dereferenced) ------------------
P = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(12)]


def c_phot(model=None, T=2, G=3, K=4, n_iter=4, flags=0, null=None, **fields):
    cm = type(p_m71_model(8)._cmodel()).from_buffer_copy(p_m71_model(8)._cmodel()) \
        if model is None else model
    for k, v in fields.items():
        setattr(cm, k, v)
    a = [ctypes.byref(cm), P[0], P[1], P[2], None, T, G, K, n_iter, flags, P[3], P[4], P[5],
         P[6], P[7], P[8], P[9], None, None]
    if null is not None:
        a[null] = None
    L = _hip.lib()
    return L.smcdet_forced_photometry(*a), L.smcdet_last_error()


def test_c_abi_refuses_unsupported_shapes():
    for kw, word in ((dict(H=33, W=32), b"pixels"), (dict(H=1, W=1025), b"pixels"),
                     (dict(K=33), b"K=33"), (dict(psf_radius=65), b"psf_radius"),
                     (dict(psf_radius=-1), b"psf_radius"),
                     (dict(T=65536, G=32768), b"problems")):
        rc, msg = c_phot(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)


def test_c_abi_refuses_invalid_arguments():
    for kw, word in ((dict(T=0), b">= 1"), (dict(G=0), b">= 1"), (dict(K=0), b">= 1"),
                     (dict(n_iter=0), b"n_iter"), (dict(n_iter=17), b"n_iter"),
                     (dict(flags=2), b"flags"), (dict(background=0.0), b"background"),
                     (dict(background=float("nan")), b"background"),
                     (dict(noise_multiplicative=-1.0), b"variance"),
                     (dict(adu_per_nmgy=0.0), b"adu_per_nmgy")):
        rc, msg = c_phot(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for pos in (1, 2, 3, 10, 11, 12, 13, 14, 15, 16):  # every required buffer
        rc, msg = c_phot(null=pos)
        assert rc == -1 and b"null" in msg, (pos, rc, msg)
    assert _hip.lib().smcdet_forced_photometry(None, *([None] * 4), 1, 1, 1, 4, 0,
                                               *([None] * 9)) == -1


def test_alias_check_covers_the_outputs():
    cm = p_basic_model(16)._cmodel()
    args = (ctypes.byref(cm), P[0], P[1], P[2], None, 2, 3, 4, 4, 0, P[3], P[4], P[5], P[6], P[7],
            P[8], P[9], P[10], None)
    _hip.check_aliases("smcdet_forced_photometry", args)
    bad = list(args)
    bad[17] = P[3]  # cov in the fluxes buffer
    with pytest.raises(ValueError, match="argument 10"):
        _hip.check_aliases("smcdet_forced_photometry", tuple(bad))


def test_params_are_the_issue_s():
    assert M71["psf_radius"] == 8 and O.E == 32 * 2.0 ** -24
