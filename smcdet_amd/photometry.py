"""Forced PSF photometry: a joint flux solve at fixed positions, with
Cramér–Rao errors.

`extract` reports isophotal fluxes: what an 8x8 tile, and then an isophote,
captures of a star's PSF (0.91 of it at the tile centre of the M71 model, 0.56
at pixel (1, 1): 0.10 and 0.64 mag lost before any isophote).  Here positions
are held fixed, the image model is given, and the fluxes of all sources of a
tile are solved jointly -- they blend -- by iteratively reweighted least
squares, each with its Cramér–Rao error: the crowded-field baseline
(DAOPHOT-style flux fitting) next to `extract`, and the data-only flux of a
condensed posterior detection.  Positions are never fitted.

Every (image, position list) pair is one wavefront of
`smcdet_forced_photometry` (include/smcdet_hip.h holds the method's
definition).  The Poisson `ImageModel` is taken as Gaussian
with variance equal to the rate, an approximation of its likelihood.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _hip
from ._hip import check, dev_f32, lib, ptr, stream_of
from .extract import Extraction, GridExtraction, _image_shape, _per_image


class Photometry(NamedTuple):
    """On the device; [T,K] for locs [T,K,2], [T,G,K] for locs [T,G,K,2].
    fluxes (nmgy) and flux_err float64: 0 and NaN in a skipped slot (past the
    count, or a location that is not finite), NaN and NaN for a dropped source
    (status bit 1) and for every source of a singular problem (status bit 2).
    background, chi2 float64 and n_pixels, n_free, status int32: [T] or [T,G].
    cov: [...,K,K] float64 or None."""
    fluxes: torch.Tensor
    flux_err: torch.Tensor
    background: torch.Tensor
    chi2: torch.Tensor
    n_pixels: torch.Tensor
    n_free: torch.Tensor
    status: torch.Tensor
    cov: Optional[torch.Tensor]


def _check_model(ImageModel, H, W):
    if not hasattr(ImageModel, "_cmodel"):
        raise TypeError("ImageModel must be a smcdet_amd.images image model")
    mh, mw = int(ImageModel.image_height), int(ImageModel.image_width)
    if (mh, mw) != (H, W):
        raise ValueError(f"the image model is {mh}x{mw}, the images are {H}x{W}")
    R = int(ImageModel.psf_radius)
    if not 0 <= R <= _hip.MAX_PSF_RADIUS:
        raise ValueError(f"psf_radius {R} outside 0..{_hip.MAX_PSF_RADIUS}")


def _check_n_iter(n_iter):
    if not isinstance(n_iter, int) or isinstance(n_iter, bool):
        raise TypeError("n_iter must be an int")
    if not 1 <= n_iter <= _hip.PHOT_MAX_ITER:
        raise ValueError(f"n_iter = {n_iter} outside 1..{_hip.PHOT_MAX_ITER}")


def _check_lists(counts, locs, T):
    """Shapes of counts and locs against T images; returns (G, K, grid)."""
    if not isinstance(locs, torch.Tensor) or not isinstance(counts, torch.Tensor):
        raise TypeError("counts and locs must be torch.Tensors")
    if locs.dim() not in (3, 4) or locs.shape[-1] != 2:
        raise ValueError(f"locs must be [T,K,2] or [T,G,K,2], got {tuple(locs.shape)}")
    grid = locs.dim() == 4
    G = locs.shape[1] if grid else 1
    K = locs.shape[-2]
    if locs.shape[0] != T or G < 1:
        raise ValueError(f"locs {tuple(locs.shape)} do not go with {T} images")
    if not 1 <= K <= _hip.PHOT_MAX_SOURCES:
        raise ValueError(f"forced_photometry: {K} position slots outside "
                         f"1..{_hip.PHOT_MAX_SOURCES} (a problem's normal matrix lives in one "
                         "wavefront's LDS slab)")
    if tuple(counts.shape) != tuple(locs.shape[:-2]):
        raise ValueError(f"counts {tuple(counts.shape)} do not go with locs {tuple(locs.shape)}")
    if counts.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"counts must be int32 or int64 (got {counts.dtype})")
    if T * G > 0x7fffffff:
        raise ValueError(f"forced_photometry: {T * G} problems exceed one launch")
    return G, K, grid


def _launch(images, counts, locs, cm, background, n_iter, fit_background, covariance):
    """images [T,H,W], counts [T,G] int32, locs [T,G,K,2] float32, contiguous,
    on the device; background [T] on the device or None.  The raw [T,G,...]
    outputs."""
    T, G, K = locs.shape[:3]
    dev = images.device
    f64 = dict(device=dev, dtype=torch.float64)
    i32 = dict(device=dev, dtype=torch.int32)
    fluxes, flux_err = torch.empty(T, G, K, **f64), torch.empty(T, G, K, **f64)
    bg_out, chi2 = torch.empty(T, G, **f64), torch.empty(T, G, **f64)
    n_pixels, n_free, status = (torch.empty(T, G, **i32) for _ in range(3))
    cov = torch.empty(T, G, K, K, **f64) if covariance else None
    flags = _hip.PHOT_FIT_BACKGROUND if fit_background else 0
    check(lib().smcdet_forced_photometry(
        _hip.ref(cm), ptr(images), ptr(counts), ptr(locs), ptr(background), T, G, K, n_iter,
        flags, ptr(fluxes), ptr(flux_err), ptr(bg_out), ptr(chi2), ptr(n_pixels), ptr(n_free),
        ptr(status), ptr(cov), stream_of(images)), "smcdet_forced_photometry")
    return Photometry(fluxes, flux_err, bg_out, chi2, n_pixels, n_free, status, cov)


def _squeeze(p, grid):
    if grid:
        return p
    return Photometry(*(None if x is None else x[:, 0] for x in p))


def forced_photometry(images, counts, locs, ImageModel, *, background=None,
                      fit_background=False, n_iter=4, covariance=False):
    """The fluxes (nmgy) that images [T,H,W] (or [H,W]) assign to the sources
    at locs [T,K,2] or [T,G,K,2] (row, column; pixel (i, j) centred at
    (i + 0.5, j + 0.5)), the first counts [T] or [T,G] of each list, under
    ImageModel (M71ImageModel, or ImageModel taken as Gaussian with variance =
    rate); the G lists of an image share it.  background: None (the model's),
    a float or [T], > 0; fit_background: the background is a free parameter
    (the given one still floors the variances at background / 4).  n_iter
    (1..16) reweighting iterations.  Returns Photometry; see its fields for
    skipped, dropped and singular sources.  Everything runs on the device."""
    images = _image_shape(images, "forced_photometry")
    T, H, W = images.shape
    G, K, grid = _check_lists(counts, locs, T)
    _check_n_iter(n_iter)
    _check_model(ImageModel, H, W)
    if background is not None:
        background = _per_image(background, "background", T, positive=True)
    elif not float(ImageModel.background) > 0:
        raise ValueError("the image model's background must be positive")
    images = dev_f32(images, "images")  # host tensors are refused: there is no CPU path
    locs = dev_f32(locs, "locs").reshape(T, G, K, 2)
    if not counts.is_cuda:
        raise RuntimeError(f"counts must live on a HIP device (got {counts.device})")
    counts = counts.to(torch.int32).reshape(T, G).contiguous()
    if background is not None:
        background = background.to(images.device)
    p = _launch(images, counts, locs, ImageModel._cmodel(), background, n_iter,
                bool(fit_background), bool(covariance))
    return _squeeze(p, grid)


def _psf_fluxes(phot_fluxes, fluxes):
    """The PSF fluxes as float32 where the solve gave one, else the given ones."""
    return torch.where(torch.isfinite(phot_fluxes), phot_fluxes.to(fluxes.dtype), fluxes)


def photometry_of(extraction, images, ImageModel, **kw):
    """Forced photometry at the positions of an Extraction or GridExtraction.
    Returns (the extraction with its fluxes replaced by the PSF fluxes in
    nmgy, order unchanged; the Photometry).  A detection whose solve failed
    (dropped, or in a singular problem) keeps its isophotal flux."""
    if not isinstance(extraction, (Extraction, GridExtraction)):
        raise TypeError("photometry_of takes an Extraction or a GridExtraction")
    phot = forced_photometry(images, extraction.counts, extraction.locs, ImageModel, **kw)
    return extraction._replace(fluxes=_psf_fluxes(phot.fluxes, extraction.fluxes)), phot


def photometry_condensed(condensed, images, ImageModel, min_prob=0.5, **kw):
    """Forced photometry at the posterior mean positions of the detections
    `condensed.as_catalog(min_prob)` keeps (at most 32 per tile).  Returns
    (Photometry [T,K'], z [T,K']): z = (PSF flux - posterior mean flux) /
    flux_err per detection, the data-only flux set against the posterior's;
    NaN where there is no detection or no solve."""
    counts, locs, fluxes = condensed.as_catalog(min_prob)
    counts, locs, fluxes = counts[:, 0], locs[:, 0], fluxes[:, 0]
    K = min(locs.shape[1], _hip.PHOT_MAX_SOURCES)
    if locs.shape[1] > K and int(counts.max()) > K:
        raise ValueError(f"photometry_condensed: a tile keeps {int(counts.max())} detections, "
                         f"above {K}")
    locs, fluxes = locs[:, :K].contiguous(), fluxes[:, :K]
    phot = forced_photometry(images, counts, locs, ImageModel, **kw)
    kept = torch.arange(K, device=counts.device)[None, :] < counts[:, None]
    z = torch.where(kept, (phot.fluxes - fluxes.double()) / phot.flux_err,
                    torch.full_like(phot.fluxes, float("nan")))
    return phot, z
