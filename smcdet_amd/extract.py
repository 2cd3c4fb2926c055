"""A classical source-extraction baseline on the GPU, with grid-search tuning.

The reference's experiment scripts (experiments/*/run_sep.py) compare the SMC
catalogs with Source Extractor through `sep`, after a grid search of its
hyperparameters for F1 on held-out tiles: 2,380 settings, a Python loop over
settings x tiles with `match_catalogs` after every setting.  Here every
(image, setting) pair is one wavefront of `smcdet_extract`
(include/smcdet_hip.h, which holds the algorithm's definition), its output has
the layout `metrics.match_catalogs` takes as `est_*`, and the whole grid search
is two launches: extract, then match.

This is a multi-threshold detector "after SExtractor / SEP"; it does not claim
parity with `sep`.  Differences from SEP:
  * there is no convolution filter (the reference passes `filter_kernel=None`:
    "no filter works better");
  * the threshold ladder is float32 and exact: r = peak / tau, q = r after
    log2(n) square roots, tau_k = tau_{k-1} * q, no pow / exp / log;
  * the pixel gather is deterministic: synchronous sweeps, an unassigned pixel
    takes the label of its brightest assigned 8-neighbour (SExtractor assigns
    blended pixels with random numbers);
  * cleaning uses each absorber's original profile (absorbing an object
    updates nothing), and the survivors' fluxes and centroids are then summed
    again over their final pixels;
  * one background and one noise level per image (no maps), images of at most
    1,024 pixels, isophotal fluxes and centroids only.
"""
from __future__ import annotations

import itertools
import math
from typing import NamedTuple, Optional

import torch

from . import _hip
from ._hip import check, dev_f32, lib, ptr, stream_of
from .metrics import match_catalogs


class Extraction(NamedTuple):
    """extract: counts [T], locs [T,K,2], fluxes [T,K]; extract_grid: [T,G],
    [T,G,K,2], [T,G,K].  n_found: the detections before the cap K; segmap
    (or None): [..., H, W] int32, 0 or the 1-based rank of the pixel's object."""
    counts: torch.Tensor
    locs: torch.Tensor
    fluxes: torch.Tensor
    n_found: torch.Tensor
    segmap: Optional[torch.Tensor]


class GridExtraction(NamedTuple):
    counts: torch.Tensor
    locs: torch.Tensor
    fluxes: torch.Tensor
    n_found: torch.Tensor
    segmap: Optional[torch.Tensor]
    settings: torch.Tensor  # [G,4] float64 (cpu): thresh, minarea, deblend_cont, clean_param


class Tuning(NamedTuple):
    f1: torch.Tensor        # [G] float32, on the device
    best: dict              # the first maximum in grid order
    best_index: int
    settings: torch.Tensor  # [G,4] float64 (cpu)


def _image_shape(images, where="extract"):
    """Type and shape of `images` (checked before anything needs a device)."""
    if not isinstance(images, torch.Tensor):
        raise TypeError("images must be a torch.Tensor")
    if images.dim() == 2:
        images = images[None]
    if images.dim() != 3 or images.shape[0] < 1:
        raise ValueError(f"images must be [T,H,W] or [H,W], got {tuple(images.shape)}")
    H, W = images.shape[1:]
    if H < 1 or W < 1 or H * W > _hip.EXTRACT_MAX_PIXELS:
        raise ValueError(f"{where}: a {H}x{W} image has {H * W} pixels, outside "
                         f"1..{_hip.EXTRACT_MAX_PIXELS} (a problem lives in one wavefront's LDS "
                         "slab)")
    return images


def _per_image(x, name, T, positive):
    if isinstance(x, torch.Tensor):
        if x.dim() > 1 or (x.dim() == 1 and x.shape[0] != T):
            raise ValueError(f"{name} must be a float or a [T] tensor, got {tuple(x.shape)}")
        x = x.detach().to(dtype=torch.float32).reshape(-1).expand(T) if x.numel() == 1 else \
            x.detach().to(dtype=torch.float32)
    else:
        x = torch.full((T,), float(x), dtype=torch.float32)
    if not bool(torch.isfinite(x).all()) or (positive and not bool((x > 0).all())):
        raise ValueError(f"{name} must be finite" + (" and positive" if positive else ""))
    return x.contiguous()


def _axis(x, name):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().reshape(-1).tolist()
    elif not isinstance(x, (list, tuple)):
        try:
            x = list(x)
        except TypeError:
            x = [x]
    if len(x) < 1:
        raise ValueError(f"{name} is empty")
    return [float(v) for v in x]


def _check_settings(thresh, minarea, cont, beta, deblend_nthresh, K):
    if not isinstance(deblend_nthresh, int) or isinstance(deblend_nthresh, bool):
        raise TypeError("deblend_nthresh must be an int")
    if not 1 <= deblend_nthresh <= 64 or deblend_nthresh & (deblend_nthresh - 1):
        raise ValueError(f"deblend_nthresh = {deblend_nthresh} must be a power of two in 1..64")
    if not isinstance(K, int) or not 1 <= K <= _hip.MATCH_MAX_SOURCES:
        raise ValueError(f"max_detections = {K} outside 1..{_hip.MATCH_MAX_SOURCES} (the source "
                         "slots of match_catalogs)")
    for v in thresh:
        if not math.isfinite(v) or v <= 0:
            raise ValueError(f"thresh = {v} must be finite and positive")
    for v in minarea:
        if v != int(v) or v < 1:
            raise ValueError(f"minarea = {v} must be an integer >= 1")
    for v in cont:
        if not math.isfinite(v) or v < 0:
            raise ValueError(f"deblend_cont = {v} must be finite and >= 0")
    for v in beta:
        if not math.isfinite(v) or v < 0:
            raise ValueError(f"clean_param = {v} must be finite and >= 0 (0: no cleaning)")


def _launch(images, background, sigma, settings, deblend_nthresh, K, segmentation_map):
    """settings: [G,4] float64 cpu.  Returns the raw [T,G,...] outputs."""
    T, H, W = images.shape
    dev = images.device
    G = settings.shape[0]
    th = settings[:, 0].to(torch.float32).to(dev).contiguous()
    ma = settings[:, 1].to(torch.int32).to(dev).contiguous()
    dc = settings[:, 2].to(torch.float32).to(dev).contiguous()
    cp = settings[:, 3].to(torch.float32).to(dev).contiguous()
    counts = torch.empty(T, G, device=dev, dtype=torch.int32)
    locs = torch.empty(T, G, K, 2, device=dev, dtype=torch.float32)
    fluxes = torch.empty(T, G, K, device=dev, dtype=torch.float32)
    n_found = torch.empty(T, G, device=dev, dtype=torch.int32)
    seg = torch.empty(T, G, H, W, device=dev, dtype=torch.int32) if segmentation_map else None
    check(lib().smcdet_extract(ptr(images), ptr(background), ptr(sigma), T, H, W, ptr(th), ptr(ma),
                               ptr(dc), ptr(cp), G, deblend_nthresh, K, ptr(counts), ptr(locs),
                               ptr(fluxes), ptr(n_found), ptr(seg), stream_of(images)),
          "smcdet_extract")
    return counts, locs, fluxes, n_found, seg


def _flux_scale(flux_scale):
    flux_scale = float(flux_scale)
    if not math.isfinite(flux_scale) or flux_scale <= 0:
        raise ValueError(f"flux_scale = {flux_scale} must be finite and positive")
    return flux_scale


def _prepare(images, background, sigma, thresh, minarea, deblend_cont, clean, clean_param,
             deblend_nthresh, max_detections, flux_scale):
    """Host-side validation (shapes and settings first, the device last), then
    the device tensors and the [G,4] table of settings."""
    images = _image_shape(images)
    T = images.shape[0]
    background = _per_image(background, "background", T, positive=False)
    sigma = _per_image(sigma, "sigma", T, positive=True)
    th, ma, dc = _axis(thresh, "thresh"), _axis(minarea, "minarea"), \
        _axis(deblend_cont, "deblend_cont")
    cp = _axis(clean_param, "clean_param") if clean else [0.0]
    _check_settings(th, ma, dc, cp, deblend_nthresh, max_detections)
    flux_scale = _flux_scale(flux_scale)
    images = dev_f32(images, "images")  # host tensors are refused: there is no CPU path
    settings = torch.tensor(list(itertools.product(th, ma, dc, cp)), dtype=torch.float64)
    return images, background.to(images.device), sigma.to(images.device), settings, flux_scale


def extract_grid(images, background, sigma, thresh, minarea=(5,), deblend_nthresh=32,
                 deblend_cont=(0.005,), clean=True, clean_param=(1.0,), max_detections=16,
                 flux_scale=1.0, segmentation_map=False):
    """Every image under every setting of the Cartesian product thresh x
    minarea x deblend_cont x clean_param (in this order, the last axis
    fastest), in one launch.  Returns GridExtraction: counts [T,G], locs
    [T,G,K,2] (NaN past the count), fluxes [T,G,K] (0 past the count; divided
    by flux_scale, the scripts' adu_per_nmgy), n_found [T,G], segmap
    [T,G,H,W] or None, settings [G,4].  clean=False passes clean_param 0."""
    images, background, sigma, settings, flux_scale = _prepare(
        images, background, sigma, thresh, minarea, deblend_cont, clean, clean_param,
        deblend_nthresh, max_detections, flux_scale)
    counts, locs, fluxes, n_found, seg = _launch(images, background, sigma, settings,
                                                 deblend_nthresh, max_detections,
                                                 segmentation_map)
    if flux_scale != 1.0:
        fluxes = fluxes / flux_scale
    return GridExtraction(counts, locs, fluxes, n_found, seg, settings)


def extract(images, background, sigma, thresh, minarea=5, deblend_nthresh=32, deblend_cont=0.005,
            clean=True, clean_param=1.0, max_detections=16, flux_scale=1.0,
            segmentation_map=False):
    """Detections of images [T,H,W] (or [H,W]) under one setting; the arguments
    are sep.extract's where they share a name (thresh in units of sigma, no
    filter).  background and sigma: floats or [T].  Returns Extraction(counts
    [T], locs [T,K,2], fluxes [T,K], n_found [T], segmap [T,H,W] or None) on
    the device, brightest first; locs are (row, column) with pixel (i, j)
    centred at (i + 0.5, j + 0.5), the SMC convention."""
    for name, v in (("thresh", thresh), ("minarea", minarea), ("deblend_cont", deblend_cont),
                    ("clean_param", clean_param)):
        if isinstance(v, (list, tuple, torch.Tensor)):
            raise TypeError(f"extract: {name} must be a number (extract_grid takes sequences)")
    r = extract_grid(images, background, sigma, [thresh], [minarea], deblend_nthresh,
                     [deblend_cont], clean, [clean_param], max_detections, flux_scale,
                     segmentation_map)
    return Extraction(r.counts[:, 0], r.locs[:, 0], r.fluxes[:, 0], r.n_found[:, 0],
                      None if r.segmap is None else r.segmap[:, 0])


def tune(images, background, sigma, true_counts, true_locs, true_fluxes, thresh, minarea=(5,),
         deblend_cont=(0.005,), clean_param=(1.0,), deblend_nthresh=32, clean=True,
         max_detections=16, locs_tol=0.5, mags_tol=0.5, mag_bins=(14.0,), flux_scale=1.0,
         max_bytes=1 << 30, flux="isophotal", image_model=None):
    """The scripts' grid search: extract_grid on held-out images, one
    match_catalogs(..., None, ...) against the truth (true_counts [T],
    true_locs [T,St,2], true_fluxes [T,St]), and per setting the F1 of the last
    magnitude bin pooled over the images.  Returns Tuning(f1 [G], best, ...):
    best is the first maximum in grid order.  Everything runs on the device;
    the grid is cut into chunks of settings whose outputs stay below max_bytes.
    flux="psf": the detections are scored with their forced PSF fluxes under
    image_model (photometry.photometry_of: one more launch per chunk between
    extract and match; nmgy, so flux_scale applies only to the isophotal flux
    a failed solve falls back to; max_detections <= 32)."""
    if int(max_bytes) < 1:
        raise ValueError("max_bytes must be positive")
    if flux not in ("isophotal", "psf"):
        raise ValueError(f"flux = {flux!r} must be 'isophotal' or 'psf'")
    if flux == "psf" and image_model is None:
        raise ValueError("flux='psf' needs image_model")
    if flux == "isophotal" and image_model is not None:
        raise ValueError("image_model is used only with flux='psf'")
    if flux == "psf":
        from . import photometry
        photometry._check_model(image_model, *_image_shape(images).shape[1:])
        if isinstance(max_detections, int) and max_detections > _hip.PHOT_MAX_SOURCES:
            raise ValueError(f"flux='psf': max_detections = {max_detections} above "
                             f"{_hip.PHOT_MAX_SOURCES}")
        if not float(image_model.background) > 0:
            raise ValueError("the image model's background must be positive")
    images, background, sigma, settings, flux_scale = _prepare(
        images, background, sigma, thresh, minarea, deblend_cont, clean, clean_param,
        deblend_nthresh, max_detections, flux_scale)
    T = images.shape[0]
    G = settings.shape[0]
    K = max_detections
    bins = torch.as_tensor(mag_bins, dtype=torch.float32).reshape(-1)
    # counts, n_found, locs, fluxes of extract and the four float32 [.,B] tables of the matching
    per_setting = T * (8 + 12 * K + 16 * bins.numel())
    if flux == "psf":
        cm = image_model._cmodel()
        # fluxes and errors (float64), background, chi2, three int32, the replaced fluxes
        per_setting += T * (16 * K + 16 + 12 + 4 * K)
    chunk = max(1, min(G, int(max_bytes) // per_setting))
    f1 = torch.empty(G, device=images.device, dtype=torch.float32)
    for g0 in range(0, G, chunk):
        counts, locs, fluxes, _, _ = _launch(images, background, sigma, settings[g0:g0 + chunk],
                                             deblend_nthresh, K, False)
        if flux_scale != 1.0:
            fluxes = fluxes / flux_scale
        if flux == "psf":
            phot = photometry._launch(images, counts, locs, cm, None, 4, False, False)
            fluxes = photometry._psf_fluxes(phot.fluxes, fluxes)
        tt, tm, et, em = match_catalogs(true_counts, true_locs, true_fluxes, counts, locs, fluxes,
                                        None, locs_tol, mags_tol, bins)
        # compute_precision_recall_f1 per setting: pooled over the images, last bin
        precision = (em.sum(0) / et.sum(0)).nan_to_num(0)
        recall = (tm.sum(0) / tt.sum(0)).nan_to_num(0)
        f1[g0:g0 + chunk] = ((2 * precision * recall) / (precision + recall)).nan_to_num(0)[:, -1]
    best = int((f1 == f1.max()).nonzero()[0])  # the first maximum in grid order
    s = settings[best].tolist()
    return Tuning(f1, dict(thresh=s[0], minarea=int(s[1]), deblend_cont=s[2], clean_param=s[3]),
                  best, settings)
