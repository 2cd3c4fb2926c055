"""A PSF-fitting detector: significance map, peaks and recentring.

`extract` is an isophotal detector and `photometry` solves fluxes at positions
somebody else supplies.  This module is the rest of the crowded-field
baseline, DAOPHOT's loop: find peaks with the PSF as matched filter, fit,
subtract, find again in the residual, refit.  Per round: one find launch
(`smcdet_psf_find`: the significance map of the residual, its peaks, a
parabolic refinement); `sweeps` times a joint flux solve (`photometry`) and one
Jacobi sweep of leave-one-out position moves (`smcdet_psf_recentre`: each
source goes to the maximum of the significance of the residual with that
source put back); one more solve; and a prune on flux / flux_err.
include/smcdet_hip.h holds the definitions; DESIGN.md §19 the bounds and what
was measured.

The method's limit: two stars closer than about a pixel share one
matched-filter peak and stay one detection (a pair 0.8 px apart is found as
one source with the summed flux).  That is the samplers' territory.  Nothing
merges or splits detections, positions move on a grid with a parabola and not
by Newton steps, and there are no sharpness or roundness cuts.
"""
from __future__ import annotations

import itertools
import math
from typing import NamedTuple

import torch

from . import _hip, photometry
from ._hip import check, dev_f32, lib, ptr, stream_of
from .extract import Tuning, _axis, _image_shape, _per_image
from .metrics import compute_precision_recall_f1, match_catalogs


class Found(NamedTuple):
    """On the device; [T] / [T,K] for find, [T,G] / [T,G,K] for find_grid.
    counts int32; locs [...,K,2] float32 (NaN past the count); fluxes float32
    nmgy (0 past the count) and flux_err float64 (NaN past it) of the last
    solve; snr float32: the last recentre's leave-one-out value; n_found int32:
    the peaks of the last round's find before the cap; status int32: the last
    solve's (photometry's bits), so a singular problem is visible."""
    counts: torch.Tensor
    locs: torch.Tensor
    fluxes: torch.Tensor
    flux_err: torch.Tensor
    snr: torch.Tensor
    n_found: torch.Tensor
    status: torch.Tensor


class GridFound(NamedTuple):
    counts: torch.Tensor
    locs: torch.Tensor
    fluxes: torch.Tensor
    flux_err: torch.Tensor
    snr: torch.Tensor
    n_found: torch.Tensor
    status: torch.Tensor
    settings: torch.Tensor  # [G,3] float64 (cpu): thresh, nms_radius, min_snr


def _int_in(v, name, lo, hi):
    if not isinstance(v, int) or isinstance(v, bool):
        raise TypeError(f"{name} must be an int")
    if not lo <= v <= hi:
        raise ValueError(f"{name} = {v} outside {lo}..{hi}")


def _check_cells(cells, H, W):
    _int_in(cells, "cells", 1, _hip.FIND_MAX_CELLS_PER_PIXEL)
    if cells * H * cells * W > _hip.FIND_MAX_CELLS:
        raise ValueError(f"a {H}x{W} image at {cells} cells per pixel has {cells * cells * H * W} "
                         f"cells, above {_hip.FIND_MAX_CELLS} (the map lives in LDS)")


def _background(background, ImageModel, T):
    if background is not None:
        return _per_image(background, "background", T, positive=True)
    if not float(ImageModel.background) > 0:
        raise ValueError("the image model's background must be positive")
    return None


def _find_launch(images, cm, background, counts, locs, fluxes, G, K, cells, thresh, nms, min_sep,
                 want_map):
    """One smcdet_psf_find launch; counts / locs / fluxes all None for empty
    lists.  Returns (counts_out, locs_out, snr_out, flux_hat, n_found, map)."""
    T, H, W = images.shape
    dev = images.device
    counts_out = torch.empty(T, G, device=dev, dtype=torch.int32)
    n_found = torch.empty(T, G, device=dev, dtype=torch.int32)
    locs_out = torch.empty(T, G, K, 2, device=dev, dtype=torch.float32)
    snr_out = torch.empty(T, G, K, device=dev, dtype=torch.float32)
    flux_hat = torch.empty(T, G, K, device=dev, dtype=torch.float32)
    smap = torch.empty(T, G, cells * H, cells * W, device=dev, dtype=torch.float32) \
        if want_map else None
    check(lib().smcdet_psf_find(
        _hip.ref(cm), ptr(images), ptr(background), ptr(counts), ptr(locs), ptr(fluxes), T, G, K,
        cells, ptr(thresh), ptr(nms), float(min_sep), ptr(counts_out), ptr(locs_out), ptr(snr_out),
        ptr(flux_hat), ptr(n_found), ptr(smap), stream_of(images)), "smcdet_psf_find")
    return counts_out, locs_out, snr_out, flux_hat, n_found, smap


def _recentre_launch(images, cm, background, counts, locs, fluxes, half, step):
    """One smcdet_psf_recentre launch: (locs_out, snr_out)."""
    T, G, K = locs.shape[:3]
    locs_out = torch.empty_like(locs)
    snr_out = torch.empty(T, G, K, device=locs.device, dtype=torch.float32)
    check(lib().smcdet_psf_recentre(
        _hip.ref(cm), ptr(images), ptr(background), ptr(counts), ptr(locs), ptr(fluxes), T, G, K,
        half, float(step), ptr(locs_out), ptr(snr_out), stream_of(images)), "smcdet_psf_recentre")
    return locs_out, snr_out


def significance_map(images, ImageModel, counts=None, locs=None, fluxes=None, *, background=None,
                     cells=2):
    """The matched-filter significance of images [T,H,W] (or [H,W]) minus the
    background and, when given, the sources at locs [T,K,2] or [T,G,K,2] with
    fluxes [T,K] or [T,G,K] (nmgy; the first counts [T] or [T,G] of each list,
    slots that are not finite ignored): snr = a / sqrt(d) at `cells` x `cells`
    candidate positions per pixel, cell (i, j) at ((i + 1/2) / cells, (j + 1/2)
    / cells).  Returns float32 [T,cH,cW], or [T,G,cH,cW] for grid lists."""
    images = _image_shape(images, "significance_map")
    T, H, W = images.shape
    given = [x is not None for x in (counts, locs, fluxes)]
    if any(given) and not all(given):
        raise ValueError("counts, locs and fluxes are given together or not at all")
    G, K, grid = (1, 1, False)
    if all(given):
        G, K, grid = photometry._check_lists(counts, locs, T)
        if not isinstance(fluxes, torch.Tensor) or tuple(fluxes.shape) != tuple(locs.shape[:-1]):
            raise ValueError(f"fluxes must be a tensor of shape {tuple(locs.shape[:-1])}")
    photometry._check_model(ImageModel, H, W)
    _check_cells(cells, H, W)
    background = _background(background, ImageModel, T)
    images = dev_f32(images, "images")  # host tensors are refused: there is no CPU path
    dev = images.device
    if all(given):
        locs = dev_f32(locs, "locs").reshape(T, G, K, 2)
        fluxes = dev_f32(fluxes, "fluxes").reshape(T, G, K)
        if not counts.is_cuda:
            raise RuntimeError(f"counts must live on a HIP device (got {counts.device})")
        counts = counts.to(torch.int32).reshape(T, G).contiguous()
    if background is not None:
        background = background.to(dev)
    thresh = torch.full((G,), float("inf"), device=dev, dtype=torch.float32)
    nms = torch.zeros(G, device=dev, dtype=torch.int32)
    smap = _find_launch(images, ImageModel._cmodel(), background, counts, locs, fluxes, G, K,
                        cells, thresh, nms, 0.0, True)[5]
    return smap if grid else smap[:, 0]


def _settings(thresh, nms_radius, min_snr):
    th, nr, ms = _axis(thresh, "thresh"), _axis(nms_radius, "nms_radius"), \
        _axis(min_snr, "min_snr")
    for v in th:
        if not math.isfinite(v):
            raise ValueError(f"thresh = {v} must be finite")
    for v in nr:
        if v != int(v) or not 0 <= v <= _hip.FIND_MAX_NMS:
            raise ValueError(f"nms_radius = {v} must be an integer in 0..{_hip.FIND_MAX_NMS}")
    for v in ms:
        if not math.isfinite(v):
            raise ValueError(f"min_snr = {v} must be finite")
    return torch.tensor(list(itertools.product(th, nr, ms)), dtype=torch.float64)


def _prepare(images, ImageModel, thresh, nms_radius, min_snr, cells, rounds, sweeps, step, half,
             min_sep, max_detections, background, where):
    """Host-side validation (shapes and settings first, the device last)."""
    images = _image_shape(images, where)
    T, H, W = images.shape
    photometry._check_model(ImageModel, H, W)
    _check_cells(cells, H, W)
    _int_in(rounds, "rounds", 1, 64)
    _int_in(sweeps, "sweeps", 1, 64)
    _int_in(half, "half", 1, _hip.FIND_MAX_HALF)
    _int_in(max_detections, "max_detections", 1, _hip.PHOT_MAX_SOURCES)
    step, min_sep = float(step), float(min_sep)
    if not (math.isfinite(step) and step > 0):
        raise ValueError(f"step = {step} must be positive and finite")
    if not (math.isfinite(min_sep) and min_sep >= 0):
        raise ValueError(f"min_sep = {min_sep} must be finite and >= 0")
    settings = _settings(thresh, nms_radius, min_snr)
    background = _background(background, ImageModel, T)
    images = dev_f32(images, "images")  # host tensors are refused: there is no CPU path
    if background is not None:
        background = background.to(images.device)
    return images, background, settings, step, min_sep


def _run(images, cm, background, settings, cells, rounds, sweeps, step, half, min_sep, K):
    """The rounds for the settings [G,3]: fixed loop counts, no host
    synchronisation.  A round whose find adds no peak still runs its solves,
    moves and prune on the sources already listed; only lists that are still
    empty pass through it unchanged."""
    T = images.shape[0]
    G = settings.shape[0]
    dev = images.device
    thresh = settings[:, 0].to(torch.float32).to(dev).contiguous()
    nms = settings[:, 1].to(torch.int32).to(dev).contiguous()
    min_snr = settings[:, 2].to(dev)[None, :, None]
    slot = torch.arange(K, device=dev)[None, None, :]
    counts = torch.zeros(T, G, device=dev, dtype=torch.int32)
    locs = torch.full((T, G, K, 2), float("nan"), device=dev, dtype=torch.float32)
    fluxes = torch.zeros(T, G, K, device=dev, dtype=torch.float32)
    flux_err = snr = n_found = status = None
    for _ in range(rounds):
        counts, locs, _, _, n_found, _ = _find_launch(images, cm, background, counts, locs, fluxes,
                                                      G, K, cells, thresh, nms, min_sep, False)
        for _ in range(sweeps):
            phot = photometry._launch(images, counts, locs, cm, background, 4, False, False)
            locs, snr = _recentre_launch(images, cm, background, counts, locs,
                                         phot.fluxes.to(torch.float32), half, step)
        phot = photometry._launch(images, counts, locs, cm, background, 4, False, False)
        status = phot.status
        # the prune, a stable compaction: kept sources first, in slot order
        keep = (slot < counts[..., None]) & torch.isfinite(phot.fluxes) & \
            torch.isfinite(phot.flux_err) & (phot.fluxes / phot.flux_err >= min_snr)
        order = torch.sort((~keep).to(torch.int8), dim=-1, stable=True).indices
        counts = keep.sum(-1, dtype=torch.int32)
        kept = slot < counts[..., None]
        locs = torch.where(kept[..., None], locs.gather(2, order[..., None].expand(-1, -1, -1, 2)),
                           torch.full_like(locs, float("nan"))).contiguous()
        fluxes = torch.where(kept, phot.fluxes.gather(2, order).to(torch.float32),
                             torch.zeros_like(fluxes)).contiguous()
        flux_err = torch.where(kept, phot.flux_err.gather(2, order),
                               torch.full_like(phot.flux_err, float("nan")))
        snr = torch.where(kept, snr.gather(2, order), torch.full_like(snr, float("nan")))
    return counts, locs, fluxes, flux_err, snr, n_found, status


def find_grid(images, ImageModel, thresh, nms_radius=(1,), min_snr=(3.0,), *, cells=2, rounds=3,
              sweeps=4, step=0.25, half=2, min_sep=0.5, max_detections=16, background=None):
    """Every image under every setting of the Cartesian product thresh x
    nms_radius x min_snr (in this order, the last axis fastest).  thresh: the
    significance a map peak needs; nms_radius (cells, 0..16): a peak beats
    every cell this close; min_snr: the flux / flux_err a source needs to
    survive a round.  cells (1..4) candidate positions per pixel and axis;
    `rounds` rounds of find, `sweeps` x (flux solve, recentre on the (2 half +
    1)^2 grid of spacing `step` px), solve and prune; a new peak lies more
    than min_sep px (Chebyshev) from every listed source.  background: None
    (the model's), a float or [T].  Returns GridFound on the device."""
    images, background, settings, step, min_sep = _prepare(
        images, ImageModel, thresh, nms_radius, min_snr, cells, rounds, sweeps, step, half,
        min_sep, max_detections, background, "find_grid")
    out = _run(images, ImageModel._cmodel(), background, settings, cells, rounds, sweeps, step,
               half, min_sep, max_detections)
    return GridFound(*out, settings)


def find(images, ImageModel, thresh, nms_radius=1, min_snr=3.0, **kw):
    """find_grid under one setting: Found with [T] / [T,K] fields."""
    for name, v in (("thresh", thresh), ("nms_radius", nms_radius), ("min_snr", min_snr)):
        if isinstance(v, (list, tuple, torch.Tensor)):
            raise TypeError(f"find: {name} must be a number (find_grid takes sequences)")
    r = find_grid(images, ImageModel, [thresh], [nms_radius], [min_snr], **kw)
    return Found(*(x[:, 0] for x in r[:7]))


def tune(images, ImageModel, true_counts, true_locs, true_fluxes, thresh, nms_radius=(1,),
         min_snr=(3.0,), *, cells=2, rounds=3, sweeps=4, step=0.25, half=2, min_sep=0.5,
         max_detections=16, background=None, locs_tol=0.5, mags_tol=0.5, mag_bins=(14.0,),
         max_bytes=1 << 30):
    """extract.tune's grid search over this detector's settings: find_grid on
    held-out images, one match_catalogs(..., None, ...) against the truth and
    per setting the F1 of the last magnitude bin pooled over the images.
    Returns extract.Tuning(f1 [G], best, best_index, settings [G,3]): best is
    the first maximum in grid order.  The grid is cut into chunks of settings
    whose tensors stay below max_bytes."""
    if int(max_bytes) < 1:
        raise ValueError("max_bytes must be positive")
    images, background, settings, step, min_sep = _prepare(
        images, ImageModel, thresh, nms_radius, min_snr, cells, rounds, sweeps, step, half,
        min_sep, max_detections, background, "tune")
    T = images.shape[0]
    G = settings.shape[0]
    K = max_detections
    bins = torch.as_tensor(mag_bins, dtype=torch.float32).reshape(-1)
    # two generations of counts, locs, fluxes, snr; the solve's float64 fluxes and errors and
    # its per-problem outputs; the prune's mask and order; the matching's four tables
    per_setting = T * (2 * (8 + 16 * K) + 16 * K + 28 + 9 * K + 16 * bins.numel())
    chunk = max(1, min(G, int(max_bytes) // per_setting))
    cm = ImageModel._cmodel()
    f1 = torch.empty(G, device=images.device, dtype=torch.float32)
    for g0 in range(0, G, chunk):
        counts, locs, fluxes = _run(images, cm, background, settings[g0:g0 + chunk], cells, rounds,
                                    sweeps, step, half, min_sep, K)[:3]
        tt, tm, et, em = match_catalogs(true_counts, true_locs, true_fluxes, counts, locs, fluxes,
                                        None, locs_tol, mags_tol, bins)
        f1[g0:g0 + chunk] = compute_precision_recall_f1(tt, tm, et, em)[2][:, -1]
    best = int((f1 == f1.max()).nonzero()[0])  # the first maximum in grid order
    s = settings[best].tolist()
    return Tuning(f1, dict(thresh=s[0], nms_radius=int(s[1]), min_snr=s[2]), best, settings)


def residual_significance(condensed, images, ImageModel, min_prob=0.5, cells=2):
    """The significance map [T,cH,cW] of images with the detections
    `condensed.as_catalog(min_prob)` keeps (at most 32 per tile) subtracted at
    their posterior mean positions and fluxes: what the posterior's detections
    leave unexplained in the data."""
    counts, locs, fluxes = condensed.as_catalog(min_prob)
    counts, locs, fluxes = counts[:, 0], locs[:, 0], fluxes[:, 0]
    K = min(locs.shape[1], _hip.PHOT_MAX_SOURCES)
    if locs.shape[1] > K and int(counts.max()) > K:
        raise ValueError(f"residual_significance: a tile keeps {int(counts.max())} detections, "
                         f"above {K}")
    return significance_map(images, ImageModel, counts, locs[:, :K].contiguous(),
                            fluxes[:, :K].contiguous(), cells=cells)
