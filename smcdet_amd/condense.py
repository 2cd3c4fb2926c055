"""Posterior catalogs condensed into detections with probabilities
(the reference has no counterpart, its notebooks scatter-plot
the sampled locations by hand).

A run leaves N catalogs per tile.  `condense` turns them into one list of
detections per tile, each with the probability that it exists, a position with
its uncertainty and a flux / magnitude with a credible interval:

  1. `source_map`: the posterior source-density map (smcdet_source_map);
  2. `find_seeds`: the peaks of the smoothed map (smcdet_map_peaks);
  3. every catalog's sources are associated with the seeds by the exact
     assignment the metrics use (`metrics.match_catalogs`, the seeds as the
     "true" catalog);
  4. per-seed posterior moments in float64 (smcdet_seed_moments);
  5. the derived fields of `CondensedCatalog`, plain torch in float64.

Everything stays on the device; inputs are HIP tensors laid out as
`metrics.match_catalogs` takes them (kept sources first).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip, metrics
from ._hip import check, dev_f32, lib, ptr, stream_of
from .metrics import _counts_i32

_F32_MAX = float(torch.finfo(torch.float32).max)


@dataclass
class SourceMap:
    """count [T,Gh,Gw]: weight of the counted sources per cell; flux: weight *
    flux per cell (None unless with_flux); outside [T]: weight of the counted
    sources in no cell; box (lo_h, lo_w, hi_h, hi_w) and tile_boxes [T,4] place
    cell (0, 0); total_weight [T] float64: the weight of all N catalogs;
    max_sources: S of the catalogs the map was made from."""
    count: torch.Tensor
    flux: Optional[torch.Tensor]
    outside: torch.Tensor
    box: Tuple[float, float, float, float]
    cells_per_pixel: int
    tile_boxes: Optional[torch.Tensor] = None
    total_weight: Optional[torch.Tensor] = None
    max_sources: Optional[int] = None


@dataclass
class Seeds:
    """n_seeds [T] int32; cell [T,K] int32 (-1 past n_seeds); mass [T,K] (0
    past n_seeds); locs [T,K,2] pixels (NaN past n_seeds)."""
    n_seeds: torch.Tensor
    cell: torch.Tensor
    mass: torch.Tensor
    locs: torch.Tensor


def _box4(box):
    b = tuple(float(x) for x in (box.tolist() if isinstance(box, torch.Tensor) else box))
    if len(b) != 4 or not all(math.isfinite(x) for x in b) or not (b[2] > b[0] and b[3] > b[1]):
        raise ValueError(f"box must be finite (lo_h, lo_w, hi_h, hi_w) with lo < hi, got {b}")
    return b


def _cbox(box):
    return (ctypes.c_float * 4)(*box)


def _check_cells_per_pixel(c, where):
    if not 1 <= c <= _hip.MAP_MAX_CELLS_PER_PIXEL:
        raise ValueError(f"{where}: cells_per_pixel = {c} outside "
                         f"1..{_hip.MAP_MAX_CELLS_PER_PIXEL}")


def _catalogs(counts, locs, fluxes, weights, where):
    locs = dev_f32(locs, "locs")
    fluxes = dev_f32(fluxes, "fluxes")
    if locs.dim() != 4 or locs.shape[-1] != 2:
        raise ValueError(f"{where}: locs must be [T,N,S,2], got {tuple(locs.shape)}")
    T, N, S = locs.shape[:3]
    if tuple(fluxes.shape) != (T, N, S):
        raise ValueError(f"{where}: fluxes has shape {tuple(fluxes.shape)}, expected {(T, N, S)}")
    if T < 1 or N < 1 or S < 1:
        raise ValueError(f"{where}: T = {T}, N = {N}, S = {S} must all be >= 1")
    counts = _counts_i32(counts, "counts", (T, N), locs.device)
    if weights is not None:
        weights = dev_f32(weights, "weights")
        if tuple(weights.shape) != (T, N):
            raise ValueError(f"{where}: weights has shape {tuple(weights.shape)}, "
                             f"expected {(T, N)}")
    return counts, locs, fluxes, weights


def _tile_boxes(tile_boxes, T, where):
    if tile_boxes is None:
        return None
    tile_boxes = dev_f32(tile_boxes, "tile_boxes")
    if tuple(tile_boxes.shape) != (T, 4):
        raise ValueError(f"{where}: tile_boxes has shape {tuple(tile_boxes.shape)}, "
                         f"expected {(T, 4)}")
    return tile_boxes


def source_map(counts, locs, fluxes, *, box, cells_per_pixel=4, weights=None, tile_boxes=None,
               with_flux=False):
    """Posterior source-density map of counts [T,N], locs [T,N,S,2], fluxes
    [T,N,S] on a grid of cells_per_pixel cells per pixel over `box` (lo_h,
    lo_w, hi_h, hi_w), ceil((hi - lo) * cells_per_pixel) cells per side (with
    tile_boxes [T,4]: each tile's own lower corner, the grid sized for the
    largest tile box).  weights [T,N]: one per catalog (None: 1).  Returns a
    SourceMap.  Unweighted counts are exact and the same on every run; weighted
    sums and the flux map may differ in their last bits between runs."""
    counts, locs, fluxes, weights = _catalogs(counts, locs, fluxes, weights, "source_map")
    T, N, S = locs.shape[:3]
    box = _box4(box)
    c = int(cells_per_pixel)
    _check_cells_per_pixel(c, "source_map")
    tile_boxes = _tile_boxes(tile_boxes, T, "source_map")
    if tile_boxes is None:
        ext_h, ext_w = box[2] - box[0], box[3] - box[1]
    else:
        ext = (tile_boxes[:, 2:] - tile_boxes[:, :2]).double().amax(0).tolist()
        ext_h, ext_w = ext
    Gh, Gw = math.ceil(ext_h * c), math.ceil(ext_w * c)
    if not (1 <= Gh <= _hip.MAP_MAX_GRID and 1 <= Gw <= _hip.MAP_MAX_GRID):
        raise ValueError(f"source_map: a {Gh}x{Gw} grid is outside 1..{_hip.MAP_MAX_GRID} cells "
                         "per side: use a smaller cells_per_pixel")
    dev = locs.device
    count = torch.empty(T, Gh, Gw, device=dev, dtype=torch.float32)
    flux = torch.empty(T, Gh, Gw, device=dev, dtype=torch.float32) if with_flux else None
    outside = torch.empty(T, device=dev, dtype=torch.float32)
    check(lib().smcdet_source_map(ptr(counts), ptr(locs), ptr(fluxes), ptr(weights), _cbox(box),
                                  ptr(tile_boxes), T, N, S, c, Gh, Gw, ptr(count), ptr(flux),
                                  ptr(outside), stream_of(locs)), "smcdet_source_map")
    total = (weights.double().sum(1) if weights is not None
             else torch.full((T,), float(N), device=dev, dtype=torch.float64))
    return SourceMap(count, flux, outside, box, c, tile_boxes, total, S)


def find_seeds(smap, *, smooth_radius=1, nms_radius=2, min_prob=0.05, max_seeds=None):
    """Seeds of a SourceMap: the peaks of its count map summed over
    (2*smooth_radius+1)^2 cells that hold at least min_prob x the tile's total
    weight and beat every cell within nms_radius (Chebyshev; ties: the lower
    flat index), by descending mass, at most max_seeds (default min(64, 2*S))
    per tile.  Returns Seeds; locs are the mass-weighted centroids of the raw
    map over each peak's smoothing window, in pixels."""
    count = dev_f32(smap.count, "smap.count")
    if count.dim() != 3:
        raise ValueError(f"find_seeds: the count map must be [T,Gh,Gw], got {tuple(count.shape)}")
    T, Gh, Gw = count.shape
    c = int(smap.cells_per_pixel)
    _check_cells_per_pixel(c, "find_seeds")
    if max_seeds is None:
        max_seeds = _hip.MATCH_MAX_SOURCES if smap.max_sources is None else \
            min(_hip.MATCH_MAX_SOURCES, 2 * int(smap.max_sources))
    K, q, p = int(max_seeds), int(smooth_radius), int(nms_radius)
    if not 1 <= K <= _hip.MATCH_MAX_SOURCES:
        raise ValueError(f"find_seeds: max_seeds = {K} outside 1..{_hip.MATCH_MAX_SOURCES} (the "
                         "association holds one seed per lane of a 64-wide wavefront)")
    if not 0 <= q <= _hip.PEAKS_MAX_SMOOTH:
        raise ValueError(f"find_seeds: smooth_radius = {q} outside 0..{_hip.PEAKS_MAX_SMOOTH}")
    if not 0 <= p <= _hip.PEAKS_MAX_NMS:
        raise ValueError(f"find_seeds: nms_radius = {p} outside 0..{_hip.PEAKS_MAX_NMS}")
    if T < 1 or Gh * Gw < 1 or Gh * Gw > _hip.PEAKS_MAX_CELLS:
        raise ValueError(f"find_seeds: a {Gh}x{Gw} grid has {Gh * Gw} cells, outside "
                         f"1..{_hip.PEAKS_MAX_CELLS} (the smoothed map of a tile lives in LDS): "
                         "use a smaller cells_per_pixel")
    if not (isinstance(min_prob, (int, float)) and 0 < min_prob <= 1):
        raise ValueError(f"find_seeds: min_prob = {min_prob} outside (0, 1]")
    dev = count.device
    if smap.total_weight is None:
        raise ValueError("find_seeds: the map carries no total_weight [T]")
    total = torch.as_tensor(smap.total_weight, dtype=torch.float64, device=dev).reshape(T)
    min_mass = (float(min_prob) * total).to(torch.float32).contiguous()
    tile_boxes = _tile_boxes(smap.tile_boxes, T, "find_seeds")
    box = _box4(smap.box)
    n_seeds = torch.empty(T, device=dev, dtype=torch.int32)
    cell = torch.empty(T, K, device=dev, dtype=torch.int32)
    mass = torch.empty(T, K, device=dev, dtype=torch.float32)
    slocs = torch.empty(T, K, 2, device=dev, dtype=torch.float32)
    check(lib().smcdet_map_peaks(ptr(count), _cbox(box), ptr(tile_boxes), T, Gh, Gw, c, q, p,
                                 ptr(min_mass), K, ptr(n_seeds), ptr(cell), ptr(mass), ptr(slocs),
                                 stream_of(count)), "smcdet_map_peaks")
    return Seeds(n_seeds, cell, mass, slocs)


def seed_moments(match_of_seed, locs, fluxes, seed_locs, *, weights=None,
                 with_matched_flux=True):
    """moments [T,K,10] float64 and matched_flux [T,N,K] (or None) of
    smcdet_seed_moments; match_of_seed [T,N,K] int32 is match_catalogs'
    match_of_true with the seeds as the true catalog."""
    locs = dev_f32(locs, "locs")
    fluxes = dev_f32(fluxes, "fluxes")
    seed_locs = dev_f32(seed_locs, "seed_locs")
    if locs.dim() != 4 or locs.shape[-1] != 2 or seed_locs.dim() != 3:
        raise ValueError("seed_moments: locs must be [T,N,S,2] and seed_locs [T,K,2]")
    T, N, S = locs.shape[:3]
    K = seed_locs.shape[1]
    if not isinstance(match_of_seed, torch.Tensor) or not match_of_seed.is_cuda:
        raise RuntimeError("match_of_seed must live on a HIP device; "
                           "smcdet_amd runs only on MI355X (gfx950)")
    if match_of_seed.dtype != torch.int32 or tuple(match_of_seed.shape) != (T, N, K) or \
            tuple(fluxes.shape) != (T, N, S) or tuple(seed_locs.shape) != (T, K, 2):
        raise ValueError("seed_moments: inconsistent shapes or match_of_seed is not int32")
    if not (1 <= K <= _hip.MATCH_MAX_SOURCES and 1 <= S <= _hip.MATCH_MAX_SOURCES):
        raise ValueError(f"seed_moments: K = {K} seeds, S = {S} slots outside "
                         f"1..{_hip.MATCH_MAX_SOURCES}")
    if weights is not None:
        weights = dev_f32(weights, "weights")
        if tuple(weights.shape) != (T, N):
            raise ValueError(f"seed_moments: weights must be {(T, N)}")
    match_of_seed = match_of_seed.contiguous()
    dev = locs.device
    moments = torch.empty(T, K, _hip.SEED_MOMENTS, device=dev, dtype=torch.float64)
    mflux = torch.empty(T, N, K, device=dev, dtype=torch.float32) if with_matched_flux else None
    check(lib().smcdet_seed_moments(ptr(match_of_seed), ptr(locs), ptr(fluxes), ptr(weights),
                                    ptr(seed_locs), T, N, S, K, ptr(moments), ptr(mflux),
                                    stream_of(locs)), "smcdet_seed_moments")
    return moments, mflux


def flux_quantiles(matched_flux, quantiles, weights=None):
    """[T,K,Q]: for each q the smallest matched flux whose cumulative weight
    among the seed's matched catalogs, sorted by flux, is >= q x the seed's
    total (no interpolation); NaN for a seed nothing matched.  matched_flux
    [T,N,K], NaN where unmatched."""
    T, N, K = matched_flux.shape
    sf, order = matched_flux.sort(dim=1)  # NaN sorts last
    ok = ~sf.isnan()
    if weights is None:
        w = ok.double()
    else:
        w = weights.double()[:, :, None].expand(T, N, K).gather(1, order) * ok
    cum = w.cumsum(1)
    total = cum[:, -1]  # [T,K]
    out = []
    for q in quantiles:
        first = (cum < float(q) * total[:, None, :]).sum(1).clamp_(max=N - 1)  # [T,K]
        v = sf.gather(1, first[:, None, :])[:, 0]
        out.append(torch.where(total > 0, v, torch.full_like(v, float("nan"))))
    return torch.stack(out, -1)


@dataclass
class CondensedCatalog:
    """One list of detections per tile, rows in seed order (descending seed
    mass); rows past n_seeds are NaN, with prob 0.  [T,K] unless stated."""
    n_seeds: torch.Tensor        # [T] int32
    seed_locs: torch.Tensor      # [T,K,2] where the seed was found
    seed_mass: torch.Tensor      # smoothed map mass at the seed
    prob: torch.Tensor           # weight of the catalogs with a source at the seed / all
    locs: torch.Tensor           # [T,K,2] posterior mean location
    locs_sd: torch.Tensor        # [T,K,2]
    locs_cov_hw: torch.Tensor    # h-w covariance
    fluxes: torch.Tensor
    fluxes_sd: torch.Tensor
    mags: torch.Tensor
    mags_sd: torch.Tensor
    flux_quantiles: torch.Tensor  # [T,K,Q]
    quantiles: Tuple[float, ...]
    expected_count: torch.Tensor  # [T] prob.sum(-1)
    unassociated: torch.Tensor    # [T] expected number of counted sources at no seed
    moments: torch.Tensor         # [T,K,10] float64 (smcdet_seed_moments)

    def _keep_first(self, min_prob):
        keep = self.prob >= min_prob
        order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
        return keep, order

    def as_catalog(self, min_prob=0.5):
        """(counts [T,1] int32, locs [T,1,K,2], fluxes [T,1,K]): the detections
        with prob >= min_prob, kept ones first (NaN after them), an N = 1
        population for `metrics.match_catalogs`."""
        keep, order = self._keep_first(min_prob)
        counts = keep.sum(1, dtype=torch.int32)
        kept = torch.arange(keep.shape[1], device=keep.device)[None, :] < counts[:, None]
        nan = torch.tensor(float("nan"), device=keep.device)
        locs = torch.where(kept[..., None], self.locs.gather(1, order[..., None].expand(-1, -1, 2)),
                           nan)
        fluxes = torch.where(kept, self.fluxes.gather(1, order), nan)
        return counts[:, None], locs[:, None].contiguous(), fluxes[:, None].contiguous()

    def to_image(self, num_tiles_per_side, tile_dim, min_prob=0.5):
        """Flat arrays over the detections with prob >= min_prob of all tiles
        (tile order, then seed order), locations in image coordinates: tile t
        (row-major, as SMCsampler) adds (t // numW, t % numW) * tile_dim.  A
        dict: tile [M] int64, locs [M,2], locs_sd [M,2], prob, fluxes,
        fluxes_sd, mags, mags_sd [M]."""
        nH, nW = (num_tiles_per_side if isinstance(num_tiles_per_side, (tuple, list))
                  else (num_tiles_per_side, num_tiles_per_side))
        T = self.prob.shape[0]
        if nH * nW != T:
            raise ValueError(f"to_image: {nH}x{nW} tiles, the catalog holds {T}")
        keep = self.prob >= min_prob
        t, k = keep.nonzero(as_tuple=True)
        off = torch.stack([torch.div(t, nW, rounding_mode="floor"), t % nW], -1) * float(tile_dim)
        return dict(tile=t, locs=self.locs[t, k] + off.to(self.locs.dtype),
                    locs_sd=self.locs_sd[t, k], prob=self.prob[t, k], fluxes=self.fluxes[t, k],
                    fluxes_sd=self.fluxes_sd[t, k], mags=self.mags[t, k],
                    mags_sd=self.mags_sd[t, k])


def derive(moments, total_weight):
    """The float64 derived fields of CondensedCatalog from moments [T,K,10] and
    total_weight [T]: a dict of float64 tensors (variances clamped at 0)."""
    m = moments.double()
    w = m[..., 0]
    mean = lambda i: m[..., i] / w  # noqa: E731 (0/0 = NaN for a seed nothing matched)
    dh, dw, f, mag = mean(1), mean(2), mean(6), mean(8)
    var = lambda i, mu: (mean(i) - mu * mu).clamp_min(0.0)  # noqa: E731 (NaN stays NaN)
    return dict(prob=w / total_weight[:, None], dh=dh, dw=dw,
                sd_h=var(3, dh).sqrt(), sd_w=var(4, dw).sqrt(), cov_hw=mean(5) - dh * dw,
                flux=f, flux_sd=var(7, f).sqrt(), mag=mag, mag_sd=var(9, mag).sqrt())


def condense(counts, locs, fluxes, *, box, weights=None, match_radius=0.75,
             quantiles=(0.05, 0.5, 0.95), cells_per_pixel=4, tile_boxes=None, smooth_radius=1,
             nms_radius=2, min_prob=0.05, max_seeds=None):
    """Condenses counts [T,N], locs [T,N,S,2], fluxes [T,N,S] (HIP tensors,
    kept sources first) into a CondensedCatalog: map, seeds, association of
    every catalog's sources with the seeds within match_radius pixels (the
    exact optimum of `metrics.match_catalogs`: the most seeds matched, then the
    least total distance), per-seed moments, derived fields."""
    counts, locs, fluxes, weights = _catalogs(counts, locs, fluxes, weights, "condense")
    T, N, S = locs.shape[:3]
    if S > _hip.MATCH_MAX_SOURCES:
        raise ValueError(f"condense: S = {S} source slots per catalog > "
                         f"{_hip.MATCH_MAX_SOURCES} (the association holds one source per lane "
                         "of a 64-wide wavefront): condense per tile, not an aggregated image")
    if max_seeds is not None and not 1 <= int(max_seeds) <= _hip.MATCH_MAX_SOURCES:
        raise ValueError(f"condense: max_seeds = {max_seeds} outside "
                         f"1..{_hip.MATCH_MAX_SOURCES}")
    if not float(match_radius) > 0:
        raise ValueError(f"condense: match_radius = {match_radius} must be positive")
    quantiles = tuple(float(q) for q in quantiles)
    if not all(0.0 <= q <= 1.0 for q in quantiles):
        raise ValueError(f"condense: quantiles {quantiles} outside [0, 1]")
    smap = source_map(counts, locs, fluxes, box=box, cells_per_pixel=cells_per_pixel,
                      weights=weights, tile_boxes=tile_boxes)
    seeds = find_seeds(smap, smooth_radius=smooth_radius, nms_radius=nms_radius,
                       min_prob=min_prob, max_seeds=max_seeds)
    K = seeds.locs.shape[1]
    # the seeds as the "true" catalog, flux 1, the magnitude test switched off
    out = metrics.match_catalogs(seeds.n_seeds, seeds.locs, torch.ones_like(seeds.mass), counts,
                                 locs, fluxes, None, float(match_radius), _F32_MAX,
                                 torch.zeros(1), return_matches=True)
    moments, mflux = seed_moments(out[4], locs, fluxes, seeds.locs, weights=weights)
    d = derive(moments, smap.total_weight)
    valid = torch.arange(K, device=locs.device)[None, :] < seeds.n_seeds[:, None]
    nan = torch.tensor(float("nan"), device=locs.device, dtype=torch.float64)

    def row(x):  # float32, NaN past n_seeds
        return torch.where(valid, x, nan).to(torch.float32)

    seed = seeds.locs.double()
    prob = torch.where(valid, d["prob"], torch.zeros_like(d["prob"])).nan_to_num(0.0)
    fq = flux_quantiles(mflux, quantiles, weights)
    counted = smap.count.double().sum((1, 2)) + smap.outside.double()
    return CondensedCatalog(
        n_seeds=seeds.n_seeds, seed_locs=seeds.locs, seed_mass=seeds.mass,
        prob=prob.to(torch.float32),
        locs=torch.stack([row(seed[..., 0] + d["dh"]), row(seed[..., 1] + d["dw"])], -1),
        locs_sd=torch.stack([row(d["sd_h"]), row(d["sd_w"])], -1),
        locs_cov_hw=row(d["cov_hw"]), fluxes=row(d["flux"]), fluxes_sd=row(d["flux_sd"]),
        mags=row(d["mag"]), mags_sd=row(d["mag_sd"]),
        flux_quantiles=torch.where(valid[..., None], fq, nan.to(torch.float32)),
        quantiles=quantiles, expected_count=prob.sum(-1).to(torch.float32),
        unassociated=((counted - moments[..., 0].sum(-1)) / smap.total_weight).to(torch.float32),
        moments=moments)


def condense_sampler(sampler, pruned=True, **kw):
    """`condense` on a run SMCsampler or MHsampler: its pruned catalogs with
    box (0, 0, tile_dim, tile_dim), or (pruned=False) the raw ones with the
    prior's padded box (the sampler's per-tile boxes where it has them);
    uniform weights, tiles flattened row-major to T."""
    if not getattr(sampler, "has_run", True) or not hasattr(sampler, "pruned_counts"):
        raise RuntimeError("condense_sampler: run the sampler first")
    if pruned:
        c, l, f = sampler.pruned_counts, sampler.pruned_locs, sampler.pruned_fluxes
        box = (0.0, 0.0, float(sampler.tile_dim), float(sampler.tile_dim))
    else:
        c, l, f = sampler.counts, sampler.locs, sampler.fluxes
        prior = sampler.Prior
        pad = float(prior.pad)
        box = (-pad, -pad, float(prior.image_height) + pad, float(prior.image_width) + pad)
        if getattr(sampler, "tile_boxes", None) is not None:
            kw.setdefault("tile_boxes", sampler.tile_boxes)
    N, S = l.shape[-3], l.shape[-2]
    return condense(c.reshape(-1, N), l.reshape(-1, N, S, 2).contiguous(),
                    f.reshape(-1, N, S).contiguous(), box=box, **kw)
