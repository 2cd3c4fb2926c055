"""Posterior calibration summaries (the reference computes them
by hand in its results notebooks): how many detectable sources every sampled
catalog holds and the count posterior of each tile, credible intervals of the
total flux with their empirical coverage and the rank of the truth, the
luminosity function's quantile bands, and bootstrap bands of the per-catalog
precision / recall / F1 rows.

All of it rests on three kernels of include/smcdet_hip.h:

  `catalog_totals`   smcdet_catalog_totals: per catalog, the number and the
                     summed flux of the counted sources above each flux cut;
  `row_summary`      smcdet_row_summary: order statistics along the catalog
                     axis (quantiles, masses below thresholds, moments), NaN
                     meaning "missing", optionally weighted;
  `bootstrap_means`  smcdet_bootstrap_means: means of resampled rows.

The rest is plain torch on the small arrays those return.  Inputs are HIP
tensors; nothing falls back to the host.

Two quantile definitions (`interpolation`):
  "linear"  `torch.quantile` / `numpy.quantile(method="linear")` over the
            entries that are not NaN; unweighted only;
  "lower"   `condense.flux_quantiles`' definition: the smallest value whose
            cumulative weight, in ascending order, reaches q x the row's total
            weight (no interpolation; q = 0 gives the minimum).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _hip
from ._hip import check, dev_f32, lib, ptr, stream_of
from ._rng import torch_seed
from .metrics import _counts_i32

_U64 = (1 << 64) - 1
_INTERPOLATION = {"linear": _hip.SUMMARY_LINEAR, "lower": _hip.SUMMARY_LOWER}
DEFAULT_LEVELS = tuple(round(0.05 * c, 2) for c in range(1, 20))  # the notebook's 0.05 .. 0.95


@dataclass
class CatalogTotals:
    """n_above [C,T,N] int32: counted sources with flux >= flux_cuts[c];
    flux_above [C,T,N] float32: their summed flux (float64 sum, rounded once)."""
    n_above: torch.Tensor
    flux_above: torch.Tensor
    flux_cuts: Tuple[float, ...]


@dataclass
class RowSummary:
    """Per row ([R] for values [R,N], [A,B] for values [A,N,B]): n_valid int32;
    weight, mean, var float64; vmin, vmax float32; quantiles [...,Q] float32;
    below / at_or_below [...,E] float64 (None without thresholds)."""
    n_valid: torch.Tensor
    weight: torch.Tensor
    mean: torch.Tensor
    var: torch.Tensor
    vmin: torch.Tensor
    vmax: torch.Tensor
    quantiles: torch.Tensor
    below: Optional[torch.Tensor]
    at_or_below: Optional[torch.Tensor]
    levels: Tuple[float, ...]


@dataclass
class Coverage:
    """levels [L]; lo, hi, covered [R,L]; rate [L] float64: the share of the
    rows kept by the mask whose interval holds the truth; pit [R] float64:
    the share of the posterior weight at or above the truth; sbc_rank [R]
    int64: the number of samples below the truth."""
    levels: Tuple[float, ...]
    lo: torch.Tensor
    hi: torch.Tensor
    covered: torch.Tensor
    rate: torch.Tensor
    pit: torch.Tensor
    sbc_rank: torch.Tensor


@dataclass
class CountPosterior:
    """mass [T,K+1] float64: weight of the catalogs with exactly k sources, k =
    0..max_count (unweighted: the number of catalogs); pmf = mass / weight;
    mode [T] int64 (ties: the lower count); weight [T] float64."""
    pmf: torch.Tensor
    mode: torch.Tensor
    mass: torch.Tensor
    weight: torch.Tensor


@dataclass
class Calibration:
    totals: CatalogTotals          # of the sampled catalogs
    true_n_above: torch.Tensor     # [T] int32
    true_flux_above: torch.Tensor  # [T] float32
    coverage: Coverage             # of the total flux above the cut, tiles with a true source
    count_posterior: CountPosterior
    confusion_samples: torch.Tensor  # [max_count+1, max_true+1] float64: catalogs (or weight)
    confusion_mode: torch.Tensor     # [max_count+1, max_true+1] int64: tiles


def catalog_totals(counts, fluxes, flux_cuts=(0.0,)):
    """Per catalog of counts [T,N] / fluxes [T,N,S] (kept sources first): the
    number of counted sources with flux >= each cut and their summed flux.
    Slots at or past the count are ignored, whatever they hold."""
    fluxes = dev_f32(fluxes, "fluxes")
    if fluxes.dim() != 3:
        raise ValueError(f"catalog_totals: fluxes must be [T,N,S], got {tuple(fluxes.shape)}")
    T, N, S = fluxes.shape
    if T < 1 or N < 1 or not 1 <= S <= _hip.MATCH_MAX_SOURCES:
        raise ValueError(f"catalog_totals: T = {T}, N = {N} must be >= 1 and S = {S} in "
                         f"1..{_hip.MATCH_MAX_SOURCES}")
    counts = _counts_i32(counts, "counts", (T, N), fluxes.device)
    cuts = tuple(float(c) for c in (flux_cuts.tolist() if isinstance(flux_cuts, torch.Tensor)
                                    else flux_cuts))
    if not 1 <= len(cuts) <= _hip.TOTALS_MAX_CUTS or any(c != c for c in cuts):
        raise ValueError(f"catalog_totals: flux_cuts must hold 1..{_hip.TOTALS_MAX_CUTS} numbers, "
                         f"got {cuts}")
    C = len(cuts)
    n_above = torch.empty(C, T, N, device=fluxes.device, dtype=torch.int32)
    flux_above = torch.empty(C, T, N, device=fluxes.device, dtype=torch.float32)
    check(lib().smcdet_catalog_totals(ptr(counts), ptr(fluxes), (ctypes.c_float * C)(*cuts), T, N,
                                      S, C, ptr(n_above), ptr(flux_above), stream_of(fluxes)),
          "smcdet_catalog_totals")
    return CatalogTotals(n_above, flux_above, cuts)


def row_summary(values, *, dim=-1, weights=None, quantiles=(), interpolation="linear",
                thresholds=None):
    """Order statistics of values along one axis: values [R,N] with dim=-1, or
    [A,N,B] with dim=1 (read in place, no transposed copy).  NaN entries are
    missing.  weights [R,N] / [A,N] >= 0 (interpolation="lower" only);
    quantiles: up to 64 levels in [0,1]; thresholds [R,E] / [A,B,E], E <= 65:
    the weight strictly below and at or below each.  Returns a RowSummary."""
    values = dev_f32(values, "values")
    if values.dim() == 2 and dim in (-1, 1):
        A, N, B = values.shape[0], values.shape[1], 1
        lead = (A,)
    elif values.dim() == 3 and dim in (1, -2):
        A, N, B = values.shape
        lead = (A, B)
    else:
        raise ValueError("row_summary: values must be [R,N] with dim=-1 or [A,N,B] with dim=1, got "
                         f"{tuple(values.shape)} with dim={dim}")
    if A < 1 or B < 1 or not 1 <= N <= _hip.SUMMARY_MAX_N:
        raise ValueError(f"row_summary: {N} entries per row outside 1..{_hip.SUMMARY_MAX_N} (a row "
                         f"is sorted in LDS), or no rows ({A} x {B})")
    if interpolation not in _INTERPOLATION:
        raise ValueError(f"row_summary: interpolation must be one of {tuple(_INTERPOLATION)}, got "
                         f"{interpolation!r}")
    if weights is not None:
        if interpolation == "linear":
            raise ValueError("row_summary: weighted quantiles are interpolation=\"lower\" "
                             "(linear interpolation is defined for unweighted rows only)")
        weights = dev_f32(weights, "weights")
        if tuple(weights.shape) != (A, N):
            raise ValueError(f"row_summary: weights has shape {tuple(weights.shape)}, expected "
                             f"{(A, N)}")
    levels = tuple(float(q) for q in (quantiles.tolist() if isinstance(quantiles, torch.Tensor)
                                      else quantiles))
    Q = len(levels)
    if Q > _hip.SUMMARY_MAX_Q or not all(0.0 <= q <= 1.0 for q in levels):
        raise ValueError(f"row_summary: at most {_hip.SUMMARY_MAX_Q} quantile levels in [0, 1], "
                         f"got {Q}: {levels}")
    E = 0
    if thresholds is not None:
        thresholds = dev_f32(thresholds, "thresholds")
        if thresholds.dim() != len(lead) + 1 or tuple(thresholds.shape[:-1]) != lead or \
                not 1 <= thresholds.shape[-1] <= _hip.SUMMARY_MAX_E:
            raise ValueError(f"row_summary: thresholds has shape {tuple(thresholds.shape)}, "
                             f"expected {lead} + (E,), E in 1..{_hip.SUMMARY_MAX_E}")
        E = thresholds.shape[-1]
    dev = values.device
    f64 = dict(device=dev, dtype=torch.float64)
    n_valid = torch.empty(lead, device=dev, dtype=torch.int32)
    weight, mean, var = (torch.empty(lead, **f64) for _ in range(3))
    vmin, vmax = (torch.empty(lead, device=dev, dtype=torch.float32) for _ in range(2))
    quant = torch.empty(lead + (Q,), device=dev, dtype=torch.float32)
    below = torch.empty(lead + (E,), **f64) if E else None
    at_or_below = torch.empty(lead + (E,), **f64) if E else None
    check(lib().smcdet_row_summary(
        ptr(values), ptr(weights), A, N, B, (ctypes.c_double * max(Q, 1))(*levels), Q,
        _INTERPOLATION[interpolation], ptr(thresholds), E, ptr(n_valid), ptr(weight), ptr(mean),
        ptr(var), ptr(vmin), ptr(vmax), ptr(quant) if Q else None, ptr(below), ptr(at_or_below),
        stream_of(values)), "smcdet_row_summary")
    return RowSummary(n_valid, weight, mean, var, vmin, vmax, quant, below, at_or_below, levels)


def _levels(levels):
    levels = DEFAULT_LEVELS if levels is None else tuple(
        float(x) for x in (levels.tolist() if isinstance(levels, torch.Tensor) else levels))
    if not levels or 2 * len(levels) > _hip.SUMMARY_MAX_Q or \
            not all(0.0 <= x <= 1.0 for x in levels):
        raise ValueError(f"1..{_hip.SUMMARY_MAX_Q // 2} credible levels in [0, 1] are needed, got "
                         f"{levels}")
    return levels


def _interval_q(levels):
    """The 2L quantile levels 0.5 -+ level / 2 (clamped to [0, 1])."""
    return tuple(max(0.5 - x / 2, 0.0) for x in levels) + tuple(min(0.5 + x / 2, 1.0)
                                                                 for x in levels)


def credible_intervals(values, levels, *, dim=-1, weights=None, interpolation=None):
    """Central credible intervals: (lo, hi), each [...,L], the quantiles at
    0.5 -+ level / 2 of `row_summary` (interpolation: "linear", or "lower" when
    weights are given)."""
    levels = _levels(levels)
    if interpolation is None:
        interpolation = "linear" if weights is None else "lower"
    L = len(levels)
    s = row_summary(values, dim=dim, weights=weights, quantiles=_interval_q(levels),
                    interpolation=interpolation)
    return s.quantiles[..., :L], s.quantiles[..., L:]


def coverage(values, truth, levels=None, mask=None, weights=None):
    """Calibration of the posterior samples values [R,N] against truth [R]:
    central intervals at `levels` (default 0.05 .. 0.95), whether each holds the
    truth (lo <= truth <= hi), the share of the rows kept by mask [R] (bool)
    where it does, the PIT value 1 - below / weight (the share of the weight at
    or above the truth) and the SBC rank (the number of samples below the
    truth, unweighted).  Returns a Coverage."""
    levels = _levels(levels)
    values = dev_f32(values, "values")
    truth = dev_f32(truth, "truth")
    if values.dim() != 2 or tuple(truth.shape) != (values.shape[0],):
        raise ValueError(f"coverage: values must be [R,N] and truth [R], got {tuple(values.shape)} "
                         f"and {tuple(truth.shape)}")
    L = len(levels)
    s = row_summary(values, weights=weights, quantiles=_interval_q(levels),
                    interpolation="linear" if weights is None else "lower",
                    thresholds=truth[:, None])
    lo, hi = s.quantiles[:, :L], s.quantiles[:, L:]
    covered = (lo <= truth[:, None]) & (truth[:, None] <= hi)
    kept = covered if mask is None else covered[mask.to(covered.device, torch.bool)]
    rank = s.below if weights is None else row_summary(values, thresholds=truth[:, None]).below
    # (a tensor divisor: the correctly rounded quotient, not a product with 1 / n)
    rate = kept.sum(0).double() / torch.full((), float(kept.shape[0]), dtype=torch.float64,
                                             device=kept.device)
    return Coverage(levels, lo, hi, covered, rate,
                    1.0 - s.below[:, 0] / s.weight, rank[:, 0].round().to(torch.int64))


def count_posterior(n_above, max_count, weights=None):
    """The posterior of the per-catalog count n_above [T,N] (integers below
    2^24) on 0..max_count (<= 64): the mass at or below each count from
    `row_summary`, differenced; catalogs with more than max_count sources are in
    no bin.  Returns a CountPosterior."""
    if not isinstance(n_above, torch.Tensor) or not n_above.is_cuda:
        raise RuntimeError("n_above must live on a HIP device; smcdet_amd runs only on MI355X "
                           "(gfx950)")
    K = int(max_count)
    if n_above.dim() != 2 or not 0 <= K < _hip.SUMMARY_MAX_E:
        raise ValueError(f"count_posterior: n_above must be [T,N] and max_count = {K} in "
                         f"0..{_hip.SUMMARY_MAX_E - 1}")
    T = n_above.shape[0]
    x = n_above.to(torch.float32)
    thr = torch.arange(K + 1, device=x.device, dtype=torch.float32).expand(T, K + 1).contiguous()
    s = row_summary(x, weights=weights, interpolation="lower", thresholds=thr)
    mass = torch.diff(s.at_or_below, dim=-1, prepend=torch.zeros_like(s.at_or_below[:, :1]))
    pmf = mass / s.weight[:, None]
    ks = torch.arange(K + 1, device=x.device)
    mode = torch.where(mass == mass.amax(-1, keepdim=True), ks, K + 1).amin(-1)
    return CountPosterior(pmf, mode, mass, s.weight)


def count_confusion(pmf_or_mode, true_counts, max_true, max_count=None):
    """Estimated count (rows) against true count (columns 0..max_true; tiles
    with more are in no column).  A floating [T,K+1] argument (a pmf or a
    CountPosterior's mass) gives the float64 sum over tiles of its rows: with
    `mass` of an unweighted posterior, the number of (tile, catalog) pairs per
    cell.  An integer [T] argument (the mode) gives the int64 number of tiles
    per cell, rows 0..max_count (default: the largest mode)."""
    x = pmf_or_mode
    tc = true_counts.to(x.device, torch.int64).reshape(-1)
    C = int(max_true) + 1
    if tc.shape[0] != x.shape[0]:
        raise ValueError(f"count_confusion: {x.shape[0]} tiles, {tc.shape[0]} true counts")
    onehot = tc[:, None] == torch.arange(C, device=x.device)[None, :]  # [T,C]
    if x.is_floating_point():
        if x.dim() != 2:
            raise ValueError("count_confusion: a floating argument must be [T, max_count+1]")
        return x.double().t() @ onehot.double()
    if x.dim() != 1:
        raise ValueError("count_confusion: an integer argument must be the modes [T]")
    K = int(x.max()) if max_count is None else int(max_count)
    rows = x.to(torch.int64)[:, None] == torch.arange(K + 1, device=x.device)[None, :]
    return (rows[:, :, None] & onehot[:, None, :]).sum(0)  # (bool -> int64)


def luminosity_function(est_total, quantiles=(0.05, 0.5, 0.95)):
    """Quantiles over catalogs of the number of sources per bin summed over
    tiles: est_total [T,N,Bins] (match_catalogs' third output with every
    catalog matched) -> [Bins,Q] ("linear" interpolation)."""
    est_total = dev_f32(est_total, "est_total")
    if est_total.dim() != 3:
        raise ValueError(f"luminosity_function: est_total must be [T,N,Bins], got "
                         f"{tuple(est_total.shape)}")
    tot = est_total.double().sum(0)
    if not bool((tot.abs() < 2.0 ** 24).all()) or not bool((tot == tot.round()).all()):
        raise ValueError("luminosity_function: the per-bin totals must be integers below 2^24 "
                         "(exact in float32)")
    return row_summary(tot.to(torch.float32)[None], dim=1, quantiles=quantiles).quantiles[0]


def bootstrap_means(values, num_samples, seed=None, indices=None):
    """[num_samples,D]: means of M rows of values [M,D] drawn with replacement.
    indices [num_samples,M] (integers in [0,M)) replays given draws; otherwise
    row j of replicate r is mulhi32(Philox(seed; r, j / 4)[j % 4], M), which
    favours no row by more than M / 2^32 (seed None: from torch's generator)."""
    values = dev_f32(values, "values")
    if values.dim() != 2 or values.shape[0] < 1 or \
            not 1 <= values.shape[1] <= _hip.BOOT_MAX_COLUMNS:
        raise ValueError(f"bootstrap_means: values must be [M,D] with M >= 1 and D in "
                         f"1..{_hip.BOOT_MAX_COLUMNS}, got {tuple(values.shape)}")
    M, D = values.shape
    Bn = int(num_samples)
    if Bn < 1:
        raise ValueError(f"bootstrap_means: num_samples = {Bn} < 1")
    if indices is not None:
        if not isinstance(indices, torch.Tensor) or not indices.is_cuda:
            raise RuntimeError("indices must live on a HIP device; smcdet_amd runs only on MI355X "
                               "(gfx950)")
        if tuple(indices.shape) != (Bn, M) or indices.is_floating_point():
            raise ValueError(f"bootstrap_means: indices must be a [{Bn},{M}] integer tensor, got "
                             f"{tuple(indices.shape)} {indices.dtype}")
        if int(indices.min()) < 0 or int(indices.max()) >= M:
            raise ValueError(f"bootstrap_means: indices must lie in [0, {M})")
        indices = indices.to(torch.int32).contiguous()
        seed = 0
    else:
        seed = torch_seed() if seed is None else int(seed) & _U64
    out = torch.empty(Bn, D, device=values.device, dtype=torch.float32)
    check(lib().smcdet_bootstrap_means(ptr(values), M, D, ptr(indices), seed, Bn, ptr(out),
                                       stream_of(values)), "smcdet_bootstrap_means")
    return out


def bootstrap_ci(values, num_samples=10000, alpha=0.1, num_comparisons=1, seed=None,
                 indices=None):
    """(lower, mean, upper), each [D]: the alpha / num_comparisons and
    1 - alpha / num_comparisons quantiles ("linear") and the mean of
    num_samples bootstrap means of the rows of values [M,D] (the reference's
    Bonferroni-corrected bands of precision / recall / F1)."""
    a = float(alpha) / float(num_comparisons)
    if not 0.0 < a <= 0.5:
        raise ValueError(f"bootstrap_ci: alpha / num_comparisons = {a} outside (0, 0.5]")
    boot = bootstrap_means(values, num_samples, seed=seed, indices=indices)
    s = row_summary(boot[None], dim=1, quantiles=(a, 1.0 - a))
    return s.quantiles[0, :, 0], s.mean[0].to(torch.float32), s.quantiles[0, :, 1]


def calibrate(true_counts, true_fluxes, est_counts, est_fluxes, *, flux_cut=0.0, levels=None,
              weights=None):
    """The calibration of a posterior against the truth: true_counts [T],
    true_fluxes [T,St], est_counts [T,N], est_fluxes [T,N,S] (kept sources
    first), weights [T,N] or None.  Counts and total fluxes are those of the
    sources with flux >= flux_cut, formed by `catalog_totals` for the samples
    and (as an N = 1 population) for the truth; the coverage rate is over the
    tiles with at least one true source.  Returns a Calibration."""
    est_fluxes = dev_f32(est_fluxes, "est_fluxes")
    true_fluxes = dev_f32(true_fluxes, "true_fluxes")
    if est_fluxes.dim() != 3 or true_fluxes.dim() != 2 or \
            true_fluxes.shape[0] != est_fluxes.shape[0]:
        raise ValueError("calibrate: true_fluxes must be [T,St] and est_fluxes [T,N,S], got "
                         f"{tuple(true_fluxes.shape)} and {tuple(est_fluxes.shape)}")
    T = est_fluxes.shape[0]
    if not isinstance(true_counts, torch.Tensor):
        raise TypeError("true_counts must be a torch.Tensor")
    tot = catalog_totals(est_counts, est_fluxes, (flux_cut,))
    true = catalog_totals(true_counts.reshape(T, 1), true_fluxes[:, None], (flux_cut,))
    tn, tf = true.n_above[0, :, 0], true.flux_above[0, :, 0]
    max_true = int(tn.max())
    max_count = min(int(tot.n_above.max()), _hip.SUMMARY_MAX_E - 1)
    cov = coverage(tot.flux_above[0], tf, levels=levels, mask=true_counts.reshape(T) > 0,
                   weights=weights)
    post = count_posterior(tot.n_above[0], max_count, weights=weights)
    return Calibration(tot, tn, tf, cov, post, count_confusion(post.mass, tn, max_true),
                       count_confusion(post.mode, tn, max_true, max_count))


def calibrate_sampler(sampler, true_counts, true_fluxes, **kw):
    """`calibrate` on a finished SMCsampler's or MHsampler's pruned catalogs,
    tiles flattened row-major to T (true_counts [T] or [numH,numW], true_fluxes
    [T,St] or [numH,numW,St] likewise); uniform weights unless given."""
    if not getattr(sampler, "has_run", True) or not hasattr(sampler, "pruned_counts"):
        raise RuntimeError("calibrate_sampler: run the sampler first")
    c, f = sampler.pruned_counts, sampler.pruned_fluxes
    N, S = f.shape[-2], f.shape[-1]
    return calibrate(true_counts.reshape(-1), true_fluxes.reshape(-1, true_fluxes.shape[-1]),
                     c.reshape(-1, N), f.reshape(-1, N, S).contiguous(), **kw)
