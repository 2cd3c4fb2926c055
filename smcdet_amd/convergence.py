"""MCMC convergence diagnostics (not in the reference): did the
chains of an `MHsampler` mix, and how much are its kept draws worth?

  `chain_stats`      smcdet_chain_stats: per row of chains [C,M], split-R-hat,
                     Geyer's initial-monotone-sequence autocorrelation time
                     tau, the effective sample size, the Monte Carlo standard
                     error of the mean and the first autocorrelations, one
                     workgroup per row, only as many lags as the rule needs;
  `rank_normalize`   average ranks over a row's pooled draws mapped to normal
                     scores (torch: one sort, two searches);
  `diagnose`         the rank-normalized and folded R-hat, bulk and tail ESS of
                     Vehtari, Gelman, Simpson, Carpenter & Buerkner (2021), all
                     quantities stacked into one launch of the kernel;
  `diagnose_sampler` the same for the traces of a finished MHsampler.

The tail term Stan adds to tau is left out.  Inputs are HIP
tensors; nothing falls back to the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import _hip
from ._hip import check, lib, ptr, stream_of


@dataclass
class ChainStats:
    """Per row (the leading dimensions of x): mean, W, var_plus, rhat, tau,
    ess, mcse float64; n_pairs, stopped int32; chain_mean, chain_var [...,m]
    float64 and rho [...,num_rho] float32 (None unless asked for); m chains of n
    draws each went into every row."""
    mean: torch.Tensor
    W: torch.Tensor
    var_plus: torch.Tensor
    rhat: torch.Tensor
    tau: torch.Tensor
    ess: torch.Tensor
    mcse: torch.Tensor
    n_pairs: torch.Tensor
    stopped: torch.Tensor
    chain_mean: Optional[torch.Tensor]
    chain_var: Optional[torch.Tensor]
    rho: Optional[torch.Tensor]
    m: int
    n: int

    @property
    def lag_blocks(self):
        """The blocks of SMCDET_CHAINS_BLOCK_PAIRS lag pairs the stopping rule
        took per row (without a rho output), int32."""
        b = _hip.CHAINS_BLOCK_PAIRS
        return torch.clamp((self.n_pairs + self.stopped + b - 1) // b, min=1)


@dataclass
class Convergence:
    """Per row: rhat (the larger of the rank-normalized and the folded
    split-R-hat), ess_bulk, ess_tail, and from the raw draws ess_mean,
    mcse_mean, tau, mean float64, stopped int32, rho [...,num_rho] float32 or
    None.  `diagnose_sampler` adds names (of the last leading dimension),
    accept_rate (post-burn-in, per chain) and frozen."""
    rhat: torch.Tensor
    ess_bulk: torch.Tensor
    ess_tail: torch.Tensor
    ess_mean: torch.Tensor
    mcse_mean: torch.Tensor
    tau: torch.Tensor
    mean: torch.Tensor
    stopped: torch.Tensor
    rho: Optional[torch.Tensor]
    names: Optional[Tuple[str, ...]] = None
    accept_rate: Optional[torch.Tensor] = None
    frozen: Optional[torch.Tensor] = None

    def warnings(self, rhat_max=1.01, ess_min=400) -> List[tuple]:
        """The rows that fail the usual thresholds (Vehtari et al. 2021):
        (index, name, rhat, ess_bulk, ess_tail) for every row with rhat >
        rhat_max, ess_bulk < ess_min or ess_tail < ess_min, or with a NaN in
        one of them; index is the row's index tuple (for a sampler: tile row,
        tile column, quantity), name that quantity's name or None."""
        ok = (self.rhat <= rhat_max) & (self.ess_bulk >= ess_min) & (self.ess_tail >= ess_min)
        out = []
        for idx in (~ok).nonzero().tolist():
            idx = tuple(idx)
            name = self.names[idx[-1]] if self.names is not None and idx else None
            out.append((idx, name, float(self.rhat[idx]), float(self.ess_bulk[idx]),
                        float(self.ess_tail[idx])))
        return out


def _shape(x, split, where):
    """(lead, C, M, m, n) of x [...,C,M] after the checks of the C ABI."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{where}: x must be a torch.Tensor")
    if x.dim() < 2:
        raise ValueError(f"{where}: x must be [...,C,M] (chains, draws), got {tuple(x.shape)}")
    lead, (C, M) = tuple(x.shape[:-2]), x.shape[-2:]
    if not 1 <= C <= _hip.CHAINS_MAX_CHAINS:
        raise ValueError(f"{where}: C = {C} chains outside 1..{_hip.CHAINS_MAX_CHAINS}")
    m, n = (2 * C, M // 2) if split else (C, M)
    if n < 4:
        raise ValueError(f"{where}: {M} draws per chain give n = {n} per "
                         f"{'split ' if split else ''}chain; at least 4 are needed")
    if m * n > _hip.CHAINS_MAX_DRAWS:
        raise ValueError(f"{where}: m*n = {m * n} draws per row above {_hip.CHAINS_MAX_DRAWS}")
    R = 1
    for d in lead:
        R *= d
    if R < 1 or R * m > 2 ** 31 - 1:
        raise ValueError(f"{where}: {R} rows of {m} chains outside 1..2^31-1 chains")
    return lead, C, M, m, n


def _dev(x, where):
    if not x.is_cuda:
        raise RuntimeError(f"{where}: x must live on a HIP device (got {x.device}); smcdet_amd "
                           "runs only on MI355X (gfx950)")


def chain_stats(x, *, split=True, max_lag=None, num_rho=0, chain_moments=False):
    """Convergence statistics of x [...,C,M]: C chains of M kept draws per row;
    the leading dimensions are kept on the outputs.  A float64 or integer x is
    converted to float32 first (as `calibration` converts counts): the
    statistics are those of the rounded draws.  split: every chain becomes its
    first and last M // 2 draws (an odd M drops the middle draw).  max_lag
    (default n - 1) bounds the lags of Geyer's sum; num_rho autocorrelations
    (<= 1024) and, with chain_moments, the per-chain means and variances are
    returned too.  Returns a ChainStats (smcdet_hip.h has the definitions)."""
    lead, C, M, m, n = _shape(x, split, "chain_stats")
    num_rho = int(num_rho)
    if not 0 <= num_rho <= _hip.CHAINS_MAX_RHO:
        raise ValueError(f"chain_stats: num_rho = {num_rho} outside 0..{_hip.CHAINS_MAX_RHO}")
    max_lag = n - 1 if max_lag is None else int(max_lag)
    if max_lag < 1:
        raise ValueError(f"chain_stats: max_lag = {max_lag} < 1")
    max_lag = min(max_lag, n - 1)
    _dev(x, "chain_stats")
    x = x.to(torch.float32).contiguous()
    dev = x.device
    R = x.numel() // (C * M)
    f64 = dict(device=dev, dtype=torch.float64)
    mean, W, vp, rhat, tau, ess, mcse = (torch.empty(lead, **f64) for _ in range(7))
    n_pairs, stopped = (torch.empty(lead, device=dev, dtype=torch.int32) for _ in range(2))
    cmean = torch.empty(lead + (m,), **f64) if chain_moments else None
    cvar = torch.empty(lead + (m,), **f64) if chain_moments else None
    rho = torch.empty(lead + (num_rho,), device=dev, dtype=torch.float32) if num_rho else None
    need = lib().smcdet_chain_stats_workspace(R, C, M, int(bool(split)))
    if need < 0:
        check(int(need), "smcdet_chain_stats_workspace")
    ws = torch.empty(need, device=dev, dtype=torch.float32) if need else None
    check(lib().smcdet_chain_stats(
        ptr(x), R, C, M, int(bool(split)), max_lag, num_rho, ptr(mean), ptr(W), ptr(vp), ptr(rhat),
        ptr(tau), ptr(ess), ptr(mcse), ptr(n_pairs), ptr(stopped), ptr(cmean), ptr(cvar), ptr(rho),
        ptr(ws), need, stream_of(x)), "smcdet_chain_stats")
    return ChainStats(mean, W, vp, rhat, tau, ess, mcse, n_pairs, stopped, cmean, cvar, rho, m, n)


def average_ranks(x):
    """[...,C,M] float64: the 1-based rank of every draw among its row's pooled
    C*M draws, ties sharing the mean of their ranks (counts, hence exact)."""
    C, M = x.shape[-2:]
    flat = x.reshape(x.shape[:-2] + (C * M,)).contiguous()
    srt = torch.sort(flat, dim=-1).values
    lo = torch.searchsorted(srt, flat, right=False)
    hi = torch.searchsorted(srt, flat, right=True)
    return ((lo + hi + 1).double() * 0.5).reshape(x.shape)


def rank_normalize(x):
    """Normal scores of x [...,C,M]: z = ndtri((r - 3/8) / (S + 1/4)) with r the
    average rank among the row's S = C*M pooled draws, formed in float64 and
    returned as float32 (Vehtari et al. 2021, eq. 14)."""
    if x.dim() < 2:
        raise ValueError(f"rank_normalize: x must be [...,C,M], got {tuple(x.shape)}")
    S = x.shape[-1] * x.shape[-2]
    r = average_ranks(x)
    return torch.special.ndtri((r - 0.375) / (S + 0.25)).to(torch.float32)


def _pooled_quantiles(flat, qs):
    """[R,len(qs)] float32 linear-interpolation quantiles of the rows of flat
    [R,S]: `calibration.row_summary` where a row fits its LDS sort, else
    `torch.quantile` (in float64, rounded once)."""
    if flat.shape[-1] <= _hip.SUMMARY_MAX_N:
        from .calibration import row_summary
        return row_summary(flat, quantiles=qs).quantiles
    q = torch.tensor(qs, device=flat.device, dtype=torch.float64)
    return torch.stack([torch.quantile(row.double(), q) for row in flat]).to(torch.float32)


def diagnose_inputs(x, tail_prob=0.05):
    """The five quantities `diagnose` passes to the kernel, [5,R,C,M] float32
    for x [R,C,M] float32: the raw draws, their normal scores, the normal
    scores of the folded draws |x - median|, and the indicators x <= q_lo and
    x >= q_hi (the pooled tail_prob and 1 - tail_prob quantiles)."""
    R, C, M = x.shape
    qs = _pooled_quantiles(x.reshape(R, C * M), (tail_prob, 0.5, 1.0 - tail_prob))
    q_lo, med, q_hi = (qs[:, i, None, None] for i in range(3))
    return torch.stack([x, rank_normalize(x), rank_normalize((x - med).abs()),
                        (x <= q_lo).to(torch.float32), (x >= q_hi).to(torch.float32)])


def diagnose(x, *, tail_prob=0.05, num_rho=0):
    """The diagnostics of Vehtari et al. (2021) for x [...,C,M] (float64 or
    integer draws are converted to float32 first), every one from split chains:
    rhat = max(split-R-hat of the normal scores, split-R-hat of the normal
    scores of |x - median|), ess_bulk = the ESS of the normal scores, ess_tail
    = the smaller ESS of the indicators x <= q_lo and x >= q_hi at the pooled
    tail_prob and 1 - tail_prob quantiles, and ess_mean, mcse_mean, tau, mean,
    stopped and rho of the raw draws.  An indicator that never changes gives a
    NaN ess_tail.  One launch of `chain_stats`.  Returns a Convergence."""
    lead, C, M, m, n = _shape(x, True, "diagnose")
    if not 0.0 < float(tail_prob) < 0.5:
        raise ValueError(f"diagnose: tail_prob = {tail_prob} outside (0, 0.5)")
    _dev(x, "diagnose")
    x = x.to(torch.float32).reshape(-1, C, M).contiguous()
    s = chain_stats(diagnose_inputs(x, float(tail_prob)), split=True, num_rho=num_rho)
    shp = lambda t: t.reshape(lead)
    ess_tail = torch.minimum(s.ess[3], s.ess[4])
    ess_tail = torch.where(torch.isnan(s.ess[3]) | torch.isnan(s.ess[4]),
                           torch.full_like(ess_tail, float("nan")), ess_tail)
    rhat = torch.maximum(s.rhat[1], s.rhat[2])
    rhat = torch.where(torch.isnan(s.rhat[1]) | torch.isnan(s.rhat[2]),
                       torch.full_like(rhat, float("nan")), rhat)
    return Convergence(shp(rhat), shp(s.ess[1]), shp(ess_tail), shp(s.ess[0]), shp(s.mcse[0]),
                       shp(s.tau[0]), shp(s.mean[0]), shp(s.stopped[0]),
                       s.rho[0].reshape(lead + (num_rho,)) if num_rho else None)


def sampler_traces(mh, flux_cuts=(0.0,), log_target=False):
    """(x [nH,nW,Q,C,M] float32, names) of a finished MHsampler: per flux cut
    the number of detectable sources and their total flux
    (`calibration.catalog_totals` on the pruned catalogs), the total intrinsic
    flux of all sources (float64 sum, rounded once) and, with log_target, the
    log target density of every kept draw."""
    from .calibration import catalog_totals
    if not getattr(mh, "has_run", False):
        raise RuntimeError("diagnose_sampler: run the sampler first")
    nH, nW = mh.tiles_shape
    C = mh.num_chains
    N, S = mh.pruned_fluxes.shape[-2:]
    M = N // C
    tot = catalog_totals(mh.pruned_counts.reshape(nH * nW, N),
                         mh.pruned_fluxes.reshape(nH * nW, N, S).contiguous(), flux_cuts)
    traces, names = [], []
    for i, cut in enumerate(tot.flux_cuts):
        traces += [tot.n_above[i].to(torch.float32), tot.flux_above[i]]
        names += [f"count(flux>={cut:g})", f"flux(flux>={cut:g})"]
    traces.append(mh.fluxes.reshape(nH * nW, N, -1).double().sum(-1).to(torch.float32))
    names.append("total_flux")
    if log_target:
        lt = mh.log_target(mh.tiled_image, mh.counts, mh.locs, mh.fluxes)
        traces.append(lt.reshape(nH * nW, N).to(torch.float32))
        names.append("log_target")
    x = torch.stack(traces, dim=1).reshape(nH, nW, len(traces), C, M)  # chain-major, as run()
    return x, tuple(names)


def diagnose_sampler(mh, flux_cuts=(0.0,), log_target=False, *, tail_prob=0.05, num_rho=0):
    """`diagnose` on the traces of a finished MHsampler (`sampler_traces`),
    rows [nH,nW,Q] with `names` naming the Q quantities; accept_rate
    [nH,nW(,C)] is the acceptance rate after the burn-in, frozen is the
    sampler's own (chains stopped by an upper-edge proposal)."""
    x, names = sampler_traces(mh, flux_cuts, log_target)
    out = diagnose(x, tail_prob=tail_prob, num_rho=num_rho)
    out.names = names
    out.accept_rate = mh.accept[..., mh.num_samples_burnin:].float().mean(-1)
    out.frozen = mh.frozen
    return out
