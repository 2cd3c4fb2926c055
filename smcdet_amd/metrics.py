"""Evaluation metrics (the reference's smcdet/metrics.py): sampled catalogs are
matched to a true catalog tile by tile and counted per magnitude bin.

The reference loops over tiles x catalogs in Python with one scipy
`linear_sum_assignment` per pair, which is why it subsamples the catalogs.
Here every (tile, catalog) pair is one wavefront of `smcdet_match_catalogs`
(include/smcdet_hip.h), so all N catalogs of all tiles can be scored
(`num_est_catalogs_to_match=None`).

Differences from the reference, both documented in the header:
  * the matching is the exact lexicographic optimum (most in-tolerance pairs,
    then the smallest sum of their distances); the reference's
    `locs_dist + oob * 1e20` loses the distances to rounding whenever an
    out-of-tolerance pair has to be assigned, and then returns some matching
    with the same number of matches, not necessarily the nearest one;
  * a source with a non-finite location or a non-finite or non-positive flux
    inside the counted slots matches nothing (the reference raises from scipy).
"""
from __future__ import annotations

import torch

from . import _hip
from ._hip import check, dev_f32, lib, ptr, stream_of


def convert_mag_to_nmgy(mag):
    return 10 ** ((22.5 - mag) / 2.5)


def convert_nmgy_to_mag(nmgy):
    return 22.5 - 2.5 * torch.log10(nmgy)


def _counts_i32(counts, name, shape, device):
    if not isinstance(counts, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not counts.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {counts.device}); "
                           "smcdet_amd runs only on MI355X (gfx950)")
    if tuple(counts.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(counts.shape)}, expected {tuple(shape)}")
    return counts.to(device=device, dtype=torch.int32).contiguous()  # the reference's .int()


def match_catalogs(true_counts, true_locs, true_fluxes, est_counts, est_locs, est_fluxes,
                   num_est_catalogs_to_match, locs_tol, mags_tol, mag_bins, *, index=None,
                   return_matches=False):
    """The reference's match_catalogs (metrics.py:8-84) on the device.

    true_counts [T], true_locs [T,St,2], true_fluxes [T,St]; est_counts [T,N],
    est_locs [T,N,Se,2], est_fluxes [T,N,Se] (HIP tensors, kept sources first,
    as SMCsampler's pruned catalogs).  Returns the reference's four
    [T, M, len(mag_bins)] float32 tensors (true total, true matches, est
    total, est matches) on the inputs' device.

    Which catalogs are matched:
      num_est_catalogs_to_match=M, index=None: M catalogs per tile drawn as the
        reference does, `torch.randint(0, N, [M])` once per tile in tile order
        from torch's global CPU generator (the reference's draws on a CPU
        default device under the same torch.manual_seed);
      index=[T,M] integer tensor: catalog index[t,j] is the j-th of tile t;
      num_est_catalogs_to_match=None (and no index): all N catalogs in order.
    return_matches=True appends match_of_true [T,M,St] int32: the est slot
    matched to each true source, or -1.
    """
    true_locs = dev_f32(true_locs, "true_locs")
    true_fluxes = dev_f32(true_fluxes, "true_fluxes")
    est_locs = dev_f32(est_locs, "est_locs")
    est_fluxes = dev_f32(est_fluxes, "est_fluxes")
    dev = true_locs.device
    if true_locs.dim() != 3 or true_locs.shape[-1] != 2:
        raise ValueError(f"true_locs must be [T,St,2], got {tuple(true_locs.shape)}")
    if est_locs.dim() != 4 or est_locs.shape[-1] != 2:
        raise ValueError(f"est_locs must be [T,N,Se,2], got {tuple(est_locs.shape)}")
    T, St = true_locs.shape[:2]
    N, Se = est_locs.shape[1:3]
    if est_locs.shape[0] != T or tuple(true_fluxes.shape) != (T, St) or \
            tuple(est_fluxes.shape) != (T, N, Se):
        raise ValueError("match_catalogs: inconsistent shapes "
                         f"{tuple(true_locs.shape)} {tuple(true_fluxes.shape)} "
                         f"{tuple(est_locs.shape)} {tuple(est_fluxes.shape)}")
    if not (1 <= St <= _hip.MATCH_MAX_SOURCES and 1 <= Se <= _hip.MATCH_MAX_SOURCES and N >= 1):
        raise ValueError(f"match_catalogs: St = {St}, Se = {Se} source slots per catalog outside "
                         f"1..{_hip.MATCH_MAX_SOURCES} (one source per lane of a 64-wide "
                         f"wavefront), or N = {N} < 1")
    tc = _counts_i32(true_counts, "true_counts", (T,), dev)
    ec = _counts_i32(est_counts, "est_counts", (T, N), dev)
    bins = torch.as_tensor(mag_bins, dtype=torch.float32).to(dev).contiguous()
    if bins.dim() != 1 or not 1 <= bins.numel() <= _hip.MATCH_MAX_BINS:
        raise ValueError(f"match_catalogs: mag_bins must hold 1..{_hip.MATCH_MAX_BINS} edges")
    B = bins.numel()

    if index is not None:
        index = torch.as_tensor(index)
        if index.dim() != 2 or index.shape[0] != T or index.is_floating_point():
            raise ValueError(f"index must be a [T,M] integer tensor, got {tuple(index.shape)} "
                             f"{index.dtype}")
        if num_est_catalogs_to_match is not None and index.shape[1] != num_est_catalogs_to_match:
            raise ValueError(f"index has {index.shape[1]} columns, num_est_catalogs_to_match is "
                             f"{num_est_catalogs_to_match}")
        if index.numel() and (int(index.min()) < 0 or int(index.max()) >= N):
            raise ValueError(f"index values must lie in [0, {N})")
        index = index.to(device=dev, dtype=torch.int64).contiguous()
        M = index.shape[1]
    elif num_est_catalogs_to_match is None:
        M = N  # every catalog, in order: a null index in the ABI
    else:
        M = int(num_est_catalogs_to_match)
        if M >= 1:  # the reference's draws, on the CPU generator, one per tile
            index = torch.stack([torch.randint(0, N, [M], device="cpu") for _ in range(T)])
            index = index.to(dev)
    outs = [torch.zeros(T, M, B, device=dev, dtype=torch.float32) for _ in range(4)]
    mot = torch.full((T, M, St), -1, device=dev, dtype=torch.int32) if return_matches else None
    if T > 0 and M > 0:
        check(lib().smcdet_match_catalogs(
            ptr(tc), ptr(true_locs), ptr(true_fluxes), ptr(ec), ptr(est_locs), ptr(est_fluxes),
            ptr(index), T, N, M, St, Se, float(locs_tol), float(mags_tol), ptr(bins), B,
            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(mot),
            stream_of(true_locs)), "smcdet_match_catalogs")
    return (*outs, mot) if return_matches else tuple(outs)


def compute_precision_recall_f1(true_total, true_matches, est_total, est_matches):
    """The reference's compute_precision_recall_f1 (metrics.py:87-92); plain
    torch on whatever device the inputs are on."""
    precision = (est_matches.sum(0) / est_total.sum(0)).nan_to_num(0)
    recall = (true_matches.sum(0) / true_total.sum(0)).nan_to_num(0)
    f1 = ((2 * precision * recall) / (precision + recall)).nan_to_num(0)
    return precision, recall, f1
