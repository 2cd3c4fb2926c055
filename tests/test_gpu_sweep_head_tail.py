"""The MH sweep's head and tail (mh_kernel.hip: everything before and after the
iteration loop): the ancestor gather from indices and from the tile pass's
bins, the persisted rate image copied in through registers with its 1/v image
written from the same registers, the rate image stored before the
log-likelihood sum, write-through or plain (SMCDET_MH_NO_WRITE_THROUGH).

Shapes: T = 2 tiles, N = 10 particles (three workgroups per tile, the last
with two idle waves) and N = 13, S = 10, states in the style of
test_gpu_geometry.PLACES scaled to the tile.  One tile per dispatch path of the
head / tail code: 32x32 R = 8 (compiled-in geometry), the same through
SMCDET_MH_GENERIC_GEOMETRY, 24x40, 16x16, and 8x8 (PSF cache, no 1/v image).
K = 0 makes the sweep a pure gather; K = 1 and K = 70 (past the 64-draw
refill, all four priority quarters) run the loop behind it.  The sampler (bins
hand-over, fused step) takes square tiles only: 24x40 is covered by the direct
sweeps.

Floats are compared by their bits (test_gpu_geometry._bits_equal).
"""
import functools

import numpy as np
import pytest
import torch

from tests._params import M71, p_m71_mh
from tests.test_gpu_geometry import GENERIC, PAD, PLACES, _bits_equal, _model, _prior

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_WT = 65536  # SMCDET_MH_NO_WRITE_THROUGH, include/smcdet_hip.h
T, S, R = 2, 10, 8

# id -> (H, W, debug flags)
TILES = {"32x32": (32, 32, 0), "32x32-generic": (32, 32, GENERIC), "24x40": (24, 40, 0),
         "16x16": (16, 16, 0), "8x8": (8, 8, 0)}
SQUARE = ["32x32", "32x32-generic", "16x16", "8x8"]


@functools.lru_cache(maxsize=None)
def _setup(h, w, N):
    """(image [1,T,h,w], counts, locs, fluxes) of one shape, built once."""
    model = _model(h, w, R)
    torch.manual_seed(100 * h + w)
    tiles = []
    for _ in range(T):
        _, l, f = _prior(0, 40, h, w, rate=0.004).sample(num_catalogs=1, device=DEV)
        tiles.append(model.sample(l, f)[0, 0, :, :, 0])
    image = torch.stack(tiles)[None].contiguous()
    g = torch.Generator().manual_seed(7 * h + w + N)
    n = T * N * S
    locs = torch.rand(n, 2, generator=g) * torch.tensor([float(h), float(w)])
    fluxes = 1.0 + 40.0 * torch.rand(n, generator=g)
    scale = torch.tensor([h / 32.0, w / 32.0])
    lo, hi = torch.tensor([-PAD + 0.05] * 2), torch.tensor([h + PAD - 0.05, w + PAD - 0.05])
    for i, hw in enumerate(PLACES):
        locs[(i * 7) % n] = torch.minimum(torch.maximum(torch.tensor(hw) * scale, lo), hi)
    counts = torch.full((1, T, N), float(S), device=DEV)
    return (image, counts, locs.reshape(1, T, N, S, 2).to(DEV).contiguous(),
            fluxes.reshape(1, T, N, S).to(DEV).contiguous())


def _ancestors(N):
    """A non-identity map with repeats (so some particles have no offspring)."""
    g = torch.Generator().manual_seed(5 + N)
    anc = torch.randint(0, N, (1, T, N), generator=g)
    anc[0, :, 0] = anc[0, :, 1]
    assert not torch.equal(anc[0, 0], torch.arange(N))
    assert all(len(set(anc[0, t].tolist())) < N for t in range(T))
    return anc.to(DEV)


def _draws(K, N, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(comp=torch.randint(0, S, (K, 1, T, N), generator=g, dtype=torch.int32),
                uloc=torch.rand(K, 1, T, N, 2, generator=g),
                uflux=torch.rand(K, 1, T, N, generator=g),
                uacc=torch.rand(K, 1, T, N, generator=g).clamp(min=1e-6))


def _sweep(tile, N, K, state, *, flags=0, ancestors=None, rate_in=None, draws=None):
    """One sweep of K iterations from state = (counts, locs, fluxes); every
    output as a dict of device tensors."""
    from smcdet_amd._rng import PhiloxStream
    h, w, tile_flags = TILES[tile]
    image = _setup(h, w, N)[0]
    counts, locs, fluxes = state
    mh = p_m71_mh(K)
    mh.debug_flags = tile_flags | flags
    mh.rng = PhiloxStream(17)
    rp = None
    if draws is not None:
        rp = dict(draws)
        rp["trace_loga"] = torch.zeros(K, 1, T, N, device=DEV)
        rp["trace_accept"] = torch.zeros(K, 1, T, N, device=DEV, dtype=torch.uint8)
    rate = torch.empty(1, T, N, h * w, device=DEV)
    tau = torch.tensor([[0.05, 0.3]], device=DEV)
    lo, fo, acc = mh.run(image, counts, locs, fluxes, tau, prior=_prior(S, S, h, w),
                         image_model=_model(h, w, R), replay=rp, ancestors=ancestors,
                         rate_in=rate_in, rate_out=rate)
    out = dict(locs=lo, fluxes=fo, counts=mh.last_counts, loglik=mh.last_loglik, rate=rate,
               acc=acc)
    if rp is not None:
        out.update(loga=rp["trace_loga"], accept=rp["trace_accept"])
    torch.cuda.synchronize()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert _bits_equal(a[k], b[k]), k


def _assert_fresh(tile, N, out):
    """The returned log-likelihoods and rate images against fresh evaluations
    of the returned state, at test_gpu_psf_cache.py's tolerances."""
    h, w, _ = TILES[tile]
    model, image = _model(h, w, R), _setup(h, w, N)[0]
    ll = model.loglikelihood(image, out["locs"], out["fluxes"])
    np.testing.assert_allclose(out["loglik"].cpu().numpy(), ll.cpu().numpy(), rtol=2e-6,
                               atol=2e-3)
    fresh = model.rate(out["locs"], out["fluxes"])[0].permute(0, 3, 1, 2).reshape(T, N, h * w)
    np.testing.assert_allclose(out["rate"][0].cpu().numpy(), fresh.cpu().numpy(), rtol=2e-5,
                               atol=2e-3)


def _gather(x, anc):
    """x [1,T,N,...] indexed by anc [1,T,N] along the particle axis."""
    return torch.stack([x[0, t][anc[0, t]] for t in range(T)])[None]


@pytest.mark.parametrize("N", [10, 13])
@pytest.mark.parametrize("tile", list(TILES))
def test_k0_sweep_is_a_pure_gather(tile, N):
    """K = 0: a first sweep renders and persists the rate images of the placed
    state; the second gathers ancestors (int64 indices) and moves nothing:
    state, counts and rate images are the ancestors' bit for bit, and the
    log-likelihood is that of the gathered state."""
    _, counts, locs, fluxes = _setup(*TILES[tile][:2], N)
    # counts that differ between particles (read and gathered, not interpreted:
    # the moved component's range is S without SMCDET_MH_COMPONENT_BY_COUNT)
    counts = (1.0 + torch.arange(T * N, device=DEV).reshape(1, T, N) % S).float().contiguous()
    first = _sweep(tile, N, 0, (counts, locs, fluxes))
    assert _bits_equal(first["locs"], locs) and _bits_equal(first["fluxes"], fluxes)
    _assert_fresh(tile, N, first)
    anc = _ancestors(N)
    out = _sweep(tile, N, 0, (counts, locs, fluxes), ancestors=anc, rate_in=first["rate"])
    assert _bits_equal(out["locs"], _gather(locs, anc))
    assert _bits_equal(out["fluxes"], _gather(fluxes, anc))
    assert _bits_equal(out["counts"], _gather(counts, anc))
    assert _bits_equal(out["rate"], _gather(first["rate"], anc))
    _assert_fresh(tile, N, out)
    # the write-through flag changes nothing
    _assert_same(out, _sweep(tile, N, 0, (counts, locs, fluxes), flags=NO_WT, ancestors=anc,
                             rate_in=first["rate"]))


@pytest.mark.parametrize("K", [1, 70])
@pytest.mark.parametrize("tile", list(TILES))
def test_sweep_from_persisted_image_equals_sweep_from_render(tile, K):
    """A sweep that starts from the persisted rate image (copied in through
    registers, the 1/v image written from them) equals, bit for bit, the sweep
    that renders the same state itself (the 1/v image filled from LDS), Philox
    draws and replayed ones (with the decision trace); the returned
    log-likelihoods and rate images are fresh; plain rate-image stores
    (SMCDET_MH_NO_WRITE_THROUGH) give the same bits."""
    N = 10
    _, counts, locs, fluxes = _setup(*TILES[tile][:2], N)
    state = (counts, locs, fluxes)
    render = _sweep(tile, N, 0, state)  # rate_out = the sweep's own render of the state
    for draws in (None, _draws(K, N, 40 + K)):
        a = _sweep(tile, N, K, state, rate_in=render["rate"], draws=draws)
        b = _sweep(tile, N, K, state, draws=draws)
        _assert_same(a, b)
        _assert_fresh(tile, N, a)
        _assert_same(a, _sweep(tile, N, K, state, flags=NO_WT, rate_in=render["rate"],
                               draws=draws))
    if K == 70:
        assert not _bits_equal(a["locs"], locs)  # the sweep did move
        assert a["accept"].float().mean() > 0.02


@pytest.mark.parametrize("K", [0, 1, 70])
def test_compiled_in_geometry_equals_generic(K):
    """32x32 / R = 8: gather from a persisted image + K iterations, the
    compiled-in geometry's head and tail against the run-time geometry's."""
    N = 13
    _, counts, locs, fluxes = _setup(32, 32, N)
    anc = _ancestors(N)
    outs = []
    for tile in ("32x32", "32x32-generic"):
        first = _sweep(tile, N, 3, (counts, locs, fluxes))
        outs.append((first, _sweep(tile, N, K, (counts, first["locs"], first["fluxes"]),
                                   ancestors=anc, rate_in=first["rate"])))
    _assert_same(outs[0][0], outs[1][0])
    _assert_same(outs[0][1], outs[1][1])


def _sampler_steps(tile, N, K, bins, fused=False, n_steps=2):
    """SMCsampler._step calls from the placed state: the first sweep renders,
    the later ones gather from the previous tile pass's bins (or indices) and
    start from the persisted rate images."""
    from smcdet_amd import _hip
    from smcdet_amd.sampler import SMCsampler
    h, w, flags = TILES[tile]
    image, _, locs, fluxes = _setup(h, w, N)
    mh = p_m71_mh(K)
    mh.debug_flags = flags
    s = SMCsampler.from_tiles(image, _prior(S, S, h, w), _model(h, w, R), mh, N, 0.5, "systematic",
                              M71["flux_detection_threshold"], 100, print_every=10 ** 9, seed=7,
                              device=DEV)
    s.ancestor_bins = bins
    s.fused_step = fused
    s.initialize()
    s.locs, s.fluxes = locs.clone(), fluxes.clone()
    s.loglik = s._fresh_loglik = s.ImageModel.loglikelihood(s.tiled_image, s.locs, s.fluxes)
    s._temper_reweight(with_resample=True)
    trace = []
    for _ in range(n_steps):
        idx, s._pending_idx = s._pending_idx, None
        before = {k: getattr(s, k).clone() for k in ("locs", "fluxes", "counts")}
        if getattr(s, "_rate_valid", False):
            before["rate"] = s._rate[s._rate_cur].clone()
        s._step(idx)
        torch.cuda.synchronize()
        st = {k: getattr(s, k).clone() for k in
              ("temperature", "log_normalizing_constant", "ess", "weights", "locs", "fluxes",
               "counts", "loglik", "mutation_acc_rates")}
        st["rate"] = s._rate[s._rate_cur].clone()
        st["idx"] = _hip.as_index(idx).clone()
        trace.append((before, st))
    return trace


@pytest.mark.parametrize("K", [0, 1, 70])
@pytest.mark.parametrize("tile", SQUARE)
def test_ancestors_from_bins_equal_indices(tile, K):
    """N = 13: the sweeps of two sampler steps with the ancestors handed over
    as the tile pass's bins and as int64 indices are bitwise equal; with K = 0
    each step is the gather of its indices."""
    N = 13
    a = _sampler_steps(tile, N, K, bins=True)
    b = _sampler_steps(tile, N, K, bins=False)
    for (_, x), (_, y) in zip(a, b):
        _assert_same(x, y)
    if K == 0:
        for before, st in a:
            idx = st["idx"].reshape(1, T, N)
            for k in ("locs", "fluxes", "counts"):
                assert _bits_equal(st[k], _gather(before[k].reshape(1, T, N, *before[k].shape[3:]),
                                                  idx).reshape(st[k].shape)), k
            if "rate" in before:
                h, w, _ = TILES[tile]
                assert _bits_equal(st["rate"].reshape(1, T, N, h * w),
                                   _gather(before["rate"].reshape(1, T, N, h * w), idx))


@pytest.mark.parametrize("tile", ["32x32", "16x16"])
def test_fused_step_equals_split_step(tile):
    """N = 12 (whole workgroups, as the fused tail needs): the fused step,
    whose stores and fences are unchanged, against the two launches."""
    from smcdet_amd import _hip
    N, K = 12, 70
    h, w, _ = TILES[tile]
    assert _hip.lib().smcdet_mh_sweep_step_fused(_hip.ref(_model(h, w, R)._cmodel()), N, S, 0) == 1
    a = _sampler_steps(tile, N, K, bins=True, fused=True, n_steps=3)
    b = _sampler_steps(tile, N, K, bins=True, fused=False, n_steps=3)
    for (_, x), (_, y) in zip(a, b):
        _assert_same(x, y)
