"""The MH sweep's wave-uniform loop control.

One particle per wavefront: the iteration count K of a wave follows from its
own particle's count (SMCDET_MH_COMPONENT_BY_COUNT) and its tile's temperature
(SMCDET_MH_SKIP_DONE), and the kernel takes both from the wave's first lane so
the K loop is scalar.  These tests pin that K stays per wave (a workgroup of
four particles with four different counts) and that a finished tile's waves
leave their gathered particles alone next to a live tile.

All draws are replayed, so a particle's moves do not depend on where in a
launch it sits.  Shapes: 8x8 (the one-slot instantiation) and 16x16 tiles,
N = 8 (two workgroups), S = 3, K = 70 (past the 64-draw refill, several
21-entry proposal batches, all four priority quarters).
"""
import numpy as np
import pytest
import torch

from tests._params import M71, p_m71_model, p_m71_prior

pytestmark = pytest.mark.gpu
DEV = "cuda"
SKIP_DONE = 4  # include/smcdet_hip.h
K, S, N = 70, 3, 8
MIXED_COUNTS = [0, 1, 3, 3, 0, 0, 2, 3]  # workgroups {0, 1, 3, 3} and {0, 0, 2, 3}


def N_(x):
    return x.detach().cpu().numpy()


def _mh(**kw):
    from smcdet_amd.kernel import SingleComponentMH
    return SingleComponentMH(K, 0.1, 2.5, M71["flux_lower"], M71["flux_upper"], **kw)


def _image(H, seed, n_w=1):
    """n_w tiles of HxH side by side, [1, n_w, H, H]"""
    torch.manual_seed(seed)
    tiles = []
    for _ in range(n_w):
        _, l, f = p_m71_prior(H, 0, 40).sample(num_catalogs=1, device=DEV)
        tiles.append(p_m71_model(H).sample(l, f)[0, 0, :, :, 0])
    return torch.stack(tiles)[None].contiguous()


def _particles(H, want, seed):
    """Particles of a count-stratified population (padded to S sources) with
    the counts `want`, in that order: counts [1,1,n], locs [1,1,n,S,2], fluxes."""
    torch.manual_seed(seed)
    prior = p_m71_prior(H, 0, S)
    counts, locs, fluxes = prior.sample(num_tiles_per_side=1, stratify_by_count=True,
                                        num_catalogs_per_count=len(want), device=DEV)
    c = N_(counts)[0, 0]
    used, idx = set(), []
    for w in want:
        i = next(i for i in range(len(c)) if int(c[i]) == w and i not in used)
        used.add(i)
        idx.append(i)
    idx = torch.tensor(idx, device=DEV)
    return (counts[:, :, idx].contiguous(), locs[:, :, idx].contiguous(),
            fluxes[:, :, idx].contiguous())


def _draws(seed, n_t, n, comp_max):
    """Replayed draws [K, 1, n_t, n]; comp below comp_max[n] (per particle)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(K, 1, n_t, n, generator=g)
    cm = torch.as_tensor(comp_max, dtype=torch.float32).clamp(min=1.0)
    comp = torch.minimum((u * cm).floor(), cm - 1).to(torch.int32)
    return dict(comp=comp.contiguous(),
                uloc=torch.rand(K, 1, n_t, n, 2, generator=g),
                uflux=torch.rand(K, 1, n_t, n, generator=g),
                uacc=torch.rand(K, 1, n_t, n, generator=g).clamp(min=1e-6))


def _take(draws, sel, t=None):
    """The draws of particles `sel` (of tile t, as a one-tile launch)."""
    out = {}
    for k, v in draws.items():
        v = v if t is None else v[:, :, t:t + 1]
        out[k] = v[:, :, :, sel].contiguous()
    return out


def _sweep(mh, img, counts, locs, fluxes, tau, draws, prior, model, **kw):
    n_t, n = locs.shape[1], locs.shape[2]
    rp = dict(draws)
    rp["trace_loga"] = torch.zeros(K, 1, n_t, n, device=DEV)
    rp["trace_accept"] = torch.zeros(K, 1, n_t, n, device=DEV, dtype=torch.uint8)
    lo, fo, _ = mh.run(img, counts, locs, fluxes, torch.tensor([tau], device=DEV), prior=prior,
                       image_model=model, replay=rp, **kw)
    torch.cuda.synchronize()
    return dict(locs=N_(lo), fluxes=N_(fo), loglik=N_(mh.last_loglik),
                accept=N_(rp["trace_accept"]), loga=N_(rp["trace_loga"]))


@pytest.mark.parametrize("H", [8, 16])
def test_iteration_count_is_per_wave_not_per_workgroup(H):
    """Counts {0, 1, 3, 3 | 0, 0, 2, 3} in one launch against the same
    particles in one launch per count: bit-equal states, log-likelihoods and
    accept traces; count-0 particles come back unchanged."""
    model, prior = p_m71_model(H), p_m71_prior(H, 0, S)
    img = _image(H, 3)
    counts, locs, fluxes = _particles(H, MIXED_COUNTS, 11)
    assert N_(counts)[0, 0].tolist() == MIXED_COUNTS
    draws = _draws(5, 1, N, MIXED_COUNTS)
    mh = _mh()
    mh.component_by_count = True
    mixed = _sweep(mh, img, counts, locs, fluxes, [0.3], draws, prior, model)
    c = np.array(MIXED_COUNTS)
    for cnt in sorted(set(MIXED_COUNTS)):
        sel = np.flatnonzero(c == cnt)
        st = torch.tensor(sel, device=DEV)
        alone = _sweep(mh, img, counts[:, :, st].contiguous(), locs[:, :, st].contiguous(),
                       fluxes[:, :, st].contiguous(), [0.3], _take(draws, torch.tensor(sel)),
                       prior, model)
        for k in ("locs", "fluxes", "loglik"):
            np.testing.assert_array_equal(mixed[k][:, :, sel], alone[k], err_msg=f"{k} count {cnt}")
        for k in ("accept", "loga"):
            np.testing.assert_array_equal(mixed[k][:, :, :, sel], alone[k],
                                          err_msg=f"{k} count {cnt}")
    zero = c == 0
    np.testing.assert_array_equal(mixed["locs"][:, :, zero], N_(locs)[:, :, zero])
    np.testing.assert_array_equal(mixed["fluxes"][:, :, zero], N_(fluxes)[:, :, zero])
    assert not mixed["accept"][:, :, :, zero].any()
    # the others did move, and a particle's padded sources did not
    assert mixed["accept"][:, :, :, ~zero].any(axis=0).all()
    pad = np.arange(S)[None] >= c[:, None]
    np.testing.assert_array_equal(mixed["fluxes"][0, 0][pad], N_(fluxes)[0, 0][pad])


@pytest.mark.parametrize("H", [8, 16])
def test_skip_done_tile_next_to_a_live_tile(H):
    """Two tiles, the first at temperature 1 with SMCDET_MH_SKIP_DONE: its
    output is its gathered input exactly; the live tile equals a launch of
    that tile alone."""
    model, prior = p_m71_model(H), p_m71_prior(H, S, S)
    img = _image(H, 4, n_w=2)
    torch.manual_seed(12)
    counts, locs, fluxes = prior.sample(num_tiles_per_side=1, stratify_by_count=True,
                                        num_catalogs_per_count=2 * N, device=DEV)
    # [1, 1, 2N, ...] -> two tiles of N particles
    counts = counts.reshape(1, 2, N).contiguous()
    locs = locs.reshape(1, 2, N, S, 2).contiguous()
    fluxes = fluxes.reshape(1, 2, N, S).contiguous()
    g = torch.Generator().manual_seed(6)
    anc = torch.randint(0, N, (1, 2, N), generator=g).to(DEV)
    draws = _draws(7, 2, N, [S] * N)
    both = _sweep(_mh(), img, counts, locs, fluxes, [1.0, 0.4], draws, prior, model,
                  ancestors=anc, flags=SKIP_DONE)
    a0 = N_(anc)[0, 0]
    np.testing.assert_array_equal(both["locs"][0, 0], N_(locs)[0, 0][a0])
    np.testing.assert_array_equal(both["fluxes"][0, 0], N_(fluxes)[0, 0][a0])
    assert not both["accept"][:, :, 0].any()
    live = _sweep(_mh(), img[:, 1:2].contiguous(), counts[:, 1:2].contiguous(),
                  locs[:, 1:2].contiguous(), fluxes[:, 1:2].contiguous(), [0.4],
                  _take(draws, torch.arange(N), t=1), prior, model,
                  ancestors=anc[:, 1:2].contiguous(), flags=SKIP_DONE)
    for k in ("locs", "fluxes", "loglik"):
        np.testing.assert_array_equal(both[k][:, 1:2], live[k], err_msg=k)
    for k in ("accept", "loga"):
        np.testing.assert_array_equal(both[k][:, :, 1:2], live[k], err_msg=k)
    assert live["accept"].any(axis=0).all()
