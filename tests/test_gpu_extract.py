"""smcdet_amd.extract on the GPU against the numpy oracle
(tests/_extract_oracle.py, pinned by tests/test_extract_oracle_host.py).

Labels, counts and segmentation maps must be equal; fluxes and locations may
differ by one float32 ulp from the oracle's float64 values rounded (the device
is free in the order of its float64 sums, about 1e-16 relative, which can move
a rounding boundary but nothing else).  That freedom could flip a decision
only where a float64 comparison is a near tie, so every case first asserts,
on the CPU side, that the oracle's smallest significance margin and smallest
clean margin exceed 1e-9: a condition on the seeds, not a tolerance."""
import functools

import numpy as np
import pytest
import torch

from smcdet_amd import extract
from tests import _extract_oracle as O
from tests import _metrics_oracle as MO
from tests._extract_cases import CASES

pytestmark = pytest.mark.gpu

BG, ETA = 104.15, 1.936  # M71-like background (ADU) and noise factor: var = ETA * rate
MARGIN = 1e-9

# name -> (seed, T, H, W, thresh, deblend_nthresh, sources per pixel)
SHAPES = {
    "8x8": (11, 48, 8, 8, 1.5, 64, 0.05),     # one pixel per lane
    "5x7": (12, 24, 5, 7, 1.5, 32, 0.06),     # idle lanes
    "1x64": (13, 12, 1, 64, 2.0, 16, 0.05),   # one row: up to 32 objects on the 64-pixel path
    "16x24": (14, 6, 16, 24, 2.0, 32, 0.03),  # strided, 6 pixels per lane
    "32x32": (15, 6, 32, 32, 1.5, 32, 0.02),  # strided, every lane slot used
}
MINAREA, CONT = [1, 5], [1e-4, 0.5]
BETAS = [0.1, 10.0]  # a second launch with clean=False adds beta = 0


def make_tiles(seed, T, H, W, density):
    """Poisson / normal tiles: a Gaussian stand-in PSF (sigma 1.2 px) on the M71
    background, Pareto fluxes; per-image backgrounds so that the [T] arguments
    are exercised."""
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:H, 0:W] + 0.5
    bg = (BG + 0.25 * np.arange(T)).astype(np.float32)
    images = np.empty((T, H, W), np.float32)
    for t in range(T):
        rate = np.full((H, W), float(bg[t]))
        for _ in range(rng.poisson(density * H * W) + 1):
            h, w = rng.uniform(-1, H + 1), rng.uniform(-1, W + 1)
            f = min(300.0 * (1 - rng.uniform()) ** (-1 / 0.7), 2e5)
            rate += f * np.exp(-((ii - h) ** 2 + (jj - w) ** 2) / (2 * 1.44)) / (2 * np.pi * 1.44)
        images[t] = rng.poisson(rate) + rng.normal(0, np.sqrt((ETA - 1) * rate))
    return images, bg, np.sqrt(ETA * bg).astype(np.float32)


def to_np(r):
    return [None if x is None else x.cpu().numpy() for x in
            (r.counts, r.locs, r.fluxes, r.n_found, r.segmap)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, settings [12,4], oracle, device outputs) of a shape, computed once:
    8 settings with cleaning in one launch and the 4 without in another."""
    seed, T, H, W, thresh, n, density = SHAPES[name]
    images, bg, sigma = make_tiles(seed, T, H, W, density)
    dev = [torch.from_numpy(x).cuda() for x in (images, bg, sigma)]
    a = extract.extract_grid(*dev, [thresh], MINAREA, n, CONT, True, BETAS, 16,
                             segmentation_map=True)
    b = extract.extract_grid(*dev, [thresh], MINAREA, n, CONT, False, BETAS, 16,
                             segmentation_map=True)
    settings = np.concatenate([a.settings.numpy(), b.settings.numpy()])
    assert a.settings.shape == (8, 4) and b.settings.shape == (4, 4)
    np.testing.assert_array_equal(settings[:8], O.settings_grid([thresh], MINAREA, CONT, BETAS))
    np.testing.assert_array_equal(settings[8:], O.settings_grid([thresh], MINAREA, CONT, [0.0]))
    got = [np.concatenate([x, y], axis=1) for x, y in zip(to_np(a), to_np(b))]
    want = O.extract_grid(images, bg, sigma, settings, n, 16)
    return (images, bg, sigma, dev, n), settings, want, got


def assert_within_one_ulp(got, want, what):
    assert got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    assert (err <= np.spacing(np.abs(want[ok]))).all(), (what, err.max())


def assert_equals_oracle(got, want, K):
    counts, locs, fluxes, n_found, segmap = got
    np.testing.assert_array_equal(n_found, want.n_found)
    np.testing.assert_array_equal(counts, want.counts)
    np.testing.assert_array_equal(counts, np.minimum(n_found, K))
    np.testing.assert_array_equal(segmap, want.segmap)
    assert_within_one_ulp(fluxes, want.fluxes, "fluxes")
    assert_within_one_ulp(locs, want.locs, "locs")
    past = np.arange(K)[None, None, :] >= counts[..., None]
    assert np.isnan(locs[past]).all() and not np.isnan(locs[~past]).any()
    assert (fluxes[past] == 0).all() and (fluxes[~past] > 0).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_oracle(name):
    _, settings, want, got = case(name)
    # the condition on the seeds: no float64 decision of any problem is a near tie
    assert want.sig_margin.min() > MARGIN, want.sig_margin.min()
    assert want.clean_margin.min() > MARGIN, want.clean_margin.min()
    assert got[0].dtype == got[3].dtype == got[4].dtype == np.int32
    assert_equals_oracle(got, want, 16)
    # the case is not trivial: blends were split, objects absorbed, the cap reached somewhere
    nf = want.n_found
    assert nf.max() >= 2 and (nf[:, settings[:, 2] < 0.1] > nf[:, settings[:, 2] > 0.1]).any()
    assert (nf[:, 8:] >= nf[:, [0, 2, 4, 6]]).all()  # cleaning only removes
    if name in ("8x8", "32x32"):
        assert (nf[:, 8:] > nf[:, [0, 2, 4, 6]]).any() and (nf[:, 8:] > nf[:, [1, 3, 5, 7]]).any()
    if name == "32x32":
        assert (nf > 16).any()


@pytest.mark.parametrize("name", ["5x7", "16x24"])
def test_grid_launch_equals_single_launches_bit_for_bit(name):
    (_, _, _, dev, n), settings, _, got = case(name)
    for g, (thresh, minarea, cont, beta) in enumerate(settings):
        r = extract.extract(*dev, thresh, int(minarea), n, cont, beta > 0,
                            beta if beta > 0 else 1.0, 16, segmentation_map=True)
        for x, y in zip(to_np(r), got):
            assert x.tobytes() == np.ascontiguousarray(y[:, g]).tobytes(), g


@pytest.mark.parametrize("name", ["8x8", "32x32"])
def test_two_runs_are_identical(name):
    (_, _, _, dev, n), settings, _, got = case(name)
    thresh = settings[0, 0]
    again = to_np(extract.extract_grid(*dev, [thresh], MINAREA, n, CONT, True, BETAS, 16,
                                       segmentation_map=True))
    for x, y in zip(again, got):
        assert x.tobytes() == np.ascontiguousarray(y[:, :8]).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_hand_worked_cases(name):
    image, kw = CASES[name]
    kw = dict(kw)
    K, beta = kw.pop("K", 16), kw.pop("clean_param", 1.0)
    want = O.extract_one(image, 0.0, 1.0, clean_param=beta, K=K, **kw)
    assert min(want.sig_margin, want.clean_margin) > MARGIN
    r = extract.extract(torch.from_numpy(image).cuda(), 0.0, 1.0, clean=beta > 0,
                        clean_param=beta if beta > 0 else 1.0, max_detections=K,
                        segmentation_map=True, **kw)
    counts, locs, fluxes, n_found, segmap = to_np(r)
    assert counts.shape == (1,) and locs.shape == (1, K, 2) and segmap.shape == (1,) + image.shape
    assert counts[0] == want.count and n_found[0] == want.n_found
    np.testing.assert_array_equal(segmap[0], want.segmap)
    assert_within_one_ulp(fluxes[0], want.fluxes, "fluxes")
    assert_within_one_ulp(locs[0], want.locs, "locs")


def serpentine():
    """A one-pixel-wide path through 32x32, brightening along its length: one
    root of 527 pixels that shrinks from its head at every level."""
    v = np.zeros((32, 32), np.float32)
    k = 0
    for i in range(0, 32, 2):
        cols = range(32) if (i // 2) % 2 == 0 else range(31, -1, -1)
        for j in cols:
            v[i, j] = 10 + 0.01 * k
            k += 1
        if i + 1 < 31:
            v[i + 1, cols[-1]] = 10 + 0.01 * k
            k += 1
    return v


def checkerboard():
    """256 isolated pixels, all different."""
    v = np.zeros((32, 32), np.float32)
    ii, jj = np.mgrid[0:32:2, 0:32:2]
    v[ii, jj] = 10 + 0.01 * ((7 * ii + 13 * jj) % 256)
    return v


@pytest.mark.parametrize("make, n_found, K", [(serpentine, 1, 16), (checkerboard, 256, 64)])
def test_worst_cases_of_the_strided_path(make, n_found, K):
    image = make()
    got, wants = [], []
    for beta in (0.0, 10.0):
        want = O.extract_one(image, 0.0, 1.0, 1.0, 1, 32, 0.005, beta, K)
        assert want.n_found == n_found and min(want.sig_margin, want.clean_margin) > MARGIN
        wants.append(want)
    r = extract.extract_grid(torch.from_numpy(image).cuda(), 0.0, 1.0, [1.0], [1], 32, [0.005],
                             True, [10.0], K, segmentation_map=True)
    got.append(to_np(extract.extract(torch.from_numpy(image).cuda(), 0.0, 1.0, 1.0, 1, 32, 0.005,
                                     False, max_detections=K, segmentation_map=True)))
    got.append([x[:, 0] for x in to_np(r)])
    for (counts, locs, fluxes, nf, segmap), want in zip(got, wants):
        assert counts[0] == min(n_found, K) and nf[0] == n_found
        np.testing.assert_array_equal(segmap[0], want.segmap)
        assert segmap.max() == n_found
        assert_within_one_ulp(fluxes[0], want.fluxes, "fluxes")
        assert_within_one_ulp(locs[0], want.locs, "locs")


def test_conveniences_of_extract():
    (images, bg, sigma, dev, n), settings, want, got = case("5x7")
    g = 1  # thresh, minarea 1, cont 1e-4, beta 10
    thresh, minarea, cont, beta = settings[g]
    # one [H,W] image, float background and sigma, no map, fluxes in other units
    r = extract.extract(dev[0][3], float(bg[3]), float(sigma[3]), thresh, int(minarea), n, cont,
                        True, beta, 16, flux_scale=241.03)
    assert r.segmap is None and r.counts.shape == (1,) and r.counts.is_cuda
    assert int(r.counts[0]) == got[0][3, g]
    np.testing.assert_allclose(r.fluxes.cpu().numpy()[0], got[2][3, g] / np.float32(241.03),
                               rtol=2.5e-7)  # (a float32 division or a product with 1 / scale)
    np.testing.assert_array_equal(r.locs.cpu().numpy()[0], got[1][3, g])
    # a smaller cap keeps the head of the list
    r = extract.extract(*dev, thresh, int(minarea), n, cont, True, beta, 2)
    np.testing.assert_array_equal(r.counts.cpu().numpy(), np.minimum(got[3][:, g], 2))
    np.testing.assert_array_equal(r.fluxes.cpu().numpy(), got[2][:, g, :2])
    np.testing.assert_array_equal(r.n_found.cpu().numpy(), got[3][:, g])


def planted(T=12, H=8, scale=241.03):
    """Tiles with a known truth: one to three sources well inside the tile."""
    rng = np.random.default_rng(21)
    ii, jj = np.mgrid[0:H, 0:H] + 0.5
    images = np.empty((T, H, H), np.float32)
    counts = np.zeros(T, np.int32)
    locs = np.zeros((T, 3, 2), np.float32)
    fluxes = np.zeros((T, 3), np.float32)
    for t in range(T):
        rate = np.full((H, H), BG)
        counts[t] = 1 + t % 3
        for s in range(counts[t]):
            h, w = rng.uniform(1, H - 1, 2)
            f = 10 ** rng.uniform(3.0, 4.3)  # ADU
            rate += f * np.exp(-((ii - h) ** 2 + (jj - w) ** 2) / (2 * 1.44)) / (2 * np.pi * 1.44)
            locs[t, s], fluxes[t, s] = (h, w), f / scale
        images[t] = rng.poisson(rate) + rng.normal(0, np.sqrt((ETA - 1) * rate))
    return images, counts, locs, fluxes


def test_tune_returns_the_oracles_f1_and_setting():
    scale, K, bins, tol = 241.03, 8, np.array([14.0, 22.0], np.float32), 0.5
    images, tc, tl, tf = planted(scale=scale)
    sigma = float(np.sqrt(ETA * BG))
    grid = ([1.5, 4.0], [1, 5], [0.005], [0.1, 10.0])
    settings = O.settings_grid(*grid)
    want = O.extract_grid(images, BG, sigma, settings, 32, K)
    assert want.sig_margin.min() > MARGIN and want.clean_margin.min() > MARGIN
    est_fluxes = (torch.from_numpy(want.fluxes) / scale).numpy()
    # no pair of the matching sits within 1e-4 of a tolerance (a float32 ulp cannot flip it)
    for t in range(len(tc)):
        for g in range(len(settings)):
            m = want.counts[t, g]
            dist, dmag, _ = MO.pair_tables(*[torch.from_numpy(x) for x in (
                tl[t, :tc[t]], tf[t, :tc[t]], want.locs[t, g, :m], est_fluxes[t, g, :m])], tol, tol)
            for x in (dist, dmag):
                assert not ((x - tol).abs() < 1e-4).any()
    index = np.tile(np.arange(len(settings)), (len(tc), 1))
    tt, tm, et, em, _ = MO.match_catalogs(tc, tl, tf, want.counts, want.locs, est_fluxes, index,
                                          tol, tol, bins)
    tt, tm, et, em = [torch.from_numpy(x).sum(0) for x in (tt, tm, et, em)]
    precision, recall = (em / et).nan_to_num(0), (tm / tt).nan_to_num(0)
    f1 = ((2 * precision * recall) / (precision + recall)).nan_to_num(0)[:, -1].numpy()
    assert f1.max() > 0.5 and f1.min() < f1.max()  # the grid matters

    args = [torch.from_numpy(x).cuda() for x in (images,)] + [BG, sigma] + \
        [torch.from_numpy(x).cuda() for x in (tc, tl, tf)]
    r = extract.tune(*args, *grid, deblend_nthresh=32, max_detections=K, locs_tol=tol,
                     mags_tol=tol, mag_bins=bins, flux_scale=scale)
    assert r.f1.is_cuda and r.f1.shape == (8,)
    np.testing.assert_allclose(r.f1.cpu().numpy(), f1, rtol=1e-6)
    best = int(np.flatnonzero(f1 == f1.max())[0])
    assert r.best_index == best
    assert r.best == dict(thresh=settings[best, 0], minarea=int(settings[best, 1]),
                          deblend_cont=settings[best, 2], clean_param=settings[best, 3])
    # chunked over the settings: the same numbers
    per_setting = len(tc) * (8 + 12 * K + 16 * len(bins))
    r3 = extract.tune(*args, *grid, deblend_nthresh=32, max_detections=K, locs_tol=tol,
                      mags_tol=tol, mag_bins=bins, flux_scale=scale, max_bytes=3 * per_setting)
    assert r3.f1.cpu().numpy().tobytes() == r.f1.cpu().numpy().tobytes()
    assert r3.best_index == r.best_index
