"""smcdet_amd.condense on the GPU against the CPU oracle
(tests/_condense_oracle.py): the source map on every dispatch path (LDS grid /
global grid, one chunk of particles / several), the peaks on hand-worked and
sampled maps, the float64 moments with their summation-order bound, and the
whole pipeline on a synthetic posterior with planted presence counts."""
import numpy as np
import pytest
import torch

from smcdet_amd import condense, metrics
from tests import _condense_oracle as O

pytestmark = pytest.mark.gpu

BOX = (-2.0, -2.0, 10.0, 8.0)  # 12 x 10 px: a 48 x 40 grid at 4 cells per pixel
C, GH, GW = 4, 48, 40
EPS = 2.0 ** -23


def cuda(*xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def tile_boxes_of(T):
    lo = np.stack([-2.0 - 0.25 * np.arange(T), -2.0 + 0.5 * np.arange(T)], -1)
    return np.concatenate([lo, lo + [12.0, 10.0]], -1).astype(np.float32)


def weights_of(T, N, seed=7):
    """multiples of 2^-10 in (0, 2]"""
    return (np.random.default_rng(seed).integers(1, 2049, (T, N)) / 1024.0).astype(np.float32)


def run_map(case, box=BOX, c=C, weights=None, tile_boxes=None, with_flux=False):
    counts, locs, fluxes = case
    sm = condense.source_map(*cuda(counts, locs, fluxes), box=box, cells_per_pixel=c,
                             weights=cuda(weights)[0], tile_boxes=cuda(tile_boxes)[0],
                             with_flux=with_flux)
    assert sm.count.dtype == torch.float32 and sm.count.is_cuda
    return sm


def check_map(sm, want, weighted, with_flux):
    """Unweighted counts are exact; weighted sums and fluxes are within
    n * 2^-23 * want (each float32 add costs at most half an ulp of the sum)."""
    count, outside = sm.count.cpu().numpy(), sm.outside.cpu().numpy()
    assert count.shape == want["count"].shape
    if not weighted:
        np.testing.assert_array_equal(count, want["count"])
        np.testing.assert_array_equal(outside, want["outside"])
        np.testing.assert_array_equal(count.astype(np.float64).sum((1, 2)) + outside,
                                      want["n_counted"])
    else:
        assert (np.abs(count - want["count"]) <= want["n_cell"] * EPS * want["count"]).all()
        assert (np.abs(outside - want["outside"])
                <= want["n_outside"] * EPS * want["outside"]).all()
    if with_flux:
        flux = sm.flux.cpu().numpy()
        err = np.abs(flux - want["flux"])
        print("flux map: max err / bound",
              float((err / np.maximum(want["n_cell"] * EPS * want["flux"], 1e-300)).max()))
        assert (err <= want["n_cell"] * EPS * want["flux"]).all()
        assert (flux[want["n_cell"] == 0] == 0).all()
    else:
        assert sm.flux is None


@pytest.fixture(scope="module")
def mapcase():
    """The shared catalogs (T = 3, N = 257: two chunks of particles, S = 5) and
    their oracle map, computed once and never modified."""
    case = O.map_case()
    lo = np.tile(np.asarray(BOX[:2]), (3, 1))
    return case, O.source_map(*case, lo, C, GH, GW)


@pytest.fixture(scope="module")
def boxcase():
    tb = tile_boxes_of(3)
    case = O.map_case(seed=4, tile_boxes=tb)
    return case, tb, O.source_map(*case, tb[:, :2], C, GH, GW)


def test_map_unweighted_shared_box(mapcase):
    case, want = mapcase
    assert want["outside"].min() > 0 and (want["n_cell"] > 0).sum() > 300
    sm = run_map(case, with_flux=True)
    assert tuple(sm.count.shape) == (3, GH, GW) and sm.cells_per_pixel == C and sm.box == BOX
    check_map(sm, want, False, True)
    np.testing.assert_array_equal(sm.total_weight.cpu().numpy(), [257.0] * 3)
    again = run_map(case)  # counts only: identical on every run
    assert torch.equal(again.count, sm.count) and torch.equal(again.outside, sm.outside)
    check_map(again, want, False, False)


def test_map_unweighted_tile_boxes(boxcase):
    case, tb, want = boxcase
    sm = run_map(case, tile_boxes=tb, with_flux=True)
    check_map(sm, want, False, True)
    # the boxes matter: the shared box bins these catalogs differently
    assert not np.array_equal(run_map(case).count.cpu().numpy(), want["count"])


def test_map_weighted(mapcase, boxcase):
    case, _ = mapcase
    w = weights_of(3, 257)
    lo = np.tile(np.asarray(BOX[:2]), (3, 1))
    check_map(run_map(case, weights=w, with_flux=True),
              O.source_map(*case, lo, C, GH, GW, weights=w), True, True)
    case, tb, _ = boxcase
    check_map(run_map(case, weights=w, tile_boxes=tb),
              O.source_map(*case, tb[:, :2], C, GH, GW, weights=w), True, False)


def test_map_one_chunk(mapcase):
    """N = 256 is one workgroup per tile, N = 257 (the shared case) two."""
    case = tuple(x[:, :256] for x in mapcase[0])
    lo = np.tile(np.asarray(BOX[:2]), (3, 1))
    check_map(run_map(case, with_flux=True), O.source_map(*case, lo, C, GH, GW), False, True)


def wide_case(Gh, Gw, T=2, N=300, S=3, seed=5):
    """Uniform sources over a Gh x Gw px box (1 cell per pixel) and 1 px beyond."""
    rng = np.random.default_rng(seed)
    locs = rng.uniform([-1.0, -1.0], [Gh + 1.0, Gw + 1.0], (T, N, S, 2))
    g = np.abs(locs - np.round(locs)) < 1e-3
    locs[g] += 0.01
    fluxes = rng.uniform(0.5, 50.0, (T, N, S)).astype(np.float32)
    counts = rng.integers(0, S + 1, (T, N)).astype(np.int32)
    return counts, locs.astype(np.float32), fluxes


@pytest.mark.parametrize("Gh,Gw,with_flux,in_lds", [
    (10, 2048, True, True),    # 2 x 20480 cells: exactly the 160 KiB of LDS
    (12, 1707, True, False),   # 2 x 20484 cells: the smallest grid past it, global adds
    (12, 1707, False, True),   # the same grid, counts only: 80 KiB, above the 64 KiB default
])
def test_map_lds_and_global_grids(Gh, Gw, with_flux, in_lds):
    assert (Gh * Gw * 4 * (2 if with_flux else 1) <= 160 * 1024) == in_lds
    case = wide_case(Gh, Gw)
    want = O.source_map(*case, np.zeros((2, 2)), 1, Gh, Gw)
    assert want["outside"].min() > 0
    sm = run_map(case, box=(0.0, 0.0, float(Gh), float(Gw)), c=1, with_flux=with_flux)
    check_map(sm, want, False, with_flux)
    w = weights_of(2, 300)
    check_map(run_map(case, box=(0.0, 0.0, float(Gh), float(Gw)), c=1, weights=w,
                      with_flux=with_flux),
              O.source_map(*case, np.zeros((2, 2)), 1, Gh, Gw, weights=w), True, with_flux)


def test_map_limits_raise():
    counts, locs, fluxes = cuda(*O.map_case(T=1, N=8))
    with pytest.raises(ValueError, match="cells_per_pixel"):
        condense.source_map(counts, locs, fluxes, box=BOX, cells_per_pixel=9)
    with pytest.raises(ValueError, match="2048"):
        condense.source_map(counts, locs, fluxes, box=(0.0, 0.0, 600.0, 8.0), cells_per_pixel=4)
    sm = condense.source_map(counts, locs, fluxes, box=(0.0, 0.0, 100.0, 100.0), cells_per_pixel=4)
    with pytest.raises(ValueError, match="32768"):
        condense.find_seeds(sm)
    with pytest.raises(ValueError, match="max_seeds"):
        condense.find_seeds(sm, max_seeds=65)
    big = torch.zeros(1, 8, 65, 2, device="cuda"), torch.ones(1, 8, 65, device="cuda")
    with pytest.raises(ValueError, match="64"):
        condense.condense(torch.zeros(1, 8, device="cuda"), *big, box=BOX)


# ---- peaks -----------------------------------------------------------------------
def run_seeds(count_map, min_mass, q, p, K, box, c, tile_boxes=None):
    """find_seeds on a given map with min_mass [T] (min_prob = 1 of that total)."""
    T = count_map.shape[0]
    smap = condense.SourceMap(cuda(np.asarray(count_map, np.float32))[0], None,
                              torch.zeros(T, device="cuda"), box, c, cuda(tile_boxes)[0],
                              cuda(np.asarray(min_mass, np.float64))[0], None)
    s = condense.find_seeds(smap, smooth_radius=q, nms_radius=p, min_prob=1.0, max_seeds=K)
    assert s.n_seeds.dtype == torch.int32 and s.cell.dtype == torch.int32
    return [x.cpu().numpy() for x in (s.n_seeds, s.cell, s.mass, s.locs)]


def check_seeds(got, want):
    """n_seeds, cells and masses equal; seed_locs within 1e-4 px (exact integer
    sums, a handful of roundings at no more than 64 px)."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2].astype(np.float32))
    np.testing.assert_array_equal(np.isnan(got[3]), np.isnan(want[3]))
    np.testing.assert_allclose(got[3], want[3], rtol=0, atol=1e-4)


@pytest.mark.parametrize("case", O.PEAK_CASES, ids=[c["name"] for c in O.PEAK_CASES])
def test_peaks_hand_worked(case):
    Gh, Gw = case["map"].shape
    got = run_seeds(case["map"][None], [case["min_mass"]], case["q"], case["p"], case["K"],
                    (0.0, 0.0, float(Gh), float(Gw)), 1)
    n = len(case["cells"])
    assert got[0].tolist() == [n] and got[1][0, :n].tolist() == case["cells"]
    assert got[2][0, :n].tolist() == case["mass"]
    want = O.find_seeds(case["map"][None], case["q"], case["p"], [case["min_mass"]], case["K"],
                        np.zeros((1, 2)), 1)
    check_seeds(got, want)
    # in pixels: 4 cells per pixel in a box whose corner is (-2, 3)
    got = run_seeds(case["map"][None], [case["min_mass"]], case["q"], case["p"], case["K"],
                    (-2.0, 3.0, -2.0 + Gh / 4.0, 3.0 + Gw / 4.0), 4)
    check_seeds(got, O.find_seeds(case["map"][None], case["q"], case["p"], [case["min_mass"]],
                                  case["K"], np.array([[-2.0, 3.0]]), 4))


@pytest.mark.parametrize("q,p,K", [(1, 2, 10), (2, 4, 10), (0, 0, 5), (8, 16, 3)])
def test_peaks_of_sampled_maps(mapcase, boxcase, q, p, K):
    _, want_map = mapcase
    min_mass = np.array([12.85, 12.85, 12.85], np.float32)  # 0.05 x 257
    lo = np.tile(np.asarray(BOX[:2]), (3, 1))
    want = O.find_seeds(want_map["count"], q, p, min_mass, K, lo, C)
    if (q, p) == (1, 2):
        assert (want[0] >= 3).all()  # at least the three stars of every tile
    if p == 0:
        assert (want[0] == K).all()  # more peaks than K
    check_seeds(run_seeds(want_map["count"], min_mass, q, p, K, BOX, C), want)
    _, tb, want_map = boxcase
    want = O.find_seeds(want_map["count"], q, p, min_mass, K, tb[:, :2].astype(np.float64), C)
    check_seeds(run_seeds(want_map["count"], min_mass, q, p, K, BOX, C, tile_boxes=tb), want)


def test_peaks_largest_grid():
    """128 x 256 = 32768 cells: the limit, 128 KiB of smoothed map in LDS."""
    rng = np.random.default_rng(9)
    m = np.zeros((2, 128, 256), np.float32)
    idx = rng.integers(0, 128 * 256, (2, 400))
    for t in range(2):
        np.add.at(m[t].reshape(-1), idx[t], rng.integers(1, 6, 400).astype(np.float32))
    m[0, 127, 255] = 50.0  # the last cell: (126, 254) is the first whose window sees it
    want = O.find_seeds(m, 1, 2, [4.0, 4.0], 64, np.zeros((2, 2)), 8)
    assert want[1][0, 0] == 126 * 256 + 254 and (want[0] > 20).all()
    check_seeds(run_seeds(m, [4.0, 4.0], 1, 2, 64, (0.0, 0.0, 16.0, 32.0), 8), want)


# ---- moments ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def momcase(mapcase):
    """The map test's catalogs, the oracle's seeds, and match_of_seed from
    match_catalogs on the device."""
    case, want_map = mapcase
    counts, locs, fluxes = case
    lo = np.tile(np.asarray(BOX[:2]), (3, 1))
    K = 10
    n_seeds, _, _, slocs = O.find_seeds(want_map["count"], 1, 2, np.full(3, 12.85, np.float32), K,
                                        lo, C)
    slocs = slocs.astype(np.float32)
    d = cuda(n_seeds, slocs, np.ones((3, K), np.float32), counts, locs, fluxes)
    out = metrics.match_catalogs(*d, None, 0.75, O.F32_MAX, torch.zeros(1), return_matches=True)
    match = out[4]
    assert match.dtype == torch.int32 and tuple(match.shape) == (3, 257, K)
    # where no rounding can flip it, the association is the oracle's
    want_match, ok = O.associate(n_seeds, slocs, counts, locs, fluxes, 0.75)
    assert ok.mean() > 0.95
    np.testing.assert_array_equal(match.cpu().numpy()[ok], want_match[ok])
    assert (want_match >= 0).sum() > 257
    return case, slocs, match


@pytest.mark.parametrize("weighted", [False, True])
def test_moments(momcase, weighted):
    (counts, locs, fluxes), slocs, match = momcase
    N = locs.shape[1]
    w = weights_of(3, N) if weighted else None
    dl, df, ds, dw = cuda(locs, fluxes, slocs, w)
    mom, mflux = condense.seed_moments(match, dl, df, ds, weights=dw)
    assert mom.dtype == torch.float64 and tuple(mom.shape) == (3, 10, 10)
    want, ab, want_flux = O.moments(match.cpu().numpy(), locs, fluxes, slocs, w)
    got = mom.cpu().numpy()
    if not weighted:
        np.testing.assert_array_equal(got[..., 0], want[..., 0])
        assert want[..., 0].max() > 100
    err, bound = np.abs(got - want), N * 2.0 ** -50 * ab
    print("moments: max err / bound per column",
          (err / np.maximum(bound, 1e-300)).max((0, 1)).round(4).tolist())
    assert (err <= bound).all()
    np.testing.assert_array_equal(mflux.cpu().numpy(), want_flux)  # NaNs included
    assert np.isnan(want_flux).any() and np.isfinite(want_flux).any()
    mom2, mflux2 = condense.seed_moments(match, dl, df, ds, weights=dw)
    assert torch.equal(mom, mom2)  # bit-identical: no atomics, a fixed order
    assert torch.equal(mflux.nan_to_num(-1.0), mflux2.nan_to_num(-1.0))
    mom3, none = condense.seed_moments(match, dl, df, ds, weights=dw, with_matched_flux=False)
    assert none is None and torch.equal(mom, mom3)


def test_moments_full_width():
    """K = S = 64 (4 lanes per seed) and K = 1 (256 lanes on one seed)."""
    rng = np.random.default_rng(3)
    for K, S, N in ((64, 64, 37), (1, 2, 300), (7, 3, 65)):
        locs = rng.uniform(0, 8, (2, N, S, 2)).astype(np.float32)
        fluxes = rng.uniform(0.5, 50, (2, N, S)).astype(np.float32)
        slocs = rng.uniform(0, 8, (2, K, 2)).astype(np.float32)
        match = rng.integers(-1, S, (2, N, K)).astype(np.int32)
        mom, mflux = condense.seed_moments(*cuda(match, locs, fluxes, slocs))
        want, ab, want_flux = O.moments(match, locs, fluxes, slocs)
        np.testing.assert_array_equal(mom.cpu().numpy()[..., 0], want[..., 0])
        assert (np.abs(mom.cpu().numpy() - want) <= N * 2.0 ** -50 * ab).all()
        np.testing.assert_array_equal(mflux.cpu().numpy(), want_flux)


# ---- end to end ------------------------------------------------------------------
PBOX = (-2.0, -2.0, 10.0, 10.0)
FIELDS = ("seed_locs", "seed_mass", "prob", "locs", "locs_sd", "locs_cov_hw", "fluxes",
          "fluxes_sd", "mags", "mags_sd", "expected_count", "unassociated")


@pytest.fixture(scope="module")
def planted():
    counts, locs, fluxes, star_locs, star_flux, presence = O.planted_posterior(seed=0)
    want = O.condense(counts, locs, fluxes, PBOX)
    got = condense.condense(*cuda(counts, locs, fluxes), box=PBOX)
    return dict(N=counts.shape[1], star_locs=star_locs, presence=presence, want=want, got=got)


def test_condense_planted_posterior(planted):
    got, want, N = planted["got"], planted["want"], planted["N"]
    assert want["margins_ok"].all()
    assert got.n_seeds.tolist() == [3, 3, 3, 3]
    np.testing.assert_array_equal(got.n_seeds.cpu().numpy(), want["n_seeds"])
    prob = got.prob.cpu().numpy()
    assert prob.dtype == np.float32 and prob.shape == (4, 12)
    d = np.linalg.norm(want["seed_locs"][:, None, :3].astype(np.float64)
                       - planted["star_locs"][:, :, None], axis=-1)
    k = d.argmin(-1)  # the seed of each star
    np.testing.assert_array_equal(prob[np.arange(4)[:, None], k].astype(np.float64) * N,
                                  planted["presence"])
    for name in FIELDS:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == np.float32, name
        np.testing.assert_allclose(g, want[name], rtol=1e-5, atol=1e-6, equal_nan=True,
                                   err_msg=name)
    np.testing.assert_array_equal(got.flux_quantiles.cpu().numpy(), want["flux_quantiles"])
    assert got.quantiles == (0.05, 0.5, 0.95)
    np.testing.assert_array_equal(got.moments.cpu().numpy()[..., 0], want["moments"][..., 0])
    assert (prob[:, 3:] == 0).all() and np.isnan(got.locs.cpu().numpy()[:, 3:]).all()


def test_as_catalog_keeps_the_probable_stars(planted):
    got = planted["got"]
    counts, locs, fluxes = got.as_catalog(0.5)
    assert tuple(counts.shape) == (4, 1) and tuple(locs.shape) == (4, 1, 12, 2)
    assert tuple(fluxes.shape) == (4, 1, 12) and counts.dtype == torch.int32
    assert counts[:, 0].tolist() == [2, 2, 2, 2]  # planted 1.0 and 0.8, not 0.3
    kept = locs[:, 0, :2].cpu().numpy().astype(np.float64)
    d = np.linalg.norm(kept[:, :, None] - planted["star_locs"][:, None, :2], axis=-1)
    assert (d.min(-1) < 0.05).all() and (np.sort(d.argmin(-1), -1) == [0, 1]).all()
    assert torch.isnan(locs[:, 0, 2:]).all() and torch.isnan(fluxes[:, 0, 2:]).all()
    # it goes straight into match_catalogs as an N = 1 population: both kept
    # detections match the two probable stars
    tl, tf = cuda(planted["star_locs"][:, :2].astype(np.float32), np.ones((4, 2), np.float32))
    out = metrics.match_catalogs(torch.full((4,), 2, device="cuda"), tl, tf, counts, locs,
                                 torch.ones_like(fluxes), None, 0.5, 0.5, torch.tensor([30.0]))
    assert out[1].sum().item() == 8 and out[3].sum().item() == 8
    assert got.as_catalog(0.0)[0][:, 0].tolist() == [12] * 4
    assert got.as_catalog(0.25)[0][:, 0].tolist() == [3] * 4


def test_to_image_offsets(planted):
    got = planted["got"]
    img = got.to_image(2, 8, 0.5)
    assert img["tile"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    keep = got.prob >= 0.5
    local = got.locs[keep].cpu().numpy()
    off = np.array([[0, 0], [0, 0], [0, 8], [0, 8], [8, 0], [8, 0], [8, 8], [8, 8]], np.float32)
    np.testing.assert_array_equal(img["locs"].cpu().numpy(), local + off)
    np.testing.assert_array_equal(img["prob"].cpu().numpy(), got.prob[keep].cpu().numpy())
    for name in ("locs_sd", "fluxes", "fluxes_sd", "mags", "mags_sd"):
        assert img[name].shape[0] == 8 and torch.isfinite(img[name]).all()
    assert got.to_image((1, 4), 8, 0.5)["locs"][2:4, 1].min() > 6.0  # tile 1 at column 8
    with pytest.raises(ValueError, match="tiles"):
        got.to_image(3, 8)


def test_condense_weighted_matches_oracle():
    counts, locs, fluxes, *_ = O.planted_posterior(seed=1, T=2, N=128)
    w = weights_of(2, 128)
    want = O.condense(counts, locs, fluxes, PBOX, weights=w, quantiles=(0.1, 0.9))
    assert want["margins_ok"].all()
    got = condense.condense(*cuda(counts, locs, fluxes), box=PBOX, weights=cuda(w)[0],
                            quantiles=(0.1, 0.9))
    np.testing.assert_array_equal(got.n_seeds.cpu().numpy(), want["n_seeds"])
    for name in FIELDS:
        # the weighted map's last bits vary: the seeds may move by that much
        tol = dict(rtol=1e-5, atol=1e-5) if name != "seed_mass" else dict(rtol=1e-5, atol=0)
        np.testing.assert_allclose(getattr(got, name).cpu().numpy(), want[name], equal_nan=True,
                                   err_msg=name, **tol)
    np.testing.assert_array_equal(got.flux_quantiles.cpu().numpy(), want["flux_quantiles"])


def test_condense_sampler_on_a_real_run():
    from smcdet_amd.sampler import SMCsampler
    from tests._params import M71, p_m71_mh, p_m71_model, p_m71_prior
    torch.manual_seed(0)
    H, S, N = 8, 4, 256
    model, prior = p_m71_model(H), p_m71_prior(H, S, S)
    # a synthetic truth image from the prior (a few sources on the padded tile)
    truth = p_m71_prior(H, 0, 100, counts_rate=0.01)
    c, l, f = truth.sample(num_catalogs=1, device=torch.device("cuda", 0))
    img = model.sample(l, f)[0, 0, :, :, 0]
    s = SMCsampler(img, H, prior, model, p_m71_mh(20), N, 0.5, "systematic",
                   M71["flux_detection_threshold"], 100, print_every=10 ** 9)
    with pytest.raises(RuntimeError, match="run the sampler"):
        condense.condense_sampler(s)
    s.run()
    for pruned in (True, False):
        cat = condense.condense_sampler(s, pruned=pruned)
        K = min(64, 2 * S)
        assert tuple(cat.prob.shape) == (1, K) and tuple(cat.locs.shape) == (1, K, 2)
        assert tuple(cat.flux_quantiles.shape) == (1, K, 3) and tuple(cat.n_seeds.shape) == (1,)
        n = int(cat.n_seeds[0])
        assert 0 <= n <= K and ((cat.prob >= 0) & (cat.prob <= 1)).all()
        assert (cat.prob[0, :n] > 0).all() and (cat.prob[0, n:] == 0).all()
        assert torch.isfinite(cat.locs[0, :n]).all() and torch.isnan(cat.locs[0, n:]).all()
        lo, hi = (0.0, float(H)) if pruned else (-4.0, H + 4.0)
        assert ((cat.locs[0, :n] >= lo) & (cat.locs[0, :n] <= hi)).all()
        assert float(cat.expected_count[0]) == pytest.approx(float(cat.prob.sum()), rel=1e-6)
        assert float(cat.unassociated[0]) >= 0
