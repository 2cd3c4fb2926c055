"""smcdet_psf_find and smcdet_psf_recentre on the device against the float64
oracle (tests/_psffind_oracle.py), within the first-order bounds of DESIGN.md
§19.5: |snr_gpu - snr| <= eps_c at E = 32 * 2^-24 per profile value, the
parabola's bound from its three values' bounds, exact agreement of everything
discrete with the oracle's rule applied to the device's own map.  Every check
prints its largest observed ratio to its bound (1.0 is the bound).

Shapes (the smallest at which each path can break): 8x8 M71 R = 8 at 2 cells
(one pixel per lane), 5x7 at 3 cells (odd, ragged, every window clipped; 1/3 is
not a float32), 12x20 R = 2 at 1 cell (windows smaller than the tile), 8x8 R =
0, 32x32 at 4 cells (both limits, the LDS maximum), 8x8 under the Poisson
ImageModel.

End-to-end tolerances (measured on the CPU): over the
separated set the oracle with a float32-emulated profile and the float64
oracle agree in their counts on 40 of 40 tiles and differ by at most 1.32e-6 px
in a position and 3.41e-5 flux errors in a flux; the device may differ from the
float64 oracle by ten times that."""
import functools

import numpy as np
import pytest
import torch

import _psffind_oracle as F
from _params import M71, p_basic_model
from smcdet_amd import _hip, photometry, psffind
from smcdet_amd.images import M71ImageModel
from smcdet_amd.metrics import compute_precision_recall_f1, match_catalogs

pytestmark = pytest.mark.gpu
NAN = float("nan")
F32 = np.float32
POS_TOL = 10 * 1.32e-6  # px: ten times the float32 / float64 oracles' largest difference
Z_TOL = 10 * 3.41e-5   # flux errors, likewise


def m71_model(H, W, R=M71["psf_radius"]):
    p = M71
    return M71ImageModel(image_height=H, image_width=W, background=p["background"], psf_radius=R,
                         adu_per_nmgy=p["adu_per_nmgy"], psf_params=p["psf_params"],
                         noise_additive=p["noise_additive"],
                         noise_multiplicative=p["noise_multiplicative"])


def m71_zero_radius():
    """M71 with R = 0: the model's own normalising constant is a sum over a
    (32 R)^2 grid, 0 at R = 0 (an infinite profile), so the R = 8 constant is
    set: one-pixel windows of the usual profile."""
    model = m71_model(8, 8, 0)
    model.psf_normalizing_constant = m71_model(8, 8).psf_normalizing_constant
    return model


#        name: (model, cells, K, T, G, per-image background, (half, step))
SHAPES = {
    "8x8": (lambda: m71_model(8, 8), 2, 16, 4, 3, True, (2, 0.25)),
    "5x7": (lambda: m71_model(5, 7), 3, 4, 3, 3, False, (3, 0.2)),
    "12x20": (lambda: m71_model(12, 20, 2), 1, 32, 3, 3, False, (1, 0.3)),
    "r0": (m71_zero_radius, 2, 4, 2, 3, False, (2, 0.25)),
    "32x32": (lambda: m71_model(32, 32), 4, 16, 1, 2, False, (2, 0.25)),
    "poisson": (lambda: p_basic_model(8), 2, 4, 3, 3, False, (2, 0.25)),
}


class Case:
    pass


@functools.lru_cache(None)
def case(name):
    """T images with 1..3 stars and G lists each: g = 0 the true sources,
    displaced by up to 0.3 px with fluxes off by up to 20 %; g = 1 one true
    source, a slot with a NaN flux and a slot with a NaN location below the
    count; g = 2 an empty list.  Every slot past a count holds a finite decoy
    the count must keep out."""
    make, cells, K, T, G, per_image_bg, move = SHAPES[name]
    c = Case()
    c.name, c.model, c.cells, c.K, c.T, c.G, c.move = name, make(), cells, K, T, G, move
    c.m = m = F.model_of(c.model)
    rng = np.random.default_rng(sum(map(ord, name)))
    scale = 1.0 if m.kind == "m71" else 20.0  # the Poisson model's fluxes are counts
    c.background = (m.background * (1 + 0.1 * np.arange(T))).astype(F32) if per_image_bg else None
    c.images = np.empty((T, m.H, m.W), F32)
    c.counts = np.zeros((T, G), np.int32)
    c.locs = np.full((T, G, K, 2), 2.25, F32)
    c.fluxes = np.full((T, G, K), 40.0 * scale, F32)
    c.truth = []
    for t in range(T):
        n = 1 + t % 3
        ll = np.stack([rng.uniform(0.3, m.H - 0.3, n), rng.uniform(0.3, m.W - 0.3, n)], 1)
        if t == 1:
            ll[0, 0] = -0.4  # in the padding: its window is clipped above
        ff = scale * np.exp(rng.uniform(np.log(40.0), np.log(200.0), n))
        B = None if c.background is None else float(c.background[t])
        c.images[t] = F.noisy(m, F.render(m, ll.astype(F32), ff, B), rng)
        c.truth.append((ll, ff))
        c.counts[t, 0] = n
        c.locs[t, 0, :n] = ll + rng.uniform(-0.3, 0.3, (n, 2))
        c.fluxes[t, 0, :n] = ff * rng.uniform(0.8, 1.2, n)
        if G > 1:
            c.counts[t, 1] = 3
            c.locs[t, 1, :3] = [ll[0], (1.5, 1.5), (NAN, 2.0)]
            c.fluxes[t, 1, :3] = [ff[0], NAN, 30.0 * scale]
    return c


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ratio(diff, tol):
    """max |diff| / tol over the finite entries (0 / 0 counts as 0)."""
    diff, tol = np.abs(np.asarray(diff, np.float64)), np.asarray(tol, np.float64)
    ok = np.isfinite(diff) & np.isfinite(tol)
    if not ok.any():
        return 0.0
    d, t = diff[ok], tol[ok]
    return float(np.max(np.where(d == 0, 0.0, d / np.where(t > 0, t, np.finfo(float).tiny))))


# ---- the device calls (all through smcdet_amd.psffind) -------------------------------------
def run_map(c, with_list, images=None):
    images = cuda(c.images if images is None else images)
    if not with_list:
        return psffind.significance_map(images, c.model, background=cuda(c.background),
                                        cells=c.cells).cpu().numpy()
    return psffind.significance_map(images, c.model, cuda(c.counts), cuda(c.locs), cuda(c.fluxes),
                                    background=cuda(c.background), cells=c.cells).cpu().numpy()


def run_find(c, thresh, nms, min_sep, sel=slice(None)):
    """(counts_out, locs_out, snr_out, flux_hat, n_found, map) as numpy."""
    out = psffind._find_launch(
        cuda(c.images[sel]), c.model._cmodel(),
        cuda(None if c.background is None else c.background[sel]), cuda(c.counts[sel]),
        cuda(c.locs[sel]), cuda(c.fluxes[sel]), c.G, c.K, c.cells,
        cuda(np.asarray(thresh, F32)), cuda(np.asarray(nms, np.int32)), min_sep, True)
    return [x.cpu().numpy() for x in out]


def run_recentre(c, sel=slice(None)):
    half, step = c.move
    out = psffind._recentre_launch(
        cuda(c.images[sel]), c.model._cmodel(),
        cuda(None if c.background is None else c.background[sel]), cuda(c.counts[sel]),
        cuda(c.locs[sel]), cuda(c.fluxes[sel]), half, step)
    return [x.cpu().numpy() for x in out]


def run_find_pipeline(model, images, thresh):
    f = psffind.find(cuda(images), model, thresh)
    return {k: v.cpu().numpy() for k, v in f._asdict().items()}


def bg_of(c, t):
    return None if c.background is None else c.background[t]


@functools.lru_cache(None)
def oracle(name, t, g):
    """(snr, eps, Stats, Residual) of problem (t, g) of a case; g = None: no list."""
    c = case(name)
    if g is None:
        return F.significance_map(c.m, c.images[t], background=bg_of(c, t), cells=c.cells)
    return F.significance_map(c.m, c.images[t], c.counts[t, g], c.locs[t, g], c.fluxes[t, g],
                              bg_of(c, t), c.cells)


# ---- the map ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_map(name):
    c = case(name)
    m = c.m
    got = run_map(c, True)
    bare = run_map(c, False)
    assert got.shape == (c.T, c.G, c.cells * m.H, c.cells * m.W) and got.dtype == F32
    assert bare.shape == (c.T, c.cells * m.H, c.cells * m.W)
    worst = worst_bare = 0.0
    for t in range(c.T):
        snr, eps, _, _ = oracle(name, t, None)
        worst_bare = max(worst_bare, ratio(bare[t] - snr, eps))
        for g in range(c.G):
            snr, eps, _, res = oracle(name, t, g)
            assert np.all(np.isfinite(snr)) and np.all(eps > 0)
            worst = max(worst, ratio(got[t, g] - snr, eps))
            if g == 1:  # the NaN-flux and NaN-location slots and the decoys are not subtracted
                assert list(res.counted) == [0]
        # an empty list is no list
        np.testing.assert_array_equal(got[t, c.G - 1] if c.G == 3 else bare[t], bare[t])
    print(f"map {name}: with a list {worst:.3g}, without {worst_bare:.3g} of the bound")
    assert worst <= 1.0 and worst_bare <= 1.0


def test_flux_hat_equals_the_one_iteration_solve_as_float32():
    """f-hat at a peak's cell centre against forced_photometry(n_iter = 1) of a
    single source there, both on the device: the same float32 profile and the
    same float64 terms in another order, which differ by at most 2 (H W + 8)
    2^-53 of the terms' absolute sums (the oracle's).  flux_hat is a float32
    output, so what can be checked is that bound plus half a float32 ulp of
    the rounding, which is about a million times larger: the two are equal
    after rounding to float32, not shown to agree in float64."""
    c = case("8x8")
    m = c.m
    rng = np.random.default_rng(8)
    images = np.stack([F.noisy(m, F.render(m, [rng.uniform(1, 7, 2)], [rng.uniform(40, 200)]), rng)
                       for _ in range(8)])
    d = Case()
    d.__dict__.update(c.__dict__)
    d.images, d.background, d.T, d.G = images, None, 8, 1
    d.counts, d.locs = np.zeros((8, 1), np.int32), c.locs[:1, :1].repeat(8, 0)
    d.fluxes = c.fluxes[:1, :1].repeat(8, 0)
    cnt, locs, snr, fhat, _, smap = run_find(d, [5.0], [16], 0.5)
    assert np.all(cnt == 1)
    worst = 0.0
    for t in range(8):
        x = int(np.argmax(smap[t, 0]))
        assert snr[t, 0, 0] == smap[t, 0].reshape(-1)[x]
        ctr = F.cell_centres(m, 2)[0][x].astype(F32)
        ph = photometry.forced_photometry(cuda(images[t]), cuda(np.ones(1, np.int32)),
                                          cuda(ctr[None, None]), c.model, n_iter=1)
        want = float(ph.fluxes[0, 0])
        st = F.significance_map(m, images[t], cells=2)[2]
        tol = 2 * (m.H * m.W + 8) * 2.0 ** -53 * (st.a_abs[x] + abs(st.a[x])) / (m.g * st.d[x])
        worst = max(worst, abs(float(fhat[t, 0, 0]) - want)
                    / (tol + 0.5 * float(np.spacing(F32(abs(want))))))
    print(f"flux_hat against the one-iteration solve, as float32: {worst:.3g} of the bound")
    assert worst <= 1.0


# ---- the peaks -------------------------------------------------------------------------------
THRESH, NMS, MIN_SEP = [2.0, 5.0, 1e9], [0, 3, 1], 1.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_peaks(name):
    """r0 is where the order's equality branch decides: with R = 0 the c x c
    cells of a pixel form the same float32 profile (dh, dw = +-1/4, r2 = 1/8 at
    c = 2), so the device's map is made of blocks of equal values and the lower
    flat index wins every suppression and every place in the order."""
    c = case(name)
    m = c.m
    th, nms = THRESH[:c.G], NMS[:c.G]
    if name == "r0":  # the empty lists at a threshold the stars' pixels pass: their blocks tie
        th = [2.0, 5.0, 5.0]
    cnt, locs, snr, fhat, n_found, smap = run_find(c, th, nms, MIN_SEP)
    capped = excluded = ties = 0
    worst_f = worst_l = 0.0
    for t in range(c.T):
        for g in range(c.G):
            n = int(min(max(c.counts[t, g], 0), c.K))
            _, _, st, res = oracle(name, t, g)
            src = c.locs[t, g][res.counted]
            nf, cells, want, _ = F.select_peaks(smap[t, g], c.cells, th[g], nms[g], MIN_SEP, src,
                                                c.K - n)
            assert n_found[t, g] == nf and cnt[t, g] == n + len(cells), (t, g)
            capped += nf > len(cells)
            excluded += F.select_peaks(smap[t, g], c.cells, th[g], nms[g], 0.0, src, 0)[0] > nf
            new = slice(n, n + len(cells))
            for x in cells:  # selected cells that won against an equal value
                i, j = divmod(x, smap.shape[-1])
                q = max(int(nms[g]), 1)
                win = smap[t, g, max(i - q, 0):i + q + 1, max(j - q, 0):j + q + 1]
                ties += int((win == smap[t, g, i, j]).sum()) > 1
            # the cells and their order: the map's values there, exactly
            np.testing.assert_array_equal(snr[t, g, new], smap[t, g].reshape(-1)[cells])
            assert np.all(np.abs(locs[t, g, new] - want) <= np.spacing(np.abs(want))), (t, g)
            worst_l = max(worst_l, ratio(locs[t, g, new] - want, np.spacing(np.abs(want))))
            # given slots bit for bit, NaN past the count and in the given slots' snr and f-hat
            assert locs[t, g, :n].tobytes() == c.locs[t, g, :n].tobytes()
            assert np.isnan(locs[t, g, n + len(cells):]).all()
            assert np.isnan(snr[t, g, :n]).all() and np.isnan(snr[t, g, n + len(cells):]).all()
            assert np.isnan(fhat[t, g, :n]).all() and np.isnan(fhat[t, g, n + len(cells):]).all()
            worst_f = max(worst_f, ratio(fhat[t, g, new] - st.fhat[cells], st.feps[cells]))
            if th[g] == 1e9:
                assert nf == 0 and cnt[t, g] == n
    print(f"peaks {name}: {capped} problems capped, {excluded} with an exclusion, {ties} "
          f"selected cells with an equal neighbour; locs {worst_l:.3g} ulp, flux_hat "
          f"{worst_f:.3g} of the bound")
    assert worst_f <= 1.0
    if name in ("8x8", "5x7"):
        assert capped > 0 and excluded > 0
    if name == "r0":
        assert ties >= c.T and np.all(smap[:, :, 0::2, 0::2] == smap[:, :, 1::2, 1::2])


def test_peaks_same_bits_again_and_among_other_neighbours():
    c = case("8x8")
    a = run_find(c, THRESH, NMS, MIN_SEP)
    b = run_find(c, THRESH, NMS, MIN_SEP)
    one = run_find(c, THRESH, NMS, MIN_SEP, slice(2, 3))
    for x, y, z in zip(a, b, one):
        assert x.tobytes() == y.tobytes()
        assert x[2:3].tobytes() == z.tobytes()
    la, lb, lone = run_recentre(c), run_recentre(c), run_recentre(c, slice(2, 3))
    for x, y, z in zip(la, lb, lone):
        assert x.tobytes() == y.tobytes()
        assert x[2:3].tobytes() == z.tobytes()


# ---- recentring --------------------------------------------------------------------------------
def test_recentre():
    """Per counted source: the chosen candidate's snr within its bound and the
    new location within twice the parabola's first-order bound (plus the final
    rounding), wherever the oracle's best candidate leads every other by more
    than twice their bounds and the parabola's curvature is clear of its
    bound; that holds for all but at most 1 in 10 of the sources.  R = 0 is
    left to the layout checks: all candidates inside a pixel tie to rounding."""
    sources = decided = 0
    worst_s = worst_l = 0.0
    for name in SHAPES:
        c = case(name)
        half, step = c.move
        locs, snr = run_recentre(c)
        assert locs.shape == c.locs.shape and snr.shape == c.fluxes.shape
        for t in range(c.T):
            for g in range(c.G):
                o = F.recentre_one(c.m, c.images[t], c.counts[t, g], c.locs[t, g], c.fluxes[t, g],
                                   half, step, bg_of(c, t))
                for k in range(c.K):
                    if k not in o["cand"]:  # unchanged, bit for bit
                        assert locs[t, g, k].tobytes() == c.locs[t, g, k].tobytes()
                        assert np.isnan(snr[t, g, k])
                        continue
                    s, eps, best, tol = o["cand"][k]
                    if not np.isfinite(eps).any():  # every candidate's window misses the image
                        assert snr[t, g, k] == -np.inf and name == "r0"
                        continue
                    assert abs(snr[t, g, k] - s.max()) <= eps[np.isfinite(eps)].max()
                    if name == "r0":
                        continue
                    sources += 1
                    others = np.arange(len(s)) != best
                    lead = np.all(s[best] - s[others] > 2 * (eps[best] + eps[others]))
                    if not (lead and np.all(np.isfinite(tol))):
                        continue
                    decided += 1
                    want = o["locs_out"][k]
                    worst_s = max(worst_s, ratio(snr[t, g, k] - s[best], eps[best]))
                    worst_l = max(worst_l, ratio(locs[t, g, k] - want,
                                                 2 * tol + np.spacing(np.abs(want))))
    print(f"recentre: {decided} of {sources} sources decided; snr {worst_s:.3g}, locs "
          f"{worst_l:.3g} of the bound")
    assert sources >= 20 and 10 * (sources - decided) <= sources
    assert worst_s <= 1.0 and worst_l <= 1.0


# ---- end to end ----------------------------------------------------------------------------------
def test_find_on_the_separated_set():
    model = m71_model(8, 8)
    m = F.model_of(model)
    tiles = F.separated_set(m)
    got = run_find_pipeline(model, np.stack([x for x, _, _ in tiles]), 5.0)
    assert got["locs"].shape == (40, 16, 2) and got["fluxes"].dtype == F32
    agree = 0
    worst_p = worst_z = 0.0
    for t, (x, _, _) in enumerate(tiles):
        want = F.find(m, x, 5.0)
        if got["counts"][t] != want.count:
            continue
        agree += 1
        n = want.count
        pairs, free = F.match(want.locs[:n], got["locs"][t, :n], 0.5)
        assert len(pairs) == n and not free
        for i, j in pairs:
            worst_p = max(worst_p, np.abs(got["locs"][t, j] - want.locs[i]).max())
            worst_z = max(worst_z, abs(float(got["fluxes"][t, j]) - float(want.fluxes[i]))
                          / want.flux_err[i])
        assert got["status"][t] == want.status
        assert np.isnan(got["locs"][t, n:]).all() and np.all(got["fluxes"][t, n:] == 0)
    print(f"find, separated set: counts agree on {agree} of 40 tiles; positions "
          f"{worst_p / POS_TOL:.3g}, fluxes {worst_z / Z_TOL:.3g} of the tolerance")
    assert agree >= 36
    assert worst_p <= POS_TOL and worst_z <= Z_TOL


def test_tune_is_find_grid_then_match():
    model = m71_model(8, 8)
    m = F.model_of(model)
    tiles = F.separated_set(m)
    images = cuda(np.stack([x for x, _, _ in tiles]))
    tc = cuda(np.array([len(ll) for _, ll, _ in tiles], np.int32))
    tl = np.full((40, 3, 2), NAN, F32)
    tf = np.zeros((40, 3), F32)
    for t, (_, ll, ff) in enumerate(tiles):
        tl[t, :len(ll)], tf[t, :len(ll)] = ll, ff
    tl, tf = cuda(tl), cuda(tf)
    tuned = psffind.tune(images, model, tc, tl, tf, [4.0, 6.0, 40.0], [0, 1], mag_bins=(14.0, 22.0),
                         max_bytes=1 << 16)
    g = psffind.find_grid(images, model, [4.0, 6.0, 40.0], [0, 1])
    assert g.settings.shape == (6, 3) and g.counts.shape == (40, 6)
    tables = match_catalogs(tc, tl, tf, g.counts, g.locs, g.fluxes, None, 0.5, 0.5,
                            torch.tensor([14.0, 22.0]))
    f1 = compute_precision_recall_f1(*tables)[2][:, -1]
    assert tuned.f1.cpu().numpy().tobytes() == f1.cpu().numpy().tobytes()
    assert torch.equal(tuned.settings, g.settings)
    assert tuned.best_index == int((f1 == f1.max()).nonzero()[0]) and tuned.best["nms_radius"] in (0, 1)
    print("tune: F1 per setting", np.round(tuned.f1.cpu().numpy(), 3).tolist())
    assert float(tuned.f1.max()) > 0.9


def test_residual_significance_is_the_map_of_the_kept_detections():
    from smcdet_amd.condense import CondensedCatalog
    c = case("8x8")
    T, K = c.T, 5
    dev = dict(device="cuda")
    prob = torch.tensor([[0.9, 0.2, 0.8, 0.0, 0.0]] * T, **dev)
    locs = torch.full((T, K, 2), NAN, **dev)
    fluxes = torch.full((T, K), NAN, **dev)
    first = torch.tensor(np.array([ll[0] for ll, _ in c.truth], F32), **dev)
    locs[:, 0], fluxes[:, 0] = first, 60.0                       # kept: the first true star
    locs[:, 1], fluxes[:, 1] = first + 2.0, 500.0                # below min_prob: not subtracted
    locs[:, 2, 0], locs[:, 2, 1], fluxes[:, 2] = 6.5, 1.5, 30.0  # kept
    z0 = torch.zeros(T, K, **dev)
    cat = CondensedCatalog(
        n_seeds=torch.full((T,), 3, dtype=torch.int32, **dev), seed_locs=locs, seed_mass=z0,
        prob=prob, locs=locs, locs_sd=torch.zeros(T, K, 2, **dev), locs_cov_hw=z0, fluxes=fluxes,
        fluxes_sd=z0, mags=z0, mags_sd=z0, flux_quantiles=torch.zeros(T, K, 1, **dev),
        quantiles=(0.5,), expected_count=prob.sum(-1), unassociated=torch.zeros(T, **dev),
        moments=torch.zeros(T, K, 10, dtype=torch.float64, **dev))
    model = m71_model(8, 8)  # (the model's own background: residual_significance takes no other)
    img = cuda(c.images)
    got = psffind.residual_significance(cat, img, model, min_prob=0.5, cells=2)
    counts, cl, cf = cat.as_catalog(0.5)
    assert counts[:, 0].tolist() == [2] * T
    direct = psffind.significance_map(img, model, counts[:, 0], cl[:, 0].contiguous(),
                                      cf[:, 0].contiguous(), cells=2)
    assert got.shape == (T, 16, 16) and got.dtype == torch.float32
    assert got.cpu().numpy().tobytes() == direct.cpu().numpy().tobytes()
    # and against the oracle, with the two kept detections subtracted
    worst = 0.0
    for t in range(T):
        snr, eps, _, res = F.significance_map(c.m, c.images[t], 2, cl[t, 0].cpu().numpy(),
                                              cf[t, 0].cpu().numpy(), cells=2)
        assert len(res.counted) == 2
        worst = max(worst, ratio(got[t].cpu().numpy() - snr, eps))
    print(f"residual_significance: {worst:.3g} of the bound")
    assert worst <= 1.0
    assert not torch.equal(got, psffind.significance_map(img, model))


def test_refusals_launch_nothing():
    """Every limit of the two entry points, with device buffers: the code comes
    back and the outputs keep their fill."""
    c = case("r0")
    L = _hip.lib()
    img, cnt, locs, fl = cuda(c.images), cuda(c.counts), cuda(c.locs), cuda(c.fluxes)
    th, nms = cuda(np.asarray(THRESH, F32)), cuda(np.asarray(NMS, np.int32))
    outs = [torch.full((c.T, c.G), -7, dtype=torch.int32).cuda(),
            torch.full((c.T, c.G, c.K, 2), -7.0).cuda(), torch.full((c.T, c.G, c.K), -7.0).cuda(),
            torch.full((c.T, c.G, c.K), -7.0).cuda(),
            torch.full((c.T, c.G), -7, dtype=torch.int32).cuda()]
    p = _hip.ptr

    def find(cm, T=c.T, G=c.G, K=c.K, cells=2, min_sep=0.5):
        return L.smcdet_psf_find(_hip.ref(cm), p(img), None, p(cnt), p(locs), p(fl), T, G, K,
                                 cells, p(th), p(nms), min_sep, *(p(o) for o in outs), None, None)

    def move(cm, K=c.K, half=2, step=0.25):
        return L.smcdet_psf_recentre(_hip.ref(cm), p(img), None, p(cnt), p(locs), p(fl), c.T, c.G,
                                     K, half, step, p(outs[1]), p(outs[2]), None)

    def model(**kw):
        cm = type(c.model._cmodel()).from_buffer_copy(c.model._cmodel())
        for k, v in kw.items():
            setattr(cm, k, v)
        return cm

    assert find(model(H=33, W=32)) == -2 and find(model(psf_radius=65)) == -2
    assert find(model(), K=33) == -2 and find(model(), T=65536, G=32768) == -2
    assert find(model(), cells=0) == -1 and find(model(), cells=5) == -1
    assert find(model(), T=0) == -1 and find(model(), min_sep=-1.0) == -1
    assert move(model(H=1, W=1025)) == -2 and move(model(), K=33) == -2
    assert move(model(), half=0) == -1 and move(model(), half=4) == -1
    assert move(model(), step=0.0) == -1
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all())
