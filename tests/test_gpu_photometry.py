"""smcdet_forced_photometry on the device against the float64 oracle
(tests/_photometry_oracle.py), within the bounds of DESIGN.md §18.5:

    |flux_gpu - flux_oracle|_k <= E c_k,   E = 32 * 2^-24,

c_k the oracle's absolute-sum scale of the normal equations' solution, and the
matching first-order bounds on flux_err, the covariance and chi2.  Every check
prints its largest observed ratio to the bound (1.0 is the bound).  No case
may sit on the singularity threshold: the oracle's squared pivots stay outside
1e-12 .. 1e-4.

Largest ratios observed on an MI355X (profiles/photometry/
pytest_gpu_photometry.txt): fluxes 0.030, flux_err and
covariance 0.062, chi2 0.019, a fitted background 0.004."""
import functools

import numpy as np
import pytest
import torch

import _photometry_oracle as O
from _params import M71, p_basic_model, p_m71_model
from smcdet_amd import extract, photometry
from smcdet_amd.images import M71ImageModel
from smcdet_amd.metrics import match_catalogs

pytestmark = pytest.mark.gpu
NAN = float("nan")


def m71_model(H, W, R=M71["psf_radius"]):
    p = M71
    return M71ImageModel(image_height=H, image_width=W, background=p["background"], psf_radius=R,
                         adu_per_nmgy=p["adu_per_nmgy"], psf_params=p["psf_params"],
                         noise_additive=p["noise_additive"],
                         noise_multiplicative=p["noise_multiplicative"])


def problems(model, catalogs, K, seed, background=None):
    """One image per catalog (locs, fluxes): the noisy render of its finite
    positions.  Returns images [T,H,W], counts [T], locs [T,K,2] (slots past a
    catalog hold a finite decoy the count must keep out)."""
    m = O.model_of(model)
    rng = np.random.default_rng(seed)
    T = len(catalogs)
    images = np.empty((T, m.H, m.W), np.float32)
    counts = np.zeros(T, np.int32)
    locs = np.full((T, K, 2), 2.25, np.float32)
    for t, (ll, ff) in enumerate(catalogs):
        ll = np.asarray(ll, np.float32).reshape(-1, 2)
        ok = np.isfinite(ll).all(1)
        B = None if background is None else float(background[t])
        images[t] = O.noisy(m, O.render(m, ll[ok], np.asarray(ff, np.float64)[ok], B), rng)
        counts[t] = len(ll)
        locs[t, :len(ll)] = ll
    return images, counts, locs


def on_device(images, counts, locs, background=None):
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (images, counts, locs)]
    if background is not None:
        d.append(torch.from_numpy(np.asarray(background, np.float32)).cuda())
    return d


def to_numpy(p):
    return {k: None if v is None else v.cpu().numpy() for k, v in p._asdict().items()}


def ratio(diff, tol):
    """max |diff| / tol over the finite entries (0 / 0 counts as 0)."""
    diff, tol = np.abs(np.asarray(diff, np.float64)), np.asarray(tol, np.float64)
    ok = np.isfinite(diff) & np.isfinite(tol)
    if not ok.any():
        return 0.0
    d, t = diff[ok], tol[ok]
    return float(np.max(np.where(d == 0, 0.0, d / np.where(t > 0, t, np.finfo(float).tiny))))


def compare(label, model, images, counts, locs, background=None, covariance=False, **kw):
    """Runs the device and the oracle on the same problems, asserts the layout
    and the bounds, prints the ratios; returns the device result (numpy)."""
    m = O.model_of(model)
    grid = locs.ndim == 4
    c4 = counts if grid else counts[:, None]
    l4 = locs if grid else locs[:, None]
    want = O.forced_photometry(m, images, c4, l4, background, kw.get("fit_background", False),
                               kw.get("n_iter", 4))
    assert O.pivots_clear_of_threshold(want["pivots"]), np.sort(want["pivots"])[:4]
    dev = on_device(images, counts, locs, background)
    got = photometry.forced_photometry(dev[0], dev[1], dev[2], model,
                                       background=dev[3] if background is not None else None,
                                       covariance=covariance, **kw)
    assert got.fluxes.dtype == torch.float64 and got.status.dtype == torch.int32
    assert got.fluxes.shape == locs.shape[:-1] and got.chi2.shape == counts.shape
    got = to_numpy(got)
    if not grid:
        want = {k: (v if k == "pivots" else v[:, 0]) for k, v in want.items()}
    for k in ("status", "n_free", "n_pixels"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("fluxes", "flux_err", "background", "chi2"):
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]), err_msg=k)
    np.testing.assert_array_equal(got["fluxes"] == 0, want["fluxes"] == 0)
    r = dict(flux=ratio(got["fluxes"] - want["fluxes"], O.E * want["c"]),
             err=ratio(got["flux_err"] - want["flux_err"], want["err_tol"]),
             chi2=ratio(got["chi2"] - want["chi2"], want["chi2_tol"]))
    if kw.get("fit_background"):
        r["bg"] = ratio(got["background"] - want["background"], O.E * want["c_background"])
    else:
        np.testing.assert_array_equal(got["background"], want["background"])
    if covariance:
        cov = got["cov"]
        assert cov.shape == locs.shape[:-1] + (locs.shape[-2],)
        assert cov.tobytes() == np.swapaxes(cov, -1, -2).copy().tobytes()  # symmetric bit for bit
        np.testing.assert_array_equal(np.isnan(cov), np.isnan(want["cov"]))
        r["cov"] = ratio(cov - want["cov"], want["cov_tol"])
        np.testing.assert_allclose(np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1)),
                                   got["flux_err"], rtol=4e-16, atol=0, equal_nan=True)
    else:
        assert got["cov"] is None
    print(f"{label}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()) + " of the bound")
    for k, v in r.items():
        assert v <= 1.0, (label, k, v)
    return got, want


# ---- M71, 8x8, R = 8: one pixel per lane ---------------------------------------------
def catalogs_8x8():
    cats = [O.CONFIGS[k] for k in O.CONFIGS]
    cats.append(([], []))                                                    # count 0
    cats.append(([(2.4, 5.1), (NAN, 3.0), (5.6, 2.2)], [45.0, 0.0, 30.0]))   # a NaN slot between
    cats.append(([(3.3, 3.9), (-20.0, 3.0)], [55.0, 0.0]))                   # a window off the image
    cats.append(([(4.2, 3.1), (4.2, 3.1), (6.0, 6.0)], [35.0, 35.0, 20.0]))  # identical positions
    return cats


@functools.lru_cache(None)
def batch_8x8():
    return problems(p_m71_model(8), catalogs_8x8(), 4, seed=101)


@pytest.mark.parametrize("fit_background, covariance", [(False, False), (True, False),
                                                        (False, True)])
def test_m71_8x8(fit_background, covariance):
    images, counts, locs = batch_8x8()
    got, want = compare(f"8x8 fit_background={fit_background}", p_m71_model(8), images, counts,
                        locs, fit_background=fit_background, covariance=covariance)
    st = got["status"]
    assert list(st) == [0, 0, 0, 0, 0, 0, 0, 1, 2]
    assert list(got["n_free"]) == [x + int(fit_background) for x in (1, 2, 2, 3, 1, 0, 2, 1, 3)]
    # count 0: nothing to solve, every slot skipped, chi2 of the background alone
    assert (got["fluxes"][5] == 0).all() and np.isnan(got["flux_err"][5]).all()
    assert np.isfinite(got["chi2"][5])
    # the NaN slot is skipped (0, NaN), its neighbours are solved; the decoy past the count too
    assert got["fluxes"][6][1] == 0 and np.isfinite(got["fluxes"][6][[0, 2]]).all()
    assert got["fluxes"][6][3] == 0 and np.isnan(got["flux_err"][6][[1, 3]]).all()
    # the source at (-20, 3) is dropped, the other one solved
    assert np.isnan(got["fluxes"][7][1]) and np.isfinite(got["fluxes"][7][0])
    # identical positions: the whole problem is NaN
    assert np.isnan(got["fluxes"][8][:3]).all() and np.isnan(got["flux_err"][8]).all()
    assert np.isnan(got["chi2"][8]) and np.isnan(got["background"][8])
    # the solved fluxes are near the truth (a gross error would be a wrong model, not rounding)
    for t, name in enumerate(O.CONFIGS):
        f = np.asarray(O.CONFIGS[name][1])
        assert np.all(np.abs(got["fluxes"][t][:len(f)] - f) < 6 * got["flux_err"][t][:len(f)])


# ---- other shapes: idle lanes, a ragged last pass, the limit ------------------------
SHAPES = {
    "5x5": (5, 5, [([(2.2, 2.7)], [40.0]), ([(0.6, 4.1), (3.8, 1.2)], [60.0, 25.0])]),
    "8x13": (8, 13, [([(3.1, 11.8), (5.2, 2.4), (6.9, 7.7)], [50.0, 30.0, 80.0]),
                     ([(7.99, 12.99)], [70.0])]),
    "32x32": (32, 32, [([(3.3, 28.4), (16.2, 15.8), (16.9, 16.7), (30.5, 1.5)],
                        [90.0, 40.0, 60.0, 20.0]), ([(31.5, 31.5), (-2.0, 10.0)], [50.0, 300.0])]),
}


@pytest.mark.parametrize("name, fit_background, covariance", [
    ("5x5", False, False), ("8x13", False, False), ("8x13", True, True), ("32x32", False, False)])
def test_other_shapes(name, fit_background, covariance):
    H, W, cats = SHAPES[name]
    model = m71_model(H, W)
    images, counts, locs = problems(model, cats, 4, seed=202)
    got, _ = compare(f"{name} fit_background={fit_background}", model, images, counts, locs,
                     fit_background=fit_background, covariance=covariance)
    assert (got["status"] == 0).all() and (got["n_pixels"] == H * W).all()


def test_window_anchor():
    """R = 2 on 16x16: between h = 3.999 and h = 4.0 the window moves by a row."""
    model = m71_model(16, 16, R=2)
    cats = [([(3.999, 5.3), (4.0, 10.6)], [80.0, 80.0]), ([(4.0, 5.3), (3.999, 10.6)], [80.0, 80.0])]
    images, counts, locs = problems(model, cats, 2, seed=303)
    m = O.model_of(model)
    a, b = O.columns(m, [(3.999, 5.3)])[:, 0], O.columns(m, [(4.0, 5.3)])[:, 0]
    rows = lambda c: sorted(set(np.flatnonzero(c) // 16))  # noqa: E731
    assert rows(a) == [1, 2, 3, 4, 5] and rows(b) == [2, 3, 4, 5, 6]
    compare("window anchor", model, images, counts, locs)


def test_full_slab():
    """K = 32 with 32 separated sources on 32x32."""
    model = m71_model(32, 32)
    rng = np.random.default_rng(404)
    hh, ww = np.meshgrid(4.0 + 8 * np.arange(4), 2.0 + 4 * np.arange(8), indexing="ij")
    ll = np.stack([hh.ravel(), ww.ravel()], -1) + rng.uniform(-0.4, 0.4, (32, 2))
    ff = rng.uniform(20.0, 200.0, 32)
    images, counts, locs = problems(model, [(ll, ff)], 32, seed=405)
    got, _ = compare("full slab", model, images, counts, locs, covariance=True)
    assert got["n_free"][0] == 32 and got["status"][0] == 0
    assert np.all(np.abs(got["fluxes"][0] - ff) < 6 * got["flux_err"][0])


def test_shared_image():
    """T = 3, G = 4: every image is shared by four lists with their own counts,
    under a per-image background."""
    model = p_m71_model(8)
    bg = np.array([80.0, 104.0, 150.0], np.float32)
    cats = [([(2.2, 2.9), (5.5, 5.1), (3.0, 6.2)], [60.0, 40.0, 25.0])] * 3
    images, _, l3 = problems(model, cats, 4, seed=505, background=bg)
    locs = np.repeat(l3[:, None], 4, axis=1).copy()
    locs[:, 1, 1] += 0.25            # list 1 displaces a source
    locs[:, 3, :, 0] = l3[:, ::-1, 0]  # list 3 holds other rows
    counts = np.tile(np.array([3, 2, 0, 4], np.int32), (3, 1))
    got, want = compare("shared image", model, images, counts, locs, background=bg)
    np.testing.assert_array_equal(got["n_free"], counts)
    assert (got["background"] == bg[:, None]).all()
    # a list's result does not depend on its neighbours in the launch
    dev = on_device(images[1:2], counts[1:2, 1:2], locs[1:2, 1:2], bg[1:2])
    alone = photometry.forced_photometry(dev[0], dev[1], dev[2], model, background=dev[3])
    assert alone.fluxes.cpu().numpy().tobytes() == got["fluxes"][1:2, 1:2].tobytes()


def test_poisson_model_16x16():
    model = p_basic_model(16)
    cats = [([(4.3, 5.1), (9.7, 11.2), (10.4, 11.9)], [3000.0, 5000.0, 2500.0]),
            ([(15.6, 0.3)], [4000.0])]
    images, counts, locs = problems(model, cats, 4, seed=606)
    got, _ = compare("poisson 16x16", model, images, counts, locs)
    assert (got["status"] == 0).all()
    compare("poisson 16x16 fit_background=True", model, images, counts, locs, fit_background=True)


# ---- determinism and layout -----------------------------------------------------------
def bits(p):
    return b"".join(x.cpu().numpy().tobytes() for x in p if x is not None)


def test_determinism_offsets_and_strides():
    model = p_m71_model(8)
    images, counts, locs = batch_8x8()
    img, cnt, loc = on_device(images, counts, locs)
    call = lambda *a: photometry.forced_photometry(*a, model, covariance=True)  # noqa: E731
    first = bits(call(img, cnt, loc))
    assert bits(call(img, cnt, loc)) == first
    # the same problems behind other allocation offsets (views into larger buffers)
    def shifted(x, k):
        buf = torch.zeros(x.numel() + k + 5, device=x.device, dtype=x.dtype)
        v = buf[k:k + x.numel()].view(x.shape)
        v.copy_(x)
        return v
    junk = [torch.empty(n, device="cuda") for n in (1031, 77, 4099)]  # move the allocator along
    assert bits(call(shifted(img, 3), shifted(cnt, 1), shifted(loc, 7))) == first
    del junk
    # non-contiguous views are made contiguous, never misread
    wide = torch.zeros(img.shape[0], 8, 16, device="cuda")
    wide[:, :, ::2] = img
    loc4 = torch.full((loc.shape[0], loc.shape[1], 4), 9.0, device="cuda")
    loc4[..., :2] = loc
    cnt2 = torch.stack([cnt, cnt + 1], 1)
    views = (wide[:, :, ::2], cnt2[:, 0], loc4[..., :2])
    assert not any(v.is_contiguous() for v in views)
    assert bits(call(*views)) == first
    # int64 counts are the same problems
    assert bits(call(img, cnt.long(), loc)) == first


# ---- photometry_of, tune, condensed catalogs -------------------------------------------
def planted_tiles(T=16, H=8):
    """Synthetic M71 tiles with a known truth: one to three stars per tile."""
    model = p_m71_model(H)
    rng = np.random.default_rng(707)
    cats = []
    for t in range(T):
        n = 1 + t % 3
        cats.append((rng.uniform(0.8, H - 0.8, (n, 2)), 10 ** rng.uniform(1.3, 2.3, n)))
    images, counts, locs = problems(model, cats, 3, seed=708)
    fluxes = np.zeros((T, 3), np.float32)
    for t, (_, f) in enumerate(cats):
        fluxes[t, :len(f)] = f
        locs[t, len(f):] = 0
    return model, images, counts, locs, fluxes


def test_tune_psf_equals_the_chain_by_hand():
    model, images, tc, tl, tf = planted_tiles()
    p = M71
    sigma = float(np.sqrt(p["noise_multiplicative"] * p["background"]))
    K, tol, bins = 8, 0.5, torch.tensor([14.0, 22.0])
    grid = dict(thresh=[1.5, 4.0], minarea=[1, 5], deblend_cont=[0.005], clean_param=[1.0])
    img, tc, tl, tf = [torch.from_numpy(x).cuda() for x in (images, tc, tl, tf)]
    common = dict(deblend_nthresh=32, max_detections=K, locs_tol=tol, mags_tol=tol, mag_bins=bins,
                  flux_scale=p["adu_per_nmgy"])
    r = extract.tune(img, p["background"], sigma, tc, tl, tf, **grid, **common, flux="psf",
                     image_model=model)
    # by hand: extract_grid -> photometry_of -> match_catalogs
    ex = extract.extract_grid(img, p["background"], sigma, **grid, deblend_nthresh=32,
                              max_detections=K, flux_scale=p["adu_per_nmgy"])
    ex2, phot = photometry.photometry_of(ex, img, model)
    assert ex2.fluxes.dtype == torch.float32 and ex2.locs is ex.locs and ex2.counts is ex.counts
    solved = torch.isfinite(phot.fluxes)
    assert torch.equal(ex2.fluxes[solved], phot.fluxes[solved].float())
    assert torch.equal(ex2.fluxes[~solved], ex.fluxes[~solved])  # a failed solve keeps its flux
    tt, tm, et, em = match_catalogs(tc, tl, tf, ex2.counts, ex2.locs, ex2.fluxes, None, tol, tol,
                                    bins)
    precision = (em.sum(0) / et.sum(0)).nan_to_num(0)
    recall = (tm.sum(0) / tt.sum(0)).nan_to_num(0)
    f1 = ((2 * precision * recall) / (precision + recall)).nan_to_num(0)[:, -1]
    assert r.f1.shape == (4,) and r.f1.cpu().numpy().tobytes() == f1.cpu().numpy().tobytes()
    assert float(r.f1.max()) > 0
    # chunked over the settings: the same bits
    r1 = extract.tune(img, p["background"], sigma, tc, tl, tf, **grid, **common, flux="psf",
                      image_model=model, max_bytes=1)
    assert r1.f1.cpu().numpy().tobytes() == r.f1.cpu().numpy().tobytes()
    # the default path is what it was: the argument's default changes nothing
    a = extract.tune(img, p["background"], sigma, tc, tl, tf, **grid, **common)
    b = extract.tune(img, p["background"], sigma, tc, tl, tf, **grid, **common, flux="isophotal")
    assert a.f1.cpu().numpy().tobytes() == b.f1.cpu().numpy().tobytes()
    assert a.best == b.best and a.best_index == b.best_index
    print(f"tune: best F1 isophotal {float(a.f1.max()):.3f}, psf {float(r.f1.max()):.3f}")


def test_photometry_of_a_single_setting():
    model, images, tc, tl, tf = planted_tiles()
    p = M71
    img = torch.from_numpy(images).cuda()
    sigma = float(np.sqrt(p["noise_multiplicative"] * p["background"]))
    ex = extract.extract(img, p["background"], sigma, 4.0, minarea=3, max_detections=4,
                         flux_scale=p["adu_per_nmgy"])
    ex2, phot = photometry.photometry_of(ex, img, model)
    assert phot.fluxes.shape == ex.fluxes.shape and isinstance(ex2, extract.Extraction)
    direct = photometry.forced_photometry(img, ex.counts, ex.locs, model)
    assert bits(direct) == bits(phot)


def test_photometry_condensed():
    from smcdet_amd.condense import CondensedCatalog
    model, images, tc, tl, tf = planted_tiles(T=4)
    T, K = 4, 5
    dev = dict(device="cuda")
    prob = torch.tensor([[0.9, 0.2, 0.8, 0.0, 0.0]] * T, **dev)
    locs = torch.full((T, K, 2), NAN, **dev)
    fluxes = torch.full((T, K), NAN, **dev)
    tl_d, tf_d = torch.from_numpy(tl).cuda(), torch.from_numpy(tf).cuda()
    locs[:, 0], fluxes[:, 0] = tl_d[:, 0], tf_d[:, 0] * 1.1     # kept: the first true star
    locs[:, 1], fluxes[:, 1] = tl_d[:, 0] + 2.0, 5.0            # below min_prob
    locs[:, 2, 0], locs[:, 2, 1], fluxes[:, 2] = 6.5, 1.5, 3.0  # kept
    z0 = torch.zeros(T, K, **dev)
    cat = CondensedCatalog(
        n_seeds=torch.full((T,), 3, dtype=torch.int32, **dev), seed_locs=locs, seed_mass=z0,
        prob=prob, locs=locs, locs_sd=torch.zeros(T, K, 2, **dev), locs_cov_hw=z0, fluxes=fluxes,
        fluxes_sd=z0, mags=z0, mags_sd=z0, flux_quantiles=torch.zeros(T, K, 1, **dev),
        quantiles=(0.5,), expected_count=prob.sum(-1), unassociated=torch.zeros(T, **dev),
        moments=torch.zeros(T, K, 10, dtype=torch.float64, **dev))
    img = torch.from_numpy(images).cuda()
    phot, z = photometry.photometry_condensed(cat, img, model, min_prob=0.5)
    counts, cl, cf = cat.as_catalog(0.5)
    direct = photometry.forced_photometry(img, counts[:, 0], cl[:, 0].contiguous(), model)
    assert bits(direct) == bits(phot)
    assert z.shape == (T, K) and torch.isnan(z[:, 2:]).all() and torch.isfinite(z[:, :2]).all()
    want = (phot.fluxes[:, :2] - cf[:, 0, :2].double()) / phot.flux_err[:, :2]
    assert torch.equal(z[:, :2], want)
