"""The image-model kernels on both sides of every dispatch boundary, against
the float64 oracle.

smcdet_loglik picks its render by shape: registers with 1, 4 or 16 pixels per
lane (<= 64, <= 256, <= 1024 pixels), the per-wave LDS image (<= 4096 pixels,
or any S > 64), and 64-pixel chunks with the tile in global memory (M71 only,
S <= 64).  smcdet_render and smcdet_psf_dense see the same shapes.  The
register render's row index was wrong on wide flat tiles (W >= 71, H <= 14:
at 8x104 pixel 831, the last of row 7, was taken for row 8, column -1), which
no square tile shows; the rectangles below include those shapes, each in both
orientations so that an H / W swap shows too.

Catalogs are built, not drawn: a grid of sources that puts every pixel in a
window with a contribution of at least 1% of the background (where S and the
radius allow it), sources exactly on integer coordinates, in the padding, on
the corners, one row / column outside reach (floor(loc) = -R-1 and dim+R), at
the last position within reach, and at +-1e5.  A mis-indexed pixel is then an
error thousands of times the tolerance.

The MH sweep runs the same wide tiles (and radii other than 8) under replayed
draws against the oracle's sweep, incremental and with full recompute.
"""
import math

import numpy as np
import pytest
import torch

from oracle import smc_oracle as O
from tests._params import BASIC_BACKGROUND, M71

pytestmark = pytest.mark.gpu
DEV = "cuda"
EUNSUPPORTED = -2
T = 3
S_VALUES = [0, 1, 64, 65]
R_VALUES = [0, 1, 8, 40]
POISSON_PSF_STDEV = 3.0   # wide enough for the coverage grid to reach 1% of the background

SQUARES = [(8, 8), (16, 16), (32, 32)]
RECTS = [(5, 13),      # 65 px: first with 4 pixels per lane
         (1, 257),     # 257 px: first with 16 pixels per lane
         (25, 41),     # 1025 px: first on the LDS path
         (64, 65),     # 4160 px: first on the global-memory path (M71 only)
         (14, 71), (10, 85), (8, 104), (4, 134), (2, 195),   # wide flat tiles
         (8, 16), (16, 32)]                                  # what tile aggregation produces
SHAPES = SQUARES + [(64, 64), (1, 1)] + RECTS + [(w, h) for h, w in RECTS]
CASES = [("m71", h, w) for h, w in SHAPES] + \
        [("poisson", h, w) for h, w in SHAPES if h * w <= 4096]

# rate images: the largest relative error against the float64 oracle over the
# square 8x8, 16x16 and 32x32 cases of test_model_at_shape (both models, every
# S / radius / N below) is RATE_RELERR_SQUARE; the other shapes get four times
# that (the sum order differs by path, the number of float32 additions per
# pixel does not).
RATE_RELERR_SQUARE = 8.8e-7   # measured on an MI355X: 8.783e-07 (m71 32x32 S=65 R=40 N=5)
RATE_RTOL = 4 * RATE_RELERR_SQUARE


def combos():
    """(S, R, N): every S with every radius; N alternates 5 / 1 so that each S
    and each radius meets both (either leaves part of a 4-wave workgroup empty)."""
    return [(S, R, 5 if (i + j) % 2 == 0 else 1)
            for i, S in enumerate(S_VALUES) for j, R in enumerate(R_VALUES)]


# ---- models ---------------------------------------------------------------
_M71_NORM_R8 = O.m71_psf_normalizer(tuple(np.float32(p) for p in M71["psf_params"]), 8)


def o_model(kind, H, W, R):
    if kind == "m71":
        p = M71
        m = O.M71Model(H, W, p["background"], max(R, 1), p["adu_per_nmgy"], p["psf_params"],
                       p["noise_additive"], p["noise_multiplicative"])
        if R == 0:
            # the normaliser sums a (32 R)^2 grid: empty at R = 0.  Both sides
            # take the radius-8 constant there.
            m.psf_radius, m.norm_const = 0, _M71_NORM_R8
        return m
    return O.BasicModel(H, W, BASIC_BACKGROUND, R, POISSON_PSF_STDEV)


def p_model(kind, H, W, R):
    from smcdet_amd.images import ImageModel, M71ImageModel
    if kind == "m71":
        p = M71
        m = M71ImageModel(image_height=H, image_width=W, background=p["background"],
                          psf_radius=max(R, 1), adu_per_nmgy=p["adu_per_nmgy"],
                          psf_params=p["psf_params"], noise_additive=p["noise_additive"],
                          noise_multiplicative=p["noise_multiplicative"])
        if R == 0:
            m.psf_radius = 0
            m.psf_normalizing_constant = torch.tensor(_M71_NORM_R8, dtype=torch.float32)
        return m
    return ImageModel(image_height=H, image_width=W, psf_radius=R, psf_stdev=POISSON_PSF_STDEV,
                      background=BASIC_BACKGROUND)


# ---- catalogs ---------------------------------------------------------------
def grid_step(R):
    return 2 * min(R, 6) + 1


N_SPECIAL = 15   # the bright source and the edge cases that lead every catalog


def grid_fits(H, W, R, S):
    st = grid_step(R)
    return S - N_SPECIAL >= math.ceil(H / st) * math.ceil(W / st)


def catalog(kind, H, W, R, S, N):
    """locs [T,1,N,S,2], fluxes [T,1,N,S] (float32).  Source 0 is the bright
    one on integer coordinates; then the edge cases, the coverage grid and
    faint fillers.  Every (tile, particle) scales the fluxes differently and
    shifts the grid and the fillers by a fraction of a pixel (the floors stay)."""
    m71 = kind == "m71"
    bright, med, unseen, gflux, faint = ((50.0, 30.0, 1000.0, 80.0, 1.0) if m71 else
                                         (9.0e5, 3000.0, 3.0e4, 3200.0, 100.0))
    mh, mw = H // 2, W // 2
    special = [
        (float(mh), float(mw), bright),          # exactly on integer coordinates
        (-0.75, 0.3 * W, med),                   # negative, inside the padding
        (0.6 * H, -0.25, med),
        (0.0, 0.0, med),                         # the corners
        (H - 0.25, W - 0.25, med),
        (0.25, W - 0.5, med),
        (float(H), float(W), med),
        (-R - 0.5, mw + 0.5, unseen),            # floor = -R-1: one row outside reach
        (H + R + 0.25, mw + 0.5, unseen),        # floor = H+R
        (mh + 0.5, -R - 0.5, unseen),
        (mh + 0.5, W + R + 0.25, unseen),
        (-R + 0.5, 0.7 * W, med),                # floor = -R: reaches row 0 only
        (0.4 * H, W + R - 0.5, med),             # floor = W+R-1: reaches the last column only
        (1.0e5, 1.0e5, unseen),                  # far outside
        (-1.0e5, 3.0, unseen),
    ]
    assert len(special) == N_SPECIAL
    st, re = grid_step(R), min(R, 6)
    grid = [(i * st + re + 0.37, j * st + re + 0.37, gflux * (1 + 0.1 * ((i + j) % 3)))
            for i in range(math.ceil(H / st)) for j in range(math.ceil(W / st))]
    src = (special + grid)[:S]
    n_fixed = min(S, N_SPECIAL)
    q = np.arange(max(S - len(src), 0)) + 1.0
    fill = [(float((a * 0.6180339887) % 1) * (H + 2) - 1,
             float((a * 0.3819660113) % 1) * (W + 2) - 1, faint) for a in q]
    src = np.array(src + fill, np.float64).reshape(S, 3)
    locs = np.broadcast_to(src[:, :2], (T, 1, N, S, 2)).copy()
    t = np.arange(T)[:, None, None, None]
    n = np.arange(N)[None, None, :, None]
    shift = 0.05 * n - 0.02 * t                              # keeps every floor
    locs[:, :, :, n_fixed:, :] += shift[..., None]
    fluxes = src[:, 2] * (1 + 0.07 * n + 0.19 * t)
    return locs.astype(np.float32), fluxes.astype(np.float32)


def window_mask(locs, H, W, R):
    """[T,1,H,W,N,S]: pixel inside source's (2R+1)^2 window anchored at floor(loc)."""
    hh = np.arange(H)[:, None, None, None]
    ww = np.arange(W)[None, :, None, None]
    fh = np.floor(locs[..., 0].astype(np.float64))[:, :, None, None]
    fw = np.floor(locs[..., 1].astype(np.float64))[:, :, None, None]
    return (np.abs(hh - fh) <= R) & (np.abs(ww - fw) <= R)


def clear_of_branch(kind, om, locs, fluxes):
    """Poisson: scale each particle's bright source until no pixel's float64
    rate lies within 1% of the likelihood's branch point 5e4 (the rate is
    linear in that flux).  Returns the fluxes and the oracle's rate."""
    if kind == "m71" or fluxes.shape[-1] == 0:
        return fluxes, O.render_rate(locs, fluxes, om)
    f0 = fluxes.copy()
    f0[..., 0] = 0
    rest = O.render_rate(locs, f0, om)                               # [T,1,H,W,N]
    psf0 = O.psf_dense(locs[..., :1, :], om)[..., 0]                 # [T,1,H,W,N]
    fb = fluxes[..., 0].copy()                                       # [T,1,N]
    for _ in range(200):
        rate = rest + psf0 * fb.astype(np.float64)[:, :, None, None, :]
        near = (np.abs(rate / 5e4 - 1) < 0.01).any(axis=(2, 3))      # [T,1,N]
        if not near.any():
            break
        fb = np.where(near, fb * np.float32(1.003), fb).astype(np.float32)
    fluxes = fluxes.copy()
    fluxes[..., 0] = fb
    rate = O.render_rate(locs, fluxes, om)
    assert not (np.abs(rate / 5e4 - 1) < 0.01).any()
    return fluxes, rate


def images(kind, om, rate, seed):
    """A noisy image per tile around the rate of the tile's particle 0."""
    g = np.random.default_rng(seed)
    r0 = rate[..., 0]
    if kind == "m71":
        sd = np.sqrt(om.noise_additive + om.noise_multiplicative * r0)
        return (r0 + sd * g.standard_normal(r0.shape)).astype(np.float32)
    return g.poisson(r0).astype(np.float32)


def oracle_loglik(kind, om, img, rate):
    x = img.astype(np.float64)[..., None]
    ll = O.m71_pixel_loglik(x, rate, om) if kind == "m71" else O.poisson_pixel_loglik(x, rate)
    return ll.sum(axis=(2, 3))


def dev(x):
    return torch.as_tensor(x, device=DEV)


def npy(t):
    return t.detach().cpu().numpy()


def relerr(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.abs(ref))) if ref.size else 0.0


def check_case(kind, H, W, S, R, N, om, pm, report):
    """One (shape, S, radius, N): psf, rate and loglikelihood against the
    oracle; appends what is wrong to `report` and returns the rate's relative
    error."""
    tag = f"{kind} {H}x{W} S={S} R={R} N={N}"
    locs, fluxes = catalog(kind, H, W, R, S, N)
    fluxes, rate_ref = clear_of_branch(kind, om, locs, fluxes)
    img = images(kind, om, rate_ref, seed=H * 1000 + W)
    dl, df, di = dev(locs), dev(fluxes), dev(img)
    if H * W > 4096 and S > 64:
        for call in (lambda: pm.rate(dl, df), lambda: pm.loglikelihood(di, dl, df)):
            with pytest.raises(RuntimeError, match=rf"\({EUNSUPPORTED}\)"):
                call()
        return 0.0
    inwin = window_mask(locs, H, W, R)
    touched = inwin.any(-1)
    psf_ref = O.psf_dense(locs, om)
    if S >= 64 and R >= 1 and grid_fits(H, W, R, S):
        # the fixture's own promise: every pixel gets >= 1% of the background
        g = getattr(om, "adu_per_nmgy", 1.0)
        best = (psf_ref * (g * fluxes.astype(np.float64))[:, :, None, None]).max(-1)
        assert touched.all() and best.min() >= 0.01 * om.background, tag
    if kind == "poisson" and S >= 1:
        # both branches of the likelihood (a one-pixel tile has the upper one only)
        assert (rate_ref > 5e4).any() and ((rate_ref < 5e4).any() or H * W == 1), tag
    # psf (S = 0 has none: the entry point refuses an empty tensor)
    if S > 0:
        got = npy(pm.psf(dl))
        atol = 2e-8 if kind == "m71" else 1e-7
        bad = ~np.isclose(got, psf_ref, rtol=2e-6, atol=atol)
        if bad.any():
            report.append(f"{tag}: psf off at {int(bad.sum())} of {bad.size}, first "
                          f"{tuple(np.argwhere(bad)[0])}")
        if (got[~inwin] != 0).any():
            report.append(f"{tag}: psf non-zero outside the windows")
    # rate
    got = npy(pm.rate(dl, df))
    err = relerr(got, rate_ref)
    print(f"RATE_RELERR {tag} {err:.3e}")
    if not err <= RATE_RTOL:
        report.append(f"{tag}: rate relative error {err:.3e} > {RATE_RTOL:.2e}")
    if (got[~touched] != np.float32(om.background)).any():
        report.append(f"{tag}: rate differs from the background outside every window")
    # loglikelihood
    ll_ref = oracle_loglik(kind, om, img, rate_ref)
    got = npy(pm.loglikelihood(di, dl, df))
    bad = ~np.isclose(got, ll_ref, rtol=2e-6, atol=5e-3)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        report.append(f"{tag}: loglik off for {int(bad.sum())} of {bad.size} particles, e.g. "
                      f"{got[i]:.6f} vs {ll_ref[i]:.6f} (|d| max "
                      f"{np.abs(got - ll_ref).max():.3e})")
    return err


@pytest.mark.parametrize("kind,H,W", CASES, ids=[f"{k}-{h}x{w}" for k, h, w in CASES])
def test_model_at_shape(kind, H, W):
    report = []
    models = {R: (o_model(kind, H, W, R), p_model(kind, H, W, R)) for R in R_VALUES}
    for S, R, N in combos():
        try:
            check_case(kind, H, W, S, R, N, *models[R], report)
        except RuntimeError as e:    # a refused call: reported with the rest
            report.append(f"{kind} {H}x{W} S={S} R={R} N={N}: {e}")
    assert not report, "\n".join(report)


@pytest.mark.parametrize("H,W", [(64, 65), (65, 64)])
def test_poisson_refused_above_lds_budget(H, W):
    """Tiles above 4096 pixels run the M71 model only."""
    pm = p_model("poisson", H, W, 8)
    locs = torch.zeros(1, 1, 1, 1, 2, device=DEV)
    fluxes = torch.ones(1, 1, 1, 1, device=DEV)
    img = torch.full((1, 1, H, W), 200.0, device=DEV)
    for call in (lambda: pm.rate(locs, fluxes), lambda: pm.loglikelihood(img, locs, fluxes),
                 lambda: pm.psf(locs)):
        with pytest.raises(RuntimeError, match=rf"\({EUNSUPPORTED}\)"):
            call()


# ---- the MH sweep on the same shapes ----------------------------------------
SWEEPS = [(8, 104, 8, 0.1), (8, 104, 40, 0.1), (24, 40, 20, 0.1), (10, 85, 8, 0.1),
          (14, 71, 8, 0.1),
          # long jumps on a tile wider than 256: union windows of up to 227 columns
          (2, 300, 64, 20.0),
          # ... and of more than 256, which the incremental sweep refuses (its
          # 16-bit row / column split of a window position is exact to 256)
          (2, 300, 64, 60.0)]


@pytest.mark.parametrize("full", [False, True], ids=["incremental", "full"])
@pytest.mark.parametrize("H,W,R,locs_stdev", SWEEPS,
                         ids=[f"{h}x{w}-R{r}-sd{s:g}" for h, w, r, s in SWEEPS])
def test_mh_sweep_vs_oracle(H, W, R, locs_stdev, full):
    """smcdet_mh_sweep under replayed draws against O.mh_sweep, decision by
    decision, and its loglik_out against a fresh oracle likelihood of the
    state it returns.  Sources sit on the tile's last pixel (the one the
    register render mis-rowed) and next to (H, -1), where it was looked for."""
    from smcdet_amd.kernel import SingleComponentMH
    from smcdet_amd.prior import M71Prior
    p = M71
    N, S, K, nT, pad = 16, 4, 20, 2, 2
    om, pm = o_model("m71", H, W, R), p_model("m71", H, W, R)
    prior = M71Prior(min_objects=S, max_objects=S, counts_rate=p["counts_rate"], image_height=H,
                     image_width=W, flux_alpha=p["flux_alpha"], flux_lower=p["flux_lower"],
                     flux_upper=p["flux_upper"], pad=pad)
    oprior = O.M71PriorP(S, S, p["counts_rate"], H, W, pad, p["flux_alpha"], p["flux_lower"],
                         p["flux_upper"])
    g = np.random.default_rng(H * 1000 + W + R)
    locs = np.empty((1, nT, N, S, 2), np.float32)
    locs[..., 0] = -pad + g.random((1, nT, N, S)) * (H + 2 * pad)
    locs[..., 1] = -pad + g.random((1, nT, N, S)) * (W + 2 * pad)
    locs[..., 0, :] = np.array([H - 0.5, W - 0.5]) + 0.3 * (g.random((1, nT, N, 2)) - 0.5)
    locs[..., 1, :] = np.array([H - 0.4, 0.4]) + 0.3 * (g.random((1, nT, N, 2)) - 0.5)
    fluxes = (2.0 + 18.0 * g.random((1, nT, N, S))).astype(np.float32)
    counts = np.full((1, nT, N), float(S), np.float32)
    truth = O.render_rate(locs[:, :, :1], fluxes[:, :, :1], om)[..., 0]
    img = (truth + np.sqrt(om.noise_additive + om.noise_multiplicative * truth)
           * g.standard_normal(truth.shape)).astype(np.float32)
    comp = g.integers(0, S, (K, 1, nT, N)).astype(np.int32)
    comp[:4] = np.array([0, 1, 0, 1], np.int32)[:, None, None, None]
    uloc = g.random((K, 1, nT, N, 2)).astype(np.float32)
    uflux = g.random((K, 1, nT, N)).astype(np.float32)
    uacc = g.random((K, 1, nT, N)).astype(np.float32)
    tau = np.full((1, nT), 0.3, np.float32)
    mh = SingleComponentMH(K, locs_stdev, 2.5, p["flux_lower"], p["flux_upper"],
                           full_recompute=full)
    tr_acc = torch.zeros(K, 1, nT, N, device=DEV, dtype=torch.uint8)
    rp = {k: torch.as_tensor(v) for k, v in
          dict(comp=comp, uloc=uloc, uflux=uflux, uacc=uacc).items()}
    rp["trace_accept"] = tr_acc
    args = (dev(img), dev(counts), dev(locs), dev(fluxes), dev(tau))
    if not full and W > 256 and 2 * R + 2 + 4.8 * locs_stdev > 256:
        with pytest.raises(RuntimeError, match=rf"\({EUNSUPPORTED}\)"):
            mh.run(*args, prior=prior, image_model=pm, replay=rp)
        return
    l1, f1, _ = mh.run(*args, prior=prior, image_model=pm, replay=rp)
    ll1 = npy(mh.last_loglik)
    l1, f1 = npy(l1), npy(f1)
    ol, of, _, loga, oacc = O.mh_sweep(img, counts, locs, fluxes, tau, oprior, om,
                                       O.MHParams(K, locs_stdev, 2.5, p["flux_lower"],
                                                  p["flux_upper"]),
                                       comp, uloc, uflux, uacc, trace=True)
    margin = np.abs(np.nan_to_num(loga - np.log(uacc.astype(np.float64)), nan=1.0))
    clear = (margin > 1e-3).all(0)                      # particles with no near-tie decision
    print(f"clear {clear.mean():.3f}  oracle accept rate {oacc.mean():.3f}")
    assert clear.mean() > 0.9
    assert 0.02 < oacc.mean() < 0.98                    # the replay both accepts and rejects
    np.testing.assert_array_equal(npy(tr_acc).astype(bool)[:, clear], oacc[:, clear])
    # (the proposals are float32 roundings of different arithmetic: two ulps at
    # the tile's far edge where those exceed the 2e-5 of the 8-pixel tiles)
    atol_loc = max(2e-5, 2 * float(np.spacing(np.float32(max(H, W) + pad))))
    np.testing.assert_allclose(l1[clear], ol[clear], rtol=0, atol=atol_loc)
    np.testing.assert_allclose(f1[clear], of[clear], rtol=3e-5, atol=1e-4)
    # the likelihood the sweep returns, of the state the sweep returns
    fresh = O.loglikelihood(img, l1, f1, om)
    np.testing.assert_allclose(ll1, fresh, rtol=3e-5, atol=1e-4)
