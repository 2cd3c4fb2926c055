"""smcdet_amd.predictive on the GPU, against the float64 oracle
(tests/_predictive_oracle.py) on both sides of every dispatch boundary of
smcdet_posterior_image: registers with 1, 4 and 16 pixels per lane (<= 64,
<= 256, <= 1024 pixels, S <= 64), the per-wave LDS image (<= 4096 pixels, or
S = 65), 64-pixel chunks (M71 above 4096 pixels), and one, two and three
chunks of catalogs with a ragged last one.  Models and built catalogs are
those of tests/test_gpu_model_shapes.py.

Tolerances, derived (r = RATE_RTOL, the project's bound on a rendered rate):
  mean  |d| <= (r + 2^-23) mean
  var   |d| <= 2 r sd rms + r^2 rms^2 + 2^-23 var   (first-order propagation
        of a relative error r in every rate; sd, rms the oracle's)
  chi2  |d| <= 2 r sum_p (|2 (x - l) / v| + eta (x - l)^2 / v^2) l + 1e-6 chi2
The replicate noise is checked exactly where the rate is the background bit
for bit (S = 0), against the two-kernel route (smcdet_render, then
smcdet_sample_image) with the M71 model, and against its law with the Poisson
model, whose draws are not continuous in the rate.
"""
import numpy as np
import pytest
import torch

from oracle import smc_oracle as SO
from smcdet_amd import _hip, predictive
from tests import _noise_stats as NS
from tests import _predictive_oracle as O
from tests.test_gpu_model_shapes import RATE_RTOL, T, catalog, images, o_model, p_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
R_TOL = RATE_RTOL
SEED = 20261019          # fixed before the first run
N_CHUNKED = 70           # three chunks of catalogs: 24 + 24 + 22

BOTH = [(8, 8), (5, 13), (13, 5), (1, 257), (16, 16), (25, 41), (32, 32)]
M71_ONLY = [(64, 65), (65, 64)]
CASES = [("m71", h, w) for h, w in BOTH + M71_ONLY] + [("poisson", h, w) for h, w in BOTH]
S_VALUES = [0, 1, 10, 65]


def dev(x):
    return torch.tensor(x, device=DEV)


def npy(t):
    return t.detach().cpu().numpy()


def radii(H, W):
    return [8, 0, 40] if (H, W) in ((8, 8), (32, 32)) else [8]


def catalog_counts(H, W):
    return [1, 5, N_CHUNKED] if (H, W) in ((8, 8), (16, 16)) else [1, 5]


def weight_modes(N, rng):
    """None; random weights with one exact zero; all the weight on one catalog."""
    w = rng.uniform(0.2, 3.0, (T, 1, N)).astype(np.float32)
    w[np.arange(T), 0, rng.integers(0, N, T)] = 0.0
    one = np.zeros((T, 1, N), np.float32)
    one[np.arange(T), 0, rng.integers(0, N, T)] = rng.uniform(0.2, 3.0, T).astype(np.float32)
    modes = [("uniform", None), ("single", one)]
    if N > 1:
        modes.append(("random", w))
    return modes


_ref_cache = {}


def reference(kind, H, W, R, S, N):
    """The oracle's rate and the test image for one (shape, radius, S, N):
    computed once, shared by the tests, never modified."""
    key = (kind, H, W, R, S, N)
    if key not in _ref_cache:
        om = o_model(kind, H, W, R)
        locs, fluxes = catalog(kind, H, W, R, S, N)
        rate = SO.render_rate(locs, fluxes, om)
        img = images(kind, om, rate, seed=H * 1000 + W)
        for a in (locs, fluxes, rate, img):
            a.setflags(write=False)
        _ref_cache[key] = (om, locs, fluxes, rate, img)
    return _ref_cache[key]


def run(pm, locs, fluxes, weights=None, img=None, seed=SEED, offset=0):
    return predictive.posterior_image(
        pm, dev(locs), dev(fluxes), weights=None if weights is None else dev(weights),
        tiled_image=None if img is None else dev(img), seed=seed, offset=offset)


def check_moments(tag, got, rate, weights, report):
    mean, var, rms = O.moments(rate, weights)
    gm, gv = npy(got.mean).astype(np.float64), npy(got.rate_var).astype(np.float64)
    em = np.abs(gm - mean) / ((R_TOL + EPS) * mean)
    bound = 2 * R_TOL * np.sqrt(var) * rms + R_TOL ** 2 * rms ** 2 + EPS * var
    ev = np.abs(gv - var) / bound
    print(f"PRED {tag}: mean err/bound {em.max():.3f}  var err/bound {ev.max():.3f}  "
          f"min var/mean^2 {(var / mean ** 2).min():.2e}")
    if not em.max() <= 1:
        report.append(f"{tag}: mean off by {em.max():.3f} of its bound")
    if not ev.max() <= 1:
        report.append(f"{tag}: var off by {ev.max():.3f} of its bound")
    if (gv < 0).any():
        report.append(f"{tag}: negative variance")


def check_chi2(tag, got, om, img, rate, report):
    want = O.chi2(om, img, rate)
    bound = 2 * R_TOL * O.chi2_sensitivity(om, img, rate) + 1e-6 * want
    err = np.abs(npy(got.chi2).astype(np.float64) - want) / bound
    print(f"PRED {tag}: chi2 err/bound {err.max():.3f}")
    if not err.max() <= 1:
        report.append(f"{tag}: chi2 off by {err.max():.3f} of its bound")


@pytest.mark.parametrize("kind,H,W", CASES, ids=[f"{k}-{h}x{w}" for k, h, w in CASES])
def test_posterior_image_at_shape(kind, H, W):
    report = []
    rng = np.random.default_rng(H * 1000 + W)
    for R in radii(H, W):
        pm = p_model(kind, H, W, R)
        for S in S_VALUES:
            if S > 64 and H * W > 4096:
                continue
            for N in catalog_counts(H, W):
                om, locs, fluxes, rate, img = reference(kind, H, W, R, S, N)
                for mode, w in weight_modes(N, rng):
                    tag = f"{kind} {H}x{W} R={R} S={S} N={N} {mode}"
                    got = run(pm, locs, fluxes, w, img)
                    assert tuple(got.mean.shape) == (T, 1, H, W)
                    assert tuple(got.chi2.shape) == tuple(got.flux_rep.shape) == (T, 1, N)
                    check_moments(tag, got, rate, w, report)
                    if mode == "single" or N == 1:
                        # one catalog holds all the weight: exactly no spread
                        if (got.rate_var != 0).any():
                            report.append(f"{tag}: var not exactly 0 for a single catalog")
                    if mode == "uniform":
                        check_chi2(tag, got, om, img, rate, report)
                        for name in ("chi2_rep", "flux_rep"):
                            if not torch.isfinite(getattr(got, name)).all():
                                report.append(f"{tag}: {name} not finite")
    assert not report, "\n".join(report)


def test_catalog_chunks_of_the_chunked_cases():
    """N_CHUNKED spans three chunks with a ragged last one at the shapes that use it."""
    for HW in (64, 256):
        assert predictive.catalog_chunks(HW, N_CHUNKED) == 3
        assert N_CHUNKED % (4 * -(-N_CHUNKED // 12)) != 0


DET_CASES = [("m71", 8, 8, 10, N_CHUNKED), ("poisson", 16, 16, 10, N_CHUNKED),
             ("m71", 32, 32, 10, 5), ("poisson", 25, 41, 10, 5), ("m71", 8, 8, 65, 5),
             ("m71", 64, 65, 10, 5)]


@pytest.mark.parametrize("kind,H,W,S,N", DET_CASES,
                         ids=[f"{k}-{h}x{w}-S{s}-N{n}" for k, h, w, s, n in DET_CASES])
def test_deterministic_and_moments_independent_of_outputs(kind, H, W, S, N):
    om, locs, fluxes, rate, img = reference(kind, H, W, 8, S, N)
    pm = p_model(kind, H, W, 8)
    w = np.random.default_rng(1).uniform(0.1, 2.0, (T, 1, N)).astype(np.float32)
    for weights in (None, w):
        a = run(pm, locs, fluxes, weights, img)
        junk = torch.full((1 << 22,), float("nan"), device=DEV)   # stir the allocator's blocks
        del junk
        b = run(pm, locs, fluxes, weights, img)
        for name in ("mean", "rate_var", "chi2", "chi2_rep", "flux_rep"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        c = run(pm, locs, fluxes, weights, None)
        assert c.chi2 is None and c.flux_rep is None
        assert torch.equal(a.mean, c.mean) and torch.equal(a.rate_var, c.rate_var)
        # another seed moves the replicates and nothing else
        d = run(pm, locs, fluxes, weights, img, seed=SEED + 1)
        assert torch.equal(a.mean, d.mean) and torch.equal(a.chi2, d.chi2)
        assert not torch.equal(a.flux_rep, d.flux_rep)


# ---- replicate noise ---------------------------------------------------------------
def two_kernel_replicates(pm, rate, seed, offset):
    """smcdet_sample_image on a [T,1,H,W,N] rate array: the draws, float32."""
    rate = rate.contiguous()
    out = torch.empty_like(rate)
    cm = pm._cmodel()
    _hip.check(_hip.lib().smcdet_sample_image(_hip.ref(cm), _hip.ptr(rate), rate.numel(), seed,
                                              offset, _hip.ptr(out), _hip.stream_of(rate)),
               "smcdet_sample_image")
    return out


def noise_var32(pm, kind, lam):
    """v(lam) in float64 from the float32 parameters the kernels hold."""
    if kind == "m71":
        return (float(np.float32(pm.noise_additive))
                + float(np.float32(pm.noise_multiplicative)) * lam)
    return lam


EXACT_SHAPES = [("m71", 8, 8), ("m71", 5, 13), ("m71", 1, 257), ("m71", 25, 41), ("m71", 64, 65),
                ("poisson", 8, 8), ("poisson", 5, 13), ("poisson", 1, 257), ("poisson", 25, 41)]


@pytest.mark.parametrize("kind,H,W", EXACT_SHAPES, ids=[f"{k}-{h}x{w}" for k, h, w in EXACT_SHAPES])
def test_replicate_counters_exact_without_sources(kind, H, W):
    """S = 0: every path's rate is the background bit for bit, so the fused
    replicates are smcdet_sample_image's draws on a constant buffer."""
    N = 5
    pm = p_model(kind, H, W, 8)
    bg = float(np.float32(pm.background))
    locs = np.zeros((T, 1, N, 0, 2), np.float32)
    fluxes = np.zeros((T, 1, N, 0), np.float32)
    img = np.full((T, 1, H, W), bg, np.float32)
    const = torch.full((T, 1, H, W, N), bg, device=DEV, dtype=torch.float32)
    v = noise_var32(pm, kind, bg)
    for seed in (SEED, 7):
        for offset in (0, 2 ** 32 - 5):
            got = run(pm, locs, fluxes, None, img, seed=seed, offset=offset)
            assert (got.mean == bg).all() and (got.rate_var == 0).all()
            x = two_kernel_replicates(pm, const, seed, offset).double()
            flux = npy(x.sum((2, 3)))
            np.testing.assert_allclose(npy(got.flux_rep), flux, rtol=EPS, atol=0,
                                       err_msg=f"seed {seed} offset {offset}")
            if kind == "m71":
                c2 = npy(((x - bg) ** 2 / v).sum((2, 3)))
                np.testing.assert_allclose(npy(got.chi2_rep), c2, rtol=1e-6, atol=0,
                                           err_msg=f"seed {seed} offset {offset}")
    # the draws do depend on the offset and the seed
    a = run(pm, locs, fluxes, None, img, seed=SEED, offset=0).flux_rep
    assert not torch.equal(a, run(pm, locs, fluxes, None, img, seed=SEED, offset=1).flux_rep)


REP_SHAPES = [(8, 8, 5), (16, 16, N_CHUNKED), (32, 32, 5), (25, 41, 5), (64, 65, 5)]


@pytest.mark.parametrize("H,W,N", REP_SHAPES, ids=[f"{h}x{w}-N{n}" for h, w, n in REP_SHAPES])
def test_replicates_with_sources_m71(H, W, N):
    """flux_rep against model.rate -> smcdet_sample_image -> float64 sum.  The
    two routes' rates differ by at most r each way and x_rep = l + sqrt(v(l)) z
    is continuous in l: d x_rep / d log l = l + (x_rep - l) eta l / (2 v) and
    eta l <= v, so |delta| <= r (sum l + 1/2 sum |x_rep - l|)."""
    om, locs, fluxes, _, img = reference("m71", H, W, 8, 10, N)
    pm = p_model("m71", H, W, 8)
    got = run(pm, locs, fluxes, None, img, seed=SEED, offset=11)
    rate = pm.rate(dev(locs), dev(fluxes))
    x = two_kernel_replicates(pm, rate, SEED, 11).double()
    lam = rate.double()
    want = npy(x.sum((2, 3)))
    bound = R_TOL * npy(lam.sum((2, 3)) + 0.5 * (x - lam).abs().sum((2, 3)))
    err = np.abs(npy(got.flux_rep).astype(np.float64) - want) / bound
    print(f"PRED m71 {H}x{W} N={N}: flux_rep err/bound {err.max():.3f}")
    assert err.max() <= 1


def test_replicates_with_sources_poisson_follow_their_law():
    """T N = 12,288 catalogs at 8x8: flux_rep is a sum of independent Poisson
    draws with total mean L = sum_p l, and chi2_rep has mean H W and variance
    sum_p (2 + 1 / l)."""
    H = W = 8
    N = 4096
    pm = p_model("poisson", H, W, 8)
    locs, fluxes = catalog("poisson", H, W, 8, 10, N)
    got = run(pm, locs, fluxes, None, np.full((T, 1, H, W), 200.0, np.float32), seed=SEED)
    lam = pm.rate(dev(locs), dev(fluxes)).double()
    L = npy(lam.sum((2, 3)))
    z_flux = (npy(got.flux_rep).astype(np.float64) - L) / np.sqrt(L)
    rep = NS.normal_report(z_flux)
    rep = {k: rep[k] for k in ("mean", "variance")}
    NS.show("flux_rep", rep)
    assert not NS.failures(rep), NS.failures(rep)
    z_chi = (npy(got.chi2_rep).astype(np.float64) - H * W) / np.sqrt(npy((2 + 1 / lam).sum((2, 3))))
    rep = {"mean": NS.normal_report(z_chi)["mean"]}
    NS.show("chi2_rep", rep)
    assert not NS.failures(rep), NS.failures(rep)


# ---- refusals -----------------------------------------------------------------------
@pytest.mark.parametrize("H,W", M71_ONLY)
def test_refusals_above_the_lds_budget(H, W):
    locs = torch.zeros(T, 1, 2, 65, 2, device=DEV)
    fluxes = torch.ones(T, 1, 2, 65, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-2\)"):     # Poisson above 4096 pixels
        predictive.posterior_image(p_model("poisson", H, W, 8), locs[..., :1, :], fluxes[..., :1])
    with pytest.raises(RuntimeError, match=r"\(-2\).*S=65"):
        predictive.posterior_image(p_model("m71", H, W, 8), locs, fluxes)
    predictive.posterior_image(p_model("m71", H, W, 8), locs[..., :64, :], fluxes[..., :64])


def test_chi2_without_an_image_is_refused():
    pm = p_model("m71", 8, 8, 8)
    cm = pm._cmodel()
    N = 4
    locs, fluxes = torch.zeros(1, N, 1, 2, device=DEV), torch.ones(1, N, 1, device=DEV)
    need = _hip.lib().smcdet_posterior_image_workspace(_hip.ref(cm), 1, N)
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    mean, var = torch.empty(1, 8, 8, device=DEV), torch.empty(1, 8, 8, device=DEV)
    chi2 = torch.empty(1, N, device=DEV)
    rc = _hip.lib().smcdet_posterior_image(
        _hip.ref(cm), None, _hip.ptr(locs), _hip.ptr(fluxes), None, 1, N, 1, 1, 0, _hip.ptr(mean),
        _hip.ptr(var), _hip.ptr(chi2), None, None, _hip.ptr(ws), need, _hip.stream_of(locs))
    assert rc == -1 and b"tiled_image" in _hip.lib().smcdet_last_error()
    # the replicate outputs alone need no image
    rep = torch.empty(1, N, device=DEV)
    rc = _hip.lib().smcdet_posterior_image(
        _hip.ref(cm), None, _hip.ptr(locs), _hip.ptr(fluxes), None, 1, N, 1, 1, 0, _hip.ptr(mean),
        _hip.ptr(var), None, None, _hip.ptr(rep), _hip.ptr(ws), need, _hip.stream_of(locs))
    assert rc == 0
    assert torch.isfinite(rep).all() and torch.isfinite(mean).all()


# ---- end to end ---------------------------------------------------------------------
def test_predictive_sampler_on_a_real_run():
    from smcdet_amd.sampler import SMCsampler
    from tests._params import M71, p_m71_mh, p_m71_model, p_m71_prior
    torch.manual_seed(0)
    H, S, N = 8, 4, 256
    model, prior = p_m71_model(H), p_m71_prior(H, S, S)
    truth = p_m71_prior(2 * H, 0, 100, counts_rate=0.01)
    c, l, f = truth.sample(num_catalogs=1, device=torch.device("cuda", 0))
    img = p_m71_model(2 * H).sample(l, f)[0, 0, :, :, 0]
    s = SMCsampler(img, H, prior, model, p_m71_mh(20), N, 0.5, "systematic",
                   M71["flux_detection_threshold"], 100, print_every=10 ** 9)
    with pytest.raises(ValueError, match="run"):
        predictive.predictive_sampler(s)
    s.run()
    got = predictive.predictive_sampler(s)
    assert got.seed == s.rng.seed
    for name in ("mean", "rate_var", "residual", "z", "pred_var"):
        assert tuple(getattr(got, name).shape) == (2, 2, H, H), name
    for name in ("chi2", "chi2_rep", "flux_rep"):
        assert tuple(getattr(got, name).shape) == (2, 2, N), name
    assert tuple(got.p_value.shape) == tuple(got.p_value_flux.shape) == (2, 2)
    assert ((got.p_value >= 0) & (got.p_value <= 1)).all()
    assert tuple(got.to_image("z").shape) == (2 * H, 2 * H)
    assert torch.equal(got.to_image(got.tiled_image), img)
    # the mean against the existing route (uniform weights after the final resample)
    rate = s.ImageModel.rate(s.locs, s.fluxes)
    want = rate.double().mean(-1)
    assert ((got.mean.double() - want).abs() <= (R_TOL + EPS) * want).all()
    x = two_kernel_replicates(s.ImageModel, rate, s.rng.seed, 0).double()
    lam = rate.double()
    bound = R_TOL * (lam.sum((2, 3)) + 0.5 * (x - lam).abs().sum((2, 3)))
    d = (got.flux_rep.double() - x.sum((2, 3))).abs()
    assert (d <= bound).all()
    # a run on data drawn from the model is not rejected outright
    print("p_value", got.p_value.cpu().tolist(), "p_value_flux", got.p_value_flux.cpu().tolist())
