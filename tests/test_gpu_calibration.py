"""smcdet_amd.calibration on the GPU against the numpy float64 oracle
(tests/_calibration_oracle.py): the three kernels at the sizes where their
paths change, then the notebook quantities on one synthetic posterior.

Tolerances: counts, masses of exact weights, min / max and
"lower" quantiles are exact; a "linear" quantile is one rounding to float32
plus the float64 lerp's own error; float64 moments differ from the oracle's by
their summation order only."""
import numpy as np
import pytest
import torch

from smcdet_amd import calibration, condense
from tests import _calibration_oracle as O

pytestmark = pytest.mark.gpu

SUMMARY_N = (1, 2, 63, 64, 65, 257, 1000, 1024, 1025, 10000, 16384)


def cuda(*xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def rows_of(N):
    """40 rows at the small N; at the large N three: ties, +-0 / +-inf, NaNs."""
    return O.summary_case(N, 40) if N < 10000 else O.summary_case(N, 5)[1:4]


def run_summary(values, weights=None, q=(), interpolation="linear", thresholds=None, dim=-1):
    v, w, th = cuda(values, weights, thresholds)
    s = calibration.row_summary(v, dim=dim, weights=w, quantiles=q, interpolation=interpolation,
                                thresholds=th)
    return s, {k: getattr(s, k).cpu().numpy() for k in
               ("n_valid", "weight", "mean", "var", "vmin", "vmax", "quantiles")} | \
        {k: None if getattr(s, k) is None else getattr(s, k).cpu().numpy()
         for k in ("below", "at_or_below")}


def same_or_within(got, want, bound, name):
    """Non-finite wanted values must be reproduced as they are; the rest lie
    within the bound."""
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=name)
    err = np.abs(got[fin] - want[fin])
    assert (err <= bound[fin]).all(), (name, err.max(), bound[fin][err.argmax()])


# ---- catalog_totals -----------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 5, 64])
@pytest.mark.parametrize("C", [1, 3])
def test_catalog_totals(S, C):
    counts, fluxes = O.totals_case(3, 257, S)
    cuts = O.TOTALS_CUTS[C]
    past = np.arange(S)[None, None, :] >= counts[..., None]
    assert (counts == 0).any() and (counts == S).any()
    if S > 1:
        assert np.isnan(fluxes[past]).any() and np.isinf(fluxes[past]).any()
        assert fluxes[0, 1, 0] == 5.0 and counts[0, 1] == S  # a counted flux equal to a cut
    want_n, want_f = O.catalog_totals(counts, fluxes, cuts)
    c, f = cuda(counts, fluxes)
    got = calibration.catalog_totals(c, f, cuts)
    assert tuple(got.n_above.shape) == tuple(got.flux_above.shape) == (C, 3, 257)
    np.testing.assert_array_equal(got.n_above.cpu().numpy(), want_n)
    gf = got.flux_above.cpu().numpy()
    w32 = O.f32(want_f)
    ulp = np.spacing(np.abs(w32))
    print(f"flux_above S={S} C={C}: {(gf != w32).sum()} of {gf.size} entries differ from the "
          "rounded float64 oracle")
    assert (np.abs(gf.astype(np.float64) - want_f) <= ulp).all()
    # float counts (the samplers' dtype) are taken too
    got2 = calibration.catalog_totals(c.float(), f, cuts)
    assert torch.equal(got2.n_above, got.n_above) and torch.equal(got2.flux_above, got.flux_above)


# ---- row_summary ----------------------------------------------------------------------
@pytest.mark.parametrize("N", SUMMARY_N)
def test_row_summary_unweighted_linear(N):
    v = rows_of(N)
    th = O.thresholds_case(v)
    want = O.row_summary(v, None, O.Q_LEVELS, "linear", th)
    assert len(O.Q_LEVELS) == 19 * 2 + 2
    _, got = run_summary(v, None, O.Q_LEVELS, "linear", th)
    for k in ("n_valid", "below", "at_or_below", "weight"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("vmin", "vmax"):  # by value: -0 == +0, NaN where the row is empty
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    tol = O.quantile_tolerance(want["quantiles"], want["v_lo"], want["v_hi"])
    same_or_within(got["quantiles"].astype(np.float64), want["quantiles"], tol, "quantiles")
    n, W = want["n_valid"].astype(np.float64), np.maximum(want["weight"], 1.0)
    same_or_within(got["mean"], want["mean"], n * 2.0 ** -53 * want["abs_sum"] / W, "mean")
    same_or_within(got["var"], want["var"], n * 2.0 ** -53 * want["abs_dev_sum"] / W, "var")


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N", SUMMARY_N)
def test_row_summary_lower(N, weighted):
    v = rows_of(N)
    rng = np.random.default_rng(N + 5)
    w = O.dyadic_weights(rng, v.shape) if weighted else None
    if weighted:
        assert (w == 0).any() or N < 8
    q = (0.0, 1.0) + O.Q_LEVELS[1:-1]
    th = O.thresholds_case(v)
    want = O.row_summary(v, w, q, "lower", th)
    _, got = run_summary(v, w, q, "lower", th)
    for k in ("n_valid", "weight", "below", "at_or_below", "vmin", "vmax"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["quantiles"], O.f32(want["quantiles"]))
    # q = 0 is the minimum, q = 1 the largest value that carries weight
    has = want["weight"] > 0
    np.testing.assert_array_equal(got["quantiles"][has, 0], got["vmin"][has])
    assert np.isnan(got["quantiles"][~has]).all()


@pytest.mark.parametrize("B", [1, 3, 17])
def test_row_summary_strided_layout_gives_the_same_bits(B):
    A, N = 2, 257
    flat = O.summary_case(N, A * B, seed=B)  # row a * B + b
    x = np.ascontiguousarray(flat.reshape(A, B, N).transpose(0, 2, 1))  # [A,N,B]
    th = O.thresholds_case(flat)
    w = O.dyadic_weights(np.random.default_rng(B), (A, N))
    for weights, interp in ((None, "linear"), (w, "lower")):
        wf = None if weights is None else np.repeat(weights, B, axis=0)
        s3, _ = run_summary(x, weights, O.Q_LEVELS, interp, th.reshape(A, B, -1), dim=1)
        s2, _ = run_summary(flat, wf, O.Q_LEVELS, interp, th)
        for k in ("n_valid", "weight", "mean", "var", "vmin", "vmax", "quantiles", "below",
                  "at_or_below"):
            a, b = getattr(s3, k), getattr(s2, k)
            assert tuple(a.shape[:2]) == (A, B), k
            # the same bits (NaN included): compare the integer views
            a = a.reshape(b.shape).contiguous()
            bits = torch.int32 if a.element_size() == 4 else torch.int64
            assert torch.equal(a.view(bits), b.view(bits)), (k, interp)


@pytest.mark.parametrize("weighted", [False, True])
def test_row_summary_lower_equals_condense_flux_quantiles(weighted):
    T, N, K = 2, 257, 5
    rng = np.random.default_rng(11)
    mf = rng.uniform(1, 30, (T, N, K)).astype(np.float32)
    mf[rng.uniform(size=mf.shape) < 0.4] = np.nan
    mf[1, :, 2] = np.nan  # a seed nothing matched
    mf[0, 3, 0] = mf[0, 4, 0]
    w = O.dyadic_weights(rng, (T, N)) if weighted else None
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    x, wd = cuda(mf, w)
    want = condense.flux_quantiles(x, qs, wd)
    got = calibration.row_summary(x, dim=1, weights=wd, quantiles=qs, interpolation="lower")
    assert tuple(got.quantiles.shape) == (T, K, len(qs))
    assert torch.equal(got.quantiles.isnan(), want.isnan()) and want.isnan().any()
    assert torch.equal(got.quantiles.nan_to_num(-1.0), want.nan_to_num(-1.0))


def test_row_summary_is_deterministic():
    v = rows_of(10000)
    w = O.dyadic_weights(np.random.default_rng(3), v.shape) * np.float32(1.0 / 3.0)  # inexact sums
    th = O.thresholds_case(v)
    a, _ = run_summary(v, w, O.Q_LEVELS, "lower", th)
    b, _ = run_summary(v, w, O.Q_LEVELS, "lower", th)
    for k in ("n_valid", "weight", "mean", "var", "vmin", "vmax", "quantiles", "below",
              "at_or_below"):
        x, y = getattr(a, k), getattr(b, k)
        bits = torch.int32 if x.element_size() == 4 else torch.int64
        assert torch.equal(x.view(bits), y.view(bits)), k


def test_row_summary_refusals():
    v = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError, match="lower"):
        calibration.row_summary(v, weights=torch.ones(2, 8, device="cuda"), quantiles=(0.5,))
    with pytest.raises(ValueError, match="16384"):
        calibration.row_summary(torch.zeros(1, 16385, device="cuda"))
    with pytest.raises(ValueError, match="64"):
        calibration.row_summary(v, quantiles=tuple(np.linspace(0, 1, 65)))
    with pytest.raises(ValueError, match="65"):
        calibration.row_summary(v, thresholds=torch.zeros(2, 66, device="cuda"))
    with pytest.raises(ValueError, match="dim"):
        calibration.row_summary(torch.zeros(2, 8, 3, device="cuda"), dim=-1)


# ---- bootstrap_means ---------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 7, 257])
@pytest.mark.parametrize("D", [1, 51, 64, 65, 256])
def test_bootstrap_means_replays_indices(M, D):
    Bn = 33
    rng = np.random.default_rng(M * 1000 + D)
    values = (rng.integers(0, 1025, (M, D)) / 1024.0).astype(np.float32)
    idx = rng.integers(0, M, (Bn, M))
    v, i = cuda(values, idx)
    got = calibration.bootstrap_means(v, Bn, indices=i)
    np.testing.assert_array_equal(got.cpu().numpy(), O.f32(O.bootstrap_means(values, idx)))
    with pytest.raises(ValueError, match="lie in"):
        calibration.bootstrap_means(v, Bn, indices=i + M)


def test_bootstrap_means_philox_draws():
    from scipy import stats
    M = D = 64
    Bn = 4096
    v = torch.eye(M, device="cuda")
    got = calibration.bootstrap_means(v, Bn, seed=20250)
    counts = got.double().cpu().numpy() * M  # multinomial counts per replicate
    assert (counts == np.round(counts)).all() and (counts.sum(1) == M).all()
    # the draws are those of the documented formula
    np.testing.assert_array_equal(
        counts, np.stack([np.bincount(r, minlength=M) for r in O.boot_indices(20250, Bn, M)]))
    pooled = counts.sum(0)
    expect = Bn * M / D
    chi2 = ((pooled - expect) ** 2 / expect).sum()
    bound = stats.chi2.ppf(1.0 - 1e-6, D - 1)
    print(f"pooled chi-square {chi2:.2f} (63 degrees of freedom), bound {bound:.2f}")
    assert chi2 < bound
    assert torch.equal(calibration.bootstrap_means(v, Bn, seed=20250), got)
    assert not torch.equal(calibration.bootstrap_means(v, Bn, seed=20251), got)
    # seed None follows torch's generator
    torch.manual_seed(5)
    a = calibration.bootstrap_means(v, 8)
    torch.manual_seed(5)
    assert torch.equal(calibration.bootstrap_means(v, 8), a)


# ---- the notebook quantities on one synthetic posterior -----------------------------------
@pytest.fixture(scope="module")
def posterior():
    case = O.posterior_case()
    dev = dict(zip(case, cuda(*case.values())))
    return case, dev, {cut: O.calibrate(case, cut) for cut in (0.0, 10.0)}


@pytest.mark.parametrize("cut", [0.0, 10.0])
def test_calibrate_against_the_oracle(posterior, cut):
    case, dev, wants = posterior
    want = wants[cut]
    cov = want["coverage"]
    # on the oracle alone: no truth within the quantile tolerance of an interval end
    s = cov["exact"]
    tol = O.quantile_tolerance(s["quantiles"], s["v_lo"], s["v_hi"])
    assert (cov["margin"] > tol).all()

    got = calibration.calibrate(dev["true_counts"], dev["true_fluxes"], dev["est_counts"],
                                dev["est_fluxes"], flux_cut=cut)
    np.testing.assert_array_equal(got.totals.n_above.cpu().numpy(), want["n_above"])
    np.testing.assert_array_equal(got.true_n_above.cpu().numpy(), want["true_n"])
    g = got.coverage
    assert g.levels == O.DEFAULT_LEVELS and tuple(g.covered.shape) == (12, 19)
    # the totals may differ from the oracle's rounded ones by an ulp; the
    # intervals are compared through the oracle run on the device's own totals
    fa = got.totals.flux_above[0].cpu().numpy()
    assert (np.abs(fa.astype(np.float64) - want["flux_above"][0])
            <= np.spacing(np.abs(O.f32(want["flux_above"][0])))).all()
    own = O.coverage(fa, got.true_flux_above.cpu().numpy(), O.DEFAULT_LEVELS,
                     case["true_counts"] > 0)
    so = own["exact"]
    L = 19
    tol = O.quantile_tolerance(so["quantiles"], so["v_lo"], so["v_hi"])
    q = torch.cat([g.lo, g.hi], -1).double().cpu().numpy()
    assert (np.abs(q - so["quantiles"]) <= tol).all()
    np.testing.assert_array_equal(g.covered.cpu().numpy(), cov["covered"])  # every entry
    np.testing.assert_array_equal(g.rate.cpu().numpy(), cov["rate"])
    np.testing.assert_array_equal(g.sbc_rank.cpu().numpy(), own["sbc_rank"])
    np.testing.assert_array_equal(g.pit.cpu().numpy(), own["pit"])
    assert g.sbc_rank.dtype == torch.int64 and tuple(g.lo.shape) == (12, L)
    # cell 44: (truth <= samples).mean()
    np.testing.assert_allclose(
        g.pit.cpu().numpy(),
        (got.true_flux_above.cpu().numpy()[:, None] <= fa).mean(-1), rtol=0, atol=1e-15)

    p = got.count_posterior
    N = case["est_counts"].shape[1]
    np.testing.assert_array_equal(p.mass.cpu().numpy(), want["post"]["mass"])
    np.testing.assert_array_equal(p.pmf.cpu().numpy() * N, want["post"]["pmf"] * N)
    np.testing.assert_array_equal(np.round(p.pmf.cpu().numpy() * N), want["post"]["mass"])
    np.testing.assert_array_equal(p.mode.cpu().numpy(), want["post"]["mode"])
    np.testing.assert_array_equal(got.confusion_samples.cpu().numpy(), want["confusion_samples"])
    np.testing.assert_array_equal(got.confusion_mode.cpu().numpy(), want["confusion_mode"])
    assert got.confusion_samples.sum() == 12 * N and got.confusion_mode.sum() == 12
    assert tuple(got.confusion_mode.shape) == (want["max_count"] + 1, want["max_true"] + 1)


def test_calibrate_weighted(posterior):
    case, dev, _ = posterior
    w = O.dyadic_weights(np.random.default_rng(4), case["est_counts"].shape)
    want = O.calibrate(case, 0.0, weights=w)
    got = calibration.calibrate(dev["true_counts"], dev["true_fluxes"], dev["est_counts"],
                                dev["est_fluxes"], weights=cuda(w)[0])
    fa = got.totals.flux_above[0].cpu().numpy()
    own = O.coverage(fa, got.true_flux_above.cpu().numpy(), O.DEFAULT_LEVELS,
                     case["true_counts"] > 0, w)
    g = got.coverage
    np.testing.assert_array_equal(g.lo.cpu().numpy(), own["lo"])  # "lower": exact
    np.testing.assert_array_equal(g.hi.cpu().numpy(), own["hi"])
    np.testing.assert_array_equal(g.covered.cpu().numpy(), own["covered"])
    np.testing.assert_array_equal(g.pit.cpu().numpy(), own["pit"])
    np.testing.assert_array_equal(g.sbc_rank.cpu().numpy(), own["sbc_rank"])
    np.testing.assert_array_equal(got.count_posterior.mass.cpu().numpy(), want["post"]["mass"])
    np.testing.assert_array_equal(got.count_posterior.pmf.cpu().numpy(), want["post"]["pmf"])
    np.testing.assert_array_equal(got.count_posterior.mode.cpu().numpy(), want["post"]["mode"])
    np.testing.assert_array_equal(got.confusion_samples.cpu().numpy(), want["confusion_samples"])


def test_count_posterior_mode_ties_go_to_the_lower_count():
    n = torch.tensor([[2, 1, 1, 2, 0, 5], [3, 3, 3, 0, 0, 0]], dtype=torch.int32, device="cuda")
    p = calibration.count_posterior(n, 3)
    assert p.mode.tolist() == [1, 0]
    assert p.mass.tolist() == [[1.0, 2.0, 2.0, 0.0], [3.0, 0.0, 0.0, 3.0]]  # the 5 is in no bin
    assert p.pmf[0].sum().item() == pytest.approx(5.0 / 6.0)


def test_credible_intervals(posterior):
    case, dev, _ = posterior
    x = dev["est_total"]  # [T,N,4]: intervals along dim 1
    lo, hi = calibration.credible_intervals(x, (0.5, 0.9), dim=1)
    assert tuple(lo.shape) == tuple(hi.shape) == (12, 4, 2)
    rows = case["est_total"].transpose(0, 2, 1).reshape(48, -1)
    s = O.row_summary(rows, None, O.interval_q((0.5, 0.9)), "linear")
    got = torch.cat([lo, hi], -1).reshape(48, 4).double().cpu().numpy()
    tol = O.quantile_tolerance(s["quantiles"], s["v_lo"], s["v_hi"])
    assert (np.abs(got - s["quantiles"]) <= tol).all()


def test_luminosity_function(posterior):
    case, dev, _ = posterior
    got = calibration.luminosity_function(dev["est_total"])
    assert tuple(got.shape) == (4, 3)
    tot = O.f32(case["est_total"].astype(np.float64).sum(0)).T  # [Bins,N]
    s = O.row_summary(tot, None, (0.05, 0.5, 0.95), "linear")
    np.testing.assert_array_equal(s["quantiles"], O.luminosity_function(case["est_total"]))
    tol = O.quantile_tolerance(s["quantiles"], s["v_lo"], s["v_hi"])
    assert (np.abs(got.double().cpu().numpy() - s["quantiles"]) <= tol).all()
    with pytest.raises(ValueError, match="integers"):
        calibration.luminosity_function(dev["est_total"] + 0.1)


def test_bootstrap_ci_with_injected_indices(posterior):
    case, dev, _ = posterior
    rows = case["rows"]  # [N,6] metric rows
    M, Bn = rows.shape[0], 200
    idx = np.random.default_rng(9).integers(0, M, (Bn, M))
    lo, mean, hi, s = O.bootstrap_ci(rows, idx, alpha=0.1, num_comparisons=6)
    glo, gmean, ghi = calibration.bootstrap_ci(dev["rows"], Bn, alpha=0.1, num_comparisons=6,
                                               indices=cuda(idx)[0])
    tol = O.quantile_tolerance(s["quantiles"], s["v_lo"], s["v_hi"])
    got = torch.stack([glo, ghi], -1).double().cpu().numpy()
    assert (np.abs(got - s["quantiles"]) <= tol).all()
    np.testing.assert_allclose(gmean.cpu().numpy(), mean, rtol=2.0 ** -23, atol=0)
    assert (glo < gmean).all() and (gmean < ghi).all()
    # with a seed: the band of the documented draws
    slo, smean, shi = calibration.bootstrap_ci(dev["rows"], Bn, alpha=0.1, num_comparisons=6,
                                               seed=77)
    wlo, wmean, whi, s = O.bootstrap_ci(rows, O.boot_indices(77, Bn, M), 0.1, 6)
    tol = O.quantile_tolerance(s["quantiles"], s["v_lo"], s["v_hi"])
    got = torch.stack([slo, shi], -1).double().cpu().numpy()
    assert (np.abs(got - s["quantiles"]) <= tol).all()


# ---- end to end -----------------------------------------------------------------------------
def test_calibrate_sampler_on_a_real_run():
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
    true_counts = torch.tensor([[1, 0], [2, 1]], device="cuda")
    true_fluxes = torch.tensor([[[900.0, 0.0], [0.0, 0.0]], [[500.0, 1200.0], [2000.0, 0.0]]],
                               device="cuda")
    with pytest.raises(RuntimeError, match="run the sampler"):
        calibration.calibrate_sampler(s, true_counts, true_fluxes)
    s.run()
    got = calibration.calibrate_sampler(s, true_counts, true_fluxes, flux_cut=100.0)
    Sp = s.pruned_fluxes.shape[-1]
    want = calibration.calibrate(true_counts.reshape(4), true_fluxes.reshape(4, 2),
                                 s.pruned_counts.reshape(4, N),
                                 s.pruned_fluxes.reshape(4, N, Sp).contiguous(), flux_cut=100.0)
    assert tuple(got.totals.n_above.shape) == (1, 4, N)
    for a, b in ((got.totals.n_above, want.totals.n_above),
                 (got.totals.flux_above, want.totals.flux_above),
                 (got.coverage.lo, want.coverage.lo), (got.coverage.hi, want.coverage.hi),
                 (got.coverage.covered, want.coverage.covered),
                 (got.coverage.sbc_rank, want.coverage.sbc_rank),
                 (got.count_posterior.mass, want.count_posterior.mass),
                 (got.count_posterior.mode, want.count_posterior.mode),
                 (got.confusion_samples, want.confusion_samples),
                 (got.confusion_mode, want.confusion_mode)):
        assert torch.equal(a, b)
    assert got.true_n_above.tolist() == [1, 0, 2, 1]
    assert float(got.confusion_samples.sum()) == 4 * N
    # the kernel's counts are the notebook's expression on the pruned fluxes
    pf = s.pruned_fluxes.reshape(4, N, Sp)
    inside = torch.arange(Sp, device="cuda") < s.pruned_counts.reshape(4, N, 1)
    assert torch.equal(got.totals.n_above[0].long(), (inside & (pf >= 100.0)).sum(-1))
