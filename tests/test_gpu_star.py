"""StarPrior (Normal fluxes, smcdet/prior.py:125-154) on the GPU: the prior
kernels, the MH and MALA sweeps' Normal instantiations against replays of the
reference (tests/golden/star_*.npz, make_star_golden.py), identities between
entry points, and the law of whole SMC runs against the reference's
(stats_star*.json).  Fixture parameters: tests/_star.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests._params import GOLDEN, golden, tiles_of
from tests._star import (STAR, STAR_MH_FIXTURES, p_star_mala, p_star_mh, p_star_mh_fixture_setup,
                         p_star_model, p_star_prior)

pytestmark = pytest.mark.gpu
DEV = "cuda"
MU, SD = STAR["flux_mean"], STAR["flux_stdev"]


def T(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to(DEV, dtype)


def N(t):
    return t.detach().cpu().numpy()


def _replay(d):
    return dict(comp=torch.as_tensor(d["comp"]), uloc=torch.as_tensor(d["uloc"]),
                uflux=torch.as_tensor(d["uflux"]), uacc=torch.as_tensor(d["uacc"]))


# ---- 1. log_prob ---------------------------------------------------------------
def test_log_prob_vs_reference():
    d = golden("star_prior.npz")
    lp = N(p_star_prior(16, 0, 3).log_prob(T(d["counts"]), T(d["locs"]), T(d["fluxes"])))
    ref = d["logprior"]
    ninf = np.isneginf(ref)
    assert ninf.sum() == 2
    assert np.array_equal(np.isneginf(lp), ninf)  # exactly -inf there, finite elsewhere
    np.testing.assert_allclose(lp[~ninf], ref[~ninf], rtol=1e-6, atol=1e-3)


# ---- 2. sample_stratified, replayed uniforms --------------------------------------
def test_prior_sample_replay_normal_flux():
    """Counts 0..3 x 16 on one 16x16 tile (N = 64, S = 3); the flux uniforms hold
    0, 2^-24, 0.5 and 1 - 2^-24 in active slots.  The kernel's convention
    (include/smcdet_hip.h): u is pulled into [2^-25, 1 - 2^-24] before the
    inverse CDF, so u = 0 gives mean - 5.42 sd.  Flux bound: erfinv_fast's
    documented 4e-7 relative error and two float32 roundings (z = sqrt2 erfinv,
    fma(sd, z, mean)): 1e-6 sd max(|z|, 1) + 2^-22 |f|."""
    from scipy.special import erfinv
    pr = p_star_prior(16, 0, 3)
    g = torch.Generator().manual_seed(5)
    uloc = torch.rand(1, 1, 64, 3, 2, generator=g)
    uflux = torch.rand(1, 1, 64, 3, generator=g)
    special = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]
    for i, u in enumerate(special):  # particles 48.. have count 3: every slot active
        uflux[0, 0, 48 + i, i % 3] = u
    c, l, f = pr.sample_stratified(1, 16, device=DEV, uloc=uloc.to(DEV), uflux=uflux.to(DEV))
    counts = np.repeat(np.arange(4.0), 16)[None, None]
    np.testing.assert_array_equal(N(c), counts.astype(np.float32))
    mask = np.arange(3)[None] < counts[..., None]
    lo, hi = -float(STAR["pad"]), 16.0 + STAR["pad"]
    locs = (lo + uloc.double().numpy() * (hi - lo)) * mask[..., None]
    np.testing.assert_allclose(N(l), locs, rtol=0, atol=4e-6)
    assert np.all(N(l)[~mask] == 0) and np.all(N(f)[~mask] == 0)
    fg = N(f).astype(np.float64)
    assert np.isfinite(fg).all()
    uc = np.clip(uflux.double().numpy(), 2.0 ** -25, 1.0 - 2.0 ** -24)
    z = np.sqrt(2.0) * erfinv(2.0 * uc - 1.0)
    f64 = (MU + SD * z) * mask
    bound = 1e-6 * SD * np.maximum(np.abs(z), 1.0) + 2.0 ** -22 * np.abs(fg)
    err = np.abs(fg - f64)
    print("max flux error / bound: %.3f" % (err[mask] / bound[mask]).max())
    assert np.all(err[mask] <= bound[mask]), (err[mask] / bound[mask]).max()
    for i, u in enumerate(special):
        print("u = %.9g -> flux %.4f" % (u, fg[0, 0, 48 + i, i % 3]))
    assert abs(fg[0, 0, 48, 0] - (MU - 5.42 * SD)) < 0.01 * SD   # u = 0
    assert fg[0, 0, 50, 2] == MU                                  # u = 0.5


# ---- 3. sample_stratified, the kernel's own generator ---------------------------
def test_prior_sample_philox_normal_flux():
    from smcdet_amd._rng import PhiloxStream
    pr = p_star_prior(8, 3, 3)
    a = pr.sample_stratified(2, 4096, device=DEV, rng=PhiloxStream(77))
    b = pr.sample_stratified(2, 4096, device=DEV, rng=PhiloxStream(77))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    fl = N(a[2]).astype(np.float64).ravel()
    n = fl.size
    assert n == 49152 and np.isfinite(fl).all()
    # 4 standard errors: sd / sqrt(n) = 1.128 and sd / sqrt(2 n) = 0.797
    assert abs(fl.mean() - MU) <= 4 * SD / np.sqrt(n), fl.mean()
    assert abs(fl.std(ddof=1) - SD) <= 4 * SD / np.sqrt(2 * n), fl.std(ddof=1)
    # strata with padded slots: exactly 0 past each count
    c, l, f = p_star_prior(8, 1, 3).sample_stratified(2, 64, device=DEV, rng=PhiloxStream(78))
    mask = np.arange(3)[None] < N(c)[..., None]
    assert np.all(N(f)[~mask] == 0) and np.all(N(l)[~mask] == 0)
    assert np.all(N(f)[mask] != 0)


# ---- 4. MH replay -------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["incremental", "full"])
@pytest.mark.parametrize("name", sorted(STAR_MH_FIXTURES))
def test_mh_replay_vs_reference(name, full):
    d = golden(name + ".npz")
    td, model, prior, mh = p_star_mh_fixture_setup(name, full_recompute=full)
    t = T(tiles_of(d["image"], td))
    tau = T(np.full(t.shape[:2], float(d["tau"])))
    mh.locs_min, mh.locs_max = torch.tensor(d["locs_min"]), torch.tensor(d["locs_max"])
    l, f, acc = mh.run(t, T(d["counts"]), T(d["locs0"]), T(d["fluxes0"]), tau, prior=prior,
                       image_model=model, replay=_replay(d))
    # (every slot is compared, padded ones included: they keep the fixture's contents)
    np.testing.assert_array_equal(N(acc), d["acc"])
    np.testing.assert_allclose(N(l), d["locs1"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(N(f), d["fluxes1"], rtol=2e-6, atol=1e-3)
    ll = model.loglikelihood(t, l, f)
    if full:
        np.testing.assert_array_equal(N(mh.last_loglik), N(ll))
    else:
        np.testing.assert_allclose(N(mh.last_loglik), N(ll), rtol=2e-6, atol=1e-3)


# ---- 5. MALA replay -----------------------------------------------------------------
def test_mala_replay_vs_reference():
    """star_mala_16x16: of 20 seeds the one whose closest decision is farthest,
    by the reference's own float32 log alpha: min |log u - log alpha| = 1.09e-2
    (stored as `min_margin`).  Gates of test_gpu_mala.py."""
    d = golden("star_mala_16x16.npz")
    assert float(d["min_margin"]) > 1e-2
    model, prior, mala = p_star_model(16), p_star_prior(16, 3, 3), p_star_mala(20, 0.1, 100)
    t = T(tiles_of(d["image"], 16))
    tau = T(np.full(t.shape[:2], float(d["tau"])))
    mala.locs_min, mala.locs_max = torch.tensor(d["locs_min"]), torch.tensor(d["locs_max"])
    l, f, acc = mala.run(t, T(d["counts"]), T(d["locs0"]), T(d["fluxes0"]), tau, prior=prior,
                         image_model=model, replay=_replay(d))
    np.testing.assert_array_equal(N(acc), d["acc"])
    np.testing.assert_allclose(N(l), d["locs1"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(N(f), d["fluxes1"], rtol=1e-4, atol=2e-3)
    ll = model.loglikelihood(t, l, f)
    np.testing.assert_allclose(N(mala.last_loglik), N(ll), rtol=2e-6, atol=1e-3)


# ---- 6. identities between entry points ---------------------------------------------
def _load(which):
    with open(os.path.join(GOLDEN, f"stats_{which}.json")) as f:
        return json.load(f)


def _kernel(cfg):
    mk = p_star_mala if cfg["kernel"] == "mala" else p_star_mh
    return mk(cfg["K"], cfg["locs_stdev"], cfg["fluxes_stdev"])


def _single_run(cfg, image, seed, fused, persist=True):
    from smcdet_amd.sampler import SMCsampler
    torch.manual_seed(seed)
    H, S = cfg["tile"], cfg["S"]
    s = SMCsampler(image, H, p_star_prior(H, S, S), p_star_model(H), _kernel(cfg), cfg["N"],
                   cfg["rho"], cfg["method"], cfg["flux_detection_threshold"],
                   cfg["max_smc_iters"], print_every=10 ** 9, fused=fused,
                   persist_rate_images=persist)
    s.run()
    return s


def test_fused_run_equals_method_by_method_run():
    ref = _load("star")
    image = torch.tensor(ref["image"], dtype=torch.float32, device=DEV)
    a = _single_run(ref["config"], image, 7, fused=True, persist=False)
    b = _single_run(ref["config"], image, 7, fused=False)
    assert a.iter == b.iter
    assert torch.equal(a.log_normalizing_constant, b.log_normalizing_constant)
    assert torch.equal(a.pruned_counts, b.pruned_counts)
    assert float(a.temperature.min()) == 1.0


def test_component_by_count_leaves_padded_slots_untouched():
    from smcdet_amd._rng import PhiloxStream
    name = "star_mh_16x16"
    d = golden(name + ".npz")
    td, model, prior, mh = p_star_mh_fixture_setup(name)
    mh.component_by_count = True
    mh.rng = PhiloxStream(9)
    t = T(tiles_of(d["image"], td))
    tau = T(np.full(t.shape[:2], float(d["tau"])))
    l, f, acc = mh.run(t, T(d["counts"]), T(d["locs0"]), T(d["fluxes0"]), tau, prior=prior,
                       image_model=model)
    mask = np.arange(3)[None] < d["counts"][..., None]
    assert (~mask).sum() == 30  # 10 particles with two padded slots, 10 with one
    np.testing.assert_array_equal(N(f)[~mask], d["fluxes0"][~mask])
    np.testing.assert_array_equal(N(l)[~mask], d["locs0"][~mask])
    assert np.any(N(f)[mask] != d["fluxes0"][mask])  # the sweep did move active sources
    fa = N(f)[mask]
    assert fa.min() >= STAR["fluxes_min"] and fa.max() <= STAR["fluxes_max"]


# ---- 7. law ---------------------------------------------------------------------------
def _se(a, b):
    return np.sqrt(np.var(a, ddof=1) / len(a) + np.var(b, ddof=1) / len(b))


def _batch_runs(cfg, image, B, seed):
    """B independent runs of the configuration as one BatchSMC call; per run
    the summaries of make_star_golden.gen_star_stats."""
    from smcdet_amd.batch import BatchSMC
    H, S, Np = cfg["tile"], cfg["S"], cfg["N"]
    images = image[None].repeat(B, 1, 1).contiguous()
    bs = BatchSMC(images, p_star_prior(H, S, S), p_star_model(H), _kernel(cfg), Np, cfg["rho"],
                  cfg["method"], cfg["flux_detection_threshold"], cfg["max_smc_iters"],
                  stopping="independent", seed=seed, device=DEV)
    s = bs.sampler
    ess_tr, tau_tr = [], []
    orig = s._temper_reweight

    def tr(with_resample, orig=orig):
        orig(with_resample)
        ess_tr.append(N(s.ess).reshape(-1).copy())
        tau_tr.append(N(s.temperature).reshape(-1).copy())

    s._temper_reweight = tr
    bs.run()
    r = bs.results()
    ess_tr, tau_tr = np.array(ess_tr), np.array(tau_tr)
    flux = N(s.posterior_mean_total_flux(s.fluxes)).reshape(-1)
    pc = N(r["pruned_counts"]).astype(np.int64)
    runs = []
    for b in range(B):
        fin = int(np.argmax(tau_tr[:, b] >= 1.0))
        assert tau_tr[fin, b] >= 1.0, "an image did not reach temperature 1"
        hist = np.bincount(pc[b], minlength=S + 1)
        runs.append(dict(logZ=float(r["log_normalizing_constant"][b]),
                         iters=float(r["num_iters"][b]), final_ess=float(r["ess"][b]),
                         inner_ess=ess_tr[:fin, b], mean_total_flux=float(flux[b]),
                         pruned_hist=hist / hist.sum()))
    return runs


def _law(which, B, min_ref):
    ref = _load(which)
    cfg, rr = ref["config"], ref["runs"]
    assert len(rr) >= min_ref
    image = torch.tensor(ref["image"], dtype=torch.float32, device=DEV)
    runs = _batch_runs(cfg, image, B, 1000)
    rho_n = cfg["rho"] * cfg["N"]

    def col(k, rows):
        return np.array([r[k] for r in rows], dtype=np.float64)

    lz, lz_ref = col("logZ", runs), col("logZ", rr)
    fe, fe_ref = col("final_ess", runs), col("final_ess", rr)
    it, it_ref = col("iters", runs), col("iters", rr)
    fl, fl_ref = col("mean_total_flux", runs), col("mean_total_flux", rr)
    H, H_ref = col("pruned_hist", runs), col("pruned_hist", rr)
    se_bins = np.sqrt(H.var(0, ddof=1) / len(H) + H_ref.var(0, ddof=1) / len(H_ref))
    dbin = np.abs(H.mean(0) - H_ref.mean(0))
    print(which, "log Z %.3f ref %.3f se %.3f | final ESS %.2f ref %.2f se %.2f | iters %.2f ref "
          "%.2f se %.3f | flux %.2f ref %.2f se %.2f | hist %s ref %s" % (
              lz.mean(), lz_ref.mean(), _se(lz, lz_ref), fe.mean(), fe_ref.mean(),
              _se(fe, fe_ref), it.mean(), it_ref.mean(), _se(it, it_ref), fl.mean(),
              fl_ref.mean(), _se(fl, fl_ref), H.mean(0).round(4), H_ref.mean(0).round(4)))
    # the gates of test_statistical_parity_vs_reference
    se = _se(lz, lz_ref)
    diff = lz.mean() - lz_ref.mean()
    assert abs(diff) <= 3 * se, (lz.mean(), lz_ref.mean(), se)
    if cfg["kernel"] != "mala":
        assert abs(diff) <= 0.01 * abs(lz_ref.mean()) + 2 * se, (lz.mean(), lz_ref.mean(), se)
    for r in runs:
        np.testing.assert_allclose(r["inner_ess"], rho_n, rtol=0.01)
    assert abs(fe.mean() - fe_ref.mean()) <= 3 * _se(fe, fe_ref), (fe.mean(), fe_ref.mean())
    assert abs(it.mean() - it_ref.mean()) <= max(3 * _se(it, it_ref), 0.5), (it.mean(),
                                                                             it_ref.mean())
    assert abs(fl.mean() - fl_ref.mean()) <= 3 * _se(fl, fl_ref), (fl.mean(), fl_ref.mean())
    assert np.all(dbin <= 3 * se_bins + 0.01), (H.mean(0).round(3), H_ref.mean(0).round(3))
    if se_bins.max() < 0.01:
        assert 0.5 * dbin.sum() <= 0.05, (H.mean(0).round(3), H_ref.mean(0).round(3))


def test_law_mh_vs_reference():
    """256 GPU runs (one BatchSMC call) against the >= 32 reference runs of
    stats_star.json: 16x16, exactly 3 true sources, StarPrior(3, 3),
    SingleComponentMH(50, 0.25, 100, 50, 2550), N = 256, systematic, rho = 0.5."""
    _law("star", 256, 32)


def test_law_mala_vs_reference():
    """128 GPU runs against the >= 24 reference runs of stats_star_mala.json
    (the same with SingleComponentMALA(25, ...))."""
    _law("star_mala", 128, 24)
