#!/usr/bin/env python
"""Golden vectors for StarPrior (Normal fluxes): runs the REFERENCE smcdet on
the CPU, as make_golden.py does (whose recorder and run_*_recorded helpers it
uses), and writes data-only fixtures under tests/golden/.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_star_golden.py fixtures
    PYTHONDONTWRITEBYTECODE=1 python -O tests/golden/make_star_golden.py mh-padded
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_star_golden.py stats mh 0 32 [PART]
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_star_golden.py stats mala 0 24 [PART]
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_star_golden.py merge mh|mala

Every fixture: ImageModel(psf_radius=8, psf_stdev=1.0, background=300),
StarPrior(flux_mean=1300, flux_stdev=250, pad=2) (experiments/jsm2024), kernel
flux bounds mean +- 5 stdev = [50, 2550].  The reference's truncated-normal
proposal asserts that every current flux lies inside the kernel's bounds
(distributions.py:51), so each run checks that its initial fluxes do.

star_mh_16x16 (counts 1..3 in S = 3 slots) is the one fixture with padded slots.
Their flux is 0, below the bounds, and the reference's assertion looks at every
slot, masked or not: as it stands the reference cannot run this shape.  That
fixture alone is therefore recorded with Python's assertions off (python -O):
the reference's arithmetic is unchanged, its guard is not evaluated.  A padded
slot that is chosen gets a truncated-normal proposal around 0 like any other
and enters the rate image with its new flux; its prior term is masked by the
count.  The float64 oracle has to reproduce every decision of the run before
it is written, as for the other MH fixture.
"""
import contextlib
import glob
import io
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import (Recorder, np32, run_mala_recorded, run_mh_recorded,  # noqa: E402
                         sampler_for, save)
from smcdet.images import ImageModel, generate_images  # noqa: E402
from smcdet.kernel import SingleComponentMALA, SingleComponentMH  # noqa: E402
from smcdet.prior import StarPrior  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests._star import STAR  # noqa: E402  (the parameters the tests rebuild the fixtures' objects from)

MU, SD = STAR["flux_mean"], STAR["flux_stdev"]
FMIN, FMAX = STAR["fluxes_min"], STAR["fluxes_max"]


def star_model(H):
    return ImageModel(image_height=H, image_width=H, psf_radius=STAR["psf_radius"],
                      psf_stdev=STAR["psf_stdev"], background=STAR["background"])


def star_prior(H, smin, smax):
    return StarPrior(min_objects=smin, max_objects=smax, image_height=H, image_width=H,
                     flux_mean=MU, flux_stdev=SD, pad=STAR["pad"])


def star_truth_image(H, seed, smax=3, exactly=None):
    """generate_images() with a StarPrior truth prior (counts 0..smax); with
    `exactly`, the first draw that has that many sources."""
    torch.manual_seed(seed)
    tp = star_prior(H, 0, smax)
    while True:
        res = generate_images(tp, star_model(H), 0.0, 0, H, 1)
        if exactly is None or int(res[0][0]) == exactly:
            return res


def assert_in_bounds(fluxes, counts):
    f, c = np.asarray(fluxes), np.asarray(counts)
    on = np.arange(f.shape[-1]) < c[..., None]
    if not np.all((f[on] >= FMIN) & (f[on] <= FMAX)):  # (not an assert: must hold under -O too)
        raise SystemExit("an initial flux of an active source is outside the kernel's bounds")


def gen_star_prior():
    """log_prob on 64 catalogs of one 16x16 tile, S = 3: counts 0..3, a location
    on loc_high, one below loc_low, an active flux of exactly 0, a negative one."""
    torch.manual_seed(31)
    pr = star_prior(16, 0, 3)
    counts, locs, fluxes = pr.sample(num_tiles_per_side=1, stratify_by_count=True,
                                     num_catalogs_per_count=16)
    locs, fluxes = locs.clone(), fluxes.clone()
    hi, lo = float(pr.loc_prior.high[0]), float(pr.loc_prior.low[0])
    # (particles 16.. have count >= 1, 32.. count >= 2, 48.. count 3)
    locs[0, 0, 20, 0, 0] = hi            # exactly on loc_high -> -inf
    locs[0, 0, 36, 1, 1] = lo - 0.25     # below loc_low -> -inf
    fluxes[0, 0, 24, 0] = 0.0            # an active flux of exactly 0: finite, no substitution
    fluxes[0, 0, 52, 2] = -75.0          # a negative flux
    # (argument validation off for this call: with it on, torch raises for the
    # location below loc_low instead of returning Uniform.log_prob's -inf)
    torch.distributions.Distribution.set_default_validate_args(False)
    try:
        lp = pr.log_prob(counts, locs, fluxes)
    finally:
        torch.distributions.Distribution.set_default_validate_args(True)
    assert np.isneginf(np32(lp)[0, 0, [20, 36]]).all() and np.isfinite(np32(lp)[0, 0, [24, 52]]).all()
    assert sorted(set(np32(counts).ravel().tolist())) == [0.0, 1.0, 2.0, 3.0]
    save("star_prior.npz", counts=np32(counts), locs=np32(locs), fluxes=np32(fluxes),
         logprior=np32(lp))


class AlphaTap:
    """The reference's own log alpha and alpha per decision: the argument of the
    .exp() whose result the kernels clamp to 1 (kernel.py:114, :262), and the
    clamped value the accept uniform is compared with."""

    def __init__(self):
        self.loga, self.alpha, self._last = [], [], None

    def __enter__(self):
        tap = self
        self._exp, self._clamp = torch.Tensor.exp, torch.Tensor.clamp

        def exp(self_):
            tap._last = self_
            return tap._exp(self_)

        def clamp(self_, *a, **k):
            out = tap._clamp(self_, *a, **k)
            if k == {"max": 1} and not a:
                tap.loga.append(tap._last.detach().double().numpy().copy())
                tap.alpha.append(out.detach().numpy().copy())
            return out

        torch.Tensor.exp, torch.Tensor.clamp = exp, clamp
        return self

    def __exit__(self, *exc):
        torch.Tensor.exp, torch.Tensor.clamp = self._exp, self._clamp
        return False

    def into(self, d):
        """Adds ref_loga [K,nt,nt,N] (float32 values), the decisions `accept`
        and the closest decision's |log u - log alpha| to a recorded run."""
        K = d["comp"].shape[0]
        assert len(self.loga) == K
        d["ref_loga"] = np.stack(self.loga)
        d["accept"] = (d["uacc"] <= np.stack(self.alpha)).astype(np.uint8)
        with np.errstate(all="ignore"):
            m = np.abs(np.log(d["uacc"].astype(np.float64)) - np.minimum(d["ref_loga"], 0))
        d["min_margin"] = np.float64(np.where(np.isfinite(m), m, np.inf).min())
        return d


def _mh_fixture(name, image, tile, prior, mh, n_per_count, tau, seeds):
    """The first of `seeds` whose run the float64 oracle reproduces decision by
    decision with |log u - log alpha| >= 1e-4 (the margin of gen_mh_teacher)."""
    from tests._star import decisions_pinned
    for seed in seeds:
        with AlphaTap() as tap:
            d = run_mh_recorded(image, tile, prior, star_model(tile), mh, n_per_count, tau, seed)
        if len(tap.loga) != d["comp"].shape[0]:
            raise SystemExit("log alpha tap out of step with the sweep")
        tap.into(d)
        assert_in_bounds(d["fluxes0"], d["counts"])
        d["seed"] = np.int32(seed)
        if decisions_pinned(d, name, 1e-4):
            save(name + ".npz", **d)
            return
    raise SystemExit(f"{name}: no seed with every decision pinned")


def gen_star_mh_padded():
    # one 16x16 tile, counts 1..3, 10 per count (N = 30: not a multiple of the 4
    # waves of a workgroup; strata with padded slots), K = 20, tau = 0.5
    if not sys.flags.optimize:
        raise SystemExit("star_mh_16x16 has padded slots: run this target with python -O "
                         "(see the module docstring)")
    res = star_truth_image(16, 61)
    mh = SingleComponentMH(20, 0.25, 100, FMIN, FMAX)
    _mh_fixture("star_mh_16x16", res[-1][0], 16, star_prior(16, 1, 3), mh, 10, 0.5,
                range(161, 261))


def gen_star_mh():
    # 2x2 tiles of 8x8 (small tiles: the per-wave PSF cache), S = 2, N = 8, K = 10, tau = 1
    res = star_truth_image(16, 62)
    mh = SingleComponentMH(10, 0.25, 100, FMIN, FMAX)
    _mh_fixture("star_mh_tiles", res[-1][0], 8, star_prior(8, 2, 2), mh, 8, 1.0, range(261, 361))


def run_mala_with_loga(image, seed):
    """run_mala_recorded plus the reference's own log alpha per decision."""
    # steps as mala_basic_16x16 (make_golden.gen_mala): 0.1 / 100
    mala = SingleComponentMALA(20, 0.1, 100, FMIN, FMAX)
    with AlphaTap() as tap:
        d = run_mala_recorded(image, 16, star_prior(16, 3, 3), star_model(16), mala, 32, 0.5, seed)
    return tap.into(d)


def gen_star_mala():
    # 16x16, S = 3, N = 32, K = 20, tau = 0.5; among 20 seeds the one whose
    # closest decision (|log u - log alpha|, the reference's own float32 log
    # alpha) is farthest: the margin is stored, no threshold fixed in advance
    res = star_truth_image(16, 63)
    best = None
    for seed in range(171, 191):
        d = run_mala_with_loga(res[-1][0], seed)
        assert_in_bounds(d["fluxes0"], d["counts"])
        print("mala seed", seed, "min margin %.3e" % d["min_margin"], flush=True)
        if best is None or d["min_margin"] > best["min_margin"]:
            best = dict(d, seed=np.int32(seed))
    print("kept seed", int(best["seed"]), "min margin %.3e" % best["min_margin"])
    save("star_mala_16x16.npz", **best)


def gen_star_stats(kernel, seeds, part=None):
    """The loop of make_golden.gen_stats: one 16x16 truth with exactly 3
    sources, sampler prior min = max = 3, N = 256, systematic, rho = 0.5."""
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "4")))
    res = star_truth_image(16, 64, exactly=3)
    img = res[-1][0]
    pr = star_prior(16, 3, 3)
    if kernel == "mh":
        mk = lambda: SingleComponentMH(50, 0.25, 100, FMIN, FMAX)  # noqa: E731
    else:
        mk = lambda: SingleComponentMALA(25, 0.25, 100, FMIN, FMAX)  # noqa: E731
    which = "star" if kernel == "mh" else "star_mala"
    model, tile, N, method, max_iters = star_model(16), 16, 256, "systematic", 100
    rows = []
    for seed in seeds:
        torch.manual_seed(seed)
        s = sampler_for(img, tile, pr, model, mk(), N, method=method, max_iters=max_iters)
        esses, taus = [], []
        orig_uw = s.update_weights

        def uw(s=s, esses=esses, taus=taus, orig_uw=orig_uw):
            orig_uw()
            esses.append(float(s.ess.flatten()[0]))
            taus.append(float(s.temperature.flatten()[0]))

        s.update_weights = uw
        orig_init = s.initialize

        def init(s=s, orig_init=orig_init):
            orig_init()
            assert_in_bounds(np32(s.fluxes), np32(s.counts))

        s.initialize = init
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            s.run()
        dt = time.perf_counter() - t0
        pc = s.pruned_counts.flatten()
        hist = np.bincount(pc.numpy().astype(np.int64), minlength=pr.max_objects + 1)
        rows.append(dict(seed=seed, logZ=float(s.log_normalizing_constant.flatten()[0]),
                         iters=int(s.iter), ess_trace=esses, tau_trace=taus,
                         final_ess=float(s.ess.flatten()[0]),
                         pruned_hist=(hist / hist.sum()).tolist(),
                         mean_total_flux=float(s.posterior_mean_total_flux(s.fluxes).flatten()[0]),
                         mean_total_flux_pruned=float(
                             s.posterior_mean_total_flux(s.pruned_fluxes).flatten()[0]),
                         runtime_s=dt))
        print(which, seed, rows[-1]["logZ"], rows[-1]["iters"], f"{dt:.1f}s", flush=True)
        cfg = dict(which=which, tile=tile, N=N, S=pr.max_objects, K=mk().num_iters,
                   method=method, counts_rate=None, rho=0.5,
                   torch_threads=torch.get_num_threads(), max_smc_iters=max_iters, kernel=kernel,
                   flux_detection_threshold=float(s.flux_detection_threshold), **STAR,
                   locs_stdev=0.25, fluxes_stdev=100.0,
                   truth_counts=int(res[0][0]), truth_locs=np32(res[1][0]).tolist(),
                   truth_fluxes=np32(res[2][0]).tolist())
        path = os.path.join(HERE, f"stats_{which}.json" if part is None
                            else f"stats_{which}.part{part}.json")
        with open(path, "w") as f:
            json.dump(dict(config=cfg, image=img.numpy().tolist(), runs=rows), f)
    print("wrote", path)


def merge_stats(kernel):
    which = "star" if kernel == "mh" else "star_mala"
    parts = sorted(glob.glob(os.path.join(HERE, f"stats_{which}.part*.json")))
    docs = [json.load(open(p)) for p in parts]
    assert docs and all(d["image"] == docs[0]["image"] and d["config"] == docs[0]["config"]
                        for d in docs)
    runs = sorted((r for d in docs for r in d["runs"]), key=lambda r: r["seed"])
    assert len({r["seed"] for r in runs}) == len(runs)
    with open(os.path.join(HERE, f"stats_{which}.json"), "w") as f:
        json.dump(dict(config=docs[0]["config"], image=docs[0]["image"], runs=runs), f)
    print("merged", len(runs), "runs of", len(parts), "parts")


if __name__ == "__main__":
    torch.set_default_dtype(torch.float32)
    what = sys.argv[1] if len(sys.argv) > 1 else "fixtures"
    if what == "fixtures":
        gen_star_prior()
        gen_star_mh()
        gen_star_mala()
    elif what == "mh-padded":
        gen_star_mh_padded()
    elif what == "stats":
        gen_star_stats(sys.argv[2], range(int(sys.argv[3]), int(sys.argv[4])),
                       part=sys.argv[5] if len(sys.argv) > 5 else None)
    elif what == "merge":
        merge_stats(sys.argv[2])
    else:
        raise SystemExit(f"unknown target {what}")
