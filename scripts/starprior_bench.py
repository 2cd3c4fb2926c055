#!/usr/bin/env python
"""StarPrior (Normal fluxes) against ParetoStarPrior on the jsm2024 tiled shape:
a 32x32 Poisson image in 16 tiles of 8x8, S = 6 (counts 0..6, 200 particles
per count = 1,400 per tile), SingleComponentMH(100, 0.25, 100, 50, 2550),
systematic resampling, rho = 0.5.  The two priors alternate in one process;
per run the wall time of SMCsampler.run() and the durations of its MH-sweep
launches (smcdet_launch_timing).  The flux-prior term is formed once per
proposal batch, not per pixel, so the sweeps should cost the same; the runs'
SMC iteration counts differ with the prior, so the wall time is also given per
iteration.  `fixed_state`: one sweep from the same stratified state (drawn from
the StarPrior, temperature 0.1) with the same Philox draws under either prior
-- the two kernels on equal work, which whole runs are not (the populations
they temper differ with the prior).  One JSON line (medians over --reps runs).

    python scripts/starprior_bench.py [--reps 20] [--out profiles/starprior/starprior_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from smcdet_amd import _hip  # noqa: E402
from smcdet_amd.images import ImageModel  # noqa: E402
from smcdet_amd.kernel import SingleComponentMH  # noqa: E402
from smcdet_amd.prior import ParetoStarPrior, StarPrior  # noqa: E402
from smcdet_amd.sampler import SMCsampler  # noqa: E402

TILE, IMAGE, S, PER_COUNT, K = 8, 32, 6, 200, 100
MEAN, SD = 1300.0, 250.0
FMIN, FMAX = MEAN - 5 * SD, MEAN + 5 * SD
MAX_LAUNCHES = 512


def priors():
    kw = dict(min_objects=0, max_objects=S, image_height=TILE, image_width=TILE, pad=2)
    # a power law over the same flux range: scale at the lower bound's side of
    # the Normal's bulk, alpha so that 1% of its mass lies above the upper bound
    return {"star": StarPrior(flux_mean=MEAN, flux_stdev=SD, **kw),
            "pareto": ParetoStarPrior(flux_scale=800.0, flux_alpha=4.0, **kw)}


def truth_image(dev):
    torch.manual_seed(3)
    model = ImageModel(image_height=IMAGE, image_width=IMAGE, psf_radius=8, psf_stdev=1.0,
                       background=300.0)
    tp = StarPrior(min_objects=0, max_objects=20, image_height=IMAGE, image_width=IMAGE,
                   flux_mean=MEAN, flux_stdev=SD, pad=2)
    _, l, f = tp.sample(num_catalogs=1, device=dev)
    return model.sample(l, f)[0, 0, :, :, 0]


def one_run(image, prior, seed):
    model = ImageModel(image_height=TILE, image_width=TILE, psf_radius=8, psf_stdev=1.0,
                       background=300.0)
    mh = SingleComponentMH(K, 0.25, 100.0, FMIN, FMAX)
    torch.manual_seed(seed)
    s = SMCsampler(image, TILE, prior, model, mh, PER_COUNT, 0.5, "systematic", 0.0, 100,
                   print_every=10 ** 9)
    _hip.launch_timing(MAX_LAUNCHES)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    sweeps = _hip.launch_timing_read(MAX_LAUNCHES)
    _hip.launch_timing(0)
    assert float(s.temperature.min()) == 1.0
    return dict(wall_ms=1e3 * wall, iters=int(s.iter), sweep_ms=statistics.median(sweeps),
                sweeps=len(sweeps), wall_ms_per_iter=1e3 * wall / max(int(s.iter), 1))


def fixed_state(image, pri, reps):
    """Median launch time of one sweep from the same state and draws, per prior."""
    from smcdet_amd._rng import PhiloxStream
    nt = IMAGE // TILE
    tiled = image.unfold(0, TILE, TILE).unfold(1, TILE, TILE).contiguous()
    model = ImageModel(image_height=TILE, image_width=TILE, psf_radius=8, psf_stdev=1.0,
                       background=300.0)
    counts, locs, fluxes = pri["star"].sample_stratified(nt, PER_COUNT, device=image.device,
                                                         rng=PhiloxStream(11))
    tau = torch.full((nt, nt), 0.1, device=image.device)
    ms = {k: [] for k in pri}
    for rep_ in range(reps + 1):
        for name in pri:
            mh = SingleComponentMH(K, 0.25, 100.0, FMIN, FMAX)
            mh.rng = PhiloxStream(5)
            _hip.launch_timing(4)
            mh.run(tiled, counts, locs, fluxes, tau, prior=pri[name], image_model=model)
            torch.cuda.synchronize()
            t = _hip.launch_timing_read(4)
            _hip.launch_timing(0)
            if rep_:  # (the first pair warms up)
                ms[name].append(t[0])
    return {k: dict(sweep_ms=statistics.median(v), sweep_ms_range=[min(v), max(v)])
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    image = truth_image(dev)
    pri = priors()
    rows = {k: [] for k in pri}
    with open(os.devnull, "w") as null:
        for rep in range(-1, a.reps):  # (pair -1 warms up: kernel load, allocator)
            for name in pri:  # alternating
                out, sys.stdout = sys.stdout, null
                try:
                    r = one_run(image, pri[name], 100 + rep)
                finally:
                    sys.stdout = out
                if rep >= 0:
                    rows[name].append(r)
    res = {"shape": dict(image=IMAGE, tile=TILE, tiles=(IMAGE // TILE) ** 2, S=S,
                         particles_per_tile=(S + 1) * PER_COUNT, K=K, reps=a.reps),
           "library": _hip.version()}
    for name, rr in rows.items():
        res[name] = {k: statistics.median(r[k] for r in rr)
                     for k in ("sweep_ms", "wall_ms", "wall_ms_per_iter", "iters")}
        res[name]["sweep_ms_range"] = [min(r["sweep_ms"] for r in rr),
                                       max(r["sweep_ms"] for r in rr)]
    res["star_vs_pareto_sweep"] = res["star"]["sweep_ms"] / res["pareto"]["sweep_ms"]
    res["fixed_state"] = fixed_state(image, pri, a.reps)
    res["fixed_state"]["star_vs_pareto_sweep"] = (res["fixed_state"]["star"]["sweep_ms"]
                                                  / res["fixed_state"]["pareto"]["sweep_ms"])
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
