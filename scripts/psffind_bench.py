"""Times the PSF-fitting detector (smcdet_amd.psffind) at its grid search's
shape, per launch kind and for a whole find_grid, next to extract_grid +
photometry_of on the same tiles in the same process, and reports the F1 both
tunings reach.

    python scripts/psffind_bench.py [--out profiles/psffind/psffind_bench.json]

Shape: --tiles 8x8 M71 tiles drawn from the prior and the image model
(images.generate_images, stars in a 4-pixel padding included) x 51 settings (17
thresh x 3 nms_radius x 1 min_snr), K = 16, psffind's defaults (2 cells per
pixel, 3 rounds, 4 sweeps, step 0.25, half 2, min_sep 0.5).  The isophotal
baseline runs 51 settings too (the same 17 thresh x 3 minarea).
Every figure is the median of --runs runs with min-max after --warmup.  A
kernel is timed alone with the library's launch-timing events (they ride on
the kernel's own dispatch packet), on the inputs the second round of the loop
gives it; a whole find_grid and extract_grid + photometry_of are timed with
stream events, alternating.  No counters are collected: what bounds the
kernels is worked out from the shapes.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, extract, photometry, psffind  # noqa: E402
from smcdet_amd.images import M71ImageModel, generate_images  # noqa: E402
from smcdet_amd.prior import M71Prior  # noqa: E402
from tests._params import M71  # noqa: E402

TILE, K = 8, 16


def spread(ms):
    return dict(runs=len(ms), ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def kernel_ms(launch):
    _hip.launch_timing(1)
    launch()
    torch.cuda.synchronize()
    ms = _hip.launch_timing_read(1)
    _hip.launch_timing(0)
    assert len(ms) == 1, ms
    return ms[0]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "psffind", "psffind_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("psffind_bench.py needs a GPU (nothing is timed on the CPU alone)")
    p = M71
    T = a.tiles
    torch.manual_seed(0)
    model = M71ImageModel(image_height=TILE, image_width=TILE, background=p["background"],
                          psf_radius=p["psf_radius"], adu_per_nmgy=p["adu_per_nmgy"],
                          psf_params=p["psf_params"], noise_additive=p["noise_additive"],
                          noise_multiplicative=p["noise_multiplicative"])
    truth = M71Prior(min_objects=0, max_objects=30, counts_rate=p["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=p["flux_alpha"],
                     flux_lower=p["flux_detection_threshold"], flux_upper=p["flux_upper"], pad=4)
    res = generate_images(truth, model, p["flux_detection_threshold"], 0, TILE, T)
    tc, tl, tf = res[3].reshape(T), res[4].reshape(T, -1, 2), res[5].reshape(T, -1)
    images = res[-1].reshape(T, TILE, TILE).contiguous()
    cm = model._cmodel()
    bg = float(p["background"])
    sigma = math.sqrt(p["noise_additive"] + p["noise_multiplicative"] * bg)
    thresh = np.arange(3.0, 11.5, 0.5).tolist()
    grid = dict(thresh=thresh, nms_radius=[0, 1, 2], min_snr=[3.0])
    settings = psffind._settings(**grid)
    G = settings.shape[0]
    dev = images.device
    th = settings[:, 0].to(torch.float32).to(dev)
    nms = settings[:, 1].to(torch.int32).to(dev)

    # the state the second round's launches see: the first round's survivors
    first = psffind._run(images, cm, None, settings, 2, 1, 4, 0.25, 2, 0.5, K)
    counts, locs, fluxes = first[:3]
    empty = (torch.zeros_like(counts), torch.full_like(locs, float("nan")),
             torch.zeros_like(fluxes))
    found = psffind._find_launch(images, cm, None, counts, locs, fluxes, G, K, 2, th, nms, 0.5,
                                 False)
    c2, l2 = found[0], found[1]
    f2 = photometry._launch(images, c2, l2, cm, None, 4, False, False).fluxes.to(torch.float32)
    ex_grid = dict(thresh=thresh, minarea=[1, 3, 5])

    kinds = dict(
        find_empty_list=lambda: psffind._find_launch(images, cm, None, *empty, G, K, 2, th, nms,
                                                     0.5, False),
        find_second_round=lambda: psffind._find_launch(images, cm, None, counts, locs, fluxes, G,
                                                       K, 2, th, nms, 0.5, False),
        photometry=lambda: photometry._launch(images, c2, l2, cm, None, 4, False, False),
        recentre=lambda: psffind._recentre_launch(images, cm, None, c2, l2, f2, 2, 0.25))
    whole = dict(
        find_grid=lambda: psffind.find_grid(images, model, max_detections=K, **grid),
        extract_grid_then_photometry_of=lambda: photometry.photometry_of(
            extract.extract_grid(images, bg, sigma, max_detections=K, deblend_nthresh=64,
                                 flux_scale=p["adu_per_nmgy"], **ex_grid), images, model))
    for _ in range(a.warmup):
        for fn in list(kinds.values()) + list(whole.values()):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in list(kinds) + list(whole)}
    for _ in range(a.runs):  # alternating, in one process
        for k, fn in kinds.items():
            ms[k].append(kernel_ms(fn))
        for k, fn in whole.items():
            ms[k].append(event_ms(fn))
    out = dict(device=torch.cuda.get_device_name(0), library=_hip.version(), T=T, H=TILE, W=TILE,
               G=G, K=K, problems=T * G, cells=2, rounds=3, sweeps=4,
               mean_sources_second_round=float(c2.float().mean()),
               launches_per_find_grid=dict(find=3, photometry=15, recentre=12),
               kernels={k: dict(spread(ms[k]),
                                ns_per_problem=1e6 * statistics.median(ms[k]) / (T * G))
                        for k in kinds},
               whole={k: spread(ms[k]) for k in whole}, counters="none collected")
    print(json.dumps(out["kernels"]), flush=True)
    print(json.dumps(out["whole"]), flush=True)

    # the F1 both tunings reach on these tiles (last bin: every true star up to magnitude 22)
    common = dict(locs_tol=0.5, mags_tol=0.5, mag_bins=(14.0, 22.0), max_detections=K)
    t_find = psffind.tune(images, model, tc, tl, tf, **grid, **common)
    t_ext = extract.tune(images, bg, sigma, tc, tl, tf, thresh=np.arange(1.0, 9.5, 0.5).tolist(),
                         minarea=list(range(1, 8)), deblend_cont=np.logspace(-10, -2, 5).tolist(),
                         clean_param=np.logspace(-1, 2, 4).tolist(), deblend_nthresh=64,
                         flux_scale=p["adu_per_nmgy"], flux="psf", image_model=model, **common)
    out["f1"] = dict(true_stars=int(tc.sum()),
                     psffind=dict(best=t_find.best, f1=float(t_find.f1.max()),
                                  f1_min=float(t_find.f1.min()), settings=G),
                     extract_psf_flux=dict(best=t_ext.best, f1=float(t_ext.f1.max()),
                                           f1_min=float(t_ext.f1.min()),
                                           settings=int(t_ext.settings.shape[0])))
    print(json.dumps(out["f1"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
