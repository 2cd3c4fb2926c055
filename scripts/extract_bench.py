"""Times smcdet_extract (smcdet_amd.extract's kernel) on the grid search of the
reference's run_sep.py scripts, the smcdet_match_catalogs launch that scores
it, and the numpy oracle (tests/_extract_oracle.py) on a slice of the same
problems.

    python scripts/extract_bench.py [--out profiles/extract/extract_bench.json]

Shape: --tiles 8x8 tiles x 2,380 settings (17 thresh x 7 minarea x 5
deblend_cont x 4 clean_param), deblend_nthresh 64, K = 16: one launch.  The
kernel is timed alone with the library's launch-timing events (they ride on
the kernel's own dispatch packet), median of --launches launches after
--warmup.  There is no sep on these machines, so the comparison is the oracle
on one host core over --cpu-problems of the same problems (whole tiles x a
stride of the settings), whose results are checked against the kernel's.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, extract  # noqa: E402
from smcdet_amd._hip import check, lib, ptr, stream_of  # noqa: E402
from tests import _extract_oracle as O  # noqa: E402

BG, ETA, SCALE = 104.15, 1.936, 241.03  # M71: background (ADU), noise factor, ADU per nmgy


def make_tiles(T, H, seed=0, density=0.03, max_true=8):
    """M71-like tiles with their truth: Poisson(density * area) sources on the
    tile and a 2-pixel rim, a Gaussian stand-in PSF (sigma 1.2 px), Pareto
    fluxes, Poisson / normal noise with variance ETA * rate.  The true catalog
    keeps the sources inside the tile."""
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:H, 0:H] + 0.5
    images = np.empty((T, H, H), np.float32)
    counts = np.zeros(T, np.int32)
    locs = np.zeros((T, max_true, 2), np.float32)
    fluxes = np.zeros((T, max_true), np.float32)
    for t in range(T):
        rate = np.full((H, H), BG)
        for _ in range(rng.poisson(density * (H + 4) ** 2)):
            h, w = rng.uniform(-2, H + 2, 2)
            f = min(300.0 * (1 - rng.uniform()) ** (-1 / 0.7), 2e5)
            rate += f * np.exp(-((ii - h) ** 2 + (jj - w) ** 2) / (2 * 1.44)) / (2 * np.pi * 1.44)
            if 0 <= h < H and 0 <= w < H and counts[t] < max_true:
                locs[t, counts[t]], fluxes[t, counts[t]] = (h, w), f / SCALE
                counts[t] += 1
        images[t] = rng.poisson(rate) + rng.normal(0, np.sqrt((ETA - 1) * rate))
    return images, counts, locs, fluxes


def timed(launch, launches, warmup):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    _hip.launch_timing(launches)
    for _ in range(launches):
        launch()
    torch.cuda.synchronize()
    ms = _hip.launch_timing_read(launches)
    _hip.launch_timing(0)
    assert len(ms) == launches, ms
    return dict(launches=launches, warmup=warmup, kernel_ms_median=statistics.median(ms),
                kernel_ms_min=min(ms), kernel_ms_max=max(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--tile-dim", type=int, default=8)
    ap.add_argument("--nthresh", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-problems", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join("profiles", "extract", "extract_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extract_bench.py needs a GPU (nothing is timed on the CPU alone)")
    dev = torch.device("cuda", 0)
    T, H, K, n = a.tiles, a.tile_dim, 16, a.nthresh
    grid = (np.arange(1.0, 9.5, 0.5), np.arange(1, 8), np.logspace(-10, -2, 5),
            np.logspace(-1, 2, 4))
    settings = torch.from_numpy(O.settings_grid(*grid))
    G = settings.shape[0]
    images, tc, tl, tf = make_tiles(T, H)
    sigma = float(np.sqrt(ETA * BG))
    d_img = torch.from_numpy(images).to(dev)
    d_bg = torch.full((T,), BG, device=dev)
    d_sigma = torch.full((T,), sigma, device=dev)

    out = {}

    def launch_extract():
        out["r"] = extract._launch(d_img, d_bg, d_sigma, settings, n, K, False)

    ext = timed(launch_extract, a.launches, a.warmup)
    counts, locs, fluxes, n_found, _ = out["r"]
    med = ext["kernel_ms_median"]
    ext.update(T=T, H=H, W=H, G=G, deblend_nthresh=n, K=K, problems=T * G,
               ns_per_problem=1e6 * med / (T * G), problems_per_s=T * G / (med * 1e-3),
               bytes_read=4 * T * H * H, bytes_written=T * G * (8 + 12 * K),
               mean_detections=float(n_found.float().mean()),
               max_detections=int(n_found.max()))
    print("extract", json.dumps(ext), flush=True)

    # the matching that scores the grid: every setting's catalog of every tile
    d_truth = [torch.from_numpy(x).to(dev) for x in (tc, tl, tf)]
    bins = torch.tensor([14.0, 22.0], device=dev)
    St = tl.shape[1]
    est_fluxes = fluxes / SCALE
    mouts = [torch.zeros(T, G, 2, device=dev) for _ in range(4)]

    def launch_match():
        check(lib().smcdet_match_catalogs(
            ptr(d_truth[0]), ptr(d_truth[1]), ptr(d_truth[2]), ptr(counts), ptr(locs),
            ptr(est_fluxes), None, T, G, G, St, K, 0.5, 0.5, ptr(bins), 2, ptr(mouts[0]),
            ptr(mouts[1]), ptr(mouts[2]), ptr(mouts[3]), None, stream_of(locs)),
            "smcdet_match_catalogs")

    match = timed(launch_match, 5, 1)
    tt, tm, et, em = [x.sum(0) for x in mouts]
    precision, recall = (em / et).nan_to_num(0), (tm / tt).nan_to_num(0)
    f1 = ((2 * precision * recall) / (precision + recall)).nan_to_num(0)[:, -1]
    best = int((f1 == f1.max()).nonzero()[0])
    match.update(problems=T * G, best_setting=settings[best].tolist(), best_f1=float(f1[best]),
                 worst_f1=float(f1.min()))
    print("match", json.dumps(match), flush=True)

    # the oracle on whole tiles x a stride of the settings, one core
    torch.set_num_threads(1)
    tiles = max(1, min(T, 10))
    per_tile = max(1, min(G, a.cpu_problems // tiles))
    pick = np.linspace(0, G - 1, per_tile).astype(int)
    t0 = time.perf_counter()
    want = O.extract_grid(images[:tiles], BG, sigma, settings.numpy()[pick], n, K)
    cpu_s = time.perf_counter() - t0
    got = [x[:tiles][:, pick].cpu().numpy() for x in (counts, n_found, locs, fluxes)]
    same = (got[0] == want.counts) & (got[1] == want.n_found)
    for g, w in ((got[2].reshape(tiles, per_tile, -1), want.locs.reshape(tiles, per_tile, -1)),
                 (got[3], want.fluxes)):
        ulp = np.spacing(np.abs(np.nan_to_num(w)))
        same &= ((np.isnan(g) == np.isnan(w)) &
                 (np.abs(np.nan_to_num(g) - np.nan_to_num(w)) <= ulp)).all(-1)
    cpu = dict(problems=tiles * per_tile, seconds=cpu_s, threads=1,
               us_per_problem=1e6 * cpu_s / (tiles * per_tile),
               problems_differing_from_kernel=int((~same).sum()),
               smallest_significance_margin=float(want.sig_margin.min()),
               smallest_clean_margin=float(want.clean_margin.min()),
               note="counts and n_found equal, locs and fluxes within one float32 ulp; random "
                    "data without decision margins, so a differing problem would be a near tie, "
                    "not an error by itself")
    print("cpu_oracle", json.dumps(cpu), flush=True)

    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(), extract=ext,
               match=match, cpu_oracle=cpu,
               speedup_per_problem_vs_cpu_oracle=cpu["us_per_problem"] * 1e3
               / ext["ns_per_problem"],
               counters="none collected")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
