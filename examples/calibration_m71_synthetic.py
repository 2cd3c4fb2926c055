"""Is the posterior calibrated?  The checks of the reference's results notebook
(experiments/m71synthetic/results/results.ipynb: count confusion matrices,
coverage of the total flux, bootstrap bands of F1) on a few synthetic 8x8 M71
tiles with a known truth, every quantity from all posterior catalogs on the
device (smcdet.calibration).

    python examples/calibration_m71_synthetic.py [num_tiles] [num_catalogs]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.calibration import bootstrap_ci, calibrate_sampler  # noqa: E402
from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.kernel import SingleComponentMH  # noqa: E402
from smcdet.metrics import convert_mag_to_nmgy, match_catalogs  # noqa: E402
from smcdet.prior import M71Prior  # noqa: E402
from smcdet.sampler import SMCsampler  # noqa: E402

# notebooks/smc.ipynb cell 2 (full-precision PSF parameters)
params = dict(flux_alpha=0.21411753249015655, flux_lower=0.06291294097900389,
              flux_upper=1804.6791992187502, flux_detection_threshold=0.25165176391601557,
              counts_rate=0.030264640226960182, background=104.1486587524414,
              adu_per_nmgy=241.02658081054688,
              psf_params=[1.107237458229065, 2.0800251960754395, 2.3254318237304688,
                          5.240590572357178, 0.7346734404563904, 0.5114791393280029],
              psf_radius=8, noise_additive=1.0000007072408224e-10,
              noise_multiplicative=1.936462640762329)
TILE = 8


def show(title, m):
    print(f"\n{title} (rows: estimated count, columns: true count)")
    print("      " + " ".join(f"{c:7d}" for c in range(m.shape[1])))
    for k in range(m.shape[0]):
        print(f"{k:5d} " + " ".join(f"{int(v):7d}" for v in m[k].tolist()))


def main():
    num_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    num_catalogs = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    torch.manual_seed(0)
    model = M71ImageModel(image_height=TILE, image_width=TILE, background=params["background"],
                          psf_radius=params["psf_radius"], adu_per_nmgy=params["adu_per_nmgy"],
                          psf_params=params["psf_params"],
                          noise_additive=params["noise_additive"],
                          noise_multiplicative=params["noise_multiplicative"])
    truth = M71Prior(min_objects=0, max_objects=30, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_detection_threshold"],
                     flux_upper=params["flux_upper"], pad=4)
    res = generate_images(truth, model, params["flux_detection_threshold"], 0, TILE, num_tiles)
    true_counts, true_locs, true_fluxes, images = res[3], res[4], res[5], res[-1]
    true_counts = true_counts.reshape(num_tiles)
    true_locs = true_locs.reshape(num_tiles, -1, 2)
    true_fluxes = true_fluxes.reshape(num_tiles, -1)
    print("true detectable counts per tile:", true_counts.tolist())

    prior = M71Prior(min_objects=10, max_objects=10, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_lower"], flux_upper=params["flux_upper"], pad=4)
    mh = SingleComponentMH(100, 0.1, 2.5, params["flux_lower"], params["flux_upper"])
    sampler = SMCsampler.from_tiles(
        images.reshape(1, num_tiles, TILE, TILE), prior, model, mh, num_catalogs, 0.5,
        "multinomial", params["flux_detection_threshold"], 100, print_every=10 ** 9)
    sampler.run()

    # counts above magnitude 24 (the notebook's cut), total flux of all kept sources
    cal = calibrate_sampler(sampler, true_counts, true_fluxes)
    cut = float(convert_mag_to_nmgy(torch.tensor(24.0)))
    counts = calibrate_sampler(sampler, true_counts, true_fluxes, flux_cut=cut)
    N = sampler.pruned_counts.shape[-1]
    print(f"\ncalibrated {num_tiles} tiles x {N} catalogs")
    for level, rate in zip(cal.coverage.levels, cal.coverage.rate.tolist()):
        print(f"nominal coverage probability = {round(level, 2)}, "
              f"empirical coverage probability = {round(rate, 2)}")
    lo, hi = cal.coverage.lo[:, 17], cal.coverage.hi[:, 17]
    print("\n90% intervals of the total flux (tiles with a true source):")
    for t in range(num_tiles):
        if int(true_counts[t]) > 0:
            print(f"  tile {t:3d}  [{float(lo[t]):9.2f}, {float(hi[t]):9.2f}]  truth "
                  f"{float(cal.true_flux_above[t]):9.2f}  PIT {float(cal.coverage.pit[t]):.3f}")
    show("posterior samples, sources brighter than magnitude 24", counts.confusion_samples)
    show("posterior mode, sources brighter than magnitude 24", counts.confusion_mode)

    # precision / recall / F1 per catalog (pooled over tiles), then bootstrap bands
    mag_bins = torch.arange(16, 24.5, 0.5)
    out = match_catalogs(true_counts, true_locs, true_fluxes,
                         sampler.pruned_counts.reshape(num_tiles, N),
                         sampler.pruned_locs.reshape(num_tiles, N, -1, 2),
                         sampler.pruned_fluxes.reshape(num_tiles, N, -1),
                         None, 0.5, 0.5, mag_bins)
    tt, tm, et, em = (x.sum(0) for x in out)  # [N,bins]
    precision = (em / et).nan_to_num(0)
    recall = (tm / tt).nan_to_num(0)
    f1 = (2 * precision * recall / (precision + recall)).nan_to_num(0)
    rows = torch.cat([precision, recall, f1], -1).contiguous()  # [N, 3 * bins]
    B = mag_bins.numel()
    lower, mean, upper = bootstrap_ci(rows, 10000, alpha=0.1, num_comparisons=3 * B)
    print(f"\nF1 per magnitude bin: mean of 10,000 bootstrap means of the {N} catalogs' rows, "
          "Bonferroni-corrected 90% band")
    edge = float("-inf")
    for b, top in enumerate(mag_bins.tolist()):
        if float(tt[:, b].sum()) + float(et[:, b].sum()) > 0:
            print(f"({edge:5.1f}, {top:4.1f}]  {float(mean[2 * B + b]):.3f}  "
                  f"[{float(lower[2 * B + b]):.3f}, {float(upper[2 * B + b]):.3f}]")
        edge = top


if __name__ == "__main__":
    main()
