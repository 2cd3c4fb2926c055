"""The reference's headline comparison (experiments/m71synthetic: run_sep.py and
results.ipynb), "SMC vs a classical detector", without sep: the baseline is
smcdet_amd.extract, tuned as run_sep.py tunes sep -- its full grid of 2,380
settings scored for F1 on held-out tiles, two launches -- and then run with
the selected setting on the tiles SMC ran on.  Prints precision / recall / F1
per magnitude bin for both, side by side.

    python examples/baseline_m71_synthetic.py [num_tiles] [num_catalogs] [num_tune_tiles]

The baseline's noise level is the image model's at the background,
sqrt(noise_additive + noise_multiplicative * background).
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.extract import extract, tune  # noqa: E402
from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.kernel import SingleComponentMH  # noqa: E402
from smcdet.metrics import compute_precision_recall_f1, match_catalogs  # noqa: E402
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


def truth_and_tiles(truth, model, num):
    res = generate_images(truth, model, params["flux_detection_threshold"], 0, TILE, num)
    return (res[3].reshape(num), res[4].reshape(num, -1, 2), res[5].reshape(num, -1),
            res[-1].reshape(num, TILE, TILE))


def main():
    num_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    num_catalogs = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    num_tune = int(sys.argv[3]) if len(sys.argv) > 3 else 200
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
    true_counts, true_locs, true_fluxes, images = truth_and_tiles(truth, model, num_tiles)
    print("true detectable counts per tile:", true_counts.tolist())
    sigma = math.sqrt(params["noise_additive"] + params["noise_multiplicative"]
                      * params["background"])

    # the baseline's hyperparameters: run_sep.py's grid on a new batch of tiles
    tune_truth = truth_and_tiles(truth, model, num_tune)
    grid = dict(thresh=torch.arange(1.0, 8.5, 0.5), minarea=torch.arange(1, 8),
                deblend_cont=torch.logspace(-10, -2, 5), clean_param=torch.logspace(-1, 2, 4))
    tuned = tune(tune_truth[3], params["background"], sigma, *tune_truth[:3], **grid,
                 deblend_nthresh=64, max_detections=16, locs_tol=0.5, mags_tol=0.5,
                 mag_bins=torch.arange(14.0, 22.5, 8), flux_scale=params["adu_per_nmgy"])
    print(f"\ntuned on {num_tune} held-out tiles x {tuned.settings.shape[0]} settings: "
          f"F1 {float(tuned.f1.min()):.3f} .. {float(tuned.f1.max()):.3f}; selected "
          + ", ".join(f"{k} = {v:g}" for k, v in tuned.best.items()))

    prior = M71Prior(min_objects=10, max_objects=10, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_lower"], flux_upper=params["flux_upper"], pad=4)
    mh = SingleComponentMH(100, 0.1, 2.5, params["flux_lower"], params["flux_upper"])
    sampler = SMCsampler.from_tiles(
        images.reshape(1, num_tiles, TILE, TILE), prior, model, mh, num_catalogs, 0.5,
        "multinomial", params["flux_detection_threshold"], 100, print_every=10 ** 9)
    sampler.run()

    mag_bins = torch.arange(16, 24.5, 0.5)
    N = sampler.pruned_counts.shape[-1]
    smc = match_catalogs(true_counts, true_locs, true_fluxes,
                         sampler.pruned_counts.reshape(num_tiles, N),
                         sampler.pruned_locs.reshape(num_tiles, N, -1, 2),
                         sampler.pruned_fluxes.reshape(num_tiles, N, -1),
                         None, 0.5, 0.5, mag_bins)
    det = extract(images, params["background"], sigma, deblend_nthresh=64, max_detections=16,
                  flux_scale=params["adu_per_nmgy"], **tuned.best)
    print("baseline detections per tile:   ", det.counts.tolist())
    base = match_catalogs(true_counts, true_locs, true_fluxes, det.counts[:, None],
                          det.locs[:, None], det.fluxes[:, None], None, 0.5, 0.5, mag_bins)
    s = compute_precision_recall_f1(*[x.flatten(0, 1) for x in smc])
    b = compute_precision_recall_f1(*[x.flatten(0, 1) for x in base])
    true_per_bin = smc[0][:, 0].sum(0)
    print(f"\n{num_tiles} tiles; SMC: {N} catalogs per tile; baseline: one catalog per tile")
    print(f"{'':>14} {'':>5} {'SMC':^28} {'baseline':^28}")
    print(f"{'mag bin':>14} {'true':>5} " + 2 * f"{'precision':>10} {'recall':>8} {'F1':>8} ")
    lo = float("-inf")
    for k, hi in enumerate(mag_bins.tolist()):
        if float(smc[0][..., k].sum() + smc[2][..., k].sum() + base[2][..., k].sum()) > 0:
            print(f"({lo:5.1f}, {hi:4.1f}] {int(true_per_bin[k]):5d} "
                  + "".join(f"{float(x[0][k]):10.3f} {float(x[1][k]):8.3f} {float(x[2][k]):8.3f} "
                            for x in (s, b)))
        lo = hi


if __name__ == "__main__":
    main()
