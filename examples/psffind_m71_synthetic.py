"""Two classical detectors on the same held-out synthetic M71 tiles: the
PSF-fitting detector (smcdet_amd.psffind: significance map, peaks, joint flux
solves and leave-one-out recentring, in rounds) and the isophotal extractor
(smcdet_amd.extract) scored with its forced PSF fluxes.  Both are tuned by
their grid search for F1 against the true detectable stars of the tiles;
prints both F1 values and the selected settings.

    python examples/psffind_m71_synthetic.py [num_tiles]

Stars closer than about a pixel share one matched-filter peak and stay one
detection: that is the method's limit and the samplers' territory.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet import extract, psffind  # noqa: E402
from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.prior import M71Prior  # noqa: E402

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


def main():
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 500
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
    res = generate_images(truth, model, params["flux_detection_threshold"], 0, TILE, num)
    true_counts = res[3].reshape(num)
    true_locs, true_fluxes = res[4].reshape(num, -1, 2), res[5].reshape(num, -1)
    images = res[-1].reshape(num, TILE, TILE).contiguous()
    print(f"{num} held-out tiles of {TILE}x{TILE}, {int(true_counts.sum())} detectable stars "
          "on them")
    score = dict(locs_tol=0.5, mags_tol=0.5, mag_bins=(14.0, 22.0), max_detections=16)

    found = psffind.tune(images, model, true_counts, true_locs, true_fluxes,
                         thresh=torch.arange(3.0, 11.5, 0.5), nms_radius=(0, 1, 2),
                         min_snr=(2.0, 3.0, 4.0), **score)
    print(f"psffind, {found.settings.shape[0]} settings: F1 {float(found.f1.min()):.3f} .. "
          f"{float(found.f1.max()):.3f}; selected "
          + ", ".join(f"{k} = {v:g}" for k, v in found.best.items()))

    sigma = math.sqrt(params["noise_additive"] + params["noise_multiplicative"]
                      * params["background"])
    iso = extract.tune(images, params["background"], sigma, true_counts, true_locs, true_fluxes,
                       thresh=torch.arange(1.0, 9.5, 0.5), minarea=torch.arange(1, 8),
                       deblend_cont=torch.logspace(-10, -2, 5),
                       clean_param=torch.logspace(-1, 2, 4), deblend_nthresh=64,
                       flux_scale=params["adu_per_nmgy"], flux="psf", image_model=model, **score)
    print(f"extract with PSF fluxes, {iso.settings.shape[0]} settings: F1 "
          f"{float(iso.f1.min()):.3f} .. {float(iso.f1.max()):.3f}; selected "
          + ", ".join(f"{k} = {v:g}" for k, v in iso.best.items()))
    print(f"\nF1 on the same tiles: psffind {float(found.f1.max()):.3f}, extract "
          f"{float(iso.f1.max()):.3f}")

    # what the selected setting leaves in the data: the residual's largest significance
    best = psffind.find(images, model, **found.best)
    left = psffind.significance_map(images, model, best.counts, best.locs, best.fluxes)
    print(f"largest residual significance per tile after the detections: median "
          f"{float(left.amax((1, 2)).median()):.2f}, max {float(left.max()):.2f} "
          f"(before: median {float(psffind.significance_map(images, model).amax((1, 2)).median()):.2f})")


if __name__ == "__main__":
    main()
