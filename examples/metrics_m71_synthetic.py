"""Scoring a run as the reference's experiments do (experiments/m71synthetic:
results.ipynb, run_sep.py), but over every posterior catalog: SMCsampler on a
few synthetic 8x8 M71 tiles with a known truth, then smcdet.metrics on all
pruned catalogs of all tiles -- one launch, no subsample of 200.

    python examples/metrics_m71_synthetic.py [num_tiles] [num_catalogs]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

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


def main():
    num_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    num_catalogs = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    torch.manual_seed(0)
    model = M71ImageModel(image_height=TILE, image_width=TILE, background=params["background"],
                          psf_radius=params["psf_radius"], adu_per_nmgy=params["adu_per_nmgy"],
                          psf_params=params["psf_params"],
                          noise_additive=params["noise_additive"],
                          noise_multiplicative=params["noise_multiplicative"])
    # the truth: independent tiles drawn from the prior (sources in the 4-pixel
    # padding shine into the tile but are pruned from the true catalog)
    truth = M71Prior(min_objects=0, max_objects=30, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_detection_threshold"],
                     flux_upper=params["flux_upper"], pad=4)
    res = generate_images(truth, model, params["flux_detection_threshold"], 0, TILE, num_tiles)
    true_counts, true_locs, true_fluxes, images = res[3], res[4], res[5], res[-1]
    true_counts = true_counts.reshape(num_tiles)
    print("true detectable counts per tile:", true_counts.tolist())

    prior = M71Prior(min_objects=10, max_objects=10, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_lower"], flux_upper=params["flux_upper"], pad=4)
    mh = SingleComponentMH(100, 0.1, 2.5, params["flux_lower"], params["flux_upper"])
    sampler = SMCsampler.from_tiles(
        images.reshape(1, num_tiles, TILE, TILE), prior, model, mh, num_catalogs, 0.5,
        "multinomial", params["flux_detection_threshold"], 100, print_every=10 ** 9)
    sampler.run()

    # every pruned catalog of every tile against its tile's truth
    N = sampler.pruned_counts.shape[-1]
    mag_bins = torch.arange(16, 24.5, 0.5)
    out = match_catalogs(true_counts, true_locs.reshape(num_tiles, -1, 2),
                         true_fluxes.reshape(num_tiles, -1),
                         sampler.pruned_counts.reshape(num_tiles, N),
                         sampler.pruned_locs.reshape(num_tiles, N, -1, 2),
                         sampler.pruned_fluxes.reshape(num_tiles, N, -1),
                         None, 0.5, 0.5, mag_bins)
    # pooled over tiles and catalogs, per magnitude bin (the notebook's tables)
    precision, recall, f1 = compute_precision_recall_f1(*[x.flatten(0, 1) for x in out])
    true_per_bin = out[0][:, 0].sum(0)
    print(f"\nscored {num_tiles} tiles x {N} catalogs = {num_tiles * N} matchings")
    print(f"{'mag bin':>14} {'true':>5} {'precision':>10} {'recall':>8} {'F1':>8}")
    lo = float("-inf")
    for b, hi in enumerate(mag_bins.tolist()):
        if float(out[0][..., b].sum()) + float(out[2][..., b].sum()) > 0:
            print(f"({lo:5.1f}, {hi:4.1f}] {int(true_per_bin[b]):5d} {float(precision[b]):10.3f} "
                  f"{float(recall[b]):8.3f} {float(f1[b]):8.3f}")
        lo = hi


if __name__ == "__main__":
    main()
