"""From posterior catalogs to a list of detections: SMCsampler on a few
synthetic 8x8 M71 tiles with a known truth, then smcdet_amd.condense turns the
N pruned catalogs of every tile into one condensed catalog -- each detection
with the probability that it exists, a position and a flux with their
uncertainties -- and scores it like a point-estimate detector's catalog,
beside the mean precision and recall of the sampled catalogs themselves.

    python examples/condense_m71_synthetic.py [num_tiles] [num_catalogs]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.condense import condense_sampler  # noqa: E402
from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.kernel import SingleComponentMH  # noqa: E402
from smcdet.metrics import match_catalogs  # noqa: E402
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
    truth = M71Prior(min_objects=0, max_objects=30, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_detection_threshold"],
                     flux_upper=params["flux_upper"], pad=4)
    res = generate_images(truth, model, params["flux_detection_threshold"], 0, TILE, num_tiles)
    true_counts, true_locs, true_fluxes, images = res[3], res[4], res[5], res[-1]
    true_counts = true_counts.reshape(num_tiles)
    true_locs = true_locs.reshape(num_tiles, -1, 2)
    true_fluxes = true_fluxes.reshape(num_tiles, -1)

    prior = M71Prior(min_objects=10, max_objects=10, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_lower"], flux_upper=params["flux_upper"], pad=4)
    mh = SingleComponentMH(100, 0.1, 2.5, params["flux_lower"], params["flux_upper"])
    sampler = SMCsampler.from_tiles(
        images.reshape(1, num_tiles, TILE, TILE), prior, model, mh, num_catalogs, 0.5,
        "multinomial", params["flux_detection_threshold"], 100, print_every=10 ** 9)
    sampler.run()

    cat = condense_sampler(sampler)  # the pruned catalogs, box (0, 0, 8, 8)
    for t in range(num_tiles):
        n = int(true_counts[t])
        print(f"\ntile {t}: {n} true detectable sources")
        for i in range(n):
            h, w = true_locs[t, i].tolist()
            print(f"    truth     ({h:5.2f}, {w:5.2f})  flux {float(true_fluxes[t, i]):8.2f}")
        print(f"  {int(cat.n_seeds[t])} detections; expected count "
              f"{float(cat.expected_count[t]):.2f}, unassociated {float(cat.unassociated[t]):.3f}")
        print(f"    {'prob':>5} {'h':>6} {'w':>6} {'sd_h':>5} {'sd_w':>5} {'flux':>8} "
              f"{'5%':>8} {'95%':>8} {'mag':>6}")
        for k in range(int(cat.n_seeds[t])):
            q = cat.flux_quantiles[t, k].tolist()
            print(f"    {float(cat.prob[t, k]):5.3f} {float(cat.locs[t, k, 0]):6.2f} "
                  f"{float(cat.locs[t, k, 1]):6.2f} {float(cat.locs_sd[t, k, 0]):5.2f} "
                  f"{float(cat.locs_sd[t, k, 1]):5.2f} {float(cat.fluxes[t, k]):8.2f} "
                  f"{q[0]:8.2f} {q[2]:8.2f} {float(cat.mags[t, k]):6.2f}")

    # the condensed catalog scored as a detector's catalog (an N = 1 population),
    # beside the sampled catalogs' own mean precision and recall
    one_bin = torch.tensor([float("inf")])
    N = sampler.pruned_counts.shape[-1]

    def score(counts, locs, fluxes):
        tt, tm, et, em = match_catalogs(true_counts, true_locs, true_fluxes, counts, locs, fluxes,
                                        None, 0.5, 0.5, one_bin)
        precision = float(em.sum() / et.sum().clamp_min(1))
        recall = float(tm.sum() / tt.sum().clamp_min(1))
        return precision, recall

    p1, r1 = score(*cat.as_catalog(0.5))
    p2, r2 = score(sampler.pruned_counts.reshape(num_tiles, N),
                   sampler.pruned_locs.reshape(num_tiles, N, -1, 2),
                   sampler.pruned_fluxes.reshape(num_tiles, N, -1))
    print(f"\n{'':>34} precision  recall")
    print(f"{'condensed catalog, prob >= 0.5':>34} {p1:9.3f} {r1:7.3f}")
    print(f"{f'mean over {num_tiles * N} sampled catalogs':>34} {p2:9.3f} {r2:7.3f}")


if __name__ == "__main__":
    main()
