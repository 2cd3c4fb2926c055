"""The reference's Normal-flux experiment (experiments/jsm2024,
normalfluxes_tiles_32x32/run_smc_mh.py) on one synthetic image, through the
drop-in alias: StarPrior(flux_mean=1300, flux_stdev=250) with the Poisson
ImageModel(psf_stdev=1.0, background=300), a 32x32 image in 8x8 tiles, up to
S = 6 sources per tile, SMC with SingleComponentMH; then the detections
(`condense_sampler`) and the posterior-predictive checks (`predictive_sampler`)
of the run.

The kernel's flux bounds are mean +- 5 stdev = [50, 2550], not jsm2024's
+- 2.5 stdev: the reference's truncated-normal proposal asserts that every
current flux lies inside the bounds (distributions.py:51), and about 1.2% of
the prior's initial draws lie outside +- 2.5 stdev.

    python examples/smc_normalfluxes_synthetic.py [num_catalogs_per_count]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.condense import condense_sampler  # noqa: E402
from smcdet.images import ImageModel, generate_images  # noqa: E402
from smcdet.kernel import SingleComponentMH  # noqa: E402
from smcdet.predictive import predictive_sampler  # noqa: E402
from smcdet.prior import StarPrior  # noqa: E402
from smcdet.sampler import SMCsampler  # noqa: E402

IMAGE, TILE, S = 32, 8, 6
MEAN, SD, PAD = 1300.0, 250.0, 2


def main():
    per_count = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    torch.manual_seed(0)
    full = ImageModel(image_height=IMAGE, image_width=IMAGE, psf_radius=8, psf_stdev=1.0,
                      background=300.0)
    truth = StarPrior(min_objects=0, max_objects=20, image_height=IMAGE, image_width=IMAGE,
                      flux_mean=MEAN, flux_stdev=SD, pad=PAD)
    res = generate_images(truth, full, 0.0, 0, IMAGE, 1)
    true_count, true_locs, true_fluxes, image = int(res[3][0]), res[4][0], res[5][0], res[-1][0]
    print(f"{true_count} true sources inside the image")

    prior = StarPrior(min_objects=0, max_objects=S, image_height=TILE, image_width=TILE,
                      flux_mean=MEAN, flux_stdev=SD, pad=PAD)
    model = ImageModel(image_height=TILE, image_width=TILE, psf_radius=8, psf_stdev=1.0,
                       background=300.0)
    mh = SingleComponentMH(100, 0.25, 100.0, MEAN - 5 * SD, MEAN + 5 * SD)
    sampler = SMCsampler(image=image, tile_dim=TILE, Prior=prior, ImageModel=model,
                         MutationKernel=mh, num_catalogs=per_count, ess_threshold_prop=0.75,
                         resample_method="multinomial", flux_detection_threshold=0.0,
                         max_smc_iters=100, print_every=10)
    sampler.run()

    nt = IMAGE // TILE
    cat = condense_sampler(sampler)  # the pruned catalogs, box (0, 0, 8, 8) per tile
    print(f"\n{'tile':>5} {'true':>4} {'E count':>8}   detections (prob, h, w, flux)")
    for t in range(nt * nt):
        r, c = divmod(t, nt)
        lo = torch.tensor([r * TILE, c * TILE], dtype=true_locs.dtype, device=true_locs.device)
        inside = ((true_locs[:true_count] >= lo) & (true_locs[:true_count] < lo + TILE)).all(-1)
        dets = ", ".join(
            f"({float(cat.prob[t, k]):.2f}, {float(cat.locs[t, k, 0]):.1f}, "
            f"{float(cat.locs[t, k, 1]):.1f}, {float(cat.fluxes[t, k]):.0f})"
            for k in range(int(cat.n_seeds[t])))
        print(f"{t:5d} {int(inside.sum()):4d} {float(cat.expected_count[t]):8.2f}   {dets}")

    post = predictive_sampler(sampler)
    print(f"\n{'tile':>5} {'flux_obs':>10} {'E flux_rep':>10} {'p(flux)':>8} {'p(chi2)':>8}")
    for t in range(nt * nt):
        r, c = divmod(t, nt)
        print(f"{t:5d} {float(post.flux_obs[r, c]):10.1f} "
              f"{float(post.flux_rep[r, c].double().mean()):10.1f} "
              f"{float(post.p_value_flux[r, c]):8.3f} {float(post.p_value[r, c]):8.3f}")


if __name__ == "__main__":
    main()
