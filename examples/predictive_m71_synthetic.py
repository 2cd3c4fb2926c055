"""Does the fitted model reproduce the image?  SMCsampler on a few synthetic
8x8 M71 tiles, then smcdet_amd.predictive: the posterior mean image, per-tile
posterior-predictive p-values (chi2 discrepancy and total flux) and the pixels
the model explains worst.  The last tile's image gets a star the sampler's
prior cannot place (ten times the prior's upper flux limit), so its p-values
show what a misfit looks like.

    python examples/predictive_m71_synthetic.py [num_tiles] [num_catalogs]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.kernel import SingleComponentMH  # noqa: E402
from smcdet.predictive import predictive_sampler  # noqa: E402
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
    images = generate_images(truth, model, params["flux_detection_threshold"], 0, TILE,
                             num_tiles)[-1].reshape(1, num_tiles, TILE, TILE).clone()
    # the misfit: a star far brighter than the prior allows, in the last tile
    dev = images.device
    star = model.rate(torch.tensor([[[[[3.5, 4.5]]]]], device=dev),
                      torch.tensor([[[[10 * params["flux_upper"]]]]], device=dev))[0, 0, :, :, 0]
    images[0, -1] += star - params["background"]

    prior = M71Prior(min_objects=10, max_objects=10, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_lower"], flux_upper=params["flux_upper"], pad=4)
    mh = SingleComponentMH(100, 0.1, 2.5, params["flux_lower"], params["flux_upper"])
    sampler = SMCsampler.from_tiles(images, prior, model, mh, num_catalogs, 0.5, "multinomial",
                                    params["flux_detection_threshold"], 100,
                                    print_every=10 ** 9)
    sampler.run()

    post = predictive_sampler(sampler)
    z = post.z[0]                                       # [num_tiles, 8, 8]
    print(f"{'tile':>4} {'flux_obs':>10} {'E flux_rep':>10} {'p(flux)':>8} {'E chi2':>9} "
          f"{'E chi2_rep':>10} {'p(chi2)':>8} {'max |z|':>8}")
    for t in range(num_tiles):
        print(f"{t:4d} {float(post.flux_obs[0, t]):10.1f} "
              f"{float(post.flux_rep[0, t].double().mean()):10.1f} "
              f"{float(post.p_value_flux[0, t]):8.3f} "
              f"{float(post.chi2[0, t].double().mean()):9.1f} "
              f"{float(post.chi2_rep[0, t].double().mean()):10.1f} "
              f"{float(post.p_value[0, t]):8.3f} {float(z[t].abs().max()):8.2f}")
    print("\nthe five pixels the model explains worst (|z| = |x - mean| / sqrt(pred_var)):")
    top = z.abs().flatten().topk(5).indices.tolist()
    for i in top:
        t, p = divmod(i, TILE * TILE)
        h, w = divmod(p, TILE)
        print(f"  tile {t} pixel ({h}, {w}): observed {float(post.tiled_image[0, t, h, w]):9.1f}  "
              f"mean {float(post.mean[0, t, h, w]):9.1f}  "
              f"rate sd {float(post.rate_var[0, t, h, w]) ** 0.5:7.2f}  "
              f"noise sd {float(post.noise_var[0, t, h, w]) ** 0.5:7.2f}  "
              f"z {float(z[t, h, w]):6.2f}")
    print(f"\nstitched mean image: {tuple(post.to_image('mean').shape)}")


if __name__ == "__main__":
    main()
