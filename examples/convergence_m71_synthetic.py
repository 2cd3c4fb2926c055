"""Did the MCMC chains mix, and what are their kept draws worth?  42 synthetic
8x8 M71 tiles (the tile count of experiments/m71/run_mcmc.py's small run), four
MH chains per tile, then split-R-hat, bulk / tail / mean ESS and the Monte
Carlo standard error of every trace (smcdet.convergence), and the (tile,
quantity) pairs that fail the usual thresholds.

    python examples/convergence_m71_synthetic.py [num_tiles] [samples_total] [burnin] [keep_every]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.convergence import diagnose_sampler  # noqa: E402
from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.prior import M71Prior  # noqa: E402
from smcdet.sampler import MHsampler  # noqa: E402

# notebooks/smc.ipynb cell 2 (full-precision PSF parameters)
params = dict(flux_alpha=0.21411753249015655, flux_lower=0.06291294097900389,
              flux_upper=1804.6791992187502, flux_detection_threshold=0.25165176391601557,
              counts_rate=0.030264640226960182, background=104.1486587524414,
              adu_per_nmgy=241.02658081054688,
              psf_params=[1.107237458229065, 2.0800251960754395, 2.3254318237304688,
                          5.240590572357178, 0.7346734404563904, 0.5114791393280029],
              psf_radius=8, noise_additive=1.0000007072408224e-10,
              noise_multiplicative=1.936462640762329)
TILE, CHAINS = 8, 4


def main():
    arg = [int(v) for v in sys.argv[1:]]
    num_tiles, total, burnin, keep = (arg + [42, 20000, 10000, 5][len(arg):])[:4]
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
                             num_tiles)[-1]
    prior = M71Prior(min_objects=10, max_objects=10, counts_rate=params["counts_rate"],
                     image_height=TILE, image_width=TILE, flux_alpha=params["flux_alpha"],
                     flux_lower=params["flux_lower"], flux_upper=params["flux_upper"], pad=4)
    mh = MHsampler.from_tiles(images.reshape(1, num_tiles, TILE, TILE), prior, model, 0.1, 2.5,
                              params["flux_detection_threshold"], total, burnin, keep,
                              print_every=10 ** 9, num_chains=CHAINS)
    mh.run()
    conv = diagnose_sampler(mh, flux_cuts=(0.0,), log_target=True)
    kept = mh.pruned_counts.shape[-1] // CHAINS
    print(f"{num_tiles} tiles x {CHAINS} chains x {kept} kept draws "
          f"({total} samples, burn-in {burnin}, every {keep}th kept)")
    print("acceptance rate after the burn-in: "
          f"{float(conv.accept_rate.mean()):.3f} (min {float(conv.accept_rate.min()):.3f}), "
          f"{int((conv.frozen != 0).sum())} frozen chains\n")
    print(f"{'tile':>4} {'quantity':<16} {'mean':>10} {'mcse':>9} {'rhat':>7} {'ess_bulk':>9} "
          f"{'ess_tail':>9} {'ess_mean':>9} {'tau':>7}")
    for t in range(num_tiles):
        for q, name in enumerate(conv.names):
            i = (0, t, q)
            print(f"{t:4d} {name:<16} {float(conv.mean[i]):10.3f} {float(conv.mcse_mean[i]):9.3g} "
                  f"{float(conv.rhat[i]):7.4f} {float(conv.ess_bulk[i]):9.0f} "
                  f"{float(conv.ess_tail[i]):9.0f} {float(conv.ess_mean[i]):9.0f} "
                  f"{float(conv.tau[i]):7.2f}")
    bad = conv.warnings(rhat_max=1.01, ess_min=400)
    print(f"\n{len(bad)} of {num_tiles * len(conv.names)} (tile, quantity) pairs fail "
          "rhat <= 1.01, ess_bulk >= 400, ess_tail >= 400 (a trace that never moves counts too):")
    for idx, name, rhat, eb, et in bad:
        print(f"  tile {idx[1]:3d} {name:<16} rhat {rhat:7.4f}  ess_bulk {eb:9.0f}  "
              f"ess_tail {et:9.0f}")


if __name__ == "__main__":
    main()
