"""Forced PSF photometry on synthetic M71 tiles: first at the true positions
(every star of the tile and its padding solved jointly; the errors' calibration
and the magnitude residuals), then at the positions smcdet_amd.extract finds,
where the isophotal fluxes `extract` reports are set against the PSF fluxes of
the same detections.  Prints the magnitude residuals of both against the truth.

    python examples/photometry_m71_synthetic.py [num_tiles]

A detection is compared with the nearest true star within 0.5 pixel.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.extract import extract  # noqa: E402
from smcdet.images import M71ImageModel, generate_images  # noqa: E402
from smcdet.photometry import forced_photometry, photometry_of  # noqa: E402
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


def mags(f):
    return 22.5 - 2.5 * torch.log10(f)


def report(name, dm):
    dm = dm[torch.isfinite(dm)]
    if dm.numel() == 0:
        print(f"{name:>28}: no sources")
        return
    print(f"{name:>28}: n {dm.numel():5d}  median {float(dm.median()):+.3f}  "
          f"rms {float(dm.pow(2).mean().sqrt()):.3f}  |dm| < 0.5: "
          f"{float((dm.abs() < 0.5).double().mean()):.3f}")


def main():
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
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
    all_counts = res[0].reshape(num).to(torch.int32)
    all_locs, all_fluxes = res[1].reshape(num, -1, 2), res[2].reshape(num, -1)
    true_counts = res[3].reshape(num)
    true_locs, true_fluxes = res[4].reshape(num, -1, 2), res[5].reshape(num, -1)
    images = res[-1].reshape(num, TILE, TILE).contiguous()
    S = all_locs.shape[1]
    print(f"{num} tiles of {TILE}x{TILE}; {int(all_counts.sum())} stars with the padding, "
          f"{int(true_counts.sum())} detectable ones on the tiles")

    # ---- at the true positions: the tile's and the padding's stars, jointly -------
    p = forced_photometry(images, all_counts, all_locs.contiguous(), model)
    live = torch.arange(S, device=images.device)[None, :] < all_counts[:, None]
    on_tile = live & ((all_locs > 0) & (all_locs < TILE)).all(-1)
    z = ((p.fluxes - all_fluxes.double()) / p.flux_err)[on_tile]
    z = z[torch.isfinite(z)]
    print(f"\nat the true positions ({int((p.status & 2).ne(0).sum())} singular tiles, "
          f"{int((p.status & 1).ne(0).sum())} with a dropped source):")
    print(f"{'(flux - truth) / flux_err':>28}: n {z.numel():5d}  mean {float(z.mean()):+.3f}  "
          f"sd {float(z.std()):.3f}")
    ok = on_tile & (p.fluxes > 0) & (all_fluxes > params["flux_detection_threshold"])
    report("PSF magnitude - truth", (mags(p.fluxes) - mags(all_fluxes.double()))[ok])

    # ---- at extract's positions: isophotal against PSF fluxes -----------------------
    sigma = math.sqrt(params["noise_additive"] + params["noise_multiplicative"]
                      * params["background"])
    det = extract(images, params["background"], sigma, thresh=3.0, minarea=3, deblend_nthresh=64,
                  max_detections=16, flux_scale=params["adu_per_nmgy"])
    det_psf, phot = photometry_of(det, images, model)
    K = det.locs.shape[1]
    d = torch.cdist(det.locs.nan_to_num(1e6), true_locs)  # [num,K,St]
    kept = torch.arange(true_locs.shape[1], device=d.device)[None, None, :] \
        < true_counts[:, None, None]
    d = torch.where(kept, d, torch.full_like(d, float("inf")))
    dist, idx = d.min(-1)
    matched = (dist < 0.5) & (torch.arange(K, device=d.device)[None, :] < det.counts[:, None])
    tm = mags(true_fluxes.gather(1, idx.clamp(max=true_fluxes.shape[1] - 1)))
    print(f"\nat extract's positions (thresh 3, minarea 3): {int(det.counts.sum())} detections, "
          f"{int(matched.sum())} within 0.5 px of a true star, "
          f"{int((~torch.isfinite(phot.fluxes) & matched).sum())} of them without a PSF solve")
    report("isophotal magnitude - truth", (mags(det.fluxes) - tm)[matched])
    report("PSF magnitude - truth", (mags(det_psf.fluxes) - tm)[matched])
    corner = matched & (((det.locs - TILE / 2).abs() > TILE / 2 - 1.5).all(-1))
    report("isophotal, tile corners", (mags(det.fluxes) - tm)[corner])
    report("PSF, tile corners", (mags(det_psf.fluxes) - tm)[corner])


if __name__ == "__main__":
    main()
