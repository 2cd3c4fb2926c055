"""The step of the reference's experiments/m71/m71.ipynb that produces
params.pkl ("Optimize image model parameters"), on a synthetic field: simulate
a calibration field with M71ImageModel.sample, start every free parameter 20 %
off, fit the image model with the catalog held fixed, and print the fitted
parameters with their standard errors next to the truth.

    python examples/fit_m71_synthetic.py [num_stars] [all]

By default the six parameters a field of this size determines are free
(adu_per_nmgy, sigma1, sigma2, b, noise_multiplicative, background); `all`
frees the notebook's nine, of which beta, sigmap and p0 are then reported with
the large errors (or as unidentified) they have here.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smcdet_amd

smcdet_amd.install_as_smcdet()

from smcdet.fit import DEFAULT_FREE, PARAM_NAMES, fit_image_model, log_theta_of  # noqa: E402
from smcdet.images import M71ImageModel  # noqa: E402

# notebooks/smc.ipynb cell 2 (full-precision PSF parameters)
truth = dict(background=104.1486587524414, adu_per_nmgy=241.02658081054688,
             psf_params=[1.107237458229065, 2.0800251960754395, 2.3254318237304688,
                         5.240590572357178, 0.7346734404563904, 0.5114791393280029],
             noise_additive=1.0000007072408224e-10, noise_multiplicative=1.936462640762329)
H, W, R = 48, 64, 8
IDENTIFIED = ("adu_per_nmgy", "sigma1", "sigma2", "b", "noise_multiplicative", "background")


def main():
    num_stars = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    free = DEFAULT_FREE if "all" in sys.argv[2:] else IDENTIFIED
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = M71ImageModel(image_height=H, image_width=W, psf_radius=R, **truth)
    lo = torch.tensor([-4.0, -4.0], device=dev)
    span = torch.tensor([H + 8.0, W + 8.0], device=dev)
    locs = lo + span * torch.rand(1, num_stars, 2, device=dev)
    fluxes = torch.exp(math.log(10.0) + math.log(100.0) * torch.rand(1, num_stars, device=dev))
    image = model.sample(locs[None, None], fluxes[None, None])[0, 0, :, :, 0][None]
    # the notebook masks a frame and the saturated pixels; here: a 2-pixel frame
    mask = torch.zeros(1, H, W, dtype=torch.uint8, device=dev)
    mask[:, 2:-2, 2:-2] = 1

    start = log_theta_of(truth)
    for k, name in enumerate(free):
        start[PARAM_NAMES.index(name)] += 0.2 if k % 2 == 0 else -0.2
    v = [math.exp(float(t)) for t in start]
    init = dict(adu_per_nmgy=v[0], psf_params=v[1:7], noise_multiplicative=v[7],
                noise_additive=v[8], background=v[9])
    fit = fit_image_model(image, locs, fluxes, init, psf_radius=R, mask=mask, free=free)

    t = log_theta_of(truth)
    print(f"{H}x{W} field, psf_radius {R}, {num_stars} stars, {int(mask.sum())} pixels in the "
          "mask")
    print(f"converged {fit.converged} after {fit.n_evals} evaluations; nll {fit.nll:.3f}; "
          f"unidentified: {fit.unidentified or 'none'}")
    print(f"{'parameter':>22} {'truth':>12} {'start':>12} {'fitted':>12} {'rel. stderr':>12} "
          f"{'(fit-truth)/stderr':>19}")
    for i, name in enumerate(PARAM_NAMES):
        row = f"{name:>22} {math.exp(float(t[i])):12.6g} {v[i]:12.6g} " \
              f"{math.exp(float(fit.log_theta[i])):12.6g} "
        if name in fit.free:
            se = float(fit.stderr[fit.free.index(name)])
            z = (float(fit.log_theta[i]) - float(t[i])) / se if se == se else float("nan")
            row += f"{se:12.3g} {z:19.2f}"
        else:
            row += f"{'fixed':>12}"
        print(row)
    fitted = fit.image_model(H, W, R)
    print(f"fitted model: psf_normalizing_constant {float(fitted.psf_normalizing_constant):.6f} "
          f"(truth {float(model.psf_normalizing_constant):.6f}); rate image "
          f"{tuple(fit.rate.shape)}, {float(fit.rate.min()):.1f} .. {float(fit.rate.max()):.1f} ADU")


if __name__ == "__main__":
    main()
