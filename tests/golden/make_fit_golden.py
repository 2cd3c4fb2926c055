"""Writes tests/golden/fit_m71_field.npz from the reference's M71ImageModel
(the checkout tests/golden/make_golden.py puts on the path; CPU): a 24x40 field
with psf_radius 8 and 12 stars, its image, locs and fluxes, and the
reference's float32 `loglikelihood` at three parameter
vectors (the M71 values and two perturbations) -- and the same reference code
run in float64, whose distance from the float32 values is what
tests/test_fit_host.py takes its bound from.  Data only.

    python tests/golden/make_fit_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402,F401  (puts the reference on the path)
from smcdet.images import M71ImageModel  # noqa: E402

from _params import M71  # noqa: E402

H, W, R, D = 24, 40, 8, 12
# order: adu_per_nmgy, sigma1, sigma2, sigmap, beta, b, p0, noise_multiplicative,
# noise_additive, background
BASE = np.array([M71["adu_per_nmgy"]] + list(M71["psf_params"])
                + [M71["noise_multiplicative"], M71["noise_additive"], M71["background"]],
                dtype=np.float64)
FACTORS = np.array([[1.0] * 10,
                    [1.03, 0.9, 1.1, 1.05, 0.95, 1.2, 0.8, 1.1, 2.0, 0.97],
                    [0.96, 1.15, 0.92, 0.9, 1.1, 0.85, 1.25, 0.9, 0.25, 1.02]])


def model(theta, dtype):
    torch.set_default_dtype(dtype)
    t = [float(v) for v in theta]
    return M71ImageModel(image_height=H, image_width=W, background=t[9], psf_radius=R,
                         adu_per_nmgy=t[0], psf_params=t[1:7], noise_additive=t[8],
                         noise_multiplicative=t[7])


def main():
    rng = np.random.default_rng(20)
    locs = np.stack([rng.uniform(-4, H + 4, D), rng.uniform(-4, W + 4, D)], -1).astype(np.float32)
    fluxes = np.exp(rng.uniform(np.log(10.0), np.log(1000.0), D)).astype(np.float32)
    torch.manual_seed(20)
    tl = torch.from_numpy(locs)[None, None, None]
    tf = torch.from_numpy(fluxes)[None, None, None]
    image = model(BASE, torch.float32).sample(tl, tf)[0, 0, :, :, 0].numpy().astype(np.float32)
    theta = BASE[None] * FACTORS
    ll32, ll64 = [], []
    for t in theta:
        for dtype, out in ((torch.float32, ll32), (torch.float64, ll64)):
            m = model(t, dtype)
            ti = torch.from_numpy(image).to(dtype)[None, None]
            out.append(float(m.loglikelihood(ti, tl.to(dtype), tf.to(dtype))[0, 0, 0]))
    torch.set_default_dtype(torch.float32)
    ll32, ll64 = np.array(ll32, np.float32), np.array(ll64, np.float64)
    diff = float(np.abs(ll32.astype(np.float64) - ll64).max())
    print("loglik float32", ll32, "float64", ll64, "largest |float32 - float64|", diff)
    np.savez(os.path.join(HERE, "fit_m71_field.npz"), image=image, locs=locs, fluxes=fluxes,
             psf_radius=np.int32(R), theta=theta, loglik_f32=ll32, loglik_f64=ll64,
             f32_f64_diff=np.float64(diff))


if __name__ == "__main__":
    main()
