"""Posterior-predictive images and model checks: does the
fitted model reproduce the image?

The reference's users answer that by hand: notebooks/mcmc.ipynb rebuilds the
image from posterior catalogs, experiments/m71/psf_comparison.ipynb plots tile
minus reconstruction, every results.ipynb compares the observed total flux
with `posterior_predictive_total_observed_flux`.  All of them materialise a
rate image per catalog ([T,H,W,N]) and reduce it with torch.

`posterior_image` does it in one fused kernel (smcdet_posterior_image): every
catalog is rendered once, and what comes out is the posterior mean and
variance of the rate per pixel (float64 accumulation) and, per catalog, the
realised discrepancy chi2, a replicate image's discrepancy chi2_rep and its
total flux flux_rep.  Neither the rate images nor the replicates are stored,
and the result is the same bits on every run.

`PosteriorImage` derives the rest in plain torch: predictive variance,
residual, z-scores, posterior-predictive p-values.  `predictive_sampler` runs
it on a finished SMCsampler / MHsampler.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _hip
from ._hip import check, dev_f32, lib, ptr, stream_of
from ._rng import torch_seed

_U64 = (1 << 64) - 1


def catalog_chunks(pixels: int, N: int) -> int:
    """Workgroups (chunks of catalogs) per tile of smcdet_posterior_image, the
    rule include/smcdet_hip.h states: the partial sums of each are added in
    chunk order."""
    if pixels > _hip.MAX_TILE_PIXELS:
        bound = min(-(-N // 4), 64, max(1, (1 << 20) // pixels))
    else:
        bound = min(-(-N // 32), 64)
    chunk = 4 * -(-N // (4 * bound))
    return -(-N // chunk)


def _noise_var(image_model, rate):
    """v(rate): noise_additive + noise_multiplicative * rate (M71), rate (Poisson)."""
    if hasattr(image_model, "noise_multiplicative"):
        return float(image_model.noise_additive) + float(image_model.noise_multiplicative) * rate
    return rate


@dataclass
class PosteriorImage:
    """What `posterior_image` returns.  mean, rate_var: [..., H, W] float32,
    the posterior mean and (population) variance of the rate.  chi2, chi2_rep,
    flux_rep: [..., N] float32 or None (computed when tiled_image was given).
    weights: [..., N] or None (uniform); tiled_image: [..., H, W] or None.
    The leading dimensions are the caller's ([T] or [numH, numW]).  The derived
    properties are plain torch in float64."""
    mean: torch.Tensor
    rate_var: torch.Tensor
    image_model: object
    chi2: Optional[torch.Tensor] = None
    chi2_rep: Optional[torch.Tensor] = None
    flux_rep: Optional[torch.Tensor] = None
    tiled_image: Optional[torch.Tensor] = None
    weights: Optional[torch.Tensor] = None
    seed: Optional[int] = None
    offset: int = 0

    def _need_image(self, what):
        if self.tiled_image is None:
            raise ValueError(f"{what} needs the observed image: pass tiled_image to "
                             "posterior_image")

    @property
    def noise_var(self):
        """v(mean).  v is linear in the rate for both models, so this is E[v(rate)]."""
        return _noise_var(self.image_model, self.mean.double())

    @property
    def pred_var(self):
        """Variance of a replicate pixel: rate_var + noise_var."""
        return self.rate_var.double() + self.noise_var

    @property
    def residual(self):
        self._need_image("residual")
        return self.tiled_image.double() - self.mean.double()

    @property
    def z(self):
        """residual / sqrt(pred_var): about N(0, 1) per pixel under the model."""
        return self.residual / self.pred_var.sqrt()

    @property
    def flux_obs(self):
        """Observed total flux of each tile, [...]."""
        self._need_image("flux_obs")
        return self.tiled_image.double().sum((-2, -1))

    def _share(self, hit):
        if self.weights is None:
            return hit.double().mean(-1)
        w = self.weights.double()
        return (w * hit).sum(-1) / w.sum(-1)

    @property
    def p_value(self):
        """Posterior-predictive p-value of the chi2 discrepancy: the weighted
        share of catalogs whose replicate fits worse than the data,
        chi2_rep >= chi2.  [...]"""
        self._need_image("p_value")
        return self._share(self.chi2_rep >= self.chi2)

    @property
    def p_value_flux(self):
        """Weighted share of catalogs with flux_rep >= flux_obs.  [...]"""
        self._need_image("p_value_flux")
        return self._share(self.flux_rep.double() >= self.flux_obs.unsqueeze(-1))

    def to_image(self, field):
        """Stitches a per-tile field [numH, numW, H, W] (a tensor, or the name
        of one: "mean", "z", ...) into the [numH*H, numW*W] image: the inverse
        of the samplers' unfold."""
        x = getattr(self, field) if isinstance(field, str) else field
        if x.dim() != 4:
            raise ValueError(f"to_image needs a [numH, numW, H, W] field, got {tuple(x.shape)}")
        nH, nW, H, W = x.shape
        return x.permute(0, 2, 1, 3).reshape(nH * H, nW * W)


def posterior_image(image_model, locs, fluxes, *, weights=None, tiled_image=None, seed=None,
                    offset=0):
    """Posterior mean and variance of the rate image and the per-catalog
    model-check sums, from the catalogs locs [T,N,S,2] / fluxes [T,N,S] (or the
    reference layout [numH,numW,N,S,2] / [numH,numW,N,S]) under `image_model`
    (ImageModel or M71ImageModel).  weights [...,N] >= 0 (None: uniform; need
    not be normalised).  tiled_image [...,H,W]: the observed tiles; with it the
    per-catalog chi2, chi2_rep and flux_rep are computed too.  seed / offset:
    the Philox key and counter base of the replicate noise (seed None: drawn
    from torch's generator, as ImageModel.sample does); replicate pixel p of
    catalog n of tile t is the draw smcdet_sample_image makes for element
    (t*H*W + p)*N + n.  HIP float32 tensors only.  Returns a PosteriorImage
    whose fields keep the leading dimensions."""
    locs = dev_f32(locs, "locs")
    fluxes = dev_f32(fluxes, "fluxes")
    if locs.dim() not in (4, 5) or locs.shape[-1] != 2:
        raise ValueError(f"locs must be [T,N,S,2] or [numH,numW,N,S,2], got {tuple(locs.shape)}")
    lead = tuple(locs.shape[:-3])
    N, S = int(locs.shape[-3]), int(locs.shape[-2])
    if tuple(fluxes.shape) != lead + (N, S):
        raise ValueError(f"fluxes has shape {tuple(fluxes.shape)}, expected {lead + (N, S)}")
    T = 1
    for d in lead:
        T *= int(d)
    H, W = int(image_model.image_height), int(image_model.image_width)
    if weights is not None:
        weights = dev_f32(weights, "weights")
        if tuple(weights.shape) != lead + (N,):
            raise ValueError(f"weights has shape {tuple(weights.shape)}, expected {lead + (N,)}")
    if tiled_image is not None:
        tiled_image = dev_f32(tiled_image, "tiled_image")
        if tuple(tiled_image.shape) != lead + (H, W):
            raise ValueError(f"tiled_image has shape {tuple(tiled_image.shape)}, expected "
                             f"{lead + (H, W)}")
    seed = torch_seed() if seed is None else int(seed) & _U64
    offset = int(offset) & _U64
    dev = locs.device
    cm = image_model._cmodel()
    need = lib().smcdet_posterior_image_workspace(_hip.ref(cm), T, N)
    if need < 0:
        check(int(need), "smcdet_posterior_image_workspace")
    workspace = torch.empty(int(need), device=dev, dtype=torch.uint8)
    mean = torch.empty(lead + (H, W), device=dev, dtype=torch.float32)
    var = torch.empty_like(mean)
    chi2 = chi2_rep = flux_rep = None
    if tiled_image is not None:
        chi2 = torch.empty(lead + (N,), device=dev, dtype=torch.float32)
        chi2_rep = torch.empty_like(chi2)
        flux_rep = torch.empty_like(chi2)
    check(lib().smcdet_posterior_image(
        _hip.ref(cm), ptr(tiled_image), ptr(locs) if S > 0 else None,
        ptr(fluxes) if S > 0 else None, ptr(weights), T, N, S, seed, offset, ptr(mean), ptr(var),
        ptr(chi2), ptr(chi2_rep), ptr(flux_rep), ptr(workspace), int(need), stream_of(locs)),
        "smcdet_posterior_image")
    return PosteriorImage(mean=mean, rate_var=var, image_model=image_model, chi2=chi2,
                          chi2_rep=chi2_rep, flux_rep=flux_rep, tiled_image=tiled_image,
                          weights=weights, seed=seed, offset=offset)


def predictive_sampler(sampler, seed=None):
    """`posterior_image` of a finished SMCsampler or MHsampler: its ImageModel,
    its tiled_image and its unpruned locs / fluxes (sub-threshold and padding
    sources emit light too), with the sampler's weights where it has them.
    seed None: the sampler's own Philox seed (the noise stream has its own
    tag, so it shares no draw with the run).  Fields come back in the reference
    layout [numH, numW, ...]."""
    if not getattr(sampler, "has_run", False):
        raise ValueError("predictive_sampler: the sampler hasn't been run yet (call run() first)")
    if seed is None:
        rng = getattr(sampler, "rng", None)
        seed = rng.seed if rng is not None else None
    return posterior_image(sampler.ImageModel, sampler.locs, sampler.fluxes,
                           weights=getattr(sampler, "weights", None),
                           tiled_image=sampler.tiled_image, seed=seed)
