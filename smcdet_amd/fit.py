"""Fit the M71 image model to calibration fields: the step of
the reference's experiments/m71/m71.ipynb ("Optimize image model parameters")
that produces params.pkl -- adu_per_nmgy, the six PSF parameters, the two noise
coefficients and the background -- from fields whose catalog is held fixed.

  `objective`        smcdet_fit_objective: the masked Gaussian negative
                     log-likelihood, its gradient and its expected Fisher
                     information in the logs of the ten parameters, float64,
                     and optionally the rate image;
  `fit_image_model`  torch.optim.LBFGS (strong Wolfe, as the notebook) over a
                     float64 host vector of the free logs; the closure is one
                     `objective` call and one 888-byte read-back;
  `ModelFit`         the fitted parameters in params.pkl's form, with their
                     covariance and relative standard errors.

Inputs are HIP tensors; nothing falls back to the host.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, lib, ptr, stream_of

PARAM_NAMES = ("adu_per_nmgy", "sigma1", "sigma2", "sigmap", "beta", "b", "p0",
               "noise_multiplicative", "noise_additive", "background")
PSF_NAMES = PARAM_NAMES[1:7]
# the notebook's choice: everything but the background
DEFAULT_FREE = PARAM_NAMES[:9]
# a free parameter is unidentified when the free block of the information has
# an eigenvalue below this times its largest, and the parameter carries weight
# in that eigenvector
UNIDENTIFIED_RTOL = 1e-12
UNIDENTIFIED_WEIGHT = 0.1


def params_dict(source):
    """A dict in the form of the reference's params.pkl from such a dict or an
    M71ImageModel."""
    if isinstance(source, dict):
        missing = [k for k in ("adu_per_nmgy", "psf_params", "noise_additive",
                               "noise_multiplicative", "background") if k not in source]
        if missing:
            raise ValueError(f"params: missing {missing}")
        pp = source["psf_params"]
        pp = pp.detach().cpu().reshape(-1).tolist() if isinstance(pp, torch.Tensor) else list(pp)
        if len(pp) != 6:
            raise ValueError("params: psf_params must hold (sigma1, sigma2, sigmap, beta, b, p0)")
        out = dict(source)
        out["psf_params"] = [float(v) for v in pp]
        for k in ("adu_per_nmgy", "noise_additive", "noise_multiplicative", "background"):
            out[k] = float(source[k])
        return out
    return dict(adu_per_nmgy=float(source.adu_per_nmgy),
                psf_params=[float(v) for v in source.psf_params],
                noise_additive=float(source.noise_additive),
                noise_multiplicative=float(source.noise_multiplicative),
                background=float(source.background))


def log_theta_of(params):
    """[10] float64 host tensor: the logs in the order of PARAM_NAMES."""
    p = params_dict(params)
    vals = [p["adu_per_nmgy"]] + p["psf_params"] + [p["noise_multiplicative"],
                                                    p["noise_additive"], p["background"]]
    bad = [n for n, v in zip(PARAM_NAMES, vals) if not (v > 0 and math.isfinite(v))]
    if bad:
        raise ValueError(f"params: {bad} must be finite and > 0 (the fit works in their logs)")
    return torch.tensor([math.log(v) for v in vals], dtype=torch.float64)


def params_of(log_theta, extra=None):
    """params.pkl's form from [10] logs; `extra` keeps the other keys of a dict."""
    v = [math.exp(float(t)) for t in log_theta]
    out = dict(extra or {})
    out.update(adu_per_nmgy=v[0], psf_params=v[1:7], noise_multiplicative=v[7],
               noise_additive=v[8], background=v[9])
    return out


def _free_index(free):
    free = tuple(free)
    unknown = [n for n in free if n not in PARAM_NAMES]
    if unknown:
        raise ValueError(f"free: unknown parameter(s) {unknown}; the names are {PARAM_NAMES}")
    if len(set(free)) != len(free) or not free:
        raise ValueError(f"free: {free} must name at least one parameter, each once")
    return [PARAM_NAMES.index(n) for n in free]


@dataclass
class FitObjective:
    """nll [] , grad [10], information [10,10]: float64 device tensors in the
    logs of PARAM_NAMES; rate [F,H,W] float32 or None."""
    nll: torch.Tensor
    grad: torch.Tensor
    information: torch.Tensor
    rate: Optional[torch.Tensor]


class _Fields:
    """The checked inputs of a fit, converted once."""

    def __init__(self, images, locs, fluxes, psf_radius, mask, counts, where):
        for name, t in (("images", images), ("locs", locs), ("fluxes", fluxes), ("mask", mask),
                        ("counts", counts)):
            if t is None and name in ("mask", "counts"):
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{where}: {name} must be a torch.Tensor")
        if images.dim() == 2:
            images, locs, fluxes = images[None], locs[None], fluxes[None]
            mask = None if mask is None else mask[None]
        if images.dim() != 3:
            raise ValueError(f"{where}: images must be [F,H,W] or [H,W], got {tuple(images.shape)}")
        F, H, W = images.shape
        if fluxes.dim() != 2 or fluxes.shape[0] != F:
            raise ValueError(f"{where}: fluxes must be [F,D] with F = {F}, got "
                             f"{tuple(fluxes.shape)}")
        D = fluxes.shape[1]
        if tuple(locs.shape) != (F, D, 2):
            raise ValueError(f"{where}: locs must be [{F},{D},2], got {tuple(locs.shape)}")
        if mask is not None and tuple(mask.shape) != (F, H, W):
            raise ValueError(f"{where}: mask must be [{F},{H},{W}], got {tuple(mask.shape)}")
        if counts is not None and tuple(counts.shape) != (F,):
            raise ValueError(f"{where}: counts must be [{F}], got {tuple(counts.shape)}")
        psf_radius = int(psf_radius)
        if not 0 <= psf_radius <= _hip.MAX_PSF_RADIUS:
            raise ValueError(f"{where}: psf_radius {psf_radius} outside 0..{_hip.MAX_PSF_RADIUS}")
        if F < 1 or H < 1 or W < 1 or F * H * W > 2 ** 31 - 1 or F * D > 2 ** 31 - 1:
            raise ValueError(f"{where}: F={F} H={H} W={W} D={D}: F, H, W >= 1 and F*H*W, F*D <= "
                             "2^31-1")
        if D and not bool((torch.isfinite(fluxes) & (fluxes >= 0)).all()):
            raise ValueError(f"{where}: fluxes must be finite and >= 0")
        if D and not bool(torch.isfinite(locs).all()):
            raise ValueError(f"{where}: locs must be finite")
        nb = _hip.FIT_BLOCK
        if F * ((H + nb - 1) // nb) * ((W + nb - 1) // nb) > _hip.FIT_MAX_BLOCKS:
            raise ValueError(f"{where}: F={F} fields of {H}x{W} are more than "
                             f"{_hip.FIT_MAX_BLOCKS} blocks of {nb}x{nb} pixels")
        for name, t in (("images", images), ("locs", locs), ("fluxes", fluxes), ("mask", mask),
                        ("counts", counts)):
            if t is not None and not t.is_cuda:
                raise RuntimeError(f"{where}: {name} must live on a HIP device (got {t.device}); "
                                   "smcdet_amd runs only on MI355X (gfx950)")
        self.images = images.to(torch.float32).contiguous()
        self.locs = locs.to(torch.float32).contiguous()
        self.fluxes = fluxes.to(torch.float32).contiguous()
        self.mask = None if mask is None else (mask != 0).to(torch.uint8).contiguous()
        self.counts = None if counts is None else counts.to(torch.int32).contiguous()
        self.F, self.H, self.W, self.D, self.R = F, H, W, D, psf_radius
        self.ws_doubles = (_hip.FIT_NORM_BLOCKS * _hip.FIT_NORM_SUMS
                           + _hip.FIT_TERMS * F * ((H + nb - 1) // nb) * ((W + nb - 1) // nb))
        self.workspace = torch.empty(self.ws_doubles, device=images.device, dtype=torch.float64)

    def call(self, log_theta, rate=False):
        """One smcdet_fit_objective launch sequence; log_theta: 10 host floats."""
        dev = self.images.device
        theta = (_hip.c_d * _hip.FIT_PARAMS)(*[float(t) for t in log_theta])
        # nll, grad and information in one buffer: one read-back of 111 float64
        out = torch.empty(1 + _hip.FIT_PARAMS + _hip.FIT_PARAMS ** 2, device=dev,
                          dtype=torch.float64)
        nll, grad, info = out[0:1], out[1:11], out[11:]
        r = torch.empty(self.F, self.H, self.W, device=dev, dtype=torch.float32) if rate else None
        check(lib().smcdet_fit_objective(
            theta, ptr(self.images), ptr(self.mask), ptr(self.locs) if self.D else None,
            ptr(self.fluxes) if self.D else None, ptr(self.counts), self.F, self.H, self.W, self.D,
            self.R, ptr(nll), ptr(grad), ptr(info), ptr(r), ptr(self.workspace), self.ws_doubles,
            stream_of(self.images)), "smcdet_fit_objective")
        return out, r


def objective(images, locs, fluxes, params, *, psf_radius, mask=None, counts=None, rate=False):
    """The fit's objective at `params` (a dict in params.pkl's form, an
    M71ImageModel, or a [10] vector of logs in the order of PARAM_NAMES) for
    images [F,H,W] (or one [H,W]), locs [F,D,2], fluxes [F,D] >= 0, mask [F,H,W]
    (non-zero: the pixel counts), counts [F].  Returns a FitObjective."""
    f = _Fields(images, locs, fluxes, psf_radius, mask, counts, "objective")
    if isinstance(params, (torch.Tensor, np.ndarray, list, tuple)):
        lt = torch.as_tensor(params, dtype=torch.float64).reshape(-1).cpu()
        if lt.numel() != _hip.FIT_PARAMS:
            raise ValueError(f"objective: a vector of logs must hold {_hip.FIT_PARAMS} values")
    else:
        lt = log_theta_of(params)
    out, r = f.call(lt.tolist(), rate)
    return FitObjective(out[0], out[1:11], out[11:].reshape(_hip.FIT_PARAMS, _hip.FIT_PARAMS), r)


def free_covariance(information, idx):
    """(covariance [k,k], stderr [k], unidentified positions) of the free block
    of a [10,10] information (float64 numpy).  The logs are dimensionless, so
    the block's eigenvalues compare as they are: one below UNIDENTIFIED_RTOL
    times the largest (or a block that is not finite) marks every free
    parameter with a squared weight above UNIDENTIFIED_WEIGHT in its
    eigenvector as unidentified: NaN in its row, column and stderr.  The rest
    is inverted without them, scaled to unit diagonal first."""
    A = np.asarray(information, dtype=np.float64)[np.ix_(idx, idx)]
    k = len(idx)
    bad = np.zeros(k, dtype=bool)
    if np.all(np.isfinite(A)):
        w, V = np.linalg.eigh(A)
        for e in np.flatnonzero(~(w > UNIDENTIFIED_RTOL * w[-1])):
            bad |= V[:, e] ** 2 > UNIDENTIFIED_WEIGHT
    else:
        bad[:] = True
    cov = np.full((k, k), np.nan)
    ok = np.flatnonzero(~bad)
    if ok.size:
        s = 1.0 / np.sqrt(np.diag(A)[ok])
        inv = np.linalg.inv(A[np.ix_(ok, ok)] * s[:, None] * s[None, :]) * s[:, None] * s[None, :]
        cov[np.ix_(ok, ok)] = inv
    return cov, np.sqrt(np.diag(cov)), [int(i) for i in np.flatnonzero(bad)]


@dataclass
class ModelFit:
    """The result of `fit_image_model`.  params: params.pkl's form; log_theta
    [10], grad [10], information [10,10] float64 host tensors in the logs of
    PARAM_NAMES (fixed parameters included); free: the fitted names;
    covariance [k,k] and stderr [k] of the free logs (a relative error each);
    unidentified: the free names whose information is numerically singular
    (NaN there); rate [F,H,W] float32 on the device."""
    params: dict
    log_theta: torch.Tensor
    nll: float
    grad: torch.Tensor
    information: torch.Tensor
    free: Tuple[str, ...]
    covariance: torch.Tensor
    stderr: torch.Tensor
    unidentified: Tuple[str, ...]
    n_evals: int
    converged: bool
    rate: Optional[torch.Tensor]

    def image_model(self, image_height, image_width, psf_radius):
        """The fitted M71ImageModel for tiles of this size."""
        from .images import M71ImageModel
        p = self.params
        return M71ImageModel(image_height=image_height, image_width=image_width,
                             background=p["background"], psf_radius=psf_radius,
                             adu_per_nmgy=p["adu_per_nmgy"], psf_params=p["psf_params"],
                             noise_additive=p["noise_additive"],
                             noise_multiplicative=p["noise_multiplicative"])


def lbfgs_minimise(z, closure, *, max_iter, steps, tolerance_grad=1e-7, tolerance_change=1e-9):
    """Up to `steps` calls of torch.optim.LBFGS.step (strong Wolfe) on the leaf
    tensor z with at most max_iter iterations and max_iter * 5 // 4 evaluations
    each; closure() sets z.grad and returns the loss.  True when a step ended
    on tolerance_grad or tolerance_change, that is, before either cap."""
    max_iter = int(max_iter)
    max_eval = max(max_iter * 5 // 4, 1)
    opt = torch.optim.LBFGS([z], max_iter=max_iter, max_eval=max_eval,
                            tolerance_grad=tolerance_grad, tolerance_change=tolerance_change,
                            line_search_fn="strong_wolfe")
    for _ in range(int(steps)):
        st = opt.state[z]
        it0, ev0 = st.get("n_iter", 0), st.get("func_evals", 0)
        opt.step(closure)
        st = opt.state[z]
        if st["n_iter"] - it0 < max_iter and st["func_evals"] - ev0 < max_eval:
            return True
    return False


def fit_image_model(images, locs, fluxes, init, *, psf_radius, mask=None, counts=None,
                    free=DEFAULT_FREE, max_iter=500, steps=10, tolerance_grad=1e-7,
                    tolerance_change=1e-9):
    """Minimise the objective over the logs of the `free` parameters from
    `init` (a dict in params.pkl's form or an M71ImageModel; the other
    parameters stay there): up to `steps` calls of torch.optim.LBFGS.step with
    max_iter iterations each and the strong-Wolfe line search, as the
    notebook.  converged: a step ended on one of the tolerances, not on its
    iteration or evaluation cap.  Returns a ModelFit."""
    idx = _free_index(free)
    f = _Fields(images, locs, fluxes, psf_radius, mask, counts, "fit_image_model")
    base = log_theta_of(init)
    z = base[idx].clone().requires_grad_(True)
    n_evals = 0

    def full(zv):
        lt = base.clone()
        lt[idx] = zv.detach()
        return lt

    def closure():
        nonlocal n_evals
        lt = full(z)
        out, _ = f.call(lt.tolist())
        host = out.cpu()  # the one read-back: nll, grad, information
        n_evals += 1
        if not bool(torch.isfinite(host[:11]).all()):
            raise FloatingPointError(
                "fit_image_model: the objective is not finite at log_theta = "
                f"{dict(zip(PARAM_NAMES, lt.tolist()))}")
        z.grad = host[1:11][idx].clone()
        return host[0]

    converged = lbfgs_minimise(z, closure, max_iter=max_iter, steps=steps,
                               tolerance_grad=tolerance_grad, tolerance_change=tolerance_change)
    lt = full(z)
    out, rate = f.call(lt.tolist(), rate=True)
    host = out.cpu()
    n_evals += 1
    info = host[11:].reshape(_hip.FIT_PARAMS, _hip.FIT_PARAMS).clone()
    cov, se, bad = free_covariance(info.numpy(), idx)
    extra = {k: v for k, v in init.items() if k != "psf_params"} if isinstance(init, dict) else None
    return ModelFit(params=params_of(lt, extra), log_theta=lt, nll=float(host[0]),
                    grad=host[1:11].clone(), information=info, free=tuple(free),
                    covariance=torch.from_numpy(cov), stderr=torch.from_numpy(se),
                    unidentified=tuple(tuple(free)[i] for i in bad), n_evals=n_evals,
                    converged=converged, rate=rate)
