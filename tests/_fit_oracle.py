"""Float64 CPU oracle of the image-model fit (smcdet_amd/fit.py),
written from the formulas of include/smcdet_hip.h, in the gather formulation:
every pixel sums the stars whose (2R+1)^2 window, anchored at floor(loc),
holds it.  nll and its gradient come from autograd, the information from the
forward-mode Jacobian of (lambda, v).  Next to every output its absolute-sum
scale, the sum over the pixels of the absolute per-pixel terms:
  nll          sum |log(2 pi v)| / 2 + (x - lambda)^2 / (2 v)
  grad[i]      sum |dnll/dlambda * lambda_i| + |dnll/dv * v_i|
  information  sum |lambda_i lambda_j| / v + |v_i v_j| / (2 v^2)."""
import math

import numpy as np
import torch

NAMES = ("adu_per_nmgy", "sigma1", "sigma2", "sigmap", "beta", "b", "p0",
         "noise_multiplicative", "noise_additive", "background")
P = len(NAMES)
F64 = torch.float64


def log_theta_of(params):
    """[10] float64 logs from a dict in the form of the reference's params.pkl."""
    pp = [float(v) for v in params["psf_params"]]
    vals = [float(params["adu_per_nmgy"])] + pp + [float(params["noise_multiplicative"]),
                                                   float(params["noise_additive"]),
                                                   float(params["background"])]
    return torch.tensor([math.log(v) for v in vals], dtype=F64)


def _profile(r2, th):
    s1, s2, sp, beta, b, p0 = (th[k] for k in range(1, 7))
    t1 = torch.exp(-r2 / (2 * s1))
    t2 = b * torch.exp(-r2 / (2 * s2))
    t3 = p0 * (1 + r2 / (beta * sp)) ** (-beta / 2)
    return (t1 + t2 + t3) / (1 + b + p0)


def _grid_r2(R):
    n = 32 * R
    g = torch.arange(n, dtype=F64) - n / 2.0 + 0.5
    return g[:, None] ** 2 + g[None, :] ** 2


def _geometry(locs, fluxes, counts, H, W, R):
    """r2 [F,H,W,D] and the weights f * [the window holds the pixel] * [d < count]."""
    locs = torch.as_tensor(locs).to(F64)
    fluxes = torch.as_tensor(fluxes).to(F64)
    Fn, D = fluxes.shape
    ph = torch.arange(H, dtype=F64)[None, :, None, None]
    pw = torch.arange(W, dtype=F64)[None, None, :, None]
    h = locs[:, None, None, :, 0]
    w = locs[:, None, None, :, 1]
    r2 = (ph + 0.5 - h) ** 2 + (pw + 0.5 - w) ** 2
    inwin = ((ph - torch.floor(h)).abs() <= R) & ((pw - torch.floor(w)).abs() <= R)
    if counts is None:
        cnt = torch.full((Fn,), D, dtype=torch.int64)
    else:
        cnt = torch.as_tensor(counts).to(torch.int64).clamp(0, D)
    live = torch.arange(D)[None, :] < cnt[:, None]
    wgt = fluxes[:, None, None, :] * inwin * live[:, None, None, :]
    return r2, wgt


def _rate_var(log_theta, r2, wgt, grid_r2):
    th = torch.exp(log_theta)
    g, nm, na, bg = th[0], th[7], th[8], th[9]
    if r2.shape[-1] == 0:
        lam = bg + 0 * g * torch.zeros(r2.shape[:-1], dtype=F64)
    else:
        C = _profile(grid_r2, th).sum()
        lam = bg + g * (wgt * _profile(r2, th)).sum(-1) / C
    return lam, na + nm * lam


def _nll(lam, v, x, m):
    return (m * (0.5 * torch.log(2 * math.pi * v) + (x - lam) ** 2 / (2 * v))).sum()


def evaluate(log_theta, images, locs, fluxes, psf_radius, mask=None, counts=None,
             information=True):
    """dict: nll (float), grad [P], rate [F,H,W] (float64 numpy), scale_nll,
    scale_rate, and with `information`: information [P,P], scale_information
    [P,P], scale_grad [P]."""
    log_theta = torch.as_tensor(log_theta, dtype=F64).clone()
    x = torch.as_tensor(images).to(F64)
    Fn, H, W = x.shape
    m = torch.ones_like(x) if mask is None else (torch.as_tensor(mask) != 0).to(F64)
    r2, wgt = _geometry(locs, fluxes, counts, H, W, psf_radius)
    grid = _grid_r2(psf_radius)
    lt = log_theta.requires_grad_(True)
    lam, v = _rate_var(lt, r2, wgt, grid)
    nll = _nll(lam, v, x, m)
    (grad,) = torch.autograd.grad(nll, lt)
    out = dict(nll=float(nll.detach()), grad=grad.numpy().copy(), rate=lam.detach().numpy().copy())
    lam, v = lam.detach(), v.detach()
    term = 0.5 * torch.log(2 * math.pi * v).abs() + (x - lam) ** 2 / (2 * v)
    out["scale_nll"] = float((m * term).sum())
    out["scale_rate"] = lam.numpy().copy()
    if information:
        J = torch.autograd.functional.jacobian(
            lambda t: torch.stack(_rate_var(t, r2, wgt, grid)), log_theta.detach(),
            vectorize=True, strategy="forward-mode")  # [2,F,H,W,P]
        Jl, Jv = J[0].reshape(-1, P), J[1].reshape(-1, P)
        wl = (m / v).reshape(-1, 1)
        wv = (m / (2 * v * v)).reshape(-1, 1)
        # (not symmetrised: the two triangles differ by the products' rounding)
        out["information"] = ((Jl * wl).T @ Jl + (Jv * wv).T @ Jv).numpy()
        out["scale_information"] = ((Jl.abs() * wl).T @ Jl.abs()
                                    + (Jv.abs() * wv).T @ Jv.abs()).numpy()
        dl = (m * (lam - x) / v).reshape(-1, 1)                          # d nll_p / d lambda
        dv = (m * (0.5 / v - (x - lam) ** 2 / (2 * v * v))).reshape(-1, 1)  # d nll_p / d v
        out["scale_grad"] = ((dl * Jl).abs() + (dv * Jv).abs()).sum(0).numpy()
    return out


def nll_at(log_theta, images, locs, fluxes, psf_radius, mask=None, counts=None):
    return evaluate(log_theta, images, locs, fluxes, psf_radius, mask, counts,
                    information=False)["nll"]


def free_index(free):
    return [NAMES.index(n) for n in free]


def fit(images, locs, fluxes, init_log_theta, psf_radius, mask=None, counts=None,
        free=NAMES[:9], max_iter=500, steps=10, tolerance_grad=1e-7, tolerance_change=1e-9):
    """The oracle's own fit: torch.optim.LBFGS (strong Wolfe) over the free
    logs, the closure by autograd.  dict: log_theta [P], nll, n_evals,
    converged, information [P,P], stderr [len(free)] (float64 numpy)."""
    idx = free_index(free)
    base = torch.as_tensor(init_log_theta, dtype=F64).clone()
    x = torch.as_tensor(images).to(F64)
    Fn, H, W = x.shape
    m = torch.ones_like(x) if mask is None else (torch.as_tensor(mask) != 0).to(F64)
    r2, wgt = _geometry(locs, fluxes, counts, H, W, psf_radius)
    grid = _grid_r2(psf_radius)
    z = base[idx].clone().requires_grad_(True)
    max_eval = max_iter * 5 // 4
    opt = torch.optim.LBFGS([z], max_iter=max_iter, max_eval=max_eval,
                            tolerance_grad=tolerance_grad, tolerance_change=tolerance_change,
                            line_search_fn="strong_wolfe")
    evals = [0]

    def closure():
        opt.zero_grad()
        lt = base.clone()
        lt[idx] = z
        loss = _nll(*_rate_var(lt, r2, wgt, grid), x, m)
        loss.backward()
        evals[0] += 1
        return loss

    converged = False
    for _ in range(steps):
        it0, ev0 = opt.state[z].get("n_iter", 0), opt.state[z].get("func_evals", 0)
        opt.step(closure)
        # a step ends on max_iter, on max_eval, or on one of the tolerances
        if (opt.state[z]["n_iter"] - it0 < max_iter
                and opt.state[z]["func_evals"] - ev0 < max_eval):
            converged = True
            break
    lt = base.clone()
    lt[idx] = z.detach()
    ev = evaluate(lt, images, locs, fluxes, psf_radius, mask, counts)
    block = ev["information"][np.ix_(idx, idx)]
    return dict(log_theta=lt.numpy(), nll=ev["nll"], n_evals=evals[0], converged=converged,
                information=ev["information"], cond=float(np.linalg.cond(block)),
                stderr=np.sqrt(np.diag(np.linalg.inv(block))))


# ---- the recovery case (tests/test_fit_host.py, tests/test_gpu_fit.py) -------------
RECOVERY_FREE = ("adu_per_nmgy", "sigma1", "sigma2", "b", "noise_multiplicative", "background")
RECOVERY_SEED = 7


def recovery_case(truth, seed=RECOVERY_SEED):
    """32x40, psf_radius 8, 16 stars uniform over the field padded by 4 px,
    fluxes log-uniform in 10..1000 nmgy, image = rate + sqrt(v) z rounded to
    float32, a mask without 2 rows, 3 columns and a 4x5 hole, every free log
    started 0.2 from the truth with alternating signs."""
    H, W, R, D = 32, 40, 8, 16
    rng = np.random.default_rng(seed)
    locs = np.stack([rng.uniform(-4, H + 4, D), rng.uniform(-4, W + 4, D)], -1)
    fluxes = np.exp(rng.uniform(np.log(10.0), np.log(1000.0), D))
    locs = locs.astype(np.float32)[None]
    fluxes = fluxes.astype(np.float32)[None]
    lt = log_theta_of(truth)
    r2, wgt = _geometry(locs, fluxes, None, H, W, R)
    lam, v = _rate_var(lt, r2, wgt, _grid_r2(R))
    z = rng.standard_normal((1, H, W))
    image = (lam.numpy() + np.sqrt(v.numpy()) * z).astype(np.float32)
    mask = np.ones((1, H, W), np.uint8)
    mask[0, [5, 20]] = 0
    mask[0, :, [3, 17, 31]] = 0
    mask[0, 10:14, 24:29] = 0
    start = lt.clone()
    for k, i in enumerate(free_index(RECOVERY_FREE)):
        start[i] += 0.2 if k % 2 == 0 else -0.2
    return dict(H=H, W=W, R=R, image=image, locs=locs, fluxes=fluxes, mask=mask,
                truth=lt.numpy(), start=start.numpy(), free=RECOVERY_FREE)


# ---- the cases of tests/test_gpu_fit.py ----------------------------------------------
def m71_truth(noise_additive=None):
    from _params import M71
    return dict(adu_per_nmgy=M71["adu_per_nmgy"], psf_params=list(M71["psf_params"]),
                noise_additive=M71["noise_additive"] if noise_additive is None else noise_additive,
                noise_multiplicative=M71["noise_multiplicative"], background=M71["background"])


def simulate(log_theta, locs, fluxes, counts, H, W, R, rng):
    """image [F,H,W] float32 = rate + sqrt(v) z at log_theta."""
    r2, wgt = _geometry(locs, fluxes, counts, H, W, R)
    lam, v = _rate_var(torch.as_tensor(log_theta, dtype=F64), r2, wgt, _grid_r2(R))
    z = rng.standard_normal(tuple(lam.shape))
    return (lam.numpy() + np.sqrt(v.numpy()) * z).astype(np.float32)


def _stars(rng, Fn, D, H, W, pad=4.0):
    locs = np.stack([rng.uniform(-pad, H + pad, (Fn, D)), rng.uniform(-pad, W + pad, (Fn, D))], -1)
    fluxes = np.exp(rng.uniform(np.log(10.0), np.log(1000.0), (Fn, D)))
    return locs.astype(np.float32), fluxes.astype(np.float32)


def fixture():
    from _params import golden
    return golden("fit_m71_field.npz")


def cases():
    """name -> dict(log_theta, image [F,H,W], locs [F,D,2], fluxes [F,D], R, mask or None,
    counts or None).  The images are simulated at the M71 values with
    noise_additive 30 and evaluated 5 % away from them in every log."""
    rng = np.random.default_rng(17)
    sim = log_theta_of(m71_truth(30.0)).numpy()
    at = sim + 0.05 * np.array([1, -1, 1, -1, 1, -1, 1, -1, 1, -1.0])
    out = {}
    # the 24x40 fixture field, a mask with holes and one fully masked 16x16 pixel block
    d = fixture()
    mask = np.ones((1, 24, 40), np.uint8)
    mask[0, 0:16, 16:32] = 0
    mask[0, 18, :] = 0
    mask[0, 20:23, 3:5] = 0
    mask[0, 17, 39] = 0
    out["fixture_masked"] = dict(log_theta=np.log(d["theta"][1]), image=d["image"][None],
                                 locs=d["locs"][None], fluxes=d["fluxes"][None],
                                 R=int(d["psf_radius"]), mask=mask, counts=None)
    # every window clipped on all sides, dimensions multiples of nothing
    locs, fluxes = _stars(rng, 1, 9, 17, 19, pad=0.0)
    locs[..., 1] = 2.0 + locs[..., 1] * np.float32(15.0 / 19.0)  # columns 2 .. 17: clipped twice
    out["clipped_17x19_R16"] = dict(log_theta=at, locs=locs, fluxes=fluxes, R=16, mask=None,
                                    counts=None,
                                    image=simulate(sim, locs, fluxes, None, 17, 19, 16, rng))
    # a star in the negative padding (floor towards -inf), one on integer coordinates, one
    # whose window misses the field, one with zero flux, and two ordinary ones
    locs = np.array([[[-2.5, 5.3], [-0.5, -0.25], [7.0, 12.0], [40.0, 60.0], [10.2, 20.7],
                      [15.6, 3.1], [3.3, 28.9]]], np.float32)
    fluxes = np.array([[300.0, 150.0, 500.0, 800.0, 0.0, 90.0, 40.0]], np.float32)
    out["edge_stars_20x33_R4"] = dict(log_theta=at, locs=locs, fluxes=fluxes, R=4, mask=None,
                                      counts=None,
                                      image=simulate(sim, locs, fluxes, None, 20, 33, 4, rng))
    # no stars at all
    e = np.zeros((1, 0, 2), np.float32)
    out["no_stars_18x21"] = dict(log_theta=at, locs=e, fluxes=e[..., 0], R=8, mask=None,
                                 counts=None, image=simulate(sim, e, e[..., 0], None, 18, 21, 8,
                                                             rng))
    # 300 stars: past the 256-star LDS chunk
    locs, fluxes = _stars(rng, 1, 300, 40, 56)
    out["stars300_40x56"] = dict(log_theta=at, locs=locs, fluxes=fluxes, R=8, mask=None,
                                 counts=None,
                                 image=simulate(sim, locs, fluxes, None, 40, 56, 8, rng))
    # three fields, ragged counts (one empty), a mask per field
    locs, fluxes = _stars(rng, 3, 7, 20, 24)
    counts = np.array([7, 0, 3], np.int32)
    mask = (rng.uniform(size=(3, 20, 24)) > 0.1).astype(np.uint8)
    out["ragged_3x20x24"] = dict(log_theta=at, locs=locs, fluxes=fluxes, R=5, mask=mask,
                                 counts=counts,
                                 image=simulate(sim, locs, fluxes, counts, 20, 24, 5, rng))
    return out
