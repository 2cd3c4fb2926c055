"""Float64 numpy oracle of smcdet_forced_photometry, written from the
definition in include/smcdet_hip.h in the gather form (every pixel gathers
the sources whose window holds it), plus the terms of the tests' error bounds
(DESIGN.md §18).  The profile is float64 here and float32 in the kernel: that
difference is what the bounds allow for."""
from typing import NamedTuple

import numpy as np

E = 32 * 2.0 ** -24          # relative error allowed on every term of the normal equations
PIVOT_MIN = 1e-8
CONFIG_TILE = 8

# the five 8x8 M71 configurations of the calibration and GPU tests:
# name -> (locs [n,2], fluxes [n] in nmgy)
CONFIGS = {
    "isolated": ([(3.7, 4.2)], [50.0]),
    "pair_0p8": ([(3.6, 3.8), (3.6, 4.6)], [60.0, 30.0]),
    "pair_0p3": ([(4.1, 3.9), (4.1, 4.2)], [80.0, 50.0]),
    "three_corner": ([(1.0, 1.0), (4.5, 5.2), (6.3, 2.1)], [40.0, 70.0, 25.0]),
    "padding": ([(-1.5, 3.3)], [150.0]),
}


class OModel(NamedTuple):
    kind: str        # "m71" or "poisson"
    H: int
    W: int
    R: int
    background: float
    g: float
    psf: tuple       # m71: the six parameters; poisson: (psf_stdev,)
    norm: float      # m71: the normalising constant C
    na: float
    nm: float


def _f32(x):
    return float(np.float32(x))


def model_of(im):
    """OModel of a smcdet_amd image model, with the float32 roundings its C
    struct carries."""
    if hasattr(im, "psf_params"):
        return OModel("m71", int(im.image_height), int(im.image_width), int(im.psf_radius),
                      _f32(im.background), _f32(im.adu_per_nmgy),
                      tuple(_f32(v) for v in im.psf_params), float(im.psf_normalizing_constant),
                      _f32(im.noise_additive), _f32(im.noise_multiplicative))
    return OModel("poisson", int(im.image_height), int(im.image_width), int(im.psf_radius),
                  _f32(im.background), 1.0, (_f32(im.psf_stdev),), 1.0, 0.0, 1.0)


def profile(m, r2):
    if m.kind == "m71":
        s1, s2, sp, beta, b, p0 = m.psf
        u = np.exp(-r2 / (2 * s1)) + b * np.exp(-r2 / (2 * s2)) + \
            p0 * (1 + r2 / (beta * sp)) ** (-beta / 2)
        return u / ((1 + b + p0) * m.norm)
    s = m.psf[0]
    return np.exp(-r2 / (2 * s * s)) / (s * np.sqrt(2 * np.pi))


def columns(m, locs):
    """phi [H*W, n] of the float32 positions locs [n,2] (finite)."""
    ph, pw = np.divmod(np.arange(m.H * m.W), m.W)
    locs = np.asarray(locs, np.float32).astype(np.float64).reshape(-1, 2)
    out = np.zeros((m.H * m.W, len(locs)))
    for k, (h, w) in enumerate(locs):
        fh, fw = np.floor(h), np.floor(w)
        inside = (np.abs(ph - fh) <= m.R) & (np.abs(pw - fw) <= m.R)
        r2 = (ph + 0.5 - h) ** 2 + (pw + 0.5 - w) ** 2
        out[:, k] = np.where(inside, profile(m, r2), 0.0)
    return out


def render(m, locs, fluxes, background=None):
    """The noise-free rate [H,W] (float64) of a catalog."""
    B = m.background if background is None else background
    return (B + m.g * columns(m, locs) @ np.asarray(fluxes, np.float64)).reshape(m.H, m.W)


def noisy(m, rate, rng):
    """rate + Normal(0, na + nm rate), rounded to float32."""
    return (rate + np.sqrt(m.na + m.nm * rate) * rng.standard_normal(rate.shape)) \
        .astype(np.float32)


def _unit_cholesky(A):
    """(factor of the unit-diagonal scaling or None, its squared pivots, the scales)."""
    sc = 1.0 / np.sqrt(np.diag(A))
    As = A * sc[:, None] * sc[None, :]
    n = len(A)
    L = np.zeros_like(As)
    piv = np.full(n, np.nan)
    for j in range(n):
        d = As[j, j] - L[j, :j] @ L[j, :j]
        piv[j] = d
        if not d >= PIVOT_MIN:
            return None, piv, sc
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (As[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, piv, sc


def solve_one(m, x, count, locs, background=None, fit_background=False, n_iter=4):
    """One problem: x [H,W], locs [K,2].  Returns a dict with the outputs of
    the definition's point 5 and, for the bounds: `pivots` (every squared
    pivot of every factorisation), `c` [K] (flux bound terms), `err_tol` [K]
    and `cov_tol` [K,K] (flux_err and covariance bounds at E), `chi2_tol`."""
    K = len(locs)
    nan = np.nan
    B = float(m.background if background is None else np.float32(background))
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1)
    locs = np.asarray(locs, np.float32).reshape(K, 2)
    count = int(min(max(count, 0), K))
    out = dict(fluxes=np.zeros(K), flux_err=np.full(K, nan), background=nan, chi2=nan,
               n_pixels=m.H * m.W, n_free=0, status=0, cov=np.full((K, K), nan), pivots=[],
               c=np.full(K, nan), err_tol=np.full(K, nan), chi2_tol=nan,
               cov_tol=np.full((K, K), nan), c_background=nan)
    cand = [k for k in range(count) if np.all(np.isfinite(locs[k]))]
    phi = columns(m, locs[cand]) if cand else np.zeros((len(x), 0))
    free = [k for i, k in enumerate(cand) if np.any(phi[:, i] != 0)]
    keep = [i for i, k in enumerate(cand) if k in free]
    if len(free) < len(cand):
        out["status"] |= 1
    out["fluxes"][cand] = nan
    ns = len(free)
    D = m.g * phi[:, keep]
    if fit_background:
        D = np.concatenate([D, np.ones((len(x), 1))], axis=1)
    P = D.shape[1]
    out["n_free"] = P
    if not (B > 0 and np.isfinite(B)):
        out["status"] |= 4
        return out
    B_fixed = 0.0 if fit_background else B
    y = x - B_fixed
    floor = 0.25 * B
    v = m.na + m.nm * np.maximum(x, floor)
    theta = np.zeros(P)
    for _ in range(n_iter):
        w = 1.0 / v
        A = D.T @ (D * w[:, None])
        b = D.T @ (w * y)
        L, piv, sc = _unit_cholesky(A)
        out["pivots"].extend(piv[np.isfinite(piv)].tolist())
        if L is None:
            out["status"] |= 2
            return out
        z = np.linalg.solve(L, b * sc)
        theta = np.linalg.solve(L.T, z) * sc
        lin = D @ theta
        v = m.na + m.nm * np.maximum(lin + B_fixed, floor)
        w_solve, A_solve = w, A
    wf = 1.0 / v + m.nm ** 2 / (2 * v ** 2)
    info = D.T @ (D * wf[:, None])
    L, piv, sc = _unit_cholesky(info)
    out["pivots"].extend(piv[np.isfinite(piv)].tolist())
    if L is None:
        out["status"] |= 2
        return out
    Li = np.linalg.inv(L)
    cov = (Li.T @ Li) * sc[:, None] * sc[None, :]
    r = y - lin
    out["fluxes"][free] = theta[:ns]
    out["flux_err"][free] = np.sqrt(np.diag(cov))[:ns]
    out["background"] = theta[ns] if fit_background else B
    out["chi2"] = float(np.sum(r * r / v))
    out["cov"][np.ix_(free, free)] = cov[:ns, :ns]
    # ---- the bounds' terms, at the final iteration -----------
    aD = np.abs(D)
    absfit = aD @ np.abs(theta)                       # sum_m |D_pm theta_m|
    s = aD.T @ (w_solve * (np.abs(y) + absfit))       # s_l
    c = np.abs(np.linalg.inv(A_solve)) @ s            # c_k
    out["c"][free] = c[:ns]
    out["c_background"] = c[ns] if fit_background else 0.0
    # d(I^-1) = -I^-1 (dI) I^-1 with |dI_ij| <= E scale(I_ij); twice that, as §17.5
    dcov = 2 * E * (np.abs(cov) @ (aD.T @ (aD * wf[:, None])) @ np.abs(cov))
    out["cov_tol"][np.ix_(free, free)] = dcov[:ns, :ns]
    out["err_tol"][free] = (np.diag(dcov) / (2 * np.sqrt(np.diag(cov))))[:ns]
    # chi2: |d lambda_p| <= E (sum_m |D_pm theta_m| + sum_m |D_pm| c_m); the
    # derivative of r^2 / v in lambda is bounded by 2 |r| / v + nm r^2 / v^2; plus the
    # float64 roundings of a sum of n terms in another order ((n + 8) 2^-53 of it), all
    # there is to differ when nothing is fitted
    dlam = E * (absfit + aD @ c)
    out["chi2_tol"] = float(np.sum((2 * np.abs(r) / v + m.nm * r * r / v ** 2) * dlam)) + \
        (len(x) + 8) * 2.0 ** -53 * out["chi2"]
    return out


def forced_photometry(m, images, counts, locs, background=None, fit_background=False, n_iter=4):
    """images [T,H,W], counts [T,G], locs [T,G,K,2], background [T] or None.
    Returns a dict of arrays shaped [T,G,...]; `pivots` is the flat list over
    all problems."""
    images = np.asarray(images)
    counts = np.asarray(counts)
    locs = np.asarray(locs)
    T, G, K = locs.shape[:3]
    res = [[solve_one(m, images[t], counts[t, g], locs[t, g],
                      None if background is None else background[t], fit_background, n_iter)
            for g in range(G)] for t in range(T)]
    out = {}
    for key in ("fluxes", "flux_err", "background", "chi2", "n_pixels", "n_free", "status",
                "cov", "c", "err_tol", "chi2_tol", "cov_tol", "c_background"):
        out[key] = np.array([[r[key] for r in row] for row in res])
    out["pivots"] = np.array([p for row in res for r in row for p in r["pivots"]])
    return out


def pivots_clear_of_threshold(pivots):
    """No squared pivot inside 1e-12 .. 1e-4: the case does not sit on the
    singularity threshold (1e-8), where float32 and float64 profiles may
    decide differently."""
    pivots = np.asarray(pivots, np.float64)
    return not np.any((pivots > 1e-12) & (pivots < 1e-4))
