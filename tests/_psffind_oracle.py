"""Float64 numpy oracle of smcdet_psf_find and smcdet_psf_recentre and of the
loop smcdet_amd.psffind.find runs around them, written from the definitions
in include/smcdet_hip.h, with the first-order bounds the GPU
tests allow.

`profile_dtype`: float64 is the oracle; float32 emulates the kernel's profile
rounding (the argument formed in float32 as render.h forms it, the profile
rounded to float32), which is what the bounds allow for:

    eps_c = E (sum_p phi_pc (|r_p| + M_p) / v_p + |a_c|) / sqrt(d_c) + 2^-24 |snr_c|

to first order in a relative error E = 32 * 2^-24 per phi (the E of §18.5),
M_p = g sum_k |f_k| phi_pk the subtracted model's share of r.

The definitions (include/smcdet_hip.h):

- A problem is one image x[H,W] with one list of n ≤ K sources (`counts [T,G]`, `locs [T,G,K,2]`, `fluxes [T,G,K]` float32 nmgy). The G lists share the image. This is the layout of `extract_grid` and `forced_photometry`. A null list means n = 0.
- B is the model's background or a per-image `background [T]` > 0. g is `adu_per_nmgy`.
- The Poisson `ImageModel` is taken as Gaussian with na = 0, nm = 1, g = 1, as `photometry` does.
- φ_pk is the render's own float32 profile: `psf_raw`·`psf_scale` of `device.h`, the argument formed as in `render.h`. It is non-zero only in the (2R+1)² window anchored at floor(loc), clipped to the image. It is widened to float64 before use. Everything after is float64 with fixed summation order.
- Variance from the data: v_p = na + nm·max(x_p, B/4). This is the first iteration of `smcdet_forced_photometry`, independent of the list.
- A listed source counts if its slot is below the count and its location and flux are finite. Other slots are ignored: not subtracted, never moved, never excluding.
- Residual: r_p = x_p − B − g·Σ_k f_k φ_pk over the counted sources.
- For a candidate position c: a_c = Σ_p φ_pc r_p / v_p and d_c = Σ_p φ_pc² / v_p over its clipped window.
  - f̂_c = a_c / (g·d_c) is the ML flux of one more source at c with everything else held.
  - snr_c = a_c / √d_c, rounded once to float32.
  - A candidate inside the image always has d_c > 0. A candidate with d_c = 0 has snr −inf.
"""
from typing import NamedTuple

import numpy as np

import _photometry_oracle as P
from _photometry_oracle import columns, model_of, noisy, render, solve_one  # noqa: F401

E = P.E
F32 = np.float32


def phi(m, locs, profile_dtype=np.float64):
    """[H*W, n] profiles of the float32 positions locs [n,2] (finite), zero
    outside each (2R+1)^2 window; float64: P.columns's values."""
    locs = np.asarray(locs, F32).reshape(-1, 2)
    ph, pw = np.divmod(np.arange(m.H * m.W), m.W)
    h, w = locs[:, 0], locs[:, 1]
    fh, fw = np.floor(h.astype(np.float64)), np.floor(w.astype(np.float64))
    inside = (np.abs(ph[:, None] - fh[None]) <= m.R) & (np.abs(pw[:, None] - fw[None]) <= m.R)
    if np.dtype(profile_dtype) == np.float64:
        r2 = (ph[:, None] + 0.5 - h.astype(np.float64)[None]) ** 2 + \
            (pw[:, None] + 0.5 - w.astype(np.float64)[None]) ** 2
        val = P.profile(m, r2)
    else:
        dh = (ph.astype(F32) + F32(0.5))[:, None] - h[None]
        dw = (pw.astype(F32) + F32(0.5))[:, None] - w[None]
        r2 = (dh.astype(np.float64) ** 2 + (dw * dw).astype(np.float64)).astype(F32)  # the fma
        val = P.profile(m, r2.astype(np.float64)).astype(F32).astype(np.float64)
    return np.where(inside, val, 0.0)


class Residual(NamedTuple):
    r: np.ndarray        # [HW] x - B - g sum f phi over the counted sources
    v: np.ndarray        # [HW] na + nm max(x, B/4)
    M: np.ndarray        # [HW] g sum |f| phi
    counted: np.ndarray  # slots that count
    cols: np.ndarray     # [HW, len(counted)] their profiles


def residual(m, x, count, locs, fluxes, background=None, profile_dtype=np.float64):
    """The residual of one problem: x [H,W]; locs [K,2], fluxes [K] or None."""
    B = float(m.background if background is None else F32(background))
    x = np.asarray(x, F32).astype(np.float64).reshape(-1)
    v = m.na + m.nm * np.maximum(x, 0.25 * B)
    if locs is None:
        locs, fluxes, count = np.zeros((0, 2), F32), np.zeros(0, F32), 0
    locs = np.asarray(locs, F32).reshape(-1, 2)
    fluxes = np.asarray(fluxes, F32).reshape(-1)
    K = len(locs)
    n = int(min(max(count, 0), K))
    counted = np.array([k for k in range(n)
                        if np.all(np.isfinite(locs[k])) and np.isfinite(fluxes[k])], int)
    cols = phi(m, locs[counted], profile_dtype)
    f = fluxes[counted].astype(np.float64)
    return Residual(x - B - m.g * (cols @ f), v, m.g * (cols @ np.abs(f)), counted, cols)


class Stats(NamedTuple):
    snr: np.ndarray    # float64, before the rounding to float32 (-inf where d = 0)
    fhat: np.ndarray   # a / (g d)
    eps: np.ndarray    # the bound on |snr_gpu - snr|
    feps: np.ndarray   # the bound on |fhat_gpu - fhat|
    a: np.ndarray
    d: np.ndarray
    a_abs: np.ndarray  # sum |phi r| / v: the scale of a's roundings


def stats(m, r, v, M, pos, profile_dtype=np.float64, chunk=2048):
    """a, d, snr, f-hat and their bounds for the candidates pos [n,2].  To first
    order in E per phi: |da| <= E sum phi (|r| + M) / v, |dd| <= 2 E d, so
    |d snr| <= (|da| + E |a|) / sqrt(d) and |d fhat| <= |da| / (g d) + 2 E |fhat|;
    plus the rounding to float32 and the float64 sums' own order."""
    pos = np.asarray(pos, F32).reshape(-1, 2)
    a, d, a_abs, m_abs = (np.empty(len(pos)) for _ in range(4))
    for i in range(0, len(pos), chunk):
        c = phi(m, pos[i:i + chunk], profile_dtype)
        a[i:i + chunk] = c.T @ (r / v)
        d[i:i + chunk] = (c * c).T @ (1.0 / v)
        a_abs[i:i + chunk] = c.T @ (np.abs(r) / v)
        m_abs[i:i + chunk] = c.T @ (M / v)
    u64 = (len(r) + 8) * 2.0 ** -53
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = np.where(d == 0, -np.inf, a / np.sqrt(d))
        fhat = a / (m.g * d)
        da = E * (a_abs + m_abs) + u64 * a_abs
        eps = (da + E * np.abs(a)) / np.sqrt(d) + 2.0 ** -24 * np.abs(snr)
        feps = da / (m.g * d) + (2 * E + 2.0 ** -24) * np.abs(fhat)
    return Stats(snr, fhat, eps, feps, a, d, a_abs)


def cell_centres(m, c):
    """([cH*cW, 2] float64 centres, cH, cW) of the candidate grid."""
    cH, cW = c * m.H, c * m.W
    i, j = np.divmod(np.arange(cH * cW), cW)
    return np.stack([(i + 0.5) / c, (j + 0.5) / c], 1), cH, cW


def significance_map(m, x, count=0, locs=None, fluxes=None, background=None, cells=2,
                     profile_dtype=np.float64):
    """(snr [cH,cW] float64, eps [cH,cW], Stats, Residual) of one problem."""
    res = residual(m, x, count, locs, fluxes, background, profile_dtype)
    ctr, cH, cW = cell_centres(m, cells)
    st = stats(m, res.r, res.v, res.M, ctr.astype(F32), profile_dtype)
    return st.snr.reshape(cH, cW), st.eps.reshape(cH, cW), st, res


def vertex(sm, s0, sp):
    """The clamped vertex of the parabola through three float32 values (given
    as floats), 0 where it is not concave."""
    den = (float(sm) - 2.0 * float(s0)) + float(sp)
    if not den < 0.0:
        return 0.0
    return min(max(0.5 * (float(sm) - float(sp)) / den, -0.5), 0.5)


def vertex_bound(sm, s0, sp, em, e0, ep):
    """First-order bound on the vertex's error from its three values' bounds:
    d delta = ((1/2 - delta) d s- + 2 delta d s0 - (1/2 + delta) d s+) / den.  inf
    where the sign of den is within the bounds (the first order says nothing)."""
    den = (float(sm) - 2.0 * float(s0)) + float(sp)
    if abs(den) <= 2.0 * (em + 2.0 * e0 + ep):
        return np.inf
    if not den < 0.0:
        return 0.0
    dl = 0.5 * (float(sm) - float(sp)) / den
    return (abs(0.5 - dl) * em + 2.0 * abs(dl) * e0 + abs(0.5 + dl) * ep) / abs(den)


def select_peaks(smap, cells, thresh, nms_radius, min_sep, src_locs, cap, eps=None):
    """The peak rule, ordering, cap and refinement applied to a float32 map
    [cH,cW].  src_locs: [ns,2] float32, the counted sources.  Returns (n_found,
    flat cells of the first `cap`, their refined float32 locs [.,2], the
    first-order bounds on the refined locs in pixels (None without eps))."""
    smap = np.asarray(smap, F32)
    cH, cW = smap.shape
    thresh = F32(thresh)
    q = int(nms_radius)
    src = np.asarray(src_locs, F32).astype(np.float64).reshape(-1, 2)
    peaks = []
    for i, j in zip(*np.nonzero(smap >= thresh)):
        v, x = smap[i, j], i * cW + j
        ok = True
        for ii in range(max(i - q, 0), min(i + q, cH - 1) + 1):
            for jj in range(max(j - q, 0), min(j + q, cW - 1) + 1):
                y, u = ii * cW + jj, smap[ii, jj]
                if y != x and not (v > u or (v == u and x < y)):
                    ok = False
        ch, cw = (i + 0.5) / cells, (j + 0.5) / cells
        for h, w in src:
            if not max(abs(ch - h), abs(cw - w)) > min_sep:
                ok = False
        if ok:
            peaks.append((-float(v), int(x)))
    peaks.sort()
    chosen = [x for _, x in peaks[:max(cap, 0)]]
    locs = np.empty((len(chosen), 2), F32)
    tol = None if eps is None else np.zeros((len(chosen), 2))
    for o, x in enumerate(chosen):
        i, j = divmod(x, cW)
        di = vertex(smap[i - 1, j], smap[i, j], smap[i + 1, j]) if 0 < i < cH - 1 else 0.0
        dj = vertex(smap[i, j - 1], smap[i, j], smap[i, j + 1]) if 0 < j < cW - 1 else 0.0
        locs[o] = (F32(((i + 0.5) + di) / cells), F32(((j + 0.5) + dj) / cells))
        if eps is not None:
            if 0 < i < cH - 1:
                tol[o, 0] = vertex_bound(smap[i - 1, j], smap[i, j], smap[i + 1, j],
                                         eps[i - 1, j], eps[i, j], eps[i + 1, j]) / cells
            if 0 < j < cW - 1:
                tol[o, 1] = vertex_bound(smap[i, j - 1], smap[i, j], smap[i, j + 1],
                                         eps[i, j - 1], eps[i, j], eps[i, j + 1]) / cells
    return len(peaks), chosen, locs, tol


def find_one(m, x, count, locs, fluxes, K, thresh, nms_radius, min_sep, background=None, cells=2,
             profile_dtype=np.float64):
    """smcdet_psf_find on one problem: a dict of counts_out, locs_out [K,2],
    snr_out [K], flux_hat [K], n_found, map, eps."""
    snr, eps, st, res = significance_map(m, x, count, locs, fluxes, background, cells,
                                         profile_dtype)
    n = 0 if locs is None else int(min(max(count, 0), K))
    given = np.full((K, 2), np.nan, F32) if locs is None else np.asarray(locs, F32).reshape(K, 2)
    smap = snr.astype(F32)
    src = given[res.counted] if len(res.counted) else np.zeros((0, 2), F32)
    n_found, chosen, new, _ = select_peaks(smap, cells, thresh, nms_radius, min_sep, src, K - n)
    out = dict(counts_out=n + len(chosen), locs_out=np.full((K, 2), np.nan, F32),
               snr_out=np.full(K, np.nan, F32), flux_hat=np.full(K, np.nan, F32), n_found=n_found,
               map=smap, eps=eps, cells=chosen, stats=st, counted=res.counted)
    out["locs_out"][:n] = given[:n]
    for o, xc in enumerate(chosen):
        out["locs_out"][n + o] = new[o]
        out["snr_out"][n + o] = smap.reshape(-1)[xc]
        out["flux_hat"][n + o] = st.fhat[xc]
    return out


def recentre_one(m, x, count, locs, fluxes, half, step, background=None,
                 profile_dtype=np.float64):
    """smcdet_psf_recentre on one problem: locs_out [K,2], snr_out [K], and
    per counted slot k `cand[k]` = (snr float64 [nc], eps [nc], chosen index,
    loc bound [2] in pixels)."""
    locs = np.asarray(locs, F32).reshape(-1, 2)
    fluxes = np.asarray(fluxes, F32).reshape(-1)
    K = len(locs)
    res = residual(m, x, count, locs, fluxes, background, profile_dtype)
    side = 2 * half + 1
    oa, ob = np.divmod(np.arange(side * side), side)
    oa, ob = oa - half, ob - half
    out = dict(locs_out=locs.copy(), snr_out=np.full(K, np.nan, F32), cand={})
    for i, k in enumerate(res.counted):
        gf = m.g * float(fluxes[k])
        rk = res.r + gf * res.cols[:, i]
        Mk = res.M + abs(gf) * res.cols[:, i]
        pos = np.stack([(float(locs[k, 0]) + oa * step).astype(F32),
                        (float(locs[k, 1]) + ob * step).astype(F32)], 1)
        st = stats(m, rk, res.v, Mk, pos, profile_dtype)
        c = st.snr.astype(F32)
        best = 0
        for q in range(1, len(c)):
            if c[q] > c[best]:
                best = q
        ia, ib = divmod(best, side)
        da = db = ta = tb = 0.0
        if 0 < ia < side - 1:
            da = vertex(c[best - side], c[best], c[best + side])
            ta = vertex_bound(c[best - side], c[best], c[best + side], st.eps[best - side],
                              st.eps[best], st.eps[best + side])
        if 0 < ib < side - 1:
            db = vertex(c[best - 1], c[best], c[best + 1])
            tb = vertex_bound(c[best - 1], c[best], c[best + 1], st.eps[best - 1], st.eps[best],
                              st.eps[best + 1])
        out["locs_out"][k] = (F32(float(locs[k, 0]) + ((ia - half) + da) * step),
                              F32(float(locs[k, 1]) + ((ib - half) + db) * step))
        out["snr_out"][k] = c[best]
        out["cand"][int(k)] = (st.snr, st.eps, best, np.array([ta, tb]) * step)
    return out


class Found(NamedTuple):
    count: int
    locs: np.ndarray      # [K,2] float32, NaN past the count
    fluxes: np.ndarray    # [K] float32, 0 past the count
    flux_err: np.ndarray  # [K] float64, NaN past the count
    snr: np.ndarray       # [K] float32, NaN past the count
    n_found: int          # of the last round's find
    status: int
    first_locs: np.ndarray  # the first round's refined peaks [., 2]


def find(m, x, thresh, nms_radius=1, min_snr=3.0, cells=2, rounds=3, sweeps=4, step=0.25, half=2,
         min_sep=0.5, max_detections=16, background=None, profile_dtype=np.float64):
    """The loop of smcdet_amd.psffind.find on one image: per round one find,
    sweeps x (a 4-iteration flux solve, one recentre), one more solve, and the
    prune that keeps flux / flux_err >= min_snr (a stable compaction)."""
    K = max_detections
    count = 0
    locs = np.full((K, 2), np.nan, F32)
    fluxes = np.zeros(K, F32)
    err = np.full(K, np.nan)
    snr = np.full(K, np.nan, F32)
    n_found = status = 0
    first = None
    for _ in range(rounds):
        f = find_one(m, x, count, locs, fluxes, K, thresh, nms_radius, min_sep, background, cells,
                     profile_dtype)
        n_found = f["n_found"]
        if first is None:
            first = f["locs_out"][:f["counts_out"]].copy()
        count, locs = f["counts_out"], f["locs_out"]
        for _ in range(sweeps):
            s = _solve(m, x, count, locs, background, profile_dtype)
            fluxes = s["fluxes"].astype(F32)
            rc = recentre_one(m, x, count, locs, fluxes, half, step, background, profile_dtype)
            locs, snr = rc["locs_out"], rc["snr_out"]
        s = _solve(m, x, count, locs, background, profile_dtype)
        status = s["status"]
        with np.errstate(invalid="ignore", divide="ignore"):
            keep = (np.arange(K) < count) & np.isfinite(s["fluxes"]) & \
                np.isfinite(s["flux_err"]) & (s["fluxes"] / s["flux_err"] >= min_snr)
        idx = np.nonzero(keep)[0]
        count = len(idx)
        nl, nf = np.full((K, 2), np.nan, F32), np.zeros(K, F32)
        ne, nsn = np.full(K, np.nan), np.full(K, np.nan, F32)
        nl[:count], nf[:count] = locs[idx], s["fluxes"][idx].astype(F32)
        ne[:count], nsn[:count] = s["flux_err"][idx], snr[idx]
        locs, fluxes, err, snr = nl, nf, ne, nsn
    return Found(count, locs, fluxes, err, snr, n_found, status, first)


def _solve(m, x, count, locs, background, profile_dtype):
    """solve_one with its profile in profile_dtype (solve_one calls
    P.columns; float32 swaps the emulated profile in for the call)."""
    if np.dtype(profile_dtype) == np.float64:
        return solve_one(m, x, count, locs, background)
    keep = P.columns
    P.columns = lambda mm, ll: phi(mm, ll, profile_dtype)
    try:
        return solve_one(m, x, count, locs, background)
    finally:
        P.columns = keep


def match(true_locs, found_locs, tol=0.5):
    """Greedy one-to-one matching within `tol` (Chebyshev): (pairs (true,
    found), unmatched found indices)."""
    true_locs = np.asarray(true_locs, np.float64).reshape(-1, 2)
    found_locs = np.asarray(found_locs, np.float64).reshape(-1, 2)
    free = list(range(len(found_locs)))
    pairs = []
    for i, t in enumerate(true_locs):
        best, bd = None, tol
        for j in free:
            d = np.max(np.abs(found_locs[j] - t))
            if d <= bd:
                best, bd = j, d
        if best is not None:
            pairs.append((i, best))
            free.remove(best)
    return pairs, free


def separated_set(m, seed=5, tiles=40, min_dist=4.0):
    """The separated set of DESIGN.md §19.4: per tile n uniform in 1..3, positions
    uniform in [0.5, 7.5]^2 redrawn until all pairwise Euclidean distances >=
    min_dist, fluxes log-uniform in 20..200, then `noisy`, all from one
    generator.  Returns [(x float32 [H,W], locs [n,2], fluxes [n])]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(tiles):
        n = int(rng.integers(1, 4))
        while True:
            locs = rng.uniform(0.5, 7.5, (n, 2))
            d = np.linalg.norm(locs[:, None] - locs[None], axis=-1)[np.triu_indices(n, 1)]
            if np.all(d >= min_dist):
                break
        fl = np.exp(rng.uniform(np.log(20.0), np.log(200.0), n))
        locs = locs.astype(F32)
        out.append((noisy(m, render(m, locs, fl), rng), locs, fl))
    return out
