"""CPU oracle for smcdet_amd.condense: float64 numpy statements
of the source map, the peaks and their centroids, the per-seed moments, the
derived fields and the quantile rule.  The map's cell index is the float32
expression of include/smcdet_hip.h; the association goes through
tests._metrics_oracle (pair_tables / solve), the exact lexicographic optimum.
"""
import numpy as np
import torch

from tests import _metrics_oracle as MO

F32_MAX = float(np.finfo(np.float32).max)


# ---- source map ---------------------------------------------------------------
def counted_mask(counts, locs, fluxes):
    """[T,N,S] bool: j < clamp(counts, 0, S), finite location, finite flux > 0."""
    S = fluxes.shape[-1]
    c = np.clip(np.asarray(counts).astype(np.int64), 0, S)
    with np.errstate(invalid="ignore"):
        return ((np.arange(S)[None, None, :] < c[:, :, None]) & np.isfinite(locs).all(-1)
                & np.isfinite(fluxes) & (fluxes > 0))


def cells_of(locs, lo, c):
    """float32 cell coordinates (ih, iw) [T,N,S] of every slot, exactly
    floorf((h - lo_h) * (float)c); lo [T,2]."""
    lo = np.asarray(lo, np.float32)[:, None, None, :]
    with np.errstate(invalid="ignore"):
        return np.floor((locs.astype(np.float32) - lo) * np.float32(c))


def source_map(counts, locs, fluxes, lo, c, Gh, Gw, weights=None):
    """dict: count, flux [T,Gh,Gw] float64 (sums of the float32 terms w and
    w * f), outside [T], n_cell [T,Gh,Gw] and n_outside [T] (contributions),
    abs sums being the sums themselves (every term is >= 0).  lo [T,2] lower
    corners.  Asserts that float32 and float64 binning agree."""
    T, N, S = fluxes.shape
    ok = counted_mask(counts, locs, fluxes)
    cell = cells_of(locs, lo, c)
    with np.errstate(invalid="ignore"):
        cell64 = np.floor((locs.astype(np.float64) - np.asarray(lo, np.float64)[:, None, None, :])
                          * c)
    assert np.array_equal(cell[ok], cell64[ok]), "float32 and float64 binning disagree"
    w = np.ones((T, N), np.float32) if weights is None else np.asarray(weights, np.float32)
    w = np.broadcast_to(w[:, :, None], (T, N, S))
    with np.errstate(invalid="ignore"):
        inside = ok & (cell[..., 0] >= 0) & (cell[..., 0] < Gh) & (cell[..., 1] >= 0) & \
            (cell[..., 1] < Gw)
        wf = (w * fluxes.astype(np.float32)).astype(np.float32)  # the float32 product
    count = np.zeros((T, Gh, Gw))
    flux = np.zeros((T, Gh, Gw))
    n_cell = np.zeros((T, Gh, Gw), np.int64)
    t, n, j = np.nonzero(inside)
    ih, iw = cell[t, n, j, 0].astype(np.int64), cell[t, n, j, 1].astype(np.int64)
    np.add.at(count, (t, ih, iw), w[t, n, j].astype(np.float64))
    np.add.at(flux, (t, ih, iw), wf[t, n, j].astype(np.float64))
    np.add.at(n_cell, (t, ih, iw), 1)
    out = ok & ~inside
    return dict(count=count, flux=flux, n_cell=n_cell,
                outside=np.where(out, w, 0).astype(np.float64).sum((1, 2)),
                n_outside=out.sum((1, 2)), n_counted=ok.sum((1, 2)))


# ---- peaks ----------------------------------------------------------------------
def smooth(m, q):
    """Box sum over (2q+1)^2 cells, zero outside the grid; m [Gh,Gw]."""
    Gh, Gw = m.shape
    pad = np.zeros((Gh + 2 * q, Gw + 2 * q))
    pad[q:q + Gh, q:q + Gw] = m
    s = np.zeros((Gh, Gw))
    for di in range(2 * q + 1):
        for dj in range(2 * q + 1):
            s += pad[di:di + Gh, dj:dj + Gw]
    return s


def peaks(m, q, p, min_mass, K, lo=(0.0, 0.0), c=1):
    """Seeds of one tile's map m [Gh,Gw]: (n, cell [K] int32, mass [K] float64,
    locs [K,2] float64), by the definitions of smcdet_map_peaks."""
    m = np.asarray(m, np.float64)
    Gh, Gw = m.shape
    s = smooth(m, q)
    found = []
    for i in range(Gh):
        for j in range(Gw):
            v, x = s[i, j], i * Gw + j
            if not (v >= min_mass and v > 0):
                continue
            good = True
            for ii in range(max(i - p, 0), min(i + p, Gh - 1) + 1):
                for jj in range(max(j - p, 0), min(j + p, Gw - 1) + 1):
                    y = ii * Gw + jj
                    if y != x and not (v > s[ii, jj] or (v == s[ii, jj] and x < y)):
                        good = False
            if good:
                found.append((-v, x))
    found.sort()
    found = found[:K]
    cell = np.full(K, -1, np.int32)
    mass = np.zeros(K)
    locs = np.full((K, 2), np.nan)
    for k, (nv, x) in enumerate(found):
        i, j = divmod(x, Gw)
        i0, i1, j0, j1 = max(i - q, 0), min(i + q, Gh - 1), max(j - q, 0), min(j + q, Gw - 1)
        win = m[i0:i1 + 1, j0:j1 + 1]
        ch = (win * (np.arange(i0, i1 + 1) + 0.5)[:, None]).sum() / win.sum()
        cw = (win * (np.arange(j0, j1 + 1) + 0.5)[None, :]).sum() / win.sum()
        cell[k], mass[k] = x, -nv
        locs[k] = lo[0] + ch / c, lo[1] + cw / c
    return len(found), cell, mass, locs


def find_seeds(count_map, q, p, min_mass, K, lo, c):
    """peaks() over the tiles: n [T], cell [T,K], mass [T,K], locs [T,K,2];
    min_mass [T], lo [T,2]."""
    res = [peaks(count_map[t], q, p, float(min_mass[t]), K, lo[t], c)
           for t in range(count_map.shape[0])]
    return (np.array([r[0] for r in res], np.int32), np.stack([r[1] for r in res]),
            np.stack([r[2] for r in res]), np.stack([r[3] for r in res]))


# Hand-worked maps (T = 1): name, map, q, p, min_mass, K and the expected
# (cells, masses, centroids in cells) of the seeds, in order.
def _m(shape, entries):
    m = np.zeros(shape, np.float32)
    for (i, j), v in entries.items():
        m[i, j] = v
    return m


PEAK_CASES = [
    # two adjacent equal cells: the lower flat index wins, the other is suppressed
    dict(name="adjacent_equal", map=_m((5, 5), {(2, 2): 4, (2, 3): 4}), q=0, p=1, min_mass=1.0,
         K=4, cells=[12], mass=[4.0], centroid=[(2.5, 2.5)]),
    # an all-equal map: every cell but (0, 0) has an equal neighbour of lower index
    dict(name="all_equal", map=np.ones((4, 4), np.float32), q=0, p=1, min_mass=1.0, K=4,
         cells=[0], mass=[1.0], centroid=[(0.5, 0.5)]),
    # a peak in the corner: its 3x3 window is clipped to 2x2; the cells (0,1),
    # (1,0), (1,1) tie at 6 and lose on the index
    dict(name="border_clipped", map=_m((6, 6), {(0, 0): 3, (0, 1): 1, (1, 0): 2}), q=1, p=2,
         min_mass=1.0, K=4, cells=[0], mass=[6.0], centroid=[(5.0 / 6.0, 4.0 / 6.0)]),
    dict(name="border_last_cell", map=_m((6, 6), {(5, 5): 7}), q=0, p=3, min_mass=7.0, K=2,
         cells=[35], mass=[7.0], centroid=[(5.5, 5.5)]),
    # four peaks, K = 3: by descending mass, equal masses by ascending index
    dict(name="more_than_K", map=_m((9, 9), {(1, 1): 5, (1, 5): 9, (5, 1): 7, (5, 5): 9}), q=0,
         p=1, min_mass=1.0, K=3, cells=[14, 50, 46], mass=[9.0, 9.0, 7.0],
         centroid=[(1.5, 5.5), (5.5, 5.5), (5.5, 1.5)]),
    # a cluster of 9 just under min_mass = 10 next to one of exactly 10; of the
    # cells that see all of the second cluster, (2,8) has the lowest index
    dict(name="under_min_mass", q=1, p=2, min_mass=10.0, K=4,
         map=_m((5, 12), {(2, 2): 5, (2, 3): 2, (1, 2): 2, (2, 9): 6, (2, 8): 2, (3, 9): 2}),
         cells=[32], mass=[10.0], centroid=[(2.7, 9.3)]),
    dict(name="empty", map=np.zeros((4, 6), np.float32), q=1, p=2, min_mass=0.5, K=4, cells=[],
         mass=[], centroid=[]),
]


# ---- association, moments, derived fields ---------------------------------------
def associate(n_seeds, seed_locs, counts, locs, fluxes, radius, rng=None):
    """match_of_seed [T,N,K] int32 by the exact lexicographic optimum (seed
    fluxes 1, the magnitude test off), and margins_ok [T,N]: no float32
    rounding can flip the catalog's association (catalog_margins_ok)."""
    T, N, S = fluxes.shape
    K = seed_locs.shape[1]
    rng = rng or np.random.default_rng(0)
    match = np.full((T, N, K), -1, np.int32)
    okm = np.ones((T, N), bool)
    for t in range(T):
        ns = int(n_seeds[t])
        sl = torch.as_tensor(seed_locs[t, :ns], dtype=torch.float32)
        sf = torch.ones(ns)
        for n in range(N):
            m = int(min(max(int(counts[t, n]), 0), S))
            el = torch.as_tensor(locs[t, n, :m], dtype=torch.float32)
            ef = torch.as_tensor(fluxes[t, n, :m], dtype=torch.float32)
            dist, _, oob = MO.pair_tables(sl, sf, el, ef, radius, F32_MAX)
            match[t, n, :ns] = MO.solve(dist.double().numpy(), oob.numpy(), radius)
            okm[t, n] = MO.catalog_margins_ok(sl, sf, el, ef, radius, F32_MAX, [], rng)
    return match, okm


def moments(match, locs, fluxes, seed_locs, weights=None):
    """(moments [T,K,10], abs [T,K,10] = sum of w |term|, matched_flux [T,N,K]
    float32, NaN where unmatched), float64 throughout."""
    T, N, K = match.shape
    S = fluxes.shape[-1]
    ok = (match >= 0) & (match < S)
    slot = np.where(ok, match, 0)
    t, n = np.arange(T)[:, None, None], np.arange(N)[None, :, None]
    h = locs[t, n, slot, 0].astype(np.float64)
    w_ = locs[t, n, slot, 1].astype(np.float64)
    f32 = fluxes[t, n, slot]
    f = f32.astype(np.float64)
    wt = np.ones((T, N)) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    wt = np.broadcast_to(wt[:, :, None], (T, N, K))
    dh = h - seed_locs[:, None, :, 0].astype(np.float64)
    dw = w_ - seed_locs[:, None, :, 1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mag = 22.5 - 2.5 * np.log10(f)
    terms = [np.ones_like(dh), dh, dw, dh * dh, dw * dw, dh * dw, f, f * f, mag, mag * mag]
    mom = np.stack([np.where(ok, wt * x, 0.0).sum(1) for x in terms], -1)
    ab = np.stack([np.where(ok, wt * np.abs(x), 0.0).sum(1) for x in terms], -1)
    return mom, ab, np.where(ok, f32, np.float32(np.nan)).astype(np.float32)


def derive(mom, total):
    """The derived float64 fields from moments [T,K,10] and total weight [T]."""
    with np.errstate(invalid="ignore", divide="ignore"):
        w = mom[..., 0]
        mean = lambda i: mom[..., i] / w  # noqa: E731
        dh, dw, f, mag = mean(1), mean(2), mean(6), mean(8)
        var = lambda i, mu: np.maximum(mean(i) - mu * mu, 0.0)  # noqa: E731
        return dict(prob=w / total[:, None], dh=dh, dw=dw, sd_h=np.sqrt(var(3, dh)),
                    sd_w=np.sqrt(var(4, dw)), cov_hw=mean(5) - dh * dw, flux=f,
                    flux_sd=np.sqrt(var(7, f)), mag=mag, mag_sd=np.sqrt(var(9, mag)))


def flux_quantiles(matched_flux, quantiles, weights=None):
    """[T,K,Q] float32: the smallest matched flux whose cumulative weight, in
    flux order, is >= q x the seed's total; NaN where nothing matched."""
    T, N, K = matched_flux.shape
    out = np.full((T, K, len(quantiles)), np.nan, np.float32)
    for t in range(T):
        for k in range(K):
            f = matched_flux[t, :, k]
            ok = ~np.isnan(f)
            if not ok.any():
                continue
            w = np.ones(N) if weights is None else np.asarray(weights[t], np.float32).astype(
                np.float64)
            order = np.argsort(f[ok], kind="stable")
            fs, cum = f[ok][order], np.cumsum(w[ok][order])
            for iq, q in enumerate(quantiles):
                out[t, k, iq] = fs[min(int((cum < float(q) * cum[-1]).sum()), len(fs) - 1)]
    return out


def condense(counts, locs, fluxes, box, weights=None, match_radius=0.75,
             quantiles=(0.05, 0.5, 0.95), c=4, q=1, p=2, min_prob=0.05, K=None):
    """The whole pipeline with a shared box; a dict of numpy arrays named as
    CondensedCatalog's fields (float64 before the final float32 cast), plus
    match [T,N,K] and margins_ok [T,N]."""
    T, N, S = fluxes.shape
    K = min(64, 2 * S) if K is None else K
    lo = np.tile(np.asarray(box[:2], np.float64), (T, 1))
    Gh, Gw = int(np.ceil((box[2] - box[0]) * c)), int(np.ceil((box[3] - box[1]) * c))
    sm = source_map(counts, locs, fluxes, lo, c, Gh, Gw, weights)
    total = (np.full(T, float(N)) if weights is None
             else np.asarray(weights, np.float32).astype(np.float64).sum(1))
    min_mass = (min_prob * total).astype(np.float32)
    n_seeds, cell, mass, slocs = find_seeds(sm["count"], q, p, min_mass, K, lo, c)
    slocs32 = slocs.astype(np.float32)
    match, okm = associate(n_seeds, slocs32, counts, locs, fluxes, match_radius)
    mom, ab, mflux = moments(match, locs, fluxes, slocs32, weights)
    d = derive(mom, total)
    valid = np.arange(K)[None, :] < n_seeds[:, None]
    row = lambda x: np.where(valid, x, np.nan).astype(np.float32)  # noqa: E731
    prob = np.nan_to_num(np.where(valid, d["prob"], 0.0))
    seed = slocs32.astype(np.float64)
    return dict(
        n_seeds=n_seeds, seed_cell=cell, seed_locs=slocs32, seed_mass=mass.astype(np.float32),
        prob=prob.astype(np.float32),
        locs=np.stack([row(seed[..., 0] + d["dh"]), row(seed[..., 1] + d["dw"])], -1),
        locs_sd=np.stack([row(d["sd_h"]), row(d["sd_w"])], -1), locs_cov_hw=row(d["cov_hw"]),
        fluxes=row(d["flux"]), fluxes_sd=row(d["flux_sd"]), mags=row(d["mag"]),
        mags_sd=row(d["mag_sd"]),
        flux_quantiles=np.where(valid[..., None], flux_quantiles(mflux, quantiles, weights),
                                np.float32(np.nan)),
        expected_count=prob.sum(-1).astype(np.float32),
        unassociated=((sm["count"].sum((1, 2)) + sm["outside"] - mom[..., 0].sum(-1))
                      / total).astype(np.float32),
        moments=mom, match=match, margins_ok=okm, source_map=sm)


# ---- synthetic inputs -------------------------------------------------------------
def map_case(seed=3, T=3, N=257, S=5, box=(-2.0, -2.0, 10.0, 8.0), c=4, tile_boxes=None):
    """Catalogs for the map / peaks / moments tests: per tile three stars
    (jittered by 0.1 px, present with probability 0.9 / 0.6 / 0.3) plus uniform
    sources, some of them outside the box; counts cover 0..S and the values -1
    and S+2 (clamped); padding is NaN; a few counted slots hold a NaN or
    infinite coordinate, or a zero, negative or infinite flux.  Every location
    is at least 1e-3 cells from a cell edge.  float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    lo = (np.tile(np.asarray(box[:2]), (T, 1)) if tile_boxes is None
          else np.asarray(tile_boxes)[:, :2]).astype(np.float64)
    counts = np.zeros((T, N), np.int32)
    locs = np.full((T, N, S, 2), np.nan, np.float32)
    fluxes = np.full((T, N, S), np.nan, np.float32)
    for t in range(T):
        stars = np.array([[1.3, 2.2], [5.1, 4.4], [7.6, 0.9]]) + 0.37 * t
        sflux = np.array([40.0, 12.0, 3.0])
        for n in range(N):
            src = [(stars[i] + rng.normal(0, 0.1, 2), sflux[i] * (1 + 0.05 * rng.normal()))
                   for i in range(3) if rng.uniform() < (0.9, 0.6, 0.3)[i]]
            for _ in range(int(rng.integers(0, 3))):
                src.append((rng.uniform([box[0] - 1.5, box[1] - 1.5], [box[2] + 1.5, box[3] + 1.5]),
                            rng.uniform(0.5, 50.0)))
            m = min(len(src), S)
            order = rng.permutation(len(src))[:m]
            for j, o in enumerate(order):
                locs[t, n, j], fluxes[t, n, j] = src[o]
            counts[t, n] = m
    # every count 0..S occurs in tile 0; -1 and S+2 exercise the clamp
    for t in range(T):
        full = np.nonzero(counts[t] < S)[0][:2]
        for n in full:  # fill to S slots, then claim S + 2
            k = counts[t, n]
            locs[t, n, k:] = rng.uniform([box[0], box[1]], [box[2], box[3]], (S - k, 2))
            fluxes[t, n, k:] = rng.uniform(0.5, 50.0, S - k)
            counts[t, n] = S + 2
        counts[t, np.nonzero(counts[t] == 1)[0][:1]] = -1
    # bad sources inside the counted slots
    bad = [(np.nan, None), (np.inf, None), (None, 0.0), (None, -1.0), (None, np.inf),
           (None, np.nan)]
    for t in range(T):
        rows = np.nonzero((counts[t] >= 2) & (counts[t] <= S))[0]
        for b, n in zip(bad, rows[3::7]):
            if b[0] is not None:
                locs[t, n, 1, t % 2] = b[0]
            else:
                fluxes[t, n, 1] = b[1]
    for t in range(T):  # move every location at least 1e-3 cells off the cell edges
        flat = locs[t].reshape(-1, 2)
        fin = np.isfinite(flat).all(-1)
        sub = flat[fin]
        g = (sub.astype(np.float64) - lo[t]) * c
        near = (np.abs(g - np.round(g)) < 1e-3).any(-1)
        while near.any():
            sub[near] += rng.uniform(0.01, 0.05, (int(near.sum()), 2)).astype(np.float32)
            g = (sub.astype(np.float64) - lo[t]) * c
            near = (np.abs(g - np.round(g)) < 1e-3).any(-1)
        flat[fin] = sub
    return counts, locs, fluxes


def planted_posterior(seed=0, T=4, N=512, S=6, box=(-2.0, -2.0, 10.0, 10.0)):
    """The end-to-end case: per tile three true stars at least 3 px apart,
    present independently with probability 1.0, 0.8 and 0.3, jittered by
    N(0, 0.1) px and 5 % in flux, slots shuffled; with probability 0.1 one
    spurious source uniform in the box, at least 2 px from every star.
    Returns counts, locs, fluxes (padding NaN), the stars' locations [T,3,2]
    and fluxes [T,3], and the planted presence counts [T,3]."""
    rng = np.random.default_rng(seed)
    probs = (1.0, 0.8, 0.3)
    counts = np.zeros((T, N), np.int32)
    locs = np.full((T, N, S, 2), np.nan, np.float32)
    fluxes = np.full((T, N, S), np.nan, np.float32)
    star_locs = np.zeros((T, 3, 2))
    star_flux = np.zeros((T, 3))
    planted = np.zeros((T, 3), np.int64)
    for t in range(T):
        while True:
            xy = rng.uniform(0.5, 7.5, (3, 2))
            d = np.linalg.norm(xy[:, None] - xy[None], axis=-1) + 10 * np.eye(3)
            if d.min() >= 3.0:
                break
        star_locs[t], star_flux[t] = xy, rng.uniform(5.0, 50.0, 3)
        for n in range(N):
            src = []
            for i in range(3):
                if rng.uniform() < probs[i]:
                    planted[t, i] += 1
                    src.append((xy[i] + rng.normal(0, 0.1, 2),
                                star_flux[t, i] * (1 + 0.05 * rng.normal())))
            if rng.uniform() < 0.1:
                while True:
                    z = rng.uniform(box[:2], box[2:])
                    if np.linalg.norm(xy - z, axis=-1).min() >= 2.0:
                        break
                src.append((z, rng.uniform(1.0, 50.0)))
            for j, o in enumerate(rng.permutation(len(src))):
                locs[t, n, j], fluxes[t, n, j] = src[o]
            counts[t, n] = len(src)
    return counts, locs, fluxes, star_locs, star_flux, planted
