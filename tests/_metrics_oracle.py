"""CPU oracle for smcdet_amd.metrics.match_catalogs: the exact lexicographic
matching (most in-tolerance pairs, then the smallest sum of their distances)
by float64 scipy `linear_sum_assignment` on where(oob, PENALTY, dist).

With at most 64 assigned pairs of distance <= locs_tol, any change in the
number of out-of-tolerance pairs moves the cost by at least
PENALTY - 64 * locs_tol > 0, so the optimum is lexicographic as long as
64 * locs_tol < PENALTY (asserted), and float64 keeps ~1e-10 of absolute
resolution on the distances next to a handful of 1e6 terms.

Distances, magnitudes and the tolerance tests are formed in float32 with the
reference's own torch expressions (metrics.py:36-57), so thresholds fall where
the reference's do.
"""
import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

PENALTY = 1e6


def mags_of(fluxes):
    return 22.5 - 2.5 * torch.log10(fluxes)


def pair_tables(true_locs, true_fluxes, est_locs, est_fluxes, locs_tol, mags_tol):
    """float32 distance [n,m], |delta mag| [n,m] and the out-of-tolerance mask of
    one (true, est) catalog pair (torch tensors holding only the counted slots)."""
    diff = true_locs[:, None, :] - est_locs[None, :, :]
    dist = diff.norm(dim=-1)
    dmag = (mags_of(true_fluxes)[:, None] - mags_of(est_fluxes)[None, :]).abs()
    bad_t = ~(torch.isfinite(true_locs).all(-1) & torch.isfinite(true_fluxes) & (true_fluxes > 0))
    bad_e = ~(torch.isfinite(est_locs).all(-1) & torch.isfinite(est_fluxes) & (est_fluxes > 0))
    oob = (dist > locs_tol) | (dmag > mags_tol) | bad_t[:, None] | bad_e[None, :]
    return dist, dmag, oob


def solve(dist, oob, locs_tol):
    """match_of_true [n] (est slot or -1) of the lexicographic optimum.  dist
    [n,m] float64 numpy, oob [n,m] bool numpy."""
    assert 64 * float(locs_tol) < PENALTY
    n, m = dist.shape
    out = np.full(n, -1, np.int32)
    if n == 0 or m == 0:
        return out
    cost = np.where(oob, PENALTY, dist)
    r, c = linear_sum_assignment(cost)
    ok = ~oob[r, c]
    out[r[ok]] = c[ok]
    return out


def bucketed(mags, matched, mag_bins):
    """[B] totals and [B] matched counts of one catalog (torch.bucketize rule)."""
    B = len(mag_bins)
    b = torch.bucketize(mags, mag_bins)
    onehot = (b[:, None] == torch.arange(B)[None, :]).float()
    return onehot.sum(0), onehot[torch.as_tensor(matched, dtype=torch.bool)].sum(0)


def match_catalogs(true_counts, true_locs, true_fluxes, est_counts, est_locs, est_fluxes,
                   index, locs_tol, mags_tol, mag_bins):
    """The four [T,M,B] float32 arrays and match_of_true [T,M,St] int32 (numpy).
    Inputs: numpy arrays or CPU tensors; index [T,M]."""
    tc = torch.as_tensor(np.asarray(true_counts)).to(torch.int64)
    tl = torch.as_tensor(np.asarray(true_locs), dtype=torch.float32)
    tf = torch.as_tensor(np.asarray(true_fluxes), dtype=torch.float32)
    ec = torch.as_tensor(np.asarray(est_counts)).to(torch.int64)
    el = torch.as_tensor(np.asarray(est_locs), dtype=torch.float32)
    ef = torch.as_tensor(np.asarray(est_fluxes), dtype=torch.float32)
    index = np.asarray(index)
    bins = torch.as_tensor(np.asarray(mag_bins), dtype=torch.float32)
    T, M = index.shape
    St, Se, B = tl.shape[1], el.shape[2], len(bins)
    outs = np.zeros((4, T, M, B), np.float32)
    mot = np.full((T, M, St), -1, np.int32)
    for t in range(T):
        n = int(min(max(int(tc[t]), 0), St))
        for j in range(M):
            e = int(index[t, j])
            m = int(min(max(int(ec[t, e]), 0), Se))
            dist, _, oob = pair_tables(tl[t, :n], tf[t, :n], el[t, e, :m], ef[t, e, :m],
                                       locs_tol, mags_tol)
            q = solve(dist.double().numpy(), oob.numpy(), locs_tol)
            mot[t, j, :n] = q
            est_matched = np.zeros(m, bool)
            est_matched[q[q >= 0]] = True
            tt, tm = bucketed(mags_of(tf[t, :n]), q >= 0, bins)
            et, em = bucketed(mags_of(ef[t, e, :m]), est_matched, bins)
            outs[0, t, j], outs[1, t, j] = tt.numpy(), tm.numpy()
            outs[2, t, j], outs[3, t, j] = et.numpy(), em.numpy()
    return outs[0], outs[1], outs[2], outs[3], mot


# ---- synthetic cases with decision margins (fixture generator and GPU tests) ----
MARGIN = 1e-4
MAG_LO, MAG_HI = 16.5, 21.2      # true and spurious magnitudes
EST_MAG_LO, EST_MAG_HI = 16.05, 21.95  # jittered magnitudes are clipped into this range


def flux_of(mag):
    return 10 ** ((22.5 - mag) / 2.5)


def catalog_margins_ok(tl, tf, el, ef, locs_tol, mags_tol, bin_sets, rng):
    """True when float32 rounding cannot flip a decision of this catalog pair:
    every distance and |delta mag| is > MARGIN from its tolerance, every est
    magnitude is > MARGIN from every bin edge, and the optimum is unchanged
    under four random +-MARGIN relative perturbations of the distances."""
    dist, dmag, oob = pair_tables(tl, tf, el, ef, locs_tol, mags_tol)
    if dist.numel() and (((dist - locs_tol).abs() <= MARGIN).any()
                         or ((dmag - mags_tol).abs() <= MARGIN).any()):
        return False
    mags = mags_of(ef)
    for bins in bin_sets:
        if mags.numel() and ((mags[:, None] - torch.as_tensor(bins, dtype=torch.float32)[None, :])
                             .abs() <= MARGIN).any():
            return False
    d64, o = dist.double().numpy(), oob.numpy()
    base = solve(d64, o, locs_tol)
    for _ in range(4):
        s = rng.choice([-1.0, 1.0], size=d64.shape)
        if not np.array_equal(solve(d64 * (1 + MARGIN * s), o, locs_tol), base):
            return False
    return True


def synth_case(seed, T, N, St, Se, frame, locs_tol, mags_tol, bin_sets, counts="cycle",
               fill=False, p_empty=0.05):
    """Catalogs built from a known truth (numpy arrays): each true source kept
    with probability 0.8 and jittered by N(0, 0.25) px and N(0, 0.3) mag, with
    probability 0.3 a second jittered copy (two est sources compete for one
    true source), 0-2 uniform spurious sources, some catalogs empty; est
    padding is NaN, true padding a decoy exactly on a true source.  counts:
    "cycle" (0..St over the tiles) or "full"; fill: top catalogs up to Se with
    spurious sources.  Every catalog is redrawn until catalog_margins_ok."""
    rng = np.random.default_rng(seed)
    edges = np.concatenate([np.asarray(b, np.float64) for b in bin_sets])
    tc = np.array([(t % (St + 1)) if counts == "cycle" else St for t in range(T)], np.int32)
    tl = np.zeros((T, St, 2), np.float32)
    tf = np.zeros((T, St), np.float32)
    ec = np.zeros((T, N), np.int32)
    el = np.full((T, N, Se, 2), np.nan, np.float32)
    ef = np.full((T, N, Se), np.nan, np.float32)
    for t in range(T):
        n = int(tc[t])
        while True:
            mags = rng.uniform(MAG_LO, MAG_HI, St)
            if (np.abs(mags_of(torch.tensor(flux_of(mags), dtype=torch.float32)).numpy()[:, None]
                       - edges[None, :]) > MARGIN).all():
                break
        tl[t] = rng.uniform(0, frame, (St, 2))
        tf[t] = flux_of(mags)
        if n > 0:  # decoys in the padding: exactly on true source 0
            tl[t, n:], tf[t, n:] = tl[t, 0], tf[t, 0]
        for c in range(N):
            while True:
                locs, mg = [], []
                if rng.uniform() >= p_empty or fill:
                    for i in range(n):
                        copies = (rng.uniform() < 0.8) + (rng.uniform() < 0.3)
                        for _ in range(copies):
                            locs.append(tl[t, i] + rng.normal(0, 0.25, 2))
                            mg.append(mags[i] + rng.normal(0, 0.3))
                    extra = (Se - len(locs)) if fill else int(rng.integers(0, 3))
                    for _ in range(max(extra, 0)):
                        locs.append(rng.uniform(0, frame, 2))
                        mg.append(rng.uniform(MAG_LO, MAG_HI))
                m = min(len(locs), Se)
                order = rng.permutation(len(locs))[:m]
                cl = np.asarray(locs, np.float32).reshape(-1, 2)[order]
                cf = flux_of(np.clip(np.asarray(mg, np.float64)[order], EST_MAG_LO,
                                     EST_MAG_HI)).astype(np.float32)
                if catalog_margins_ok(torch.tensor(tl[t, :n]), torch.tensor(tf[t, :n]),
                                      torch.tensor(cl), torch.tensor(cf), locs_tol, mags_tol,
                                      bin_sets, rng):
                    break
            ec[t, c] = m
            el[t, c, :m], ef[t, c, :m] = cl, cf
    return dict(true_counts=tc, true_locs=tl, true_fluxes=tf, est_counts=ec, est_locs=el,
                est_fluxes=ef)
