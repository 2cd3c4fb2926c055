"""numpy float64 restatement of smcdet_amd.calibration, written
from the definitions in include/smcdet_hip.h, plus the seeded cases the host
and GPU tests share.  Everything is plain loops over rows: the cases are small.
"""
import numpy as np

DEFAULT_LEVELS = tuple(round(0.05 * c, 2) for c in range(1, 20))
BOOT_TAG = 0x42530000
_M32 = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10 and the bootstrap indices -------------------------------------
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Arrays of uint32 counters (broadcast together) and scalar keys -> four
    uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    A, B = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = A * c0, B * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32)
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def boot_indices(seed, Bn, M):
    """[Bn,M] int64: idx[r,j] = mulhi32(x[j % 4], M), x = Philox(counter (r,
    j // 4, 0, tag), key (seed low, seed high))."""
    seed = int(seed) & ((1 << 64) - 1)
    quads = (M + 3) // 4
    x = philox4x32(np.arange(Bn)[:, None], np.arange(quads)[None, :], 0, BOOT_TAG,
                   seed & 0xFFFFFFFF, seed >> 32)
    x = np.stack(x, -1).reshape(Bn, 4 * quads)[:, :M]
    return ((x * np.uint64(M)) >> np.uint64(32)).astype(np.int64)


# ---- the three kernels ------------------------------------------------------------
def catalog_totals(counts, fluxes, cuts):
    """n_above [C,T,N] int64 and flux_above [C,T,N] float64 (not yet rounded)."""
    T, N, S = fluxes.shape
    cnt = np.clip(np.asarray(counts, np.int64), 0, S)
    inside = np.arange(S)[None, None, :] < cnt[..., None]
    f = np.asarray(fluxes, np.float32)
    n, fl = [], []
    for c in cuts:
        with np.errstate(invalid="ignore"):
            hit = inside & (f >= np.float32(c))
        n.append(hit.sum(-1))
        fl.append(np.where(hit, f.astype(np.float64), 0.0).sum(-1))
    return np.stack(n), np.stack(fl)


def quantile_linear(v, q):
    """v: ascending float32 valid entries (n >= 1).  float64 result before the
    one rounding to float32, with the two order statistics used."""
    pos = float(q) * float(len(v) - 1)
    lo = int(np.floor(pos))
    g = pos - lo
    hi = min(lo + 1, len(v) - 1)
    vlo, vhi = float(v[lo]), float(v[hi])
    if g == 0.0:
        return vlo, vlo, vhi
    with np.errstate(invalid="ignore"):
        return vlo + (vhi - vlo) * g, vlo, vhi


def quantile_lower(v, w, q):
    """v ascending valid entries, w their float64 weights in that order."""
    cum = np.cumsum(w)
    total = cum[-1]
    first = int((cum < float(q) * total).sum())
    return float(v[min(first, len(v) - 1)])


def row_summary(values, weights=None, q=(), interpolation="linear", thresholds=None):
    """values [R,N] float32, weights [R,N] or None, thresholds [R,E] or None ->
    a dict of float64 arrays (quantiles not yet rounded to float32; `v_lo` /
    `v_hi` [R,Q] are the order statistics a linear quantile was formed from)."""
    values = np.asarray(values, np.float32)
    R, N = values.shape
    Q = len(q)
    E = 0 if thresholds is None else thresholds.shape[1]
    out = dict(n_valid=np.zeros(R, np.int64), weight=np.zeros(R), mean=np.full(R, np.nan),
               var=np.full(R, np.nan), vmin=np.full(R, np.nan), vmax=np.full(R, np.nan),
               quantiles=np.full((R, Q), np.nan), v_lo=np.full((R, Q), np.nan),
               v_hi=np.full((R, Q), np.nan), below=np.zeros((R, E)), at_or_below=np.zeros((R, E)),
               abs_sum=np.zeros(R), abs_dev_sum=np.zeros(R))
    for r in range(R):
        ok = ~np.isnan(values[r])
        idx = np.flatnonzero(ok)
        v = values[r, idx]
        w = np.ones(len(v)) if weights is None else np.asarray(weights[r], np.float64)[idx]
        order = np.lexsort((idx, v))  # by value, then by index
        v, w = v[order], w[order]
        out["n_valid"][r] = len(v)
        W = w.sum()
        out["weight"][r] = W
        v64 = v.astype(np.float64)
        if len(v):
            out["vmin"][r], out["vmax"][r] = v64[0], v64[-1]
        for k in range(E):
            e = np.float32(thresholds[r, k])
            with np.errstate(invalid="ignore"):
                out["below"][r, k] = w[v < e].sum()
                out["at_or_below"][r, k] = w[v <= e].sum()
        if not W > 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            mean = (w * v64).sum() / W
            out["mean"][r] = mean
            out["var"][r] = max(((w * (v64 - mean) ** 2).sum()) / W, 0.0) \
                if not np.isnan(mean) else np.nan
            out["abs_sum"][r] = np.abs(w * v64).sum()
            out["abs_dev_sum"][r] = np.abs(w * (v64 - mean) ** 2).sum()
        for k, qq in enumerate(q):
            if interpolation == "linear":
                out["quantiles"][r, k], out["v_lo"][r, k], out["v_hi"][r, k] = \
                    quantile_linear(v, qq)
            else:
                out["quantiles"][r, k] = quantile_lower(v, w, qq)
    return out


def bootstrap_means(values, indices):
    """[Bn,D] float64: (sum_j values[idx[r,j]]) / M."""
    v = np.asarray(values, np.float64)
    return v[indices].sum(1) / float(v.shape[0])


# ---- the Python layer ---------------------------------------------------------------
def interval_q(levels):
    return tuple(max(0.5 - x / 2, 0.0) for x in levels) + tuple(min(0.5 + x / 2, 1.0)
                                                                 for x in levels)


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def coverage(values, truth, levels=DEFAULT_LEVELS, mask=None, weights=None):
    """Cells 39 and 44 of the results notebook: intervals, covered, rate, PIT,
    rank.  `margin` [R,2L]: the distance of the truth from each interval end."""
    L = len(levels)
    truth = np.asarray(truth, np.float32)
    s = row_summary(values, weights, interval_q(levels),
                    "linear" if weights is None else "lower", truth[:, None])
    qf = f32(s["quantiles"])
    lo, hi = qf[:, :L], qf[:, L:]
    covered = (lo <= truth[:, None]) & (truth[:, None] <= hi)
    kept = covered if mask is None else covered[np.asarray(mask, bool)]
    rank = row_summary(values, None, (), "linear", truth[:, None])["below"][:, 0]
    return dict(lo=lo, hi=hi, covered=covered, rate=kept.astype(np.float64).mean(0),
                pit=1.0 - s["below"][:, 0] / s["weight"], sbc_rank=rank.astype(np.int64),
                margin=np.abs(s["quantiles"] - truth[:, None].astype(np.float64)),
                exact=s)


def count_posterior(n_above, max_count, weights=None):
    n_above = np.asarray(n_above)
    T, N = n_above.shape
    w = np.ones((T, N)) if weights is None else np.asarray(weights, np.float64)
    mass = np.stack([(w * (n_above == k)).sum(1) for k in range(max_count + 1)], -1)
    return dict(mass=mass, pmf=mass / w.sum(1)[:, None], mode=mass.argmax(-1))  # first maximum


def count_confusion(x, true_counts, max_true, max_count=None):
    """x [T,K+1] float (mass or pmf) or [T] int (modes, rows 0..max_count)."""
    x = np.asarray(x)
    tc = np.asarray(true_counts, np.int64)
    if x.ndim == 2:
        out = np.zeros((x.shape[1], max_true + 1))
        for t in range(len(tc)):
            if tc[t] <= max_true:
                out[:, tc[t]] += x[t]
        return out
    K = int(x.max()) if max_count is None else max_count
    out = np.zeros((K + 1, max_true + 1), np.int64)
    for t in range(len(tc)):
        if tc[t] <= max_true and x[t] <= K:
            out[x[t], tc[t]] += 1
    return out


def luminosity_function(est_total, q=(0.05, 0.5, 0.95)):
    tot = np.asarray(est_total, np.float64).sum(0)  # [N,Bins]
    return row_summary(f32(tot).T, None, q, "linear")["quantiles"]  # [Bins,Q]


def bootstrap_ci(values, indices, alpha=0.1, num_comparisons=1):
    """Cell 51 with given draws: (lower, mean, upper), float64, from the
    float32 replicate means."""
    boot = f32(bootstrap_means(values, indices))
    a = alpha / num_comparisons
    s = row_summary(boot.T, None, (a, 1.0 - a), "linear")
    return s["quantiles"][:, 0], s["mean"], s["quantiles"][:, 1], s


# ---- cases ------------------------------------------------------------------------
Q_LEVELS = (0.0,) + interval_q(DEFAULT_LEVELS) + (1.0,)  # 19 * 2 levels plus 0 and 1


def dyadic_weights(rng, shape, zero_share=0.1):
    """Multiples of 2^-10 in (0, 2], some exactly zero: every partial sum of up
    to 2^40 of them is exact in float64."""
    w = rng.integers(1, 2049, shape) / 1024.0
    w[rng.uniform(size=shape) < zero_share] = 0.0
    return w.astype(np.float32)


def summary_case(N, R, seed=0):
    """values [R,N] float32 with the special rows first (as far as R and N
    allow): all equal; small integers (massive ties); +-0 and +-inf among
    normals; NaNs scattered; all NaN.  The rest are lognormal draws."""
    rng = np.random.default_rng(1000 * seed + N)
    v = rng.lognormal(1.0, 1.0, (R, N)).astype(np.float32)
    v[0] = np.float32(3.25)
    if R > 1:
        v[1] = rng.integers(0, 5, N).astype(np.float32)
    if R > 2:
        v[2] = rng.normal(0, 1, N).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf, 0.0, -0.0], np.float32)
        k = min(N, len(special))
        v[2, rng.permutation(N)[:k]] = special[:k]
    if R > 3:
        v[3, rng.uniform(size=N) < 0.3] = np.nan
    if R > 4:
        v[4] = np.nan
    return v


def thresholds_case(values, E=5, seed=0):
    """[R,E]: entries of the row itself (ties with the data), 0, and values
    outside its range."""
    rng = np.random.default_rng(seed + 7)
    R, N = values.shape
    th = np.empty((R, E), np.float32)
    for r in range(R):
        pick = values[r, rng.integers(0, N, E)]
        th[r] = np.where(np.isnan(pick), np.float32(1.5), pick)
    th[:, 0] = 0.0
    th[:, 1] = -1e30
    th[:, 2] = np.inf
    return th


def totals_case(T=3, N=257, S=5, seed=0):
    """counts [T,N] (0 and S included), fluxes [T,N,S] with NaN / +inf at or
    past the counts, and fluxes exactly at the cuts."""
    rng = np.random.default_rng(seed + 31 * S)
    counts = rng.integers(0, S + 1, (T, N)).astype(np.int32)
    counts[0, 0], counts[0, 1] = 0, S
    fluxes = rng.lognormal(2.0, 1.0, (T, N, S)).astype(np.float32)
    past = np.arange(S)[None, None, :] >= counts[..., None]
    junk = rng.choice(np.array([np.nan, np.inf, 0.0, 7.0], np.float32), (T, N, S))
    fluxes = np.where(past, junk, fluxes)
    fluxes[0, 1, 0] = np.float32(5.0)  # equal to a cut, inside the counted slots
    fluxes[1, 1, 0] = np.float32(20.0)
    counts[1, 1] = max(counts[1, 1], 1)
    return counts, fluxes


TOTALS_CUTS = {1: (5.0,), 3: (0.0, 5.0, 20.0)}


def posterior_case(T=12, N=1000, S=5, seed=8):
    """A synthetic posterior around continuous truths: true_counts [T],
    true_fluxes [T,S]; est_counts [T,N], est_fluxes [T,N,S] (kept first, zeros
    after); est_total [T,N,4]: per-bin source counts for the luminosity
    function; metric rows [N,6] in [0,1] (multiples of 2^-10)."""
    rng = np.random.default_rng(seed)
    true_counts = rng.integers(0, S, T).astype(np.int32)
    true_counts[0] = 0
    true_fluxes = np.zeros((T, S), np.float32)
    for t in range(T):
        true_fluxes[t, :true_counts[t]] = rng.lognormal(3.0, 0.7, true_counts[t])
    est_counts = np.clip(true_counts[:, None] + rng.integers(-1, 2, (T, N)), 0, S).astype(np.int32)
    # a tile without a true source never gets an empty catalog: its total flux
    # then has no atom at the truth (0), which would make `covered` rest on a tie
    est_counts[true_counts == 0] = np.maximum(est_counts[true_counts == 0], 1)
    base = np.where(true_fluxes > 0, true_fluxes, np.float32(30.0))[:, None, :]
    base = base * rng.lognormal(0.0, 0.15, (T, 1, 1))  # a per-tile bias: some truths fall outside
    est_fluxes = (base * rng.lognormal(0.0, 0.25, (T, N, S))).astype(np.float32)
    est_fluxes[np.arange(S)[None, None, :] >= est_counts[..., None]] = 0.0
    edges = np.array([0.0, 10.0, 20.0, 40.0, np.inf])
    kept = est_fluxes > 0
    est_total = np.stack([(kept & (est_fluxes >= edges[b]) & (est_fluxes < edges[b + 1])).sum(-1)
                          for b in range(4)], -1).astype(np.float32)
    rows = (rng.integers(0, 1025, (N, 6)) / 1024.0).astype(np.float32)
    return dict(true_counts=true_counts, true_fluxes=true_fluxes, est_counts=est_counts,
                est_fluxes=est_fluxes, est_total=est_total, rows=rows)


def quantile_tolerance(want, v_lo, v_hi):
    """One rounding to float32 plus the float64 lerp's own error."""
    with np.errstate(invalid="ignore"):
        return 2.0 ** -23 * np.abs(want) + 2.0 ** -50 * np.maximum(np.abs(v_lo), np.abs(v_hi))


def calibrate(case, flux_cut, levels=DEFAULT_LEVELS, weights=None):
    """The whole of `calibration.calibrate` on a posterior_case."""
    n, fl = catalog_totals(case["est_counts"], case["est_fluxes"], (flux_cut,))
    tn, tf = catalog_totals(case["true_counts"][:, None], case["true_fluxes"][:, None],
                            (flux_cut,))
    tn, tf = tn[0, :, 0], f32(tf[0, :, 0])
    cov = coverage(f32(fl[0]), tf, levels, case["true_counts"] > 0, weights)
    max_count, max_true = int(n.max()), int(tn.max())
    post = count_posterior(n[0], max_count, weights)
    return dict(n_above=n, flux_above=fl, true_n=tn, true_flux=tf, coverage=cov, post=post,
                confusion_samples=count_confusion(post["mass"], tn, max_true),
                confusion_mode=count_confusion(post["mode"], tn, max_true, max_count),
                max_count=max_count, max_true=max_true)
