"""A numpy float64 oracle of smcdet_amd.convergence, written directly from the
definitions (include/smcdet_hip.h), the derived error bounds of
DESIGN.md §14.5, and the seeded cases the host and GPU tests share.

Everything here is plain numpy: no torch, no device."""
import functools
import math
import statistics

import numpy as np

LDS_DRAWS = 16384     # SMCDET_CHAINS_LDS_DRAWS
BLOCK_PAIRS = 8       # SMCDET_CHAINS_BLOCK_PAIRS
U32 = 2.0 ** -24      # unit roundoff of float32
U64 = 2.0 ** -53      # unit roundoff of float64


# ---- the definitions ----------------------------------------------------------------
def split_chains(x, split):
    """x [C,M] -> [m,n]: with split, chain c becomes rows 2c (draws [0,n)) and
    2c+1 (draws [M-n,M)), n = M // 2."""
    x = np.asarray(x)
    C, M = x.shape
    if not split:
        return x
    n = M // 2
    return np.stack([x[:, :n], x[:, M - n:]], axis=1).reshape(2 * C, n)


def autocov(d, t):
    """[m]: the biased autocovariance a_j(t) of the centered chains d [m,n]."""
    n = d.shape[1]
    if t >= n:
        return np.zeros(d.shape[0])
    return np.einsum("ji,ji->j", d[:, :n - t], d[:, t:]) / n


def autocov_fft(d):
    """[m,n]: the same by numpy.fft (an independent route, all lags)."""
    m, n = d.shape
    L = 1
    while L < 2 * n:
        L *= 2
    f = np.fft.rfft(d, L, axis=1)
    return np.fft.irfft(f * np.conj(f), L, axis=1)[:, :n] / n


def row_stats(x, split=True, max_lag=None, num_rho=0):
    """The statistics of one row x [C,M] (float32 values, float64 arithmetic).
    Besides the outputs of smcdet_chain_stats: P (every pair looked at: the K
    kept and, when stopped, the refused one), eps_rho (the bound on the kernel's
    error in any rho_t, §14.5) and margin (the distance from 0 of the pairs that
    decide the cut-off: the last kept and the refused one)."""
    c = split_chains(np.asarray(x), split)
    m, n = c.shape
    assert n >= 4
    nan = float("nan")
    out = dict(m=m, n=n, n_pairs=0, stopped=0, P=[], margin=math.inf, eps_rho=nan,
               rho=np.full(num_rho, nan, np.float64), xmax=float(np.abs(c).max()))
    if not np.isfinite(c).all():
        out.update(mean=nan, W=nan, var_plus=nan, rhat=nan, tau=nan, ess=nan, mcse=nan,
                   chain_mean=np.full(m, nan), chain_var=np.full(m, nan))
        return out
    c = c.astype(np.float64)
    mu = c.mean(axis=1)
    d = c - mu[:, None]
    a0 = autocov(d, 0)
    W = a0.mean() * n / (n - 1)
    mean = mu.mean()
    bn = ((mu - mean) ** 2).sum() / (m - 1) if m > 1 else 0.0
    vp = W * (n - 1) / n + bn
    out.update(mean=mean, W=W, var_plus=vp, chain_mean=mu, chain_var=a0 * n / (n - 1))
    if not W > 0.0:
        out.update(rhat=nan, tau=nan, ess=nan, mcse=nan)
        return out
    out["eps_rho"] = eps_rho(c, a0)
    out["eps_f64"] = eps_f64(c, a0)

    @functools.lru_cache(maxsize=None)
    def rho(t):
        return 1.0 if t == 0 else 1.0 - (W - autocov(d, t).mean()) / vp

    lmax = min(n - 1, n - 1 if max_lag is None else max_lag)
    K, s, pmin, P = 0, 0.0, math.inf, []
    k = 0
    while 2 * k + 1 <= lmax:
        p = rho(2 * k) + rho(2 * k + 1)
        P.append(p)
        if p <= 0.0:
            out["stopped"] = 1
            break
        pmin = min(pmin, p)
        s += pmin
        K += 1
        k += 1
    tau = max(-1.0 + 2.0 * s, 1.0 / math.log10(m * n))
    ess = m * n / tau
    for t in range(min(num_rho, n)):
        out["rho"][t] = rho(t)
    decisive = P[-2:] if out["stopped"] else P[-1:]
    out.update(rhat=math.sqrt(vp / W), tau=tau, ess=ess, mcse=math.sqrt(vp / ess), n_pairs=K, P=P,
               margin=min(abs(p) for p in decisive), floor=tau == 1.0 / math.log10(m * n))
    return out


def chain_stats(x, split=True, max_lag=None, num_rho=0):
    """row_stats over the rows of x [R,C,M], stacked into arrays."""
    rows = [row_stats(r, split, max_lag, num_rho) for r in np.asarray(x)]
    out = {}
    for k in ("mean", "W", "var_plus", "rhat", "tau", "ess", "mcse", "eps_rho", "eps_f64",
              "margin", "xmax"):
        out[k] = np.array([r.get(k, float("nan")) for r in rows], np.float64)
    for k in ("n_pairs", "stopped"):
        out[k] = np.array([r[k] for r in rows], np.int32)
    for k in ("chain_mean", "chain_var", "rho"):
        out[k] = np.stack([r[k] for r in rows])
    out["m"], out["n"] = rows[0]["m"], rows[0]["n"]
    return out


# ---- the error bounds ---------------------------------------------
def _mean_shift(c, a0):
    """r: the bound on |kernel mu_j - oracle mu_j| relative to the row's
    sqrt(mean_j a_j(0)).  Both are float64 sums of exact float32 values in
    different orders: each is within gamma * max|x| of the true mean, with
    gamma = (n / 64 + 8) u64 for the kernel (lane-strided partial sums, a
    six-step butterfly, one division) and at most that for numpy's pairwise
    sum."""
    n = c.shape[1]
    gamma = 2.0 * (n / 64.0 + 8.0) * U64
    return gamma * np.abs(c).max() / math.sqrt(a0.mean())


def eps_rho(c, a0):
    """|rho_t (kernel) - rho_t (oracle)| <= eps_rho for every t >= 1: one
    float32 rounding per centered draw (2 u32 + u32^2 of a_j(0), by
    Cauchy-Schwarz), float64 accumulation in another order (n u64 per sum, both
    sides, and the few operations that form rho), and the shift of the means
    (2 r + r^2)."""
    m, n = c.shape
    r = _mean_shift(c, a0)
    return 2.0 * U32 + U32 * U32 + (4.0 * n + 2.0 * m + 64.0) * U64 + 2.0 * r + r * r


def eps_f64(c, a0):
    """Relative bound for the float64-only outputs W, var_plus and rhat (and
    the absolute bound on mean and chain_mean relative to max|x|): summation
    order and the shift of the means, no float32 rounding."""
    m, n = c.shape
    r = _mean_shift(c, a0)
    return (4.0 * n / 64.0 + 4.0 * m + 64.0) * U64 + 4.0 * r + 2.0 * r * r


def tau_bound(o):
    """|tau (kernel) - tau (oracle)| per row: P_k = rho_2k + rho_2k+1 is off by
    at most 2 eps_rho, the running minimum and the floor are 1-Lipschitz, and K
    of them are doubled: 4 K eps_rho (+ rounding of the sum itself)."""
    return 4.0 * np.maximum(o["n_pairs"], 1) * o["eps_rho"] + 64.0 * U64 * np.abs(o["tau"])


# ---- rank normalization, folding, tail indicators -----------------------------------
def average_ranks(x):
    """x [C,M] -> float64 [C,M]: 1-based ranks among the pooled draws, ties
    sharing their mean rank."""
    flat = np.asarray(x).reshape(-1)
    srt = np.sort(flat)
    lo = np.searchsorted(srt, flat, side="left")
    hi = np.searchsorted(srt, flat, side="right")
    return ((lo + hi + 1) * 0.5).reshape(np.shape(x))


_NORMAL = statistics.NormalDist()


def rank_normalize(x):
    """float64 normal scores (the caller rounds to float32)."""
    r = average_ranks(x)
    S = r.size
    u, inv = np.unique(r, return_inverse=True)
    z = np.array([_NORMAL.inv_cdf((v - 0.375) / (S + 0.25)) for v in u])
    return z[inv].reshape(r.shape)


def linear_quantile(flat, q):
    """float32: numpy / torch "linear" quantile of the float32 values formed
    in float64 from the two order statistics and rounded once (the definition
    of smcdet_row_summary)."""
    v = np.sort(np.asarray(flat, np.float32).reshape(-1)).astype(np.float64)
    pos = q * (v.size - 1)
    lo = int(math.floor(pos))
    g = pos - lo
    hi = min(lo + 1, v.size - 1)
    return np.float32(v[lo] if g == 0.0 else v[lo] + (v[hi] - v[lo]) * g)


def diagnose_inputs(x, tail_prob=0.05):
    """Row x [C,M] float32 -> dict of the five quantities `diagnose` feeds the
    kernel, with the ranks and thresholds they were made from."""
    x = np.asarray(x, np.float32)
    q_lo, med, q_hi = (linear_quantile(x, q) for q in (tail_prob, 0.5, 1.0 - tail_prob))
    folded = np.abs(x - med)  # float32 arithmetic, as on the device
    return dict(raw=x, ranks=average_ranks(x), z=rank_normalize(x),
                folded=folded, ranks_folded=average_ranks(folded), z_folded=rank_normalize(folded),
                lo=(x <= q_lo).astype(np.float32), hi=(x >= q_hi).astype(np.float32),
                q_lo=q_lo, med=med, q_hi=q_hi)


def compose(stats):
    """The Convergence fields from the stats (chain_stats dicts) of the five
    quantities, in `diagnose`'s order: raw, z, z_folded, lo, hi."""
    raw, z, zf, lo, hi = stats
    return dict(rhat=np.maximum(z["rhat"], zf["rhat"]),  # (numpy's maximum / minimum keep NaN)
                ess_bulk=z["ess"], ess_tail=np.minimum(lo["ess"], hi["ess"]),
                ess_mean=raw["ess"], mcse_mean=raw["mcse"], tau=raw["tau"], mean=raw["mean"],
                stopped=raw["stopped"])


# ---- seeded cases -------------------------------------------------------------------
PHIS = (0.0, 0.5, 0.9, 0.99, -0.5)
BURNIN = 200


def ar1(rng, phi, shape, loc=0.0, scale=1.0):
    """AR(1) chains x_t = phi x_{t-1} + e_t along the last axis after a burn-in
    of 200 steps, float32."""
    M = shape[-1]
    e = rng.standard_normal(shape[:-1] + (M + BURNIN,))
    x = np.zeros_like(e)
    prev = np.zeros(shape[:-1])
    for t in range(M + BURNIN):
        prev = phi * prev + e[..., t]
        x[..., t] = prev
    return (loc + scale * x[..., BURNIN:]).astype(np.float32)


def sticky(rng, shape, stay=0.8):
    """An integer-valued chain on 0..4 that keeps its value with probability
    `stay` (many ties), float32."""
    M = shape[-1]
    jump = rng.uniform(size=shape) >= stay
    fresh = rng.integers(0, 5, size=shape)
    x = np.empty(shape, np.float32)
    prev = fresh[..., 0]
    for t in range(M):
        prev = np.where(jump[..., t], fresh[..., t], prev)
        x[..., t] = prev
    return x


def phi_rows(seed, C, M, loc=0.0):
    """[5,C,M]: one row per phi of PHIS."""
    rng = np.random.default_rng(seed)
    return np.stack([ar1(rng, phi, (C, M), loc=loc) for phi in PHIS])


def special_rows(seed=7, C=3, M=40):
    """[8,C,M] and the names of the rows."""
    rng = np.random.default_rng(seed)
    base = ar1(rng, 0.5, (8, C, M))
    names = ("nan", "inf", "constant", "one_constant_chain", "sticky", "signed_zero",
             "different_means", "constant_chains_apart")
    base[0, 1, 5] = np.nan
    base[1, 2, M - 1] = np.inf
    base[2] = 2.5
    base[3, 0] = -1.25
    base[4] = sticky(rng, (C, M))
    z = rng.integers(0, 3, size=(C, M))
    base[5] = np.where(z == 0, np.float32(-0.0), np.where(z == 1, np.float32(0.0),
                                                          np.float32(1.0)))
    base[6] += (100.0 * np.arange(C, dtype=np.float32))[:, None]
    base[7] = np.arange(C, dtype=np.float32)[:, None]  # W == 0 with B > 0
    return base, names


def _case(x, split=True, max_lag=None, num_rho=0):
    return dict(x=np.ascontiguousarray(x, dtype=np.float32), split=split, max_lag=max_lag,
                num_rho=num_rho)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(x [R,C,M] float32, split, max_lag, num_rho): every shape
    and cut-off the GPU tests run.  Half-lengths n in {4, 5, 63, 64, 65, 127,
    128, 129, 1000, 5000}, odd M, C in {1, 2, 3, 32}, both paths, every phi."""
    out = {}
    # (n, C, odd M): the five phis as rows
    for i, (n, C, odd) in enumerate([(4, 32, 1), (5, 3, 0), (63, 1, 1), (64, 2, 0), (65, 3, 1),
                                     (127, 1, 0), (128, 32, 1), (129, 2, 0), (1000, 3, 1),
                                     (5000, 1, 0)]):
        out[f"split_n{n}_C{C}"] = _case(phi_rows(100 + i, C, 2 * n + odd),
                                        num_rho=(0, 1, 64, 1024)[i % 4])
    out["unsplit_C2_M129"] = _case(phi_rows(120, 2, 129), split=False, num_rho=64)
    out["unsplit_C1_M10000"] = _case(phi_rows(121, 1, 10000), split=False)  # K in the hundreds
    out["mcmc_C4_M10000"] = _case(phi_rows(122, 4, 10000), num_rho=64)      # workspace path
    out["split_n5000_C32"] = _case(phi_rows(123, 32, 10001)[2:4])           # workspace, m = 64
    out["lds_limit"] = _case(phi_rows(124, 4, 4096), num_rho=1)             # m n = 16384: LDS
    out["lds_limit_plus_chain"] = _case(phi_rows(125, 4, 4098), num_rho=1)  # m n = 16392
    out["one_row_4x16384"] = _case(phi_rows(126, 4, 16384)[1:2], split=False, num_rho=1024)
    out["max_lag_5"] = _case(phi_rows(127, 2, 600), max_lag=5, num_rho=64)  # below the cut-off
    out["max_lag_3_n4"] = _case(phi_rows(128, 3, 8, loc=3.0), max_lag=3, num_rho=1024)
    # cut-offs K one pair below, at and one pair above the lag block (seeds found by
    # find_block_seeds(); test_convergence_host asserts the K they give)
    for K, seed in BLOCK_SEEDS:
        out[f"block_K{K}"] = _case(ar1(np.random.default_rng(seed), BLOCK_PHI, (1, 2, 1200)))
    x, _ = special_rows()
    out["special"] = _case(x, num_rho=64)
    out["special_unsplit"] = _case(x, split=False)
    return out


# (K, seed): AR(1), phi = BLOCK_PHI, C = 2, M = 1200, split, whose cut-off is K pairs
# (phi = 0.8 has its cut-off around the block size at this length; 0.9 lies above it)
BLOCK_PHI = 0.8
BLOCK_SEEDS = ((7, 1006), (8, 1012), (9, 1010))


def find_block_seeds(limit=400):
    """The first seeds whose cut-off is 7, 8 and 9 pairs with a margin above
    400 x the bound on rho (how BLOCK_SEEDS was made)."""
    found = {}
    for seed in range(1000, 1000 + limit):
        x = ar1(np.random.default_rng(seed), BLOCK_PHI, (1, 2, 1200))
        r = row_stats(x[0])
        K = r["n_pairs"]
        if K in (7, 8, 9) and K not in found and r["stopped"] and \
                r["margin"] > 400.0 * r["eps_rho"]:
            found[K] = seed
        if len(found) == 3:
            break
    return tuple(sorted(found.items()))


@functools.lru_cache(maxsize=None)
def expected(name):
    c = cases()[name]
    return chain_stats(c["x"], c["split"], c["max_lag"], c["num_rho"])


@functools.lru_cache(maxsize=None)
def diagnose_cases():
    """name -> x [R,C,M] float32 for `diagnose`: the tie-heavy integer chain
    and an AR(1) case."""
    rng = np.random.default_rng(300)
    return dict(sticky=sticky(rng, (3, 4, 500)),
                ar1=np.stack([ar1(rng, phi, (4, 500)) for phi in (0.0, 0.9)]))


def big_diagnose_row():
    """[4,5000] float32, phi = 0.5: a pooled row above calibration.row_summary's
    16384 entries, for `diagnose`'s torch.quantile route."""
    return phi_rows(140, 4, 5000)[1]
