"""Inputs and acceptance criteria of the tile-pass tests (tile.h: temper ->
reweight -> resampling indices), shared by tests/test_gpu_tile_pass.py (the
kernels) and tests/test_tile_oracle_host.py (the criteria themselves, on the
CPU).  Everything is generated from seeded numpy generators; nothing here
touches a GPU.

Particle counts (N_CASES): for each of the six tile_kernel<512, PER>
instantiations the full size 512 * PER (the unmasked fast path) and masked
neighbours: one particle, less than a wave, one past a wave, one short of and
one past every PER boundary, register slots that no thread uses (1536), cumsum
chunks that are empty for the last threads (3592, 4088) and ragged counts.

Tiles: every count makes one launch of T = 6 tiles (TILES) whose neighbours in
memory look nothing like them; the three largest log-likelihoods of a tile
sit at its last index, its first index and the last index below a multiple of
512, and a guard row of +3e38 follows the last tile, so a dropped or
duplicated boundary element, or a read past the tile, moves ESS by far more
than any tolerance.

The tempering increment is judged by its ESS bracket, not by its distance
from scipy's root (increment_check): brentq returns a point within
tol = xtol + rtol * |x| of a sign change of the objective it was given, and
the float32 objective (the reference's, and the kernel's) differs from the
float64 one by a relative theta = 4 * 2^-23 * d * max|l| + c in ESS, so
ESS64(d + tol) <= thr * (1 + theta) and ESS64(d - tol) >= thr * (1 - theta).
The first term of theta bounds the rounding of each d * l_i and d * lmax to
float32 (exponent error <= 2^-23 * d * max|l|; ESS is a squared sum over a sum
of squares: factor 4).  c covers the float32 sums and the exponential: it is
measured (measured_c) as four times the largest relative difference between
the float32-mode and the float64-mode oracle ESS at the float64 root over the
offset-0 tiles of every count, and is no less than 4e-6.

Measured here: the largest such difference is 1.6e-06, so c = 6.3e-06.  With
it the float32-mode oracle's increments hold the bracket on every input
without drawing on theta at all (the worst tile keeps 0.36 * theta to spare
inside tol alone), and no tile of any count uses the near-threshold exemption
(exemption count 0).  tests/test_tile_oracle_host.py asserts these figures.
"""
import functools

import numpy as np
from scipy.optimize import brentq

from oracle import smc_oracle as O

F32 = np.float32

N_CASES = {
    1: (1, 2, 7, 64, 65, 511, 512),
    2: (513, 1000, 1024),
    4: (1025, 1536, 2047, 2048),
    8: (2049, 3592, 4088, 4095, 4096),
    16: (4097, 5000, 8191, 8192),
    32: (8193, 10000, 16383, 16384),
}
ALL_N = tuple(n for per in sorted(N_CASES) for n in N_CASES[per])
KTB = 512
GUARD = F32(3e38)

# (kind, scale, entry temperature, offset, log Z on entry)
TILES = (
    ("chi2", 3.0, 0.0, 0.0, 0.0),
    ("chi2", 40.0, 0.0, -1e4, -3.5),      # the realistic magnitude of a tile's log-likelihood
    ("chi2", 400.0, 0.3, 0.0, 12.25),
    ("chi2", 4000.0, 0.99, 0.0, -1000.0),
    ("const", 0.0, 0.3, -7.25, 0.5),      # ESS = N at every delta: delta = 1 - tau
    ("chi2", 40.0, 1.0, 0.0, 7.0),        # enters at temperature 1: delta = 0
)
T = len(TILES)


def per_of(N):
    """The PER of the tile_kernel instantiation that launch_tile picks."""
    per = -(-N // KTB)
    return next(p for p in (1, 2, 4, 8, 16, 32) if per <= p)


def place_adversarially(l):
    """Largest element to the last index, second largest to index 0, third
    largest to the last index below a multiple of 512 (N > 512): swaps, in
    place."""
    N = l.size
    taken = []

    def move(dst):
        free = np.ones(N, bool)
        free[taken] = False
        src = int(np.flatnonzero(free)[np.argmax(l[free])])
        l[src], l[dst] = l[dst], l[src]
        taken.append(dst)
    move(N - 1)
    if N > 1:
        move(0)
    if N > KTB:
        move(((N - 1) // KTB) * KTB - 1)
    return l


def chi2_loglik(rng, n, scale, offset):
    """-(chi2_5 * scale) + offset in float32.  Populations of fewer than four
    spread over less than one nat instead: at N = 2 ESS tends to 1 = 0.5 * N
    as the two log-likelihoods part, and a tile there would sit within
    rounding of the threshold (the exemption the criteria must not need)."""
    x = rng.chisquare(5, n)
    if n < 4:
        x = 4.0 + (x % 1.0) / scale
    return (-(x * scale) + offset).astype(F32)


@functools.lru_cache(maxsize=None)
def _tiles(N):
    rng = np.random.default_rng([N, 2026])
    ll = np.empty((T + 1, N), F32)
    for t, (kind, scale, _, offset, _) in enumerate(TILES):
        if kind == "const":
            ll[t] = F32(offset)
        else:
            ll[t] = place_adversarially(chi2_loglik(rng, N, scale, offset))
    ll[T] = GUARD
    ll.setflags(write=False)
    return ll


def tile_inputs(N):
    """loglik [T+1, N] (read-only; row T is the +3e38 guard), tau_in [T],
    logZ_in [T], ess_threshold."""
    tau = np.array([s[2] for s in TILES], F32)
    lz = np.array([s[4] for s in TILES], F32)
    return _tiles(N), tau, lz, 0.5 * N


def nonfinite_inputs(N):
    """tile_inputs with a few -inf in tile 0 and tile 2 (at the first index,
    the last, around a multiple of 512 and mid-tile) and one NaN in tile 1
    and tile 3.  Returns (loglik, tau_in, logZ_in, thr)."""
    ll, tau, lz, thr = tile_inputs(N)
    ll = ll.copy()
    for t in (0, 2):
        ll[t, [1, N // 3, KTB - 1, KTB, N - 2]] = -np.inf
    ll[1, N // 2] = np.nan
    ll[3, N - 1] = np.nan
    return ll, tau, lz, thr


# ---------------------------------------------------------------------------
# acceptance criteria
# ---------------------------------------------------------------------------
def ess64(l, d):
    """(sum e)^2 / sum e^2, e = exp(d * l - max), float64, over the finite
    log-likelihoods."""
    l = np.asarray(l, np.float64)
    x = float(d) * l[np.isfinite(l)]
    e = np.exp(x - x.max())
    return float(e.sum() ** 2 / (e * e).sum())


def theta_of(d, l, c):
    l = np.asarray(l, np.float64)
    return 4.0 * 2.0 ** -23 * abs(float(d)) * float(np.abs(l[np.isfinite(l)]).max()) + c


def increment_check(l, top, d_k, thr, c, jumped):
    """Judges one population's tempering increment.  l: its log-likelihoods;
    top = 1 - tau_in (float64); d_k: the float32 increment under test; jumped:
    whether the answer under test is exactly the no-root answer (delta =
    1 - tau_in in float32).  Returns (ok, kind, detail), kind one of "nan",
    "bracket", "jump", "exempt"."""
    l = np.asarray(l, np.float64)
    if np.isnan(l).any():  # the reference's f(top) is NaN: not < 0, so no root-find
        return bool(jumped), "nan", "NaN log-likelihood: expected delta = 1 - tau"
    ftop = ess64(l, top) - thr
    if ftop < 0:
        d = float(d_k)
        tol = 1e-6 + 1e-6 * d
        th = theta_of(d, l, c)
        hi, lo = ess64(l, d + tol), ess64(l, d - tol)
        need = max(hi / thr - 1.0, 1.0 - lo / thr) / th
        ok = hi <= thr * (1 + th) and lo >= thr * (1 - th)
        return ok, "bracket", (f"d={d:.9g} ESS64(d+tol)/thr-1={hi / thr - 1:.3e} "
                               f"ESS64(d-tol)/thr-1={lo / thr - 1:.3e} theta={th:.3e} "
                               f"used={need:.3f}")
    th = theta_of(top, l, c)
    if abs(ftop) / thr <= th:
        return True, "exempt", f"|f(top)|/thr={abs(ftop) / thr:.3e} <= theta={th:.3e}"
    return bool(jumped), "jump", f"f(top)/thr={ftop / thr:.3e}: expected delta = 1 - tau"


def jump_temperature(tau_in):
    """float32(tau_in + float32(1 - tau_in)), 1 - tau_in formed in float64."""
    tau_in = np.asarray(tau_in, F32)
    top = (1.0 - tau_in.astype(np.float64)).astype(F32)
    return (tau_in + top).astype(F32)


def check_tiles(ll, tau_in, tau_out, thr, c, details=None):
    """increment_check of every tile of a launch.  Returns (failures,
    n_exempt), failures a list of messages; every tile's figures are appended
    to `details` when it is a list."""
    tau_in, tau_out = np.asarray(tau_in, F32), np.asarray(tau_out, F32)
    d_k = (tau_out - tau_in).astype(F32)
    jump = jump_temperature(tau_in)
    bad, n_exempt = [], 0
    for t in range(tau_in.size):
        ok, kind, detail = increment_check(ll[t], 1.0 - float(tau_in[t]), d_k[t], thr, c,
                                           tau_out[t] == jump[t])
        n_exempt += kind == "exempt"
        if details is not None:
            details.append(f"tile {t} ({kind}): {detail}")
        if not ok:
            bad.append(f"tile {t} ({kind}): tau {tau_in[t]:.9g} -> {tau_out[t]:.9g}; {detail}")
    return bad, n_exempt


def oracle_tau_out(ll, tau_in, thr, dtype=np.float32):
    """The oracle's temper (smc_oracle.temper) per tile of ll [T, n], without
    the tile's -inf particles (weight 0 at every delta > 0; brentq itself
    stops at f(0) = NaN with them)."""
    tau_in = np.asarray(tau_in, F32)
    out = np.empty_like(tau_in)
    for t in range(tau_in.size):
        l = np.asarray(ll[t])
        l = l[~np.isneginf(l)]
        out[t] = O.temper(l[None, None], tau_in[t].reshape(1, 1), thr, dtype)[0][0, 0]
    return out


@functools.lru_cache(maxsize=None)
def measured_c_raw():
    """Largest relative difference between the float32-mode and float64-mode
    oracle ESS at the float64 root, over the offset-0 tiles of every count
    that have a root."""
    worst = 0.0
    for N in ALL_N:
        ll, tau, _, thr = tile_inputs(N)
        for t, (kind, _, _, offset, _) in enumerate(TILES):
            if kind != "chi2" or offset != 0.0:
                continue
            top = 1.0 - float(tau[t])
            if top <= 0 or O.tempering_objective(ll[t], top, thr) >= 0:
                continue
            root = brentq(lambda d: O.tempering_objective(ll[t], d, thr), 0.0, top,
                          xtol=1e-12, rtol=1e-12)
            e64 = O.tempering_objective(ll[t], root, thr) + thr
            e32 = O.tempering_objective(ll[t], root, thr, np.float32) + thr
            worst = max(worst, abs(e32 - e64) / e64)
    return worst


def measured_c():
    return max(4.0 * measured_c_raw(), 4e-6)


def weight_rtol(d, l):
    """1e-5 + 2^-22 * max|d * l|: the float32 products d * l_i and d * lmax
    against the oracle's float64 ones."""
    l = np.asarray(l, np.float64)
    return 1e-5 + 2.0 ** -22 * abs(float(d)) * float(np.abs(l[np.isfinite(l)]).max())


def log_weights_f32(d, l):
    """nan_to_num(float32(d) * l, nan=-inf): one float32 multiply per element."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = (F32(d) * np.asarray(l, F32)).astype(F32)
    return np.nan_to_num(x, nan=-np.inf)


# ---------------------------------------------------------------------------
# aggregation segments
# ---------------------------------------------------------------------------
AGG_N = (5000, 1536)
AGG_GAP = 7
AGG_TAU = (0.0, 0.3)
_AGG_LENGTHS = {
    5000: ((0, 1, 63, 449, 512, 513, 1000, "gap", "rest"),
           (1000, 513, "gap", 0, 512, 449, 63, 1, "rest")),
    # (the eight lengths sum past 1536: its two tiles share them)
    1536: ((0, 1, 63, 449, 512, "gap", "rest"),
           (513, 0, 1, 63, "gap", 449, "rest")),
}


@functools.lru_cache(maxsize=None)
def agg_inputs(N):
    """Two tiles of hand-made segments.  Returns (ll_parent [3,N], ll_child
    [3,N] (row 2: guard), l = float32(parent - child) [2,N], segments: a list
    of (tile, first particle, length), in_segment [2,N] bool).  Particles of
    no segment hold l = +3e38."""
    rng = np.random.default_rng([N, 77])
    child = (rng.normal(0, 5, (3, N))).astype(F32)
    l = np.full((3, N), GUARD, F32)
    segs, inseg = [], np.zeros((2, N), bool)
    scales = (3.0, 40.0, 400.0)
    for t, spec in enumerate(_AGG_LENGTHS[N]):
        s0 = 0
        for k, n in enumerate(spec):
            if n == "gap":
                s0 += AGG_GAP
                continue
            if n == "rest":
                n = N - s0
            assert n >= 0 and s0 + n <= N
            segs.append((t, s0, n))
            if n:
                l[t, s0:s0 + n] = place_adversarially(
                    chi2_loglik(rng, n, scales[k % 3], -50.0 * (k % 2)))
                inseg[t, s0:s0 + n] = True
            s0 += n
        assert s0 == N
    parent = (l.astype(np.float64) + child).astype(F32)
    parent[l == GUARD] = GUARD
    child[l == GUARD] = 0
    with np.errstate(over="ignore"):
        leff = (parent - child).astype(F32)
    for a in (parent, child, leff):
        a.setflags(write=False)
    return parent, child, leff[:2], tuple(segs), inseg
