"""The tile-pass criteria on the CPU (tests/_tile_cases.py): the float32-mode
oracle stays inside them on every input, three deliberately wrong numpy
variants of the oracle fall outside them at every particle count, and the
replayed-uniform resampling oracles agree with a loop written from the
definition.  No GPU, no project kernel: this is the evidence that
tests/test_gpu_tile_pass.py would notice a subtly wrong kernel."""
import numpy as np
import pytest

from oracle import agg_oracle as A
from oracle import smc_oracle as O
from tests import _tile_cases as C

F32 = np.float32


def test_case_table_covers_every_instantiation():
    for per, counts in C.N_CASES.items():
        assert 512 * per in counts
        assert all(C.per_of(n) == per for n in counts)
        assert any(n != 512 * per for n in counts)
    ll, tau, lz, thr = C.tile_inputs(1536)
    assert ll.shape == (C.T + 1, 1536) and (ll[C.T] == C.GUARD).all()
    for t in range(4):  # adversarial placement
        order = np.argsort(ll[t])[::-1]
        assert list(order[:3]) == [1535, 0, 1023]


def test_measured_c_is_documented():
    raw = C.measured_c_raw()
    print(f"largest float32-vs-float64 oracle ESS difference at the root: {raw:.3e}; "
          f"c = {C.measured_c():.3e}")
    assert C.measured_c() == max(4 * raw, 4e-6)
    # the figures the module docstring records (numpy's float32 summation order
    # depends on the CPU's vector width: the same to a factor of two)
    assert "is 1.6e-06, so c = 6.3e-06" in C.__doc__
    assert 0.8e-6 < raw < 3.2e-6


@pytest.fixture(scope="module")
def c():
    return C.measured_c()


def test_float32_oracle_stays_inside_the_criteria(c):
    """Every input, the float32-mode oracle's increment: the bracket holds
    with the measured c, and no tile needs the near-threshold exemption."""
    exempt, worst = 0, -np.inf
    for N in C.ALL_N:
        ll, tau, _, thr = C.tile_inputs(N)
        out = C.oracle_tau_out(ll[:C.T], tau, thr, np.float32)
        bad, ne = C.check_tiles(ll, tau, out, thr, c)
        assert not bad, (N, bad)
        exempt += ne
        d = (out - tau).astype(F32)
        for t in range(C.T):
            _, kind, detail = C.increment_check(ll[t], 1.0 - float(tau[t]), d[t], thr, c, True)
            if kind == "bracket":
                worst = max(worst, float(detail.rsplit("used=", 1)[1]))
    print(f"float32 oracle: largest share of theta used {worst:.3f}; exempt tiles {exempt}")
    assert exempt == 0
    assert worst <= 1.0


def test_nonfinite_inputs_stay_inside_the_criteria(c):
    for N in (1000, 4100):
        ll, tau, _, thr = C.nonfinite_inputs(N)
        out = C.oracle_tau_out(ll[:C.T], tau, thr, np.float32)
        bad, ne = C.check_tiles(ll, tau, out, thr, c)
        assert not bad and ne == 0, (N, bad, ne)
        jump = C.jump_temperature(tau)
        assert out[1] == jump[1] and out[3] == jump[3]  # the NaN tiles


def _variant_inputs(name, N):
    ll, tau, _, thr = C.tile_inputs(N)
    flat = ll.reshape(-1)
    if name == "drop_last":
        rows = [flat[t * N:t * N + N - 1] for t in range(C.T)]
    elif name == "one_past_end":
        rows = [flat[t * N:t * N + N + 1] for t in range(C.T)]
    else:
        rows = [ll[t] for t in range(C.T)]
    thr_v = 0.5 * 512 * C.per_of(N) if name == "full_threshold" else thr
    return rows, thr_v


@pytest.mark.parametrize("name", ["drop_last", "one_past_end", "full_threshold"])
def test_criteria_reject_wrong_variants(name, c):
    """The float32-mode oracle run on every tile without its last particle,
    with the element after its last particle, or with the threshold of a full
    tile (0.5 * 512 * PER): rejected at every particle count above 2 (the
    threshold variant at every masked count: at N = 512 * PER it is the
    right threshold)."""
    with np.errstate(over="ignore", invalid="ignore"):
        for N in C.ALL_N:
            if N <= 2 or (name == "full_threshold" and N == 512 * C.per_of(N)):
                continue
            ll, tau, _, thr = C.tile_inputs(N)
            rows, thr_v = _variant_inputs(name, N)
            # (a threshold at or above the population size has its root at delta = 0)
            out = np.array([tau[t] if thr_v >= r.size else
                            C.oracle_tau_out(r[None], tau[t:t + 1], thr_v, np.float32)[0]
                            for t, r in enumerate(rows)], F32)
            bad, _ = C.check_tiles(ll, tau, out, thr, c)
            assert bad, f"{name} passes the criteria at N = {N}"


# ---------------------------------------------------------------------------
# the replayed-uniform resampling oracles against the definition
# ---------------------------------------------------------------------------
def _loop_multinomial(W, u):
    run, bins = 0.0, []
    for w in W:
        run += float(F32(w))
        bins.append(F32(run))
    out = []
    for x in u:
        target = F32(F32(x) * bins[-1])
        i = 0
        while i < len(bins) and not bins[i] > target:
            i += 1
        out.append(min(i, len(bins) - 1))
    return out


HAND = [
    [0.25, 0.25, 0.25, 0.25],                 # ties
    [0.0, 0.0, 0.5, 0.0, 0.0, 0.5, 0.0],      # zero-weight runs, also at both ends
    [0.1, 0.2, 0.3],                          # mass short of 1
    [1.0],
    [0.0, 0.0, 0.0],                          # no mass at all: every index clamps to the last
    [1e-8, 0.5, 1e-8, 0.5 - 2e-8],
]
U_HAND = [0.0, 0.25, 0.5, 0.75, float(np.nextafter(F32(1), F32(0))), 0.1, 0.999, 1 / 3]


def test_multinomial_oracle_matches_definition():
    rng = np.random.default_rng(4)
    for W in HAND + [rng.gamma(0.3, size=37).tolist()]:
        u = (U_HAND * len(W))[:max(len(W), 1)]
        u = (u + U_HAND)[:len(W)]
        got = O.multinomial_resample_index(np.array(W, F32), np.array(u, F32))
        assert got.tolist() == _loop_multinomial(W, u), W
    # leading dimensions, and one uniform per particle of every tile
    W = rng.random((2, 3, 11)).astype(F32)
    u = rng.random((2, 3, 11)).astype(F32)
    got = O.multinomial_resample_index(W, u)
    for h in range(2):
        for w in range(3):
            assert got[h, w].tolist() == _loop_multinomial(W[h, w], u[h, w])


def test_intracount_oracle_matches_definition():
    rng = np.random.default_rng(5)
    segs = [(0, 4), (4, 0), (4, 7), (13, 3), (16, 1), (17, 3), (20, 4)]  # 11..12 in no segment
    w = np.zeros(24, F32)
    for (a, n), W in zip([s for s in segs if s[1]], HAND):
        assert n == len(W)
        w[a:a + n] = W
    w[11:13] = 9.0
    u = np.array((U_HAND * 3)[:24], F32)
    got = A.intracount_resample_index(w[None, None], [[segs]], u[None, None])[0, 0]
    want = np.full(24, -1)
    for a, n in segs:
        if n:
            want[a:a + n] = a + np.array(_loop_multinomial(w[a:a + n], u[a:a + n]))
    assert got.tolist() == want.tolist()
    assert (got[11:13] == -1).all()
    # contiguous group sizes, as sort_by_count returns them
    sizes = [5, 0, 8, 11]
    w2 = rng.random(24).astype(F32)
    got = A.intracount_resample_index(w2[None, None], [[sizes]], u[None, None])[0, 0]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            assert got[a:b].tolist() == (a + np.array(_loop_multinomial(w2[a:b], u[a:b]))).tolist()
