"""The tile pass (tile.h: temper -> reweight -> resampling indices, launched by
smc_kernels.hip) through the C ABI against the float64 oracle at ragged
particle counts: every tile_kernel<512, PER> instantiation at its full size
(the unmasked fast path) and at masked neighbours (tests/_tile_cases.py, which
also states the acceptance criteria and why the tempering increment is judged
by its ESS bracket).  Each launch is six tiles of unlike scale and entry
temperature with their largest log-likelihoods on the tile's boundaries, a
+3e38 row behind the last tile and a sentinel row behind every output.
tests/test_tile_oracle_host.py shows on the CPU that these criteria reject an
oracle that drops the last particle, reads one past the end or uses the full
tile's threshold."""
import numpy as np
import pytest
import torch

from oracle import agg_oracle as A
from oracle import smc_oracle as O
from tests import _tile_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SENT = F32(-12345.5)   # float outputs' guard and prefill
ISENT = -99            # index outputs' guard and prefill
METHODS = ("systematic", "multinomial")


def D(x):
    return torch.from_numpy(np.array(x)).to(DEV)  # (a copy: some inputs are read-only)


def H(t):
    return t.detach().cpu().numpy()


def _method(name):
    from smcdet_amd import _hip
    return (_hip.SMCDET_RESAMPLE_SYSTEMATIC if name == "systematic"
            else _hip.SMCDET_RESAMPLE_MULTINOMIAL)


class Buffers:
    """The tile pass's buffers for T tiles of N particles, each with one guard
    row (element) more than the launch is told about."""

    def __init__(self, ll, tau_in, lz_in, prefill=SENT):
        ll = np.asarray(ll, F32)
        self.T, self.N = len(tau_in), ll.shape[1]
        assert ll.shape[0] == self.T + 1
        T, N = self.T, self.N
        self.ll = D(ll)
        self.tau = D(np.append(np.asarray(tau_in, F32), SENT))
        self.prev = D(np.full(T + 1, prefill, F32))
        self.lw = D(np.full((T + 1, N), prefill, F32))
        self.W = D(np.full((T + 1, N), prefill, F32))
        self.ess = D(np.full(T + 1, prefill, F32))
        self.lz = D(np.append(np.asarray(lz_in, F32), SENT))
        self.idx = D(np.full((T + 1, N), ISENT, np.int64))

    def out(self):
        """Outputs as numpy, after asserting that every guard is untouched."""
        torch.cuda.synchronize()
        T = self.T
        res = {}
        for k in ("tau", "prev", "lw", "W", "ess", "lz", "idx"):
            a = H(getattr(self, k))
            sent = ISENT if k == "idx" else SENT
            assert (a[T] == sent).all(), f"{k}: guard row overwritten"
            res[k] = a[:T].copy()
        return res


def temper_reweight(b, thr, method, seed=7, offset=3, flags=0, fin=None, it=0, live=None,
                    go=None, live_host=None):
    from smcdet_amd import _hip
    return _hip.lib().smcdet_temper_reweight(
        _hip.ptr(b.ll), _hip.ptr(b.tau), _hip.ptr(b.prev), _hip.ptr(b.lw), _hip.ptr(b.W),
        _hip.ptr(b.ess), _hip.ptr(b.lz), b.T, b.N, float(thr), _method(method), seed, offset,
        _hip.ptr(b.idx), flags, _hip.ptr(fin), it, _hip.ptr(live),
        _hip.ptr(go), live_host, _hip.stream_of(b.ll))


def three_calls(b, thr, method, seed=7, offset=3, u=None):
    from smcdet_amd import _hip
    L, st = _hip.lib(), _hip.stream_of(b.ll)
    _hip.check(L.smcdet_temper(_hip.ptr(b.ll), _hip.ptr(b.tau), _hip.ptr(b.prev), b.T, b.N,
                               float(thr), st), "temper")
    _hip.check(L.smcdet_update_weights(_hip.ptr(b.ll), _hip.ptr(b.tau), _hip.ptr(b.prev),
                                       _hip.ptr(b.lw), _hip.ptr(b.W), _hip.ptr(b.ess),
                                       _hip.ptr(b.lz), b.T, b.N, st), "update_weights")
    _hip.check(L.smcdet_resample_index(_hip.ptr(b.W), b.T, b.N, _method(method), seed, offset,
                                       _hip.ptr(u), _hip.ptr(b.idx), st), "resample_index")


def replay_uniforms(T, N, seed):
    """U [T] (systematic) and u [T, N] (multinomial), with the uniforms 0 and
    nextafter(1, 0) planted in every tile."""
    rng = np.random.default_rng([seed, N])
    U = rng.random(T).astype(F32)
    U[0], U[-1] = 0.0, np.nextafter(F32(1), F32(0))
    u = rng.random((T, N)).astype(F32)
    u[:, 0] = 0.0
    u[:, N // 2] = np.nextafter(F32(1), F32(0))
    u[:, N - 1] = np.where(np.arange(T) % 2 == 0, np.nextafter(F32(1), F32(0)), 0.0)
    return U, u


def check_replayed_indices(W):
    """smcdet_resample_index on the weights W [T, N] (a kernel's own) with
    replayed uniforms: bit-equal to the oracles, both methods; its output's
    guard row stays."""
    from smcdet_amd import _hip
    T, N = W.shape
    U, u = replay_uniforms(T, N, 11)
    Wd = D(W)
    for method, uu in (("systematic", U), ("multinomial", u)):
        idx = D(np.full((T + 1, N), ISENT, np.int64))
        ud = D(uu)
        _hip.check(_hip.lib().smcdet_resample_index(
            _hip.ptr(Wd), T, N, _method(method), 0, 0, _hip.ptr(ud), _hip.ptr(idx),
            _hip.stream_of(Wd)), "resample_index")
        got = H(idx)
        assert (got[T] == ISENT).all(), "idx: guard row overwritten"
        if method == "systematic":
            ref = O.systematic_resample_index(W[None], U[None])[0]
        else:
            ref = O.multinomial_resample_index(W, u)
        np.testing.assert_array_equal(got[:T], ref, err_msg=f"{method} N={N}")


def check_against_oracle(ll, tau_in, lz_in, thr, out, skip=()):
    """The criteria of tests/_tile_cases.py on one launch's outputs (tiles in
    `skip` excepted)."""
    c = C.measured_c()
    T, N = len(tau_in), ll.shape[1]
    keep = [t for t in range(T) if t not in skip]
    tau_in = np.asarray(tau_in, F32)
    lz_in = np.asarray(lz_in, F32)
    details = []
    bad, n_exempt = C.check_tiles(ll, tau_in, out["tau"], thr, c, details)
    print(f"N={N}", *details, sep="\n  ")
    bad = [m for m in bad if int(m.split()[1]) not in skip]
    assert not bad, "\n".join([f"N={N}"] + bad)
    assert n_exempt == 0
    np.testing.assert_array_equal(out["prev"][keep].view(np.uint32),
                                  tau_in[keep].view(np.uint32))
    d = (out["tau"] - tau_in).astype(F32)
    Wo, esso, lzo = O.update_weights(ll[:T, None], out["tau"][:, None], tau_in[:, None],
                                     lz_in[:, None], N)
    for t in keep:
        msg = f"N={N} tile {t}"
        np.testing.assert_array_equal(out["lw"][t].view(np.uint32),
                                      C.log_weights_f32(d[t], ll[t]).view(np.uint32),
                                      err_msg=msg)
        rt = C.weight_rtol(d[t], ll[t])
        np.testing.assert_allclose(out["W"][t], Wo[t, 0], rtol=rt, atol=1e-12, err_msg=msg)
        np.testing.assert_allclose(out["ess"][t], esso[t, 0], rtol=rt, err_msg=msg)
        np.testing.assert_allclose(out["lz"][t], lzo[t, 0], rtol=1e-6, atol=1e-4, err_msg=msg)
        assert abs(out["W"][t].astype(np.float64).sum() - 1.0) <= N * 2.0 ** -24, msg
        assert (out["W"][t][~np.isfinite(ll[t])] == 0).all(), msg
    assert out["idx"][keep].min() >= 0 and out["idx"][keep].max() < N


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", C.ALL_N)
def test_temper_reweight_vs_oracle(N, method):
    """smcdet_temper_reweight, one launch: increments inside their ESS
    bracket (or exactly 1 - tau), temperature_prev, float32 log weights bit
    for bit, W / ESS / log Z against the float64 oracle at the kernel's own
    temperatures, untouched guards; then the indices of those weights with
    replayed uniforms, bit-equal to the oracle's."""
    ll, tau_in, lz_in, thr = C.tile_inputs(N)
    b = Buffers(ll, tau_in, lz_in)
    from smcdet_amd import _hip
    _hip.check(temper_reweight(b, thr, method), "temper_reweight")
    out = b.out()
    check_against_oracle(ll, tau_in, lz_in, thr, out)
    # the delta = 0 tile: uniform weights, ESS = N, log Z unchanged, exactly
    t = C.T - 1
    assert out["tau"][t] == 1.0 and (out["W"][t] == F32(1) / F32(N)).all()
    assert out["ess"][t] == F32(N) and out["lz"][t] == lz_in[t]
    if method == "systematic":
        assert (np.diff(out["idx"], axis=1) >= 0).all()
        check_replayed_indices(out["W"])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("N", C.ALL_N)
def test_three_calls_equal_one(N, method):
    """smcdet_temper, smcdet_update_weights and smcdet_resample_index against
    smcdet_temper_reweight on the same inputs, seed and offset: every output
    bit-identical (the fused form takes the weights' exponent maximum as
    fl(d * lmax) instead of reducing it: tile.h's claim that the two are
    equal)."""
    from smcdet_amd import _hip
    ll, tau_in, lz_in, thr = C.tile_inputs(N)
    one, three = Buffers(ll, tau_in, lz_in), Buffers(ll, tau_in, lz_in)
    _hip.check(temper_reweight(one, thr, method), "temper_reweight")
    three_calls(three, thr, method)
    a, b = one.out(), three.out()
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == F32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        np.testing.assert_array_equal(x, y, err_msg=f"N={N} {k}")


@pytest.mark.parametrize("N", [1000, 4100])
def test_nonfinite_loglikelihoods(N):
    """-inf particles get weight 0 and the rest obey the criteria without
    them; a NaN particle sends its tile to temperature 1 (the reference's
    f(1 - tau) is NaN, so it takes no root) with weight 0."""
    from smcdet_amd import _hip
    ll, tau_in, lz_in, thr = C.nonfinite_inputs(N)
    for method in METHODS:
        b = Buffers(ll, tau_in, lz_in)
        _hip.check(temper_reweight(b, thr, method), "temper_reweight")
        out = b.out()
        check_against_oracle(ll, tau_in, lz_in, thr, out)
        jump = C.jump_temperature(tau_in)
        assert out["tau"][1] == jump[1] and out["tau"][3] == jump[3]
        assert out["tau"][0] < 1 and out["tau"][2] < 1
        three = Buffers(ll, tau_in, lz_in)
        three_calls(three, thr, method)
        for k, v in three.out().items():
            np.testing.assert_array_equal(v, out[k], err_msg=f"N={N} {k}")
    check_replayed_indices(out["W"])


# ---------------------------------------------------------------------------
# flags, bookkeeping, predicate
# ---------------------------------------------------------------------------
FLAG_N = 1000
FLAG_TAU = np.array([0.0, 1.0, 0.5, 1.0, 0.999], F32)


def _flag_inputs(T=5):
    rng = np.random.default_rng(99)
    ll = np.empty((T + 1, FLAG_N), F32)
    for t, scale in enumerate((3.0, 40.0, 40.0, 400.0, 3.0)[:T]):
        ll[t] = C.place_adversarially(C.chi2_loglik(rng, FLAG_N, scale, 0.0))
    ll[T] = C.GUARD
    return ll, FLAG_TAU[:T].copy(), np.arange(T, dtype=F32) * 2.5 - 3, 0.5 * FLAG_N


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("freeze", [True, False], ids=["freeze", "nofreeze"])
def test_flags_finished_iter_and_live(freeze, method):
    from smcdet_amd import _hip
    ll, tau_in, lz_in, thr = _flag_inputs()
    T, N = 5, FLAG_N
    b = Buffers(ll, tau_in, lz_in)
    fin = D(np.array([-1, 3, -1, -1, -1, ISENT], np.int32))
    live = D(np.array([0, 0, 0, ISENT], np.int32))
    host = _hip.HostInts(2)
    host[0], host[1] = ISENT, ISENT
    _hip.check(temper_reweight(b, thr, method, flags=_hip.SMCDET_SMC_FREEZE_DONE if freeze else 0,
                               fin=fin, it=9, live=live, live_host=host.dev(0)),
               "temper_reweight")
    out = b.out()
    done = (1, 3)
    check_against_oracle(ll, tau_in, lz_in, thr, out, skip=done if freeze else ())
    assert out["tau"][0] < 1 and out["tau"][2] < 1 and out["tau"][4] == 1
    for t in done:
        assert out["tau"][t] == 1.0
        assert (out["W"][t] == F32(1) / F32(N)).all()
        assert (out["lw"][t] == 0).all()
        if freeze:
            assert out["prev"][t] == 1.0
            assert out["lz"][t] == lz_in[t] and out["ess"][t] == SENT  # prefilled values kept
            np.testing.assert_array_equal(out["idx"][t], np.arange(N))
        else:
            assert out["prev"][t] == 1.0 and out["ess"][t] == F32(N) and out["lz"][t] == lz_in[t]
    np.testing.assert_array_equal(H(fin), [-1, 3, -1, 9, 9, ISENT])
    np.testing.assert_array_equal(H(live), [0, 0, 2, ISENT])
    assert host[0] == 2 and host[1] == ISENT
    check_replayed_indices(out["W"])


@pytest.mark.parametrize("tau0,expect", [(0.0, 1), (1.0, 0)])
def test_live_count_single_tile(tau0, expect):
    """T = 1 takes tile_status's path without the ticket."""
    from smcdet_amd import _hip
    ll, _, lz_in, thr = _flag_inputs(1)
    tau_in = np.array([tau0], F32)
    for flags in (0, _hip.SMCDET_SMC_FREEZE_DONE):
        b = Buffers(ll, tau_in, lz_in)
        fin = D(np.array([-1, ISENT], np.int32))
        live = D(np.array([0, 0, 0, ISENT], np.int32))
        host = _hip.HostInts(1)
        host[0] = ISENT
        _hip.check(temper_reweight(b, thr, "systematic", flags=flags, fin=fin, it=4, live=live,
                                   live_host=host.dev(0)), "temper_reweight")
        out = b.out()
        assert (out["tau"][0] < 1) == bool(expect)
        np.testing.assert_array_equal(H(live), [0, 0, expect, ISENT])
        np.testing.assert_array_equal(H(fin), [-1 if expect else 4, ISENT])
        assert host[0] == expect


def _assert_untouched(b, tau_in, lz_in):
    torch.cuda.synchronize()
    T = b.T
    np.testing.assert_array_equal(H(b.tau)[:T], tau_in)
    np.testing.assert_array_equal(H(b.lz)[:T], lz_in)
    for k in ("prev", "lw", "W", "ess"):
        assert (H(getattr(b, k)) == SENT).all(), k
    assert (H(b.idx) == ISENT).all()


def test_go_zero_writes_nothing():
    from smcdet_amd import _hip
    ll, tau_in, lz_in, thr = _flag_inputs()
    b = Buffers(ll, tau_in, lz_in)
    fin = D(np.array([-1, 3, -1, -1, -1], np.int32))
    live = D(np.zeros(4, np.int32))
    go = D(np.zeros(1, np.int32))
    host = _hip.HostInts(1)
    host[0] = ISENT
    _hip.check(temper_reweight(b, thr, "systematic", fin=fin, it=9, live=live, go=go,
                               live_host=host.dev(0)), "temper_reweight")
    _assert_untouched(b, tau_in, lz_in)
    np.testing.assert_array_equal(H(fin), [-1, 3, -1, -1, -1])
    assert (H(live) == 0).all() and host[0] == ISENT
    # and with go = 1 the same launch runs
    go.fill_(1)
    _hip.check(temper_reweight(b, thr, "systematic", fin=fin, it=9, live=live, go=go,
                               live_host=host.dev(0)), "temper_reweight")
    torch.cuda.synchronize()
    assert H(live)[2] == 2 and host[0] == 2 and (H(b.W)[:5] != SENT).all()


def test_too_many_particles_is_unsupported():
    """N = 16385 > 512 * 32: SMCDET_EUNSUPPORTED before any device work."""
    from smcdet_amd import _hip
    N = 16385
    ll = np.zeros((3, N), F32)
    tau_in, lz_in = np.zeros(2, F32), np.ones(2, F32)
    b = Buffers(ll, tau_in, lz_in)
    L, st = _hip.lib(), _hip.stream_of(b.ll)
    assert temper_reweight(b, 0.5 * N, "systematic") == -2
    assert L.smcdet_temper(_hip.ptr(b.ll), _hip.ptr(b.tau), _hip.ptr(b.prev), 2, N, 0.5 * N,
                           st) == -2
    assert L.smcdet_update_weights(_hip.ptr(b.ll), _hip.ptr(b.tau), _hip.ptr(b.prev),
                                   _hip.ptr(b.lw), _hip.ptr(b.W), _hip.ptr(b.ess),
                                   _hip.ptr(b.lz), 2, N, st) == -2
    assert L.smcdet_resample_index(_hip.ptr(b.ll), 2, N, _method("systematic"), 0, 0, None,
                                   _hip.ptr(b.idx), st) == -2
    _assert_untouched(b, tau_in, lz_in)


# ---------------------------------------------------------------------------
# aggregation segments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.AGG_N)
def test_aggregation_segments(N):
    """smcdet_aggregate_temper / smcdet_aggregate_reweight on hand-made
    segments of two tiles (lengths 0, 1, 63, 449, 512, 513, 1000 and the rest,
    with a gap of particles in no segment that hold +3e38): per segment the
    increment's ESS bracket at thr = 0.5 * length, exactly 1 for the empty
    segment; w_intra, the group evidence and ESS against the float64 oracle;
    replayed intracount indices bit-equal to the oracle's; sentinels kept
    outside the segments and behind the last tile."""
    from smcdet_amd import _hip
    c = C.measured_c()
    parent, child, l, segs, inseg = C.agg_inputs(N)
    T, G = 2, len(segs)
    tau_in = np.array(C.AGG_TAU, F32)
    st_, ss_, sl_ = (D(np.array([s[k] for s in segs], np.int32)) for k in range(3))
    P, Cd, tau = D(parent), D(child), D(tau_in)
    delta = D(np.full(G + 1, SENT, F32))
    L, st = _hip.lib(), _hip.stream_of(P)
    _hip.check(L.smcdet_aggregate_temper(_hip.ptr(P), _hip.ptr(Cd), _hip.ptr(tau), T, N, G,
                                         _hip.ptr(st_), _hip.ptr(ss_), _hip.ptr(sl_), 0.5,
                                         _hip.ptr(delta), st), "aggregate_temper")
    dk = H(delta)
    assert dk[G] == SENT
    bad, n_exempt = [], 0
    for g, (t, s0, n) in enumerate(segs):
        top = 1.0 - float(tau_in[t])
        if n == 0:
            assert dk[g] == 1.0
            continue
        ok, kind, detail = C.increment_check(l[t, s0:s0 + n], top, dk[g], 0.5 * n, c,
                                             dk[g] == F32(top))
        n_exempt += kind == "exempt"
        if not ok:
            bad.append(f"segment {g} {segs[g]} ({kind}): delta {dk[g]:.9g}; {detail}")
    assert not bad, "\n".join(bad)
    assert n_exempt == 0
    # reweight at the tile's increment: the minimum over its segments
    d_tile = np.array([min(dk[g] for g, s in enumerate(segs) if s[0] == t) for t in range(T)], F32)
    tau_new = (tau_in + d_tile).astype(F32)
    lnc_in = (np.arange(G, dtype=F32) * 1.5 - 4).astype(F32)
    lw = D(np.full((T + 1, N), SENT, F32))
    wi = D(np.full((T + 1, N), SENT, F32))
    idx = D(np.full((T + 1, N), ISENT, np.int64))
    lnc = D(np.append(lnc_in, SENT))
    ess = D(np.full(G + 1, SENT, F32))
    rng = np.random.default_rng([N, 5])
    u = rng.random((T, N)).astype(F32)
    for t, s0, n in segs:
        if n:
            u[t, s0] = 0.0
            u[t, s0 + n - 1] = np.nextafter(F32(1), F32(0))
    tn, ud = D(tau_new), D(u)
    _hip.check(L.smcdet_aggregate_reweight(
        _hip.ptr(P), _hip.ptr(Cd), _hip.ptr(tn), _hip.ptr(tau), T, N, G, _hip.ptr(st_),
        _hip.ptr(ss_), _hip.ptr(sl_), _hip.ptr(lw), _hip.ptr(wi), _hip.ptr(lnc), _hip.ptr(ess),
        0, 0, _hip.ptr(ud), _hip.ptr(idx), st), "aggregate_reweight")
    torch.cuda.synchronize()
    lw, wi, idx, lnc, ess = H(lw), H(wi), H(idx), H(lnc), H(ess)
    assert (lw[T] == SENT).all() and (wi[T] == SENT).all() and (idx[T] == ISENT).all()
    assert lnc[G] == SENT and ess[G] == SENT
    out_of = ~inseg
    assert (lw[:T][out_of] == SENT).all() and (wi[:T][out_of] == SENT).all()
    assert (idx[:T][out_of] == ISENT).all()
    d = (tau_new - tau_in).astype(F32)
    for g, (t, s0, n) in enumerate(segs):
        msg = f"N={N} segment {g} {segs[g]}"
        if n == 0:
            assert lnc[g] == lnc_in[g], msg  # an empty group's evidence stays
            continue
        sl = slice(s0, s0 + n)
        lg = l[t, sl]
        np.testing.assert_array_equal(lw[t, sl].view(np.uint32),
                                      (d[t] * lg).astype(F32).view(np.uint32), err_msg=msg)
        w_o, _, lnc_o = A.update_weights_groups(lg[None, None], [[[n]]], tau_new[t].reshape(1, 1),
                                                tau_in[t].reshape(1, 1), [[[float(lnc_in[g])]]])
        rt = C.weight_rtol(d[t], lg)
        np.testing.assert_allclose(wi[t, sl], w_o[0, 0], rtol=rt, atol=1e-12, err_msg=msg)
        np.testing.assert_allclose(ess[g], 1.0 / (w_o[0, 0] ** 2).sum(), rtol=rt, err_msg=msg)
        np.testing.assert_allclose(lnc[g], lnc_o[0][0][0], rtol=1e-6, atol=1e-4, err_msg=msg)
        assert abs(wi[t, sl].astype(np.float64).sum() - 1.0) <= n * 2.0 ** -24, msg
        assert idx[t, sl].min() >= s0 and idx[t, sl].max() < s0 + n, msg
    by_tile = [[[(s0, n) for (t, s0, n) in segs if t == tt] for tt in range(T)]]
    wk = np.where(inseg, wi[:T], 0).astype(F32)
    ref = A.intracount_resample_index(wk[None], by_tile, u[None])[0]
    np.testing.assert_array_equal(idx[:T][inseg], ref[inseg])
