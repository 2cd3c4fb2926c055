"""The Philox instantiations of the three MCMC sweep kernels (what the product
and bench.py run: REPLAY = false in mh_kernel.hip / mala_kernel.hip, the
r_comp == null path of chain_kernel.hip) against their replay twins, which
every oracle comparison of the suite runs through.

Each case runs the kernel twice from the same inputs through the public API:
once drawing in-kernel from PhiloxStream(SEED) at a set offset, once
replaying the arrays tests/_streams.py computes on the host for that seed and
offset.  Everything the call returns must be equal bit for bit: the counter
(offset + k with its carry), the pid of every tile / particle / chain, the
two tags, the component choice among Sj, the lane-to-iteration mapping of
the 64-draw cache and the offsets of successive launches all sit in code the
replay twins skip.

Shapes: N or C = 5 (a workgroup of four waves and a ragged one with a lone
wave 0), two tiles or more (pid depends on the tile), K = 70 iterations
(past the 64-draw refill and the proposal batch cut at it).

Every case also checks that the sweep did something (accept flags of both
kinds, sources that moved, by-count padding that did not): two runs that
both stood still would be equal too.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import _streams as ST
from tests._params import (BASIC_FLUX_SCALE, M71, golden, o_m71_mh, o_m71_model, o_m71_prior,
                           p_basic_mh, p_basic_model, p_basic_prior, p_m71_mh, p_m71_model,
                           p_m71_prior, tiles_of)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 0x3C6EF372A54FF53A  # both key words non-zero and different
K = 70
NP = 5                     # particles per tile / chains per tile
CARRY = 2 ** 32 - 20       # iterations 20.. carry into the counter's high word
GENERIC = 32768            # SMCDET_MH_GENERIC_GEOMETRY, include/smcdet_hip.h


def N(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    """As test_gpu_geometry._bits_equal: floats by their bits."""
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert _bits_equal(a[k], b[k]), k


def _torch_replay(rp):
    return {k: torch.as_tensor(v) for k, v in rp.items()}


@pytest.fixture(scope="module")
def image32():
    """Two 32x32 M71 tiles, [1, 2, 32, 32]."""
    torch.manual_seed(3)
    model, truth = p_m71_model(32), p_m71_prior(32, 0, 40, counts_rate=0.004)
    tiles = []
    for _ in range(2):
        _, l, f = truth.sample(num_catalogs=1, device=DEV)
        tiles.append(model.sample(l, f)[0, 0, :, :, 0])
    return torch.stack(tiles)[None].contiguous()


def _image(name):
    """The tiled image [nH,nW,H,W] of a sweep case."""
    if name == "m71-8x8-2x2":
        t = tiles_of(golden("mh_m71_tiles.npz")["image"], 8)
    elif name == "m71-8x8-1x2":
        t = tiles_of(golden("mh_m71_tiles.npz")["image"], 8)[:1]
    elif name == "basic-16x16-1x2":
        t = np.stack([golden("mh_basic_16x16.npz")["image"]] * 2)[None]
    else:
        raise KeyError(name)
    return torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32), device=DEV)


def _state(shape, S, H, pad, flux_lo, flux_hi, seed, counts=None):
    """locs [nH,nW,N,S,2] uniform over the location box less a margin of 0.5,
    fluxes [nH,nW,N,S] uniform in [flux_lo, flux_hi]; zeros at index >= count."""
    g = torch.Generator().manual_seed(seed)
    locs = torch.rand(*shape, S, 2, generator=g) * (H + 2 * pad - 1.0) - (pad - 0.5)
    fluxes = flux_lo + (flux_hi - flux_lo) * torch.rand(*shape, S, generator=g)
    if counts is not None:
        live = torch.arange(S)[None, None, None] < counts.cpu()[..., None]
        locs, fluxes = locs * live[..., None], fluxes * live
    return locs.to(DEV).contiguous(), fluxes.to(DEV).contiguous()


# ---- the two sweeps ------------------------------------------------------------------
def _mala(K_):
    from smcdet_amd.kernel import SingleComponentMALA
    return SingleComponentMALA(K_, 0.1, 2.5, M71["flux_lower"], M71["flux_upper"])


class Case:
    def __init__(self, family, image, H, S, tau, offset=0, flags=0, by_count=False, basic=False):
        self.family, self.image, self.H, self.S = family, image, H, S
        self.tau, self.offset, self.flags = tau, offset, flags
        self.by_count, self.basic = by_count, basic

    def build(self, image32):
        from smcdet_amd._rng import PhiloxStream
        H, S = self.H, self.S
        self.data = image32 if self.image == "image32" else _image(self.image)
        nH, nW = self.data.shape[:2]
        self.shape = (nH, nW, NP)
        self.counts = torch.full(self.shape, float(S), device=DEV)
        if self.by_count:  # 0..S across the particles, another order in the second tile
            c = torch.arange(NP, dtype=torch.float32) % (S + 1)
            self.counts = torch.stack([c, c.flip(0)])[None].to(DEV).contiguous()
            assert self.counts.shape == self.shape
        if self.basic:
            self.model, self.prior = p_basic_model(H), p_basic_prior(H, S, S)
            self.kernel = p_basic_mh(K)
            rng_f, pad = (BASIC_FLUX_SCALE * 0.9, BASIC_FLUX_SCALE * 3.6), 2
        else:
            self.model = p_m71_model(H)
            self.prior = p_m71_prior(H, 0, S) if self.by_count else p_m71_prior(H, S, S)
            self.kernel = p_m71_mh(K) if self.family == "mh" else _mala(K)
            rng_f, pad = (1.0, 41.0), 4
        self.locs, self.fluxes = _state(self.shape, S, H, pad, *rng_f, seed=11 + S,
                                        counts=self.counts if self.by_count else None)
        self.kernel.debug_flags = self.flags
        self.kernel.component_by_count = self.by_count
        self.kernel.rng = PhiloxStream(SEED)
        self.temperature = torch.tensor(self.tau, device=DEV)
        return self

    def replay(self, offset):
        nH, nW, n = self.shape
        return ST.sweep_replay(self.family, SEED, offset, K, nH, nW, n, self.S,
                               counts=N(self.counts) if self.by_count else None)

    def run(self, state, offset, replay=None, ancestors=None, rate_in=None):
        """One sweep from state = (counts, locs, fluxes): everything it returns
        (and, replaying an MH sweep, its accept trace)."""
        counts, locs, fluxes = state
        rate = torch.empty(*self.shape, self.H * self.H, device=DEV)
        rp = None
        if replay is not None:
            rp = _torch_replay(replay)
            if self.family == "mh":
                rp["trace_accept"] = torch.zeros(K, *self.shape, device=DEV, dtype=torch.uint8)
        self.kernel.rng.offset = offset
        l, f, acc = self.kernel.run(self.data, counts, locs, fluxes, self.temperature,
                                    prior=self.prior, image_model=self.model, replay=rp,
                                    ancestors=ancestors, rate_in=rate_in, rate_out=rate)
        torch.cuda.synchronize()
        out = dict(locs=l, fluxes=f, counts=self.kernel.last_counts,
                   loglik=self.kernel.last_loglik, acc=acc, rate=rate)
        return out, (rp or {}).get("trace_accept")


SWEEPS = {
    "mh-c2-geofixed": Case("mh", "image32", 32, 10, [[0.05, 0.3]]),
    "mh-c2-generic": Case("mh", "image32", 32, 10, [[0.05, 0.3]], flags=GENERIC),
    "mh-8x8-carry": Case("mh", "m71-8x8-2x2", 8, 4, [[0.05, 0.3], [0.6, 1.0]], offset=CARRY),
    "mh-poisson-16x16": Case("mh", "basic-16x16-1x2", 16, 3, [[0.1, 0.6]], basic=True),
    "mh-8x8-by-count": Case("mh", "m71-8x8-1x2", 8, 4, [[0.2, 0.7]], by_count=True),
    "mala-32x32": Case("mala", "image32", 32, 10, [[0.05, 1.0]]),
    "mala-8x8-carry": Case("mala", "m71-8x8-2x2", 8, 4, [[0.05, 0.3], [0.6, 1.0]], offset=CARRY),
    "mala-8x8-by-count": Case("mala", "m71-8x8-1x2", 8, 4, [[0.2, 0.7]], by_count=True),
}


def _liveness(case, out, accept):
    """Some accept flag is 1 and some is 0 (MH: the replay twin's trace; the
    MALA sweep exposes no flags: some but not all selectable sources moved),
    some source moved, by-count padding did not."""
    S = case.S
    moved = (out["locs"] != case.locs).any(-1) | (out["fluxes"] != case.fluxes)
    pad = torch.arange(S, device=DEV)[None, None, None] >= case.counts[..., None]
    assert moved.any()
    if accept is not None:
        flags = accept[:, case.counts > 0]
        assert flags.any() and not flags.all()
    else:
        assert not moved[~pad].all()
    if case.by_count:
        assert pad.any() and (case.counts == 0).any()
        assert not moved[pad].any()
        assert _bits_equal(out["locs"][pad], case.locs[pad])
        assert _bits_equal(out["fluxes"][pad], case.fluxes[pad])


@pytest.mark.parametrize("name", list(SWEEPS))
def test_sweep_philox_equals_replay(image32, name):
    """locs, fluxes, last_counts, last_loglik, the acceptance rate and
    rate_out of one SingleComponentMH / SingleComponentMALA run."""
    case = SWEEPS[name].build(image32)
    state = (case.counts, case.locs, case.fluxes)
    phil, _ = case.run(state, case.offset)
    assert case.kernel.rng.offset == case.offset + K
    rep, accept = case.run(state, case.offset, replay=case.replay(case.offset))
    _assert_same(phil, rep)
    _liveness(case, phil, accept)


def test_mh_two_chained_runs_continue_the_stream(image32):
    """Two run() calls on one PhiloxStream (the second gathers ancestors and
    starts from the first's persisted rate images, as test_gpu_geometry's
    _two_sweeps): the second equals a replay generated at the offset the first
    call left in rng.offset, which lies past the first call's counters."""
    case = SWEEPS["mh-c2-geofixed"].build(image32)
    g = torch.Generator().manual_seed(2)
    anc = torch.randint(0, NP, case.shape, generator=g).to(DEV)

    def two(offsets=None):
        state, offs, outs, rate, acc = (case.counts, case.locs, case.fluxes), [], [], None, []
        case.kernel.rng.offset = 0
        for i in range(2):
            off = case.kernel.rng.offset  # what the previous call left
            offs.append(off)
            rp = None if offsets is None else case.replay(offsets[i])
            out, a = case.run(state, off, replay=rp, ancestors=anc if i else None, rate_in=rate)
            state, rate = (out["counts"], out["locs"], out["fluxes"]), out["rate"]
            outs.append(out)
            acc.append(a)
        return outs, offs, acc

    phil, offs, _ = two()
    assert offs[0] == 0 and offs[1] >= K, offs
    rep, _, acc = two(offsets=offs)
    for a, b in zip(phil, rep):
        _assert_same(a, b)
    # a second sweep that restarted the stream would repeat the first's draws
    assert not np.array_equal(case.replay(offs[0])["uacc"], case.replay(offs[1])["uacc"])
    for a in acc:
        assert a.any() and not a.all()
    assert not _bits_equal(phil[0]["locs"], case.locs)
    assert not _bits_equal(phil[1]["locs"], phil[0]["locs"])


@pytest.mark.parametrize("fused_step", [False, True], ids=["two-launch", "fused"])
def test_sampler_step_philox_equals_replay(image32, fused_step):
    """The path SMCsampler takes for the C2 geometry, smcdet_mh_sweep_step
    (two-launch form, the default, and the fused form), through
    SMCsampler._step, which takes a replay: three steps drawing from the
    sampler's PhiloxStream against three steps replaying the host arrays at
    the offsets the stream had before each step (the step's resampling draws
    from the same stream, after the sweep's counters, in both runs)."""
    from smcdet_amd.sampler import SMCsampler
    S = 10
    keys = ("temperature", "log_normalizing_constant", "ess", "weights", "locs", "fluxes",
            "counts", "loglik", "mutation_acc_rates")

    def steps(replaying):
        s = SMCsampler.from_tiles(image32, p_m71_prior(32, S, S), p_m71_model(32), p_m71_mh(K),
                                  NP, 0.5, "systematic", M71["flux_detection_threshold"], 100,
                                  print_every=10 ** 9, seed=SEED, device=DEV)
        s.fused_step = fused_step
        assert s._step_entry() and s.MutationKernel.rng is s.rng
        s.initialize()
        s._temper_reweight(with_resample=True)
        trace, offs, accs = [], [], []
        for _ in range(3):
            idx, s._pending_idx = s._pending_idx, None
            offs.append(s.rng.offset)
            rp = None
            if replaying:
                rp = _torch_replay(ST.sweep_replay("mh", SEED, offs[-1], K, 1, 2, NP, S))
                rp["trace_accept"] = torch.zeros(K, 1, 2, NP, device=DEV, dtype=torch.uint8)
                accs.append(rp["trace_accept"])
            s._step(idx, replay=rp)
            torch.cuda.synchronize()
            st = {k: getattr(s, k).clone() for k in keys}
            st["rate"] = s._rate[s._rate_cur].clone()
            trace.append(st)
        return trace, offs, accs

    phil, offs, _ = steps(False)
    rep, offs_r, accs = steps(True)
    assert offs == offs_r and all(b >= a + K for a, b in zip(offs, offs[1:])), offs
    for a, b in zip(phil, rep):
        _assert_same(a, b)
    for a in accs:
        assert a.any() and not a.all()
    assert not _bits_equal(phil[0]["locs"], phil[2]["locs"])


# ---- the chains ----------------------------------------------------------------------
C2 = dict(H=32, S=10, total=151, burnin=7, keep=4)  # keep does not divide total - burnin
CHUNKS = {"one-launch": 10 ** 9, "chunked": 37}      # chunk ends off the 64-draw grid


def _chain_run(tiles, prior, model, sl, sf, total, burnin, keep, print_every, offset,
               replay=None):
    """MHsampler over `tiles` with NP chains per tile, started from its own
    seeded prior draw: (accept, kept locs, kept fluxes, frozen) and the
    initial state."""
    from smcdet_amd.sampler import MHsampler
    s = MHsampler.from_tiles(tiles, prior, model, sl, sf, M71["flux_detection_threshold"], total,
                             burnin, keep, print_every=print_every, num_chains=NP, seed=SEED)
    init = (s.locs.clone(), s.fluxes.clone())
    s.rng.offset = offset
    with contextlib.redirect_stdout(io.StringIO()):
        s.run(replay=None if replay is None else _torch_replay(replay))
    torch.cuda.synchronize()
    assert s.rng.offset == offset + max(total - 1, 1)
    return dict(accept=s.accept, locs=s.locs, fluxes=s.fluxes, frozen=s.frozen), init


@pytest.fixture(scope="module")
def c2_chains(image32):
    """The four runs of the 1x2 tiles of 32x32, S = 10, C = 5 case: Philox and
    replay, in one launch and in chunks of 37 iterations."""
    H, S, total, burnin, keep = (C2[k] for k in ("H", "S", "total", "burnin", "keep"))
    rp = ST.chain_replay(SEED, 0, total - 1, 1, 2, NP, S)
    runs, inits = {}, []
    for mode, pe in CHUNKS.items():
        for kind in ("philox", "replay"):
            runs[kind, mode], init = _chain_run(
                image32, p_m71_prior(H, S, S), p_m71_model(H), 0.1, 2.5, total, burnin, keep, pe,
                0, replay=rp if kind == "replay" else None)
            inits.append(init)
    for init in inits[1:]:
        assert _bits_equal(init[0], inits[0][0]) and _bits_equal(init[1], inits[0][1])
    return dict(runs=runs, replay=rp, init=inits[0])


@pytest.mark.parametrize("mode", list(CHUNKS))
def test_chain_philox_equals_replay_c2(c2_chains, mode):
    """accept (int32) and the kept locs, fluxes and frozen flags, Philox
    against the replay run of the same print_every (a chunked run re-renders
    its rate image at every launch, on both sides)."""
    phil, rep = c2_chains["runs"]["philox", mode], c2_chains["runs"]["replay", mode]
    M = (C2["total"] - C2["burnin"] + C2["keep"] - 1) // C2["keep"]
    assert phil["accept"].dtype == torch.int32
    assert tuple(phil["accept"].shape) == (1, 2, NP, C2["total"] - 1)
    assert tuple(phil["locs"].shape) == (1, 2, NP * M, C2["S"], 2)
    _assert_same(phil, rep)
    acc = phil["accept"]
    assert acc.any() and not acc.all()
    assert acc.reshape(2 * NP, -1).any(-1).all()  # every chain accepted something
    kept = phil["locs"].reshape(1, 2, NP, M, C2["S"], 2)
    assert (kept[:, :, :, 0] != kept[:, :, :, -1]).any()
    assert not _bits_equal(kept[:, :, :, 0], c2_chains["init"][0])  # burn-in moved them


def test_chain_chunked_continues_the_stream_c2(c2_chains):
    """The two Philox runs against each other, by the criterion of
    test_gpu_mcmc.test_mh_chain_chunked_equals_single_launch: a chunked run
    that restarted its stream at each chunk would decide differently."""
    a = N(c2_chains["runs"]["philox", "one-launch"]["accept"])
    b = N(c2_chains["runs"]["philox", "chunked"]["accept"])
    assert (a == b).mean() > 0.97


def test_chain_replay_vs_oracle_c2(image32, c2_chains):
    """The replay arrays of the Philox stream through the C restatement, chain
    by chain (as test_mh_chain_poisson_many_chains_vs_oracle slices them), by
    the criteria of test_mh_chain_c2_vs_oracle: the accept flags equal on more
    than 0.99 of each chain's iterations, the kept locs within 1e-4 up to the
    chain's first differing decision.  Waves 1..3 of a workgroup, with 17x17
    windows whose positions past the first 64 and old-only positions go
    through the wave's LDS scratch, against an oracle."""
    H, S, total, burnin, keep = (C2[k] for k in ("H", "S", "total", "burnin", "keep"))
    Kc = total - 1
    M = (total - burnin + keep - 1) // keep
    rp = c2_chains["replay"]
    run = c2_chains["runs"]["replay", "one-launch"]
    init_l, init_f = (N(x) for x in c2_chains["init"])
    gl = N(run["locs"]).reshape(1, 2, NP, M, S, 2)
    ga = N(run["accept"])
    img = N(image32)
    for c in range(NP):
        sub = {k: np.ascontiguousarray(v[:, :, :, c]) for k, v in rp.items()}
        ol, of_, oacc = c_oracle.mh_chain(img, np.full((1, 2), S, np.float32), init_l[:, :, c],
                                          init_f[:, :, c], o_m71_prior(H, S, S), o_m71_model(H),
                                          o_m71_mh(1), total, burnin, keep, sub)
        for t in range(2):
            eq = ga[0, t, c] == oacc[0, t]
            print(f"chain {c} tile {t}: accept flags equal {eq.mean():.4f}, "
                  f"accepted {oacc[0, t].mean():.2f}")
            assert eq.mean() > 0.99, (c, t, eq.mean())
            m = M if eq.all() else max(0, (int(np.argmax(~eq)) - burnin) // keep)
            np.testing.assert_allclose(gl[0, t, c, :m], ol[0, t, :m], rtol=0, atol=1e-4)


@pytest.mark.parametrize("total", [41, 2, 1])
def test_chain_philox_equals_replay_small_runs(total):
    """2x2 tiles of 8x8, S = 3, C = 5, the Poisson / Pareto family, offset
    2^32 - 20, every sample kept.  total = 41: iterations 20..39 carry into
    the counter's high word; total = 2: one iteration, samples 0 and 1;
    total = 1: no iteration, sample 0 only, `accept` empty (the replay arrays
    then hold one unread row: the C ABI refuses null replay pointers)."""
    H, S = 8, 3
    tiles = torch.as_tensor(np.ascontiguousarray(
        tiles_of(golden("mh_basic_16x16.npz")["image"], H), dtype=np.float32), device=DEV)
    rp = ST.chain_replay(SEED, CARRY, max(total - 1, 1), 2, 2, NP, S)

    def run(replay):
        prior = p_basic_prior(H, S, S)
        prior.flux_lower, prior.flux_upper = BASIC_FLUX_SCALE * 0.9, 1e6
        return _chain_run(tiles, prior, p_basic_model(H), 0.1, 100, total, 0, 1, 10 ** 9, CARRY,
                          replay=replay)

    (phil, init), (rep, init_r) = run(None), run(rp)
    assert _bits_equal(init[0], init_r[0]) and _bits_equal(init[1], init_r[1])
    _assert_same(phil, rep)
    assert tuple(phil["accept"].shape) == (2, 2, NP, total - 1)
    kept = phil["locs"].reshape(2, 2, NP, total, S, 2)
    assert _bits_equal(kept[:, :, :, 0].contiguous(), init[0])  # sample 0: the initial state
    if total >= 2:
        acc = phil["accept"]
        assert acc[..., 0].any() and not acc[..., 0].all()
        moved = (kept[:, :, :, 1:] != kept[:, :, :, :-1]).any(-1).any(-1)  # [2,2,C,total-1]
        assert torch.equal(moved, acc.bool())
    if total == 41:  # draws on both sides of the carry were used
        assert acc[..., :20].any() and acc[..., 20:].any()
