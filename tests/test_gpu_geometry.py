"""The MH sweep with the 32x32 / psf_radius 8 tile geometry compiled in
(mh_sweep_kernel<..., GeoFixed<32, 32, 8>>, mh_kernel.hip) against the sweep
that reads H, W and R at run time (SMCDET_MH_GENERIC_GEOMETRY): only integer
addressing differs, so everything a sweep returns is bit-identical.

Shapes: T = 2 tiles, N = 10 particles (three workgroups per tile, the last
with two idle waves: the n >= N exit), K = 70 (past the 64-draw refill, all
four priority quarters), S = 10, and S = 3 with SMCDET_MH_COMPONENT_BY_COUNT
and counts 0..3.  The states are built so that every form of the union window
is evaluated (PLACES below; the slot counts are asserted on the host).

Floats are compared by their bits (stricter than torch.equal: -0.0 != 0.0,
and a NaN equals itself).
"""
import math

import pytest
import torch

from tests._params import M71, p_m71_mh

pytestmark = pytest.mark.gpu
DEV = "cuda"
GENERIC = 32768  # SMCDET_MH_GENERIC_GEOMETRY, include/smcdet_hip.h
H = W = 32
R = 8
T, N, K = 2, 10, 70
PAD = 4  # the location box is [-4, 36]

# (h, w) of the placed sources; the union window of a move that keeps its
# anchor (floor) is the (2R+1)^2 box at the anchor clipped to the tile
PLACES = [
    # interior: 17x17 boxes, 5 slots -> the 16x16 block form + row and column strip
    (15.5, 16.4), (12.3, 20.7), (20.6, 11.2),
    # within 8 px of an edge: clipped boxes of 4 slots (12x17, 17x12)
    (3.5, 16.5), (28.5, 16.5), (16.5, 3.5), (16.5, 28.5),
    # 3 slots (10x17), 2 slots (11x11 corners, 5x17), 1 slot (6x6 from the padding)
    (1.5, 16.5), (16.5, 30.5),
    (2.5, 2.5), (2.5, 29.5), (29.5, 2.5), (29.5, 29.5), (-3.5, 16.5),
    (-2.5, -2.5), (34.5, 34.5), (-2.5, 34.5),
    # 16-row / 16-column boxes: the block form without the row / column strip,
    # and 16x16 (4 slots: per pixel)
    (7.5, 16.5), (24.5, 16.5), (16.5, 7.5), (16.5, 24.5), (7.5, 7.5), (24.5, 24.5),
    # h or w within 0.02 of an integer: about half the proposals (sd 0.1) move
    # the anchor -> 18x17 / 17x18 (5 slots, two windows) and 18x18 (6 slots)
    (15.01, 16.5), (15.99, 16.5), (16.5, 15.01), (16.5, 20.99), (15.005, 15.995),
    (18.99, 12.01), (7.99, 16.5), (16.5, 24.01), (0.01, 0.01), (31.99, 16.5),
    # the padding: -4..0 and 32..36
    (-3.9, 16.5), (-0.5, 10.5), (33.5, 16.5), (35.9, 16.5), (16.5, -2.0), (16.5, 35.0),
    (-3.0, 35.0), (35.5, -3.5),
]


def _bits_equal(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _model(h=H, w=W, r=R):
    from smcdet_amd.images import M71ImageModel
    p = M71
    return M71ImageModel(image_height=h, image_width=w, background=p["background"],
                         psf_radius=r, adu_per_nmgy=p["adu_per_nmgy"],
                         psf_params=p["psf_params"], noise_additive=p["noise_additive"],
                         noise_multiplicative=p["noise_multiplicative"])


def _prior(smin, smax, h=H, w=W, rate=0.003125):
    from smcdet_amd.prior import M71Prior
    p = M71
    return M71Prior(min_objects=smin, max_objects=smax, counts_rate=rate, image_height=h,
                    image_width=w, flux_alpha=p["flux_alpha"], flux_lower=p["flux_lower"],
                    flux_upper=p["flux_upper"], pad=PAD)


def _slots(h, w):
    """64-position slots of the same-anchor union window of a source at (h, w)."""
    fh, fw = math.floor(h), math.floor(w)
    rows = min(fh + R, H - 1) - max(fh - R, 0) + 1
    cols = min(fw + R, W - 1) - max(fw - R, 0) + 1
    return rows, cols, -(-(rows * cols) // 64)


def test_places_cover_every_window_form():
    """(host arithmetic) 1..5-slot boxes, the block form with and without its
    strips, anchors next to an integer in h, in w and in both, both paddings."""
    geo = [_slots(h, w) for h, w in PLACES]
    assert {g[2] for g in geo} == {1, 2, 3, 4, 5}
    assert {(17, 17), (16, 17), (17, 16)} <= {g[:2] for g in geo if g[2] == 5}
    assert (16, 16, 4) in geo
    near = [(abs(h - round(h)) <= 0.02, abs(w - round(w)) <= 0.02) for h, w in PLACES]
    assert {(True, False), (False, True), (True, True)} <= set(near)
    assert any(h < 0 for h, _ in PLACES) and any(h > H for h, _ in PLACES)
    assert any(w < 0 for _, w in PLACES) and any(w > W for _, w in PLACES)


@pytest.fixture(scope="module")
def image():
    """Two 32x32 M71 tiles, [1, 2, 32, 32]."""
    torch.manual_seed(3)
    tiles = []
    for _ in range(T):
        _, l, f = _prior(0, 40, rate=0.004).sample(num_catalogs=1, device=DEV)
        tiles.append(_model().sample(l, f)[0, 0, :, :, 0])
    return torch.stack(tiles)[None].contiguous()


def _state(S, seed):
    """locs [1,T,N,S,2], fluxes [1,T,N,S]: PLACES dealt over the T*N*S sources
    (a stride coprime to S spreads them over particles and lanes), the rest
    uniform over the tile."""
    g = torch.Generator().manual_seed(seed)
    n = T * N * S
    locs = torch.rand(n, 2, generator=g) * H
    fluxes = 1.0 + 40.0 * torch.rand(n, generator=g)
    stride = 7
    assert math.gcd(stride, n) == 1 and len(PLACES) <= n
    for i, hw in enumerate(PLACES):
        locs[(i * stride) % n] = torch.tensor(hw)
    return (locs.reshape(1, T, N, S, 2).to(DEV).contiguous(),
            fluxes.reshape(1, T, N, S).to(DEV).contiguous())


def _counts(S, by_count):
    if not by_count:
        return torch.full((1, T, N), float(S), device=DEV)
    c = torch.tensor([0, 1, 2, 3, 1, 2, 3, 0, 2, 1], dtype=torch.float32)  # <= S = 3
    return torch.stack([c, c.flip(0)])[None].to(DEV).contiguous()


def _draws(seed, S, counts=None):
    g = torch.Generator().manual_seed(seed)
    top = torch.full((1, T, N), float(S)) if counts is None else counts.cpu().clamp(min=1.0)
    comp = torch.minimum((torch.rand(K, 1, T, N, generator=g) * top).floor(), top - 1)
    return dict(comp=comp.to(torch.int32).contiguous(),
                uloc=torch.rand(K, 1, T, N, 2, generator=g),
                uflux=torch.rand(K, 1, T, N, generator=g),
                uacc=torch.rand(K, 1, T, N, generator=g).clamp(min=1e-6))


def _two_sweeps(image, S, by_count, flags, draws=None, model=None, prior=None, state=None):
    """Two chained sweeps: the first renders its rate images and persists them,
    the second gathers ancestors and starts from the persisted images.
    Everything the sweeps return, as a dict of device tensors."""
    from smcdet_amd._rng import PhiloxStream
    model = model or _model()
    prior = prior or (_prior(0, S) if by_count else _prior(S, S))
    h, w = model.image_height, model.image_width
    counts = _counts(S, by_count)
    locs, fluxes = state if state is not None else _state(S, 11 + S)
    tau = torch.tensor([[0.05, 0.3]], device=DEV)
    mh = p_m71_mh(K)
    mh.debug_flags = flags
    mh.component_by_count = by_count
    mh.rng = PhiloxStream(17)
    g = torch.Generator().manual_seed(2)
    anc = torch.randint(0, N, (1, T, N), generator=g).to(DEV)
    out = {}
    rate = [torch.empty(1, T, N, h * w, device=DEV) for _ in range(2)]
    for i in range(2):
        rp = None
        if draws is not None:
            rp = dict(draws[i])
            rp["trace_loga"] = torch.zeros(K, 1, T, N, device=DEV)
            rp["trace_accept"] = torch.zeros(K, 1, T, N, device=DEV, dtype=torch.uint8)
        locs, fluxes, acc = mh.run(image, counts, locs, fluxes, tau, prior=prior,
                                   image_model=model, replay=rp,
                                   ancestors=anc if i else None,
                                   rate_in=rate[0] if i else None, rate_out=rate[i])
        counts = mh.last_counts
        out.update({f"locs{i}": locs, f"fluxes{i}": fluxes, f"counts{i}": counts,
                    f"loglik{i}": mh.last_loglik, f"rate{i}": rate[i], f"acc{i}": acc})
        if rp is not None:
            out.update({f"loga{i}": rp["trace_loga"], f"accept{i}": rp["trace_accept"]})
    torch.cuda.synchronize()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert _bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("S,by_count", [(10, False), (3, True)], ids=["S10", "S3-by-count"])
def test_sweep_is_bit_identical_to_generic_geometry(image, S, by_count):
    """Philox draws (the product's instantiation): locs, fluxes, counts,
    log-likelihoods, persisted rate images and acceptance rates of two chained
    sweeps."""
    spec = _two_sweeps(image, S, by_count, 0)
    gen = _two_sweeps(image, S, by_count, GENERIC)
    _assert_same(spec, gen)
    # the sweeps did move: sources placed next to an integer crossed it (moved
    # anchors were accepted, not only evaluated), and by-count padding stayed put
    locs0 = _state(S, 11 + S)[0]
    assert (spec["locs0"].floor() != locs0.floor()).any()
    if by_count:
        c = _counts(S, True)
        pad = torch.arange(S, device=DEV)[None, None, None] >= c[..., None]
        assert torch.equal(spec["locs0"][pad], locs0[pad])


def _edge_draws(state, S):
    """Replayed draws of two sweeps; in the first, particle 4 of tile 1 proposes
    source 2 -- placed 0.01 below the box's upper edge in h -- at iteration 37
    with a uniform that lands the proposal exactly on the edge
    (distributions.py:44-48), and never before."""
    t, n, j, k = 1, 4, 2, 37
    locs, fluxes = state
    locs = locs.clone()
    locs[0, t, n, j, 0] = H + PAD - 0.01
    d = [_draws(5, S), _draws(6, S)]
    comp = d[0]["comp"]
    early = comp[:k, 0, t, n]
    early[early == j] = (j + 1) % S
    comp[k, 0, t, n] = j
    d[0]["uloc"][k, 0, t, n, 0] = 0.9999999
    return (locs, fluxes), d, (t, n, k)


def test_replay_twin_decision_trace_is_bit_identical(image):
    """Recorded draws (the REPLAY = 1 twin, which the oracle-parity and
    teacher-forced tests run through): every output and the decision trace
    (log alpha, accept) with and without the flag; one proposal onto the upper
    box edge freezes its particle in both."""
    S = 10
    state, draws, (t, n, k) = _edge_draws(_state(S, 11 + S), S)
    spec = _two_sweeps(image, S, False, 0, draws=draws, state=state)
    gen = _two_sweeps(image, S, False, GENERIC, draws=draws, state=state)
    _assert_same(spec, gen)
    loga, acc = spec["loga0"][:, 0, t, n], spec["accept0"][:, 0, t, n]
    assert float(loga[k]) == -math.inf
    assert not acc[k:].any()
    assert spec["accept0"].float().mean() > 0.02 and spec["accept1"].float().mean() > 0.02


def _sampler_steps(image, flags, n_steps=3):
    from smcdet_amd.sampler import SMCsampler
    S = 10
    mh = p_m71_mh(K)
    mh.debug_flags = flags
    s = SMCsampler.from_tiles(image, _prior(S, S), _model(), mh, N, 0.5, "systematic",
                              M71["flux_detection_threshold"], 100, print_every=10 ** 9, seed=7,
                              device=DEV)
    s.initialize()
    s.locs, s.fluxes = _state(S, 11 + S)
    s.loglik = s._fresh_loglik = s.ImageModel.loglikelihood(s.tiled_image, s.locs, s.fluxes)
    s._temper_reweight(with_resample=True)
    trace = []
    for _ in range(n_steps):
        idx, s._pending_idx = s._pending_idx, None
        s._step(idx)
        torch.cuda.synchronize()
        assert s._rate_valid
        st = {k: getattr(s, k).clone() for k in
              ("temperature", "log_normalizing_constant", "ess", "weights", "locs", "fluxes",
               "counts", "loglik", "mutation_acc_rates")}
        st["rate"] = s._rate[s._rate_cur].clone()
        trace.append(st)
    return trace


def test_three_sampler_steps_are_bit_identical(image):
    """Three consecutive SMCsampler._step calls from the placed state: the
    resampling bins handed from one step's tile pass to the next sweep and the
    persisted rate images (rendered by the first sweep, read by the next two)."""
    spec, gen = _sampler_steps(image, 0), _sampler_steps(image, GENERIC)
    for a, b in zip(spec, gen):
        _assert_same(a, b)
    assert (spec[0]["temperature"] > 0).all()
    assert not _bits_equal(spec[0]["locs"], spec[2]["locs"])


@pytest.mark.parametrize("h,w,r", [(24, 40, 8), (32, 32, 6)], ids=["24x40", "32x32-R6"])
def test_other_shapes_ignore_the_flag(h, w, r):
    """Every other shape has one kernel, with or without the flag."""
    S = 10
    model, prior = _model(h, w, r), _prior(S, S, h, w)
    torch.manual_seed(4)
    tiles = []
    for _ in range(T):
        _, l, f = _prior(0, 40, h, w, rate=0.004).sample(num_catalogs=1, device=DEV)
        tiles.append(model.sample(l, f)[0, 0, :, :, 0])
    img = torch.stack(tiles)[None].contiguous()
    g = torch.Generator().manual_seed(9)
    locs = torch.rand(1, T, N, S, 2, generator=g) * torch.tensor([h + 2.0 * PAD, w + 2.0 * PAD]) \
        - PAD
    state = (locs.to(DEV).contiguous(),
             (1.0 + 40.0 * torch.rand(1, T, N, S, generator=g)).to(DEV).contiguous())
    a = _two_sweeps(img, S, False, 0, model=model, prior=prior, state=state)
    b = _two_sweeps(img, S, False, GENERIC, model=model, prior=prior, state=state)
    _assert_same(a, b)
    assert not _bits_equal(a["locs1"], state[0])
