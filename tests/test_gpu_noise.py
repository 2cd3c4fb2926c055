"""What smcdet_sample_image computes (model_kernels.hip: sample_image_kernel,
std_normal, poisson_draw), called through the C ABI on constant-rate buffers
of 2^20 elements.

Deterministic properties are bit-exact: the Philox counter of element i is
offset + i, keyed by the seed alone.  The law is judged by tests/_noise_stats.py
(every |z| <= 4.5, every Kolmogorov-Smirnov / chi^2 p >= 1e-5; shown sound on
numpy's draws by test_noise_stats_host.py) at one seed fixed before the first
run.  Poisson rates run up to 1e6, the ceiling smcdet_hip.h states: with the
transformed-rejection acceptance test in float32 the draws at 3e5 and 1e6 were
over-dispersed (variance / rate 1.01 and 1.05).
"""
import numpy as np
import pytest
import torch

from smcdet_amd import _hip
from tests import _noise_stats as NS
from tests._params import M71, p_basic_model, p_m71_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_DRAWS = 1 << 20
SEED, SEED_B = 20261019, 20261020          # fixed before the first run
M71_RATES = [M71["background"], 1e3, 1e5]
POISSON_RATES = [0.05, 1.0, 9.99, 10.0, 10.01, 30.0, 1e3, 5e4, 3e5, 1e6]


def draw(model, rate, seed, offset=0, count=None, out=None):
    """smcdet_sample_image on `rate` (a float32 device tensor); returns out."""
    if out is None:
        out = torch.empty_like(rate)
    count = rate.numel() if count is None else count
    rc = _hip.lib().smcdet_sample_image(_hip.ref(model._cmodel()), _hip.ptr(rate), count, seed,
                                        offset, _hip.ptr(out), _hip.stream_of(rate))
    assert rc == 0, _hip.lib().smcdet_last_error().decode()
    return out


def const(v, n=N_DRAWS):
    return torch.full((n,), float(v), device=DEV, dtype=torch.float32)


def mixed_m71(n=N_DRAWS):
    r = torch.tensor(M71_RATES, dtype=torch.float32)
    return r[torch.arange(n) % 3].to(DEV)


def models():
    return [("m71", p_m71_model(8), mixed_m71()),
            ("poisson", p_basic_model(8), torch.tensor([0.5, 7.0, 12.0, 300.0, 2e5],
                                                       dtype=torch.float32).repeat(N_DRAWS // 5 + 1)
             [:N_DRAWS].to(DEV))]


@pytest.mark.parametrize("which", [0, 1], ids=["m71", "poisson"])
def test_seed_offset_count_and_in_place(which):
    _, model, rate = models()[which]
    a = draw(model, rate, SEED)
    assert torch.equal(a, draw(model, rate, SEED))            # same seed, same draw
    b = draw(model, rate, SEED_B)
    assert float((a != b).float().mean()) > 0.5               # another seed, another draw
    inplace = rate.clone()
    assert torch.equal(draw(model, inplace, SEED, out=inplace), a)
    # offset k: the counters of elements k.. of the offset-0 draw
    for k in (1, 255, 4096 + 37):
        tail = draw(model, rate[k:].contiguous(), SEED, offset=k)
        assert torch.equal(tail, a[k:]), k
    big = (1 << 32) - 5                                       # the counter's high word
    c = draw(model, rate[:64].contiguous(), SEED, offset=big)
    d = draw(model, rate[15:64].contiguous(), SEED, offset=big + 15)   # (the rates cycle by 3 or 5)
    assert torch.equal(c[15:], d)
    # count short of the buffer: the tail keeps its sentinel
    cnt = 4096 + 37
    out = torch.full_like(rate, -12345.0)
    draw(model, rate, SEED, count=cnt, out=out)
    assert torch.equal(out[:cnt], a[:cnt]) and bool((out[cnt:] == -12345.0).all())
    # count 0 is accepted and writes nothing
    out = torch.full_like(rate, -12345.0)
    draw(model, rate, SEED, count=0, out=out)
    assert bool((out == -12345.0).all())


def test_manual_seed_makes_sample_repeatable():
    for model in (p_m71_model(8), p_basic_model(8)):
        locs = torch.tensor([[3.3, 4.1], [6.0, 1.5]], device=DEV).expand(1, 1, 5, 2, 2).contiguous()
        fluxes = torch.tensor([40.0, 900.0], device=DEV).expand(1, 1, 5, 2).contiguous()
        torch.manual_seed(11)
        a = model.sample(locs, fluxes)
        torch.manual_seed(11)
        b = model.sample(locs, fluxes)
        torch.manual_seed(12)
        c = model.sample(locs, fluxes)
        assert a.shape == (1, 1, 8, 8, 5)
        assert torch.equal(a, b) and not torch.equal(a, c)
        # the five catalogs are the same: their noise is not
        assert not torch.equal(a[..., 0], a[..., 1])


def test_poisson_degenerate_rates_and_integers():
    model = p_basic_model(8)
    rate = torch.tensor([0.0, -1.0, float("nan"), -0.0, -float("inf")],
                        device=DEV).repeat(1000)
    assert bool((draw(model, rate, SEED) == 0).all())
    for lam in (0.05, 9.99, 10.0, 1e3, 1e6):
        k = draw(model, const(lam, 1 << 16), SEED)
        assert bool((k >= 0).all()) and bool((k == torch.floor(k)).all()), lam


def _m71_residual(model, rate, x):
    r = rate.double().cpu().numpy()
    sd = np.sqrt(float(np.float32(model.noise_additive))
                 + float(np.float32(model.noise_multiplicative)) * r)
    return (x.double().cpu().numpy() - r) / sd


@pytest.mark.parametrize("rate", M71_RATES + ["mixed"], ids=["background", "1e3", "1e5", "mixed"])
def test_m71_noise_law(rate):
    model = p_m71_model(8)
    r = mixed_m71() if rate == "mixed" else const(rate)
    za = _m71_residual(model, r, draw(model, r, SEED))
    zb = _m71_residual(model, r, draw(model, r, SEED_B))
    rep = NS.normal_report(za, zb)
    NS.show(f"m71 rate {rate}", rep)
    assert NS.failures(rep) == []


@pytest.mark.parametrize("lam", POISSON_RATES)
def test_poisson_noise_law(lam):
    """With the acceptance test in float32 (same seed, same n) the variance's z
    was 35.3 at 3e5 and 94.5 at 1e6, and within 1.5 up to 5e4."""
    model = p_basic_model(8)
    k = draw(model, const(lam), SEED).cpu().numpy()
    rep = NS.poisson_report(k, float(np.float32(lam)))
    NS.show(f"poisson rate {lam:g}", rep)
    assert NS.failures(rep) == []
