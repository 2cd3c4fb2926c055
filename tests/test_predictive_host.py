"""smcdet_amd.predictive without a GPU: the float64 oracle
(tests/_predictive_oracle.py) on cases worked by hand, the derived fields and
p-values of PosteriorImage from planted arrays, to_image against the tiling
the tests use, the wrappers' refusal of CPU tensors, and the argument
validation of the two entry points (no kernel is launched: every call fails
before any device work)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import smc_oracle as SO
from smcdet_amd import _hip, predictive
from tests import _predictive_oracle as O
from tests._params import M71, tiles_of

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "smcdet_hip.h")
EINVAL, EUNSUPPORTED = -1, -2


# ---- the oracle, by hand ---------------------------------------------------------
def test_oracle_two_catalogs_by_hand():
    """One pixel, rates 1 and 3, weights 1 and 3 (unnormalised): w~ = 1/4, 3/4,
    mean 2.5, var = 0.25 * 1.5^2 + 0.75 * 0.5^2 = 0.75, rms^2 = 0.25 + 6.75."""
    rate = np.array([1.0, 3.0]).reshape(1, 1, 1, 1, 2)
    w = np.array([1.0, 3.0]).reshape(1, 1, 2)
    mean, var, rms = O.moments(rate, w)
    assert mean.item() == 2.5 and var.item() == 0.75 and rms.item() == math.sqrt(7.0)
    mean, var, _ = O.moments(rate)
    assert mean.item() == 2.0 and var.item() == 1.0
    # Poisson discrepancy at x = 2: (2-1)^2 / 1 and (2-3)^2 / 3
    basic = SO.BasicModel(1, 1, 1.0, 0, 1.0)
    x = np.full((1, 1, 1, 1), 2.0)
    np.testing.assert_allclose(O.chi2(basic, x, rate)[0, 0], [1.0, 1.0 / 3.0], rtol=1e-15)
    # |2 (x - l) / v| l + (x - l)^2 / v^2 l: 2 + 1 and 2 + 1/3
    np.testing.assert_allclose(O.chi2_sensitivity(basic, x, rate)[0, 0], [3.0, 2.0 + 1.0 / 3.0],
                               rtol=1e-15)
    # M71 noise: v = a + b l
    m71 = SO.M71Model(1, 1, 1.0, 1, 1.0, M71["psf_params"], 0.5, 2.0)
    np.testing.assert_allclose(O.chi2(m71, x, rate)[0, 0], [1.0 / 2.5, 1.0 / 6.5], rtol=1e-15)
    assert O.noise_var(m71, 3.0) == 6.5 and O.eta(m71) == 2.0 and O.eta(basic) == 1.0


def test_oracle_renders_through_smc_oracle():
    """A 1x1 tile, radius 0, sources at the pixel centre: rate = B + f / (s sqrt(2 pi))."""
    basic = SO.BasicModel(1, 1, 10.0, 0, 2.0)
    locs = np.full((1, 1, 2, 1, 2), 0.5, np.float32)
    fluxes = np.array([5.0, 15.0], np.float32).reshape(1, 1, 2, 1)
    peak = 1.0 / (2.0 * math.sqrt(2 * math.pi))
    out = O.posterior_image(basic, locs, fluxes, image=np.full((1, 1, 1, 1), 12.0))
    np.testing.assert_allclose(out["rate"][0, 0, 0, 0], [10 + 5 * peak, 10 + 15 * peak], rtol=1e-12)
    np.testing.assert_allclose(out["mean"].item(), 10 + 10 * peak, rtol=1e-12)
    np.testing.assert_allclose(out["rate_var"].item(), (5 * peak) ** 2, rtol=1e-12)
    np.testing.assert_allclose(out["pred_var"].item(), (5 * peak) ** 2 + 10 + 10 * peak, rtol=1e-12)
    np.testing.assert_allclose(out["residual"].item(), 2 - 10 * peak, rtol=1e-12)
    assert out["flux_obs"].item() == 12.0


def test_oracle_p_value_ties_and_weights():
    rep = np.array([[1.0, 2.0, 3.0, 4.0]])
    obs = np.array([[2.0, 2.0, 2.0, 5.0]])       # below, tie, above, below
    assert O.p_value(rep, obs)[0] == 0.5
    assert O.p_value(rep, obs, np.array([[4.0, 2.0, 2.0, 8.0]]))[0] == 0.25


# ---- PosteriorImage, plain torch -------------------------------------------------
class _M71Like:
    image_height = image_width = 2
    noise_additive, noise_multiplicative = 0.5, 2.0


class _PoissonLike:
    image_height = image_width = 2


def _planted(model, weights):
    mean = torch.tensor([[[1.0, 2.0], [3.0, 4.0]]])
    var = torch.tensor([[[0.5, 0.0], [1.0, 2.0]]])
    x = torch.tensor([[[2.0, 2.0], [1.0, 7.0]]])             # flux_obs = 12
    chi2 = torch.tensor([[1.0, 2.0, 3.0, 4.0]])
    chi2_rep = torch.tensor([[0.5, 2.0, 4.0, 1.0]])          # below, tie, above, below
    flux_rep = torch.tensor([[12.0, 11.0, 13.0, 12.5]])      # tie, below, above, above
    return predictive.PosteriorImage(mean=mean, rate_var=var, image_model=model, chi2=chi2,
                                     chi2_rep=chi2_rep, flux_rep=flux_rep, tiled_image=x,
                                     weights=weights)


@pytest.mark.parametrize("model,noise", [(_M71Like, lambda m: 0.5 + 2.0 * m),
                                         (_PoissonLike, lambda m: m)], ids=["m71", "poisson"])
def test_derived_fields_from_planted_arrays(model, noise):
    pi = _planted(model(), None)
    m = pi.mean.double()
    assert torch.equal(pi.noise_var, noise(m))
    assert torch.equal(pi.pred_var, pi.rate_var.double() + noise(m))
    assert torch.equal(pi.residual, pi.tiled_image.double() - m)
    assert torch.equal(pi.z, pi.residual / pi.pred_var.sqrt())
    assert pi.flux_obs.tolist() == [12.0]
    assert pi.p_value.tolist() == [0.5]          # the tie counts
    assert pi.p_value_flux.tolist() == [0.75]


def test_p_values_with_unnormalised_weights():
    w = torch.tensor([[4.0, 2.0, 2.0, 8.0]])
    pi = _planted(_M71Like(), w)
    assert pi.p_value.tolist() == [0.25]         # (2 + 2) / 16
    assert pi.p_value_flux.tolist() == [0.875]   # (4 + 2 + 8) / 16
    got = pi.p_value.numpy()
    np.testing.assert_array_equal(got, O.p_value(pi.chi2_rep.numpy(), pi.chi2.numpy(), w.numpy()))
    zero = _planted(_M71Like(), torch.tensor([[0.0, 0.0, 1.0, 0.0]]))
    assert zero.p_value.tolist() == [1.0] and zero.p_value_flux.tolist() == [1.0]


def test_fields_that_need_the_image_say_so():
    pi = predictive.PosteriorImage(mean=torch.ones(1, 2, 2), rate_var=torch.zeros(1, 2, 2),
                                   image_model=_PoissonLike())
    assert torch.equal(pi.pred_var, torch.ones(1, 2, 2, dtype=torch.float64))
    for name in ("residual", "z", "flux_obs", "p_value", "p_value_flux"):
        with pytest.raises(ValueError, match="tiled_image"):
            getattr(pi, name)


def test_to_image_inverts_tiles_of():
    img = np.arange(12 * 12, dtype=np.float32).reshape(12, 12)
    tiles = torch.from_numpy(np.ascontiguousarray(tiles_of(img, 4)))      # [3,3,4,4]
    pi = predictive.PosteriorImage(mean=tiles, rate_var=torch.zeros_like(tiles),
                                   image_model=_PoissonLike())
    assert torch.equal(pi.to_image("mean"), torch.from_numpy(img))
    assert torch.equal(pi.to_image(tiles * 2), torch.from_numpy(img) * 2)
    # the samplers' own tiling
    t = torch.from_numpy(img)
    unfolded = t.unfold(0, 4, 4).unfold(1, 4, 4).contiguous()
    assert torch.equal(pi.to_image(unfolded), t)
    with pytest.raises(ValueError, match="numH"):
        pi.to_image(torch.zeros(3, 4, 4))


def test_catalog_chunks_rule():
    assert predictive.catalog_chunks(64, 1) == 1 and predictive.catalog_chunks(64, 32) == 1
    assert predictive.catalog_chunks(64, 33) == 2
    assert predictive.catalog_chunks(64, 70) == 3            # 24 + 24 + 22
    assert predictive.catalog_chunks(64, 10000) == 63        # chunks of 160
    assert predictive.catalog_chunks(64 * 65, 5) == 2
    assert predictive.catalog_chunks(65536, 400) == 15


# ---- wrappers --------------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors():
    from tests._params import p_m71_model
    pm = p_m71_model(8)
    locs, fluxes = torch.zeros(1, 4, 2, 2), torch.ones(1, 4, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        predictive.posterior_image(pm, locs, fluxes)
    with pytest.raises(RuntimeError, match="HIP device"):
        predictive.posterior_image(pm, locs[None], fluxes[None],
                                   tiled_image=torch.zeros(1, 1, 8, 8))

    class NotRun:
        has_run = False
    with pytest.raises(ValueError, match="run"):
        predictive.predictive_sampler(NotRun())


def test_module_is_a_drop_in_name():
    import smcdet_amd
    assert "predictive" in smcdet_amd._DROP_IN


# ---- the C ABI: every argument validated before any device work -------------------
def _model(kind=1, H=8, W=8):
    m = _hip.ImageModelC()
    m.model, m.H, m.W, m.psf_radius = kind, H, W, 8
    m.background, m.adu_per_nmgy, m.psf_norm = 100.0, 1.0, 1.0
    m.psf_params[:] = [1.0, 2.0, 2.0, 5.0, 0.5, 0.5]
    m.noise_additive, m.noise_multiplicative = 1e-10, 1.9
    return m


P = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(10)]
BIG = 1 << 40


def _call(model=None, kind=1, H=8, W=8, T=1, N=4, S=3, img=P[0], locs=P[1], fluxes=P[2],
          weights=None, mean=P[3], var=P[4], chi2=P[5], chi2_rep=P[6], flux_rep=P[7], ws=P[8],
          ws_bytes=0):
    """smcdet_posterior_image with placeholder device pointers (never
    dereferenced) and, unless told otherwise, a workspace of 0 bytes: a call
    that passes every other check stops at the workspace size."""
    m = _model(kind, H, W) if model is None else model
    return _hip.lib().smcdet_posterior_image(ctypes.byref(m), img, locs, fluxes, weights, T, N, S,
                                             1, 0, mean, var, chi2, chi2_rep, flux_rep, ws,
                                             ws_bytes, None)


def _err():
    return _hip.lib().smcdet_last_error().decode()


def _ws(kind=1, H=8, W=8, T=1, N=4):
    return _hip.lib().smcdet_posterior_image_workspace(ctypes.byref(_model(kind, H, W)), T, N)


def test_abi_names_bound_and_abi_version_unchanged():
    hdr = open(HEADER).read()
    for name in ("smcdet_posterior_image", "smcdet_posterior_image_workspace"):
        assert name in _hip.EXPORTS and name in _hip._OUTS and name in hdr
    assert "#define SMCDET_ABI_VERSION 20" in hdr and _hip.ABI_VERSION == 20
    assert "added under SMCDET_ABI_VERSION 20" in hdr
    assert "bit-identical" in hdr


def test_abi_null_buffers_are_einval():
    L = _hip.lib()
    assert L.smcdet_posterior_image(None, None, None, None, None, 1, 1, 1, 0, 0, None, None, None,
                                    None, None, None, 0, None) == EINVAL
    assert "null" in _err()
    for kw in (dict(mean=None), dict(var=None), dict(ws=None), dict(locs=None),
               dict(fluxes=None)):
        assert _call(**kw) == EINVAL, kw
        assert "null" in _err(), kw
    assert L.smcdet_posterior_image_workspace(None, 1, 1) == EINVAL


def test_abi_chi2_needs_the_image():
    assert _call(img=None) == EINVAL and "tiled_image" in _err()
    # without chi2 the image is optional: the call goes on to the workspace check
    assert _call(img=None, chi2=None) == EINVAL and "workspace" in _err()


def test_abi_optional_buffers_and_s0_pass_validation():
    """Nullable outputs, null weights and S = 0 with null catalogs are legal:
    such a call fails only at the (deliberately short) workspace."""
    for kw in (dict(chi2=None, chi2_rep=None, flux_rep=None), dict(weights=P[9]),
               dict(S=0, locs=None, fluxes=None), dict(chi2_rep=None)):
        assert _call(**kw) == EINVAL, kw
        assert "workspace" in _err(), kw


@pytest.mark.parametrize("kw", [dict(T=0), dict(N=0), dict(S=-1), dict(T=-3)])
def test_abi_empty_shapes_are_refused(kw):
    assert _call(ws_bytes=BIG, **kw) in (EINVAL, EUNSUPPORTED)
    assert _err()


def test_abi_limits_are_eunsupported():
    assert _call(T=65536, ws_bytes=BIG) == EUNSUPPORTED and "65535" in _err()
    assert _call(kind=2, H=64, W=65, ws_bytes=BIG) == EUNSUPPORTED and "M71" in _err()
    assert _call(H=64, W=65, S=65, ws_bytes=BIG) == EUNSUPPORTED and "S=65" in _err()
    assert _call(H=300, W=300, ws_bytes=BIG) == EUNSUPPORTED
    # the same shapes through the workspace function
    assert _ws(T=65536) == EUNSUPPORTED
    assert _ws(kind=2, H=64, W=65) == EUNSUPPORTED
    assert _ws(T=0) in (EINVAL, EUNSUPPORTED) and _ws(N=0) in (EINVAL, EUNSUPPORTED)
    # S = 65 is fine up to 4096 pixels, T = 65535 too (stops at the workspace)
    assert _call(H=64, W=64, S=65) == EINVAL and "workspace" in _err()
    assert _call(T=65535) == EINVAL and "workspace" in _err()


@pytest.mark.parametrize("kind,H,W,T,N", [(1, 8, 8, 1, 4), (2, 16, 16, 3, 257),
                                          (1, 32, 32, 64, 4096), (1, 64, 65, 2, 9)])
def test_abi_short_workspace_names_the_size(kind, H, W, T, N):
    need = _ws(kind, H, W, T, N)
    assert need > 0
    assert _call(kind=kind, H=H, W=W, T=T, N=N, ws_bytes=need - 1) == EINVAL
    msg = _err()
    assert "workspace" in msg and str(need) in msg and str(need - 1) in msg


def test_workspace_is_monotone_and_as_documented():
    for kind, H, W in ((1, 8, 8), (2, 16, 16), (1, 25, 41), (1, 64, 65)):
        prev = 0
        for N in list(range(1, 300)) + [1000, 2047, 2048, 2049, 4096, 10000, 16384]:
            need = _ws(kind, H, W, 3, N)
            assert need >= prev, (H, W, N)
            prev = need
            if H * W <= 4096:
                C = min(-(-N // 32), 64)
            else:
                C = 4 * min(-(-N // 4), 64, max(1, (1 << 20) // (H * W)))
            assert need == 8 * 3 + 16 * 3 * C * H * W, (H, W, N)
            assert predictive.catalog_chunks(H * W, N) <= C
        prev = 0
        for T in (1, 2, 3, 7, 100, 1000, 65535):
            need = _ws(kind, H, W, T, 257)
            assert need > prev, (H, W, T)
            prev = need
