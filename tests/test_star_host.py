"""StarPrior (Normal fluxes) without a GPU: the class and its C description,
the header, host validation and the refusals of the C ABI (every call here
stops in a host check: null buffers and T = 0, never a made-up device
pointer), and the fixtures themselves -- the test-side float64 Normal log
prior against the reference's recorded values, and the float64 oracle's MH
sweep against every recorded decision of the MH fixtures with
|log u - log alpha| >= 1e-4."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from smcdet_amd import _hip
from tests._params import golden
from tests._star import (STAR, STAR_MH_FIXTURES, decision_margin, normal_log_prior, o_star_prior,
                         oracle_mh_trace, p_star_prior)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2


def test_class_signature_and_attributes():
    from smcdet_amd.prior import PointProcessPrior, StarPrior
    assert issubclass(StarPrior, PointProcessPrior)
    sig = inspect.signature(StarPrior.__init__)
    kinds = {n: p.kind for n, p in sig.parameters.items()}
    assert kinds["args"] is inspect.Parameter.VAR_POSITIONAL
    assert kinds["flux_mean"] is inspect.Parameter.KEYWORD_ONLY
    assert kinds["flux_stdev"] is inspect.Parameter.KEYWORD_ONLY
    assert kinds["kwargs"] is inspect.Parameter.VAR_KEYWORD
    pr = StarPrior(1, 3, 16, 16, flux_mean=1300, flux_stdev=250, pad=2)
    assert (pr.min_objects, pr.max_objects, pr.image_height, pr.pad) == (1, 3, 16, 2)
    assert pr.flux_mean == 1300 and pr.flux_stdev == 250
    assert isinstance(pr.flux_prior, torch.distributions.Normal)
    assert float(pr.flux_prior.loc) == 1300.0 and float(pr.flux_prior.scale) == 250.0
    assert pr.num_counts == 3 and pr.tile_boxes((2, 2)) is None
    lcp = pr.log_count_prior_per_tile(torch.tensor([[-2.0, -2.0, 18.0, 18.0]]))
    np.testing.assert_allclose(lcp.numpy(), np.full((1, 3), -np.log(3.0)))


def test_alias_import_resolves():
    import sys
    import smcdet_amd
    saved = {k: v for k, v in sys.modules.items() if k == "smcdet" or k.startswith("smcdet.")}
    try:
        smcdet_amd.install_as_smcdet()
        from smcdet.prior import StarPrior
        from smcdet_amd.prior import StarPrior as P
        assert StarPrior is P
    finally:
        for k in [k for k in sys.modules if k == "smcdet" or k.startswith("smcdet.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_cprior_fields_and_cache_follow_rebinding():
    pr = p_star_prior(16, 1, 3)
    c = pr._cprior()
    assert c.kind == _hip.SMCDET_PRIOR_NORMAL == 3
    assert (c.min_objects, c.max_objects) == (1, 3)
    assert (c.loc_low, c.loc_high_h, c.loc_high_w) == (-2.0, 18.0, 18.0)
    assert (c.flux_lower, c.flux_upper, c.flux_alpha) == (1300.0, 250.0, 0.0)
    assert pr._cprior() is c  # cached while no attribute is rebound
    pr.flux_stdev = 125.0
    c2 = pr._cprior()
    assert c2 is not c and c2.flux_upper == 125.0 and c2.flux_lower == 1300.0
    pr.flux_mean = 900.0
    assert pr._cprior().flux_lower == 900.0


def test_header_define_and_abi():
    with open(os.path.join(ROOT, "include", "smcdet_hip.h")) as f:
        h = f.read()
    assert re.search(r"^#define SMCDET_PRIOR_NORMAL 3\b", h, re.M)
    assert re.search(r"^#define SMCDET_ABI_VERSION 20\b", h, re.M)
    assert _hip.ABI_VERSION == 20 and _hip.lib().smcdet_abi_version() == 20
    assert "NORMAL: flux_mean" in h and "NORMAL: flux_stdev" in h


def _prior(kind=3, mean=1300.0, sd=250.0):
    p = _hip.PriorC()
    p.kind, p.min_objects, p.max_objects = kind, 1, 3
    p.loc_low, p.loc_high_h, p.loc_high_w = -2.0, 18.0, 18.0
    p.flux_alpha, p.flux_lower, p.flux_upper = 0.0, mean, sd
    return p


def _log_prior_rc(p):
    """smcdet_log_prior with null buffers: validate_prior runs first, the null
    check right after it -- nothing is launched."""
    L = _hip.lib()
    rc = L.smcdet_log_prior(ctypes.byref(p), None, None, None, 1, 1, 3, None, None, None)
    return rc, L.smcdet_last_error()


@pytest.mark.parametrize("sd", [0.0, -1.0, float("inf"), float("nan")])
def test_validate_prior_rejects_bad_stdev(sd):
    rc, err = _log_prior_rc(_prior(sd=sd))
    assert rc == EINVAL and b"stdev" in err, (rc, err)


@pytest.mark.parametrize("mean", [float("inf"), float("-inf"), float("nan")])
def test_validate_prior_rejects_nonfinite_mean(mean):
    rc, err = _log_prior_rc(_prior(mean=mean))
    assert rc == EINVAL and b"mean" in err, (rc, err)


def test_validate_prior_kinds():
    rc, err = _log_prior_rc(_prior(kind=4))
    assert rc == EINVAL and b"unknown prior kind 4" in err, (rc, err)
    # kind 3 itself passes validate_prior: the call stops at the null buffers
    rc, err = _log_prior_rc(_prior())
    assert rc == EINVAL and b"null buffer" in err, (rc, err)
    # a negative mean is a valid Normal
    rc, err = _log_prior_rc(_prior(mean=-5.0))
    assert rc == EINVAL and b"null buffer" in err, (rc, err)


def _model(kind, H=8):
    m = _hip.ImageModelC()
    m.model, m.H, m.W, m.psf_radius = kind, H, H, 8
    m.background, m.adu_per_nmgy, m.psf_norm = 300.0, 1.0, 1.0
    m.psf_params[:] = [1.0, 2.0, 2.0, 5.0, 0.5, 0.5]
    m.noise_additive, m.noise_multiplicative = 1e-10, 1.9
    return m


def _mh():
    mh = _hip.MHC()
    mh.num_iters, mh.locs_stdev, mh.fluxes_stdev = 1, 0.25, 100.0
    mh.fluxes_min, mh.fluxes_max = 50.0, 2550.0
    mh.locs_min_h = mh.locs_min_w = -2.0
    mh.locs_max_h = mh.locs_max_w = 18.0
    return mh


def _sweep_rc(name, model_kind):
    """smcdet_mh_sweep / smcdet_mala_sweep with every buffer null and T = 0."""
    L = _hip.lib()
    m, p, mh = _model(model_kind), _prior(), _mh()
    nargs = len(_hip._SIGS[name][0])
    args = [ctypes.byref(m), ctypes.byref(p), ctypes.byref(mh), None, None, 0, 4, 3]
    args += [None] * (nargs - len(args))
    args[17], args[18], args[20] = 1, 0, 0  # seed, offset, flags
    rc = getattr(L, name)(*args)
    return rc, L.smcdet_last_error()


@pytest.mark.parametrize("name", ["smcdet_mh_sweep", "smcdet_mh_sweep_step", "smcdet_mala_sweep"])
def test_sweeps_refuse_normal_prior_with_m71_model(name):
    if name == "smcdet_mh_sweep_step":
        # (needs a tail descriptor to get past its own null check)
        L = _hip.lib()
        m, p, mh, tail = _model(_hip.SMCDET_MODEL_M71), _prior(), _mh(), _hip.SmcTailC()
        args = [ctypes.byref(m), ctypes.byref(p), ctypes.byref(mh), None, None, 0, 4, 3]
        args += [None] * (len(_hip._SIGS[name][0]) - len(args))
        args[17], args[18], args[20], args[26] = 1, 0, 0, ctypes.byref(tail)
        rc, err = L.smcdet_mh_sweep_step(*args), L.smcdet_last_error()
    else:
        rc, err = _sweep_rc(name, _hip.SMCDET_MODEL_M71)
    assert rc == EUNSUPPORTED and b"Normal flux prior" in err and b"POISSON" in err, (rc, err)


@pytest.mark.parametrize("name", ["smcdet_mh_sweep", "smcdet_mala_sweep"])
def test_sweeps_take_normal_prior_with_poisson_model(name):
    # past the refusal: the call stops at the null buffers instead
    rc, err = _sweep_rc(name, _hip.SMCDET_MODEL_POISSON)
    assert rc == EINVAL and b"null buffer" in err, (rc, err)


def test_mh_chain_refuses_normal_prior():
    L = _hip.lib()
    m, p, mh = _model(_hip.SMCDET_MODEL_POISSON), _prior(), _mh()
    args = [ctypes.byref(m), ctypes.byref(p), ctypes.byref(mh), None, 0, 1, 3, None, None, None,
            10, 2, 1, 0, 10, 1, 0, None, None, None, None, None, None]
    rc = L.smcdet_mh_chain(*args)
    err = L.smcdet_last_error()
    assert rc == EUNSUPPORTED and b"smcdet_mh_chain" in err and b"Normal flux prior" in err, (rc,
                                                                                             err)


def test_aggregate_sweep_refuses_normal_prior():
    L = _hip.lib()
    m, p, mh = _model(_hip.SMCDET_MODEL_POISSON), _prior(), _mh()
    args = [ctypes.byref(m), ctypes.byref(p), ctypes.byref(mh), 0, None, None, 1, 4, 3]
    args += [None] * (len(_hip._SIGS["smcdet_aggregate_sweep"][0]) - len(args))
    args[16], args[17] = 1, 0  # seed, offset
    rc = L.smcdet_aggregate_sweep(*args)
    err = L.smcdet_last_error()
    assert rc == EUNSUPPORTED and b"smcdet_aggregate_sweep" in err and \
        b"Normal flux prior" in err, (rc, err)


class _Img:
    """What the samplers' constructors look at before they refuse."""
    is_cuda = False
    shape = (16, 16)

    def dim(self):
        return 2


def test_python_classes_refuse_at_construction():
    from smcdet_amd.aggregate import Aggregate
    from smcdet_amd.images import M71ImageModel
    from smcdet_amd.sampler import MHsampler, SMCsampler
    from tests._params import p_m71_model
    from tests._star import p_star_mala, p_star_mh, p_star_model
    pr = p_star_prior(16, 3, 3)
    m71 = p_m71_model(16)
    assert isinstance(m71, M71ImageModel)
    for kernel in (p_star_mh(5), p_star_mala(5)):
        with pytest.raises(NotImplementedError, match="StarPrior"):
            SMCsampler(_Img(), 16, pr, m71, kernel, 8, 0.5, "systematic", 0.0, 10)
    with pytest.raises(NotImplementedError, match="StarPrior"):
        MHsampler(_Img(), 16, pr, p_star_model(16), 0.25, 100.0, 0.0, 10, 2)
    with pytest.raises(NotImplementedError, match="StarPrior"):
        Aggregate(pr, p_star_model(16), p_star_mh(5), None, None, None, None, None, None, 0.0,
                  "systematic", 0.5)


def test_float64_normal_log_prior_matches_reference():
    d = golden("star_prior.npz")
    lp = normal_log_prior(d["counts"], d["locs"], d["fluxes"], o_star_prior(16, 0, 3))
    ref = d["logprior"]
    assert sorted(set(d["counts"].ravel().tolist())) == [0.0, 1.0, 2.0, 3.0]
    ninf = np.isneginf(ref)
    assert ninf.sum() == 2 and np.array_equal(np.isneginf(lp), ninf)
    np.testing.assert_allclose(lp[~ninf], ref[~ninf], rtol=1e-6, atol=1e-3)
    # the edge cases are in the fixture: an active flux of exactly 0 (finite: no
    # substitution) and a negative one
    on = np.arange(3) < d["counts"][..., None]
    assert (d["fluxes"][on] == 0).sum() == 1 and (d["fluxes"][on] < 0).sum() == 1
    assert np.isfinite(ref[(on & (d["fluxes"] <= 0)).any(-1)]).all()


@pytest.mark.parametrize("name", sorted(STAR_MH_FIXTURES))
def test_float64_oracle_reproduces_mh_fixture_decisions(name):
    d = golden(name + ".npz")
    on = np.arange(d["fluxes0"].shape[-1]) < d["counts"][..., None]
    f0 = d["fluxes0"][on]
    assert f0.min() >= STAR["fluxes_min"] and f0.max() <= STAR["fluxes_max"]
    l, f, acc_rate, loga, acc = oracle_mh_trace(d, name)
    np.testing.assert_array_equal(acc, d["accept"].astype(bool))
    m = decision_margin(d, loga)
    print(name, "smallest |log u - log alpha| %.3e" % m)
    assert m >= 1e-4
    np.testing.assert_allclose(l, d["locs1"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(f, d["fluxes1"], rtol=1e-6, atol=5e-4)
    np.testing.assert_array_equal(acc_rate.astype(np.float32), d["acc"])
    if name == "star_mh_16x16":  # strata with padded slots, N no multiple of 4
        assert d["counts"].shape[-1] == 30 and set(d["counts"].ravel().tolist()) == {1.0, 2.0, 3.0}
