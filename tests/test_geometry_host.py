"""SMCDET_MH_GENERIC_GEOMETRY on the host side (no GPU): the flag's value in
the ctypes binding equals the header's, it is a bit of its own, and the product
library takes it -- it is not one of the diagnostic build's flags.  Nothing is
launched: the calls carry null buffers and end at argument validation, which
comes after the check of the flags."""
import ctypes
import os
import re

from smcdet_amd import _hip

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "smcdet_hip.h")


def _mh_flags():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {k: int(v) for k, v in re.findall(r"#define (SMCDET_MH_\w+) (\d+)u", txt)}


def test_flag_value_matches_the_header_and_is_a_free_bit():
    flags = _mh_flags()
    v = flags["SMCDET_MH_GENERIC_GEOMETRY"]
    assert v == _hip.SMCDET_MH_GENERIC_GEOMETRY == 2 * flags["SMCDET_MH_NO_BLOCK"]
    assert v & (v - 1) == 0
    assert all(v & o == 0 for k, o in flags.items() if k != "SMCDET_MH_GENERIC_GEOMETRY")
    assert "#define SMCDET_ABI_VERSION 20" in open(HEADER).read() and _hip.ABI_VERSION == 20


def _null_buffer_call(L, flags):
    m = _hip.ImageModelC()
    m.model, m.H, m.W, m.psf_radius = 1, 32, 32, 8
    m.background, m.adu_per_nmgy, m.psf_norm = 100.0, 1.0, 1.0
    m.psf_params[:] = [1.0, 2.0, 2.0, 5.0, 0.5, 0.5]
    m.noise_additive, m.noise_multiplicative = 1e-10, 1.9
    p = _hip.PriorC()
    p.kind, p.min_objects, p.max_objects = 1, 10, 10
    p.loc_low, p.loc_high_h, p.loc_high_w = -4.0, 36.0, 36.0
    p.poisson_mean, p.flux_alpha, p.flux_lower, p.flux_upper = 5.0, 0.2, 0.06, 1800.0
    mh = _hip.MHC()
    mh.num_iters, mh.locs_stdev, mh.fluxes_stdev = 1, 0.1, 2.5
    mh.fluxes_min, mh.fluxes_max = 0.06, 1800.0
    mh.locs_min_h = mh.locs_min_w = -4.0
    mh.locs_max_h = mh.locs_max_w = 36.0
    return L.smcdet_mh_sweep(ctypes.byref(m), ctypes.byref(p), ctypes.byref(mh), None, None,
                             1, 64, 10, None, None, None, None, None, None, None, None, None,
                             1, 0, None, flags, None, None, None, None, None, None)


def test_product_build_does_not_refuse_the_flag():
    L = _hip.lib()
    assert not _hip.is_diag(L)
    g = _hip.SMCDET_MH_GENERIC_GEOMETRY
    for flags in (0, g, g | 2048 | 16384):  # with the product's other diagnostic flags
        assert _null_buffer_call(L, flags) == -1, flags  # SMCDET_EINVAL
        assert b"null buffer" in L.smcdet_last_error(), flags
    # a diagnostic-build flag is refused at the same place, with or without it
    for flags in (4096, g | 4096):
        assert _null_buffer_call(L, flags) == -2, flags  # SMCDET_EUNSUPPORTED
        assert b"diagnostic build" in L.smcdet_last_error(), flags
