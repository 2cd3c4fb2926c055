"""SMCDET_MH_NO_WRITE_THROUGH on the host side (no GPU): the flag's value in the
ctypes binding equals the header's, it is a bit of its own, and the product
library takes it (nothing is launched: the call carries null buffers and ends
at argument validation, which comes after the check of the flags)."""
from smcdet_amd import _hip
from tests.test_geometry_host import _mh_flags, _null_buffer_call


def test_flag_value_matches_the_header_and_is_a_free_bit():
    flags = _mh_flags()
    v = flags["SMCDET_MH_NO_WRITE_THROUGH"]
    assert v == _hip.SMCDET_MH_NO_WRITE_THROUGH == 2 * flags["SMCDET_MH_GENERIC_GEOMETRY"]
    assert v & (v - 1) == 0
    assert all(v & o == 0 for k, o in flags.items() if k != "SMCDET_MH_NO_WRITE_THROUGH")


def test_product_build_does_not_refuse_the_flag():
    L = _hip.lib()
    assert not _hip.is_diag(L)
    w = _hip.SMCDET_MH_NO_WRITE_THROUGH
    for flags in (w, w | _hip.SMCDET_MH_GENERIC_GEOMETRY):
        assert _null_buffer_call(L, flags) == -1, flags  # SMCDET_EINVAL
        assert b"null buffer" in L.smcdet_last_error(), flags
