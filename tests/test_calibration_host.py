"""smcdet_amd.calibration without a GPU: the numpy oracle
(tests/_calibration_oracle.py) against torch.quantile and
condense.flux_quantiles on the CPU, the header / binding bookkeeping, the
argument validation of the three entry points (no kernel is launched: every
call carries a null pointer or a size the host check refuses), the wrappers'
refusal of CPU tensors and the Philox index formula."""
import ctypes
import os

import numpy as np
import pytest
import torch

from smcdet_amd import _hip, calibration, condense
from tests import _calibration_oracle as O

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "smcdet_hip.h")
NAMES = ("smcdet_catalog_totals", "smcdet_row_summary", "smcdet_bootstrap_means")


# ---- the oracle against independent implementations -----------------------------
@pytest.mark.parametrize("N", [1, 2, 65, 1000])
def test_oracle_linear_quantiles_match_torch(N):
    rng = np.random.default_rng(N)
    v = rng.lognormal(1.0, 1.0, (4, N)).astype(np.float32)
    v[1] = np.round(v[1])  # ties
    got = O.row_summary(v, None, O.Q_LEVELS, "linear")["quantiles"]
    want = torch.quantile(torch.from_numpy(v).double(),
                          torch.tensor(O.Q_LEVELS, dtype=torch.float64), dim=-1).t().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


def test_oracle_linear_quantiles_skip_nan():
    v = np.array([[3.0, np.nan, 1.0, 2.0, np.nan]], np.float32)
    s = O.row_summary(v, None, (0.0, 0.25, 0.5, 1.0), "linear", np.array([[2.0]], np.float32))
    assert s["quantiles"][0].tolist() == [1.0, 1.5, 2.0, 3.0]
    assert s["n_valid"][0] == 3 and s["mean"][0] == 2.0 and s["var"][0] == 2.0 / 3.0
    assert s["below"][0, 0] == 1 and s["at_or_below"][0, 0] == 2
    s = O.row_summary(np.full((1, 4), np.nan, np.float32), None, (0.5,), "linear",
                      np.array([[0.0]], np.float32))
    assert s["n_valid"][0] == 0 and np.isnan(s["quantiles"]).all() and np.isnan(s["mean"][0])
    assert s["below"][0, 0] == 0 and s["at_or_below"][0, 0] == 0


def test_oracle_lower_quantiles_equal_condense_on_cpu():
    """interpolation="lower" is condense.flux_quantiles' definition (plain torch)."""
    rng = np.random.default_rng(2)
    mf = rng.uniform(1, 30, (2, 40, 3)).astype(np.float32)
    mf[rng.uniform(size=mf.shape) < 0.4] = np.nan
    mf[1, :, 2] = np.nan
    mf[0, 3, 0] = mf[0, 4, 0]
    w = O.dyadic_weights(rng, (2, 40))
    qs = (0.0, 0.05, 0.26, 0.5, 0.95, 1.0)
    for weights in (None, w):
        want = condense.flux_quantiles(torch.from_numpy(mf), qs,
                                       None if weights is None else torch.from_numpy(weights))
        rows = mf.transpose(0, 2, 1).reshape(6, 40)
        wr = None if weights is None else np.repeat(weights, 3, axis=0)
        got = O.row_summary(rows, wr, qs, "lower")["quantiles"].reshape(2, 3, len(qs))
        np.testing.assert_array_equal(O.f32(got), want.numpy())


def test_posterior_case_rests_on_no_tie():
    """Every truth of the shared posterior case is farther from both ends of
    every interval than the quantile tolerance, so `covered` can be compared in
    every entry on the GPU."""
    case = O.posterior_case()
    assert (case["true_counts"] == 0).any() and (case["true_counts"] > 0).sum() >= 4
    for cut in (0.0, 10.0):
        cov = O.calibrate(case, cut)["coverage"]
        s = cov["exact"]
        tol = O.quantile_tolerance(s["quantiles"], s["v_lo"], s["v_hi"])
        assert (cov["margin"] > tol).all()
        assert 0.1 < cov["covered"].mean() < 0.9  # both outcomes occur


# ---- header, constants, bindings ---------------------------------------------------
def test_abi_names_and_constants():
    hdr = open(HEADER).read()
    for name, value in (("TOTALS_MAX_CUTS", 8), ("SUMMARY_MAX_N", 16384), ("SUMMARY_MAX_Q", 64),
                        ("SUMMARY_MAX_E", 65), ("SUMMARY_LINEAR", 0), ("SUMMARY_LOWER", 1),
                        ("BOOT_MAX_COLUMNS", 256)):
        assert getattr(_hip, name) == value
        assert f"#define SMCDET_{name} {value} " in hdr.replace("\n", " \n")
    assert "#define SMCDET_ABI_VERSION 20" in hdr and _hip.ABI_VERSION == 20
    assert "added under SMCDET_ABI_VERSION 20" in hdr
    for name in NAMES:
        assert name in hdr and name in _hip.EXPORTS and name in _hip._OUTS
        assert hasattr(_hip.lib(), name)
    assert _hip.lib().smcdet_abi_version() == 20
    assert any(p.endswith("summary_kernel.hip") for p in _hip.SOURCES)
    assert "calibration" in __import__("smcdet_amd")._DROP_IN


def test_philox_tag_is_new():
    dev = open(os.path.join(os.path.dirname(HEADER), "..", "smcdet_amd", "csrc",
                            "device.h")).read()
    import re
    tags = re.findall(r"(kTag\w+) = (0x[0-9a-f]+)u", dev)
    assert ("kTagBoot", hex(_hip.BOOT_TAG)) in tags and O.BOOT_TAG == _hip.BOOT_TAG
    assert len({v for _, v in tags}) == len(tags)


# ---- the C ABI: every argument validated before any device work -------------------
def _totals(T=1, N=4, S=3, C=1, p=None):
    return _hip.lib().smcdet_catalog_totals(p, p, p, T, N, S, C, p, p, None)


def _summary(A=1, N=4, B=1, Q=1, interp=0, E=1, p=None, weights=None, q=None):
    return _hip.lib().smcdet_row_summary(p, weights, A, N, B, q, Q, interp, p, E, p, p, p, p, p, p,
                                         p, p, p, None)


def _boot(M=4, D=3, Bn=2, p=None):
    return _hip.lib().smcdet_bootstrap_means(p, M, D, None, 0, Bn, p, None)


@pytest.mark.parametrize("call", [_totals, _summary, _boot])
def test_abi_null_pointer_is_einval(call):
    assert call() == -1
    assert "null" in _hip.lib().smcdet_last_error().decode()


@pytest.mark.parametrize("call,kw,word", [
    (_totals, dict(C=9), "8"), (_totals, dict(S=65), "64"), (_totals, dict(T=2 ** 30, N=4), "2^31"),
    (_summary, dict(N=16385), "16384"), (_summary, dict(Q=65), "64"), (_summary, dict(E=66), "65"),
    (_summary, dict(A=2 ** 20, B=2 ** 12), "2^31"), (_boot, dict(D=257), "256")])
def test_abi_limits_are_eunsupported_and_named(call, kw, word):
    assert call(**kw) == -2
    assert word in _hip.lib().smcdet_last_error().decode()


@pytest.mark.parametrize("call,kw", [
    (_totals, dict(T=0)), (_totals, dict(N=0)), (_totals, dict(S=0)), (_totals, dict(C=0)),
    (_summary, dict(A=0)), (_summary, dict(N=0)), (_summary, dict(B=0)), (_summary, dict(Q=-1)),
    (_summary, dict(E=-1)), (_summary, dict(interp=2)),
    (_boot, dict(M=0)), (_boot, dict(D=0)), (_boot, dict(Bn=0))])
def test_abi_sizes_are_einval(call, kw):
    assert call(**kw) == -1


def test_abi_limits_pass_on_to_the_null_check():
    """The largest supported sizes are not refused as limits (the null buffers are)."""
    assert _summary(N=16384, Q=64, E=65) == -1
    assert _totals(C=8, S=64) == -1 and _boot(D=256) == -1
    assert "null" in _hip.lib().smcdet_last_error().decode()


def test_abi_linear_with_weights_is_einval():
    # the weights pointer is a placeholder; every other buffer is null
    assert _summary(interp=_hip.SUMMARY_LINEAR, weights=ctypes.c_void_p(64)) == -1
    assert "weights" in _hip.lib().smcdet_last_error().decode()
    assert _summary(interp=_hip.SUMMARY_LOWER, weights=ctypes.c_void_p(64)) == -1
    assert "null" in _hip.lib().smcdet_last_error().decode()


# ---- the Python layer ------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors():
    case = O.posterior_case(T=2, N=8)
    t = {k: torch.from_numpy(v) for k, v in case.items()}
    calls = [
        lambda: calibration.catalog_totals(t["est_counts"], t["est_fluxes"]),
        lambda: calibration.row_summary(t["rows"]),
        lambda: calibration.row_summary(t["est_total"], dim=1, quantiles=(0.5,)),
        lambda: calibration.credible_intervals(t["rows"], (0.9,)),
        lambda: calibration.coverage(t["rows"], t["rows"][:, 0]),
        lambda: calibration.count_posterior(t["est_counts"], 5),
        lambda: calibration.luminosity_function(t["est_total"]),
        lambda: calibration.bootstrap_means(t["rows"], 4, seed=1),
        lambda: calibration.bootstrap_ci(t["rows"], 4, seed=1),
        lambda: calibration.calibrate(t["true_counts"], t["true_fluxes"], t["est_counts"],
                                      t["est_fluxes"]),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_count_confusion_is_plain_torch():
    mass = torch.tensor([[3.0, 1.0, 0.0], [0.0, 2.0, 2.0], [1.0, 1.0, 2.0]], dtype=torch.float64)
    true = torch.tensor([0, 2, 2])
    got = calibration.count_confusion(mass, true, 2)
    assert got.tolist() == [[3.0, 0.0, 1.0], [1.0, 0.0, 3.0], [0.0, 0.0, 4.0]]
    np.testing.assert_array_equal(got.numpy(), O.count_confusion(mass.numpy(), true.numpy(), 2))
    mode = torch.tensor([0, 1, 2])
    got = calibration.count_confusion(mode, true, 2, 3)
    assert got.tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 0]]
    np.testing.assert_array_equal(got.numpy(), O.count_confusion(mode.numpy(), true.numpy(), 2, 3))
    # a true count above max_true is in no column
    assert calibration.count_confusion(mode, true, 1, 2).sum() == 1


# ---- the bootstrap's index formula ---------------------------------------------------
def test_philox_known_answers():
    """Random123's published vectors for Philox4x32-10."""
    assert [int(x) for x in O.philox4x32(0, 0, 0, 0, 0, 0)] == \
        [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert [int(x) for x in O.philox4x32(f, f, f, f, f, f)] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


@pytest.mark.parametrize("M", [1, 3, 2 ** 31 - 1])
def test_boot_index_formula_stays_in_range(M):
    """mulhi32(x, M) lies in [0, M) for every 32-bit x: the extremes, then
    Philox draws laid out as the kernel lays them out."""
    x = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], np.uint64)
    idx = (x * np.uint64(M)) >> np.uint64(32)
    assert idx.min() >= 0 and idx.max() < M and idx[0] == 0 and idx[-1] == M - 1
    if M <= 3:
        idx = O.boot_indices(12345, 50, M)
        assert idx.shape == (50, M) and idx.min() >= 0 and idx.max() < M
        if M == 3:
            assert set(np.unique(idx)) == {0, 1, 2}
    else:  # the formula on 4000 draws without an [Bn, M] array
        draws = np.stack(O.philox4x32(np.arange(1000), 0, 0, O.BOOT_TAG, 12345, 0), -1)
        idx = (draws * np.uint64(M)) >> np.uint64(32)
        assert idx.min() >= 0 and idx.max() < M and idx.max() > M // 2
