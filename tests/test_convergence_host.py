"""smcdet_amd.convergence without a GPU: the numpy oracle
(tests/_convergence_oracle.py) against an independent FFT autocovariance and
the AR(1) theory, the margins every GPU case rests on, the header / binding
bookkeeping, and the refusals of the C entry points (no kernel is launched:
every call carries a null pointer or a size the host check refuses) and of the
Python layer."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from smcdet_amd import _hip, convergence
from tests import _convergence_oracle as O

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "smcdet_hip.h")
NAMES = ("smcdet_chain_stats", "smcdet_chain_stats_workspace")


# ---- the oracle is sound -----------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 64, 129, 1000])
def test_direct_autocovariance_equals_fft(n):
    rng = np.random.default_rng(n)
    c = O.ar1(rng, 0.9, (3, n)).astype(np.float64)
    d = c - c.mean(axis=1, keepdims=True)
    fft = O.autocov_fft(d)
    for t in range(n):
        np.testing.assert_allclose(O.autocov(d, t), fft[:, t], rtol=0, atol=1e-10 * fft[:, 0].max())
    assert (O.autocov(d, n) == 0).all()


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9, -0.5])
def test_ar1_tau_approaches_theory(phi):
    """One chain of 200,000 draws, unsplit: tau -> (1 + phi) / (1 - phi).  The
    initial-sequence estimator's standard error is about tau * sqrt(2 (2 K + 1)
    / n) for a cut-off at K pairs (Geyer 1992, the window estimator's variance);
    the band is five of those plus the truncation bias phi^(2K) / (1 - phi)."""
    n = 200_000
    x = O.ar1(np.random.default_rng(11), phi, (1, n))
    r = O.row_stats(x, split=False)
    theory = (1 + phi) / (1 - phi)
    K = r["n_pairs"]
    band = 5 * theory * math.sqrt(2 * (2 * K + 1) / n) + 2 * abs(phi) ** (2 * K) / (1 - abs(phi))
    assert abs(r["tau"] - theory) < band, (r["tau"], theory, band)
    assert band < 0.2 * theory + 0.05


def test_iid_ess_is_about_all_draws():
    x = O.ar1(np.random.default_rng(5), 0.0, (8, 4, 2000))
    o = O.chain_stats(x)
    assert o["m"] == 8 and o["n"] == 1000
    # tau = -1 + 2 sum of K ~ 1-3 pairs, each 1 +- a few / sqrt(m n): within 15 %
    assert np.all(np.abs(o["ess"] / 8000 - 1) < 0.15)
    assert np.all(np.abs(o["rhat"] - 1) < 0.01)


def test_tau_respects_its_floor():
    """An antithetic chain has -1 + 2 sum P' far below 1 / log10(m n)."""
    x = np.tile(np.array([1.0, -1.0], np.float32), 50)[None] * \
        np.random.default_rng(3).uniform(0.9, 1.1, (2, 100)).astype(np.float32)
    r = O.row_stats(x)
    assert r["floor"] and r["tau"] == 1 / math.log10(200) and r["ess"] == 200 / r["tau"]
    assert -1 + 2 * sum(np.minimum.accumulate(r["P"][:r["n_pairs"]])) < 0.1 < r["tau"]


def test_split_drops_the_middle_draw():
    x = np.arange(2 * 9, dtype=np.float32).reshape(2, 9)
    c = O.split_chains(x, True)
    assert c.tolist() == [[0, 1, 2, 3], [5, 6, 7, 8], [9, 10, 11, 12], [14, 15, 16, 17]]
    assert O.split_chains(x, False) is x or (O.split_chains(x, False) == x).all()


def test_oracle_degenerate_rows():
    x, names = O.special_rows()
    o = O.chain_stats(x, num_rho=4)
    for i, name in enumerate(names):
        dead = name in ("nan", "inf", "constant", "constant_chains_apart")
        assert np.isnan(o["rhat"][i]) == dead and np.isnan(o["ess"][i]) == dead, name
        assert np.isnan(o["rho"][i]).all() == dead
        if dead:
            assert o["n_pairs"][i] == 0 and o["stopped"][i] == 0
    assert np.isnan(o["mean"][:2]).all() and o["mean"][2] == 2.5 and o["W"][2] == 0
    assert o["W"][7] == 0 and o["var_plus"][7] == 0.8  # B / n of the means 0, 0, 1, 1, 2, 2
    assert o["rhat"][6] > 50  # chains 100 apart


# ---- every GPU case rests on no tie ----------------------------------------------------
@pytest.mark.parametrize("name", sorted(O.cases()))
def test_gpu_case_rests_on_no_tie(name):
    """The pairs that decide the cut-off (the last kept, the first refused) are
    farther from 0 than 20 x the bound 2 eps_rho on a pair's error."""
    e = O.expected(name)
    live = ~np.isnan(e["rhat"])
    assert live.any()
    assert np.all(e["margin"][live] > 20 * 2 * e["eps_rho"][live]), (e["margin"], e["eps_rho"])
    # the bound itself is the float32 rounding term, not an artefact of the offsets
    assert np.all(e["eps_rho"][live] < 1.01 * 2 * O.U32 + 1e-9)


def test_gpu_cases_cover_the_cut_offs():
    """K = 1, the lag block size -1 / +0 / +1 pairs, hundreds of pairs, lags that
    ran out, a max_lag below the natural cut-off, and both storage paths."""
    B = O.BLOCK_PAIRS
    for K, _ in O.BLOCK_SEEDS:
        e = O.expected(f"block_K{K}")
        assert e["n_pairs"].tolist() == [K] and e["stopped"].tolist() == [1]
    assert [K for K, _ in O.BLOCK_SEEDS] == [B - 1, B, B + 1]
    allK = np.concatenate([O.expected(n)["n_pairs"] for n in O.cases()])
    allS = np.concatenate([O.expected(n)["stopped"] for n in O.cases()])
    assert (allK == 1).any() and (allK > 300).any() and ((allS == 0) & (allK > 0)).any()
    assert (O.expected("unsplit_C1_M10000")["n_pairs"] > 50).any()
    free = O.chain_stats(O.cases()["max_lag_5"]["x"])
    assert (free["n_pairs"] > O.expected("max_lag_5")["n_pairs"]).any()
    sizes = {n: O.expected(n)["m"] * O.expected(n)["n"] for n in O.cases()}
    assert sizes["lds_limit"] == O.LDS_DRAWS == _hip.CHAINS_LDS_DRAWS
    assert sizes["lds_limit_plus_chain"] == O.LDS_DRAWS + O.expected("lds_limit_plus_chain")["m"]
    assert sizes["mcmc_C4_M10000"] == 40000 and sizes["one_row_4x16384"] == 65536
    assert sizes["split_n5000_C1"] == 10000 <= O.LDS_DRAWS  # run_mcmc with one chain: LDS
    halves = {O.expected(n)["n"] for n in O.cases() if n.startswith("split_n")}
    assert halves == {4, 5, 63, 64, 65, 127, 128, 129, 1000, 5000}
    rhos = {O.cases()[n]["num_rho"] for n in O.cases()}
    assert {0, 1, 64, 1024} <= rhos
    assert any(c["num_rho"] > O.expected(n)["n"] - 1 for n, c in O.cases().items())


@pytest.mark.parametrize("name", sorted(O.diagnose_cases()))
def test_diagnose_case_thresholds_meet_no_draw_by_accident(name):
    """The tail thresholds and the median lie strictly between two draws (so a
    last-bit difference cannot move a draw across them), except on the integer
    chain, where they are draws on purpose; the stacked quantities' cut-offs
    rest on no tie either."""
    for x in O.diagnose_cases()[name]:
        q = O.diagnose_inputs(x)
        for key in ("q_lo", "med", "q_hi"):
            gap = np.abs(x.astype(np.float64) - float(q[key])).min()
            if name == "sticky":
                assert gap == 0.0
            else:
                assert gap > 8 * np.spacing(np.float32(abs(q[key])))
        for key in ("raw", "z", "z_folded", "lo", "hi"):
            r = O.row_stats(q[key].astype(np.float32))
            assert r["margin"] > 20 * 2 * r["eps_rho"], (name, key)


def test_big_diagnose_row_thresholds_meet_no_draw():
    x = O.big_diagnose_row()
    assert x.size > _hip.SUMMARY_MAX_N
    for q in (0.05, 0.5, 0.95):
        v = O.linear_quantile(x, q)
        assert np.abs(x.astype(np.float64) - float(v)).min() > 8 * np.spacing(np.float32(abs(v)))


def test_rank_normalize_oracle_handles_ties():
    x = np.array([[1.0, 2.0, 2.0, 5.0], [2.0, 0.0, 9.0, 9.0]], np.float32)
    assert O.average_ranks(x).tolist() == [[2.0, 4.0, 4.0, 6.0], [4.0, 1.0, 7.5, 7.5]]
    z = O.rank_normalize(x)
    assert z[0, 1] == z[0, 2] == z[1, 0] and z[1, 1] < z[0, 0] < z[0, 1] < z[0, 3] < z[1, 2]
    mid = O.rank_normalize(np.arange(5, dtype=np.float32)[None])  # (3 - 3/8) / (5 + 1/4) = 1/2
    assert abs(mid[0, 2]) < 1e-15 and abs(mid[0, 0] + mid[0, 4]) < 1e-15
    got = convergence.average_ranks(torch.from_numpy(x))
    assert got.tolist() == O.average_ranks(x).tolist()
    zt = convergence.rank_normalize(torch.from_numpy(x))
    np.testing.assert_allclose(zt.numpy(), z, atol=2e-7)


# ---- header, constants, bindings -------------------------------------------------------
def test_abi_names_and_constants():
    hdr = open(HEADER).read()
    for name, value in (("CHAINS_MAX_CHAINS", 32), ("CHAINS_MAX_DRAWS", 1048576),
                        ("CHAINS_MAX_RHO", 1024), ("CHAINS_LDS_DRAWS", O.LDS_DRAWS),
                        ("CHAINS_BLOCK_PAIRS", O.BLOCK_PAIRS)):
        assert getattr(_hip, name) == value
        assert f"#define SMCDET_{name} {value} " in hdr.replace("\n", " \n")
    assert "#define SMCDET_ABI_VERSION 20" in hdr and _hip.ABI_VERSION == 20
    assert "MCMC convergence diagnostics (added under SMCDET_ABI_VERSION 20)" in hdr
    for name in NAMES:
        assert name in hdr and name in _hip.EXPORTS and name in _hip._OUTS
        assert hasattr(_hip.lib(), name)
    assert _hip.lib().smcdet_abi_version() == 20
    assert any(p.endswith("convergence_kernel.hip") for p in _hip.SOURCES)
    srcs = open(os.path.join(ROOT, "Makefile")).read().split("SRCS :=")[1].split("\n")[0].split()
    listed = [os.path.basename(p) for p in _hip.SOURCES if p.endswith(".hip")]
    assert [os.path.basename(s) for s in srcs] == listed
    assert "convergence" in __import__("smcdet_amd")._DROP_IN


# ---- the C ABI: every argument validated before any device work ---------------------
def _stats(R=1, C=2, M=16, split=1, max_lag=7, num_rho=0, base=None, ws=None, ws_floats=0):
    """Null buffers, or with `base` distinct placeholder addresses (never read:
    only calls the host checks refuse are made)."""
    p = [None if base is None else ctypes.c_void_p(base + 64 * i) for i in range(11)]
    return _hip.lib().smcdet_chain_stats(p[0], R, C, M, split, max_lag, num_rho, *p[1:10], None,
                                         None, p[10], ws, ws_floats, None)


def _err():
    return _hip.lib().smcdet_last_error().decode()


def test_abi_null_pointer_is_einval():
    assert _stats() == -1 and "null" in _err()
    assert _stats(num_rho=4) == -1 and "null" in _err()


@pytest.mark.parametrize("kw,word", [
    (dict(C=33), "32"), (dict(C=32, M=2 * 16384 + 2), "1048576"),
    (dict(C=1, M=1048577, split=0), "1048576"), (dict(num_rho=1025), "1024"),
    (dict(R=2 ** 26, C=32), "2^31")])
def test_abi_limits_are_eunsupported_and_named(kw, word):
    assert _stats(**kw) == -2
    assert word in _err()
    if "num_rho" not in kw:
        assert _hip.lib().smcdet_chain_stats_workspace(kw.get("R", 1), kw.get("C", 2),
                                                       kw.get("M", 16), kw.get("split", 1)) == -2
        assert word in _err()


@pytest.mark.parametrize("kw", [dict(R=0), dict(C=0), dict(M=0), dict(M=7), dict(M=3, split=0),
                                dict(max_lag=0), dict(num_rho=-1)])
def test_abi_sizes_are_einval(kw):
    assert _stats(**kw) == -1
    assert "null" not in _err()


def test_abi_limits_pass_on_to_the_null_check():
    """The largest supported sizes are not refused as limits (the null buffers are)."""
    assert _stats(C=32, M=32768, num_rho=1024) == -1 and "null" in _err()
    assert _stats(C=1, M=1048576, split=0) == -1 and "null" in _err()
    assert _stats(M=8) == -1 and "null" in _err()  # n = 4


def test_abi_workspace_sizes():
    L = _hip.lib()
    assert L.smcdet_chain_stats_workspace(5, 4, 4096, 1) == 0          # m n = 16384: LDS
    assert L.smcdet_chain_stats_workspace(5, 4, 4098, 1) == 5 * 16392
    assert L.smcdet_chain_stats_workspace(3, 4, 10001, 1) == 3 * 40000  # the middle draw is dropped
    assert L.smcdet_chain_stats_workspace(996, 1, 10000, 1) == 0        # run_mcmc, one chain
    assert L.smcdet_chain_stats_workspace(1, 4, 16384, 0) == 65536
    assert L.smcdet_chain_stats_workspace(1, 1, 7, 1) == -1 and "4" in _err()


def test_abi_small_workspace_is_einval_and_names_the_size():
    """Placeholder pointers everywhere (nothing is launched: the workspace check
    refuses the call first)."""
    for ws, floats in ((None, 0), (ctypes.c_void_p(1 << 20), 5 * 16392 - 1)):
        assert _stats(R=5, C=4, M=4098, base=4096, ws=ws, ws_floats=floats) == -1
        assert str(5 * 16392) in _err() and "workspace" in _err()


# ---- the Python layer ------------------------------------------------------------------
def test_python_refusals_name_the_limit():
    z = torch.zeros
    for call, word in [
            (lambda: convergence.chain_stats(z(10)), "C,M"),
            (lambda: convergence.chain_stats(z(2, 33, 8)), "32"),
            (lambda: convergence.chain_stats(z(2, 2, 7)), "at least 4"),
            (lambda: convergence.chain_stats(z(2, 2, 3), split=False), "at least 4"),
            (lambda: convergence.chain_stats(z(1, 32, 32770)), "1048576"),
            (lambda: convergence.chain_stats(z(2, 2, 8), num_rho=1025), "1024"),
            (lambda: convergence.chain_stats(z(2, 2, 8), max_lag=0), "max_lag"),
            (lambda: convergence.diagnose(z(2, 2, 7)), "at least 4"),
            (lambda: convergence.diagnose(z(2, 2, 8), tail_prob=0.5), "tail_prob"),
            (lambda: convergence.rank_normalize(z(8)), "C,M")]:
        with pytest.raises(ValueError, match=word):
            call()


def test_wrappers_refuse_cpu_tensors():
    x = torch.from_numpy(O.cases()["split_n5_C3"]["x"])
    for call in (lambda: convergence.chain_stats(x), lambda: convergence.diagnose(x)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()


def test_unrun_sampler_raises_without_a_device():
    class Unrun:
        has_run = False
    with pytest.raises(RuntimeError, match="run the sampler first"):
        convergence.diagnose_sampler(Unrun())


def test_warnings_lists_failing_rows():
    f = lambda *v: torch.tensor(v, dtype=torch.float64).reshape(1, 1, -1)
    c = convergence.Convergence(f(1.0, 1.02, 1.0, float("nan")), f(500, 500, 399, 500),
                                f(450, 450, 450, 450), f(1, 1, 1, 1), f(1, 1, 1, 1), f(1, 1, 1, 1),
                                f(0, 0, 0, 0), torch.ones(1, 1, 4, dtype=torch.int32), None,
                                names=("a", "b", "c", "d"))
    w = c.warnings()
    assert [(i, n) for i, n, *_ in w] == [((0, 0, 1), "b"), ((0, 0, 2), "c"), ((0, 0, 3), "d")]
    assert c.warnings(rhat_max=1.05, ess_min=100)[0][1] == "d"
    lag = convergence.ChainStats(*([None] * 7), torch.tensor([0, 7, 8, 8, 20]),
                                 torch.tensor([0, 1, 0, 1, 1]), None, None, None, 2, 100)
    assert lag.lag_blocks.tolist() == [1, 1, 1, 2, 3]
