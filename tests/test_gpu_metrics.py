"""smcdet_amd.metrics.match_catalogs on the GPU against the reference's
recorded outputs (tests/golden/metrics.npz) and the CPU oracle
(tests/_metrics_oracle.py: the exact lexicographic optimum).  The in-test
cases keep the fixture generator's margins (synth_case), so float32 rounding on
the device cannot flip a tolerance, a bin or the optimum."""
import os

import numpy as np
import pytest
import torch

from smcdet_amd import metrics
from tests import _metrics_oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
NAMES = ("true_total", "true_matches", "est_total", "est_matches")
INPUTS = ("true_counts", "true_locs", "true_fluxes", "est_counts", "est_locs", "est_fluxes")
BINS = np.arange(16, 24.5, 0.5, dtype=np.float32)
TOL = 0.5


def dev_args(case):
    return [torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in INPUTS]


def run(case, bins, M=None, index=None, locs_tol=TOL, mags_tol=TOL):
    idx = None if index is None else torch.from_numpy(np.asarray(index))
    out = metrics.match_catalogs(*dev_args(case), M, locs_tol, mags_tol, torch.from_numpy(bins),
                                 index=idx, return_matches=True)
    assert all(o.is_cuda for o in out)
    assert all(o.dtype == torch.float32 for o in out[:4]) and out[4].dtype == torch.int32
    return [o.cpu().numpy() for o in out]


def check_against_oracle(case, bins, index=None, **kw):
    N = case["est_counts"].shape[1]
    T = case["est_counts"].shape[0]
    full = np.tile(np.arange(N), (T, 1)) if index is None else np.asarray(index)
    got = run(case, bins, index=index, **kw)
    want = O.match_catalogs(*[case[k] for k in INPUTS], full, kw.get("locs_tol", TOL),
                            kw.get("mags_tol", TOL), bins)
    for g, w, name in zip(got, want, NAMES + ("match_of_true",)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    return got


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def small(gold):
    """(device outputs with the stored index, oracle outputs), computed once."""
    got = run(gold, gold["mag_bins"], index=gold["index"])
    want = O.match_catalogs(*[gold[k] for k in INPUTS], gold["index"], TOL, TOL, gold["mag_bins"])
    return got, want


def test_small_equals_oracle_everywhere(small):
    got, want = small
    assert got[0].shape == (24, 32, 17) and got[4].shape == (24, 32, 10)
    for g, w, name in zip(got, want, NAMES + ("match_of_true",)):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_small_equals_reference(gold, small):
    got, _ = small
    lex = gold["ref_is_lex"]
    assert 0 < (~lex).sum() <= 0.02 * lex.size  # the fixture holds non-lexicographic cases
    for k, name in enumerate(NAMES):
        np.testing.assert_array_equal(got[k][lex], gold[f"ref_{name}"][lex], err_msg=name)
    np.testing.assert_array_equal(got[0], gold["ref_true_total"])
    np.testing.assert_array_equal(got[2], gold["ref_est_total"])
    np.testing.assert_array_equal(got[1].sum(-1), gold["ref_true_matches"].sum(-1))
    np.testing.assert_array_equal(got[3].sum(-1), gold["ref_est_matches"].sum(-1))


def test_small_draws_the_references_index(gold, small):
    torch.manual_seed(int(gold["seed"]))
    out = metrics.match_catalogs(*dev_args(gold), 32, TOL, TOL, torch.from_numpy(gold["mag_bins"]))
    assert len(out) == 4
    lex = gold["ref_is_lex"]
    for k, name in enumerate(NAMES):
        o = out[k].cpu().numpy()
        np.testing.assert_array_equal(o, small[0][k], err_msg=name)
        np.testing.assert_array_equal(o[lex], gold[f"ref_{name}"][lex], err_msg=name)


def test_bin2_equals_reference_and_oracle(gold):
    got = check_against_oracle(gold, gold["mag_bins2"], index=gold["index2"])
    assert got[0].shape == (24, 8, 2)
    lex = gold["ref_is_lex2"]
    for k, name in enumerate(NAMES):
        np.testing.assert_array_equal(got[k][lex], gold[f"ref2_{name}"][lex], err_msg=name)
    np.testing.assert_array_equal(got[0], gold["ref2_true_total"])
    np.testing.assert_array_equal(got[2], gold["ref2_est_total"])
    np.testing.assert_array_equal(got[1].sum(-1), gold["ref2_true_matches"].sum(-1))
    np.testing.assert_array_equal(got[3].sum(-1), gold["ref2_est_matches"].sum(-1))


def test_all_catalogs_in_order(gold):
    every = run(gold, gold["mag_bins"])  # num_est_catalogs_to_match=None
    assert every[0].shape == (24, 64, 17)
    by_index = run(gold, gold["mag_bins"], index=np.tile(np.arange(64), (24, 1)))
    for a, b in zip(every, by_index):
        np.testing.assert_array_equal(a, b)
    # float counts, as the samplers hold them, are cast like the reference's .int()
    f = dict(gold)
    f["true_counts"] = gold["true_counts"].astype(np.float32)
    f["est_counts"] = gold["est_counts"].astype(np.float32)
    for a, b in zip(every, run(f, gold["mag_bins"])):
        np.testing.assert_array_equal(a, b)
    # the stored subsample is a gather of the full result
    sub = run(gold, gold["mag_bins"], index=gold["index"])
    t = np.arange(24)[:, None]
    for a, b in zip(every, sub):
        np.testing.assert_array_equal(a[t, gold["index"]], b)


def test_same_call_twice_is_identical(gold):
    a = run(gold, gold["mag_bins"], index=gold["index"])
    b = run(gold, gold["mag_bins"], index=gold["index"])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_rectangular_and_empty_sides():
    """St != Se with cycling counts: n = 0, m = 0, n > m and n < m (the
    transposed side) all occur."""
    case = O.synth_case(11, 14, 12, 6, 9, 8.0, TOL, TOL, [BINS], p_empty=0.15)
    n = case["true_counts"][:, None]
    m = case["est_counts"]
    assert (n == 0).any() and (m == 0).any() and ((n > 0) & (m == 0)).any()
    assert ((n > m) & (m > 0)).any() and ((n < m) & (n > 0)).any()
    check_against_oracle(case, BINS)
    # and with more true than est slots
    case = O.synth_case(12, 10, 6, 9, 4, 8.0, TOL, TOL, [BINS])
    assert (case["true_counts"][:, None] > case["est_counts"]).any()
    check_against_oracle(case, BINS)


def test_one_by_one():
    case = O.synth_case(13, 4, 6, 1, 1, 2.0, TOL, TOL, [BINS], p_empty=0.2)
    got = check_against_oracle(case, BINS)
    assert (got[4] == 0).any() and (got[4] == -1).any()


@pytest.mark.parametrize("S", [33, 64])
def test_full_catalogs(S):
    """Full counts on a 16x16 frame: dense enough for long reassignment chains."""
    case = O.synth_case(20 + S, 4, 16, S, S, 16.0, TOL, TOL, [BINS], counts="full", fill=True)
    assert (case["true_counts"] == S).all() and (case["est_counts"] == S).all()
    got = check_against_oracle(case, BINS)
    assert got[1].sum() > 0.5 * 4 * 16 * S * 0.8  # most kept true sources are matched


def one_problem(true_xy, true_mag, est_xy, est_mag):
    n, m = len(true_xy), len(est_xy)
    return dict(true_counts=np.array([n], np.int32),
                true_locs=np.asarray(true_xy, np.float32).reshape(1, n, 2),
                true_fluxes=O.flux_of(np.asarray(true_mag, np.float64)).astype(np.float32)[None],
                est_counts=np.array([[m]], np.int32),
                est_locs=np.asarray(est_xy, np.float32).reshape(1, 1, m, 2),
                est_fluxes=O.flux_of(np.asarray(est_mag, np.float64)).astype(np.float32)[None, None])


@pytest.mark.parametrize("perm", [(0, 1, 2), (2, 0, 1), (1, 2, 0)])
def test_reassignment_chain_where_greedy_is_wrong(perm):
    """True A, B, C on a line, est a, b, c: the nearest pairs are B-a and C-b
    (0.05 px each), which strand A; the only 3-matching is A-a, B-b, C-c."""
    true_xy = [(0.0, 1.0), (0.4, 1.0), (0.8, 1.0)]
    est_xy = [(0.35, 1.0), (0.75, 1.0), (1.25, 1.0)]
    case = one_problem(true_xy, [19.2] * 3, [est_xy[k] for k in perm], [19.2] * 3)
    got = check_against_oracle(case, BINS)
    np.testing.assert_array_equal(got[4][0, 0], np.argsort(perm))
    assert got[1].sum() == 3 and got[3].sum() == 3


def test_all_out_of_tolerance():
    true_xy = [(1.0, 1.0), (3.0, 3.0), (5.0, 2.0)]
    far = one_problem(true_xy, [18.2, 19.2, 20.2], [(x + 2.0, y) for x, y in true_xy] + [(7., 7.)],
                      [18.2, 19.2, 20.2, 20.7])
    got = check_against_oracle(far, BINS)
    assert got[1].sum() == 0 and got[3].sum() == 0 and got[0].sum() == 3 and got[2].sum() == 4
    assert (got[4] == -1).all()
    # on the spot but a magnitude apart
    dim = one_problem(true_xy, [18.2, 19.2, 20.2], true_xy, [19.2, 20.2, 21.2])
    got = check_against_oracle(dim, BINS)
    assert got[1].sum() == 0 and (got[4] == -1).all()


def test_partial_workgroup_and_single_tile(gold):
    one = {k: gold[k][3:4] for k in INPUTS}  # T = 1, true count 3
    idx = np.array([[5, 0, 63, 17, 5]])      # M = 5: one full workgroup of problems and a part
    got = check_against_oracle(one, BINS, index=idx)
    assert got[0].shape == (1, 5, 17)
    for g in got:
        np.testing.assert_array_equal(g[0, 0], g[0, 4])  # the repeated catalog


def test_bad_sources_match_nothing():
    """Inside the counted slots: a NaN location, a zero, a negative and an
    infinite flux are out of tolerance with everything; they are binned by
    torch.bucketize's rule (NaN and +inf magnitudes fall in no bin)."""
    true_xy = [(1.0, 1.0), (3.0, 3.0), (5.0, 2.0), (6.0, 6.0)]
    case = one_problem(true_xy, [18.2, 19.2, 20.2, 17.2], true_xy, [18.2, 19.2, 20.2, 17.2])
    case["est_locs"][0, 0, 0, 1] = np.nan
    case["est_fluxes"][0, 0, 1] = 0.0
    case["est_fluxes"][0, 0, 2] = -1.0
    case["true_fluxes"][0, 3] = np.inf
    got = check_against_oracle(case, BINS)
    assert (got[4] == -1).all() and got[1].sum() == 0
    assert got[2].sum() == 2  # est 0 (finite magnitude) and est 3 are binned
    assert got[0].sum() == 4 and got[0][0, 0, 0] == 1  # flux +inf: magnitude -inf, first bin


def test_precision_recall_f1_on_device(gold):
    for prefix, ins in (("prf", [gold[f"ref_{n}"] for n in NAMES]),
                        ("prf0", [gold[f"prf0_in_{n}"] for n in NAMES])):
        got = metrics.compute_precision_recall_f1(*[torch.from_numpy(x).cuda() for x in ins])
        for g, name in zip(got, ("precision", "recall", "f1")):
            assert g.is_cuda
            np.testing.assert_array_equal(g.cpu().numpy(), gold[f"{prefix}_{name}"])
