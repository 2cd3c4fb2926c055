"""tests/_extract_oracle.py pinned on hand-worked cases, so that the GPU tests
(tests/test_gpu_extract.py), which compare the kernel with this oracle, are
not circular.  The same cases (tests/_extract_cases.py) run on the device
there."""
import math

import numpy as np
import pytest

from tests import _extract_oracle as O
from tests._extract_cases import CASES, plateau_image


def run(name):
    image, kw = CASES[name]
    return O.extract_one(image, 0.0, 1.0, **kw)


def test_ladder_is_exact_float32():
    taus = O.ladder(16, 1, 4)
    assert [float(t) for t in taus] == [1, 2, 4, 8] and all(t.dtype == np.float32 for t in taus)
    # op by op: r = p / tau, five square roots, successive products
    p, tau = np.float32(37.25), np.float32(1.7)
    q = p / tau
    for _ in range(5):
        q = np.sqrt(q)
    want = [tau]
    for _ in range(31):
        want.append(want[-1] * q)
    got = O.ladder(p, tau, 32)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert got[-1] < p


def test_diagonal_connectivity_and_minarea():
    r = run("diag_minarea3")
    assert r.count == r.n_found == 1
    assert r.fluxes[0] == 30 and tuple(r.locs[0]) == (1.5, 1.5)
    assert np.isnan(r.locs[1:]).all() and (r.fluxes[1:] == 0).all()
    want = np.zeros((5, 7), np.int32)
    want[0, 0] = want[1, 1] = want[2, 2] = 1
    np.testing.assert_array_equal(r.segmap, want)

    r = run("diag_minarea1")
    assert r.count == 2 and list(r.fluxes[:2]) == [30, 10]
    assert tuple(r.locs[1]) == (4.5, 6.5) and r.segmap[4, 6] == 2

    r = run("diag_minarea4")
    assert r.count == r.n_found == 0 and not r.segmap.any()
    assert np.isnan(r.locs).all() and not r.fluxes.any()


def test_cap_keeps_the_brightest_and_counts_all():
    r = run("diag_K1")
    assert r.count == 1 and r.n_found == 2 and r.fluxes.shape == (1,) and r.fluxes[0] == 30
    assert r.segmap[4, 6] == 2  # ranks above K stay in the map


def test_ridge_deblends_and_gathers_with_the_tie_rule():
    r = run("ridge_split")
    assert r.count == 2 and list(r.fluxes[:2]) == [34, 32]
    # the `2` pixel is reached in the second sweep, from both sides at v = 8:
    # the tie goes to the lower-numbered leaf
    np.testing.assert_array_equal(r.segmap[1], [0, 1, 1, 1, 1, 2, 2, 2, 0])
    assert r.locs[0, 0] == 1.5 and r.locs[0, 1] == np.float32(89 / 34)
    assert tuple(r.locs[1]) == (1.5, 6.5)
    # the comparisons met: 26, 20 and 8 against 0.005 * 66
    assert r.sig_margin == pytest.approx((8 - 0.33) / 8, rel=1e-6)

    for name in ("ridge_whole", "ridge_n1"):
        r = run(name)
        assert r.count == 1 and r.fluxes[0] == 66
        np.testing.assert_array_equal(r.segmap[1], [0, 1, 1, 1, 1, 1, 1, 1, 0])
    assert run("ridge_whole").sig_margin == pytest.approx((33 - 26) / 33, rel=1e-6)
    assert run("ridge_n1").sig_margin == np.inf  # n = 1: nothing is compared


def test_plateau_nan_and_everything_above():
    r = run("plateau")
    assert r.count == 1 and r.fluxes[0] == 80 and tuple(r.locs[0]) == (3.0, 3.0)
    assert r.segmap.sum() == 16

    r = run("all_nan")
    assert r.count == 0 and not r.segmap.any()

    r = run("nan_speckled")  # 5 NaN 5 5 NaN 0.5: {2, 3} and {0}
    assert r.count == 2 and list(r.fluxes[:2]) == [10, 5]
    np.testing.assert_array_equal(r.segmap, [[2, 0, 1, 1, 0, 0]])
    assert tuple(r.locs[0]) == (0.5, 3.0) and tuple(r.locs[1]) == (0.5, 0.5)

    r = run("all_above")
    assert r.count == 1 and r.fluxes[0] == 48 and tuple(r.locs[0]) == (2.0, 2.0)
    assert (r.segmap == 1).all()


def test_non_positive_or_non_finite_tau_detects_nothing():
    for thresh, sigma in ((0.0, 1.0), (-1.0, 1.0), (np.inf, 1.0), (np.nan, 1.0), (1.0, 0.0)):
        r = O.extract_one(plateau_image(), 0.0, sigma, thresh, minarea=1)
        assert r.count == r.n_found == 0 and not r.segmap.any()


def test_clean_rule_by_hand():
    """A 3x3 block of 1000 (object j) and one pixel four columns to the right
    of its centre (object i), tau = 1, beta = 1, minarea = 1.
    j: F = 9000, moments hh = ww = 2/3, hw = 0 (no 1/12: 4/9 > 1/144), a_j =
    sqrt(2/3), c_hh = c_ww = 3/2, c_hw = 0, amp = 9000 / (200 pi) = 14.3239.
    i: one pixel: hh = ww = 0 -> 1/12 each, a_i = sqrt(1/12); dh = 0, dw = 4.
    16 < 100 (a_i + a_j)^2 = 122.1; alpha = (amp - 1) 100 pi / 9 = 465.09;
    val = 1 + alpha * 1.5 * 16 = 11163.2; amp / val = 1.28314e-3, against
    mthresh_i = v_i - 1: absorbed at v_i = 1.001, kept at 1.002."""
    amp = 9000 / (200 * math.pi)
    alpha = (amp - 1) * 100 * math.pi / 9
    val = 1 + alpha * 1.5 * 16
    assert amp == pytest.approx(14.3239, rel=1e-5) and alpha == pytest.approx(465.09, rel=1e-5)
    assert val == pytest.approx(11163.2, rel=1e-5) and amp / val == pytest.approx(1.28314e-3,
                                                                                 rel=1e-5)
    assert 16 < 100 * (math.sqrt(2 / 3) + math.sqrt(1 / 12)) ** 2 == pytest.approx(122.14, rel=1e-4)
    lo, hi = float(np.float32(1.001)) - 1, float(np.float32(1.002)) - 1
    assert lo < amp / val < hi

    r = run("clean_absorb")
    assert r.count == r.n_found == 1
    F = 9000 + float(np.float32(1.001))
    assert r.flux64[0] == pytest.approx(F, rel=1e-15)
    assert r.locs64[0, 0] == pytest.approx(2.5, rel=1e-15)
    assert r.locs64[0, 1] == pytest.approx((9000 * 2.5 + float(np.float32(1.001)) * 6.5) / F,
                                           rel=1e-15)
    assert r.segmap[2, 6] == 1 and r.segmap.astype(bool).sum() == 10
    assert r.clean_margin == pytest.approx((amp / val - lo) / (amp / val), rel=1e-6)

    r = run("clean_keep")
    assert r.count == 2 and r.fluxes[0] == 9000 and r.fluxes[1] == np.float32(1.002)
    assert r.segmap[2, 6] == 2

    r = run("clean_off")  # beta = 0: the rule is skipped
    assert r.count == 2 and r.clean_margin > 0.9


def test_faint_absorber_never_cleans():
    # diag_minarea1 runs with beta = 1: amp = 30 / (200 pi) < tau stops the rule
    r = run("diag_minarea1")
    assert r.count == 2 and r.clean_margin < 1


def test_grid_order_and_stacking():
    s = O.settings_grid([1.5, 3.0], [1, 5], [1e-4], [0.0, 10.0])
    assert s.shape == (8, 4)
    assert s[0].tolist() == [1.5, 1, 1e-4, 0.0] and s[1].tolist() == [1.5, 1, 1e-4, 10.0]
    assert s[2].tolist() == [1.5, 5, 1e-4, 0.0] and s[4].tolist() == [3.0, 1, 1e-4, 0.0]
    imgs = np.stack([plateau_image(), 2 * plateau_image()])
    g = O.extract_grid(imgs, 0.0, [1.0, 1.0], s, deblend_nthresh=4, K=3)
    assert g.counts.shape == (2, 8) and g.locs.shape == (2, 8, 3, 2) and g.fluxes.shape == (2, 8, 3)
    assert g.segmap.shape == (2, 8, 6, 6) and (g.counts == 1).all()
    assert (g.fluxes[0, :, 0] == 80).all() and (g.fluxes[1, :, 0] == 160).all()
