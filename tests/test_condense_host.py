"""smcdet_amd.condense without a GPU: the CPU oracle (tests/_condense_oracle.py)
against hand-worked maps and a synthetic posterior with planted presence
counts, the argument validation of the three entry points (no kernel is
launched: every call fails on a null pointer or an unsupported shape) and the
Python wrappers' refusals."""
import os

import numpy as np
import pytest
import torch

from smcdet_amd import _hip, condense
from tests import _condense_oracle as O

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "smcdet_hip.h")


@pytest.mark.parametrize("case", O.PEAK_CASES, ids=[c["name"] for c in O.PEAK_CASES])
def test_oracle_peaks_on_hand_worked_maps(case):
    n, cell, mass, locs = O.peaks(case["map"], case["q"], case["p"], case["min_mass"], case["K"])
    assert n == len(case["cells"])
    assert cell[:n].tolist() == case["cells"] and (cell[n:] == -1).all()
    assert mass[:n].tolist() == case["mass"] and (mass[n:] == 0).all()
    np.testing.assert_allclose(locs[:n].reshape(-1, 2), np.asarray(case["centroid"]).reshape(-1, 2),
                               rtol=0, atol=1e-12)
    assert np.isnan(locs[n:]).all()


def test_oracle_peaks_in_pixels():
    """lo + centroid / c: the corner case at 4 cells per pixel in a box at (-2, 3)."""
    case = O.PEAK_CASES[2]
    _, _, _, locs = O.peaks(case["map"], 1, 2, 1.0, 4, lo=(-2.0, 3.0), c=4)
    np.testing.assert_allclose(locs[0], [-2.0 + 5.0 / 24.0, 3.0 + 4.0 / 24.0], atol=1e-12)


def test_oracle_smooth_and_quantiles():
    m = np.arange(12.0).reshape(3, 4)
    s = O.smooth(m, 1)
    assert s[0, 0] == 0 + 1 + 4 + 5 and s[1, 1] == m[0:3, 0:3].sum() and s[2, 3] == 6 + 7 + 10 + 11
    np.testing.assert_array_equal(O.smooth(m, 0), m)
    # fluxes 1..4 present, one catalog unmatched: cumulative weights 1, 2, 3, 4
    mf = np.array([3.0, np.nan, 1.0, 4.0, 2.0], np.float32).reshape(1, 5, 1)
    q = O.flux_quantiles(mf, (0.0, 0.25, 0.26, 0.5, 0.95, 1.0))
    assert q[0, 0].tolist() == [1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    w = np.array([[1.0, 5.0, 1.0, 1.0, 5.0]], np.float32)  # flux 2 weighs 5 of 8
    q = O.flux_quantiles(mf, (0.125, 0.5, 0.76), w)
    assert q[0, 0].tolist() == [1.0, 2.0, 3.0]
    assert np.isnan(O.flux_quantiles(np.full((1, 3, 2), np.nan, np.float32), (0.5,))).all()


def test_oracle_counted_rule_and_cell_index():
    locs = np.array([[[[0.1, 0.1], [np.nan, 1.0], [1.0, 1.0], [9.0, 9.0]],
                      [[0.3, 0.6], [0.3, 0.6], [0.3, 0.6], [0.3, 0.6]],
                      [[-0.1, 0.2], [0.2, 0.2], [0.2, 0.2], [0.2, 0.2]]]], np.float32)
    fluxes = np.array([[[1.0, 1.0, 0.0, 1.0], [2.0, -1.0, np.inf, 4.0], [1.0, 1.0, 1.0, 1.0]]],
                      np.float32)
    counts = np.array([[3, 9, -1]])  # the first three slots; clamped to 4; clamped to 0
    ok = O.counted_mask(counts, locs, fluxes)
    assert ok[0].tolist() == [[True, False, False, False], [True, False, False, True],
                              [False] * 4]
    sm = O.source_map(counts, locs, fluxes, np.zeros((1, 2)), 2, 2, 2)
    assert sm["count"][0].tolist() == [[1.0, 2.0], [0.0, 0.0]]  # (0,0); (0,1) twice
    assert sm["flux"][0].tolist() == [[1.0, 6.0], [0.0, 0.0]]
    assert sm["outside"][0] == 0 and sm["n_counted"][0] == 3
    sm = O.source_map(counts, locs, fluxes, np.zeros((1, 2)), 2, 1, 1)  # a 1x1 grid
    assert sm["count"][0, 0, 0] == 1 and sm["outside"][0] == 2


@pytest.fixture(scope="module")
def planted():
    counts, locs, fluxes, star_locs, star_flux, presence = O.planted_posterior(seed=0)
    return dict(counts=counts, locs=locs, fluxes=fluxes, star_locs=star_locs,
                star_flux=star_flux, presence=presence,
                out=O.condense(counts, locs, fluxes, (-2.0, -2.0, 10.0, 10.0)))


def seed_of_star(out, star_locs):
    """[T,3] the seed nearest to each star and its distance."""
    d = np.linalg.norm(out["seed_locs"][:, None, :3].astype(np.float64) - star_locs[:, :, None],
                       axis=-1)
    return d.argmin(-1), d.min(-1)


def test_oracle_recovers_planted_posterior(planted):
    out = planted["out"]
    N = planted["counts"].shape[1]
    assert out["n_seeds"].tolist() == [3, 3, 3, 3]
    assert planted["out"]["margins_ok"].all()  # no association rests on a rounding
    k, dist = seed_of_star(out, planted["star_locs"])
    assert (np.sort(k, -1) == np.arange(3)).all()
    # a seed is the centroid of >= 100 draws of sd 0.1 px around the star
    assert dist.max() < 0.1
    t = np.arange(4)[:, None]
    np.testing.assert_array_equal(out["prob"][t, k].astype(np.float64) * N, planted["presence"])
    assert (planted["presence"][:, 0] == N).all()
    np.testing.assert_allclose(out["locs"][t, k], planted["star_locs"], atol=0.05)
    np.testing.assert_allclose(out["fluxes"][t, k], planted["star_flux"], rtol=0.02)
    assert (out["prob"][:, 3:] == 0).all() and np.isnan(out["locs"][:, 3:]).all()
    # the spurious sources (about 0.1 per catalog) are all that is unassociated
    spurious = planted["counts"].sum(1) - planted["presence"].sum(1)
    np.testing.assert_allclose(out["unassociated"], spurious / N, rtol=1e-6)
    np.testing.assert_allclose(out["expected_count"], planted["presence"].sum(1) / N, rtol=1e-6)
    q = out["flux_quantiles"][t, k]
    assert (q[..., 0] < q[..., 1]).all() and (q[..., 1] < q[..., 2]).all()
    np.testing.assert_allclose(q[..., 1], planted["star_flux"], rtol=0.03)


def test_map_case_covers_what_it_claims():
    counts, locs, fluxes = O.map_case()
    S = fluxes.shape[-1]
    assert set(counts[0].tolist()) >= set(range(S + 1)) | {-1, S + 2}
    ok = O.counted_mask(counts, locs, fluxes)
    inside = np.arange(S)[None, None] < np.clip(counts, 0, S)[..., None]
    assert (inside & ~ok).sum() >= 6  # counted slots holding NaN / inf / flux <= 0
    # padding is NaN; the catalog whose count is -1 still holds its source
    assert np.isnan(locs[~inside & (counts >= 0)[..., None]]).all()
    assert np.isfinite(locs[counts == -1][:, 0]).all()
    sm = O.source_map(counts, locs, fluxes, np.full((3, 2), -2.0), 4, 48, 40)
    assert (sm["outside"] > 0).all() and (sm["count"].sum((1, 2)) > 100).all()
    assert (sm["count"].sum((1, 2)) + sm["outside"] == sm["n_counted"]).all()


# ---- the C ABI: every argument validated before any device work -------------------
def _map(T=1, N=4, S=3, c=4, Gh=8, Gw=8, p=None):
    return _hip.lib().smcdet_source_map(p, p, p, None, p, None, T, N, S, c, Gh, Gw, p, None, p,
                                        None)


def _peaks(T=1, Gh=8, Gw=8, c=4, q=1, nms=2, K=4, p=None):
    return _hip.lib().smcdet_map_peaks(p, p, None, T, Gh, Gw, c, q, nms, p, K, p, p, p, p, None)


def _moments(T=1, N=4, S=3, K=4, p=None):
    return _hip.lib().smcdet_seed_moments(p, p, p, None, p, T, N, S, K, p, None, None)


@pytest.mark.parametrize("call", [_map, _peaks, _moments])
def test_abi_null_pointer_is_einval(call):
    assert call() == -1
    assert "null" in _hip.lib().smcdet_last_error().decode()


@pytest.mark.parametrize("call,kw", [
    (_map, dict(c=9)), (_map, dict(c=0)), (_map, dict(Gh=2049)), (_map, dict(Gw=2049)),
    (_peaks, dict(K=65)), (_peaks, dict(c=9)), (_peaks, dict(Gh=256, Gw=129)),
    (_peaks, dict(q=9)), (_peaks, dict(nms=17)), (_moments, dict(K=65)), (_moments, dict(S=65))])
def test_abi_limits_are_eunsupported(call, kw):
    assert call(**kw) == -2
    assert _hip.lib().smcdet_last_error().decode()


def test_abi_peaks_limit_names_the_remedy():
    assert _peaks(Gh=182, Gw=182) == -2
    assert "cells_per_pixel" in _hip.lib().smcdet_last_error().decode()
    assert _peaks(Gh=128, Gw=256) == -1  # exactly 32768 cells pass on to the null check


@pytest.mark.parametrize("call,kw", [
    (_map, dict(T=0)), (_map, dict(N=0)), (_map, dict(S=0)), (_map, dict(Gh=0)),
    (_peaks, dict(T=0)), (_peaks, dict(K=0)), (_peaks, dict(Gw=0)),
    (_moments, dict(T=0)), (_moments, dict(N=0)), (_moments, dict(K=0))])
def test_abi_sizes_are_einval(call, kw):
    assert call(**kw) == -1


def test_abi_constants_mirrored():
    hdr = open(HEADER).read()
    for name, value in (("MAP_MAX_CELLS_PER_PIXEL", 8), ("MAP_MAX_GRID", 2048),
                        ("PEAKS_MAX_CELLS", 32768), ("PEAKS_MAX_SMOOTH", 8),
                        ("PEAKS_MAX_NMS", 16), ("SEED_MOMENTS", 10)):
        assert getattr(_hip, name) == value
        assert f"#define SMCDET_{name} {value}" in hdr
    assert "#define SMCDET_ABI_VERSION 20" in hdr and _hip.ABI_VERSION == 20
    for name in ("smcdet_source_map", "smcdet_map_peaks", "smcdet_seed_moments"):
        assert name in _hip.EXPORTS and name in _hip._OUTS


# ---- the Python layer ------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors():
    counts, locs, fluxes = [torch.from_numpy(x) for x in O.map_case(T=1, N=8)]
    box = (-2.0, -2.0, 10.0, 8.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        condense.source_map(counts, locs, fluxes, box=box)
    with pytest.raises(RuntimeError, match="HIP device"):
        condense.condense(counts, locs, fluxes, box=box)
    smap = condense.SourceMap(torch.zeros(1, 8, 8), None, torch.zeros(1), (0.0, 0.0, 2.0, 2.0), 4,
                              total_weight=torch.ones(1))
    with pytest.raises(RuntimeError, match="HIP device"):
        condense.find_seeds(smap)
    with pytest.raises(RuntimeError, match="HIP device"):
        condense.seed_moments(torch.zeros(1, 8, 4, dtype=torch.int32), locs, fluxes,
                              torch.zeros(1, 4, 2))


def test_derive_matches_oracle_on_cpu():
    """The derived fields are plain torch: the same float64 formulas as the oracle."""
    rng = np.random.default_rng(1)
    x = rng.normal(0.1, 0.2, (2, 3, 50, 2))
    f = rng.uniform(1, 30, (2, 3, 50))
    mag = 22.5 - 2.5 * np.log10(f)
    mom = np.stack([np.full((2, 3), 50.0), x[..., 0].sum(-1), x[..., 1].sum(-1),
                    (x[..., 0] ** 2).sum(-1), (x[..., 1] ** 2).sum(-1),
                    (x[..., 0] * x[..., 1]).sum(-1), f.sum(-1), (f * f).sum(-1), mag.sum(-1),
                    (mag * mag).sum(-1)], -1)
    mom[1, 2] = 0.0  # a seed nothing matched
    total = np.array([64.0, 50.0])
    want = O.derive(mom, total)
    got = condense.derive(torch.from_numpy(mom), torch.from_numpy(total))
    for k, v in want.items():
        np.testing.assert_allclose(got[k].numpy(), v, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    np.testing.assert_allclose(want["sd_h"][0, 0], x[0, 0, :, 0].std(), rtol=1e-9)
    np.testing.assert_allclose(want["cov_hw"][0, 1], np.cov(x[0, 1].T, bias=True)[0, 1], rtol=1e-9)
    assert want["prob"][0, 0] == 50.0 / 64.0 and np.isnan(want["flux"][1, 2])


def test_flux_quantiles_match_oracle_on_cpu():
    rng = np.random.default_rng(2)
    mf = rng.uniform(1, 30, (2, 40, 3)).astype(np.float32)
    mf[rng.uniform(size=mf.shape) < 0.4] = np.nan
    mf[1, :, 2] = np.nan
    mf[0, 3, 0] = mf[0, 4, 0]  # a tie
    w = (rng.integers(1, 2048, (2, 40)) / 1024.0).astype(np.float32)
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    for weights in (None, w):
        got = condense.flux_quantiles(torch.from_numpy(mf), qs,
                                      None if weights is None else torch.from_numpy(weights))
        np.testing.assert_array_equal(got.numpy(), O.flux_quantiles(mf, qs, weights))
