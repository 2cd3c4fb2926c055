"""smcdet_amd.metrics without a GPU: the CPU oracle against the reference's
recorded outputs (tests/golden/metrics.npz, written by
tests/golden/make_metrics_golden.py), the pure-torch helpers, the drop-in alias
and the argument validation of smcdet_match_catalogs.  No kernel launches:
every ABI call here fails on a null pointer or an unsupported shape."""
import os

import numpy as np
import pytest
import torch

from smcdet_amd import _hip, metrics
from tests import _metrics_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
NAMES = ("true_total", "true_matches", "est_total", "est_matches")
INPUTS = ("true_counts", "true_locs", "true_fluxes", "est_counts", "est_locs", "est_fluxes")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def oracle_small(gold):
    return O.match_catalogs(*[gold[k] for k in INPUTS], gold["index"], float(gold["locs_tol"]),
                            float(gold["mags_tol"]), gold["mag_bins"])


def test_fixture_shapes(gold):
    assert gold["ref_true_total"].shape == (24, 32, 17)
    assert gold["est_locs"].shape == (24, 64, 10, 2)
    assert sorted(set(gold["true_counts"].tolist())) == list(range(11))
    assert (gold["est_counts"] == 0).any()
    assert np.isnan(gold["est_fluxes"]).any()  # NaN padding


def test_oracle_totals_equal_reference(gold, oracle_small):
    np.testing.assert_array_equal(oracle_small[0], gold["ref_true_total"])
    np.testing.assert_array_equal(oracle_small[2], gold["ref_est_total"])


def test_oracle_cardinality_equals_reference(gold, oracle_small):
    # the bins cover every magnitude of the fixture, so the sums over bins are
    # the numbers of matches
    assert np.array_equal(gold["ref_true_total"].sum(-1),
                          np.clip(gold["true_counts"], 0, 10)[:, None].repeat(32, 1))
    np.testing.assert_array_equal(oracle_small[1].sum(-1), gold["ref_true_matches"].sum(-1))
    np.testing.assert_array_equal(oracle_small[3].sum(-1), gold["ref_est_matches"].sum(-1))
    np.testing.assert_array_equal(oracle_small[1].sum(-1), oracle_small[3].sum(-1))
    np.testing.assert_array_equal((oracle_small[4] >= 0).sum(-1), oracle_small[1].sum(-1))


def test_oracle_equals_reference_where_reference_is_lexicographic(gold, oracle_small):
    lex = gold["ref_is_lex"]
    for k, name in enumerate(NAMES):
        np.testing.assert_array_equal(oracle_small[k][lex], gold[f"ref_{name}"][lex])
    # the recorded flag is what the oracle says today
    same = np.logical_and.reduce([(oracle_small[k] == gold[f"ref_{n}"]).all(-1)
                                  for k, n in enumerate(NAMES)])
    np.testing.assert_array_equal(same, lex)
    assert 1.0 - lex.mean() <= 0.02


def test_oracle_bin2_equals_reference(gold):
    ora = O.match_catalogs(*[gold[k] for k in INPUTS], gold["index2"], float(gold["locs_tol"]),
                           float(gold["mags_tol"]), gold["mag_bins2"])
    lex = gold["ref_is_lex2"]
    assert ora[0].shape == (24, 8, 2)
    np.testing.assert_array_equal(ora[0], gold["ref2_true_total"])
    np.testing.assert_array_equal(ora[2], gold["ref2_est_total"])
    np.testing.assert_array_equal(ora[1].sum(-1), gold["ref2_true_matches"].sum(-1))
    np.testing.assert_array_equal(ora[3].sum(-1), gold["ref2_est_matches"].sum(-1))
    for k, name in enumerate(NAMES):
        np.testing.assert_array_equal(ora[k][lex], gold[f"ref2_{name}"][lex])


def test_oracle_is_brute_force_on_tiny_problems():
    """All assignments enumerated: most in-tolerance pairs, then least distance."""
    import itertools
    rng = np.random.default_rng(5)
    for _ in range(60):
        n, m = map(int, rng.integers(1, 5, 2))
        dist = rng.uniform(0, 1.0, (n, m))
        oob = dist > 0.5
        q = O.solve(dist, oob, 0.5)
        best = None
        small, big = (n, m) if n <= m else (m, n)
        for perm in itertools.permutations(range(big), small):
            pairs = [(i, perm[i]) if n <= m else (perm[i], i) for i in range(small)]
            good = [(i, j) for i, j in pairs if not oob[i, j]]
            key = (-len(good), sum(dist[i, j] for i, j in good))
            if best is None or key < best[0]:
                best = (key, good)
        want = np.full(n, -1, np.int32)
        for i, j in best[1]:
            want[i] = j
        np.testing.assert_array_equal(q, want)


def test_precision_recall_f1_bit_for_bit(gold):
    for prefix, ins in (("prf", [gold[f"ref_{n}"] for n in NAMES]),
                        ("prf0", [gold[f"prf0_in_{n}"] for n in NAMES])):
        got = metrics.compute_precision_recall_f1(*[torch.from_numpy(x) for x in ins])
        for g, name in zip(got, ("precision", "recall", "f1")):
            assert g.dtype == torch.float32
            np.testing.assert_array_equal(g.numpy(), gold[f"{prefix}_{name}"])
    zb = int(gold["prf_zero_bin"])
    assert (gold["prf0_precision"][..., zb] == 0).all() and (gold["prf0_f1"][..., zb] == 0).all()


def test_converters_bit_for_bit(gold):
    nmgy = metrics.convert_mag_to_nmgy(torch.from_numpy(gold["conv_mags"]))
    np.testing.assert_array_equal(nmgy.numpy(), gold["conv_nmgy"])
    back = metrics.convert_nmgy_to_mag(torch.from_numpy(gold["conv_nmgy"]))
    np.testing.assert_array_equal(back.numpy(), gold["conv_mags_back"])


def test_dropin_alias_resolves_metrics():
    import smcdet_amd
    smcdet_amd.install_as_smcdet()
    from smcdet.metrics import compute_precision_recall_f1, match_catalogs
    assert match_catalogs is metrics.match_catalogs
    assert compute_precision_recall_f1 is metrics.compute_precision_recall_f1


def _call(T=1, N=4, M=4, St=4, Se=4, B=4, locs_tol=0.5, mags_tol=0.5):
    """smcdet_match_catalogs with every pointer null: whatever the shapes, it
    must return before any device work."""
    none = [None] * 7
    return _hip.lib().smcdet_match_catalogs(*none, T, N, M, St, Se, locs_tol, mags_tol, None, B,
                                            None, None, None, None, None, None)


def test_abi_limits_mirrored():
    assert _hip.MATCH_MAX_SOURCES == 64 and _hip.MATCH_MAX_BINS == 64
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "..", "include", "smcdet_hip.h")).read()
    assert "#define SMCDET_MATCH_MAX_SOURCES 64" in hdr
    assert "#define SMCDET_MATCH_MAX_BINS 64" in hdr


def test_abi_null_pointer_is_einval():
    assert _call() == -1
    assert "null" in _hip.lib().smcdet_last_error().decode()


@pytest.mark.parametrize("kw", [dict(St=65), dict(Se=65), dict(B=65)])
def test_abi_limits_are_eunsupported(kw):
    assert _call(**kw) == -2
    assert _hip.lib().smcdet_last_error().decode()


def test_abi_null_index_needs_all_catalogs():
    assert _call(N=8, M=4) == -1
    assert "index" in _hip.lib().smcdet_last_error().decode()


@pytest.mark.parametrize("kw", [dict(T=0), dict(N=0), dict(M=0), dict(locs_tol=0.0),
                                dict(mags_tol=-1.0)])
def test_abi_sizes_and_tolerances_are_einval(kw):
    assert _call(**kw) == -1


def test_match_catalogs_refuses_cpu_tensors(gold):
    args = [torch.from_numpy(gold[k]) for k in INPUTS]
    with pytest.raises(RuntimeError, match="HIP device"):
        metrics.match_catalogs(*args, 32, 0.5, 0.5, torch.from_numpy(gold["mag_bins"]))
