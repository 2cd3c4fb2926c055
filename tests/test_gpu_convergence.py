"""smcdet_amd.convergence on the GPU against the numpy float64 oracle
(tests/_convergence_oracle.py): `chain_stats` at the shapes where the kernel
changes path, the special rows, determinism and layouts, then `diagnose` and
`diagnose_sampler` against the oracle's composition.

Tolerances: n_pairs, stopped and the NaN pattern are exact
(test_convergence_host shows every case's deciding pairs are 20 bounds from 0);
mean, W, var_plus, rhat and the chain moments are float64 throughout and
differ by summation order (eps_f64); every rho_t carries one float32 rounding
per centered draw (eps_rho, about 2^-23), tau 4 K eps_rho, ess and mcse what
follows from tau's.  Each test prints the largest observed error next to its
bound."""
import numpy as np
import pytest
import torch

from smcdet_amd import convergence
from tests import _convergence_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def N(t):
    return None if t is None else t.detach().cpu().numpy()


def run(case, **kw):
    x = torch.from_numpy(case["x"]).to(DEV)
    s = convergence.chain_stats(x, split=case["split"], max_lag=case["max_lag"],
                                num_rho=case["num_rho"], chain_moments=True, **kw)
    return s, {k: N(getattr(s, k)) for k in ("mean", "W", "var_plus", "rhat", "tau", "ess", "mcse",
                                             "n_pairs", "stopped", "chain_mean", "chain_var",
                                             "rho")}


def bounds(e):
    """Per-row absolute bounds of every float output."""
    f64, tau, dt = e["eps_f64"], e["tau"], O.tau_bound(e)
    rel_tau = dt / (tau - dt)
    return dict(mean=f64 * e["xmax"], W=f64 * e["W"], var_plus=f64 * e["var_plus"],
                rhat=f64 * e["rhat"], tau=dt, ess=e["ess"] * rel_tau,
                mcse=e["mcse"] * (rel_tau + f64),
                chain_mean=(f64 * e["xmax"])[:, None] + 0 * e["chain_mean"],
                chain_var=f64[:, None] * (e["chain_var"] + e["W"][:, None]),
                rho=e["eps_rho"][:, None] + O.U32 * np.abs(e["rho"]))


def check_against_oracle(got, e, label):
    """Exact integers and NaN pattern; floats within their bound on the rows
    the oracle calls ordinary, and the kept moments of the W == 0 rows."""
    np.testing.assert_array_equal(got["n_pairs"], e["n_pairs"], err_msg=label)
    np.testing.assert_array_equal(got["stopped"], e["stopped"], err_msg=label)
    live = ~np.isnan(e["rhat"])
    b = bounds(e)
    worst = {}
    for k, bound in b.items():
        g, w = got[k], e[k]
        if g is None or g.size == 0:
            continue
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{label} {k} NaN pattern")
        err = np.abs(g.astype(np.float64) - w)[live]
        fin = np.isfinite(err)
        ratio = err[fin] / bound[live][fin]
        worst[k] = (float(err[fin].max(initial=0.0)), float(ratio.max(initial=0.0)))
        assert (ratio <= 1.0).all(), (label, k, err[fin].max(), bound[live][fin].min())
    dead = ~live & ~np.isnan(e["mean"])  # W == 0: mean, W, var_plus and the moments are kept
    if dead.any():
        assert (got["W"][dead] == 0).all() and (got["chain_var"][dead] == 0).all()
        for k in ("mean", "var_plus", "chain_mean"):
            np.testing.assert_allclose(got[k][dead], e[k][dead], rtol=1e-14, atol=0)
    print(f"{label}: " + ", ".join(f"{k} err {v[0]:.3g} ({v[1]:.3g} of its bound)"
                                   for k, v in worst.items()))
    return worst


# ---- chain_stats against the oracle ---------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in O.cases() if not n.startswith("special")))
def test_chain_stats_vs_oracle(name):
    case, e = O.cases()[name], O.expected(name)
    s, got = run(case)
    R = case["x"].shape[0]
    assert (s.m, s.n) == (e["m"], e["n"]) and tuple(s.rhat.shape) == (R,)
    assert tuple(s.chain_mean.shape) == (R, e["m"])
    if case["num_rho"]:
        assert tuple(s.rho.shape) == (R, case["num_rho"])
        assert (got["rho"][:, 0] == 1.0).all()
        assert np.isnan(got["rho"][:, e["n"]:]).all() and not np.isnan(got["rho"][:, :e["n"]]).any()
    else:
        assert s.rho is None
    check_against_oracle(got, e, name)
    looked_at = e["n_pairs"] + e["stopped"]  # pairs the rule formed, the refused one included
    want_blocks = np.maximum((looked_at + O.BLOCK_PAIRS - 1) // O.BLOCK_PAIRS, 1)
    np.testing.assert_array_equal(N(s.lag_blocks), want_blocks)


@pytest.mark.parametrize("name", ["special", "special_unsplit"])
def test_special_rows(name):
    case, e = O.cases()[name], O.expected(name)
    _, names = O.special_rows()
    s, got = run(case)
    check_against_oracle(got, e, name)
    for i, row in enumerate(names):
        dead = row in ("nan", "inf", "constant", "constant_chains_apart")
        for k in ("rhat", "tau", "ess", "mcse"):
            assert np.isnan(got[k][i]) == dead, (row, k)
        if dead:
            assert got["n_pairs"][i] == 0 and got["stopped"][i] == 0
            if case["num_rho"]:
                assert np.isnan(got["rho"][i]).all()
        if row in ("nan", "inf"):
            assert all(np.isnan(got[k][i]).all() for k in ("mean", "W", "var_plus", "chain_mean",
                                                           "chain_var"))
    i = names.index("one_constant_chain")
    assert np.isfinite(got["ess"][i]) and (got["chain_var"][i] == 0).sum() == (2 if case["split"]
                                                                                else 1)
    assert got["rhat"][names.index("different_means")] > 50
    assert got["mean"][names.index("constant")] == 2.5
    j = names.index("sticky")
    assert got["chain_mean"][j].min() >= 0 and got["chain_mean"][j].max() <= 4


def test_integer_and_float64_inputs_are_converted():
    x = O.cases()["special"]["x"][4:5]  # the sticky integer chain
    want = convergence.chain_stats(torch.from_numpy(x).to(DEV))
    for dtype in (torch.int64, torch.int32, torch.float64):
        got = convergence.chain_stats(torch.from_numpy(x).to(DEV, dtype))
        assert torch.equal(got.ess, want.ess) and torch.equal(got.rhat, want.rhat)


# ---- determinism and layouts ------------------------------------------------------------
@pytest.mark.parametrize("name", ["split_n1000_C3", "lds_limit_plus_chain"])
def test_two_calls_return_the_same_bits(name):
    case = O.cases()[name]
    a, _ = run(case)
    b, _ = run(case)
    for k in ("mean", "W", "var_plus", "rhat", "tau", "ess", "mcse", "n_pairs", "stopped",
              "chain_mean", "chain_var", "rho"):
        u, v = getattr(a, k), getattr(b, k)
        if u is None:
            assert v is None
            continue
        assert torch.equal(u.view(torch.int64 if u.dtype == torch.float64 else torch.int32),
                           v.view(torch.int64 if v.dtype == torch.float64 else torch.int32)), k


def test_leading_dimensions_and_views():
    x = torch.from_numpy(O.phi_rows(130, 3, 140)).to(DEV)             # [5,3,140]
    x = torch.stack([x, x.flip(0), 2 * x, x + 1]).reshape(2, 2, 5, 3, 140)
    flat = convergence.chain_stats(x.reshape(20, 3, 140), num_rho=8, chain_moments=True)
    lead = convergence.chain_stats(x, num_rho=8, chain_moments=True)
    assert tuple(lead.rhat.shape) == (2, 2, 5) and tuple(lead.rho.shape) == (2, 2, 5, 8)
    assert tuple(lead.chain_mean.shape) == (2, 2, 5, 6) and tuple(lead.n_pairs.shape) == (2, 2, 5)
    for k in ("mean", "rhat", "tau", "ess", "mcse", "n_pairs", "stopped", "rho", "chain_var"):
        assert torch.equal(getattr(lead, k).reshape(getattr(flat, k).shape), getattr(flat, k)), k
    # a non-contiguous view (draws strided, chains transposed) against its contiguous copy
    big = torch.from_numpy(O.phi_rows(131, 280, 3)).to(DEV)           # [5,280,3]
    view = big.transpose(1, 2)[:, :, ::2]                             # [5,3,140]
    assert not view.is_contiguous()
    a = convergence.chain_stats(view, num_rho=8)
    b = convergence.chain_stats(view.contiguous(), num_rho=8)
    for k in ("mean", "rhat", "tau", "ess", "mcse", "n_pairs", "stopped", "rho"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ---- diagnose against the oracle's composition --------------------------------------------
@pytest.mark.parametrize("name", sorted(O.diagnose_cases()))
def test_diagnose_vs_oracle(name):
    x = O.diagnose_cases()[name]
    xd = torch.from_numpy(x).to(DEV)
    R = x.shape[0]
    want = [O.diagnose_inputs(r) for r in x]
    # the ranks compare exactly, the indicators too; the normal scores to float32 rounding
    np.testing.assert_array_equal(N(convergence.average_ranks(xd)),
                                  np.stack([w["ranks"] for w in want]))
    inp = N(convergence.diagnose_inputs(xd))
    med = torch.from_numpy(np.array([w["med"] for w in want])).to(DEV)[:, None, None]
    np.testing.assert_array_equal(N(convergence.average_ranks((xd - med).abs())),
                                  np.stack([w["ranks_folded"] for w in want]))
    np.testing.assert_array_equal(inp[0], x)
    np.testing.assert_array_equal(inp[3], np.stack([w["lo"] for w in want]))
    np.testing.assert_array_equal(inp[4], np.stack([w["hi"] for w in want]))
    for q, key in ((1, "z"), (2, "z_folded")):
        z = np.stack([w[key] for w in want])
        err = np.abs(inp[q] - z).max()
        print(f"{name}: {key} differs from the float64 oracle by at most {err:.3g}")
        assert err <= O.U32 * np.abs(z).max() + 1e-12  # one rounding to float32
    # the diagnostics from the very inputs the kernel saw, within the kernel's bounds
    got = convergence.diagnose(xd, num_rho=16)
    stats = [O.chain_stats(inp[q], True, None, 16 if q == 0 else 0) for q in range(5)]
    comp = O.compose(stats)
    g = {k: N(getattr(got, k)) for k in comp}
    np.testing.assert_array_equal(g["stopped"], comp["stopped"])
    b = [bounds(s) for s in stats]
    limits = dict(rhat=np.maximum(b[1]["rhat"], b[2]["rhat"]), ess_bulk=b[1]["ess"],
                  ess_tail=np.maximum(b[3]["ess"], b[4]["ess"]), ess_mean=b[0]["ess"],
                  mcse_mean=b[0]["mcse"], tau=b[0]["tau"], mean=b[0]["mean"])
    for k, lim in limits.items():
        np.testing.assert_array_equal(np.isnan(g[k]), np.isnan(comp[k]), err_msg=k)
        err = np.abs(g[k] - comp[k])
        fin = np.isfinite(err)
        print(f"{name}: {k} err {err[fin].max(initial=0):.3g}, "
              f"bound {lim[fin].min(initial=np.inf):.3g}")
        assert (err[fin] <= lim[fin]).all(), (k, err, lim)
    rho_err = np.abs(N(got.rho) - stats[0]["rho"])
    assert (rho_err <= b[0]["rho"]).all()
    assert tuple(got.rhat.shape) == (R,) and tuple(got.rho.shape) == (R, 16)
    if name == "sticky":
        assert float(got.rhat.min()) >= 0.99 and bool(torch.isfinite(got.ess_tail).all())


def test_diagnose_uses_torch_quantile_above_the_lds_sort():
    """A pooled row above calibration.row_summary's limit (16384 entries) takes
    torch.quantile: the same thresholds as the oracle's definition."""
    x = O.big_diagnose_row()[None]
    xd = torch.from_numpy(x).to(DEV)
    w = O.diagnose_inputs(x[0])
    inp = convergence.diagnose_inputs(xd)
    np.testing.assert_array_equal(N(inp[3])[0], w["lo"])
    np.testing.assert_array_equal(N(inp[4])[0], w["hi"])
    np.testing.assert_array_equal(N(convergence.average_ranks((xd - float(w["med"])).abs()))[0],
                                  w["ranks_folded"])
    c = convergence.diagnose(xd)
    assert 1.0 <= float(c.rhat) < 1.01 and 2000 < float(c.ess_bulk) < 20000 * np.log10(20000)


# ---- diagnose_sampler ---------------------------------------------------------------------
def _mh(num_chains=3, **kw):
    from smcdet_amd.sampler import MHsampler
    from tests._params import M71, golden, p_m71_model, p_m71_prior, tiles_of
    d = golden("mcmc_m71_tiles.npz")
    tiles = torch.as_tensor(tiles_of(d["image"], 8)[:2, :2].copy(), device=DEV)
    return MHsampler.from_tiles(tiles, p_m71_prior(8, 3, 3), p_m71_model(8), 0.1, 2.5,
                                M71["flux_detection_threshold"], 400, 100, 2, print_every=10 ** 9,
                                num_chains=num_chains, seed=9, **kw)


@pytest.fixture(scope="module")
def finished_mh():
    mh = _mh()
    mh.run()
    return mh


def _hand_traces(mh, cuts):
    """The traces from mh.pruned_* and mh.fluxes with plain torch."""
    nH, nW = mh.tiles_shape
    C, S = mh.num_chains, mh.pruned_fluxes.shape[-1]
    M = mh.pruned_fluxes.shape[-2] // C
    slot = torch.arange(S, device=DEV) < mh.pruned_counts[..., None]
    rows = []
    for cut in cuts:
        on = slot & (mh.pruned_fluxes >= cut)
        rows += [on.sum(-1).float(), (mh.pruned_fluxes.double() * on).sum(-1).float()]
    rows.append(mh.fluxes.double().sum(-1).float())
    return torch.stack(rows, dim=2).reshape(nH, nW, len(rows), C, M)


def test_diagnose_sampler(finished_mh):
    mh = finished_mh
    cuts = (0.0, 2000.0)
    got = convergence.diagnose_sampler(mh, flux_cuts=cuts, num_rho=4)
    x, names = convergence.sampler_traces(mh, cuts)
    assert tuple(x.shape) == (2, 2, 5, 3, 150) and len(names) == 5 and names[-1] == "total_flux"
    hand = _hand_traces(mh, cuts)
    assert torch.equal(x[:, :, 0::2], hand[:, :, 0::2])  # counts and the intrinsic flux
    fl, hf = x[:, :, 1:4:2], hand[:, :, 1:4:2]           # catalog_totals' float64 slot-order sums
    assert bool(((fl - hf).abs() <= 1e-6 * hf.abs()).all())
    # chain-major: chain c of tile (h, w) is the kept samples [c * M, (c + 1) * M)
    assert torch.equal(x[1, 0, 4, 2], mh.fluxes[1, 0, 300:450].double().sum(-1).float())
    want = convergence.diagnose(x, num_rho=4)
    for k in ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "tau", "mean", "stopped",
              "rho"):
        assert torch.equal(torch.nan_to_num(getattr(got, k).double(), nan=-7.0),
                           torch.nan_to_num(getattr(want, k).double(), nan=-7.0)), k
    assert tuple(got.rhat.shape) == (2, 2, 5) and got.names == names
    assert torch.equal(got.accept_rate, mh.accept[..., 100:].float().mean(-1))
    assert tuple(got.accept_rate.shape) == (2, 2, 3) and got.frozen is mh.frozen
    assert bool(torch.isfinite(got.ess_mean[:, :, 4]).all())  # the total flux always moves
    for idx, name, *_ in got.warnings():
        assert name == names[idx[-1]] and len(idx) == 3
    assert len(got.warnings(rhat_max=float("inf"), ess_min=0)) == \
        int(torch.isnan(got.rhat + got.ess_bulk + got.ess_tail).sum())


def test_diagnose_sampler_log_target(finished_mh):
    got = convergence.diagnose_sampler(finished_mh, log_target=True)
    assert got.names[-1] == "log_target" and tuple(got.rhat.shape) == (2, 2, 4)
    x, _ = convergence.sampler_traces(finished_mh, log_target=True)
    lt = finished_mh.log_target(finished_mh.tiled_image, finished_mh.counts, finished_mh.locs,
                                finished_mh.fluxes)
    assert torch.equal(x[:, :, 3].reshape(2, 2, -1), lt.float())
    finite = torch.isfinite(lt).all(-1)
    assert bool(finite.any()) and bool(torch.isfinite(got.ess_mean[:, :, 3][finite]).all())


def test_identical_chains_have_no_between_chain_variance():
    """Three chains from one starting state under the same replayed draws are
    the same chain: unsplit, B = 0 and rhat = sqrt((n - 1) / n) exactly as the
    formula gives it."""
    mh = _mh()
    K = 399
    g = torch.Generator().manual_seed(4)
    one = dict(comp=torch.randint(0, 3, (K, 2, 2, 1), generator=g, dtype=torch.int32),
               uloc=torch.rand(K, 2, 2, 1, 2, generator=g),
               uflux=torch.rand(K, 2, 2, 1, generator=g),
               uacc=torch.rand(K, 2, 2, 1, generator=g))
    replay = {k: v.expand(K, 2, 2, 3, *v.shape[4:]).contiguous() for k, v in one.items()}
    mh.locs = mh.locs[:, :, :1].expand(2, 2, 3, 3, 2).contiguous()
    mh.fluxes = mh.fluxes[:, :, :1].expand(2, 2, 3, 3).contiguous()
    mh.run(replay=replay)
    x, names = convergence.sampler_traces(mh)
    assert torch.equal(x[..., 0, :], x[..., 1, :]) and torch.equal(x[..., 0, :], x[..., 2, :])
    s = convergence.chain_stats(x, split=False, chain_moments=True)
    live = ~torch.isnan(s.rhat)
    assert bool(live[:, :, 2].all())
    n = 150
    # (the mean of three equal float64 means may differ from them in the last bit, so
    # B / n is a few 1e-32 of mean^2 rather than exactly 0)
    within = s.W[live] * (n - 1) / n
    assert bool(((s.var_plus[live] - within).abs() <= 1e-15 * within).all())
    assert bool(((s.rhat[live] - ((n - 1) / n) ** 0.5).abs() < 1e-15).all())
    assert bool((s.chain_mean[..., 0] == s.chain_mean[..., 2]).all())
    assert bool((s.chain_var[..., 0] == s.chain_var[..., 1]).all())


def test_unrun_sampler_raises():
    with pytest.raises(RuntimeError, match="run the sampler first"):
        convergence.diagnose_sampler(_mh())
