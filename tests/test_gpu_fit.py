"""The image-model fit on the GPU: `fit.objective` against the
float64 oracle on every path of the kernel, run-to-run determinism, agreement
with the product's float32 likelihood, and `fit.fit_image_model` against the
oracle's own fit on the recovery case.

Float64 outputs: |kernel - oracle| <= K 2^-52 times the oracle's absolute-sum
scale of that output (the sum over the pixels of the absolute per-pixel terms),
K = 1024 (DESIGN.md §17.5 derives it from the kernel's operation chain; a
float32 intermediate costs 2^-24 relative in lambda, which the residual
x - lambda amplifies: 10^5 units and more, against 1024).  `rate`: one float32
rounding of the float64 value on top of that.
Every test prints the largest observed error next to its bound."""
import pickle

import numpy as np
import pytest
import torch

import _fit_oracle as O
from _params import M71, p_m71_mh, p_m71_prior
from smcdet_amd import fit
from smcdet_amd.images import M71ImageModel

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
K = 1024
U52 = 2.0 ** -52


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def cases():
    out = O.cases()
    for c in out.values():
        c["oracle"] = O.evaluate(c["log_theta"], c["image"], c["locs"], c["fluxes"], c["R"],
                                 c["mask"], c["counts"])
    return out


@pytest.fixture(scope="module")
def recovery():
    c = O.recovery_case(O.m71_truth())
    c["fit"] = O.fit(c["image"], c["locs"], c["fluxes"], c["start"], c["R"], c["mask"],
                     free=c["free"])
    return c


def run(c, rate=True):
    return fit.objective(T(c["image"]), T(c["locs"]), T(c["fluxes"]), c["log_theta"],
                         psf_radius=c["R"], mask=T(c["mask"]), counts=T(c["counts"]), rate=rate)


def check_against_oracle(name, got, ev):
    """The four outputs within their bounds; prints error / (2^-52 scale) next to K."""
    nll = float(got.nll)
    grad = got.grad.cpu().numpy()
    info = got.information.cpu().numpy()
    worst = {}
    e = abs(nll - ev["nll"])
    worst["nll"] = e / (U52 * ev["scale_nll"])
    assert e <= K * U52 * ev["scale_nll"], ("nll", e)
    for what, a, ref, scale in (("grad", grad, ev["grad"], ev["scale_grad"]),
                                ("information", info, ev["information"],
                                 ev["scale_information"])):
        err = np.abs(a - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(scale > 0, err / (U52 * scale), np.where(err > 0, np.inf, 0.0))
        worst[what] = float(ratio.max())
        assert np.all(err <= K * U52 * scale), (what, err, K * U52 * scale)
    assert np.array_equal(info, info.T)
    line = ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
    if got.rate is not None:
        rate = got.rate.cpu().numpy().astype(np.float64)
        err = np.abs(rate - ev["rate"])
        bound = (2.0 ** -24 + K * U52) * ev["scale_rate"]
        assert got.rate.dtype == torch.float32 and np.all(err <= bound)
        line += f", rate {float((err / bound).max()):.3g} of its bound (one float32 rounding)"
    print(f"{name}: largest |kernel - oracle| / (2^-52 scale), bound K = {K}: {line}")


@pytest.mark.parametrize("name", ["fixture_masked", "clipped_17x19_R16", "edge_stars_20x33_R4",
                                  "no_stars_18x21", "stars300_40x56", "ragged_3x20x24"])
def test_objective_against_oracle(cases, name):
    c = cases[name]
    check_against_oracle(name, run(c), c["oracle"])
    without = run(c, rate=False)  # masked pixels are then skipped: the same sums
    assert without.rate is None
    check_against_oracle(name + " (no rate)", without, c["oracle"])


def test_two_calls_return_the_same_bits(cases):
    for name in ("stars300_40x56", "fixture_masked"):
        a, b = run(cases[name]), run(cases[name])
        for x, y in ((a.nll, b.nll), (a.grad, b.grad), (a.information, b.information),
                     (a.rate, b.rate)):
            assert torch.equal(x, y)


def test_same_bits_after_reallocating_the_inputs(cases):
    c = cases["ragged_3x20x24"]
    a = run(c)
    junk = [torch.empty(n, device=DEV) for n in (1000, 3333, 70000)]  # moves the next blocks
    b = run({k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v)
             for k, v in c.items()})
    del junk
    for x, y in ((a.nll, b.nll), (a.grad, b.grad), (a.information, b.information)):
        assert torch.equal(x, y)
    # the fields' sums add: each field alone, summed in float64 on the host
    parts = []
    for f in range(3):
        one = fit.objective(T(c["image"][f:f + 1]), T(c["locs"][f:f + 1]),
                            T(c["fluxes"][f:f + 1]), c["log_theta"], psf_radius=c["R"],
                            mask=T(c["mask"][f:f + 1]), counts=T(c["counts"][f:f + 1]))
        parts.append(float(one.nll))
    ev = c["oracle"]
    assert abs(sum(parts) - float(a.nll)) <= 2 * K * U52 * ev["scale_nll"]


def test_nll_equals_the_products_loglikelihood():
    """The fixture field with a full mask: nll = -M71ImageModel.loglikelihood
    within what tests/test_gpu_parity.py allows that float32 kernel against its
    float64 oracle (rtol 2e-6, atol 5e-3)."""
    d = O.fixture()
    th = d["theta"][0]
    model = M71ImageModel(image_height=24, image_width=40, background=th[9],
                          psf_radius=int(d["psf_radius"]), adu_per_nmgy=th[0],
                          psf_params=list(th[1:7]), noise_additive=th[8],
                          noise_multiplicative=th[7])
    ll = model.loglikelihood(T(d["image"])[None, None], T(d["locs"])[None, None, None],
                             T(d["fluxes"])[None, None, None])
    got = fit.objective(T(d["image"]), T(d["locs"]), T(d["fluxes"]), model,
                        psf_radius=int(d["psf_radius"]))
    a, b = float(got.nll), -float(ll[0, 0, 0])
    print(f"nll {a:.6f}, -loglikelihood {b:.6f}, difference {abs(a - b):.3g}, "
          f"bound {2e-6 * abs(b) + 5e-3:.3g}")
    np.testing.assert_allclose(b, a, rtol=2e-6, atol=5e-3)


def test_fit_recovers_what_the_oracle_fit_recovers(recovery):
    c, of = recovery, recovery["fit"]
    idx = O.free_index(c["free"])
    init = fit.params_of(c["start"])
    args = (c["image"], c["locs"], c["fluxes"], c["R"], c["mask"])
    mf = fit.fit_image_model(T(c["image"]), T(c["locs"]), T(c["fluxes"]), init,
                             psf_radius=c["R"], mask=T(c["mask"]), free=c["free"])
    assert mf.converged and of["converged"]
    lt = mf.log_theta.numpy()
    fixed = [i for i in range(O.P) if i not in idx]
    np.testing.assert_allclose(lt[fixed], c["start"][fixed], rtol=0, atol=1e-15)
    at = O.evaluate(lt, *args)
    excess = at["nll"] - of["nll"]
    print(f"evaluations {mf.n_evals} (oracle {of['n_evals']}), oracle nll at the GPU's optimum "
          f"{at['nll']:.9f}, the oracle's minimum {of['nll']:.9f}, excess {excess:.3g} (< 1e-4)")
    assert excess < 1e-4
    assert abs(mf.nll - at["nll"]) <= K * U52 * at["scale_nll"]
    # stderr against the oracle's information at the same point: first-order
    # propagation |d cov| <= |cov| E |cov| of E = K 2^-52 scale through the 6x6
    # inverse (twice that, for the second order), plus the inverse's own rounding
    block = at["information"][np.ix_(idx, idx)]
    cov = np.linalg.inv(block)
    E = K * U52 * at["scale_information"][np.ix_(idx, idx)]
    dcov = 2 * np.diag(np.abs(cov) @ E @ np.abs(cov)) \
        + 64 * np.linalg.cond(block) * 2.0 ** -53 * np.diag(cov)
    se = np.sqrt(np.diag(cov))
    bound = dcov / (2 * se)
    err = np.abs(mf.stderr.numpy() - se)
    print(f"stderr {mf.stderr.numpy()}, largest error / bound {float((err / bound).max()):.3g}")
    assert np.all(err <= bound)
    assert mf.unidentified == () and torch.isfinite(mf.covariance).all()
    z = (lt[idx] - c["truth"][idx]) / mf.stderr.numpy()
    assert np.all(np.abs(z) < 4)
    assert tuple(mf.rate.shape) == (1, 32, 40) and mf.rate.dtype == torch.float32
    # params: params.pkl's form, through pickle, into a model the sampler takes
    back = pickle.loads(pickle.dumps(mf.params))
    assert back == mf.params and set(back) >= {"adu_per_nmgy", "psf_params", "noise_additive",
                                               "noise_multiplicative", "background"}
    model = mf.image_model(16, 16, 8)
    assert isinstance(model, M71ImageModel) and model.psf_params == back["psf_params"]
    from smcdet_amd.sampler import SMCsampler
    img = T(c["image"][0, :16, :16])
    s = SMCsampler(img, 16, p_m71_prior(16, 2, 2), model, p_m71_mh(5), 64, 0.5, "systematic",
                   M71["flux_detection_threshold"], 100, print_every=10 ** 9)
    s.run()
    assert torch.isfinite(s.log_normalizing_constant).all()


def test_free_single_and_all_ten_on_the_fixture_field():
    d = O.fixture()
    R = int(d["psf_radius"])
    init = fit.params_of(np.log(d["theta"][1]))  # noise_additive 2e-10
    data = (T(d["image"]), T(d["locs"]), T(d["fluxes"]))
    one = fit.fit_image_model(*data, init, psf_radius=R, free=("background",))
    assert one.converged and one.free == ("background",) and one.stderr.shape == (1,)
    assert torch.isfinite(one.grad).all() and float(one.grad[:9].abs().max()) > 1.0
    # stopped on |g| <= 1e-7 or on a change of nll below 1e-9 ~ g^2 / (2 I): ten times that
    assert abs(float(one.grad[9])) <= 10 * (2e-9 * float(one.information[9, 9])) ** 0.5
    fixed = one.log_theta.numpy()[:9]
    np.testing.assert_allclose(fixed, np.log(d["theta"][1][:9]), rtol=0, atol=1e-15)
    assert one.nll < float(fit.objective(*data, init, psf_radius=R).nll)
    every = fit.fit_image_model(*data, init, psf_radius=R, free=fit.PARAM_NAMES, max_iter=60,
                                steps=2)
    print(f"all ten free: nll {every.nll:.4f} after {every.n_evals} evaluations, unidentified "
          f"{every.unidentified}")
    assert every.nll <= one.nll and "noise_additive" in every.unidentified
    k = fit.PARAM_NAMES.index("noise_additive")
    assert np.isnan(float(every.stderr[k])) and torch.isfinite(every.grad).all()
    assert every.params["noise_additive"] > 0
