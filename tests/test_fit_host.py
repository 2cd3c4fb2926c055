"""The image-model fit without a GPU: the float64 oracle
against its own finite differences, a closed form and the reference's
likelihood; the oracle's own fit on the recovery case the GPU test repeats;
the Python argument checks and the C entry point's validation."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import _fit_oracle as O
from smcdet_amd import _hip, fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smcdet_hip.h")


@pytest.fixture(scope="module")
def recovery():
    c = O.recovery_case(O.m71_truth())
    c["fit"] = O.fit(c["image"], c["locs"], c["fluxes"], c["start"], c["R"], c["mask"],
                     free=c["free"])
    return c


# ---- the oracle's gradient and information -----------------------------------------------
def test_oracle_gradient_agrees_with_central_differences(recovery):
    """h = 1e-5 in every log: the truncation h^2/6 |d3 nll| is taken to be below
    1e-9 of the largest information entry of the row (third derivatives within
    60 times the second), the cancellation 8 eps |nll| / h is about 1e-6."""
    c = recovery
    args = (c["image"], c["locs"], c["fluxes"], c["R"], c["mask"])
    ev = O.evaluate(c["start"], *args)
    h = 1e-5
    for i in range(O.P):
        e = np.zeros(O.P)
        e[i] = h
        fd = (O.nll_at(c["start"] + e, *args) - O.nll_at(c["start"] - e, *args)) / (2 * h)
        bound = 1e-9 * np.abs(ev["information"][i]).max() + 1e-6
        print(f"{O.NAMES[i]}: |fd - grad| = {abs(fd - ev['grad'][i]):.3g}, bound {bound:.3g}")
        assert abs(fd - ev["grad"][i]) <= bound


@pytest.mark.parametrize("name", ["fixture_masked", "edge_stars_20x33_R4", "ragged_3x20x24"])
def test_oracle_information_is_symmetric_and_psd(name):
    c = O.cases()[name]
    ev = O.evaluate(c["log_theta"], c["image"], c["locs"], c["fluxes"], c["R"], c["mask"],
                    c["counts"])
    info = ev["information"]
    # the two triangles are computed separately: equal within the products' rounding
    assert np.all(np.abs(info - info.T) <= 16 * 2.0 ** -53 * ev["scale_information"])
    info = 0.5 * (info + info.T)
    s = 1.0 / np.sqrt(np.diag(info))
    w = np.linalg.eigvalsh(info * s[:, None] * s[None, :])
    assert w.min() >= -1e-13 * w.max()
    assert np.all(ev["scale_information"] >= np.abs(info) * (1 - 1e-12))
    assert np.all(ev["scale_grad"] >= np.abs(ev["grad"]) * (1 - 1e-12))
    assert ev["scale_nll"] >= abs(ev["nll"])
    # the scales are the plain sums of absolute per-pixel terms: on a single pixel
    # they are the absolute values of the outputs themselves
    one = np.zeros(c["image"].shape, np.uint8)
    one[0, 7, 9] = 1
    e1 = O.evaluate(c["log_theta"], c["image"], c["locs"], c["fluxes"], c["R"], one, c["counts"])
    np.testing.assert_allclose(e1["scale_information"], np.abs(e1["information"]), rtol=1e-12)
    assert np.all(e1["scale_grad"] >= np.abs(e1["grad"]) * (1 - 1e-12))
    assert abs(e1["scale_nll"] - abs(e1["nll"])) <= 1e-12 * e1["scale_nll"] or e1["nll"] < 0


def test_oracle_noise_information_closed_form():
    """10^3 pixels, no stars: lambda = B, v = na + nm B, and the (nm, nm) entry
    is sum (nm lambda / v)^2 / 2."""
    lt = O.log_theta_of(O.m71_truth(30.0)).numpy()
    e = np.zeros((1, 0, 2), np.float32)
    image = np.full((1, 25, 40), 100.0, np.float32)
    ev = O.evaluate(lt, image, e, e[..., 0], 8)
    nm, na, B = np.exp(lt[7]), np.exp(lt[8]), np.exp(lt[9])
    want = 1000 * 0.5 * (nm * B / (na + nm * B)) ** 2
    assert abs(ev["information"][7, 7] - want) <= 1e-12 * want
    assert np.all(ev["information"][1:7] == 0) and np.all(ev["grad"][:7] == 0)


# ---- the cases of tests/test_gpu_fit.py ---------------------------------------------------
def test_gpu_case_geometry_is_what_the_names_say():
    cases = O.cases()
    e = cases["edge_stars_20x33_R4"]
    fl = np.floor(e["locs"][0])
    assert fl[0, 0] == -3 and fl[1, 0] == -1 and fl[1, 1] == -1   # floor, not truncation
    assert np.all(e["locs"][0, 2] == fl[2])                         # integer coordinates
    assert fl[3, 0] - e["R"] > 19 and e["fluxes"][0, 4] == 0         # off the field; zero flux
    c = cases["clipped_17x19_R16"]
    fl = np.floor(c["locs"][0])
    assert np.all(fl - 16 <= 0) and np.all(fl[:, 0] + 16 >= 16) and np.all(fl[:, 1] + 16 >= 18), fl
    assert cases["stars300_40x56"]["fluxes"].shape[1] > 256
    m = cases["fixture_masked"]["mask"][0]
    assert not m[0:16, 16:32].any() and m[0:16, 0:16].all()
    n = cases["no_stars_18x21"]
    assert n["fluxes"].shape == (1, 0) and n["locs"].shape == (1, 0, 2)
    r = cases["ragged_3x20x24"]
    assert r["counts"].tolist() == [7, 0, 3] and r["fluxes"].shape == (3, 7)


# ---- the oracle against the reference ---------------------------------------------------
def test_oracle_matches_the_reference_loglikelihood():
    """-nll with a full mask against the reference's float32 loglikelihood at the
    fixture's three parameter vectors.  Bound: four times what
    tests/golden/make_fit_golden.py measured between the reference in float32 and
    the same code in float64 (5.98e-4 nats; the factor is for summation order)."""
    d = O.fixture()
    assert d["image"].shape == (24, 40) and d["locs"].shape == (12, 2)
    measured = float(d["f32_f64_diff"])
    assert 0 < measured < 1e-2
    for k in range(3):
        nll = O.nll_at(np.log(d["theta"][k]), d["image"][None], d["locs"][None],
                       d["fluxes"][None], int(d["psf_radius"]))
        err = abs(-nll - float(d["loglik_f32"][k]))
        print(f"theta {k}: |oracle - reference float32| = {err:.3g}, bound {4 * measured:.3g}; "
              f"against its float64 run {abs(-nll - float(d['loglik_f64'][k])):.3g}")
        assert err <= 4 * measured


# ---- the oracle's own fit on the recovery case ------------------------------------------
def test_oracle_fit_recovers_the_truth(recovery):
    c, f = recovery, recovery["fit"]
    idx = O.free_index(c["free"])
    args = (c["image"], c["locs"], c["fluxes"], c["R"], c["mask"])
    z = (f["log_theta"][idx] - c["truth"][idx]) / f["stderr"]
    print(f"evaluations {f['n_evals']}, condition number {f['cond']:.3g}, z {np.round(z, 2)}")
    assert f["converged"]
    assert f["nll"] <= O.nll_at(c["truth"], *args)
    assert f["cond"] < 1e6
    assert np.all(np.abs(z) < 4)
    fixed = [i for i in range(O.P) if i not in idx]
    assert np.array_equal(f["log_theta"][fixed], c["start"][fixed])
    assert int(c["mask"].sum()) == 32 * 40 - 2 * 40 - 3 * 30 - 20


def test_converged_means_a_tolerance_not_a_cap(recovery):
    """A step that ends on its iteration or evaluation cap (max_iter * 5 // 4) is
    not convergence: the oracle's fit and the product's loop (driven here by the
    oracle's objective) both say so with max_iter = 4, far from the optimum."""
    c = recovery
    nine = O.NAMES[:9]
    args = (c["image"], c["locs"], c["fluxes"], c["start"], c["R"], c["mask"])
    short = O.fit(*args, free=nine, max_iter=4, steps=1)
    g = O.evaluate(short["log_theta"], c["image"], c["locs"], c["fluxes"], c["R"], c["mask"],
                   information=False)["grad"]
    assert not short["converged"] and np.abs(g[:9]).max() > 1.0
    assert recovery["fit"]["converged"]

    idx = O.free_index(c["free"])
    for max_iter, steps, want in ((4, 1, False), (500, 10, True)):
        z = torch.from_numpy(c["start"][idx]).clone().requires_grad_(True)
        evals = [0]

        def closure():
            lt = c["start"].copy()
            lt[idx] = z.detach().numpy()
            ev = O.evaluate(lt, c["image"], c["locs"], c["fluxes"], c["R"], c["mask"],
                            information=False)
            z.grad = torch.from_numpy(ev["grad"][idx].copy())
            evals[0] += 1
            return torch.tensor(ev["nll"], dtype=torch.float64)

        assert fit.lbfgs_minimise(z, closure, max_iter=max_iter, steps=steps) is want
        assert evals[0] <= steps * max(max_iter * 5 // 4, 1) + steps
    np.testing.assert_allclose(z.detach().numpy(), recovery["fit"]["log_theta"][idx], atol=1e-6)


# ---- Python argument checks that need no device ---------------------------------------
def _host_inputs():
    return torch.zeros(1, 8, 8), torch.zeros(1, 2, 2), torch.ones(1, 2)


def test_python_refuses_unknown_names_negative_fluxes_and_host_tensors():
    img, locs, fluxes = _host_inputs()
    init = O.m71_truth()
    with pytest.raises(ValueError, match="unknown parameter"):
        fit.fit_image_model(img, locs, fluxes, init, psf_radius=4, free=("sigma1", "gamma"))
    with pytest.raises(ValueError, match="at least one"):
        fit.fit_image_model(img, locs, fluxes, init, psf_radius=4, free=())
    with pytest.raises(ValueError, match="finite and >= 0"):
        fit.objective(img, locs, -fluxes, init, psf_radius=4)
    with pytest.raises(ValueError, match="finite and >= 0"):
        fit.fit_image_model(img, locs, fluxes * float("nan"), init, psf_radius=4)
    with pytest.raises(ValueError, match="locs must be finite"):
        fit.objective(img, locs * float("nan"), fluxes, init, psf_radius=4)
    with pytest.raises(ValueError, match="blocks of 16x16"):
        fit.objective(torch.zeros(2 ** 24, 1, 1), torch.zeros(2 ** 24, 0, 2),
                      torch.zeros(2 ** 24, 0), init, psf_radius=4)
    with pytest.raises(RuntimeError, match="HIP device"):
        fit.objective(img, locs, fluxes, init, psf_radius=4)
    with pytest.raises(RuntimeError, match="HIP device"):
        fit.fit_image_model(img, locs, fluxes, init, psf_radius=4)
    with pytest.raises(ValueError, match="psf_radius"):
        fit.objective(img, locs, fluxes, init, psf_radius=65)
    with pytest.raises(ValueError, match="locs"):
        fit.objective(img, locs[:, :1], fluxes, init, psf_radius=4)
    with pytest.raises(ValueError, match="> 0"):
        fit.log_theta_of(dict(init, noise_additive=0.0))


def test_params_round_trip():
    init = dict(O.m71_truth(), flux_alpha=0.2)  # other keys of params.pkl are kept
    lt = fit.log_theta_of(init)
    assert lt.dtype == torch.float64 and tuple(fit.PARAM_NAMES) == O.NAMES
    np.testing.assert_array_equal(lt.numpy(), O.log_theta_of(init).numpy())
    back = pickle.loads(pickle.dumps(fit.params_of(lt, {"flux_alpha": 0.2})))
    assert back["flux_alpha"] == 0.2
    np.testing.assert_allclose(back["psf_params"], init["psf_params"], rtol=1e-15)
    from smcdet_amd.images import M71ImageModel
    m = M71ImageModel(image_height=8, image_width=8, psf_radius=4,
                      **{k: back[k] for k in ("background", "adu_per_nmgy", "psf_params",
                                              "noise_additive", "noise_multiplicative")})
    np.testing.assert_allclose(fit.log_theta_of(m).numpy(), lt.numpy(), rtol=0, atol=1e-15)


def test_free_covariance_marks_singular_directions():
    """The rule of DESIGN.md §17.4: eigenvalues of the free block below 1e-12 of
    the largest, and the parameters that carry them."""
    info = np.zeros((10, 10))
    info[0, 0], info[1, 1], info[0, 1], info[1, 0] = 4.0, 9.0, 1.0, 1.0
    info[8, 8] = 1e-22  # what a noise_additive of 1e-10 leaves
    cov, se, bad = fit.free_covariance(info, [0, 1, 8])
    assert bad == [2] and np.isnan(se[2]) and np.isnan(cov[2]).all() and np.isnan(cov[:, 2]).all()
    np.testing.assert_allclose(cov[:2, :2], np.linalg.inv(info[:2, :2]), rtol=1e-12)
    cov, se, bad = fit.free_covariance(info, [0, 1])
    assert bad == [] and np.all(np.isfinite(cov))
    info[8, 8] = 1e-6  # small but above the threshold: kept
    cov, se, bad = fit.free_covariance(info, [8, 0, 1])
    assert bad == [] and abs(se[0] - 1e3) < 1e-6
    # two exactly collinear parameters lose both; the third stays
    info[5, 5], info[6, 6], info[5, 6], info[6, 5] = 4.0, 1.0, 2.0, 2.0
    cov, se, bad = fit.free_covariance(info, [1, 5, 6])
    assert bad == [1, 2] and abs(se[0] - 1.0 / 3.0) < 1e-15
    info[2, 2] = float("nan")
    assert fit.free_covariance(info, [0, 2])[2] == [0, 1]


# ---- header, bindings, and the C entry point's validation -------------------------------
def test_abi_names_and_constants():
    hdr = open(HEADER).read()
    for name, value in (("FIT_PARAMS", 10), ("FIT_TERMS", 66), ("FIT_BLOCK", 16),
                        ("FIT_NORM_BLOCKS", 64), ("FIT_NORM_SUMS", 7),
                        ("FIT_MAX_BLOCKS", 2 ** 24 - 1)):
        assert getattr(_hip, name) == value
        assert f"#define SMCDET_{name} {value} " in hdr.replace("\n", " \n")
    assert "#define SMCDET_ABI_VERSION 20" in hdr and _hip.ABI_VERSION == 20
    assert "image-model fit (added under SMCDET_ABI_VERSION 20)" in hdr
    name = "smcdet_fit_objective"
    assert name in hdr and name in _hip.EXPORTS and name in _hip._OUTS
    assert hasattr(_hip.lib(), name)
    assert any(p.endswith("fit_kernel.hip") for p in _hip.SOURCES)
    assert "fit" in __import__("smcdet_amd")._DROP_IN


def _call(F=1, H=8, W=8, D=2, R=4, theta=None, null=(), ws_doubles=None):
    """Placeholder addresses (never read: only calls the host checks refuse)."""
    th = (ctypes.c_double * 10)(*([0.0] * 10 if theta is None else theta))
    p = {k: ctypes.c_void_p(0x10000 * (i + 1)) for i, k in enumerate(
        ("images", "mask", "locs", "fluxes", "counts", "nll", "grad", "information", "rate",
         "workspace"))}
    for k in null:
        p[k] = None
    need = 64 * 7 + 66 * max(F, 0) * ((H + 15) // 16) * ((W + 15) // 16)
    return _hip.lib().smcdet_fit_objective(
        None if "log_theta" in null else th, p["images"], p["mask"], p["locs"], p["fluxes"],
        p["counts"], F, H, W, D, R, p["nll"], p["grad"], p["information"], p["rate"],
        p["workspace"], need if ws_doubles is None else ws_doubles, None)


def _err():
    return _hip.lib().smcdet_last_error().decode()


@pytest.mark.parametrize("null", ["log_theta", "images", "locs", "fluxes", "nll", "grad",
                                  "information", "workspace"])
def test_abi_null_required_buffer_is_einval(null):
    assert _call(null=(null,)) == -1 and "null" in _err()


@pytest.mark.parametrize("kw,word", [
    (dict(F=0), "F=0"), (dict(H=0), "H=0"), (dict(W=-1), "W=-1"), (dict(D=-1), "D=-1"),
    (dict(R=-1), "psf_radius"), (dict(R=65), "psf_radius"),
    (dict(theta=[0.0] * 4 + [float("nan")] + [0.0] * 5), "log_theta[4]"),
    (dict(theta=[float("inf")] + [0.0] * 9), "log_theta[0]"),
    (dict(ws_doubles=64 * 7 + 66 - 1), "workspace"),
])
def test_abi_bad_sizes_are_einval(kw, word):
    assert _call(**kw) == -1 and word in _err()


@pytest.mark.parametrize("kw,word", [
    (dict(F=3, H=32768, W=32768), "pixels"), (dict(F=32768, D=65536), "stars"),
    (dict(F=2 ** 24, H=1, W=1), "pixel blocks"), (dict(F=2 ** 23, H=17, W=1), "pixel blocks"),
])
def test_abi_shapes_above_the_limits_are_eunsupported(kw, word):
    assert _call(**kw) == -2 and word in _err()
