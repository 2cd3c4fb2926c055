"""The PSF-fitting detector without a device: the float64 oracle
(tests/_psffind_oracle.py) against a closed form and on the cases DESIGN.md
§19 quotes, and the refusals of the Python layer and of the C ABI (all before
any device work).

Measured with this oracle (float64 profile; the prototype's figures in
brackets): a noise-free isolated 50 nmgy star at five positions -- the peak
refinement off by at most 0.0476 px [0.048], after the pipeline 0.0168 px
[0.017] and 1.13 % in flux [1.2 %]; three_corner 3 detections at most 0.075 px
off; padding found at row -1.355 [-1.35]; the separated set 80 of 80 with 0
spurious and max |z| 4.65 [80/80, 0, 4.6]; no peak on 200 blank tiles."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _photometry_oracle as P
import _psffind_oracle as F
import smcdet_amd
from _params import p_m71_model
from smcdet_amd import _hip, psffind

MODEL = F.model_of(p_m71_model(8))
ROOT = os.path.dirname(_hip._HERE)
HEADER = open(os.path.join(ROOT, "include", "smcdet_hip.h")).read()


# ---- the oracle ------------------------------------------------------------------------
def test_oracle_profile_is_the_photometry_oracle_s():
    locs = [(3.7, 4.2), (-1.5, 3.3), (0.6, 7.9)]
    assert np.array_equal(F.phi(MODEL, locs), P.columns(MODEL, locs))
    d = np.abs(F.phi(MODEL, locs, np.float32) - F.phi(MODEL, locs))
    assert 0 < d.max() <= 4 * 2.0 ** -24 * F.phi(MODEL, locs).max()


def test_oracle_matches_the_closed_form():
    """With an empty list f-hat at a cell is the one-iteration flux solve of a
    single source at that cell's centre: the same sums."""
    m = MODEL
    x = F.noisy(m, F.render(m, [(3.7, 4.2)], [50.0]), np.random.default_rng(7))
    _, _, st, _ = F.significance_map(m, x, cells=2)
    ctr, cH, cW = F.cell_centres(m, 2)
    assert (cH, cW) == (16, 16)
    worst = 0.0
    for xc in range(0, 256, 5):
        r = F.solve_one(m, x, 1, ctr[xc:xc + 1].astype(np.float32), n_iter=1)
        worst = max(worst, abs(r["fluxes"][0] - st.fhat[xc]) / abs(st.fhat[xc]))
    print(f"closed form: {worst:.3g} relative")
    assert worst <= 1e-12


@pytest.mark.parametrize("loc", [(3.7, 4.2), (0.6, 0.6), (4.0, 4.0), (7.3, 2.45), (2.13, 6.9)])
def test_noise_free_isolated_star(loc):
    m = MODEL
    x = F.render(m, [loc], [50.0]).astype(np.float32)
    f = F.find(m, x, 5.0)
    assert f.count == 1 and len(f.first_locs) == 1
    d0 = np.abs(f.first_locs[0] - np.array(loc)).max()
    d1 = np.abs(f.locs[0] - np.array(loc)).max()
    df = abs(f.fluxes[0] / 50.0 - 1.0)
    print(f"{loc}: refinement {d0:.4f} px, pipeline {d1:.4f} px, flux {100 * df:.2f} %")
    assert d0 <= 0.06 and d1 <= 0.025 and df <= 0.015


def test_three_corner_and_padding():
    m = MODEL
    rng = np.random.default_rng(11)
    found = {}
    for name, (ll, ff) in P.CONFIGS.items():  # the noise drawn in CONFIGS order
        x = F.noisy(m, F.render(m, np.asarray(ll, np.float32), ff), rng)
        found[name] = F.find(m, x, 5.0)
    f = found["three_corner"]
    pairs, free = F.match(P.CONFIGS["three_corner"][0], f.locs[:f.count], 0.15)
    assert f.count == 3 and len(pairs) == 3 and not free
    f = found["padding"]
    assert f.count == 1 and f.locs[0, 0] < 0
    # the documented limit: a pair 0.8 px apart stays one detection
    assert found["pair_0p8"].count == 1
    print("pair_0p8 found as", found["pair_0p8"].locs[0], found["pair_0p8"].fluxes[0], "nmgy")


def test_separated_set():
    """40 tiles of 1..3 stars at least 4 px apart: every true star matched
    within 0.5 px (Chebyshev) and no other detection."""
    m = MODEL
    total = matched = spurious = 0
    for x, ll, _ in F.separated_set(m):
        f = F.find(m, x, 5.0)
        pairs, free = F.match(ll, f.locs[:f.count], 0.5)
        total, matched, spurious = total + len(ll), matched + len(pairs), spurious + len(free)
    print(f"separated set: {matched} of {total} matched, {spurious} spurious")
    assert matched == total and spurious == 0


def test_blank_tiles_give_no_peak():
    m = MODEL
    rng = np.random.default_rng(11)
    blank = F.render(m, np.zeros((0, 2)), [])
    for _ in range(200):
        f = F.find_one(m, F.noisy(m, blank, rng), 0, None, None, 16, 5.0, 1, 0.5)
        assert f["n_found"] == 0 and f["counts_out"] == 0


def test_oracle_peak_rule():
    """Ties go to the lower flat index; the cap keeps the largest; listed
    sources exclude by Chebyshev distance; uncounted slots exclude nothing."""
    s = np.zeros((8, 8), np.float32)
    s[2, 2] = s[2, 3] = 7.0
    s[6, 6] = 9.0
    n, cells, locs, _ = F.select_peaks(s, 1, 5.0, 1, 0.5, np.zeros((0, 2)), 8)
    assert n == 2 and cells == [6 * 8 + 6, 2 * 8 + 2]
    n, cells, _, _ = F.select_peaks(s, 1, 5.0, 0, 0.5, np.zeros((0, 2)), 2)
    assert n == 3 and cells == [54, 18]
    n, cells, _, _ = F.select_peaks(s, 1, 5.0, 1, 0.5, [(6.9, 6.1)], 8)
    assert n == 1 and cells == [18]
    m = MODEL
    x = F.render(m, [(3.7, 4.2)], [50.0]).astype(np.float32)
    a = F.find_one(m, x, 0, None, None, 4, 5.0, 1, 0.5)
    locs = np.array([(3.7, 4.2), (np.nan, 1.0), (3.7, 4.2), (3.7, 4.2)], np.float32)
    b = F.find_one(m, x, 2, locs, np.array([np.nan, 5.0, 50.0, 50.0], np.float32), 4, 5.0, 1, 0.5)
    assert b["counts_out"] == 3 and a["cells"] == b["cells"]
    np.testing.assert_array_equal(a["map"], b["map"])


# ---- plumbing -----------------------------------------------------------------------------
def test_exported_and_listed():
    assert "psffind" in smcdet_amd._DROP_IN
    L = _hip.lib()
    for name in ("smcdet_psf_find", "smcdet_psf_recentre"):
        assert name in _hip.EXPORTS and name in _hip._OUTS
        assert hasattr(L._cdll, name)
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", HEADER).group(1)
        assert len(proto.split(",")) == len(_hip._SIGS[name][0])
        outs = _hip._OUTS[name][0]
        params = [p.strip() for p in proto.split(",")]
        assert all("const" not in params[o] and "*" in params[o] for o in outs)
        assert sum("*" in p and "const" not in p for p in params[:-1]) == len(outs)
    for macro, value in (("FIND_MAX_CELLS_PER_PIXEL", 4), ("FIND_MAX_CELLS", 16384),
                         ("FIND_MAX_NMS", 16), ("FIND_MAX_HALF", 3)):
        assert int(re.search(rf"#define SMCDET_{macro} (\d+)", HEADER).group(1)) == \
            getattr(_hip, macro) == value


def test_sources_match_the_makefile():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    hdrs = re.search(r"^HDRS := (.*)$", mk, re.M).group(1).split()
    want = [p.replace("$(CSRC)", "smcdet_amd/csrc") for p in srcs + hdrs]
    assert [os.path.relpath(p, ROOT) for p in _hip.SOURCES] == want
    assert "smcdet_amd/csrc/find_kernel.hip" in want


IMG = torch.zeros(2, 8, 8)


def grid(**kw):
    a = dict(images=IMG, ImageModel=p_m71_model(8), thresh=[5.0])
    a.update(kw)
    return psffind.find_grid(**a)


@pytest.mark.parametrize("kw, match", [
    (dict(images=torch.zeros(2, 25, 41)), "1025 pixels"),
    (dict(ImageModel=p_m71_model(16)), "image model is 16x16"),
    (dict(cells=0), "cells"), (dict(cells=5), "cells"),
    (dict(rounds=0), "rounds"), (dict(sweeps=0), "sweeps"),
    (dict(half=0), "half"), (dict(half=4), "half"),
    (dict(step=0.0), "step"), (dict(step=float("inf")), "step"),
    (dict(min_sep=-0.1), "min_sep"),
    (dict(max_detections=0), "max_detections"), (dict(max_detections=33), "max_detections"),
    (dict(thresh=[]), "thresh is empty"), (dict(thresh=[float("nan")]), "thresh"),
    (dict(nms_radius=[17]), "nms_radius"), (dict(nms_radius=[1.5]), "nms_radius"),
    (dict(min_snr=[float("inf")]), "min_snr"),
    (dict(background=0.0), "background"),
    (dict(background=torch.tensor([100.0, -1.0])), "background"),
])
def test_python_validation(kw, match):
    with pytest.raises(ValueError, match=match):
        grid(**kw)


def test_python_type_errors_and_host_tensors():
    with pytest.raises(TypeError, match="int"):
        grid(cells=2.0)
    with pytest.raises(TypeError, match="image model"):
        grid(ImageModel=object())
    with pytest.raises(TypeError, match="find_grid takes sequences"):
        psffind.find(IMG, p_m71_model(8), [5.0])
    with pytest.raises(RuntimeError, match="HIP device"):
        grid()  # valid arguments, host tensors: refused, there is no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        psffind.find(IMG, p_m71_model(8), 5.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        psffind.significance_map(IMG, p_m71_model(8))
    with pytest.raises(RuntimeError, match="HIP device"):
        psffind.tune(IMG, p_m71_model(8), torch.zeros(2), torch.zeros(2, 1, 2), torch.zeros(2, 1),
                     [5.0])
    with pytest.raises(ValueError, match="max_bytes"):
        psffind.tune(IMG, p_m71_model(8), torch.zeros(2), torch.zeros(2, 1, 2), torch.zeros(2, 1),
                     [5.0], max_bytes=0)
    with pytest.raises(ValueError, match="together"):
        psffind.significance_map(IMG, p_m71_model(8), counts=torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="fluxes must be"):
        psffind.significance_map(IMG, p_m71_model(8), torch.ones(2, dtype=torch.int32),
                                 torch.zeros(2, 4, 2), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="33 position slots"):
        psffind.significance_map(IMG, p_m71_model(8), torch.ones(2, dtype=torch.int32),
                                 torch.zeros(2, 33, 2), torch.zeros(2, 33))


def test_residual_significance_checks_before_the_device():
    class Stub:
        def __init__(self, n, K):
            self.n, self.K = n, K

        def as_catalog(self, min_prob):
            return (torch.full((2, 1), self.n, dtype=torch.int32), torch.zeros(2, 1, self.K, 2),
                    torch.zeros(2, 1, self.K))

    with pytest.raises(ValueError, match="keeps 40 detections"):
        psffind.residual_significance(Stub(40, 48), IMG, p_m71_model(8))
    with pytest.raises(ValueError, match="image model is 16x16"):
        psffind.residual_significance(Stub(2, 4), IMG, p_m71_model(16))
    with pytest.raises(ValueError, match="cells"):
        psffind.residual_significance(Stub(2, 4), IMG, p_m71_model(8), cells=5)
    with pytest.raises(RuntimeError, match="HIP device"):  # 48 slots, 2 kept: cut to 32, then refused
        psffind.residual_significance(Stub(2, 48), IMG, p_m71_model(8))


def test_settings_are_the_product_last_axis_fastest():
    s = psffind._settings([5.0, 6.0], [0, 1], [3.0, 4.0, 5.0])
    assert s.shape == (12, 3) and s.dtype == torch.float64
    assert s[0].tolist() == [5.0, 0.0, 3.0] and s[1].tolist() == [5.0, 0.0, 4.0]
    assert s[3].tolist() == [5.0, 1.0, 3.0] and s[6].tolist() == [6.0, 0.0, 3.0]


# ---- the C ABI's refusals (placeholder pointers, never dereferenced) ------------------
PTR = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(16)]


def cmodel(**fields):
    cm = type(p_m71_model(8)._cmodel()).from_buffer_copy(p_m71_model(8)._cmodel())
    for k, v in fields.items():
        setattr(cm, k, v)
    return cm


def c_find(T=2, G=3, K=4, cells=2, min_sep=0.5, null=(), **fields):
    a = [ctypes.byref(cmodel(**fields)), PTR[0], None, PTR[1], PTR[2], PTR[3], T, G, K, cells,
         PTR[4], PTR[5], min_sep, PTR[6], PTR[7], PTR[8], PTR[9], PTR[10], None, None]
    for i in null:
        a[i] = None
    L = _hip.lib()
    return L.smcdet_psf_find(*a), L.smcdet_last_error()


def c_move(T=2, G=3, K=4, half=2, step=0.25, null=(), **fields):
    a = [ctypes.byref(cmodel(**fields)), PTR[0], None, PTR[1], PTR[2], PTR[3], T, G, K, half, step,
         PTR[4], PTR[5], None]
    for i in null:
        a[i] = None
    L = _hip.lib()
    return L.smcdet_psf_recentre(*a), L.smcdet_last_error()


@pytest.mark.parametrize("call", [c_find, c_move])
def test_c_abi_refuses_unsupported_shapes(call):
    for kw, word in ((dict(H=33, W=32), b"pixels"), (dict(H=1, W=1025), b"pixels"),
                     (dict(K=33), b"K=33"), (dict(psf_radius=65), b"psf_radius"),
                     (dict(psf_radius=-1), b"psf_radius"), (dict(T=65536, G=32768), b"problems")):
        rc, msg = call(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    # (1,024 pixels at 4 cells per pixel are the 16,384 cells of the map's limit: the cell
    # limit cannot be passed without passing one of the two others)


@pytest.mark.parametrize("call", [c_find, c_move])
def test_c_abi_refuses_invalid_arguments(call):
    for kw, word in ((dict(T=0), b">= 1"), (dict(G=0), b">= 1"), (dict(K=0), b">= 1"),
                     (dict(background=0.0), b"background"),
                     (dict(background=float("nan")), b"background"),
                     (dict(noise_multiplicative=-1.0), b"variance"),
                     (dict(adu_per_nmgy=0.0), b"adu_per_nmgy")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_c_abi_find_arguments():
    for kw, word in ((dict(cells=0), b"cells=0"), (dict(cells=5), b"cells=5"),
                     (dict(min_sep=-1.0), b"min_sep"), (dict(min_sep=float("nan")), b"min_sep")):
        rc, msg = c_find(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for pos in (1, 10, 11, 13, 14, 15, 16, 17):  # every required buffer
        rc, msg = c_find(null=(pos,))
        assert rc == -1 and b"null" in msg, (pos, rc, msg)
    for pos in (3, 4, 5):  # a list is given whole or not at all
        rc, msg = c_find(null=(pos,))
        assert rc == -1 and b"together" in msg, (pos, rc, msg)


def test_c_abi_recentre_arguments():
    for kw, word in ((dict(half=0), b"half=0"), (dict(half=4), b"half=4"),
                     (dict(step=0.0), b"step"), (dict(step=float("nan")), b"step")):
        rc, msg = c_move(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    for pos in (1, 3, 4, 5, 11, 12):
        rc, msg = c_move(null=(pos,))
        assert rc == -1 and b"null" in msg, (pos, rc, msg)


def test_alias_check_covers_the_outputs():
    cm = cmodel()
    args = [ctypes.byref(cm), PTR[0], None, PTR[1], PTR[2], PTR[3], 2, 3, 4, 2, PTR[4], PTR[5],
            0.5, PTR[6], PTR[7], PTR[8], PTR[9], PTR[10], PTR[11], None]
    _hip.check_aliases("smcdet_psf_find", tuple(args))
    for out in range(13, 19):
        bad = list(args)
        bad[out] = PTR[2]  # an output in the locs buffer
        with pytest.raises(ValueError, match=f"argument {out}"):
            _hip.check_aliases("smcdet_psf_find", tuple(bad))
    args = [ctypes.byref(cm), PTR[0], None, PTR[1], PTR[2], PTR[3], 2, 3, 4, 2, 0.25, PTR[4],
            PTR[5], None]
    _hip.check_aliases("smcdet_psf_recentre", tuple(args))
    bad = list(args)
    bad[11] = PTR[2]  # recentring in place is refused: the sweep is Jacobi
    with pytest.raises(ValueError, match="argument 11"):
        _hip.check_aliases("smcdet_psf_recentre", tuple(bad))
