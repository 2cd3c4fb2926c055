"""smcdet_amd.extract without a device: the Python validation errors and the C
ABI's refusals (both come before any device work)."""
import ctypes
import os
import re

import pytest
import torch

import smcdet_amd
from smcdet_amd import _hip, extract

P = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(12)]  # placeholders, never dereferenced


def c_extract(T=2, H=8, W=8, G=3, n=32, K=16, null=None, n_found=P[10], segmap=P[11]):
    a = [P[0], P[1], P[2], T, H, W, P[3], P[4], P[5], P[6], G, n, K, P[7], P[8], P[9], n_found,
         segmap, None]
    if null is not None:
        a[null] = None
    L = _hip.lib()
    return L.smcdet_extract(*a), L.smcdet_last_error()


def test_exported_and_listed():
    assert "extract" in smcdet_amd._DROP_IN
    assert "smcdet_extract" in _hip.EXPORTS and "smcdet_extract" in _hip._OUTS
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "smcdet_hip.h")).read()
    assert int(re.search(r"#define SMCDET_EXTRACT_MAX_PIXELS (\d+)", header).group(1)) == \
        _hip.EXTRACT_MAX_PIXELS == 1024


def test_c_abi_refuses_unsupported_shapes():
    for kw, word in ((dict(H=33, W=32), b"pixels"), (dict(H=1, W=1025), b"pixels"),
                     (dict(K=65), b"K=65"), (dict(n=3), b"power of two"),
                     (dict(n=128), b"power of two"), (dict(n=48), b"power of two")):
        rc, msg = c_extract(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)


def test_c_abi_refuses_invalid_arguments():
    for kw in (dict(T=0), dict(H=0), dict(W=-1), dict(G=0), dict(K=0), dict(n=0)):
        rc, msg = c_extract(**kw)
        assert rc == -1 and b">= 1" in msg, (kw, rc, msg)
    for pos in (0, 1, 2, 6, 7, 8, 9, 13, 14, 15):  # every required buffer
        rc, msg = c_extract(null=pos)
        assert rc == -1 and b"null" in msg, (pos, rc, msg)


def test_alias_check_covers_the_outputs():
    args = (P[0], P[1], P[2], 2, 8, 8, P[3], P[4], P[5], P[6], 3, 32, 16, P[7], P[8], P[9], P[10],
            P[11], None)
    _hip.check_aliases("smcdet_extract", args)
    bad = list(args)
    bad[17] = P[13 - 6]  # segmap in the counts buffer
    with pytest.raises(ValueError, match="argument 13"):
        _hip.check_aliases("smcdet_extract", tuple(bad))


IMG = torch.zeros(2, 8, 8)


def call(**kw):
    a = dict(images=IMG, background=0.0, sigma=1.0, thresh=1.5)
    a.update(kw)
    return extract.extract(**a)


@pytest.mark.parametrize("kw, match", [
    (dict(images=torch.zeros(8)), "must be"),
    (dict(images=torch.zeros(2, 2, 8, 8)), "must be"),
    (dict(images=torch.zeros(0, 8, 8)), "must be"),
    (dict(images=torch.zeros(1, 33, 32)), "1056 pixels"),
    (dict(max_detections=65), "max_detections"),
    (dict(max_detections=0), "max_detections"),
    (dict(deblend_nthresh=3), "power of two"),
    (dict(deblend_nthresh=128), "power of two"),
    (dict(deblend_nthresh=0), "power of two"),
    (dict(minarea=0), "minarea"),
    (dict(minarea=2.5), "minarea"),
    (dict(thresh=0.0), "thresh"),
    (dict(thresh=float("nan")), "thresh"),
    (dict(thresh=float("inf")), "thresh"),
    (dict(sigma=0.0), "sigma"),
    (dict(sigma=float("inf")), "sigma"),
    (dict(sigma=torch.tensor([1.0, -1.0])), "sigma"),
    (dict(sigma=torch.ones(3)), "sigma"),
    (dict(background=float("nan")), "background"),
    (dict(background=torch.zeros(2, 2)), "background"),
    (dict(deblend_cont=-1e-3), "deblend_cont"),
    (dict(clean_param=-1.0), "clean_param"),
    (dict(flux_scale=0.0), "flux_scale"),
])
def test_python_validation(kw, match):
    with pytest.raises(ValueError, match=match):
        call(**kw)


def test_python_type_errors_and_host_tensors():
    with pytest.raises(TypeError, match="torch.Tensor"):
        call(images=[[0.0]])
    with pytest.raises(TypeError, match="extract_grid"):
        call(thresh=[1.5, 2.0])
    with pytest.raises(TypeError, match="int"):
        call(deblend_nthresh=32.0)
    # valid arguments, host tensor: refused, as everywhere (no CPU path)
    with pytest.raises(RuntimeError, match="HIP device"):
        call()
    with pytest.raises(RuntimeError, match="HIP device"):
        extract.extract_grid(IMG, 0.0, 1.0, [1.5, 2.0], [1, 5])
    with pytest.raises(RuntimeError, match="HIP device"):
        extract.tune(IMG, 0.0, 1.0, torch.zeros(2), torch.zeros(2, 1, 2), torch.zeros(2, 1),
                     [1.5, 2.0])


def test_grid_validation_names_the_axis():
    with pytest.raises(ValueError, match="empty"):
        extract.extract_grid(IMG, 0.0, 1.0, [])
    with pytest.raises(ValueError, match="minarea"):
        extract.extract_grid(IMG, 0.0, 1.0, [1.5], [1, 0])
    with pytest.raises(ValueError, match="max_bytes"):
        extract.tune(IMG, 0.0, 1.0, torch.zeros(2), torch.zeros(2, 1, 2), torch.zeros(2, 1),
                     [1.5], max_bytes=0)
