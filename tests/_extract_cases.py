"""Hand-worked cases of smcdet_extract's definition, shared by the oracle's own
test (tests/test_extract_oracle_host.py, which states the expected results)
and the device test (tests/test_gpu_extract.py)."""
import numpy as np


def diag_image():
    v = np.zeros((5, 7), np.float32)
    for ij in ((0, 0), (1, 1), (2, 2), (4, 6)):
        v[ij] = 10
    return v


def ridge_image():
    v = np.zeros((3, 9), np.float32)
    v[1] = (0, 8, 16, 8, 2, 8, 16, 8, 0)
    return v


def plateau_image():
    v = np.zeros((6, 6), np.float32)
    v[1:5, 1:5] = 5
    return v


def nan_speckled_image():
    return np.array([[5, np.nan, 5, 5, np.nan, 0.5]], np.float32)


def clean_pair_image(vi):
    v = np.zeros((8, 8), np.float32)
    v[1:4, 1:4] = 1000
    v[2, 6] = vi
    return v


# name -> (image, keyword arguments of extract_one); background 0, sigma 1, so
# tau = thresh.  Shared with the device tests.
CASES = {
    "diag_minarea3": (diag_image(), dict(thresh=1, minarea=3, clean_param=0)),
    "diag_minarea1": (diag_image(), dict(thresh=1, minarea=1, clean_param=1)),
    "diag_minarea4": (diag_image(), dict(thresh=1, minarea=4, clean_param=0)),
    "diag_K1": (diag_image(), dict(thresh=1, minarea=1, clean_param=0, K=1)),
    "ridge_split": (ridge_image(), dict(thresh=1, minarea=1, deblend_nthresh=4,
                                        deblend_cont=0.005, clean_param=0)),
    "ridge_whole": (ridge_image(), dict(thresh=1, minarea=1, deblend_nthresh=4,
                                        deblend_cont=0.5, clean_param=0)),
    "ridge_n1": (ridge_image(), dict(thresh=1, minarea=1, deblend_nthresh=1,
                                     deblend_cont=0.005, clean_param=0)),
    "plateau": (plateau_image(), dict(thresh=1, minarea=5, clean_param=1)),
    "all_nan": (np.full((4, 5), np.nan, np.float32), dict(thresh=1, minarea=1)),
    "nan_speckled": (nan_speckled_image(), dict(thresh=1, minarea=1, clean_param=0)),
    "all_above": (np.full((4, 4), 3, np.float32), dict(thresh=1, minarea=5, clean_param=10)),
    "clean_absorb": (clean_pair_image(1.001), dict(thresh=1, minarea=1, clean_param=1)),
    "clean_keep": (clean_pair_image(1.002), dict(thresh=1, minarea=1, clean_param=1)),
    "clean_off": (clean_pair_image(1.001), dict(thresh=1, minarea=1, clean_param=0)),
}
