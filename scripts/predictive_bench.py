"""Times `smcdet_amd.predictive.posterior_image` (smcdet_posterior_image) at
the shape of the reference's m71 notebooks, 1000 tiles of 8x8 with 10,000
catalogs of S = 10, and at 64 tiles of 32x32 with 4096 catalogs (M71 model).

    python scripts/predictive_bench.py [--out profiles/predictive/predictive_bench.json]

Three things per shape, on the same device and inputs, in one process: the
fused call (mean, variance, chi2, chi2_rep, flux_rep); the existing route to
the same outputs (`ImageModel.rate`, float64 torch mean / var over catalogs,
smcdet_sample_image into a second array, float64 torch pixel sums); and
`ImageModel.loglikelihood`, which renders the same catalogs and reduces them to
one number each, so its ratio to the fused call prices the draws and the
float64 sums.  Each is timed with device events around the whole Python call
(allocations included), median and range of --launches calls after --warmup.
`torch.cuda.max_memory_allocated` is recorded for both routes (above what the
inputs hold), and the fused outputs are compared with the existing route's.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, predictive  # noqa: E402
from tests._params import p_m71_model  # noqa: E402

SHAPES = [dict(name="1000x8x8_N10000_S10", T=1000, H=8, N=10000, S=10),
          dict(name="64x32x32_N4096_S10", T=64, H=32, N=4096, S=10)]


def make_data(model, T, H, N, S, dev, seed=0):
    """Per tile S stars uniform on the tile padded by 2 px, fluxes log-uniform
    in 1..100 nmgy; each catalog jitters them by 0.1 px and 5 % in flux.  The
    tile image is one noisy draw from the stars themselves."""
    g = torch.Generator(device=dev).manual_seed(seed)
    tl = torch.rand(T, 1, 1, S, 2, device=dev, generator=g) * (H + 4) - 2
    tf = 10 ** (2 * torch.rand(T, 1, 1, S, device=dev, generator=g))
    locs = (tl + 0.1 * torch.randn(T, 1, N, S, 2, device=dev, generator=g)).contiguous()
    fluxes = (tf * (1 + 0.05 * torch.randn(T, 1, N, S, device=dev, generator=g))).clamp_(min=0.01)
    torch.manual_seed(seed)
    img = model.sample(tl.contiguous(), tf.contiguous())[..., 0].contiguous()
    return img, locs, fluxes.contiguous()


def existing_route(model, img, locs, fluxes, seed):
    rate = model.rate(locs, fluxes)                                   # [T,1,H,W,N] float32
    lam = rate.double()
    mean, var = lam.mean(-1), lam.var(-1, unbiased=False)
    x = torch.empty_like(rate)
    cm = model._cmodel()
    _hip.check(_hip.lib().smcdet_sample_image(_hip.ref(cm), _hip.ptr(rate), rate.numel(), seed, 0,
                                              _hip.ptr(x), _hip.stream_of(rate)),
               "smcdet_sample_image")
    v = float(model.noise_additive) + float(model.noise_multiplicative) * lam
    x = x.double()
    flux_rep = x.sum((2, 3))
    chi2_rep = ((x - lam) ** 2 / v).sum((2, 3))
    chi2 = ((img.double()[..., None] - lam) ** 2 / v).sum((2, 3))
    return mean, var, chi2, chi2_rep, flux_rep


def timed(fn, warmup, launches):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), launches=launches)


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return out, int(peak)


def reldiff(a, b):
    return float(((a.double() - b.double()).abs() / b.double().abs().clamp_min(1e-300)).max())


def bench_shape(sh, dev, warmup, launches, seed=20261019):
    T, H, N, S = sh["T"], sh["H"], sh["N"], sh["S"]
    model = p_m71_model(H)
    img, locs, fluxes = make_data(model, T, H, N, S, dev)
    fused = lambda: predictive.posterior_image(model, locs, fluxes, tiled_image=img,  # noqa: E731
                                               seed=seed)
    old = lambda: existing_route(model, img, locs, fluxes, seed)  # noqa: E731
    ll = lambda: model.loglikelihood(img, locs, fluxes)  # noqa: E731
    got, peak_fused = peak_above_inputs(fused)
    want, peak_old = peak_above_inputs(old)
    res = dict(sh, pixels=H * H, rate_array_bytes=4 * T * H * H * N,
               workspace_bytes=int(_hip.lib().smcdet_posterior_image_workspace(
                   _hip.ref(model._cmodel()), T, N)),
               catalog_chunks=predictive.catalog_chunks(H * H, N),
               peak_bytes_fused=peak_fused, peak_bytes_existing=peak_old,
               agreement=dict(
                   mean_max_rel=reldiff(got.mean, want[0]),
                   var_max_abs_over_mean_sq=float(((got.rate_var.double() - want[1]).abs()
                                                   / want[0] ** 2).max()),
                   chi2_max_rel=reldiff(got.chi2, want[2]),
                   chi2_rep_max_rel=reldiff(got.chi2_rep, want[3]),
                   flux_rep_max_rel=reldiff(got.flux_rep, want[4])))
    del got, want
    # alternate the three so that a drift of the box hits them alike
    res["fused"] = timed(fused, warmup, launches)
    res["existing"] = timed(old, warmup, launches)
    res["loglik"] = timed(ll, warmup, launches)
    res["fused_again"] = timed(fused, 1, launches)
    res["existing_over_fused"] = res["existing"]["median_ms"] / res["fused"]["median_ms"]
    res["fused_over_loglik"] = res["fused"]["median_ms"] / res["loglik"]["median_ms"]
    res["catalogs_per_s_fused"] = T * N / (res["fused"]["median_ms"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/predictive/predictive_bench.json")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predictive_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    out = dict(device=torch.cuda.get_device_name(0), library=_hip.version(),
               warmup=args.warmup, launches=args.launches,
               timing="torch device events around the whole Python call, one process",
               shapes=[bench_shape(sh, dev, args.warmup, args.launches) for sh in SHAPES])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
