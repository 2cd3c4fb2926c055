"""Times the three calibration kernels (smcdet_catalog_totals,
smcdet_row_summary, smcdet_bootstrap_means) at the shape of the reference's
m71synthetic results notebook -- T = 1000 tiles, N = 10,000 catalogs, S = 10
slots, one flux cut, 19 credible levels; 17 x 3 metric columns and 10,000
bootstrap replicates -- next to their torch counterparts on the same device and
inputs, in the same process, alternating with them run by run:

    catalog totals        fluxes.sum(-1)
    38 linear quantiles   torch.quantile(x, q, dim=-1)
    weighted "lower"      torch.sort + gather + cumsum + searchsorted
    quantiles over [1, 10000, 51] along dim 1    torch.quantile(x, q, dim=0)
    bootstrap means       chunked rows[randint].mean(1)

    python scripts/calibration_bench.py [--out profiles/calibration/calibration_bench.json]

Every figure is the median (with min and max) of --runs timings by device
events around one call, after --warmup calls.  Bytes are computed from the
shapes; peak memory is torch.cuda.max_memory_allocated over one call beyond
what was allocated before it.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, calibration  # noqa: E402


def stats(ms):
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), runs=len(ms))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def alternate(ours, theirs, runs, warmup):
    """ours and theirs timed in turn, run by run."""
    for _ in range(warmup):
        ours()
        theirs()
    ev = [(timed(ours), timed(theirs)) for _ in range(runs)]
    torch.cuda.synchronize()
    return (stats([a.elapsed_time(b) for (a, b), _ in ev]),
            stats([a.elapsed_time(b) for _, (a, b) in ev]))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def sort_lds_bytes(rows, N, key_bytes):
    """LDS traffic of the bitonic network: every stage reads all P keys and
    writes back those it swaps (at most all)."""
    P = max(64, 1 << (N - 1).bit_length())
    k = int(math.log2(P))
    stages = k * (k + 1) // 2
    return dict(P=P, stages=stages, read=rows * stages * P * key_bytes,
                read_and_write_at_most=2 * rows * stages * P * key_bytes)


def entry(ours, theirs, bytes_moved, peak_ours, peak_theirs, **extra):
    gb = bytes_moved / (ours["ms_median"] * 1e-3) / 1e9
    return dict(kernel=ours, torch=theirs, torch_over_kernel=theirs["ms_median"] / ours["ms_median"],
                bytes_moved=bytes_moved, kernel_GBps=gb, peak_bytes_kernel=peak_ours,
                peak_bytes_torch=peak_theirs, **extra)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--catalogs", type=int, default=10000)
    ap.add_argument("--sources", type=int, default=10)
    ap.add_argument("--columns", type=int, default=51)
    ap.add_argument("--replicates", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out",
                    default=os.path.join("profiles", "calibration", "calibration_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibration_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    T, N, S, D, Bn = a.tiles, a.catalogs, a.sources, a.columns, a.replicates
    g = torch.Generator(device=dev).manual_seed(0)
    counts = torch.randint(0, S + 1, (T, N), device=dev, generator=g, dtype=torch.int32)
    fluxes = torch.exp(2.0 + torch.randn(T, N, S, device=dev, generator=g))
    fluxes[torch.arange(S, device=dev)[None, None, :] >= counts[..., None]] = 0.0
    weights = torch.rand(T, N, device=dev, generator=g)
    levels = calibration.DEFAULT_LEVELS
    q = calibration._interval_q(levels)
    qt = torch.tensor(q, device=dev, dtype=torch.float32)
    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(),
               shape=dict(T=T, N=N, S=S, cuts=1, levels=len(levels), columns=D, replicates=Bn),
               runs=a.runs, warmup=a.warmup)

    # ---- per-catalog totals --------------------------------------------------------
    def ours():
        return calibration.catalog_totals(counts, fluxes, (0.0,))

    def theirs():
        return fluxes.sum(-1)

    tot = ours()
    same = float((tot.flux_above[0] - theirs()).abs().max())
    k, t = alternate(ours, theirs, a.runs, a.warmup)
    res["catalog_totals"] = entry(k, t, 4 * T * N * S + 4 * T * N + 8 * T * N, peak_bytes(ours),
                                  peak_bytes(theirs), torch_is="fluxes.sum(-1)",
                                  max_abs_diff_from_torch=same)
    print("catalog_totals", json.dumps(res["catalog_totals"]), flush=True)
    x = tot.flux_above[0].contiguous()  # [T,N]
    truth = x[:, :1].contiguous()
    del tot

    # ---- 38 linear quantiles per row -------------------------------------------------
    def ours():
        return calibration.row_summary(x, quantiles=q, thresholds=truth)

    def theirs():
        return torch.quantile(x, qt, dim=-1)

    diff = float((ours().quantiles - theirs().t()).abs().max())
    k, t = alternate(ours, theirs, a.runs, a.warmup)
    res["row_summary_linear"] = entry(
        k, t, 4 * T * N, peak_bytes(ours), peak_bytes(theirs),
        torch_is="torch.quantile(x [T,N], 38 levels, dim=-1)", max_abs_diff_from_torch=diff,
        lds_sort=sort_lds_bytes(T, N, 4), lds_bytes=_hip_lds(N, False))
    print("row_summary_linear", json.dumps(res["row_summary_linear"]), flush=True)

    # ---- weighted "lower" quantiles ----------------------------------------------------
    def ours():
        return calibration.row_summary(x, weights=weights, quantiles=q, interpolation="lower",
                                       thresholds=truth)

    def theirs():
        sf, order = x.sort(-1)
        cw = weights.double().gather(-1, order).cumsum(-1)
        target = qt.double()[None, :] * cw[:, -1:]
        first = torch.searchsorted(cw, target).clamp_(max=N - 1)
        return sf.gather(-1, first)

    same = bool(torch.equal(ours().quantiles, theirs()))
    k, t = alternate(ours, theirs, a.runs, a.warmup)
    res["row_summary_weighted_lower"] = entry(
        k, t, 8 * T * N, peak_bytes(ours), peak_bytes(theirs),
        torch_is="sort + gather(weights) + float64 cumsum + searchsorted + gather",
        equals_torch=same, lds_sort=sort_lds_bytes(T, N, 8), lds_bytes=_hip_lds(N, True))
    print("row_summary_weighted_lower", json.dumps(res["row_summary_weighted_lower"]), flush=True)

    # ---- bootstrap means ---------------------------------------------------------------
    rows = torch.rand(N, D, device=dev, generator=g)
    chunk = 100

    def ours():
        return calibration.bootstrap_means(rows, Bn, seed=1)

    def theirs():
        out = torch.empty(Bn, D, device=dev)
        for r0 in range(0, Bn, chunk):
            idx = torch.randint(0, N, (min(chunk, Bn - r0), N), device=dev)
            out[r0:r0 + idx.shape[0]] = rows[idx].mean(1)
        return out

    k, t = alternate(ours, theirs, max(a.runs // 4, 3), 1)
    res["bootstrap_means"] = entry(
        k, t, 4 * N * D + 4 * Bn * D, peak_bytes(ours), peak_bytes(theirs),
        torch_is=f"rows[randint] .mean(1) in chunks of {chunk} replicates",
        gathered_bytes=4 * Bn * N * D,
        gathered_GBps=4 * Bn * N * D / (k["ms_median"] * 1e-3) / 1e9)
    print("bootstrap_means", json.dumps(res["bootstrap_means"]), flush=True)

    # ---- quantiles along dim 1 of [1, Bn, D] (B-strided rows) ---------------------------
    boot = ours()[None].contiguous()
    alpha = 0.1 / D
    qa = (alpha, 1.0 - alpha)
    qat = torch.tensor(qa, device=dev, dtype=torch.float32)

    def ours():
        return calibration.row_summary(boot, dim=1, quantiles=qa)

    def theirs():
        return torch.quantile(boot[0], qat, dim=0)

    diff = float((ours().quantiles[0] - theirs().t()).abs().max())
    k, t = alternate(ours, theirs, a.runs, a.warmup)
    res["row_summary_strided"] = entry(
        k, t, 4 * Bn * D, peak_bytes(ours), peak_bytes(theirs),
        torch_is="torch.quantile(x [Bn,D], 2 levels, dim=0)", max_abs_diff_from_torch=diff,
        note=f"{D} workgroups only: one per column")
    print("row_summary_strided", json.dumps(res["row_summary_strided"]), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


def _hip_lds(N, weighted):
    """LDS bytes of one row_summary workgroup (summary_kernel.hip summary_lds_bytes)."""
    P = max(64, 1 << (N - 1).bit_length())
    threads = min(max(P // 8, 64), 1024)
    return (threads + 24) * 8 + P * (8 if weighted else 4)


if __name__ == "__main__":
    main()
