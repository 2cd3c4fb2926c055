"""Times smcdet_match_catalogs (smcdet_amd.metrics.match_catalogs' kernel) on
the shape the reference's m71synthetic notebook scores, and the CPU oracle
(tests/_metrics_oracle.py, float64 scipy) on a slice of the same problems.

    python scripts/metrics_bench.py [--out profiles/metrics/metrics_bench.json]

Two kernel shapes, each timed alone with the library's launch-timing events
(smcdet_launch_timing: the events ride on the kernel's own dispatch packet),
median of --launches launches after --warmup:
  full       T=1000 tiles, N=10,000 catalogs, S=10, B=17, every catalog matched
  subsample  the same data, M=200 catalogs per tile (the reference's choice)
The CPU figure is one core on --cpu-problems of those problems.  Bytes are
computed from the shapes: the catalogs, counts and index the kernel reads and
the four [T,M,B] arrays it writes.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip  # noqa: E402
from smcdet_amd._hip import check, lib, ptr, stream_of  # noqa: E402
from tests import _metrics_oracle as O  # noqa: E402


def make_data(T, N, S, frame, dev, seed=0, chunk=50):
    """A truth per tile and N catalogs built from it on the device: each true
    source kept with probability 0.8 and jittered (0.25 px, 0.3 mag), empty
    slots filled with a uniform spurious source with probability 0.1, kept
    sources compacted to the front (smcdet_prune's layout)."""
    g = torch.Generator(device=dev).manual_seed(seed)

    def rand(*shape):
        return torch.rand(*shape, device=dev, generator=g)

    def randn(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    tc = torch.randint(0, S + 1, (T,), device=dev, generator=g, dtype=torch.int32)
    tl = rand(T, S, 2) * frame
    tm = 17.0 + 5.0 * rand(T, S)
    tf = 10 ** ((22.5 - tm) / 2.5)
    ec = torch.empty(T, N, device=dev, dtype=torch.int32)
    el = torch.empty(T, N, S, 2, device=dev)
    ef = torch.empty(T, N, S, device=dev)
    slot = torch.arange(S, device=dev)
    for a in range(0, T, chunk):
        b = min(a + chunk, T)
        real = (slot[None, None, :] < tc[a:b, None, None]) & (rand(b - a, N, S) < 0.8)
        spur = ~real & (rand(b - a, N, S) < 0.1)
        locs = torch.where(real[..., None], tl[a:b, None] + 0.25 * randn(b - a, N, S, 2),
                           rand(b - a, N, S, 2) * frame)
        mags = torch.where(real, tm[a:b, None] + 0.3 * randn(b - a, N, S),
                           17.0 + 5.0 * rand(b - a, N, S))
        valid = real | spur
        order = torch.argsort((~valid).to(torch.int8), dim=-1, stable=True)
        ec[a:b] = valid.sum(-1).to(torch.int32)
        el[a:b] = torch.gather(locs, 2, order[..., None].expand(-1, -1, -1, 2))
        ef[a:b] = torch.gather(10 ** ((22.5 - mags) / 2.5), 2, order)
    return tc, tl, tf, ec, el, ef


def time_kernel(data, index, M, bins, tols, launches, warmup):
    tc, tl, tf, ec, el, ef = data
    T, N, S = ef.shape
    B = bins.numel()
    outs = [torch.zeros(T, M, B, device=tl.device) for _ in range(4)]

    def launch():
        check(lib().smcdet_match_catalogs(
            ptr(tc), ptr(tl), ptr(tf), ptr(ec), ptr(el), ptr(ef), ptr(index), T, N, M, S, S,
            tols[0], tols[1], ptr(bins), B, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
            ptr(outs[3]), None, stream_of(tl)), "smcdet_match_catalogs")

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    _hip.launch_timing(launches)
    for _ in range(launches):
        launch()
    torch.cuda.synchronize()
    ms = _hip.launch_timing_read(launches)
    _hip.launch_timing(0)
    assert len(ms) == launches, ms
    # bytes by shape: the counted est slots (locs + flux) of every matched
    # catalog, its count and index entry, the truth per problem, the outputs
    idx = index
    est_sources = int((ec.gather(1, idx) if idx is not None else ec).sum())
    true_sources = int(tc.sum()) * M
    read = 12 * (est_sources + true_sources) + T * M * (4 + 4 + (8 if idx is not None else 0))
    written = 4 * T * M * B * 4
    med = statistics.median(ms)
    return dict(T=T, N=N, M=M, S=S, B=B, problems=T * M, launches=launches, warmup=warmup,
                kernel_ms_median=med, kernel_ms_min=min(ms), kernel_ms_max=max(ms),
                ns_per_problem=1e6 * med / (T * M), problems_per_s=T * M / (med * 1e-3),
                bytes_read=read, bytes_written=written,
                achieved_GBps=(read + written) / (med * 1e-3) / 1e9,
                input_array_bytes=int(el.numel() + ef.numel() + ec.numel()) * 4), outs


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--catalogs", type=int, default=10000)
    ap.add_argument("--sources", type=int, default=10)
    ap.add_argument("--subsample", type=int, default=200)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-problems", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join("profiles", "metrics", "metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py needs a GPU (nothing is timed on the CPU alone)")
    dev = torch.device("cuda", 0)
    T, N, S = a.tiles, a.catalogs, a.sources
    bins = torch.arange(16, 24.5, 0.5).to(dev)
    tols = (0.5, 0.5)
    data = make_data(T, N, S, 8.0, dev)
    full, outs = time_kernel(data, None, N, bins, tols, a.launches, a.warmup)
    print("full", json.dumps(full), flush=True)

    # the CPU oracle on the first problems of the full run, one core
    per_tile = min(N, 200)
    tiles = max(1, min(T, a.cpu_problems // per_tile))
    host = [x[:tiles].cpu().numpy() for x in data[:3]] + \
           [x[:tiles, :per_tile].cpu().numpy() for x in data[3:]]
    torch.set_num_threads(1)
    index = np.tile(np.arange(per_tile), (tiles, 1))
    t0 = time.perf_counter()
    want = O.match_catalogs(*host, index, tols[0], tols[1], bins.cpu().numpy())
    cpu_s = time.perf_counter() - t0
    got = [o[:tiles, :per_tile].cpu().numpy() for o in outs]
    differ = int((~np.logical_and.reduce([(g == w).all(-1) for g, w in zip(got, want)])).sum())
    cpu = dict(problems=tiles * per_tile, seconds=cpu_s,
               us_per_problem=1e6 * cpu_s / (tiles * per_tile), threads=1,
               problems_differing_from_kernel=differ,
               note="random data without decision margins: a differing problem is a float32 "
                    "threshold or near-tie, not an error by itself")
    print("cpu_oracle", json.dumps(cpu), flush=True)
    del outs

    g = torch.Generator().manual_seed(0)
    M = min(a.subsample, N)
    index = torch.stack([torch.randint(0, N, [M], generator=g) for _ in range(T)]).to(dev)
    sub, _ = time_kernel(data, index, M, bins, tols, a.launches, a.warmup)
    print("subsample", json.dumps(sub), flush=True)

    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(),
               full=full, subsample=sub, cpu_oracle=cpu,
               speedup_per_problem_vs_cpu_oracle=cpu["us_per_problem"] * 1e3
               / full["ns_per_problem"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
