"""Times smcdet_chain_stats at the shape of the reference's MCMC baseline
(experiments/m71/run_mcmc.py: 332 cutouts, 10,000 kept draws per chain) -- 332
tiles x 3 quantities, C = 4 chains and C = 1, M = 10,000 -- next to the same
quantities by torch on the same device and inputs, in the same process,
alternating with it run by run:

    split chains, float64 means, float32 centered draws,
    torch.fft.rfft / irfft autocovariance over ALL lags (zero-padded to 2n),
    rho, the pairs, and Geyer's cut-off by cumprod / cummin on the device
    (no host loop).

    python scripts/convergence_bench.py [--out profiles/convergence/convergence_bench.json]

The rows are AR(1) chains, one phi per quantity (--phis), so the number of lag
blocks the kernel takes is that of chains thinned to different degrees; it is
reported per phi.  Every figure is the median (with min and max) of --runs
timings by device events around one call, after --warmup calls; peak memory is
torch.cuda.max_memory_allocated over one call beyond what was allocated before
it.  Nothing is promised: the file records what was measured.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, convergence  # noqa: E402


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


def ar1_rows(tiles, phis, C, M, seed=0, burnin=200):
    """[tiles, len(phis), C, M] float32 AR(1) chains (numpy, then to the device)."""
    rng = np.random.default_rng(seed)
    phi = np.asarray(phis, np.float64)[None, :, None]
    prev = np.zeros((tiles, len(phis), C))
    out = np.empty((tiles, len(phis), C, M), np.float32)
    for t in range(M + burnin):
        prev = phi * prev + rng.standard_normal(prev.shape)
        if t >= burnin:
            out[..., t - burnin] = prev
    return torch.from_numpy(out)


def torch_chain_stats(x):
    """(rhat, tau, ess, mcse, n_pairs) of x [R,C,M], split chains, by FFT over
    all lags."""
    R, C, M = x.shape
    n = M // 2
    c = torch.stack([x[..., :n], x[..., M - n:]], dim=2).reshape(R, 2 * C, n)
    m = 2 * C
    mu = c.double().mean(-1)
    d = (c.double() - mu[..., None]).float()
    L = 1 << (2 * n - 1).bit_length()
    f = torch.fft.rfft(d, L, dim=-1)
    acov = torch.fft.irfft(f * f.conj(), L, dim=-1)[..., :n].double() / n   # [R,m,n]
    a0 = acov[..., 0]
    W = a0.mean(-1) * n / (n - 1)
    bn = mu.var(-1, unbiased=True) if m > 1 else torch.zeros_like(W)
    vp = W * (n - 1) / n + bn
    rho = 1.0 - (W[:, None] - acov.mean(1)) / vp[:, None]                    # [R,n]
    rho[:, 0] = 1.0
    K2 = n // 2
    P = rho[:, 0:2 * K2:2] + rho[:, 1:2 * K2:2]
    alive = (P > 0).to(torch.float64).cumprod(-1)
    Pm = torch.cummin(torch.where(alive > 0, P, torch.full_like(P, float("inf"))), -1).values
    s = torch.where(alive > 0, Pm, torch.zeros_like(Pm)).sum(-1)
    tau = torch.clamp(-1.0 + 2.0 * s, min=1.0 / math.log10(m * n))
    ess = m * n / tau
    return torch.sqrt(vp / W), tau, ess, torch.sqrt(vp / ess), alive.sum(-1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=332)
    ap.add_argument("--draws", type=int, default=10000)
    ap.add_argument("--chains", type=int, nargs="+", default=[4, 1])
    ap.add_argument("--phis", type=float, nargs="+", default=[0.3, 0.7, 0.9])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out",
                    default=os.path.join("profiles", "convergence", "convergence_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convergence_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(), runs=a.runs,
               warmup=a.warmup, phis=a.phis, lds_draws=_hip.CHAINS_LDS_DRAWS,
               block_pairs=_hip.CHAINS_BLOCK_PAIRS,
               torch_is="float32 rfft / irfft autocovariance over all lags + cumprod / cummin "
                        "cut-off")
    for C in a.chains:
        x4 = ar1_rows(a.tiles, a.phis, C, a.draws, seed=C).to(dev)
        x = x4.reshape(-1, C, a.draws)
        R = x.shape[0]

        def ours():
            return convergence.chain_stats(x)

        def theirs():
            return torch_chain_stats(x)

        s, t = ours(), theirs()
        blocks = s.lag_blocks.reshape(a.tiles, len(a.phis)).double()
        same_K = float((s.n_pairs == t[4]).double().mean())
        agree = (s.n_pairs == t[4])
        tau_diff = float(((s.tau - t[1]).abs() / s.tau)[agree].max())
        k, th = alternate(ours, theirs, a.runs, a.warmup)
        m, n = s.m, s.n
        entry = dict(
            shape=dict(tiles=a.tiles, quantities=len(a.phis), rows=R, C=C, M=a.draws, m=m, n=n),
            path="LDS" if m * n <= _hip.CHAINS_LDS_DRAWS else "workspace",
            kernel=k, torch=th, torch_over_kernel=th["ms_median"] / k["ms_median"],
            peak_bytes_kernel=peak_bytes(ours), peak_bytes_torch=peak_bytes(theirs),
            input_bytes=4 * R * C * a.draws,
            lag_blocks_mean_per_phi=blocks.mean(0).tolist(),
            lag_blocks_max_per_phi=blocks.max(0).values.tolist(),
            lag_blocks_if_all_lags=-(-((n - 1 + 1) // 2) // _hip.CHAINS_BLOCK_PAIRS),
            n_pairs_mean_per_phi=s.n_pairs.reshape(a.tiles, -1).double().mean(0).tolist(),
            rows_with_equal_cutoff=same_K, max_rel_tau_diff_on_those=tau_diff)
        res[f"C{C}"] = entry
        print(f"C{C}", json.dumps(entry), flush=True)
        del x, x4, s, t
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
