"""Times the three condense kernels (smcdet_source_map, smcdet_map_peaks,
smcdet_seed_moments) and the whole `smcdet_amd.condense.condense` call at the
shape of the reference's m71synthetic notebook: 1000 tiles of 8x8 with 2 px of
padding, N = 10,000 catalogs, S = 10, 4 cells per pixel (a 48x48 grid).

    python scripts/condense_bench.py [--out profiles/condense/condense_bench.json]

Each kernel is timed alone with the library's launch-timing events (they ride
on the kernel's own dispatch packet), median of --launches launches after
--warmup; the whole call with torch events around it.  Beside them, on the
same device and inputs: the same map by torch scatter-add
(`index_put_(accumulate=True)` and `bincount`, with and without the time to
form the cell indices) and the same moments by torch gather + masked float64
sums, both checked against the kernels' outputs.  Bytes are computed from the
shapes and the counts of counted / matched sources.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, condense, metrics  # noqa: E402

BOX = (-2.0, -2.0, 10.0, 10.0)
TILE = 8.0


def make_data(T, N, S, dev, seed=0, chunk=50):
    """Per tile 0..S true stars on the 8x8 tile; each catalog keeps a star with
    the star's own probability (uniform in 0.2..1) jittered by 0.1 px and 5 %
    in flux, fills an empty slot with a source uniform in the padded box with
    probability 0.05, and compacts the kept slots to the front."""
    g = torch.Generator(device=dev).manual_seed(seed)

    def rand(*shape):
        return torch.rand(*shape, device=dev, generator=g)

    def randn(*shape):
        return torch.randn(*shape, device=dev, generator=g)

    tc = torch.randint(0, S + 1, (T,), device=dev, generator=g)
    tl = rand(T, S, 2) * TILE
    tf = 10 ** (0.4 * (5.5 * rand(T, S)))  # 1..158
    tp = 0.2 + 0.8 * rand(T, S)
    ec = torch.empty(T, N, device=dev, dtype=torch.int32)
    el = torch.empty(T, N, S, 2, device=dev)
    ef = torch.empty(T, N, S, device=dev)
    slot = torch.arange(S, device=dev)
    for a in range(0, T, chunk):
        b = min(a + chunk, T)
        real = (slot[None, None, :] < tc[a:b, None, None]) & (rand(b - a, N, S) < tp[a:b, None])
        spur = ~real & (rand(b - a, N, S) < 0.05)
        locs = torch.where(real[..., None], tl[a:b, None] + 0.1 * randn(b - a, N, S, 2),
                           BOX[0] + rand(b - a, N, S, 2) * (BOX[2] - BOX[0]))
        flux = torch.where(real, tf[a:b, None] * (1 + 0.05 * randn(b - a, N, S)),
                           1.0 + 50.0 * rand(b - a, N, S))
        valid = real | spur
        order = torch.argsort((~valid).to(torch.int8), dim=-1, stable=True)
        ec[a:b] = valid.sum(-1).to(torch.int32)
        el[a:b] = torch.gather(locs, 2, order[..., None].expand(-1, -1, -1, 2))
        ef[a:b] = torch.gather(flux, 2, order)
    return ec, el, ef


def stats(ms):
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), runs=len(ms))


def time_kernel(launch, launches, warmup):
    """Durations of the library launches inside `launch` (one per call)."""
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
    return stats(ms)


def time_torch(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(runs)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--catalogs", type=int, default=10000)
    ap.add_argument("--sources", type=int, default=10)
    ap.add_argument("--cells-per-pixel", type=int, default=4)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "condense", "condense_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("condense_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    T, N, S, c = a.tiles, a.catalogs, a.sources, a.cells_per_pixel
    counts, locs, fluxes = make_data(T, N, S, dev)
    G = int((BOX[2] - BOX[0]) * c)
    cells = G * G
    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(),
               shape=dict(T=T, N=N, S=S, cells_per_pixel=c, grid=[G, G], box=list(BOX)))

    # ---- the map -----------------------------------------------------------------
    smap = condense.source_map(counts, locs, fluxes, box=BOX, cells_per_pixel=c)
    n_counted = int(smap.count.double().sum() + smap.outside.double().sum())
    kern = time_kernel(lambda: condense.source_map(counts, locs, fluxes, box=BOX,
                                                   cells_per_pixel=c), a.launches, a.warmup)
    call = time_torch(lambda: condense.source_map(counts, locs, fluxes, box=BOX,
                                                  cells_per_pixel=c), a.launches, a.warmup)
    want_blocks = -(-4096 // T)
    chunk_len = max(256, -(-N // want_blocks))
    blocks = T * -(-N // chunk_len)
    read = 4 * T * N + 12 * n_counted
    kern.update(call_with_memsets_and_allocation=call, counted_sources=n_counted,
                workgroups=blocks, bytes_read=read, lds_adds=n_counted,
                global_atomic_bytes_at_most=4 * blocks * cells,
                read_GBps=read / (kern["ms_median"] * 1e-3) / 1e9,
                atomic_GBps_at_most=4 * blocks * cells / (kern["ms_median"] * 1e-3) / 1e9)
    res["source_map_kernel"] = kern
    print("source_map", json.dumps(kern), flush=True)

    # torch: the same map by scatter-add
    def cell_index():
        ok = (torch.arange(S, device=dev)[None, None] < counts.clamp(0, S)[..., None]) & \
            torch.isfinite(locs).all(-1) & torch.isfinite(fluxes) & (fluxes > 0)
        ij = torch.floor((locs - BOX[0]) * float(c))
        ok &= (ij >= 0).all(-1) & (ij < G).all(-1)
        t = torch.arange(T, device=dev)[:, None, None].expand(T, N, S)
        return (t[ok] * cells + ij[..., 0][ok].long() * G + ij[..., 1][ok].long())

    idx = cell_index()
    ones = torch.ones(idx.numel(), device=dev)

    def scatter():
        return torch.zeros(T * cells, device=dev).index_put_((idx,), ones, accumulate=True)

    same = bool(torch.equal(scatter().view(T, G, G), smap.count))
    tm = dict(index_put_scatter_only=time_torch(scatter, a.launches, a.warmup),
              bincount_scatter_only=time_torch(
                  lambda: torch.bincount(idx, minlength=T * cells), a.launches, a.warmup),
              cell_index_and_index_put=time_torch(
                  lambda: torch.zeros(T * cells, device=dev).index_put_(
                      (cell_index(),), ones, accumulate=True), 5, 1),
              equals_kernel=same, index_bytes=8 * idx.numel())
    res["source_map_torch"] = tm
    res["source_map_speedup_vs_index_put_scatter_only"] = \
        tm["index_put_scatter_only"]["ms_median"] / kern["ms_median"]
    res["source_map_speedup_vs_cell_index_and_index_put"] = \
        tm["cell_index_and_index_put"]["ms_median"] / kern["ms_median"]
    print("source_map_torch", json.dumps(tm), flush=True)
    del idx, ones

    # ---- the peaks ---------------------------------------------------------------
    K = min(64, 2 * S)
    seeds = condense.find_seeds(smap)
    pk = time_kernel(lambda: condense.find_seeds(smap), a.launches, a.warmup)
    pk.update(K=K, seeds_found=int(seeds.n_seeds.sum()), bytes_read=4 * T * cells,
              read_GBps=4 * T * cells / (pk["ms_median"] * 1e-3) / 1e9)
    res["map_peaks_kernel"] = pk
    print("map_peaks", json.dumps(pk), flush=True)

    # ---- the moments -------------------------------------------------------------
    match = metrics.match_catalogs(seeds.n_seeds, seeds.locs, torch.ones_like(seeds.mass),
                                   counts, locs, fluxes, None, 0.75,
                                   float(torch.finfo(torch.float32).max), torch.zeros(1),
                                   return_matches=True)[4]
    mom, mflux = condense.seed_moments(match, locs, fluxes, seeds.locs)
    n_matched = int((match >= 0).sum())
    mk = time_kernel(lambda: condense.seed_moments(match, locs, fluxes, seeds.locs), a.launches,
                     a.warmup)
    moved = 4 * T * N * K + 12 * n_matched + 4 * T * N * K
    mk.update(K=K, matched_sources=n_matched, bytes_read=4 * T * N * K + 12 * n_matched,
              bytes_written=4 * T * N * K + 80 * T * K, GBps=moved / (mk["ms_median"] * 1e-3) / 1e9)
    res["seed_moments_kernel"] = mk
    print("seed_moments", json.dumps(mk), flush=True)

    def torch_moments():
        ok = match >= 0
        slot = match.clamp_min(0).long()
        h = locs[..., 0].gather(2, slot).double() - seeds.locs[:, None, :, 0].double()
        w = locs[..., 1].gather(2, slot).double() - seeds.locs[:, None, :, 1].double()
        f = fluxes.gather(2, slot).double()
        mag = 22.5 - 2.5 * torch.log10(f)
        zero = torch.zeros((), device=dev, dtype=torch.float64)
        cols = [ok.double(), h, w, h * h, w * w, h * w, f, f * f, mag, mag * mag]
        return torch.stack([torch.where(ok, x, zero).sum(1) for x in cols], -1)

    tmom = torch_moments()
    rel = float(((tmom - mom).abs() / mom.abs().clamp_min(1e-300)).nan_to_num(0).max())
    tmm = time_torch(torch_moments, 5, 1)
    tmm.update(max_rel_diff_from_kernel=rel)
    res["seed_moments_torch"] = tmm
    res["seed_moments_speedup_vs_torch"] = tmm["ms_median"] / mk["ms_median"]
    print("seed_moments_torch", json.dumps(tmm), flush=True)
    del tmom, mflux, match

    # ---- the whole call ----------------------------------------------------------
    whole = time_torch(lambda: condense.condense(counts, locs, fluxes, box=BOX,
                                                 cells_per_pixel=c), a.launches, 1)
    cat = condense.condense(counts, locs, fluxes, box=BOX, cells_per_pixel=c)
    whole.update(detections_above_half=int((cat.prob >= 0.5).sum()),
                 expected_count_mean=float(cat.expected_count.mean()),
                 unassociated_mean=float(cat.unassociated.mean()))
    res["condense_call"] = whole
    print("condense", json.dumps(whole), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
