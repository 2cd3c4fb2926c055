"""Times smcdet_forced_photometry (smcdet_amd.photometry's kernel) at the grid
search's shape and at a population's shape, against float64 torch on the same
problems.

    python scripts/photometry_bench.py [--out profiles/photometry/photometry_bench.json]

Grid search: --tiles 8x8 M71 tiles x 2,380 settings (extract_bench.py's grid),
K = 16, the positions smcdet_extract finds: the photometry launch that sits
between the extract and the match launches of extract.tune(flux="psf").
Population: --tiles tiles x --catalogs catalogs of S = 10 slots, counts uniform
in 0..10, positions uniform on the tile and a 1-pixel rim.
Every figure is the median of --runs runs with min-max.  The kernel is timed
alone with the library's launch-timing events (they ride on the kernel's own
dispatch packet).  Torch (a dense design matrix from ImageModel.psf, then
torch.linalg.cholesky_ex / cholesky_solve / cholesky_inverse in float64,
chunked to fit memory) is timed with stream events in the same process,
alternating with the kernel, on --torch-settings of the settings (all tiles);
the kernel is timed on that subset too.  No counters are collected: what
bounds the kernel is worked out from the shapes.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, extract, photometry  # noqa: E402
from smcdet_amd.images import M71ImageModel  # noqa: E402
from tests import _extract_oracle as XO  # noqa: E402
from tests._params import M71  # noqa: E402


def m71_model(H):
    p = M71
    return M71ImageModel(image_height=H, image_width=H, background=p["background"],
                         psf_radius=p["psf_radius"], adu_per_nmgy=p["adu_per_nmgy"],
                         psf_params=p["psf_params"], noise_additive=p["noise_additive"],
                         noise_multiplicative=p["noise_multiplicative"])


def make_tiles(model, T, seed=0, density=0.03):
    """Tiles drawn from the image model itself: Poisson(density * area) stars
    on the tile and a 2-pixel rim, Pareto fluxes (nmgy)."""
    H = model.image_height
    g = torch.Generator().manual_seed(seed)
    S = 12
    n = torch.poisson(torch.full((T,), density * (H + 4) ** 2), generator=g).clamp(max=S)
    locs = torch.rand(T, 1, 1, S, 2, generator=g) * (H + 4) - 2
    fluxes = (1.2 * (1 - torch.rand(T, 1, 1, S, generator=g)) ** (-1 / 0.7)).clamp(max=800.0)
    fluxes = fluxes * (torch.arange(S)[None, None, None, :] < n[:, None, None, None])
    torch.manual_seed(seed)
    images = model.sample(locs.cuda(), fluxes.cuda())  # [T,1,H,W,1]
    return images[:, 0, :, :, 0].contiguous()


def spread(ms):
    return dict(runs=len(ms), ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def kernel_ms(launch):
    _hip.launch_timing(1)
    launch()
    torch.cuda.synchronize()
    ms = _hip.launch_timing_read(1)
    _hip.launch_timing(0)
    assert len(ms) == 1, ms
    return ms[0]


def reductions(n_free, n_iter=4):
    """float64 wave reductions of a problem with P free parameters: per
    iteration P(P+1)/2 matrix entries and P right-hand sides, the information
    once more, and chi2."""
    P = n_free.double()
    tri = P * (P + 1) / 2
    return n_iter * (tri + P) + tri + 1


def torch_photometry(model, images, counts, locs, n_iter=4, chunk=65536, solve_on=None):
    """The definition in float64 torch: images [T,H,W], counts [T,G], locs
    [T,G,K,2].  Returns fluxes, flux_err [T,G,K] (NaN where the kernel gives
    NaN or skips).  Slots that are not solved get a unit row so that the
    batched factorisation stays defined.  solve_on: the device of everything
    after the design matrix (default: the images')."""
    T, G, K = locs.shape[:3]
    H, W = images.shape[1:]
    g, B = float(model.adu_per_nmgy), float(model.background)
    na, nm = float(model.noise_additive), float(model.noise_multiplicative)
    solve_on = images.device if solve_on is None else torch.device(solve_on)
    fl = torch.empty(T, G, K, device=solve_on, dtype=torch.float64)
    er = torch.empty_like(fl)
    failed = 0
    per_tile = max(1, chunk // G)
    for t0 in range(0, T, per_tile):
        t1 = min(T, t0 + per_tile)
        live = torch.arange(K, device=images.device)[None, None, :] < counts[t0:t1, :, None]
        ll = torch.where(live[..., None], locs[t0:t1], torch.full_like(locs[t0:t1], -100.0))
        phi = model.psf(ll[:, None].contiguous())  # [t,1,H,W,G,K]
        D = g * phi[:, 0].permute(0, 3, 1, 2, 4).reshape(-1, H * W, K).to(solve_on).double()
        live = live.reshape(-1, K).to(solve_on) & (D != 0).any(1)
        x = images[t0:t1].reshape(t1 - t0, 1, H * W).expand(-1, G, -1).reshape(-1, H * W) \
            .to(solve_on).double()
        eye = torch.diag_embed((~live).double())
        y = x - B
        v = na + nm * x.clamp_min(B / 4)
        for _ in range(n_iter):
            Dw = D / v[:, :, None]
            A = D.transpose(1, 2) @ Dw + eye
            L = torch.linalg.cholesky_ex(A).L
            th = torch.cholesky_solve((Dw.transpose(1, 2) @ y[:, :, None]), L)[:, :, 0]
            v = na + nm * ((D @ th[:, :, None])[:, :, 0] + B).clamp_min(B / 4)
        info = D.transpose(1, 2) @ (D * (1 / v + nm * nm / (2 * v * v))[:, :, None]) + eye
        fac = torch.linalg.cholesky_ex(info)
        failed += int((fac.info != 0).sum())
        cov = torch.cholesky_inverse(fac.L)
        nan = torch.full_like(th, float("nan"))
        fl[t0:t1] = torch.where(live, th, nan).reshape(t1 - t0, G, K)
        er[t0:t1] = torch.where(live, cov.diagonal(dim1=1, dim2=2).sqrt(), nan).reshape(
            t1 - t0, G, K)
    return fl, er, failed


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1000)
    ap.add_argument("--catalogs", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-settings", type=int, default=238)
    ap.add_argument("--out", default=os.path.join("profiles", "photometry",
                                                  "photometry_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometry_bench.py needs a GPU (nothing is timed on the CPU alone)")
    dev = torch.device("cuda", 0)
    T, H, K = a.tiles, 8, 16
    model = m71_model(H)
    cm = model._cmodel()
    images = make_tiles(model, T)
    bg = float(M71["background"])
    sigma = float(np.sqrt(M71["noise_multiplicative"] * bg))

    # ---- the grid search's shape ----------------------------------------------------
    grid = (np.arange(1.0, 9.5, 0.5), np.arange(1, 8), np.logspace(-10, -2, 5),
            np.logspace(-1, 2, 4))
    settings = torch.from_numpy(XO.settings_grid(*grid))
    G = settings.shape[0]
    d_bg, d_sigma = torch.full((T,), bg, device=dev), torch.full((T,), sigma, device=dev)
    ext_ms = []
    for i in range(3 + 1):
        ms = kernel_ms(lambda: extract._launch(images, d_bg, d_sigma, settings, 64, K, False))
        if i:
            ext_ms.append(ms)
    counts, locs, _, _, _ = extract._launch(images, d_bg, d_sigma, settings, 64, K, False)
    out = {}

    def launch_grid():
        out["grid"] = photometry._launch(images, counts, locs, cm, None, 4, False, False)

    pick = torch.linspace(0, G - 1, min(G, a.torch_settings)).long().to(dev)
    c_sub, l_sub = counts[:, pick].contiguous(), locs[:, pick].contiguous()

    def launch_sub():
        out["sub"] = photometry._launch(images, c_sub, l_sub, cm, None, 4, False, False)

    for _ in range(a.warmup):
        launch_grid()
        launch_sub()
        torch_photometry(model, images, c_sub, l_sub)
    torch.cuda.synchronize()
    grid_ms, sub_ms, torch_ms = [], [], []
    for _ in range(a.runs):  # alternating, in one process
        grid_ms.append(kernel_ms(launch_grid))
        sub_ms.append(kernel_ms(launch_sub))
        ms, tres = event_ms(lambda: torch_photometry(model, images, c_sub, l_sub))
        torch_ms.append(ms)
    p = out["grid"]
    red = reductions(p.n_free)
    res_grid = dict(T=T, H=H, W=H, G=G, K=K, problems=T * G, n_iter=4, **spread(grid_ms))
    med = res_grid["ms_median"]
    res_grid.update(
        ns_per_problem=1e6 * med / (T * G),
        mean_free_parameters=float(p.n_free.double().mean()),
        max_free_parameters=int(p.n_free.max()),
        problems_singular=int((p.status & 2).ne(0).sum()),
        problems_with_dropped_source=int((p.status & 1).ne(0).sum()),
        mean_wave_reductions_per_problem=float(red.mean()),
        bytes_read=4 * T * H * H + T * G * (4 + 8 * K),
        bytes_written=T * G * (16 * K + 16 + 12),
        extract_launch=spread(ext_ms))
    res_grid["GB_per_s"] = (res_grid["bytes_read"] + res_grid["bytes_written"]) / (med * 1e6)
    print("grid", json.dumps(res_grid), flush=True)

    def agreement(ps, tf, te):
        both = torch.isfinite(ps.flux_err) & torch.isfinite(tf)
        z = ((ps.fluxes - tf).abs() / ps.flux_err)[both]
        return dict(sources_solved_by_both=int(both.sum()),
                    sources_solved_by_one=int((torch.isfinite(ps.flux_err)
                                               ^ torch.isfinite(tf)).sum()),
                    max_flux_difference_in_flux_err=float(z.max()) if z.numel() else None,
                    max_rel_flux_err_difference=float(
                        ((ps.flux_err - te).abs() / ps.flux_err)[both].max())
                    if z.numel() else None)

    ps, (tf, te, tfail) = out["sub"], tres
    # the same float64 torch code with its linear algebra on the host, on a few tiles
    nt = min(T, 8)
    hf, he, hfail = torch_photometry(model, images[:nt], c_sub[:nt], l_sub[:nt], solve_on="cpu")
    host = agreement(photometry.Photometry(*(None if x is None else x[:nt].cpu() for x in ps)),
                     hf, he)
    host.update(tiles=nt, factorisations_failed=hfail)
    res_torch = dict(settings=int(pick.numel()), problems=T * int(pick.numel()),
                     kernel=spread(sub_ms), torch_float64=spread(torch_ms),
                     speedup=statistics.median(torch_ms) / statistics.median(sub_ms),
                     **agreement(ps, tf, te), factorisations_failed=tfail,
                     torch_solving_on_the_host=host,
                     note="factorisations_failed: information matrices for which torch's "
                          "batched float64 cholesky_ex reported info != 0 (with the linear "
                          "algebra on the device, and with the same code on the host); a "
                          "comparison is meaningful where none failed.  torch has no "
                          "unit-diagonal scaling and no pivot rule, so a problem the kernel "
                          "calls singular may come out finite there (solved by one)")
    print("torch", json.dumps(res_torch), flush=True)
    del out["grid"], out["sub"], p, ps, tres, tf, te, counts, locs, hf, he

    # ---- a population's shape -------------------------------------------------------
    N, S = a.catalogs, 10
    g = torch.Generator(device=dev).manual_seed(1)
    pc = torch.randint(0, S + 1, (T, N), generator=g, device=dev, dtype=torch.int32)
    pl = torch.rand(T, N, S, 2, generator=g, device=dev) * (H + 2) - 1
    pm = []

    def launch_pop():
        out["pop"] = photometry._launch(images, pc, pl, cm, None, 4, False, False)

    for _ in range(a.warmup):
        launch_pop()
    for _ in range(a.runs):
        pm.append(kernel_ms(launch_pop))
    p = out["pop"]
    res_pop = dict(T=T, N=N, S=S, H=H, W=H, problems=T * N, n_iter=4, **spread(pm))
    med = res_pop["ms_median"]
    res_pop.update(ns_per_problem=1e6 * med / (T * N),
                   mean_free_parameters=float(p.n_free.double().mean()),
                   problems_singular=int((p.status & 2).ne(0).sum()),
                   mean_wave_reductions_per_problem=float(reductions(p.n_free).mean()),
                   bytes_read=4 * T * H * H + T * N * (4 + 8 * S),
                   bytes_written=T * N * (16 * S + 16 + 12))
    res_pop["GB_per_s"] = (res_pop["bytes_read"] + res_pop["bytes_written"]) / (med * 1e6)
    print("population", json.dumps(res_pop), flush=True)

    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(), grid_search=res_grid,
               torch_comparison=res_torch, population=res_pop, counters="none collected")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
