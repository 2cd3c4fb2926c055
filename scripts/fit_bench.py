"""Times the image-model fit's objective (smcdet_fit_objective through
smcdet_amd.fit.objective) and a whole fit at the shape of the reference's
experiments/m71/m71.ipynb ("Optimize image model parameters"): one 120x160
field, psf_radius 16, a 10-pixel frame and the saturated pixels masked out.
The notebook does not print its star count: 1,000 stars are ASSUMED here
(--stars), uniform over the field padded by 4 px, log-uniform in 1..1000 nmgy.

Next to it the same objective by plain torch autograd on the same device, in
the same process, alternating with it run by run: float64, the dense [H,W,D]
profile tensor and the normaliser's (32R)^2 grid rebuilt and back-propagated
through at every evaluation, as the notebook's cell does.  It returns nll and
its gradient only (no information, no rate image).

    python scripts/fit_bench.py [--out profiles/fit/fit_bench.json]

Every per-call figure is the median (with min and max) of --runs wall-clock
timings of one call up to and including the read-back of its result (what an
L-BFGS closure waits for), after --warmup calls.  A whole fit is
torch.optim.LBFGS (strong Wolfe) with --max-iter iterations per step and
--steps steps over the notebook's nine free parameters from the same start,
--fit-runs times with each closure, alternating, after one untimed fit each
(median, min and max of the wall clock).  No ratio is promised: the file records what was
measured.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smcdet_amd import _hip, fit  # noqa: E402

TRUTH = dict(background=104.1486587524414, adu_per_nmgy=241.02658081054688,
             psf_params=[1.107237458229065, 2.0800251960754395, 2.3254318237304688,
                         5.240590572357178, 0.7346734404563904, 0.5114791393280029],
             noise_additive=1.0000007072408224e-10, noise_multiplicative=1.936462640762329)
F64 = torch.float64


def stats(ms):
    return dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), runs=len(ms))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


class TorchObjective:
    """nll(log_theta) by torch in float64 on the device: the gather formulation
    of include/smcdet_hip.h with a dense [H,W,D] profile tensor."""

    def __init__(self, image, locs, fluxes, mask, R):
        H, W = image.shape
        self.x, self.m, self.f = image.to(F64), mask.to(F64), fluxes.to(F64)
        ph = torch.arange(H, device=image.device, dtype=F64)[:, None, None]
        pw = torch.arange(W, device=image.device, dtype=F64)[None, :, None]
        h, w = locs[:, 0].to(F64), locs[:, 1].to(F64)
        self.r2 = (ph + 0.5 - h) ** 2 + (pw + 0.5 - w) ** 2
        self.inwin = ((ph - torch.floor(h)).abs() <= R) & ((pw - torch.floor(w)).abs() <= R)
        n = 32 * R
        g = torch.arange(n, device=image.device, dtype=F64) - n / 2.0 + 0.5
        self.grid = g[:, None] ** 2 + g[None, :] ** 2

    @staticmethod
    def profile(r2, th):
        s1, s2, sp, beta, b, p0 = (th[k] for k in range(1, 7))
        t = torch.exp(-r2 / (2 * s1)) + b * torch.exp(-r2 / (2 * s2)) \
            + p0 * (1 + r2 / (beta * sp)) ** (-beta / 2)
        return t / (1 + b + p0)

    def nll(self, log_theta):
        th = torch.exp(log_theta)
        C = self.profile(self.grid, th).sum()
        lam = th[9] + th[0] * (self.profile(self.r2, th) * self.inwin * self.f).sum(-1) / C
        v = th[8] + th[7] * lam
        return (self.m * (0.5 * torch.log(2 * math.pi * v) + (self.x - lam) ** 2 / (2 * v))).sum()

    def value_and_grad(self, log_theta_host):
        lt = log_theta_host.to(self.x.device).requires_grad_(True)
        loss = self.nll(lt)
        (g,) = torch.autograd.grad(loss, lt)
        return torch.cat([loss.detach()[None], g]).cpu()  # one read-back


def lbfgs(closure_of, start, idx, max_iter, steps):
    """torch.optim.LBFGS over start[idx] with closure_of(full log_theta) ->
    host tensor [nll, grad[10]]; (nll, evaluations, seconds)."""
    z = start[idx].clone().requires_grad_(True)
    n = [0]
    last = [None]

    def closure():
        lt = start.clone()
        lt[idx] = z.detach()
        out = closure_of(lt)
        n[0] += 1
        z.grad = out[1:11][idx].clone()
        last[0] = float(out[0])
        return out[0]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit.lbfgs_minimise(z, closure, max_iter=max_iter, steps=steps)
    torch.cuda.synchronize()
    return last[0], n[0], time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=120)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--psf-radius", type=int, default=16)
    ap.add_argument("--stars", type=int, default=1000)
    ap.add_argument("--frame", type=int, default=10)
    ap.add_argument("--saturation", type=float, default=20000.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--fit-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "fit", "fit_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    H, W, R, D = a.height, a.width, a.psf_radius, a.stars
    locs = torch.tensor([-4.0, -4.0], device=dev) \
        + torch.tensor([H + 8.0, W + 8.0], device=dev) * torch.rand(1, D, 2, device=dev)
    fluxes = torch.exp(math.log(1000.0) * torch.rand(1, D, device=dev))
    truth = fit.log_theta_of(TRUTH)
    blank = torch.zeros(1, H, W, device=dev)
    rate = fit.objective(blank, locs, fluxes, truth, psf_radius=R, rate=True).rate.double()
    v = TRUTH["noise_additive"] + TRUTH["noise_multiplicative"] * rate
    image = (rate + v.sqrt() * torch.randn_like(rate)).float()
    mask = torch.zeros(1, H, W, dtype=torch.uint8, device=dev)
    mask[:, a.frame:H - a.frame, a.frame:W - a.frame] = 1
    mask &= (image < a.saturation).to(torch.uint8)

    fields = fit._Fields(image, locs, fluxes, R, mask, None, "fit_bench")
    tobj = TorchObjective(image[0], locs[0], fluxes[0], mask[0], R)
    start = truth.clone()
    idx = [fit.PARAM_NAMES.index(nm) for nm in fit.DEFAULT_FREE]
    start[idx] += torch.tensor([0.1, -0.1] * 5)[:len(idx)].double()

    def ours():
        return fields.call(start.tolist())[0].cpu()

    def theirs():
        return tobj.value_and_grad(start)

    o, t = ours(), theirs()
    agree = dict(nll_rel=abs(float(o[0] - t[0])) / abs(float(t[0])),
                 grad_rel=float(((o[1:11] - t[1:]).abs() / t[1:].abs().clamp_min(1e-300)).max()))
    for _ in range(a.warmup):
        ours()
        theirs()
    pairs = [(wall_ms(ours), wall_ms(theirs)) for _ in range(a.runs)]
    k, th = stats([p[0] for p in pairs]), stats([p[1] for p in pairs])
    def fit_ours():
        return lbfgs(lambda lt: fields.call(lt.tolist())[0].cpu(), start, idx, a.max_iter, a.steps)

    def fit_theirs():
        return lbfgs(tobj.value_and_grad, start, idx, a.max_iter, a.steps)

    fit_ours(), fit_theirs()  # untimed: the optimiser's first use
    fits = [(fit_ours(), fit_theirs()) for _ in range(a.fit_runs)]
    fo, ft = fits[0]
    so = stats([1e3 * f[0][2] for f in fits])
    st = stats([1e3 * f[1][2] for f in fits])
    res = dict(device=torch.cuda.get_device_name(0), library=_hip.version(),
               shape=dict(H=H, W=W, psf_radius=R, stars=D, stars_assumed=True, frame=a.frame,
                          saturation_adu=a.saturation, masked_in=int(mask.sum()),
                          profile_evaluations_per_call=int((tobj.inwin.sum())) + (32 * R) ** 2),
               timing="wall clock of one call including the read-back of its result",
               torch_is="float64 autograd through the dense [H,W,D] profile and the (32R)^2 "
                        "normaliser grid; nll and gradient only",
               objective=k, torch_objective=th, torch_over_kernel=th["ms_median"] / k["ms_median"],
               agreement_at_start=agree,
               fit=dict(free=list(fit.DEFAULT_FREE), max_iter=a.max_iter, steps=a.steps,
                        kernel=dict(nll=fo[0], evaluations=fo[1], **so),
                        torch=dict(nll=ft[0], evaluations=ft[1], **st)))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
