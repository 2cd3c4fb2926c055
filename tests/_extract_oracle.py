"""numpy restatement of smcdet_extract's definition (include/smcdet_hip.h): the
float32 detection values and threshold ladder op by op, everything else in
float64.  Components come from scipy.ndimage.label with the 3x3 structure, an
independent route to the labels the kernel gets by index propagation.

Besides the outputs every problem returns two margins, the smallest relative
distance |lhs - rhs| / max(|lhs|, |rhs|) of
  * a significance comparison (excess flux against deblend_cont * F_root),
  * a comparison of the clean rule (and of the 1/144 test of the moments),
so that a test can require that no decision of a case hangs on the last bits
of a float64 sum, whose order the device is free to choose.
"""
import math
from types import SimpleNamespace

import numpy as np
from scipy import ndimage

F32, F64 = np.float32, np.float64
S8 = np.ones((3, 3), dtype=int)
U = 100.0 * np.pi


def components(mask):
    """8-connected components of a [H,W] bool mask as sorted flat-index arrays,
    ordered by their smallest index."""
    lab, n = ndimage.label(mask, structure=S8)
    flat = lab.ravel()
    comps = [np.flatnonzero(flat == i + 1) for i in range(n)]
    return sorted(comps, key=lambda c: c[0])


def ladder(peak, tau, n):
    """tau_0 .. tau_{n-1}, float32 op by op."""
    q = F32(peak) / F32(tau)
    for _ in range(int(math.log2(n))):
        q = np.sqrt(q, dtype=F32)
    taus = [F32(tau)]
    for _ in range(1, n):
        taus.append(F32(taus[-1] * q))
    return taus


def _rel(a, b):
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 else np.inf


class _Margins:
    def __init__(self):
        self.sig = np.inf
        self.clean = np.inf


def _leaves(root, vf, vd, H, W, tau, n, cont, mg):
    taus = ladder(vf[root].max(), tau, n)
    f_root = vd[root].sum()
    rhs = F64(cont) * f_root
    out = []

    def descend(pix, k):  # pix: a significant node of level k
        if k + 1 >= n:
            out.append(pix)
            return
        mask = np.zeros(H * W, dtype=bool)
        mask[pix[vf[pix] > taus[k + 1]]] = True
        sig = []
        for c in components(mask.reshape(H, W)):
            ex = (vd[c] - F64(taus[k + 1])).sum()
            mg.sig = min(mg.sig, _rel(ex, rhs))
            if ex > rhs:
                sig.append(c)
        if not sig:
            out.append(pix)
        for c in sig:
            descend(c, k + 1)

    descend(root, 0)
    return out


def _gather(root, leaves, vf, H, W):
    leaves = sorted(leaves, key=lambda c: c.min())
    label = np.full(H * W, -1, dtype=int)
    for i, c in enumerate(leaves):
        label[c] = i
    in_root = np.zeros(H * W, dtype=bool)
    in_root[root] = True
    while True:
        todo = [p for p in root if label[p] < 0]
        if not todo:
            break
        new = label.copy()
        for p in todo:
            i, j = divmod(int(p), W)
            best = None
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    ii, jj = i + di, j + dj
                    if (di or dj) and 0 <= ii < H and 0 <= jj < W:
                        pn = ii * W + jj
                        if in_root[pn] and label[pn] >= 0:
                            key = (-vf[pn], label[pn])
                            if best is None or key < best:
                                best = key
            if best is not None:
                new[p] = best[1]
        label = new
    return [np.flatnonzero(label == i) for i in range(len(leaves))]


def _stats(pix, vf, vd, W, tau, minarea, mg):
    x = vd[pix]
    h = (pix // W) + 0.5
    w = (pix % W) + 0.5
    F = x.sum()
    hb, wb = (x * h).sum() / F, (x * w).sum() / F
    hh = (x * h * h).sum() / F - hb * hb
    ww = (x * w * w).sum() / F - wb * wb
    hw = (x * h * w).sum() / F - hb * wb
    det = hh * ww - hw * hw
    mg.clean = min(mg.clean, _rel(det, 1.0 / 144.0))
    if det < 1.0 / 144.0:
        hh += 1.0 / 12.0
        ww += 1.0 / 12.0
    d = hh * ww - hw * hw
    a = math.sqrt((hh + ww) / 2 + math.sqrt(((hh - ww) / 2) ** 2 + hw * hw))
    mth = 0.0
    if len(pix) >= minarea:
        mth = F64(np.sort(vf[pix])[::-1][minarea - 1]) - F64(tau)
    return SimpleNamespace(pix=pix, F=F, h=hb, w=wb, a=a, chh=ww / d, cww=hh / d, chw=-2 * hw / d,
                           npix=len(pix), mth=mth, first=int(pix.min()))


def _absorbs(j, i, tau, beta, mg):
    def lt(a, b):
        mg.clean = min(mg.clean, _rel(a, b))
        return a < b

    dh, dw = i.h - j.h, i.w - j.w
    if not lt(dh * dh + dw * dw, 100.0 * (i.a + j.a) ** 2):
        return False
    amp = j.F / (2 * U)
    if not lt(F64(tau), amp):
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = (np.power(amp / F64(tau), 1.0 / beta) - 1.0) * U / j.npix
        val = 1.0 + alpha * (j.chh * dh * dh + j.cww * dw * dw + j.chw * dh * dw)
        if not (lt(1.0, val) and lt(val, 1e10)):
            return False
        return lt(i.mth, amp * np.power(val, -beta))


def extract_one(image, background, sigma, thresh, minarea=5, deblend_nthresh=32,
                deblend_cont=0.005, clean_param=1.0, K=16):
    """One problem.  Returns count, n_found, locs [K,2] / fluxes [K] float32
    (NaN / 0 past the count), flux64 / locs64 (all survivors, float64),
    segmap [H,W] int32 and the two margins."""
    image = np.asarray(image, dtype=F32)
    H, W = image.shape
    mg = _Margins()
    v = image - F32(background)
    tau = F32(thresh) * F32(sigma)
    cont, beta = F64(F32(deblend_cont)), F64(F32(clean_param))
    objects = []
    if np.isfinite(tau) and tau > 0:
        vf = v.ravel()
        vd = vf.astype(F64)
        with np.errstate(invalid="ignore"):
            above = v > tau
        for root in components(above):
            if len(root) < minarea:
                continue
            leaves = _leaves(root, vf, vd, H, W, tau, int(deblend_nthresh), cont, mg)
            sets = [root] if len(leaves) == 1 else _gather(root, leaves, vf, H, W)
            objects += [_stats(s, vf, vd, W, tau, int(minarea), mg) for s in sets]
        if beta > 0:
            objects.sort(key=lambda o: (-o.F, o.first))
            owner = list(range(len(objects)))
            for i in range(1, len(objects)):
                for j in range(i):
                    if owner[j] == j and _absorbs(objects[j], objects[i], tau, beta, mg):
                        owner[i] = j
                        break
            merged = []
            for j, o in enumerate(objects):
                if owner[j] == j:
                    pix = np.sort(np.concatenate([objects[i].pix for i in range(len(objects))
                                                  if owner[i] == j]))
                    x = vd[pix]
                    F = x.sum()
                    merged.append(SimpleNamespace(
                        pix=pix, F=F, h=(x * ((pix // W) + 0.5)).sum() / F,
                        w=(x * ((pix % W) + 0.5)).sum() / F, first=int(pix.min())))
            objects = merged
        objects.sort(key=lambda o: (-o.F, o.first))
    n = len(objects)
    locs = np.full((K, 2), np.nan, dtype=F32)
    fluxes = np.zeros(K, dtype=F32)
    seg = np.zeros(H * W, dtype=np.int32)
    for r, o in enumerate(objects):
        seg[o.pix] = r + 1
        if r < K:
            fluxes[r] = F32(o.F)
            locs[r] = (F32(o.h), F32(o.w))
    return SimpleNamespace(
        count=min(n, K), n_found=n, locs=locs, fluxes=fluxes, segmap=seg.reshape(H, W),
        flux64=np.array([o.F for o in objects], dtype=F64),
        locs64=np.array([(o.h, o.w) for o in objects], dtype=F64).reshape(n, 2),
        sig_margin=mg.sig, clean_margin=mg.clean)


def settings_grid(thresh, minarea, deblend_cont, clean_param):
    """[G,4] float64: the Cartesian product in this order, last axis fastest."""
    return np.array([(a, b, c, d) for a in thresh for b in minarea for c in deblend_cont
                     for d in clean_param], dtype=F64)


def extract_grid(images, background, sigma, settings, deblend_nthresh=32, K=16):
    """All problems of images [T,H,W] x settings [G,4]; stacked outputs."""
    images = np.asarray(images, dtype=F32)
    T = images.shape[0]
    background = np.broadcast_to(np.asarray(background, dtype=F32), (T,))
    sigma = np.broadcast_to(np.asarray(sigma, dtype=F32), (T,))
    res = [[extract_one(images[t], background[t], sigma[t], s[0], int(s[1]), deblend_nthresh,
                        s[2], s[3], K) for s in settings] for t in range(T)]

    def stack(name):
        return np.array([[getattr(r, name) for r in row] for row in res])

    return SimpleNamespace(
        counts=stack("count").astype(np.int32), n_found=stack("n_found").astype(np.int32),
        locs=stack("locs"), fluxes=stack("fluxes"), segmap=stack("segmap"),
        sig_margin=stack("sig_margin"), clean_margin=stack("clean_margin"), problems=res)
