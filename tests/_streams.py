"""Host restatement of the Philox streams of the three MCMC sweep kernels
(smcdet_mh_sweep and its step forms, smcdet_mala_sweep, smcdet_mh_chain), as
the replay arrays those kernels take in place of their own draws.

Read from `refill` in smcdet_amd/csrc/mh_kernel.hip, mala_kernel.hip and
chain_kernel.hip, and from philox4x32 / u01 / RngTag in device.h: this file is
the place to change when a kernel's draw layout changes.

Iteration k of particle (or chain) `pid`, seed s, counter base `offset`:

    ctr  = offset + k                                   (64 bits, wraps)
    r0   = philox(ctr_lo, ctr_hi, pid mod 2^32, tag0; key = (s_lo, s_hi))
    r1   = philox(ctr_lo, ctr_hi, pid mod 2^32, tag1; key = (s_lo, s_hi))
    u01  = float32(x >> 8) * 2^-24
    comp = min(int32(u01(r0.x) * float32(Sj)), Sj - 1)  (float32 product)
    uloc = (u01(r0.y), u01(r0.z)),  uflux = u01(r0.w),  uacc = u01(r1.x)

Sj is S, or clip(int(count), 0, S) per particle in the by-count mode of the
two sweeps (the chains always choose among S).  A particle with Sj = 0 makes
no iteration: its `comp` entries are never read and are emitted as 0.

pid = t*N + n (sweeps) or t*C + c (chains), t the row-major tile index; the
arrays are [K,nH,nW,N(,2)] / [K,nH,nW,C(,2)], the layout of the kernels'
replay buffers.  For the chains K = num_samples_total - 1 and `offset` is the
base of the whole run: a chunked run (print_every) continues the counters.
"""
import numpy as np

from tests._calibration_oracle import philox4x32

TAGS = {
    "mh": (0x4D480000, 0x4D480001),
    "mala": (0x4D4C0000, 0x4D4C0001),
    "chain": (0x43480000, 0x43480001),
}
# the names of those constants in device.h's RngTag
TAG_NAMES = {
    "mh": ("kTagMH0", "kTagMH1"),
    "mala": ("kTagMALA0", "kTagMALA1"),
    "chain": ("kTagChain0", "kTagChain1"),
}
_M64 = (1 << 64) - 1


def u01(x):
    """device.h u01: 24 mantissa bits, [0, 1)."""
    return (np.asarray(x, np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def counters(offset, K):
    """(c0, c1) uint64 arrays [K]: low and high words of offset + k."""
    ctr = [(int(offset) + k) & _M64 for k in range(int(K))]
    return (np.array([c & 0xFFFFFFFF for c in ctr], np.uint64),
            np.array([c >> 32 for c in ctr], np.uint64))


def raw(tags, seed, offset, K, pids):
    """(r0, r1): two 4-tuples of uint64 arrays [K, *pids.shape] holding the
    uint32 words of the two Philox calls of every (iteration, pid)."""
    seed = int(seed) & _M64
    pids = np.asarray(pids, np.int64)
    c0, c1 = counters(offset, K)
    ex = (slice(None),) + (None,) * pids.ndim
    c2 = (pids & 0xFFFFFFFF).astype(np.uint64)[None]
    return tuple(philox4x32(c0[ex], c1[ex], c2, tag, seed & 0xFFFFFFFF, seed >> 32)
                 for tag in tags)


def draws(family, seed, offset, K, pids, Sj):
    """The replay arrays of `family` ("mh", "mala", "chain") for the particles
    `pids` (any shape P) with Sj (broadcast to P) selectable components:
    comp [K,*P] int32, uloc [K,*P,2], uflux / uacc [K,*P] float32."""
    pids = np.asarray(pids, np.int64)
    Sj = np.broadcast_to(np.asarray(Sj, np.int32), pids.shape)
    r0, r1 = raw(TAGS[family], seed, offset, K, pids)
    prod = u01(r0[0]) * Sj[None].astype(np.float32)
    assert prod.dtype == np.float32
    comp = np.minimum(prod.astype(np.int32), Sj[None] - 1)
    comp = np.where(Sj[None] > 0, comp, 0).astype(np.int32)
    return dict(comp=np.ascontiguousarray(comp),
                uloc=np.ascontiguousarray(np.stack([u01(r0[1]), u01(r0[2])], -1)),
                uflux=np.ascontiguousarray(u01(r0[3])),
                uacc=np.ascontiguousarray(u01(r1[0])))


def _pids(nH, nW, n):
    return np.arange(nH * nW * n, dtype=np.int64).reshape(nH, nW, n)


def sweep_replay(family, seed, offset, K, nH, nW, N, S, counts=None):
    """Replay arrays [K,nH,nW,N(,2)] of an MH ("mh") or MALA ("mala") sweep.
    counts [nH,nW,N]: the by-count mode (SMCDET_MH_COMPONENT_BY_COUNT)."""
    assert family in ("mh", "mala")
    Sj = S if counts is None else np.clip(np.asarray(counts).astype(np.int32), 0, S)
    return draws(family, seed, offset, K, _pids(nH, nW, N), Sj)


def chain_replay(seed, offset, K, nH, nW, C, S):
    """Replay arrays [K,nH,nW,C(,2)] of MHsampler's chains, K = total - 1."""
    return draws("chain", seed, offset, K, _pids(nH, nW, C), S)
