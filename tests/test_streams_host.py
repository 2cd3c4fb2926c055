"""tests/_streams.py, the host restatement of the sweep kernels' Philox
streams (the replay arrays test_gpu_streams.py feeds the replay twins): its
constants against device.h, the value ranges, the 64-bit counter, the
separation of pids / offsets / tags and the continuation of a stream."""
import os
import re

import numpy as np
import pytest

from tests import _streams as ST
from tests._calibration_oracle import philox4x32

DEVICE_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smcdet_amd", "csrc",
                        "device.h")
FAMILIES = ("mh", "mala", "chain")
SEED = 0x1234_5678_9ABC_DEF0  # both key words non-zero and different


def _device_tags():
    tags = re.findall(r"(kTag\w+) = (0x[0-9a-f]+)u", open(DEVICE_H).read())
    assert len(tags) >= 15
    return {k: int(v, 16) for k, v in tags}


def test_tags_equal_device_h():
    dev = _device_tags()
    for fam in FAMILIES:
        for name, val in zip(ST.TAG_NAMES[fam], ST.TAGS[fam]):
            assert dev[name] == val, name


def test_sweep_tags_are_distinct_from_every_other_tag():
    dev = _device_tags()
    ours = {n for fam in FAMILIES for n in ST.TAG_NAMES[fam]}
    assert len(ours) == 6 and ours <= set(dev)
    vals = [ST.TAGS[fam][i] for fam in FAMILIES for i in (0, 1)]
    assert len(set(vals)) == 6
    others = {v for k, v in dev.items() if k not in ours}
    assert not set(vals) & others


def test_philox_known_answer():
    """Random123's known-answer vectors for Philox4x32-10 (kat_vectors): the
    generator under the streams is the published one."""
    got = philox4x32(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = philox4x32(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(x) for x in got] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("family", FAMILIES)
def test_uniforms_are_24_bit_fractions_in_unit_interval(family):
    d = ST.draws(family, SEED, 0, 200, np.arange(48).reshape(2, 24), 7)
    for k in ("uloc", "uflux", "uacc"):
        u = d[k]
        assert u.dtype == np.float32
        assert (u >= 0).all() and (u < 1).all()
        scaled = u.astype(np.float64) * 2.0 ** 24
        assert (scaled == np.floor(scaled)).all()
    # the top of the range is reached by the restated u01, and stays below 1
    assert ST.u01(0xFFFFFFFF) == np.float32(1 - 2.0 ** -24)
    assert ST.u01(0xFF) == 0 and ST.u01(0x100) == np.float32(2.0 ** -24)


@pytest.mark.parametrize("family", FAMILIES)
def test_comp_in_range(family):
    pids = np.arange(40).reshape(1, 2, 20)
    for S in (1, 3, 10, 64):
        d = ST.draws(family, SEED, 5, 300, pids, S)
        assert d["comp"].dtype == np.int32 and d["comp"].shape == (300, 1, 2, 20)
        assert d["comp"].min() >= 0 and d["comp"].max() < S
        if S > 1:  # every component is chosen
            assert set(np.unique(d["comp"])) == set(range(S))


def test_comp_by_count():
    """Sj = clip(int(count), 0, S) per particle; the draws other than comp do
    not depend on it, and comp is the float32 product's integer part."""
    S = 4
    counts = np.array([[[0, 1, 2, 3, 4], [4.9, 7, -1, 2.5, 0]]], np.float32)
    Sj = np.array([[[0, 1, 2, 3, 4], [4, 4, 0, 2, 0]]])
    d = ST.sweep_replay("mh", SEED, 0, 500, 1, 2, 5, S, counts=counts)
    full = ST.sweep_replay("mh", SEED, 0, 500, 1, 2, 5, S)
    for k in ("uloc", "uflux", "uacc"):
        np.testing.assert_array_equal(d[k], full[k])
    for idx in np.ndindex(1, 2, 5):
        c = d["comp"][(slice(None),) + idx]
        s = int(Sj[idx])
        if s == 0:
            assert (c == 0).all()  # never read (the particle makes no iteration)
        else:
            assert c.min() >= 0 and c.max() == s - 1
    # against the definition, from the raw words
    r0, _ = ST.raw(ST.TAGS["mh"], SEED, 0, 500, np.array([8]))
    u = (r0[0][:, 0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    np.testing.assert_array_equal(d["comp"][:, 0, 1, 3], np.minimum(np.floor(u * 2), 1))


@pytest.mark.parametrize("family", FAMILIES)
def test_counter_carries_into_the_high_word(family):
    """offset = 2^32 - 20, K = 70: iterations 0..19 use c1 = 0, 20..69 c1 = 1
    with c0 restarting at 0."""
    off, K = 2 ** 32 - 20, 70
    c0, c1 = ST.counters(off, K)
    assert (c1[:20] == 0).all() and (c1[20:] == 1).all()
    assert int(c0[19]) == 0xFFFFFFFF and int(c0[20]) == 0 and int(c0[69]) == 49
    tag0, tag1 = ST.TAGS[family]
    pid = 6
    d = ST.draws(family, SEED, off, K, np.array([pid]), 10)
    for k, (lo, hi) in {0: (2 ** 32 - 20, 0), 19: (2 ** 32 - 1, 0), 20: (0, 1), 69: (49, 1)}.items():
        x = philox4x32(lo, hi, pid, tag0, SEED & 0xFFFFFFFF, SEED >> 32)
        y = philox4x32(lo, hi, pid, tag1, SEED & 0xFFFFFFFF, SEED >> 32)
        assert d["uloc"][k, 0, 0] == ST.u01(x[1]) and d["uloc"][k, 0, 1] == ST.u01(x[2])
        assert d["uflux"][k, 0] == ST.u01(x[3]) and d["uacc"][k, 0] == ST.u01(y[0])
        assert d["comp"][k, 0] == min(int(np.float32(ST.u01(x[0])) * np.float32(10)), 9)
    # a counter that dropped the carry would repeat the draws of offset 0 from k = 20
    low = ST.draws(family, SEED, 0, 50, np.array([pid]), 10)
    assert not np.array_equal(d["uacc"][20:], low["uacc"])
    # the 64-bit sum wraps
    w0, w1 = ST.counters(2 ** 64 - 1, 2)
    assert (int(w0[0]), int(w1[0]), int(w0[1]), int(w1[1])) == (0xFFFFFFFF, 0xFFFFFFFF, 0, 0)


def _all_differ(a, b):
    return all(not np.array_equal(a[k], b[k]) for k in ("comp", "uloc", "uflux", "uacc"))


@pytest.mark.parametrize("family", FAMILIES)
def test_pids_offsets_tags_and_seeds_give_different_draws(family):
    K, S = 100, 10
    base = ST.draws(family, SEED, 0, K, np.array([3]), S)
    assert _all_differ(base, ST.draws(family, SEED, 0, K, np.array([4]), S))
    assert _all_differ(base, ST.draws(family, SEED, K, K, np.array([3]), S))
    assert _all_differ(base, ST.draws(family, SEED + 1, 0, K, np.array([3]), S))
    assert _all_differ(base, ST.draws(family, SEED + (1 << 32), 0, K, np.array([3]), S))
    # the two tags of the family: the accept uniform is not one of r0's words
    r0, r1 = ST.raw(ST.TAGS[family], SEED, 0, K, np.array([3]))
    for w in r0:
        assert not np.array_equal(ST.u01(w)[:, 0], base["uacc"][:, 0])
    assert not any(np.array_equal(a, b) for a in r0 for b in r1)
    # and the three families do not share a stream
    for other in FAMILIES:
        if other != family:
            assert _all_differ(base, ST.draws(other, SEED, 0, K, np.array([3]), S))


def test_pid_is_taken_modulo_2_32():
    a = ST.draws("mh", SEED, 0, 8, np.array([5]), 4)
    b = ST.draws("mh", SEED, 0, 8, np.array([5 + 2 ** 32]), 4)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("o,K,K1", [(0, 100, 64), (2 ** 32 - 20, 70, 37), (11, 70, 1)])
def test_stream_is_the_concatenation_of_its_parts(family, o, K, K1):
    pids = np.arange(12).reshape(2, 6)
    whole = ST.draws(family, SEED, o, K, pids, 5)
    head = ST.draws(family, SEED, o, K1, pids, 5)
    tail = ST.draws(family, SEED, o + K1, K - K1, pids, 5)
    for k in whole:
        np.testing.assert_array_equal(whole[k], np.concatenate([head[k], tail[k]]))


def test_layouts():
    """[K,nH,nW,N(,2)] with pid = t*N + n, t row-major over the tiles."""
    K, nH, nW, N, S = 3, 2, 2, 5, 4
    d = ST.sweep_replay("mala", SEED, 9, K, nH, nW, N, S)
    assert d["comp"].shape == (K, nH, nW, N) and d["uloc"].shape == (K, nH, nW, N, 2)
    assert d["uflux"].shape == d["uacc"].shape == (K, nH, nW, N)
    one = ST.draws("mala", SEED, 9, K, np.array([(1 * nW + 0) * N + 3]), S)
    for k in d:
        np.testing.assert_array_equal(d[k][:, 1, 0, 3], one[k][:, 0])
    c = ST.chain_replay(SEED, 9, K, nH, nW, N, S)
    one = ST.draws("chain", SEED, 9, K, np.array([(0 * nW + 1) * N + 4]), S)
    for k in c:
        np.testing.assert_array_equal(c[k][:, 0, 1, 4], one[k][:, 0])
        assert c[k].flags["C_CONTIGUOUS"]
    assert ST.chain_replay(SEED, 0, 0, 1, 1, 2, 3)["uloc"].shape == (0, 1, 1, 2, 2)
