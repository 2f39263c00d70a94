"""Inputs of the per-segment trim tests (include/pcp.h, I5b), built once and never modified, so the
CPU test can assert the conditions the GPU test relies on.

Crafted case: test_gpu_icp_plane._case(sum(SIZES), 7) -- one 1000-record table, keys with every 8th
INT64_MAX, indices past the table and the three invalid records -- cut into SIZES, with a NaN
coordinate in query off[8] + 4321 and one pose per segment.  70000 is the smallest size that makes a
workgroup walk its slot range many times (4096 keys a round), 63 / 64 / 65 straddle a 64-query
chunk, 5 has fewer than 6 pairs.  For the point trim segment s's d2 is scaled by (s + 1)^2 in fp32,
so that the segments differ in scale and one pooled quantile is wrong for most of them.
"""
import functools

import numpy as np

import batch_trim_ref as bt
import trim_ref as tr

NO_KEY = tr.NO_KEY
SIZES = [0, 1, 5, 63, 64, 65, 257, 1000, 70000, 3000]
NAN_SEG, NAN_AT = 8, 4321
PLANE_PARAMS = [(0.5, 1.5, 0.0), (0.5, 3.0, 0.0), (0.9, 1.0, 0.0)]
POINT_PARAMS = [(0.9, 1.0, 0.0), (0.5, 1.5, 0.1)]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class Crafted:
    pass


@functools.lru_cache(maxsize=None)
def crafted():
    from pointcloudprocess_amd import synth
    from test_gpu_icp_plane import _case
    c = Crafted()
    c.off = offsets(SIZES)
    _, c.q, c.keys, c.pts, c.rows = _case(int(c.off[-1]), 7)
    c.nan_at = int(c.off[NAN_SEG]) + NAN_AT
    c.q[c.nan_at, 0] = np.nan
    c.Ts = np.stack([synth.rigid(0.3 * s - 1.0, 0.1 * s, -0.2, (0.05 * s, -0.07, 0.02 * s))
                     for s in range(len(SIZES))])
    # the point trim's keys: segment s's d2 times (s + 1)^2, one fp32 product
    d2 = tr.high_words(c.keys).view(np.float32).copy()
    for s in range(len(SIZES)):
        d2[c.off[s]:c.off[s + 1]] *= np.float32((s + 1) ** 2)
    c.pkeys = np.where(c.keys != NO_KEY, tr.make_keys(d2.view(np.uint32), c.keys.view(np.uint64) & np.uint64(0xFFFFFFFF)),
                       np.int64(NO_KEY))
    for a in (c.off, c.q, c.keys, c.pkeys, c.pts, c.rows, c.Ts):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def plane_ref(frac, mult, d_floor):
    c = crafted()
    out, stats = bt.rtrim(c.Ts, c.q, c.keys, c.off, c.pts, c.rows[:, :3], frac, mult, d_floor)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


@functools.lru_cache(maxsize=None)
def point_ref(frac, mult, d_floor):
    c = crafted()
    out, stats = bt.trim(c.pkeys, c.off, frac, mult, d_floor)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


def edge_batch():
    """(keys, off) of one batch whose segments hold the edge values of the high word: all-equal d2
    (ties straddle every rank), +inf and NaN patterns among ordinary ones, all INT64_MAX, one
    ordinary segment, an empty one."""
    rng = np.random.default_rng(19)
    sizes = [5000, 3000, 700, 4097, 0, 64]
    off = offsets(sizes)
    high = rng.uniform(0, 0.25, int(off[-1])).astype(np.float32).view(np.uint32)
    low = rng.integers(0, 1000, int(off[-1])).astype(np.uint32)
    high[off[0]:off[1]] = np.float32(0.0625).view(np.uint32)
    seg1 = high[off[1]:off[2]]
    seg1[::7] = 0x7F800000   # +inf
    seg1[3::11] = 0x7FC00000  # a NaN pattern
    seg1[5::13] = 0xFFFFFFFF  # a NaN pattern above every finite value in unsigned order
    keys = tr.make_keys(high, low)
    keys[off[2]:off[3]] = NO_KEY
    keys[off[3] + 1:off[4]:5] = NO_KEY
    return keys, off
