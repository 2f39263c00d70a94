"""Numpy reference of the per-segment trims of a batch (include/pcp.h, I5b), written from the
contract text, not from the kernels: for every segment s the single-pair reference on that slice
alone,

  * point trim: trim_ref.trim(keys[off[s]:off[s + 1]], frac, mult, d_floor);
  * plane trim: rtrim_ref.rtrim(Ts[s], q[off[s]:off[s + 1]], keys[off[s]:off[s + 1]], points,
    normals, frac, mult, d_floor),

with frac, mult and d_floor shared by all segments.  Returns the nq output keys (int64) and an
(nseg, 4) uint64 array of rows [m, kept, sel, bits of cut]; an empty segment's row is
[0, 0, 0, bits(f2)], which is what both references write for no keys.
"""
import numpy as np

import rtrim_ref
import trim_ref

NO_KEY = trim_ref.NO_KEY


def _slices(off):
    return [(int(off[s]), int(off[s + 1])) for s in range(len(off) - 1)]


def trim(keys, off, frac, mult=1.0, d_floor=0.0):
    keys = np.ascontiguousarray(np.asarray(keys).view(np.int64))
    out = np.full(keys.shape[0], NO_KEY, dtype=np.int64)
    stats = np.zeros((len(off) - 1, 4), dtype=np.uint64)
    for s, (a, b) in enumerate(_slices(off)):
        out[a:b], stats[s] = trim_ref.trim(keys[a:b], frac, mult, d_floor)
    return out, stats


def rtrim(Ts, q, keys, off, points, normals, frac, mult=1.0, d_floor=0.0):
    keys = np.ascontiguousarray(np.asarray(keys).view(np.int64))
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    Ts = np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4)
    out = np.full(keys.shape[0], NO_KEY, dtype=np.int64)
    stats = np.zeros((len(off) - 1, 4), dtype=np.uint64)
    for s, (a, b) in enumerate(_slices(off)):
        out[a:b], stats[s] = rtrim_ref.rtrim(Ts[s], q[a:b], keys[a:b], points, normals, frac, mult, d_floor)
    return out, stats


def differing_segments(keys_a, keys_b, off):
    """The segments in which two key arrays differ."""
    return [s for s, (a, b) in enumerate(_slices(off)) if not np.array_equal(keys_a[a:b], keys_b[a:b])]
