"""CPU checks of tests/batch_trim_ref.py (the per-segment trims of pcp.h I5b) on hand-made inputs whose
answers are known, and of the conditions the GPU test's crafted inputs must meet (so that nothing
there passes by rejecting everything, by keeping everything, or because one pooled quantile would
have done)."""
import numpy as np

import batch_trim_cases as cases
import batch_trim_ref as bt
import trim_ref as tr

NO_KEY = tr.NO_KEY


def _bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def _keys(d2, low=None):
    d2 = np.asarray(d2, dtype=np.float32)
    low = np.arange(len(d2)) if low is None else low
    return tr.make_keys(d2.view(np.uint32), low)


def test_two_segments_with_known_order_statistics():
    # segment 0: 1 .. 10 (shuffled), segment 1: 100 .. 500; frac 0.5 -> r = floor(0.5 * (m - 1))
    a = np.float32([7, 1, 10, 3, 5, 2, 9, 4, 8, 6])
    b = np.float32([300, 100, 500, 200, 400])
    keys = _keys(np.concatenate([a, b]))
    out, st = bt.trim(keys, [0, 10, 15], 0.5)
    assert st[0].tolist() == [10, 5, _bits(5.0), _bits(5.0)]    # r = 4: the 5th smallest
    assert st[1].tolist() == [5, 3, _bits(300.0), _bits(300.0)]  # r = 2
    assert np.array_equal(out[:10] != NO_KEY, a <= 5) and np.array_equal(out[10:] != NO_KEY, b <= 300)
    assert np.array_equal(out[out != NO_KEY], keys[out != NO_KEY])  # a kept key is unchanged
    # one pooled quantile over all 15 keys: r = 7, sel = 8 -- every key of segment 1 would go
    pooled, pst = tr.trim(keys, 0.5)
    assert pst.tolist() == [15, 8, _bits(8.0), _bits(8.0)] and (pooled[10:] == NO_KEY).all()
    assert bt.differing_segments(pooled, out, [0, 10, 15]) == [0, 1]
    # mult and the floor act per segment on the same scalars: cut = max(4 * sel, 30^2)
    out, st = bt.trim(keys, [0, 10, 15], 0.5, 2.0, 30.0)
    assert st[0].tolist() == [10, 10, _bits(5.0), _bits(900.0)]
    assert st[1].tolist() == [5, 5, _bits(300.0), _bits(1200.0)]


def test_empty_and_all_invalid_segments():
    keys = np.concatenate([_keys([1, 2, 3]), np.full(4, NO_KEY, dtype=np.int64), _keys([9, 8])])
    off = [0, 0, 3, 3, 7, 9, 9]
    out, st = bt.trim(keys, off, 1.0, 1.0, 0.5)
    f2 = _bits(0.25)
    assert st.tolist() == [[0, 0, 0, f2], [3, 3, _bits(3.0), _bits(3.0)], [0, 0, 0, f2], [0, 0, 0, f2],
                           [2, 2, _bits(9.0), _bits(9.0)], [0, 0, 0, f2]]
    assert (out[3:7] == NO_KEY).all() and np.array_equal(out[:3], keys[:3]) and np.array_equal(out[7:], keys[7:])
    out, st = bt.trim(np.zeros(0, dtype=np.int64), [0], 0.5)  # no segment at all
    assert out.shape == (0,) and st.shape == (0, 4)


def test_ties_across_the_cut():
    # segment 0: four copies of 2 around the rank; all of them survive, the 3 does not
    keys = _keys([2, 1, 2, 3, 2, 2, 5, 5, 5])
    out, st = bt.trim(keys, [0, 6, 9], 0.4)  # r = floor(0.4 * 5) = 2 -> sel = 2; r = floor(0.8) = 0
    assert st[0].tolist() == [6, 5, _bits(2.0), _bits(2.0)]
    assert st[1].tolist() == [3, 3, _bits(5.0), _bits(5.0)]
    assert (out[:6] != NO_KEY).tolist() == [True, True, True, False, True, True]


def test_plane_trim_per_segment_pose():
    # the plane z = 0 with normal +z; segment s is lifted by its own pose, so rho = (z + t_s)^2
    pts = np.zeros((4, 3), dtype=np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (4, 1))
    nrm[3] = 0  # an invalid record
    z = np.float32([0.1, 0.2, 0.3, 0.4, 0.1, 0.2, 0.3])
    q = np.zeros((7, 3), dtype=np.float32)
    q[:, 2] = z
    keys = _keys(np.full(7, 0.5), low=np.array([0, 1, 2, 0, 1, 3, 2]))
    Ts = np.stack([np.eye(4), np.eye(4)])
    Ts[1, 2, 3] = 1.0
    out, st = bt.rtrim(Ts, q, keys, [0, 4, 7], pts, nrm, 0.5)
    r0 = np.float32(np.float64(np.float32(0.2)) ** 2)
    r1 = np.float32(np.float64(np.float32(1.0) + np.float32(0.1)) ** 2)
    assert st[0].tolist() == [4, 2, _bits(r0), _bits(r0)]  # r = 1
    assert st[1].tolist() == [2, 1, _bits(r1), _bits(r1)]  # the invalid record is not usable; r = 0
    assert (out != NO_KEY).tolist() == [True, True, False, False, True, False, False]
    assert np.array_equal(out[out != NO_KEY], keys[out != NO_KEY])  # the high word stays the point d2


def _big(c):
    return [s for s, n in enumerate(cases.SIZES) if n >= 63]


def test_crafted_plane_case_conditions():
    c = cases.crafted()
    assert np.isnan(c.q[c.nan_at]).any() and c.keys[c.nan_at] != NO_KEY
    out, st = cases.plane_ref(0.5, 1.5, 0.0)
    share = [int(st[s, 1]) / cases.SIZES[s] for s in _big(c)]
    print("plane trim (0.5, 1.5): kept share per segment", ["%.3f" % v for v in share])
    for s in _big(c):
        assert st[s, 1] >= 0.4 * cases.SIZES[s] and st[s, 1] < st[s, 0], (s, st[s].tolist())
    assert out[c.nan_at] == NO_KEY  # the NaN query's pair is not usable
    assert st[0].tolist() == [0, 0, 0, 0]
    assert st[2, 0] < 6  # the five-query segment


def test_crafted_point_case_conditions():
    c = cases.crafted()
    out, st = cases.point_ref(0.9, 1.0, 0.0)
    share = [int(st[s, 1]) / cases.SIZES[s] for s in _big(c)]
    print("point trim (0.9, 1.0): kept share per segment", ["%.3f" % v for v in share])
    for s in _big(c):
        assert st[s, 1] >= 0.7 * cases.SIZES[s] and st[s, 1] < st[s, 0], (s, st[s].tolist())
    # what the feature exists for: one pooled quantile over all keys is wrong in most segments.  At
    # (0.9, 1.0) segments 3 .. 7 lie wholly under the pooled cut, which keeps all of them, while
    # their own quantile rejects a tenth; the second parameter set is printed for the record
    for frac, mult, fl in cases.POINT_PARAMS:
        pooled, _ = tr.trim(c.pkeys, frac, mult, fl)
        diff = bt.differing_segments(pooled, cases.point_ref(frac, mult, fl)[0], c.off)
        print(f"pooled trim ({frac}, {mult}, {fl}) differs in segments", diff)
        if (frac, mult, fl) == (0.9, 1.0, 0.0):
            assert len(diff) >= 5 and set(range(3, 8)) <= set(diff)


def test_edge_batch_conditions():
    keys, off = cases.edge_batch()
    out, st = bt.trim(keys, off, 0.5)
    b = _bits(0.0625)
    assert st[0].tolist() == [5000, 5000, b, b]  # all equal: the ties straddle the rank, all kept
    assert st[2].tolist() == [0, 0, 0, 0] and st[4].tolist() == [0, 0, 0, 0]
    out, st = bt.trim(keys, off, 1.0)
    assert st[1, 2] == 0xFFFFFFFF and st[1, 3] == 0  # sel is a NaN pattern: c is NaN, cut = f2 = 0
    assert st[1, 1] == 0
    out, st = bt.trim(keys, off, 0.5)
    assert st[1, 2] < 0x7F800000 and 0 < st[1, 1] < st[1, 0]
    out, st = bt.trim(keys, off, 0.8)
    assert st[1, 2] == 0x7F800000  # +inf selected: every non-NaN key is kept
    assert st[1, 1] == int((tr.high_words(keys[off[1]:off[2]]) <= 0x7F800000).sum())
