"""pcp_minmax_segments_aos48 (include/pcp.h, V): row s must be, bit for bit, what the two existing
entries give one after the other, ops.minmax(ops.transform(segment s, T_s)), dense and non-dense;
the numpy reference tests/rot_batch_ref.py (written from the contract) must give the same values.

Segments: sizes 0, 1, 63, 64, 65 (a wave), 257 (a workgroup and one record) and 5000 (three tiles of
2048 records); NaN and +-inf points first, last and inside a segment, on both sides of a tile edge
and as a whole segment; a segment whose coordinates and data[3] are all negative, so that its max
stays at the reference's DBL_MIN start.  Coordinates are map coordinates (thousands of metres), the
poses small rigids about the scene's origin.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_ctypes as ora
import rot_batch_ref as rb

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 5000, 3, 100]
NEG = 8


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def span():
    from pointcloudprocess_amd import synth
    rng = np.random.default_rng(41)
    off = rb.offsets(SIZES)
    xyz = rng.uniform(-25.0, 25.0, (int(off[-1]), 3)) + rb.OFF
    w = rng.uniform(-2.0, 2.0, int(off[-1]))
    nan, inf = np.nan, np.inf
    xyz[off[5]] = [nan, 1.0, 2.0]            # first of a segment
    xyz[off[5] + 100] = [3500.0, inf, 40.0]  # inside
    xyz[off[6] - 1] = [3500.0, -1800.0, -inf]  # last of a segment
    xyz[off[6] + 2047] = [nan, nan, nan]     # both sides of a tile edge
    xyz[off[6] + 2048] = [inf, -1800.0, 40.0]
    xyz[off[7]:off[8]] = [[nan, 0.0, 0.0], [0.0, -inf, 0.0], [inf, inf, nan]]  # a whole segment
    xyz[off[NEG]:off[NEG + 1]] = -rng.uniform(900.0, 1000.0, (SIZES[NEG], 3))
    w[off[NEG]:off[NEG + 1]] = -1.0
    cloud = ora.make_cloud(xyz)
    cloud["w"] = w
    Ts = np.stack([rb.conj(synth.rigid(0.4 * k - 1.0, 0.1 * k, -0.2, (0.05 * k, -0.07, 0.02 * k)))
                   for k in range(len(SIZES))])
    Ts[NEG] = synth.rigid(0.01, 0.0, 0.0, (0.0, 0.0, 0.0))  # about the origin: the points stay negative
    return cloud, off, Ts


def _composed(ctx, dcloud, off, Ts, dense):
    from pointcloudprocess_amd import ops
    rows = []
    for s in range(len(off) - 1):
        seg = dcloud[int(off[s]):int(off[s + 1])]
        T = np.eye(4) if Ts is None else Ts[s]
        rows.append(ops.minmax(ctx, ops.transform(ctx, seg, T, is_dense=dense), is_dense=dense))
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("with_T", [True, False])
def test_rows_equal_transform_then_minmax(ctx, span, dense, with_T):
    from pointcloudprocess_amd import ops
    cloud, off, Ts = span
    Ts = Ts if with_T else None
    d = ops.cloud_to_device(cloud, ctx.device)
    emn, emx = _composed(ctx, d, off, Ts, dense)
    before = ctx.alloc_stats()[0]
    mn, mx = ops.minmax_segments(ctx, d, off, T=Ts, is_dense=dense)
    assert ctx.alloc_stats()[0] == before
    assert mn.shape == (len(SIZES), 4) and mx.shape == (len(SIZES), 4)
    assert np.array_equal(_bits(mn), _bits(emn)), np.argwhere(_bits(mn) != _bits(emn))
    assert np.array_equal(_bits(mx), _bits(emx)), np.argwhere(_bits(mx) != _bits(emx))
    # the numpy reference of the contract agrees in value
    xyzw = np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["w"]], axis=1)
    for s in range(len(SIZES)):
        rmn, rmx = rb.minmax_rows(xyzw[off[s]:off[s + 1]], np.eye(4) if Ts is None else Ts[s], dense)
        assert np.array_equal(mn[s], rmn) and np.array_equal(mx[s], rmx), s
    # an empty segment, and with !dense the all-non-finite one, keep the starts; the negative segment's max too
    assert (mn[0] == rb.DBL_MAX).all() and (mx[0] == rb.DBL_MIN).all()
    if not dense:
        assert (mn[7] == rb.DBL_MAX).all() and (mx[7] == rb.DBL_MIN).all()
        assert np.isfinite(mn[5]).all() and np.isfinite(mx[6]).all()
    assert (mx[NEG] == rb.DBL_MIN).all() and (mn[NEG, :3] < -899.0).all() and mn[NEG, 3] == -1.0
    # a second run: the same bits
    mn2, mx2 = ops.minmax_segments(ctx, d, off, T=Ts, is_dense=dense)
    assert np.array_equal(_bits(mn2), _bits(mn)) and np.array_equal(_bits(mx2), _bits(mx))


def test_one_pose_for_all_and_a_single_segment(ctx, span):
    from pointcloudprocess_amd import ops
    cloud, off, Ts = span
    d = ops.cloud_to_device(cloud, ctx.device)
    emn, emx = _composed(ctx, d, off, np.stack([Ts[3]] * len(SIZES)), False)
    mn, mx = ops.minmax_segments(ctx, d, off, T=Ts[3], is_dense=False)
    assert np.array_equal(_bits(mn), _bits(emn)) and np.array_equal(_bits(mx), _bits(emx))
    seg = d[int(off[6]):int(off[7])]
    mn1, mx1 = ops.minmax_segments(ctx, seg, [0, SIZES[6]], T=Ts[3], is_dense=False)
    assert np.array_equal(_bits(mn1[0]), _bits(emn[6])) and np.array_equal(_bits(mx1[0]), _bits(emx[6]))


def test_arguments_and_balance(ctx, span):
    from pointcloudprocess_amd import ops
    cloud, off, Ts = span
    lib = ctx.lib
    d = ops.cloud_to_device(cloud, ctx.device)
    n, B = len(cloud), len(SIZES)
    p = C.c_void_p(d.data_ptr())
    i64 = lambda v: (C.c_int64 * len(v))(*[int(x) for x in v])
    T = (C.c_double * (16 * B))(*Ts.reshape(-1))
    mn, mx = (C.c_double * (4 * B))(*([7.0] * (4 * B))), (C.c_double * (4 * B))(*([7.0] * (4 * B)))
    before = ctx.alloc_stats()[0]
    fn = lib.pcp_minmax_segments_aos48
    good = [ctx.h, p, n, i64(off), B, 1, T, mn, mx]
    bad_start, bad_end, bad_order = off.copy(), off.copy(), off.copy()
    bad_start[0] = 1
    bad_end[-1] = n - 1
    bad_order[3], bad_order[4] = off[4], off[3]
    for pos, bad in [(0, None), (1, None), (2, -1), (3, None), (3, i64(bad_start)), (3, i64(bad_end)),
                     (3, i64(bad_order)), (4, -1), (7, None), (8, None)]:
        args = list(good)
        args[pos] = bad
        assert fn(*args) == -1, (pos, bad)
        assert ctx.alloc_stats()[0] == before
    # nseg > 65535 (every segment empty, so the offsets themselves are in order)
    big = i64([0] * 65538)
    assert fn(ctx.h, None, 0, big, 65536, 1, None, mn, mx) == -1
    # a rejected call, and nseg == 0, write nothing
    assert fn(ctx.h, None, 0, i64([0]), 0, 1, None, None, None) == 0
    assert fn(ctx.h, None, 0, i64([0]), 0, 1, None, mn, mx) == 0
    assert list(mn) == [7.0] * (4 * B) and list(mx) == [7.0] * (4 * B)
    assert ctx.alloc_stats()[0] == before
    # 65535 empty segments: every row keeps the starts
    emn, emx = ops.minmax_segments(ctx, d[:0], [0] * 65536)
    assert emn.shape == (65535, 4) and (emn == rb.DBL_MAX).all() and (emx == rb.DBL_MIN).all()
    assert ctx.alloc_stats()[0] == before
