"""pcp_get_rot_icp_batch (include/pcp.h, I5d) on the street scene at map coordinates
(rot_batch_ref.scene: 30 000 target points, frames of 0, 1, 2, 63, 64, 65, 1000 and 3000 points, a
different small start pose per frame).

1. Composition, bit for bit.  The expectation is built from public entries that existed before:
   ops.transform per frame, ops.centroid(target), numpy float32(xyz - c), an fp32 GridIndex, ICPBatch,
   new_poses and run_dev / run_trimmed_dev, then the reference's un-centring in numpy.  Rotation
   blocks, err, steps and kept must be equal in every bit; t' within 4 eps (|t| + sum |R_rk c_k| +
   |c_r|) per row (four roundings of terms no larger than that sum, should a host compiler contract).
   ops.transform's moved points must equal rot_batch_ref.xform, the contract's arithmetic in numpy.
2. Freezing: the frames of 0, 1 and 2 points return err = -1 and the exact identity.
3. Recovery against the per-frame path of the parent (a loop of ops.get_rot_icp over the same moved
   frames and the same target), per frame of at least 1000 points:
     e = RMS over the frame's points of |final p - T_true p|,  |e_batch - e_loop| <= max(0.05 e_loop, 2e-4 m).
   Measured on an MI355X, rmax 0.5, 20 iterations: see the table there.
4. Non-finite frame points with frames_dense = False get no pair: the call equals, bit for bit, the
   call with those points moved far outside rmax (both sort last in their frame and join no sum).
5. Empty inputs, argument errors (nothing written), the allocator's balance, repeatability.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_ctypes as ora
import rot_batch_ref as rb
import rtrim_ref as rr

pytestmark = pytest.mark.gpu

RMAX = 0.5
CELL = 0.25
B = len(rb.SIZES)


class Bag:
    pass


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


@pytest.fixture(scope="module")
def g(ctx):
    """The scene on the device and the staged fp32 arrays of the expectation, built once."""
    from pointcloudprocess_amd import ops
    s = rb.scene()
    b = Bag()
    b.s = s
    b.dtgt = ops.cloud_to_device(ora.make_cloud(s.tgt), ctx.device)
    b.dframes = ops.cloud_to_device(ora.make_cloud(s.frames), ctx.device)
    b.c = ops.centroid(ctx, b.dtgt)[0]
    moved = []
    for k in range(B):
        seg = b.dframes[int(s.off[k]):int(s.off[k + 1])]
        m = ops.cloud_to_host(ops.transform(ctx, seg, s.T0[k]))
        moved.append(np.stack([m["x"], m["y"], m["z"]], axis=1).reshape(-1, 3))
    b.moved = moved
    b.q32 = np.concatenate([(m - b.c[:3]).astype(np.float32) for m in moved])
    b.t32 = torch.from_numpy((s.tgt - b.c[:3]).astype(np.float32)).to(ctx.device)
    b.index = ops.GridIndex(ctx, b.t32, cell_size=CELL)
    b.batch = ops.ICPBatch(b.index, torch.from_numpy(b.q32).to(ctx.device), s.off)
    yield b
    b.batch.close()
    b.index.close()


def test_staging_arithmetic_is_the_contracts(g):
    """ops.transform (the entry the expectation moves the frames with) equals the numpy transform of
    the contract bit for bit, and the staged queries equal rot_batch_ref.stage."""
    s = g.s
    for k in range(B):
        seg = s.frames[s.off[k]:s.off[k + 1]]
        assert np.array_equal(_bits(g.moved[k]), _bits(rb.xform(s.T0[k], seg))), k
        assert np.array_equal(g.q32[s.off[k]:s.off[k + 1]].view(np.int32), rb.stage(s.T0[k], seg, g.c).view(np.int32)), k


def _expected(ctx, g, iters, do_scale, trim):
    b = g.batch
    T_dev, stats = b.new_poses()
    rows = None
    if trim is None:
        b.run_dev(g.t32, T_dev, stats, RMAX, iters, do_scale)
    else:
        rows = b.run_trimmed_dev(g.t32, T_dev, stats, RMAX, *trim, iters=iters, do_scale=do_scale).cpu().numpy()
    T, st = T_dev.cpu().numpy().reshape(B, 4, 4), stats.cpu().numpy()
    err = np.where((st[:, 0] == 0) & (st[:, 3] > 0), st[:, 1].astype(np.float32), np.float32(-1.0)).astype(np.float32)
    return T, st, err, rows


@pytest.mark.parametrize("iters,do_scale,trimmed", [(0, False, False), (1, False, False), (4, False, False),
                                                    (4, True, False), (4, False, True), (4, True, True)])
def test_composition_bit_for_bit(ctx, g, iters, do_scale, trimmed):
    from pointcloudprocess_amd import ops
    s = g.s
    trim = rr.SCENE_PTRIM if trimmed else None
    T, st, eerr, rows = _expected(ctx, g, iters, do_scale, trim)
    before = ctx.alloc_stats()[0]
    err, mats, steps, kept = ops.get_rot_icp_batch(ctx, g.dtgt, g.dframes, s.off, RMAX, T0=s.T0, iters=iters,
                                                   do_scale=do_scale, trim=trim, cell_size=CELL)
    assert ctx.alloc_stats()[0] == before
    assert np.array_equal(err.view(np.int32), eerr.view(np.int32)), (err, eerr)
    assert np.array_equal(steps, st[:, 3].astype(np.int32))
    if trimmed:
        assert np.array_equal(kept, rows[:, 1] if iters else np.zeros(B, dtype=np.int64))
    else:
        assert kept is None
    for k in range(B):
        if st[k, 3] > 0:
            e = rb.uncentre(T[k], g.c)
            assert np.array_equal(_bits(mats[k][:, :3]), _bits(e[:, :3])) and np.array_equal(mats[k][3], e[3]), k
            assert (np.abs(mats[k][:3, 3] - e[:3, 3]) <= rb.uncentre_bound(T[k], g.c)).all(), k
        else:
            assert np.array_equal(_bits(mats[k]), _bits(np.eye(4))), k
    # freezing: the frames of 0, 1 and 2 points never solve; with iterations the others do
    assert (err[:3] == -1).all() and (steps[:3] == 0).all()
    if iters:
        assert (err[3:] > 0).all() and (steps[3:] == iters).all(), (err, steps)
        assert all(not np.array_equal(mats[k], np.eye(4)) for k in range(3, B))
        if trimmed:
            assert (kept[3:] >= 3).all() and (kept[3:] < np.array(rb.SIZES[3:])).all(), kept
    else:
        assert (err == -1).all()
    # a second run: the same bits
    err2, mats2, steps2, kept2 = ops.get_rot_icp_batch(ctx, g.dtgt, g.dframes, s.off, RMAX, T0=s.T0, iters=iters,
                                                       do_scale=do_scale, trim=trim, cell_size=CELL)
    assert np.array_equal(_bits(mats2), _bits(mats)) and np.array_equal(err2.view(np.int32), err.view(np.int32))
    assert np.array_equal(steps2, steps) and (kept is None or np.array_equal(kept2, kept))


def test_recovery_against_the_per_frame_path(ctx, g):
    """20 iterations: the batch (target centroid, one index, per-segment sums) against a loop of
    ops.get_rot_icp (joint centroid, one handle per frame) over the same moved frames and target."""
    from pointcloudprocess_amd import ops
    s = g.s
    err, mats, steps, _ = ops.get_rot_icp_batch(ctx, g.dtgt, g.dframes, s.off, RMAX, T0=s.T0, iters=20, cell_size=CELL)
    checked = 0
    for k in range(B):
        if rb.SIZES[k] < 1000:
            continue
        seg = g.dframes[int(s.off[k]):int(s.off[k + 1])]
        moved = ops.transform(ctx, seg, s.T0[k])
        _, M = ops.get_rot_icp(ctx, g.dtgt, moved, RMAX, iters=20, cell_size=CELL)
        xyz = s.frames[s.off[k]:s.off[k + 1]]
        e_batch = rb.rms_to_truth(mats[k] @ s.T0[k], s.T_true[k], xyz)
        e_loop = rb.rms_to_truth(M @ s.T0[k], s.T_true[k], xyz)
        print(f"frame {k} ({rb.SIZES[k]} points): e_batch {e_batch:.6e} m  e_loop {e_loop:.6e} m  "
              f"diff {abs(e_batch - e_loop):.3e}  err {err[k]:.5f}  steps {steps[k]}")
        assert abs(e_batch - e_loop) <= max(0.05 * e_loop, 2e-4), (k, e_batch, e_loop)
        checked += 1
    assert checked == 2


def test_non_finite_frame_points_get_no_pair(ctx, g):
    from pointcloudprocess_amd import ops
    s = g.s
    a7, b7 = int(s.off[7]), int(s.off[8])
    at = [a7, a7 + 1500, b7 - 1]
    bad = s.frames.copy()
    bad[at[0]] = [np.nan, -1800.0, 40.0]
    bad[at[1]] = [3500.0, np.inf, 40.0]
    bad[at[2]] = [np.nan, np.nan, -np.inf]
    far = s.frames.copy()
    far[at] += 1000.0  # beyond the target's box in +x, +y and +z: the last cell, the last place of the frame's order
    run = lambda xyz, dense: ops.get_rot_icp_batch(
        ctx, g.dtgt, ops.cloud_to_device(ora.make_cloud(xyz), ctx.device), s.off, RMAX, T0=s.T0, iters=4,
        cell_size=CELL, frames_dense=dense)
    base = run(s.frames, True)
    e_bad, m_bad, st_bad, _ = run(bad, False)
    e_far, m_far, st_far, _ = run(far, True)
    assert np.array_equal(_bits(m_bad), _bits(m_far)) and np.array_equal(e_bad.view(np.int32), e_far.view(np.int32))
    assert np.array_equal(st_bad, st_far) and st_bad[7] == 4 and e_bad[7] > 0
    # the other frames are untouched; frame 7 lost three queries of 3000 and moved by rounding at most
    assert np.array_equal(_bits(m_bad[:7]), _bits(base[1][:7])) and np.array_equal(e_bad[:7].view(np.int32),
                                                                                    base[0][:7].view(np.int32))
    assert np.isfinite(m_bad).all()
    # dense = True transforms the NaN points too; they still get no key, and nothing else changes
    e_d, m_d, _, _ = run(bad, True)
    assert np.array_equal(_bits(m_d), _bits(m_bad)) and np.array_equal(e_d.view(np.int32), e_bad.view(np.int32))


def test_empty_inputs_errors_and_balance(ctx, g):
    from pointcloudprocess_amd import ops
    s, lib = g.s, ctx.lib
    fn = lib.pcp_get_rot_icp_batch
    nt, nq = len(s.tgt), len(s.frames)
    pt, pf = C.c_void_p(g.dtgt.data_ptr()), C.c_void_p(g.dframes.data_ptr())
    i64 = lambda v: (C.c_int64 * len(v))(*[int(x) for x in v])
    T0 = (C.c_double * (16 * B))(*s.T0.reshape(-1))
    M = (C.c_double * (16 * B))(*([7.0] * (16 * B)))
    err = (C.c_float * B)(*([7.0] * B))
    steps = (C.c_int32 * B)(*([7] * B))
    kept = (C.c_int64 * B)(*([7] * B))
    f3 = lambda *v: (C.c_float * 3)(*v)
    before = ctx.alloc_stats()[0]
    good = [ctx.h, pt, nt, 1, pf, nq, 1, i64(s.off), B, T0, RMAX, 2, 0, None, CELL, M, err, steps, kept]
    bad_start, bad_end, bad_order = s.off.copy(), s.off.copy(), s.off.copy()
    bad_start[0] = 1
    bad_end[-1] = nq - 1
    bad_order[4], bad_order[5] = s.off[5], s.off[4]
    nan, inf = float("nan"), float("inf")
    cases = [(0, None), (1, None), (2, -1), (4, None), (5, -1), (7, None), (7, i64(bad_start)), (7, i64(bad_end)),
             (7, i64(bad_order)), (8, -1), (11, -1), (15, None), (16, None),
             (13, f3(-0.1, 1.0, 0.0)), (13, f3(1.5, 1.0, 0.0)), (13, f3(nan, 1.0, 0.0)), (13, f3(0.5, -1.0, 0.0)),
             (13, f3(0.5, inf, 0.0)), (13, f3(0.5, 1.0, -0.1)), (13, f3(0.5, 1.0, nan))]
    for pos, bad in cases:
        args = list(good)
        args[pos] = bad
        assert fn(*args) == -1, (pos, bad)
        assert ctx.alloc_stats()[0] == before
    assert fn(ctx.h, pt, nt, 1, None, 0, 1, i64([0] * 65538), 65536, None, RMAX, 2, 0, None, CELL, M, err, steps,
              kept) == -1
    assert fn(ctx.h, pt, nt, 1, pf, 1 << 31, 1, i64([0] * (B - 1) + [1 << 31] * 2), B, T0, RMAX, 2, 0, None, CELL, M,
              err, steps, kept) == -1  # pcp_icp_check_sizes
    for rmax in (0.0, -1.0, nan):  # UNSUPPORTED, as pcp_get_rot_icp
        args = list(good)
        args[10] = rmax
        assert fn(*args) == -5, rmax
        assert b"rmax must be > 0" in lib.pcp_last_error(ctx.h)
    # nseg == 0: PCP_OK, null outputs are legal
    assert fn(ctx.h, pt, nt, 1, None, 0, 1, i64([0]), 0, None, RMAX, 2, 0, None, CELL, None, None, None, None) == 0
    assert fn(ctx.h, pt, nt, 1, None, 0, 1, i64([0]), 0, None, RMAX, 2, 0, None, CELL, M, err, steps, kept) == 0
    # none of the calls above wrote anything
    assert list(M) == [7.0] * (16 * B) and list(err) == [7.0] * B and list(steps) == [7] * B and list(kept) == [7] * B
    assert ctx.alloc_stats()[0] == before
    # no target, or no frame points: identities, err = -1, steps = 0, kept = 0
    eye = np.tile(np.eye(4), (B, 1, 1))
    e, m, st, kp = ops.get_rot_icp_batch(ctx, g.dtgt[:0], g.dframes, s.off, RMAX, T0=s.T0, trim=rr.SCENE_PTRIM)
    assert (e == -1).all() and np.array_equal(_bits(m), _bits(eye)) and (st == 0).all() and (kp == 0).all()
    e, m, st, kp = ops.get_rot_icp_batch(ctx, g.dtgt, g.dframes[:0], [0] * (B + 1), RMAX, T0=s.T0)
    assert (e == -1).all() and np.array_equal(_bits(m), _bits(eye)) and (st == 0).all() and kp is None
    assert ctx.alloc_stats()[0] == before
    # T0 = None is the identity pose through the same arithmetic
    ident = np.tile(np.eye(4), (B, 1, 1))
    r0 = ops.get_rot_icp_batch(ctx, g.dtgt, g.dframes, s.off, RMAX, T0=None, iters=2, cell_size=CELL)
    r1 = ops.get_rot_icp_batch(ctx, g.dtgt, g.dframes, s.off, RMAX, T0=ident, iters=2, cell_size=CELL)
    assert np.array_equal(_bits(r0[1]), _bits(r1[1])) and np.array_equal(r0[0].view(np.int32), r1[0].view(np.int32))
    assert ctx.alloc_stats()[0] == before
