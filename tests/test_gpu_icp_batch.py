"""GPU checks of batched registration (include/pcp.h, I5) against the single-pair handle and the
independent numpy reference tests/icp_batch_ref.py.

Scene: a 30000-point street scene (extent 50 m) with 200 of its own points appended again (the
duplicates exercise the tie rule), fp32 index with 0.25 m cells, GPU normals (k = 16), one plane
table.  Eight segments of 0, 1, 63, 64, 65, 1000, 8000 and 3000 queries: segment s is its own street
scene moved by the inverse of its own T_true; segment 7 is turned by 90.5 degrees and starts at 90.
rmax = 0.5.  The brute-force keys and ONE stepwise run of four iterations are computed once and
shared.  Tolerances are those of test_gpu_icp_plane.py: counts exact, sums to rtol 1e-12 / atol
1e-12 max|acc| (every product is one of widened fp32 values; only the order of the sum differs),
poses and stats to 1e-9 against the reference's solve, 1e-12 between two GPU paths.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_batch_ref as bref
import icp_plane_ref as ref

pytestmark = pytest.mark.gpu

NO_KEY = bref.NO_KEY
RMAX = 0.5
ITERS = 4
SIZES = [0, 1, 63, 64, 65, 1000, 8000, 3000]


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _close(g, e):
    return np.allclose(g, e, rtol=1e-12, atol=1e-12 * max(np.abs(e).max(), 1e-300))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _segment(n, seed, T_true):
    from pointcloudprocess_amd import synth
    if n == 0:
        return np.zeros((0, 3), dtype=np.float32)
    return synth.apply_inverse(synth.street_scene(n, seed, extent=(50.0, 50.0)), T_true).numpy()


def _single_keys(index, ctx, q, off, Ts, rmax):
    """Per segment: a pcp_icp over that segment's queries alone, its keys at the segment's pose."""
    from pointcloudprocess_amd import ops
    out = np.full(len(q), NO_KEY, dtype=np.int64)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        if a == b:
            continue
        icp = ops.ICP(index, _dev(ctx, q[a:b]))
        T_dev, _ = icp.new_pose(Ts[s])
        out[a:b] = icp.keys_dev(T_dev, rmax).cpu().numpy()
        icp.close()
    return out


def _unkeyed(keys, off):
    """Per segment the fraction of queries without a key (0 for an empty segment)."""
    return [float((keys[off[s]:off[s + 1]] == NO_KEY).mean()) if off[s + 1] > off[s] else 0.0
            for s in range(len(off) - 1)]


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    from pointcloudprocess_amd import ops, synth
    s = Scene()
    base = synth.street_scene(30000, 11, extent=(50.0, 50.0)).numpy()
    s.tgt = np.concatenate([base, base[::150]])  # 200 duplicates at higher indices
    assert len(s.tgt) == 30200
    s.dtgt = _dev(ctx, s.tgt)
    ix64 = ops.GridIndex(ctx, s.dtgt.double())
    s.drows = ops.normals_knn(ix64, 16)
    ix64.close()
    s.rows = s.drows.cpu().numpy()
    s.index = ops.GridIndex(ctx, s.dtgt, cell_size=0.25)
    s.planes = ops.IcpPlanes(ctx, s.dtgt, s.drows)
    s.T_true = [synth.rigid(1.0, 0.4, -0.3, t=(0.15, -0.10, 0.05)) for _ in SIZES]
    s.T_true[5] = synth.rigid(-0.8, 0.2, 0.5, t=(-0.1, 0.12, 0.03))
    s.T_true[7] = synth.rigid(90.5, 0.3, -0.2, t=(0.1, 0.1, -0.05))
    s.T0 = np.stack([np.eye(4)] * len(SIZES))
    s.T0[7] = synth.rigid(90.0, 0.0, 0.0, t=(0.0, 0.0, 0.0))
    s.segs = [_segment(n, 100 + k, s.T_true[k]) for k, n in enumerate(SIZES)]
    s.off = _offsets(SIZES)
    s.q = np.concatenate(s.segs)
    s.dq = _dev(ctx, s.q)
    # the reference keys at the start poses, and the condition that nothing passes by skipping
    s.ref_keys = bref.batch_keys(s.T0, s.q, s.off, s.tgt, RMAX)
    s.unkeyed = _unkeyed(s.ref_keys, s.off)
    # one stepwise run
    s.batch = ops.ICPBatch(s.index, s.dq, s.off)
    T_dev, stats = s.batch.new_poses(s.T0)
    s.steps = []
    for _ in range(ITERS):
        T_prev = T_dev.cpu().numpy().reshape(-1, 4, 4).copy()
        st_prev = stats.cpu().numpy().copy()
        keys = s.batch.keys_dev(T_dev, RMAX)
        acc = s.batch.accumulate_plane(T_dev, keys, s.planes)
        s.batch.solve_plane_dev(acc, T_dev, stats)
        s.steps.append((T_prev, st_prev, keys.cpu().numpy().copy(), acc.cpu().numpy().copy(),
                        T_dev.cpu().numpy().reshape(-1, 4, 4).copy(), stats.cpu().numpy().copy()))
    yield s
    s.batch.close()
    s.planes.close()
    s.index.close()


def test_reference_pairs_most_queries(scene):
    print("unkeyed fraction per segment:", ["%.3f" % u for u in scene.unkeyed])
    for k, n in enumerate(SIZES):
        if n >= 63:
            assert scene.unkeyed[k] <= 0.25, (k, scene.unkeyed[k])
    j = scene.ref_keys[scene.ref_keys != NO_KEY] & 0xFFFFFFFF
    assert (j < 30000).all()  # a duplicate (index >= 30000) never beats its original


# ------------------------------------------------------------------ 1, 2: keys
def test_keys_equal_single_handles_and_reference(ctx, scene):
    from pointcloudprocess_amd import ops
    q = scene.q.copy()
    nan_at = int(scene.off[6]) + 4321
    q[nan_at, 1] = np.nan
    dq = _dev(ctx, q)
    b = ops.ICPBatch(scene.index, dq, scene.off)
    T_dev, _ = b.new_poses(scene.T0)
    got = b.keys_dev(T_dev, RMAX).cpu().numpy()
    b.close()
    exp = scene.ref_keys.copy()
    exp[nan_at] = NO_KEY
    single = _single_keys(scene.index, ctx, q, scene.off, scene.T0, RMAX)
    print("mismatch vs single:", int((got != single).sum()), "vs reference:", int((got != exp).sum()))
    assert got[nan_at] == NO_KEY
    assert np.array_equal(got.view(np.uint64), single.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    # the first iteration of the shared stepwise run saw the same keys but for the NaN query
    same = np.arange(len(q)) != nan_at
    assert np.array_equal(scene.steps[0][2][same], exp[same])


def _cut(scene, cap=2000):
    sizes = [min(n, cap) for n in SIZES]
    segs = [sg[:n] for sg, n in zip(scene.segs, sizes)]
    return np.concatenate(segs), _offsets(sizes)


def _check_keys(ctx, index, tgt, q, off, Ts, rmax, min_keyed=None):
    from pointcloudprocess_amd import ops
    b = ops.ICPBatch(index, _dev(ctx, q), off)
    T_dev, _ = b.new_poses(Ts)
    got = b.keys_dev(T_dev, rmax).cpu().numpy()
    b.close()
    single = _single_keys(index, ctx, q, off, Ts, rmax)
    exp = bref.batch_keys(Ts, q, off, tgt, rmax)
    print("unkeyed:", ["%.3f" % u for u in _unkeyed(exp, off)], "mismatch vs single:",
          int((got != single).sum()), "vs reference:", int((got != exp).sum()))
    if min_keyed is not None:
        for s, u in enumerate(_unkeyed(exp, off)):
            if off[s + 1] - off[s] >= 63:
                assert 1.0 - u >= min_keyed, (s, u)
    assert np.array_equal(got.view(np.uint64), single.view(np.uint64))
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    return got


def test_keys_wide_rmax(ctx, scene):
    """rmax = 0.9: more than three 0.25 m cells."""
    q, off = _cut(scene)
    _check_keys(ctx, scene.index, scene.tgt, q, off, scene.T0, 0.9, min_keyed=0.75)


def test_keys_segment_outside_the_box(ctx, scene):
    """Segment 6's pose moves it 500 m away from the target's box: every key is INT64_MAX, the
    other segments are untouched."""
    q, off = _cut(scene)
    Ts = scene.T0.copy()
    Ts[6, :3, 3] = [500.0, -300.0, 80.0]
    got = _check_keys(ctx, scene.index, scene.tgt, q, off, Ts, RMAX)
    assert (got[off[6]:off[7]] == NO_KEY).all()
    keep = np.r_[0:off[6], off[7]:off[8]]
    cutkeys = np.concatenate([scene.ref_keys[scene.off[s]:scene.off[s] + (off[s + 1] - off[s])]
                              for s in range(len(SIZES))])
    assert np.array_equal(got[keep], cutkeys[keep])


def test_keys_brick_table(ctx):
    """Two clusters 5 km apart with 5 cm cells: the index uses the brick (sparse) cell table."""
    from pointcloudprocess_amd import ops, synth
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 2, size=(20000, 3)).astype(np.float32)
    tgt = np.concatenate([a, a[:5000] + np.float32(5000.0)])
    index = ops.GridIndex(ctx, _dev(ctx, tgt), cell_size=0.05)
    assert ctx.lib.pcp_index_cells(index.h) < 1e9  # sparse (brick) mode
    sizes = [0, 1, 65, 2000, 1500]
    off = _offsets(sizes)
    pick = rng.permutation(20000)[:off[-1]]  # the near cluster (a rotation about the origin moves the far one by metres)
    pick[off[4]:] = 20000 + rng.integers(0, 5000, sizes[4])  # the last segment, identity pose: the far cluster
    q = (tgt[pick] + rng.normal(scale=0.01, size=(len(pick), 3))).astype(np.float32)
    Ts = np.stack([synth.rigid(0.1, 0.0, 0.0, (0.01, 0.0, 0.0)), np.eye(4), synth.rigid(-0.2, 0.1, 0.0, (0, 0.01, 0)),
                   synth.rigid(0.1, 0.0, 0.0, (0.01, 0.0, 0.0)), np.eye(4)])
    _check_keys(ctx, index, tgt, q, off, Ts, 0.1, min_keyed=0.75)
    index.close()


# ------------------------------------------------------------------ 3: stepwise against the reference
def test_stepwise_loop_matches_reference(scene):
    B = len(SIZES)
    for it, (T_prev, st_prev, keys, acc, T_new, stats) in enumerate(scene.steps):
        eacc, eT, est = bref.batch_step(T_prev, st_prev, scene.q, scene.off, keys, scene.tgt, scene.rows[:, :3])
        for s in range(B):
            if s >= 2 and st_prev[s, 0] == 0 and eacc[s, 0] >= 6:
                mp = ref.min_pivot(eacc[s])
                assert not (1e-11 <= mp <= 1e-9), (it, s, mp)  # the decision is not a coin toss
            print(f"it={it} seg={s} pairs={int(acc[s, 0])} status={stats[s, 0]:.0f} "
                  f"|T-T_ref|={np.abs(T_new[s] - eT[s]).max():.2e} |stats-ref|={np.abs(stats[s] - est[s]).max():.2e}")
            assert acc[s, 0] == eacc[s, 0]
            assert _close(acc[s], eacc[s]), (it, s)
            assert stats[s, 0] == est[s, 0], (it, s)
            assert np.abs(T_new[s] - eT[s]).max() < 1e-9, (it, s)
            assert np.abs(stats[s] - est[s]).max() < 1e-9, (it, s)
        assert np.array_equal(acc[0], np.zeros(30))  # the empty segment
        for s in (0, 1):  # fewer than 6 pairs: failed, pose untouched, iterations solved still 0
            assert stats[s, 0] == -1 and stats[s, 3] == 0
            assert np.array_equal(T_new[s], scene.T0[s])
    final = scene.steps[-1][5]
    assert (final[2:, 0] == 0).all() and (final[2:, 3] == ITERS).all()


# ------------------------------------------------------------------ 4: the device loop
def test_run_plane_dev_equals_stepwise_and_repeats(ctx, scene):
    before = ctx.alloc_stats()[0]
    runs = []
    for _ in range(2):
        T_dev, stats = scene.batch.new_poses(scene.T0)
        scene.batch.run_plane_dev(scene.planes, T_dev, stats, RMAX, ITERS)
        runs.append((T_dev.cpu().numpy().copy(), stats.cpu().numpy().copy()))
    assert ctx.alloc_stats()[0] == before
    T, st = runs[0]
    assert np.abs(T.reshape(-1, 4, 4) - scene.steps[-1][4]).max() < 1e-12
    assert np.abs(st - scene.steps[-1][5]).max() < 1e-12
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64))
    assert np.array_equal(runs[0][1].view(np.int64), runs[1][1].view(np.int64))


# ------------------------------------------------------------------ 5: segment independence
def test_segments_are_independent(ctx, scene):
    from pointcloudprocess_amd import ops
    perm = [6, 0, 7, 3, 1, 5, 2, 4]
    sizes = [SIZES[p] for p in perm]
    off = _offsets(sizes)
    q = np.concatenate([scene.segs[p] for p in perm])
    b = ops.ICPBatch(scene.index, _dev(ctx, q), off)
    T_dev, stats = b.new_poses(scene.T0[perm])
    keys = b.keys_dev(T_dev, RMAX).cpu().numpy()
    b.run_plane_dev(scene.planes, T_dev, stats, RMAX, ITERS)
    T, st = T_dev.cpu().numpy().reshape(-1, 4, 4), stats.cpu().numpy()
    b.close()
    for k, p in enumerate(perm):
        assert np.array_equal(keys[off[k]:off[k + 1]], scene.ref_keys[scene.off[p]:scene.off[p + 1]]), p
        assert np.abs(T[k] - scene.steps[-1][4][p]).max() < 1e-12, p
        assert np.abs(st[k] - scene.steps[-1][5][p]).max() < 1e-12, p
    # a batch of one segment: the same keys as inside the batch of eight
    for p in (5, 7):
        b1 = ops.ICPBatch(scene.index, _dev(ctx, scene.segs[p]), [0, SIZES[p]])
        T1, _ = b1.new_poses(scene.T0[p])
        k1 = b1.keys_dev(T1, RMAX).cpu().numpy()
        b1.close()
        assert np.array_equal(k1, scene.steps[0][2][scene.off[p]:scene.off[p + 1]]), p


# ------------------------------------------------------------------ 6: convergence
def test_convergence(scene):
    """test_gpu_icp_plane.test_convergence's bound per segment: < 5 mm and < 0.02 deg after four
    iterations, segment 7 from its 90 degree start."""
    for s in (5, 6, 7):
        ang, tr = ref.pose_error(scene.steps[-1][4][s], scene.T_true[s])
        print(f"seg {s}: {ang:.5f} deg {tr * 1e3:.2f} mm")
        assert tr < 0.005 and ang < 0.02, (s, ang, tr)


# ------------------------------------------------------------------ 7: arguments and allocator balance
def test_argument_checks_and_balance(ctx, scene):
    from pointcloudprocess_amd import _lib, ops
    lib = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr())
    nq = len(scene.q)
    B = len(SIZES)
    offs = (C.c_int64 * (B + 1))(*[int(v) for v in scene.off])
    before = ctx.alloc_stats()[0]

    def create(target=scene.index.h, q=p(scene.dq), stride=12, n=nq, off=offs, nseg=B, out=True):
        h = C.c_void_p()
        rc = lib.pcp_icp_batch_create(ctx.h, target, q, stride, n, off, nseg, C.byref(h) if out else None)
        assert h.value is None or rc == 0
        ctx.sync()
        assert rc == 0 or ctx.alloc_stats()[0] == before, "a rejected create kept blocks"
        return rc, h

    def arr(*v):
        return (C.c_int64 * len(v))(*v)

    assert create(target=None)[0] == -1
    assert create(q=None)[0] == -1
    assert create(off=None)[0] == -1
    assert create(out=False)[0] == -1
    assert create(n=-1, off=arr(0, -1), nseg=1)[0] == -1
    assert create(n=1 << 31, off=arr(0, 1 << 31), nseg=1)[0] == -1
    assert create(nseg=-1)[0] == -1
    assert create(n=0, off=(C.c_int64 * 65537)(), nseg=65536)[0] == -1
    assert create(stride=10)[0] == -1 and create(stride=8)[0] == -1 and create(stride=14)[0] == -1
    assert create(off=arr(1, 5, nq), nseg=2)[0] == -1          # does not start at 0
    assert create(off=arr(0, 5, nq - 1), nseg=2)[0] == -1      # does not end at nq
    assert create(off=arr(0, 9, 5, nq), nseg=3)[0] == -1       # decreases
    ix64 = ops.GridIndex(ctx, scene.dtgt[:500].double())
    mid = ctx.alloc_stats()[0]
    h = C.c_void_p()
    assert lib.pcp_icp_batch_create(ctx.h, ix64.h, p(scene.dq), 12, nq, offs, B, C.byref(h)) == -1  # fp64 index
    assert ctx.alloc_stats()[0] == mid
    ix64.close()
    assert lib.pcp_icp_batch_create(None, scene.index.h, p(scene.dq), 12, nq, offs, B, C.byref(h)) == -1
    assert lib.pcp_icp_batch_destroy(None) == -1

    # stride 0 = 12, a wide stride, 65535 segments (all but the first empty)
    rc, h = create(stride=0)
    assert rc == 0 and lib.pcp_icp_batch_queries(h) == nq and lib.pcp_icp_batch_segments(h) == B
    assert ctx.alloc_stats()[0] == before + 3
    T_dev, stats = scene.batch.new_poses(scene.T0)
    keys = torch.zeros(nq, dtype=torch.int64, device=ctx.device)
    acc = torch.zeros((B, 30), dtype=torch.float64, device=ctx.device)
    pl = scene.planes.h
    assert lib.pcp_icp_batch_keys_dev(ctx.h, None, p(T_dev), RMAX, p(keys)) == -1
    assert lib.pcp_icp_batch_keys_dev(ctx.h, h, None, RMAX, p(keys)) == -1
    assert lib.pcp_icp_batch_keys_dev(ctx.h, h, p(T_dev), RMAX, None) == -1
    assert lib.pcp_icp_batch_keys_dev(ctx.h, h, p(T_dev), -1.0, p(keys)) == -1
    assert lib.pcp_icp_batch_keys_dev(ctx.h, h, p(T_dev), float("nan"), p(keys)) == -1
    assert lib.pcp_icp_batch_accumulate_plane(ctx.h, h, None, p(keys), pl, p(acc)) == -1
    assert lib.pcp_icp_batch_accumulate_plane(ctx.h, h, p(T_dev), None, pl, p(acc)) == -1
    assert lib.pcp_icp_batch_accumulate_plane(ctx.h, h, p(T_dev), p(keys), None, p(acc)) == -1
    assert lib.pcp_icp_batch_accumulate_plane(ctx.h, h, p(T_dev), p(keys), pl, None) == -1
    assert lib.pcp_icp_batch_solve_plane_dev(ctx.h, None, B, p(T_dev), p(stats)) == -1
    assert lib.pcp_icp_batch_solve_plane_dev(ctx.h, p(acc), B, None, p(stats)) == -1
    assert lib.pcp_icp_batch_solve_plane_dev(ctx.h, p(acc), B, p(T_dev), None) == -1
    assert lib.pcp_icp_batch_solve_plane_dev(ctx.h, p(acc), -1, p(T_dev), p(stats)) == -1
    assert lib.pcp_icp_batch_run_plane_dev(ctx.h, None, pl, p(T_dev), RMAX, 1, p(stats)) == -1
    assert lib.pcp_icp_batch_run_plane_dev(ctx.h, h, None, p(T_dev), RMAX, 1, p(stats)) == -1
    assert lib.pcp_icp_batch_run_plane_dev(ctx.h, h, pl, None, RMAX, 1, p(stats)) == -1
    assert lib.pcp_icp_batch_run_plane_dev(ctx.h, h, pl, p(T_dev), RMAX, 1, None) == -1
    assert lib.pcp_icp_batch_run_plane_dev(ctx.h, h, pl, p(T_dev), RMAX, -1, p(stats)) == -1
    small = ops.IcpPlanes(ctx, scene.dtgt[:-1], scene.drows[:-1])
    rc = lib.pcp_icp_batch_run_plane_dev(ctx.h, h, small.h, p(T_dev), RMAX, 1, p(stats))  # planes size != target's
    assert rc == -1 and b"plane records" in lib.pcp_last_error(ctx.h)
    small.close()
    ctx.sync()
    assert np.array_equal(T_dev.cpu().numpy().reshape(-1, 4, 4), scene.T0) and stats.cpu().numpy().max() == 0
    assert ctx.alloc_stats()[0] == before + 3
    assert lib.pcp_icp_batch_destroy(h) == 0
    assert ctx.alloc_stats()[0] == before

    wide = torch.full((nq, 5), 7.5, dtype=torch.float32, device=ctx.device)
    wide[:, :3] = scene.dq
    bw = ops.ICPBatch(scene.index, wide[:, :3], scene.off)
    Tw, _ = bw.new_poses(scene.T0)
    assert np.array_equal(bw.keys_dev(Tw, RMAX).cpu().numpy(), scene.steps[0][2])
    bw.close()
    assert ctx.alloc_stats()[0] == before

    # nseg == 0, and every segment empty: legal, nothing is paired, every solve fails
    e3 = torch.zeros((0, 3), dtype=torch.float32, device=ctx.device)
    b0 = ops.ICPBatch(scene.index, e3, [0])
    assert lib.pcp_icp_batch_segments(b0.h) == 0 and lib.pcp_icp_batch_queries(b0.h) == 0
    T0, s0 = b0.new_poses()
    assert b0.keys_dev(T0, RMAX).numel() == 0 and b0.accumulate_plane(T0, b0.keys_dev(T0, RMAX), scene.planes).numel() == 0
    b0.solve_plane_dev(torch.zeros((0, 30), dtype=torch.float64, device=ctx.device), T0, s0)
    b0.run_plane_dev(scene.planes, T0, s0, RMAX, 2)
    b0.close()
    be = ops.ICPBatch(scene.index, e3, [0, 0, 0, 0])
    Te, se = be.new_poses()
    ke = be.keys_dev(Te, RMAX)
    acc_e = torch.full((3, 30), 5.0, dtype=torch.float64, device=ctx.device)
    be.accumulate_plane(Te, ke, scene.planes, acc=acc_e)
    assert np.array_equal(acc_e.cpu().numpy(), np.zeros((3, 30)))
    be.run_plane_dev(scene.planes, Te, se, RMAX, 2)
    assert np.array_equal(se.cpu().numpy(), np.tile([-1.0, 0, 0, 0], (3, 1)))
    assert np.array_equal(Te.cpu().numpy(), np.tile(np.eye(4).reshape(16), (3, 1)))
    be.close()
    many = np.zeros(65536, dtype=np.int64)
    many[1:] = 70
    bm = ops.ICPBatch(scene.index, scene.dq[:70], many)  # 65535 segments: the first has 70 queries
    Tm, _ = bm.new_poses()
    assert np.array_equal(bm.keys_dev(Tm, RMAX).cpu().numpy(),
                          bref.keys(np.eye(4), scene.q[:70], scene.tgt, RMAX))
    bm.close()
    ctx.sync()
    assert ctx.alloc_stats()[0] == before

    # a rejection reached through the ops layer keeps the allocator balanced
    with pytest.raises(_lib.PcpError) as ei:
        ops.ICPBatch(scene.index, scene.dq, [0, 5, 3, nq])
    assert ei.value.code == -1 and "decrease" in str(ei.value)
    assert ctx.alloc_stats()[0] == before
