"""GPU checks of the trim by plane residual (include/pcp.h, I3b) against the numpy reference
tests/rtrim_ref.py.  The statistic is one fp64 expression of fp32 inputs rounded once to fp32 and the
selection is integer counting, so outputs and stats are compared for EXACT equality: all n output
keys and all four stats, no tolerances.

The crafted cases use the 1000-record table and the keys of test_gpu_icp_plane._case (every 8th key
INT64_MAX, indices past the table including 0xffffffff, the three invalid records) plus one query
with a NaN coordinate.  Their queries are uniform in a 40 m cube, so the residuals are metres, not
centimetres: the rule is scale-free, and with frac 0.5, mult 1.5 the reference keeps |r| <= 1.5 x
the median, about two thirds of the queries (asserted >= 40 %, so nothing passes by rejecting all).

The scene tests use the cluttered street scene of test_gpu_icp_trim.py (30000 target / 8000 query
points, extent 50 m, 25 % clutter at 0.15 .. 0.45 m, rmax 0.5, GPU normals with k = 16) for
rtrim_ref.SCENE_ITERS = 6 iterations from the identity.  tools/rtrim_reference.py (fp64 CPU: exact
neighbours, fp64 normals) prints for it, after 6 iterations,
    point trim    frac 0.6 mult 1 floor 0.02:   6.87 mm
    residual trim frac 0.5 mult 3 floor 0:      1.21 mm      ratio 5.7
test_scene_accuracy holds the GPU's residual-trimmed error to within 25 % of that 1.21 mm (the margin
is for the GPU's fp32 normals against the tool's fp64 ones) and to at most a third of the error of
the GPU's own point-trimmed loop on the same scene.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import icp_plane_ref as ref
import oracle_ctypes as ora
import rtrim_ref as rr
import trim_ref as tr
from test_gpu_icp_plane import NTAB, _case

pytestmark = pytest.mark.gpu

NO_KEY = tr.NO_KEY
RMAX, ITERS = 0.5, rr.SCENE_ITERS
FRAC, MULT, FLOOR = rr.SCENE_RTRIM
NAN_QUERY = 9  # the crafted query that gets a NaN coordinate (its key is an ordinary one)


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)  # a copy: the shared cases are read-only


def _strided(ctx, a, width):
    full = np.full((a.shape[0], width), 7.5, dtype=np.float32)
    full[:, :3] = a
    return _dev(ctx, full)[:, :3]


def _bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def _crafted(nq):
    """_case(nq) with a NaN coordinate in one query; computed once per size and never modified."""
    T, q, keys, pts, rows = _case(nq, 100 + nq % 97)
    if nq >= 63:
        q[NAN_QUERY, 1] = np.nan
    for a in (T, q, keys, pts, rows):
        a.setflags(write=False)
    return T, q, keys, pts, rows


@functools.lru_cache(maxsize=None)
def _crafted_ref(nq, frac, mult, d_floor):
    T, q, keys, pts, rows = _crafted(nq)
    out, stats = rr.rtrim(T, q, keys, pts, rows[:, :3], frac, mult, d_floor)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


class Table:
    """Device table and queries of a crafted case in one of the two stride layouts."""

    def __init__(self, ctx, nq, wide=False, negate=False):
        from pointcloudprocess_amd import ops
        T, q, keys, pts, rows = _crafted(nq)
        rows = np.where(np.arange(6) < 3, -rows, rows).astype(np.float32) if negate else rows
        if wide:
            self.dq, dp, dn = _strided(ctx, q, 4), _strided(ctx, pts, 4), _dev(ctx, rows)
            assert nq == 0 or self.dq.stride(0) == 4
        else:
            self.dq, dp, dn = _dev(ctx, q), _dev(ctx, pts), _dev(ctx, rows[:, :3])
        self.planes = ops.IcpPlanes(ctx, dp, dn)
        assert self.planes.size == NTAB and self.planes.valid == NTAB - 3
        self.T_dev = _dev(ctx, T.reshape(16))
        self.keys = keys

    def close(self):
        self.planes.close()


def _gpu_rtrim(ctx, tab, keys, frac, mult, d_floor, inplace):
    from pointcloudprocess_amd import ops
    dk = _dev(ctx, keys)
    before = ctx.alloc_stats()[0]
    if inplace:
        out, trim = ops.icp_trim_keys_plane(ctx, tab.T_dev, tab.dq, dk, tab.planes, frac, mult, d_floor, out=dk)
        assert out.data_ptr() == dk.data_ptr()
    else:
        out, trim = ops.icp_trim_keys_plane(ctx, tab.T_dev, tab.dq, dk, tab.planes, frac, mult, d_floor)
        assert np.array_equal(dk.cpu().numpy(), keys)  # the input is left alone
    assert ctx.alloc_stats()[0] == before
    return out.cpu().numpy(), trim.cpu().numpy().view(np.uint64)


def _check(ctx, tab, keys, expect, frac, mult=1.0, d_floor=0.0):
    eo, es = expect
    for inplace in (False, True):
        go, gs = _gpu_rtrim(ctx, tab, keys, frac, mult, d_floor, inplace)
        assert np.array_equal(gs, es), (inplace, frac, mult, d_floor, gs.tolist(), es.tolist())
        assert np.array_equal(go, eo), (inplace, frac, mult, d_floor, int((go != eo).sum()))


# ------------------------------------------------------------------ 1. crafted cases, bit-exact
@pytest.mark.parametrize("wide", [False, True], ids=["q12-t12-n12", "q16-t16-n24"])
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257, 70000, 600000])
def test_crafted_cases_match_reference(ctx, nq, wide):
    """Empty call, partial / full waves, a partial block, several blocks, and 600000 pairs over the
    capped grid (2048 blocks of 256 stride twice); both stride layouts; out of place and in place."""
    eo, es = _crafted_ref(nq, 0.5, 1.5, 0.0)
    print(f"nq={nq} wide={wide} usable={int(es[0])} kept={int(es[1])} "
          f"|r| cut={np.sqrt(es[3:].astype(np.uint32).view(np.float32)[0]):.4g} m")
    if nq >= 63:
        assert es[1] >= 0.4 * nq and es[1] < es[0]  # the reference keeps much and rejects some
        assert eo[NAN_QUERY] == NO_KEY and _crafted(nq)[2][NAN_QUERY] != NO_KEY
    if nq == 0:
        assert es.tolist() == [0, 0, 0, 0]
    tab = Table(ctx, nq, wide)
    _check(ctx, tab, tab.keys, (eo, es), 0.5, 1.5, 0.0)
    tab.close()


# ------------------------------------------------------------------ 2. ties
def test_ties(ctx):
    """20000 of 70000 pairs are copies of one (q, j), hence one rho; frac puts the rank in the middle
    of that run, so sel is its pattern and the whole run is kept."""
    n, ncopy, src = 70000, 20000, 100
    T, q, keys, pts, rows = (a.copy() for a in _crafted(n))
    pos = np.random.default_rng(31).permutation(n)[:ncopy]
    q[pos], keys[pos] = q[src], keys[src]
    rk = rr.residual_keys(T, q, keys, pts, rows[:, :3])
    b = np.sort(tr.high_words(rk[rk != NO_KEY]))
    b_run = int(tr.high_words(rk[src:src + 1])[0])
    lo, hi = np.searchsorted(b, b_run, "left"), np.searchsorted(b, b_run, "right") - 1
    assert hi - lo + 1 >= ncopy and rk[src] != NO_KEY
    frac = float(lo + hi) / 2.0 / (b.size - 1)
    assert lo < tr.rank(frac, b.size) < hi
    eo, es = rr.rtrim(T, q, keys, pts, rows[:, :3], frac)
    assert es.tolist() == [b.size, hi + 1, b_run, b_run] and (eo[pos] == keys[src]).all()
    tab = Table(ctx, n)
    tab.dq = _dev(ctx, q)
    _check(ctx, tab, keys, (eo, es), frac)
    tab.close()


# ------------------------------------------------------------------ 3. extremes
def test_extremes(ctx):
    n = 70000
    T, q, keys, pts, rows = _crafted(n)
    tab = Table(ctx, n)
    rk = rr.residual_keys(T, q, keys, pts, rows[:, :3])
    b = tr.high_words(rk[rk != NO_KEY])
    # frac 0: the smallest residual is the cut, it and its exact ties survive
    eo, es = _crafted_ref(n, 0.0, 1.0, 0.0)
    assert es.tolist() == [b.size, int((b == b.min()).sum()), int(b.min()), int(b.min())] and 1 <= es[1] < 6
    _check(ctx, tab, keys, (eo, es), 0.0)
    # frac 1: the largest residual is the cut, every usable pair survives and only those
    eo, es = _crafted_ref(n, 1.0, 1.0, 0.0)
    assert es.tolist() == [b.size, b.size, int(b.max()), int(b.max())] and np.array_equal(eo != NO_KEY, rk != NO_KEY)
    _check(ctx, tab, keys, (eo, es), 1.0)
    # a floor above every residual (|r| < 1000 m) keeps everything usable whatever frac and mult say
    eo, es = _crafted_ref(n, 0.1, 0.0, 1000.0)
    assert es[1] == es[0] == b.size and es[3] == _bits(1e6) and b.max() < _bits(1e6)
    _check(ctx, tab, keys, (eo, es), 0.1, 0.0, 1000.0)
    # m == 0, by each rule: no key at all, every index past the table, every record invalid
    f2 = _bits(np.float32(0.5) * np.float32(0.5))
    high = tr.high_words(keys)
    for name, k in (("no keys", np.full(n, NO_KEY, dtype=np.int64)),
                    ("past the table", tr.make_keys(high, np.where(np.arange(n) % 2, NTAB, 0xFFFFFFFF))),
                    ("invalid records", tr.make_keys(high, 1 + np.arange(n) % 3))):
        eo, es = rr.rtrim(T, q, k, pts, rows[:, :3], 0.5, 2.0, 0.5)
        assert es.tolist() == [0, 0, 0, f2] and (eo == NO_KEY).all(), name
        _check(ctx, tab, k, (eo, es), 0.5, 2.0, 0.5)
    tab.close()


# ------------------------------------------------------------------ 4. composition, invariance
def test_composition_and_sign_invariance(ctx):
    from pointcloudprocess_amd import ops
    n = 70000
    T, q, keys, pts, rows = _crafted(n)
    eo, es = _crafted_ref(n, 0.5, 1.5, 0.0)
    tab, neg = Table(ctx, n), Table(ctx, n, negate=True)
    go, gs = _gpu_rtrim(ctx, tab, keys, 0.5, 1.5, 0.0, False)
    kept = go != NO_KEY
    assert kept.sum() == gs[1] == es[1]
    assert np.array_equal(go[kept], keys[kept])  # all 64 bits: the high word is still the point d2
    acc = ops.icp_accumulate_plane(ctx, tab.T_dev, tab.dq, _dev(ctx, go), tab.planes).cpu().numpy()
    eacc, _ = ref.accumulate(T, q, eo, pts, rows[:, :3])
    assert acc[0] == int(gs[1]) == eacc[0]
    assert abs(acc[29] - eacc[29]) <= 1e-12 * eacc[29]  # [29] still sums the keys' point d2
    for inplace in (False, True):
        no, ns = _gpu_rtrim(ctx, neg, keys, 0.5, 1.5, 0.0, inplace)
        assert np.array_equal(no, go) and np.array_equal(ns, gs)
    runs = [_gpu_rtrim(ctx, tab, keys, 0.5, 1.5, 0.0, False) for _ in range(2)]
    for ro, rs in runs:  # the same result on every run
        assert np.array_equal(ro, go) and np.array_equal(rs, gs)
    tab.close()
    neg.close()


# ------------------------------------------------------------------ the cluttered street scene
class Scene:
    pass


@pytest.fixture(scope="module")
def scene(ctx):
    """The scene, its GPU normals and plane table, and ONE stepwise residual-trimmed run of ITERS
    iterations (keys_dev, icp_trim_keys_plane in place, icp_accumulate_plane, solve_plane_dev)."""
    from pointcloudprocess_amd import ops, synth
    s = Scene()
    s.T_true = synth.rigid(1.0, 0.4, -0.3, t=(0.15, -0.10, 0.05))
    tgt, q = synth.icp_pair(30000, 8000, 11, 12, s.T_true, extent=(50.0, 50.0))
    s.tgt = tgt.numpy()
    s.q = tr.cluttered_queries(q.numpy(), s.T_true)
    s.dtgt, s.dq = tgt.to(ctx.device), _dev(ctx, s.q)
    ix64 = ops.GridIndex(ctx, tgt.double().to(ctx.device))
    s.drows = ops.normals_knn(ix64, 16)
    ix64.close()
    s.rows = s.drows.cpu().numpy()
    s.index = ops.GridIndex(ctx, s.dtgt, cell_size=0.25)
    s.planes = ops.IcpPlanes(ctx, s.dtgt, s.drows)
    icp = ops.ICP(s.index, s.dq)
    T_dev, stats = icp.new_pose()
    s.steps = []
    for _ in range(ITERS):
        T_prev = T_dev.cpu().numpy().reshape(4, 4).copy()
        keys = icp.keys_dev(T_dev, RMAX)
        raw = keys.cpu().numpy().copy()
        _, trim = ops.icp_trim_keys_plane(ctx, T_dev, s.dq, keys, s.planes, FRAC, MULT, FLOOR, out=keys)
        acc = ops.icp_accumulate_plane(ctx, T_dev, s.dq, keys, s.planes)
        icp.solve_plane_dev(acc, T_dev, stats)
        s.steps.append(dict(T_prev=T_prev, raw=raw, keys=keys.cpu().numpy().copy(),
                            trim=trim.cpu().numpy().view(np.uint64).copy(), acc=acc.cpu().numpy().copy(),
                            T=T_dev.cpu().numpy().reshape(4, 4).copy(), stats=stats.cpu().numpy().copy()))
    icp.close()
    yield s
    s.planes.close()
    s.index.close()


# ------------------------------------------------------------------ 5. scene
def test_scene_steps_match_reference(scene):
    for it, st in enumerate(scene.steps):
        eo, es = rr.rtrim(st["T_prev"], scene.q, st["raw"], scene.tgt, scene.rows[:, :3], FRAC, MULT, FLOOR)
        cut = np.sqrt(es[3:].astype(np.uint32).view(np.float32)[0])
        print(f"it={it} m={int(es[0])} kept={int(es[1])} |r| cut={cut:.4f} m pairs={int(st['acc'][0])} "
              f"err={ref.pose_error(st['T'], scene.T_true)}")
        assert np.array_equal(st["trim"], es), (it, st["trim"].tolist(), es.tolist())
        assert np.array_equal(st["keys"], eo), (it, int((st["keys"] != eo).sum()))
        assert 6 <= es[1] < es[0]  # the trim did reject pairs
        assert st["acc"][0] == int(es[1])


def test_device_loop_equals_stepwise(ctx, scene):
    from pointcloudprocess_amd import ops
    icp = ops.ICP(scene.index, scene.dq)
    before = ctx.alloc_stats()[0]
    T_dev, stats = icp.new_pose()
    trim = icp.run_plane_rtrimmed_dev(scene.planes, scene.dq, T_dev, stats, RMAX, FRAC, MULT, FLOOR, ITERS)
    T = T_dev.cpu().numpy().reshape(4, 4)
    st = stats.cpu().numpy()
    tm = trim.cpu().numpy().view(np.uint64)
    assert ctx.alloc_stats()[0] == before
    icp.close()
    last = scene.steps[-1]
    assert st[3] == ITERS and st[0] == 0
    assert np.array_equal(T.view(np.int64), last["T"].view(np.int64))  # bit for bit
    assert np.array_equal(st, last["stats"])
    assert np.array_equal(tm, last["trim"])


def test_scene_accuracy(ctx, scene):
    from pointcloudprocess_amd import ops
    ang, trn = ref.pose_error(scene.steps[-1]["T"], scene.T_true)
    icp = ops.ICP(scene.index, scene.dq)
    T_dev, stats = icp.new_pose()
    pf, pm, pd = rr.SCENE_PTRIM
    icp.run_plane_trimmed_dev(scene.planes, scene.dq, T_dev, stats, RMAX, pf, pm, pd, ITERS)
    ang_p, trn_p = ref.pose_error(T_dev.cpu().numpy().reshape(4, 4), scene.T_true)
    icp.close()
    kept = int(scene.steps[-1]["trim"][1])
    print(f"residual trim: {trn * 1e3:.3f} mm {ang:.4f} deg ({kept} kept), deviation from the fp64 figure "
          f"{100 * (trn / rr.REF_RTRIMMED_M - 1):+.1f} %; point trim: {trn_p * 1e3:.3f} mm {ang_p:.4f} deg "
          f"(fp64 figure {rr.REF_POINT_TRIMMED_M * 1e3:.2f} mm); ratio {trn_p / trn:.2f}")
    assert abs(trn - rr.REF_RTRIMMED_M) <= 0.25 * rr.REF_RTRIMMED_M
    assert trn <= trn_p / 3.0


def test_get_rot_icp_plane_rtrimmed(ctx, scene):
    """The AoS48 entry equals its own steps done by hand (joint centroid, fp32 centring, automatic
    cell size, normals of the fp64 src, plane table, the residual-trimmed loop, un-centring): the
    same pose within the bound test_gpu_icp_trim.py uses for this step, and kept_out == trim[1] of
    the last iteration."""
    from pointcloudprocess_amd import ops
    s_xyz, t_xyz = scene.tgt.astype(np.float64), scene.q.astype(np.float64)
    src = ops.cloud_to_device(ora.make_cloud(s_xyz), ctx.device)
    tmp = ops.cloud_to_device(ora.make_cloud(t_xyz), ctx.device)
    before = ctx.alloc_stats()[0]
    err, M, kept = ops.get_rot_icp_plane_rtrimmed(ctx, src, tmp, RMAX, FRAC, MULT, FLOOR, iters=ITERS, normals_k=16)
    assert ctx.alloc_stats()[0] == before
    ang, trn = ref.pose_error(M, scene.T_true)
    print(f"get_rot rtrimmed: err={err:.5f} {trn * 1e3:.3f} mm {ang:.4f} deg kept={kept}")
    assert np.isfinite(M).all() and err > 0 and kept >= 6
    assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() < 1e-14
    c = ops.centroid_concat(ctx, src, tmp)[0][:3]
    fs, ft = _dev(ctx, (s_xyz - c).astype(np.float32)), _dev(ctx, (t_xyz - c).astype(np.float32))
    index = ops.GridIndex(ctx, fs)
    icp = ops.ICP(index, ft)
    ix64 = ops.GridIndex(ctx, src)
    rows = ops.normals_knn(ix64, 16)
    ix64.close()
    planes = ops.IcpPlanes(ctx, fs, rows)
    T_dev, stats = icp.new_pose()
    trim = icp.run_plane_rtrimmed_dev(planes, ft, T_dev, stats, RMAX, FRAC, MULT, FLOOR, ITERS)
    T = T_dev.cpu().numpy().reshape(4, 4).copy()
    T[:3, 3] = (T[:3, 3] - T[:3, :3] @ c) + c
    st = stats.cpu().numpy()
    planes.close()
    icp.close()
    index.close()
    assert kept == int(trim.cpu().numpy()[1])
    assert np.abs(M - T).max() < 1e-12 and abs(err - st[1]) < 1e-6 * st[1]
    assert ctx.alloc_stats()[0] == before


def test_trim_to_fewer_than_six_pairs_freezes_pose(ctx, scene):
    """frac = 0 with no floor keeps the smallest residual (and its exact ties) only: the solve fails,
    the status latches and T stays where it was."""
    from pointcloudprocess_amd import ops
    icp = ops.ICP(scene.index, scene.dq)
    T_dev, stats = icp.new_pose()
    trim = icp.run_plane_rtrimmed_dev(scene.planes, scene.dq, T_dev, stats, RMAX, 0.0, 1.0, 0.0, 2)
    st, tm = stats.cpu().numpy(), trim.cpu().numpy()
    icp.close()
    assert 1 <= tm[1] < 6 and st[0] == -1 and st[3] == 0
    assert np.array_equal(T_dev.cpu().numpy().reshape(4, 4), np.eye(4))


# ------------------------------------------------------------------ 6. arguments and allocation
def test_trim_keys_plane_argument_errors(ctx):
    n = 257
    tab = Table(ctx, n)
    dk = _dev(ctx, tab.keys)
    out = torch.full((n,), 55, dtype=torch.int64, device=ctx.device)
    trim = torch.full((4,), 77, dtype=torch.int64, device=ctx.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib = ctx.lib
    before = ctx.alloc_stats()[0]
    nan, inf = float("nan"), float("inf")
    good = [ctx.h, p(tab.T_dev), p(tab.dq), 12, n, p(dk), tab.planes.h, 0.5, 1.0, 0.0, p(out), p(trim)]
    for pos, bad in ((0, None), (1, None), (2, None), (3, 10), (3, 8), (3, 13), (4, -1), (4, 1 << 31), (5, None), (6, None),
                     (7, -0.01), (7, 1.5), (7, nan), (8, -1.0), (8, inf), (8, nan), (9, -0.1), (9, inf), (9, nan),
                     (10, None), (11, None)):
        args = list(good)
        args[pos] = bad
        assert lib.pcp_icp_trim_keys_plane(*args) == -1, (pos, bad)
        assert ctx.alloc_stats()[0] == before
    assert out.cpu().tolist() == [55] * n and trim.cpu().tolist() == [77] * 4  # a rejected call writes nothing
    assert np.array_equal(dk.cpu().numpy(), tab.keys)
    # stride 0 is 12; n == 0 with null query and key pointers is a valid call
    good[3] = 0
    assert lib.pcp_icp_trim_keys_plane(*good) == 0
    eo, es = _crafted_ref(n, 0.5, 1.0, 0.0)
    assert np.array_equal(out.cpu().numpy(), eo) and np.array_equal(trim.cpu().numpy().view(np.uint64), es)
    assert lib.pcp_icp_trim_keys_plane(ctx.h, p(tab.T_dev), None, 12, 0, None, tab.planes.h, 0.5, 2.0, 0.5, None,
                                       p(trim)) == 0
    assert trim.cpu().tolist() == [0, 0, 0, _bits(0.25)]
    assert ctx.alloc_stats()[0] == before
    tab.close()


def test_loop_argument_errors(ctx, scene):
    from pointcloudprocess_amd import _lib, ops
    lib = ctx.lib
    before = ctx.alloc_stats()[0]
    icp = ops.ICP(scene.index, scene.dq)
    mid = ctx.alloc_stats()[0]
    T_dev, stats = icp.new_pose()
    with pytest.raises(_lib.PcpError) as ei:  # nq != the handle's count
        icp.run_plane_rtrimmed_dev(scene.planes, scene.dq[:-1], T_dev, stats, RMAX, FRAC, MULT, FLOOR, 1)
    assert ei.value.code == -1 and "queries" in str(ei.value)
    small = ops.IcpPlanes(ctx, scene.dtgt[:-1], scene.drows[:-1])
    with pytest.raises(_lib.PcpError) as ei:  # planes size != the target's
        icp.run_plane_rtrimmed_dev(small, scene.dq, T_dev, stats, RMAX, FRAC, MULT, FLOOR, 1)
    assert ei.value.code == -1 and "plane records" in str(ei.value)
    small.close()
    assert ctx.alloc_stats()[0] == mid
    p = lambda t: C.c_void_p(t.data_ptr())
    nq = scene.dq.shape[0]
    trim = torch.full((4,), 77, dtype=torch.int64, device=ctx.device)
    good = [ctx.h, icp.h, scene.planes.h, p(scene.dq), 12, nq, p(T_dev), RMAX, FRAC, MULT, FLOOR, 1, p(stats), p(trim)]
    for pos, bad in ((1, None), (2, None), (3, None), (6, None), (12, None), (13, None), (4, 10), (7, -1.0),
                     (8, 1.5), (8, float("nan")), (9, -1.0), (9, float("inf")), (10, -0.1), (10, float("nan")),
                     (11, -1)):
        args = list(good)
        args[pos] = bad
        assert lib.pcp_icp_run_plane_rtrimmed_dev(*args) == -1, (pos, bad)
    assert np.array_equal(T_dev.cpu().numpy(), np.eye(4).reshape(16)) and stats.cpu().numpy().max() == 0
    assert trim.cpu().tolist() == [77] * 4
    assert ctx.alloc_stats()[0] == mid
    good[11] = 0  # iters == 0: nothing runs, trim_dev is untouched
    assert lib.pcp_icp_run_plane_rtrimmed_dev(*good) == 0 and trim.cpu().tolist() == [77] * 4
    icp.close()
    assert ctx.alloc_stats()[0] == before
    cloud = ops.cloud_to_device(ora.make_cloud(scene.tgt[:500].astype(np.float64)), ctx.device)
    for rmax in (0.0, -1.0):
        with pytest.raises(_lib.PcpError) as ei:
            ops.get_rot_icp_plane_rtrimmed(ctx, cloud, cloud, rmax, FRAC, iters=2)
        assert ei.value.code == -5  # PCP_ERR_UNSUPPORTED
    for frac, mult, fl in ((1.5, 1.0, 0.0), (0.5, -1.0, 0.0), (0.5, 1.0, float("inf"))):
        with pytest.raises(_lib.PcpError) as ei:
            ops.get_rot_icp_plane_rtrimmed(ctx, cloud, cloud, RMAX, frac, mult, fl, iters=2)
        assert ei.value.code == -1
    assert ctx.alloc_stats()[0] == before


def test_zero_queries(ctx):
    """nq == 0 behaves as the point-trimmed loop does: the solve fails, T is frozen, the trim of no
    pairs reports {0, 0, 0, bits(f2)}."""
    from pointcloudprocess_amd import ops
    rng = np.random.default_rng(8)
    tgt = _dev(ctx, rng.uniform(-5, 5, (2000, 3)).astype(np.float32))
    nrm = _dev(ctx, np.tile(np.float32([0, 0, 1]), (2000, 1)))
    e3 = torch.zeros((0, 3), dtype=torch.float32, device=ctx.device)
    before = ctx.alloc_stats()[0]
    index = ops.GridIndex(ctx, tgt, cell_size=0.25)
    planes = ops.IcpPlanes(ctx, tgt, nrm)
    icp = ops.ICP(index, e3)
    T_dev, stats = icp.new_pose()
    trim = icp.run_plane_rtrimmed_dev(planes, e3, T_dev, stats, RMAX, 0.5, 2.0, 0.5, 2)
    assert trim.cpu().tolist() == [0, 0, 0, _bits(0.25)]
    assert stats.cpu().numpy()[0] == -1 and np.array_equal(T_dev.cpu().numpy(), np.eye(4).reshape(16))
    icp.close()
    planes.close()
    index.close()
    assert ctx.alloc_stats()[0] == before
