"""The 23 Kabsch accumulators of every ICP pass, bit for bit (MI355X).

Inputs on which every fp32 intermediate of the accumulation is a representable number: all
coordinates are multiples of h = 2^-5 m, the queries lie in a 64-step box offset by (1024, -512,
256) m, rmax is at most 16 steps, and the poses are lattice translations, alone or after a 90
degree turn about z, so the fp32 chain R q + t is exact too.  Then a wave's centred fp32 sums
(chunk_accumulate: 64 pairs; LaneAcc: 32 chunks x 64 lanes) stay below 2048 * 63 * 79 < 2^24 steps^2
and every un-centred fp64 term below 2^53: any summation order gives the same 23 doubles, and
kabsch_ref.exact_acc (integer arithmetic on the reference's own pairs) must be met with
np.array_equal.  exact_acc returns those bounds for the data at hand and every test asserts them
before it looks at the GPU's numbers.  A wrong term in the un-centring, a dropped d2 or a lane /
value mix-up on a partial chunk changes an integer, which no tolerance hides.

Correspondences and d2 are compared with kabsch_ref.correspond (the lattice is dense in ties, so
the (d2, index) order is stressed as well).  Every pass that writes accumulators is shown to have
had work (last_searched, last_fallback, the pair count); no pass is ever switched off.
"""
import functools

import numpy as np
import pytest
import torch

import kabsch_ref as kr

pytestmark = pytest.mark.gpu

H = 2.0 ** -5
OFF = np.array([1024.0, -512.0, 256.0])
NQS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4500]
ROT90Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def pose(steps, R=None):
    """[R, t]: R (identity or the quarter turn) about the box's corner, then `steps` lattice steps."""
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
        T[:3, 3] = OFF - R @ OFF + [63 * H, 0.0, 0.0]  # the turned box lands on the box
    T[:3, 3] += np.asarray(steps, dtype=np.float64) * H
    return T


@functools.lru_cache(maxsize=None)
def scene(nq, nt, seed):
    """(queries with three non-finite rows mixed in, targets), fp32.  Queries: nq lattice points of
    the 64-step box.  Targets: nt distinct lattice points of the box grown by 8 steps, none beyond
    step 40 in x, so the queries near the far x face have nothing within rmax; nt <= 2: at the
    box's centre, one step apart (every query between them is a tie)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 64, (nq, 3)).astype(np.float64) * H + OFF
    if nt <= 2:
        t = (np.array([[32, 32, 32], [33, 32, 32]], dtype=np.float64)[:nt]) * H + OFF
    else:
        sites = rng.choice(49 * 80 * 80, nt, replace=False)
        t = np.stack([sites // 6400 - 8, (sites // 80) % 80 - 8, sites % 80 - 8], 1).astype(np.float64) * H + OFF
    bad = np.array([[np.nan, OFF[1], OFF[2]], [OFF[0], np.inf, OFF[2]], [np.nan, np.nan, np.nan]])
    at = rng.permutation(nq + 3)[:3]
    full = np.empty((nq + 3, 3))
    mask = np.ones(nq + 3, bool)
    mask[at] = False
    full[mask] = q
    full[~mask] = bad
    return full.astype(np.float32), t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _expected(nq, nt, seed, tkey, rmax, lo, hi):
    q, tgt = scene(nq, nt, seed)
    T = np.array(tkey).reshape(4, 4)
    img, exact_pose = kr.xform32(T, q)
    fin = np.isfinite(q).all(1)
    assert exact_pose and np.isfinite(img[fin]).all()
    ei, ed, exact_d2 = kr.correspond(tgt, img, rmax)
    assert exact_d2
    m = (ei >= lo) & (ei < hi)
    acc, info = kr.exact_acc(img[m], tgt[ei[m]], ed[m], centres=img[fin])
    return ei, ed, acc, info


def expected(nq, nt, seed, T, rmax, lo=0, hi=1 << 31):
    """The reference at pose T: correspondences, d2, the exact sums over the pairs whose target
    index is in [lo, hi), and the exactness conditions -- asserted here, before any GPU number."""
    ei, ed, acc, info = _expected(nq, nt, seed, tuple(np.asarray(T, dtype=np.float64).ravel()), float(rmax), lo, hi)
    assert info["fp32"] and info["exact64"] and info["k"] <= 5
    assert info["bound"] < 2 ** 24 and info["bound64"] < 2 ** 53, info
    return ei, ed, acc


def make(ctx, nq, nt, seed, cell):
    from pointcloudprocess_amd import ops
    q, tgt = scene(nq, nt, seed)
    index = ops.GridIndex(ctx, torch.from_numpy(tgt).to(ctx.device), cell_size=cell)
    return index, ops.ICP(index, torch.from_numpy(q).to(ctx.device))


def run_steps(icp, nq, nt, seed, poses, rmax):
    """Steps through `poses`, comparing everything at each; returns per step (pairs, settled by the
    verify pass, searched, fallback)."""
    work = []
    for it, T in enumerate(poses):
        ei, ed, eacc = expected(nq, nt, seed, T, rmax)
        acc, ci, cd = icp.step(T, rmax, corr=True)
        gi, gd, gacc = ci.cpu().numpy(), cd.cpu().numpy(), acc.cpu().numpy().copy()
        assert np.array_equal(gi, ei), f"step {it}: {(gi != ei).sum()} mismatching correspondences"
        assert np.array_equal(gd[ei >= 0], ed[ei >= 0]), f"step {it}"
        assert np.array_equal(gacc[:23], eacc), f"step {it}: accumulators {np.flatnonzero(gacc[:23] != eacc)} differ"
        searched = icp.last_searched()
        work.append((int(eacc[0]), nq - searched, searched, icp.last_fallback()))
    return work


WALK = [pose((0, 0, 0)), pose((1, 0, 0)), pose((1, 0, 0)), pose((1, 1, 0)), pose((1, 1, -1))]


@pytest.mark.parametrize("nt,cell,rmax", [(1, 0.1, 0.5), (2, 0.3, 0.5), (3000, 0.1, 0.25), (3000, 0.3, 0.5)])
@pytest.mark.parametrize("nq", NQS)
def test_shapes(ctx, nq, nt, cell, rmax):
    """Every chunk and stretch edge of the query count, against 1, 2 and 3000 targets: the
    first-launch octant kernel (step 0 searches everything), then the verify pass with the octant
    list pass and the fallback behind it, at poses one lattice step apart and at a repeated pose."""
    index, icp = make(ctx, nq, nt, 100 + nq, cell)
    work = run_steps(icp, nq, nt, 100 + nq, WALK, rmax)
    print(f"nq {nq} nt {nt} cell {cell}: (pairs, settled, searched, fallback) per step {work}")
    assert work[0][2] == nq and work[0][1] == 0  # the first launch: every finite query searched
    if nq >= 63:  # (fewer queries may all take one path)
        assert all(0 < w[0] < nq for w in work), work  # pairs, and queries with nothing within rmax
        # the verify pass settled queries one step away and at the repeated pose ...
        assert min(work[1][1], work[2][1], work[3][1], work[4][1]) > 0, work
        # ... the octant pass settled some of the list it left (not all of it fell through) ...
        assert sum(w[2] - w[3] for w in work[1:]) > 0, work
        # ... and the fallback ran behind the first launch and behind the lists
        assert work[0][3] > 0 and min(w[3] for w in work[1:]) > 0, work
        if nt == 3000:  # more pairs than searched queries: the verify pass wrote pairs of its own
            assert max(w[0] - w[2] for w in work[1:]) > 0, work
    icp.close()
    index.close()


@pytest.mark.parametrize("nq", [65, 2049])
def test_quarter_turn_poses(ctx, nq):
    """R = a quarter turn about z (exact in the fp32 chain) and lattice translations."""
    index, icp = make(ctx, nq, 3000, 7, 0.1)
    poses = [pose((0, 0, 0), ROT90Z), pose((0, 1, 0), ROT90Z), pose((0, 1, 0), ROT90Z), pose((-1, 1, 1), ROT90Z)]
    work = run_steps(icp, nq, 3000, 7, poses, 0.25)
    assert all(w[0] > 0 for w in work) and work[2][1] > 0, work
    icp.close()
    index.close()


@pytest.mark.parametrize("g", [1, 2, 4, 8])
def test_lane_groups(ctx, g):
    """G lanes per query in the octant passes (first launch and lists) and in the fallback."""
    nq = 2049
    index, icp = make(ctx, nq, 3000, 11, 0.1)
    icp.set_options(oct_lanes_first=g, oct_lanes_list=g, ring_lanes=g)
    work = run_steps(icp, nq, 3000, 11, WALK, 0.25)
    assert work[0][2] == nq and work[0][3] > 0, work                  # first-launch octant, fallback
    assert sum(w[1] for w in work[1:]) > 0, work                      # verify
    assert sum(w[2] for w in work[1:]) > 0 and sum(w[3] for w in work[1:]) > 0, work  # list pass, its fallback
    icp.close()
    index.close()


@pytest.mark.parametrize("lookahead", [True, False])
@pytest.mark.parametrize("wide", [False, True])
def test_cache_forms_and_lookahead(ctx, wide, lookahead):
    """12-byte and 16-byte cache records, with the search centred ahead on the path (from the third
    launch of a shrinking walk) and on the query itself."""
    nq = 2049
    index, icp = make(ctx, nq, 3000, 13, 0.3)
    icp.set_options(wide_cache=wide, lookahead=lookahead)
    # steps of 4, 2, 1, 1 lattice steps along x: a shrinking, collinear walk
    poses = [pose((0, 0, 0)), pose((4, 0, 0)), pose((6, 0, 0)), pose((7, 0, 0)), pose((8, 0, 0))]
    work, betas = [], []
    for k in range(len(poses)):
        work += run_steps(icp, nq, 3000, 13, poses[k:k + 1], 0.5)
        betas.append(icp.last_lookahead()[0])
    assert sum(w[1] for w in work[1:]) > 0 and sum(w[2] for w in work[1:]) > 0, work
    assert (max(betas[2:]) > 0) == lookahead and betas[0] == betas[1] == 0, betas
    icp.close()
    index.close()


def test_graph_replay_device_poses(ctx):
    """Device-pose launches with PCP_ICP_OPT_GRAPH (the chain is replayed from the third launch)."""
    nq = 2049
    index, icp = make(ctx, nq, 3000, 17, 0.1)
    icp.set_options(graph=True)
    T_dev, _ = icp.new_pose()
    for it, T in enumerate(WALK + [pose((2, 1, -1)), pose((2, 1, -1))]):
        _, _, eacc = expected(nq, 3000, 17, T, 0.25)
        T_dev.copy_(torch.from_numpy(T.reshape(16).copy()).to(ctx.device))
        gacc = icp.step_dev(T_dev, 0.25).cpu().numpy().copy()
        assert eacc[0] > 0
        assert np.array_equal(gacc[:23], eacc), f"launch {it}: accumulators {np.flatnonzero(gacc[:23] != eacc)} differ"
    icp.close()
    index.close()


def test_sparse_grid_box_search(ctx):
    """A second lattice cluster 64 m away along every axis makes the dense cell table too large:
    the index keeps bricks and every query goes through the general box search, at every launch."""
    from pointcloudprocess_amd import ops
    nq, seed = 2049, 19
    q, tgt = scene(nq, 3000, seed)
    far = (tgt[:100].astype(np.float64) + 64.0).astype(np.float32)
    both = np.concatenate([tgt, far])
    index = ops.GridIndex(ctx, torch.from_numpy(both).to(ctx.device), cell_size=0.1)
    assert ctx.lib.pcp_index_cells(index.h) < 0.5 * 660 ** 3  # bricks, not the (66 m / 0.1 m)^3 table
    icp = ops.ICP(index, torch.from_numpy(q).to(ctx.device))
    for it, T in enumerate(WALK[:3]):
        ei, ed, eacc = expected(nq, 3000, seed, T, 0.25)  # the far cluster is out of every query's reach
        acc, ci, cd = icp.step(T, 0.25, corr=True)
        assert np.array_equal(ci.cpu().numpy(), ei) and np.array_equal(cd.cpu().numpy()[ei >= 0], ed[ei >= 0])
        assert eacc[0] > 0 and np.array_equal(acc.cpu().numpy()[:23], eacc), f"step {it}"
        assert icp.last_searched() == nq  # no verify pass on a sparse grid: all searched, every time
    icp.close()
    index.close()


def test_sharded_accumulations(ctx):
    """accumulate_keys (host pose) and keys_owner + accumulate_owned (device pose) over two target
    shards: each shard's sums are the exact sums of the pairs whose winner it owns."""
    from pointcloudprocess_amd import distributed as D, ops
    nq, nt, seed = 2049, 3000, 23
    q, tgt = scene(nq, nt, seed)
    dq = torch.from_numpy(q).to(ctx.device)
    bounds = [0, 1300, nt]
    engines = [D.GpuEngine(ctx, torch.from_numpy(tgt[bounds[r]:bounds[r + 1]]).to(ctx.device), dq, cell_size=0.1)
               for r in range(2)]
    bnd = torch.tensor(bounds, dtype=torch.int64, device=ctx.device)
    T_dev, _ = engines[0].new_pose(np.eye(4))
    for T in (pose((0, 0, 0)), pose((1, -1, 0), ROT90Z)):
        ei, ed, _ = expected(nq, nt, seed, T, 0.25)
        local = [engines[r].keys(T, 0.25, bounds[r]) for r in range(2)]
        keys = torch.minimum(local[0], local[1])
        k = keys.cpu().numpy()
        none = k == np.iinfo(np.int64).max
        assert np.array_equal(none, ei < 0)
        assert np.array_equal((k[~none] & 0xFFFFFFFF).astype(np.int32), ei[~none])
        assert np.array_equal((k[~none] >> 32).astype(np.uint32).view(np.float32), ed[~none])
        T_dev.copy_(torch.from_numpy(T.reshape(16).copy()).to(ctx.device))
        local_dev = [engines[r].keys_dev(T_dev, 0.25, bounds[r]).clone() for r in range(2)]
        owner = ops.keys_owner(ctx, torch.minimum(local_dev[0], local_dev[1]), bnd)
        for r in range(2):
            _, _, eacc = expected(nq, nt, seed, T, 0.25, bounds[r], bounds[r + 1])
            assert eacc[0] > 0
            a = engines[r].accumulate_keys(T, keys, bounds[r], bounds[r + 1]).cpu().numpy().copy()
            assert np.array_equal(a[:23], eacc), f"accumulate_keys, shard {r}"
            b = engines[r].accumulate_owned(T_dev, local_dev[r], owner, r, bounds[r], bounds[r + 1]).cpu().numpy().copy()
            assert np.array_equal(b[:23], eacc), f"accumulate_owned, shard {r}"
    for e in engines:
        e.close()
