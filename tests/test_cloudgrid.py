"""CloudGrid (cloud_grid.cpp) -- the map cache behind every ICP target.

CPU: the C restatement (oracle/pcp_oracle.c ora_grid_*) against a line-by-line pure-Python
restatement of add_cloud_internal / get_cloud_with_pos / get_grid_cloud on small clouds
(parity unpinned otherwise: the reference has no test or fixture for CloudGrid), and both against
hand-derived counts on the edge inputs of cloudgrid_ref.py: predicate and match boundaries, NaN z,
non-finite and out-of-range x / y (test_gpu_cloudgrid_edges.py runs the same inputs on the GPU).
GPU: libpcp's pcp_grid_* byte-exact against the C restatement: the greedy 4 cm
de-duplication per 1 m cell (including the (int) truncation that merges (-1, 1) into cell 0 and
incremental adds), the box query order, and get_grid_cloud's matching and push order."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_ctypes as ora  # noqa: E402
import cloudgrid_ref as ref  # noqa: E402
from cloudgrid_ref import PyGrid  # noqa: E402


def scene(n, seed, span=6.0, dup=0.3):
    """Points around the origin (negative coordinates: the truncation quirk), a tall
    structure (cells with > 1.5 m of z) and near-duplicates (< 4 cm apart)."""
    rng = np.random.default_rng(seed)
    m = int(n * (1 - dup))
    xyz = np.empty((n, 3))
    xyz[:m, :2] = rng.uniform(-span, span, (m, 2))
    xyz[:m, 2] = rng.normal(0, 0.05, m)
    wall = rng.random(m) < 0.3
    xyz[:m][wall, 2] = rng.uniform(0, 4.0, wall.sum())
    src = rng.integers(0, m, n - m)
    xyz[m:] = xyz[src] + rng.uniform(-0.05, 0.05, (n - m, 3))
    perm = rng.permutation(n)
    return ora.make_cloud(xyz[perm], rgba=rng.integers(0, 2**31, n).astype(np.uint32),
                          stamp=np.arange(n, dtype=np.uint32))


def recs(a):
    return np.asarray([r.tobytes() for r in a])


def test_oracle_grid_vs_python_restatement():
    c1, c2 = scene(3000, 1), scene(2000, 2)
    g, pg = ora.Grid(), PyGrid()
    for c in (c1, c2):
        g.add_cloud(c)
        pg.add(c)
    assert g.size == sum(len(v) for v in pg.cells.values())
    for (i0, i1, j0, j1) in [(-7, 7, -7, 7), (-2, 3, 0, 1), (0, 1, -1, 2)]:
        assert np.array_equal(recs(g.box(i0, i1, j0, j1)), recs(pg.box(i0, i1, j0, j1)))
    src = scene(800, 3)
    so, dst = g.match(src, 0.3)
    pso, pdst = pg.match(src, 0.3)
    assert len(dst) > 0 and np.array_equal(recs(so), recs(pso)) and np.array_equal(recs(dst), recs(pdst))


# ------------------------------------------------------------------ edges (cloudgrid_ref.py)
# The C restatement against the Python one on the hand-built edge inputs, and both against the
# counts worked out by hand: the same inputs run on the GPU in test_gpu_cloudgrid_edges.py.
DEDUPE_CASES = ref.dedupe_cases()
MATCH_CASES = ref.match_cases()


def both(clouds):
    """the clouds added to the C and to the Python restatement; their kept points agree"""
    g, pg = ora.Grid(), PyGrid()
    for c in clouds:
        g.add_cloud(c)
        pg.add(c)
    assert g.size == pg.size
    assert np.array_equal(recs(g.points()), recs(pg.points()))
    return g, pg


def test_trunc_x86():
    t = ref.trunc_x86
    assert [t(v) for v in (0.0, -0.0, 0.99, -0.99, 1.0, -1.0, 5.999, -5.999)] == [0, 0, 0, 0, 1, -1, 5, -5]
    assert t(2147483647.5) == 2**31 - 1 and t(-2147483648.5) == -2**31 and t(-2147483648.0) == -2**31
    for v in (np.nan, np.inf, -np.inf, 2147483648.0, -2147483649.0, 3e10, -3e10, 1e300):
        assert t(v) == -2**31, v


def test_occupied_subcells():
    pts = ref.mk([(0.01, 0.01, 0.01), (0.02, 0.03, 0.04), (0.05, 0.01, 0.01), (-0.01, 0.01, 0.01),
                  (0.01, 0.01, 0.01 + ref.Z_ALIAS)])
    assert ref.occupied_subcells(pts) == 4


@pytest.mark.parametrize("name,xyz,kept", DEDUPE_CASES, ids=[c[0] for c in DEDUPE_CASES])
def test_oracle_dedupe_edges(name, xyz, kept):
    if len(xyz) == 2:  # what each construction claims about its pair
        a, b = xyz
        d = np.abs(a - b)
        if "eq_0.04" in name:
            assert d.max() == ref.DUP_X and ref.sq_dist(a, b) == ref.DUP_2 and float(np.float32(ref.DUP_2)) < ref.DUP_2
        if "above_0.04" in name:
            assert d.max() == np.nextafter(ref.DUP_X, 1.0)
        if "float_rounds_below" in name:
            assert d.max() <= ref.DUP_X and ref.sq_dist(a, b) > ref.DUP_2 > float(np.float32(ref.sq_dist(a, b)))
        if "clearly_above" in name:
            assert d.max() <= ref.DUP_X and float(np.float32(ref.sq_dist(a, b))) > ref.DUP_2
        if name.startswith("subcell"):
            axes = range(3) if "corner" in name else [int(name[len("subcell_face")])]
            sa, sb = np.floor(a / ref.SUB), np.floor(b / ref.SUB)
            assert all(sa[ax] != sb[ax] for ax in axes) and np.sqrt(ref.sq_dist(a, b)) <= 0.0300001
    for order in (slice(None), slice(None, None, -1)):  # the first arrival is the kept one
        cloud = ref.mk(xyz)[order]
        g, pg = both([cloud])
        assert g.size == kept
        assert sorted(recs(g.points())) == sorted(recs(cloud[:kept]))
    g, pg = both([ref.mk(xyz[:1]), ref.mk(xyz[1:], base=100)])  # the same through a second add
    assert g.size == kept


def test_oracle_z_alias_cloud():
    cloud = ref.z_alias_cloud()
    g, pg = both([cloud])
    lo, hi = ora.Grid(), ora.Grid()
    lo.add_cloud(cloud[0::2])
    hi.add_cloud(cloud[1::2])
    assert g.size == lo.size + hi.size and 0 < lo.size < 200 and 0 < hi.size < 200


@pytest.mark.parametrize("name,grid,src,dis,ns,nd", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_oracle_match_edges(name, grid, src, dis, ns, nd):
    gc, sc = ref.mk(grid), ref.mk(src, base=5000)
    g, pg = both([gc])
    assert g.size == len(gc)  # no construction loses a point to the de-duplication
    so, dst = g.match(sc, dis)
    pso, pdst = pg.match(sc, dis)
    assert (len(so), len(dst)) == (ns, nd)
    assert np.array_equal(recs(so), recs(pso)) and np.array_equal(recs(dst), recs(pdst))
    if name.startswith("nan_z"):
        assert np.isnan(dst["z"]).sum() == 1
    if name == "500_sources_50_points":  # cell order, every source
        assert np.array_equal(recs(dst), recs(gc[:50])) and np.array_equal(recs(so), recs(sc))
    if name == "interleaved_sources":
        assert np.array_equal(recs(so), recs(sc[0::4])) and np.array_equal(recs(dst), recs(gc[:50]))


def test_oracle_nonfinite_cells():
    cloud, kept, kept_min_row = ref.nonfinite_cloud()
    g, pg = both([cloud])
    assert g.size == kept
    pts = g.points()
    # the INT_MIN cells sort first: (INT_MIN, INT_MIN), then (INT_MIN, 7)
    assert [ref.trunc_x86(p["x"]) for p in pts[:1 + kept_min_row]] == [ref.INT_MIN] * (1 + kept_min_row)
    assert np.isnan(pts[0]["y"]) and ref.trunc_x86(pts[1 + kept_min_row]["x"]) > ref.INT_MIN
    row = g.box(ref.INT_MIN, ref.INT_MIN + 1, 7, 8)
    assert len(row) == kept_min_row and np.array_equal(recs(row), recs(pg.box(ref.INT_MIN, ref.INT_MIN + 1, 7, 8)))
    assert np.array_equal(recs(row), recs(cloud[[1, 3, 5, 6, 9, 12, 13, 14]]))
    assert len(g.box(0, 1, 7, 8)) == 2 and len(g.box(5, 6, ref.INT_MIN, ref.INT_MIN + 1)) == 2
    for src in (ref.mk([(np.nan, 7.5, 1.0)], base=9000), cloud):
        so, dst = g.match(src, 0.3)
        pso, pdst = pg.match(src, 0.3)
        assert len(so) > 0
        assert np.array_equal(recs(so), recs(pso)) and np.array_equal(recs(dst), recs(pdst))


@pytest.mark.gpu
@pytest.mark.parametrize("n,span", [(20_000, 6.0), (400_000, 40.0)])
def test_gpu_grid_matches_oracle(n, span):
    import torch
    from pointcloudprocess_amd import cloudgrid, ops
    ctx = ops.Context(0)
    c1, c2 = scene(n, 11, span), scene(n // 2, 12, span)
    g, og = cloudgrid.CloudGrid(ctx), ora.Grid()
    for c in (c1, c2):  # two adds: the second one's points meet the first one's kept points
        g.add_cloud_internal(ops.cloud_to_device(c, ctx.device))
        og.add_cloud(c)
    assert g.size == og.size
    got = ops.cloud_to_host(g.get_grid_cloud())
    assert np.array_equal(recs(got), recs(og.points()))
    for mn, mx in [((-3.5, -2.2), (2.5, 4.0)), ((-span, -span), (span, span)), ((0.2, 0.7), (1.0, 1.0))]:
        got = ops.cloud_to_host(g.get_cloud_with_pos(mn, mx))
        exp = og.box(int(mn[0]), math.ceil(mx[0]), int(mn[1]), math.ceil(mx[1]))
        assert np.array_equal(recs(got), recs(exp)), (mn, mx)
    rot = np.eye(4)
    rot[0, 3], rot[1, 3] = -1.7, 2.9
    got = ops.cloud_to_host(g.get_cloud_with_pos_rot(rot, 3))
    assert np.array_equal(recs(got), recs(og.box(-1 - 3, -1 + 3, 2 - 3, 2 + 3)))
    src = scene(n // 4, 13, span)
    so, dst = g.get_grid_cloud_match(ops.cloud_to_device(src, ctx.device), 0.3)
    eso, edst = og.match(src, 0.3)
    assert len(edst) > 0
    assert np.array_equal(recs(ops.cloud_to_host(so)), recs(eso))
    assert np.array_equal(recs(ops.cloud_to_host(dst)), recs(edst))
    g.clear()
    assert g.size == 0
    g.close()
    ctx.close()
