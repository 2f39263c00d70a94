"""CloudGrid on the GPU (cloudgrid.hip, pcp_grid_*) at the paths and edges the random scene of
test_cloudgrid.py never reaches, byte-exact on the 48-byte records against the C restatement
(ora.Grid), for small clouds also against the Python one (cloudgrid_ref.PyGrid), and for the
hand-built cases against counts worked out by hand.

  * the de-duplication's brute scan: taken mid-cell, taken before the first arrival because old
    kept points already fill the hash, not taken just under the limit, taken in one cell among
    many -- pcp_grid_last_dedupe says which path ran, and how many arrivals it tested is
    predicted on the CPU (cloudgrid_ref.brute_arrivals);
  * the sub-cell hash: long probe runs, chains, the z field's wrap-around;
  * the duplicate predicate and the match predicate at their boundaries;
  * NaN z, and non-finite or out-of-range x / y (cell INT_MIN on that axis);
  * box ranges, count-only calls, capacity errors, empty grids and inputs, clear and re-add.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cloudgrid_ref as ref
import oracle_ctypes as ora
from cloudgrid_ref import PyGrid
from test_cloudgrid import DEDUPE_CASES, MATCH_CASES, recs, scene

pytestmark = pytest.mark.gpu

HASH_LIMIT = 2048 * 3 // 4  # cloudgrid.hip: kHashSlots * 3 / 4 occupied sub-cells
ERR_CAPACITY = -7


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    c = ops.Context(0)
    yield c
    c.close()


def dev(ctx, cloud):
    from pointcloudprocess_amd import ops
    return ops.cloud_to_device(cloud if cloud.flags.writeable else cloud.copy(), ctx.device)


def host(t):
    from pointcloudprocess_amd import ops
    return ops.cloud_to_host(t)


def gpu_grid(ctx, clouds=()):
    from pointcloudprocess_amd.cloudgrid import CloudGrid
    g = CloudGrid(ctx)
    for c in clouds:
        g.add_cloud_internal(dev(ctx, c))
    return g


def ora_grid(clouds):
    og = ora.Grid()
    for c in clouds:
        og.add_cloud(c)
    return og


def same_points(g, og):
    assert g.size == og.size
    assert np.array_equal(recs(host(g.get_grid_cloud())), recs(og.points()))


def same_match(ctx, g, og, src, dis):
    so, dst = g.get_grid_cloud_match(dev(ctx, src), dis)
    eso, edst = og.match(src, dis)
    so, dst = host(so), host(dst)
    assert np.array_equal(recs(so), recs(eso)) and np.array_equal(recs(dst), recs(edst))
    return so, dst


# the brute column and the oracle's result for it, shared by C1, C3 and C4
@functools.lru_cache(maxsize=None)
def column3000():
    cloud = ref.column(3000, 21)
    kept = ora_grid([cloud]).points()
    cloud.setflags(write=False)
    kept.setflags(write=False)
    return cloud, kept


@functools.lru_cache(maxsize=None)
def scene5000():
    """an ordinary 12 m x 12 m scene and the Python restatement's kept points for it"""
    sc = scene(5000, 31)
    pg = PyGrid()  # 5 000 points over 144 cells are within its reach
    pg.add(sc)
    sc.setflags(write=False)
    return sc, recs(pg.points())


# ---------------------------------------------------------------------------- C1 - C5: paths
def test_brute_fallback_mid_cell(ctx):
    cloud, kept = column3000()
    assert ref.occupied_subcells(kept) > HASH_LIMIT
    switched, tested = ref.brute_arrivals(cloud[:0], cloud)
    assert switched == 1 and 0 < tested < len(cloud)
    g = gpu_grid(ctx, [cloud])
    assert g.last_dedupe == (1, tested)
    assert g.cells == 1 and g.size == len(kept)
    assert np.array_equal(recs(host(g.get_grid_cloud())), recs(kept))
    g.close()


def test_brute_scan_reaches_newest_and_oldest_kept(ctx):
    """In a uniform cloud an arrival's conflict is hardly ever the point kept just before it, so a
    scan that stops one short of the kept list passes the test above.  Here 300 arrivals conflict
    with nothing but the newest kept point, and the last one with the oldest."""
    n, pairs = 2400, 300
    cloud = ref.echo_column(n, pairs, 24)
    og = ora_grid([cloud])
    switched, tested = ref.brute_arrivals(cloud[:0], cloud)
    assert switched == 1 and tested > 2 * pairs + 1  # the switch comes before the tail
    kept = set(og.points()["stamp_id"].tolist())
    fresh_kept = [n + 2 * i in kept for i in range(pairs)]
    assert sum(fresh_kept) > pairs // 2
    assert not any(n + 2 * i + 1 in kept for i in range(pairs) if fresh_kept[i])
    assert 0 in kept and n + 2 * pairs not in kept
    g = gpu_grid(ctx, [cloud])
    assert g.last_dedupe == (1, tested)
    same_points(g, og)
    g.close()


def test_just_under_the_hash_limit(ctx):
    cloud = ref.column(1500, 22)
    og = ora_grid([cloud])
    occ = ref.occupied_subcells(og.points())
    assert HASH_LIMIT * 0.9 < occ <= HASH_LIMIT  # load factor 0.68 .. 0.75 of the 2048 slots
    assert og.size > occ  # and some chains longer than one
    g = gpu_grid(ctx, [cloud])
    assert g.last_dedupe == (0, 0)
    same_points(g, og)
    g.close()


def test_brute_from_the_first_arrival(ctx):
    cloud, kept = column3000()
    second = ref.jittered(kept, 1000, 23, base=10_000)
    og = ora_grid([cloud, second])
    assert len(kept) < og.size < len(kept) + 1000  # some of the second cloud kept, some dropped
    g = gpu_grid(ctx, [cloud])
    g.add_cloud_internal(dev(ctx, second))
    assert g.last_dedupe == (1, 1000) == ref.brute_arrivals(kept, second)
    same_points(g, og)
    before = host(g.get_grid_cloud()).copy()
    g.add_cloud_internal(dev(ctx, second))  # again: every point is now a duplicate
    assert g.last_dedupe == (1, 1000)
    assert g.size == og.size and np.array_equal(recs(host(g.get_grid_cloud())), recs(before))
    g.close()


@pytest.mark.parametrize("shift", [(3.0, 3.0), (-7.0, -9.0)], ids=["brute_cell_last", "brute_cell_inside"])
def test_one_brute_cell_among_many(ctx, shift):
    """The column moved to cell (8, 10), after every key of the scene, or to cell (-1, -1) among the
    scene's points: the cells after it start from a clean hash and the hash path."""
    column, _ = column3000()
    column = column.copy()
    column["x"] += shift[0]
    column["y"] += shift[1]
    column["stamp_id"] += 100_000
    cell = (ref.trunc_x86(column["x"][0]), ref.trunc_x86(column["y"][0]))
    assert cell == ((8, 10) if shift == (3.0, 3.0) else (-1, -1))
    sc, sc_kept = scene5000()
    rng = np.random.default_rng(32)
    cloud = np.concatenate([sc, column])[rng.permutation(len(sc) + len(column))]
    og = ora_grid([cloud])
    keys = sorted({(ref.trunc_x86(p["x"]), ref.trunc_x86(p["y"])) for p in og.points()})
    assert (keys[-1] == cell) == (shift == (3.0, 3.0)) and keys[0] != cell and len(keys) > 100
    assert ref.occupied_subcells(og.box(cell[0], cell[0] + 1, cell[1], cell[1] + 1)) > HASH_LIMIT
    g = gpu_grid(ctx, [cloud])
    assert g.last_dedupe[0] == 1 and g.last_dedupe[1] > 0
    assert g.cells == len(keys)
    same_points(g, og)
    gs = gpu_grid(ctx, [sc])  # the scene alone: no cell near the limit
    assert gs.last_dedupe == (0, 0)
    assert np.array_equal(recs(host(gs.get_grid_cloud())), sc_kept)
    gs.close()
    g.close()


def test_split_add_equals_one_add(ctx):
    a = scene(5000, 41)
    rng = np.random.default_rng(42)
    pick = rng.integers(0, len(a), 3000)
    b = a[pick].copy()
    for ax in "xyz":
        b[ax] += rng.uniform(-0.03, 0.03, len(b))
    b["stamp_id"] = np.arange(len(b), dtype=np.uint32) + 50_000
    og = ora_grid([a, b])
    assert og.size == ora_grid([np.concatenate([a, b])]).size and ora_grid([a]).size < og.size < len(a) + len(b)
    g2, g1 = gpu_grid(ctx, [a, b]), gpu_grid(ctx, [np.concatenate([a, b])])
    same_points(g2, og)
    same_points(g1, og)
    g1.close()
    g2.close()


# ---------------------------------------------------------------------------- C6, C7: predicate
@pytest.mark.parametrize("name,xyz,kept", DEDUPE_CASES, ids=[c[0] for c in DEDUPE_CASES])
def test_dedupe_edges(ctx, name, xyz, kept):
    for order in (slice(None), slice(None, None, -1)):
        cloud = ref.mk(xyz)[order]
        g, og, pg = gpu_grid(ctx, [cloud]), ora_grid([cloud]), PyGrid()
        pg.add(cloud)
        got = recs(host(g.get_grid_cloud()))
        assert g.size == kept, name
        assert np.array_equal(got, recs(og.points())) and np.array_equal(got, recs(pg.points()))
        g.close()
    # the same through a second add: the first point is then an old kept point
    clouds = [ref.mk(xyz[:1]), ref.mk(xyz[1:], base=100)]
    g = gpu_grid(ctx, clouds)
    assert g.size == kept
    same_points(g, ora_grid(clouds))
    g.close()


def test_z_alias_cloud(ctx):
    cloud = ref.z_alias_cloud()
    g, og, pg = gpu_grid(ctx, [cloud]), ora_grid([cloud]), PyGrid()
    pg.add(cloud)
    same_points(g, og)
    assert np.array_equal(recs(host(g.get_grid_cloud())), recs(pg.points()))
    assert g.last_dedupe == (0, 0)
    g.close()


# ---------------------------------------------------------------------------- C8: match
@pytest.mark.parametrize("name,grid,src,dis,ns,nd", MATCH_CASES, ids=[c[0] for c in MATCH_CASES])
def test_match_edges(ctx, name, grid, src, dis, ns, nd):
    gc, sc = ref.mk(grid), ref.mk(src, base=5000)
    g, og, pg = gpu_grid(ctx, [gc]), ora_grid([gc]), PyGrid()
    pg.add(gc)
    same_points(g, og)
    so, dst = same_match(ctx, g, og, sc, dis)
    pso, pdst = pg.match(sc, dis)
    assert (len(so), len(dst)) == (ns, nd), name
    assert np.array_equal(recs(so), recs(pso)) and np.array_equal(recs(dst), recs(pdst))
    if name.startswith("nan_z"):
        assert np.isnan(dst["z"]).sum() == 1
    g.close()


# ---------------------------------------------------------------------------- C9: non-finite x / y
def test_nonfinite_and_out_of_range_cells(ctx):
    cloud, kept, kept_min_row = ref.nonfinite_cloud()
    g, og, pg = gpu_grid(ctx, [cloud]), ora_grid([cloud]), PyGrid()
    pg.add(cloud)
    assert g.size == kept
    same_points(g, og)
    got = host(g.get_grid_cloud())
    assert np.array_equal(recs(got), recs(pg.points()))
    assert all(ref.trunc_x86(p["x"]) == ref.INT_MIN for p in got[:1 + kept_min_row])  # those cells sort first
    row = host(g.box(ref.INT_MIN, ref.INT_MIN + 1, 7, 8))
    assert len(row) == kept_min_row
    assert np.array_equal(recs(row), recs(og.box(ref.INT_MIN, ref.INT_MIN + 1, 7, 8)))
    col = host(g.box(5, 6, ref.INT_MIN, ref.INT_MIN + 1))
    assert len(col) == 2 and np.array_equal(recs(col), recs(og.box(5, 6, ref.INT_MIN, ref.INT_MIN + 1)))
    for src in (ref.mk([(np.nan, 7.5, 1.0)], base=9000), cloud):
        so, dst = same_match(ctx, g, og, src, 0.3)
        assert len(so) > 0
    # a second add meets the old non-finite points
    g.add_cloud_internal(dev(ctx, cloud))
    og.add_cloud(cloud)
    same_points(g, og)
    g.close()


def test_nan_x_source_matches_nothing(ctx):
    name, grid, src, dis, ns, nd = [c for c in MATCH_CASES if c[0] == "nan_x_source"][0]
    g = gpu_grid(ctx, [ref.mk(grid)])
    assert g.size == len(grid) and g.cells == 1
    # the control: a finite source of cell (0, 7) does match, so the cell is populated and tall
    so, dst = g.get_grid_cloud_match(dev(ctx, ref.mk([(0.35, 7.5, 1.0)])), dis)
    assert (len(so), len(dst)) == (1, 2)
    so, dst = g.get_grid_cloud_match(dev(ctx, ref.mk(src)), dis)
    assert len(so) == 0 and len(dst) == 0
    g.close()


# ---------------------------------------------------------------------------- C10: box, lifecycle
@functools.lru_cache(maxsize=None)
def rows_scene():
    """cells in rows 1, 2, 3, 6 and -2 (rows 0, 4, 5 empty), columns -1 .. 2"""
    rng = np.random.default_rng(51)
    xs = np.concatenate([rng.uniform(1.0, 4.0, 600), rng.uniform(6.0, 7.0, 200), rng.uniform(-3.0, -2.0, 200)])
    xyz = np.stack([xs, rng.uniform(-2.0, 3.0, 1000), rng.uniform(0.0, 3.0, 1000)], axis=1)
    cloud = ref.mk(xyz)
    cloud.setflags(write=False)
    return cloud


def test_box_ranges(ctx):
    cloud = rows_scene()
    g, og, pg = gpu_grid(ctx, [cloud]), ora_grid([cloud]), PyGrid()
    pg.add(cloud)
    same_points(g, og)
    boxes = [(-4, 8, -3, 4), (0, 7, 0, 1), (4, 6, -3, 4), (10, 20, 10, 20), (-50, -10, -3, 4), (3, 3, -3, 4),
             (5, 2, -3, 4), (1, 4, 2, 2), (1, 4, 3, -1), (-3, -1, -2, 0), (-2, 0, -1, 1), (6, 7, -1, 3)]
    for b in boxes:
        got = recs(host(g.box(*b)))
        assert np.array_equal(got, recs(og.box(*b))) and np.array_equal(got, recs(pg.box(*b))), b
    assert len(g.box(10, 20, 10, 20)) == 0 and len(g.box(5, 2, -3, 4)) == 0 and len(g.box(4, 6, -3, 4)) == 0
    assert len(g.box(-4, 8, -3, 4)) == g.size
    # get_cloud_with_pos_rot: the default 60 m reach covers a small grid entirely
    rot = np.eye(4)
    rot[0, 3], rot[1, 3] = 2.5, 0.5
    got = host(g.get_cloud_with_pos_rot(rot))
    assert len(got) == g.size and np.array_equal(recs(got), recs(og.box(2 - 60, 2 + 60, 0 - 60, 0 + 60)))
    # the pose is a float matrix: 2.99999999 is 3.0f, cell 3
    rot[0, 3] = 2.99999999
    assert float(np.float32(rot[0, 3])) == 3.0 and int(rot[0, 3]) == 2
    got = host(g.get_cloud_with_pos_rot(rot, 1))
    assert np.array_equal(recs(got), recs(og.box(2, 4, -1, 1)))
    assert not np.array_equal(recs(got), recs(og.box(1, 3, -1, 1)))
    g.close()


def test_count_only_and_capacity(ctx):
    import torch
    cloud = rows_scene()
    g, og = gpu_grid(ctx, [cloud]), ora_grid([cloud])
    lib = ctx.lib
    n = C.c_int64(-1)
    # count only: out_dev NULL
    assert lib.pcp_grid_box(ctx.h, g.h, 1, 4, -3, 4, None, 0, C.byref(n)) == 0
    nbox = len(og.box(1, 4, -3, 4))
    assert n.value == nbox > 0
    assert lib.pcp_grid_points(ctx.h, g.h, None, 0, C.byref(n)) == 0 and n.value == og.size
    # cap one too small: an error, the needed size still reported
    out = torch.zeros((nbox, 48), dtype=torch.uint8, device=ctx.device)
    n.value = -1
    assert lib.pcp_grid_box(ctx.h, g.h, 1, 4, -3, 4, C.c_void_p(out.data_ptr()), nbox - 1, C.byref(n)) == ERR_CAPACITY
    assert n.value == nbox
    assert lib.pcp_grid_box(ctx.h, g.h, 1, 4, -3, 4, C.c_void_p(out.data_ptr()), nbox, C.byref(n)) == 0
    assert np.array_equal(recs(host(out)), recs(og.box(1, 4, -3, 4)))
    src = ref.mk(np.stack([cloud["x"], cloud["y"], cloud["z"]], axis=1)[::3] + 0.01, base=7000)
    eso, edst = og.match(src, 0.3)
    assert len(edst) > 1
    sd = dev(ctx, src)
    so = torch.zeros((len(src), 48), dtype=torch.uint8, device=ctx.device)
    dst = torch.zeros((len(edst), 48), dtype=torch.uint8, device=ctx.device)
    ns, nd = C.c_int64(-1), C.c_int64(-1)
    args = (ctx.h, g.h, C.c_void_p(sd.data_ptr()), len(src), 0.3, C.c_void_p(so.data_ptr()), C.byref(ns),
            C.c_void_p(dst.data_ptr()))
    assert lib.pcp_grid_match(*args, len(edst) - 1, C.byref(nd)) == ERR_CAPACITY
    assert (ns.value, nd.value) == (len(eso), len(edst))
    assert lib.pcp_grid_match(*args, len(edst), C.byref(nd)) == 0
    assert (ns.value, nd.value) == (len(eso), len(edst))
    assert np.array_equal(recs(host(so[:ns.value])), recs(eso)) and np.array_equal(recs(host(dst)), recs(edst))
    same_points(g, og)  # the grid is untouched by the rejected calls
    g.close()


def test_empty_grid_and_empty_inputs(ctx):
    cloud = rows_scene()
    g = gpu_grid(ctx)
    assert (g.size, g.cells, g.last_dedupe) == (0, 0, (0, 0))
    assert len(g.get_grid_cloud()) == 0 and len(g.box(-5, 5, -5, 5)) == 0
    so, dst = g.get_grid_cloud_match(dev(ctx, cloud[:10]), 0.3)
    assert len(so) == 0 and len(dst) == 0
    g.add_cloud_internal(dev(ctx, cloud[:0]))  # 0 points into an empty grid
    assert (g.size, g.cells) == (0, 0)
    g.add_cloud_internal(dev(ctx, cloud))
    og = ora_grid([cloud])
    same_points(g, og)
    g.add_cloud_internal(dev(ctx, cloud[:0]))  # 0 points into a populated one
    assert g.last_dedupe == (0, 0)
    same_points(g, og)
    so, dst = g.get_grid_cloud_match(dev(ctx, cloud[:0]), 0.3)  # no sources
    assert len(so) == 0 and len(dst) == 0
    g.close()


def test_clear_then_readd(ctx):
    cloud, other = rows_scene(), ref.column(300, 61)
    g = gpu_grid(ctx, [other, cloud])
    g.clear()
    assert (g.size, g.cells) == (0, 0) and len(g.get_grid_cloud()) == 0 and len(g.box(-5, 8, -5, 8)) == 0
    g.add_cloud_internal(dev(ctx, cloud))
    fresh = gpu_grid(ctx, [cloud])
    assert np.array_equal(recs(host(g.get_grid_cloud())), recs(host(fresh.get_grid_cloud())))
    same_points(g, ora_grid([cloud]))
    fresh.close()
    g.close()
