"""pcp_radius_count -> pcp_scan_counts -> pcp_radius_fill (the build's radiusSearch) with every
path forced (MI355X), bit for bit against the exhaustive fp64 reference of tests/radius_ref.py
and against the oracle's kd-tree.  The inputs are tests/radius_cases.py's, the same arrays that
tests/test_radius_ref.py holds the oracle to on the CPU and proves to have teeth.

A release build cannot say which pass answered a row, so every search test asserts its own
geometry from the built index: r / ix.cell_size is below 3 cells (the cell-ring pass plus the
far list) or at least 3 (the two-level brick search directly), as the case intends for that
(cell size, r); and pcp_index_cells equals the dense cell product of the bounding box (a dense
table) or is smaller (the brick table), as the case intends.  A changed constant or cell-size
rule fails those asserts instead of quietly moving a case off its path.

Which branch each case forces (numbers: 1 near/far dispatch, 2 sparse grids, 3 non-identity
mapping, 4 row ordering in k_sort_rows, 5 max_nn, 6 strict d2 < r*r, 7 odd queries,
8 pcp_scan_counts):

  lattice          4, 6, 1.  Exact d2 ties by the thousand in every row and >= 1000 pairs exactly
                   on each sphere (asserted on the CPU); cells 0.25 (points on cell faces) and
                   0.1 put r = 0.25 .. 1.25 on both sides of the dispatch (asserted here).
  lattice_mapped   3, 4, 5.  NaN rows plus an `indices` subset: tied rows through the mapping,
                   one run cut by max_nn inside ties.  ix.identity_mapping is asserted False.
  ladder           4, 1, 2, 5.  One query, rows of exactly 1, 2, 3, 63/64/65, 127/128/129,
                   511/512/513, 1023/1024/1025 and 1100 entries (asserted from the reference):
                   a bitonic sort of every pad size, both sides of kSortMax, the in-place
                   insertion sort.  Cells 0.05 (dense; near up to the whole-core row) and 0.01
                   (sparse; far from r >= 0.03).  max_nn in {1, m-1, m, m+1} on the rows of 64
                   and 1025 (append rows against insertion rows) and {size-1, size, size+1}
                   (the "unlimited" switch of radius_cap).
  ladder_nan       3 x 4.  The same with every 7th point NaN: a mapped row at the cap, in the
                   bitonic sort and in the in-place sort.
  ladder_subset    3.  The same through an `indices` subset, rows up to 129.
  duplicates       4, 5.  200 bit-identical points per site: rows that start with 200 entries at
                   d2 == 0; max_nn = 100 cuts inside the tie, 200 at its end; near and far.
  two_clusters     2, 1.  The build must go sparse (asserted: fewer cells than the dense product).
                   r = 0.05 and 0.3 run the ring pass over cell_id's empty bricks, r = 0.5 is
                   3.125 coarsened cells: brick_search over the sparse table.  Queries inside,
                   just outside, and between the clusters (empty rows).
  odd, odd_aos48,  7.  NaN / +-inf rows among finite ones, queries 0.5 / 2 / 10 cells outside the
  odd_everything   box, 1e12 m away (cell_f saturates) with r / h = 2.5 and 5, r = 0, r = 1e200
                   (r*r = inf: every row holds every point), 48-byte query stride.
  none_finite,     7.  An index with no finite point, and with exactly one (a query exactly r
  one_finite       away from it: strict).
  switch_lattice,  1.  r an ulp below, at and an ulp above 3 cells; on the lattice the queries on
  switch_uniform   cell faces are the ones the near pass has to defer.
  normals          ops.normals_radius over rows of 1, 2, 3, 4 and > 1024 points (asserted).
  scan             8.  pcp_scan_counts around one tile, two and three levels, totals past 2^32.

Checked once against builds of radius.hip (then part of knn.hip) with one comparison changed each: `<=` for the strict
`<` (fails lattice, lattice_mapped, one_finite, switch_lattice, the lattice normals), the bitonic
sort comparing d2 alone (lattice, lattice_mapped, duplicates, switch_lattice, the normals), no
mapping after the in-place sort (ladder_nan on both grids), the insertion rows' tie at the cut
decided by d2 alone (lattice_mapped max_nn = 40).  A near pass that never defers passes every
test: below 3 cells the rings hold every hit, the deferral only repeats the work.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_ctypes as ora
import radius_cases as rc
from radius_ref import ref_radius

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)  # a copy: the cases are read-only


def _index(ctx, c, cell):
    from pointcloudprocess_amd import ops
    return ops.GridIndex(ctx, _dev(ctx, c.t), cell_size=cell,
                         indices=None if c.indices is None else torch.from_numpy(c.indices))


def _geometry(ctx, ix, c):
    """(cell size, cells of the index, cells a dense table over the bounding box would have)."""
    h = ix.cell_size
    cells = int(ctx.lib.pcp_index_cells(ix.h))
    p = c.t if c.indices is None else c.t[c.indices]
    p = p[np.isfinite(p).all(1)]
    dense = int(np.prod(np.floor((p.max(0) - p.min(0)) / h) + 2)) if len(p) else None
    return h, cells, dense


def _same(got, want, label):
    (go, gi, gd), (wo, wi, wd) = got, want
    if not np.array_equal(go, wo):
        bad = np.flatnonzero(np.diff(go) != np.diff(wo))
        raise AssertionError(f"{label}: {len(bad)} row lengths differ, first rows {bad[:5].tolist()}: "
                             f"got {np.diff(go)[bad[:5]].tolist()}, expected {np.diff(wo)[bad[:5]].tolist()}")
    for name, g, w in (("indices", gi, wi), ("d2", gd, wd)):
        if not np.array_equal(g, w):
            at = np.flatnonzero(g != w)
            rows = np.unique(np.searchsorted(wo, at, side="right") - 1)
            raise AssertionError(f"{label}: {name} differ in {len(rows)} rows, first rows {rows[:5].tolist()}, "
                                 f"first entry {int(at[0])}: got {g[at[0]]!r}, expected {w[at[0]]!r}")
    assert go.dtype == np.int64 and gi.dtype == np.int32 and gd.dtype == np.float64


@pytest.mark.parametrize("name,grid", rc.GRID_PARAMS, ids=[f"{n}-grid{g}" for n, g in rc.GRID_PARAMS])
def test_radius_paths(ctx, name, grid):
    from pointcloudprocess_amd import ops
    c, ref = rc.case(name)
    g = c.grids[grid]
    ix = _index(ctx, c, g.cell)
    h, cells, dense = _geometry(ctx, ix, c)
    print(f"{name}: cell_size {g.cell} -> {h}, {ix.size} points, cells {cells}, dense product {dense}")
    assert ix.size == ref.size
    assert ix.identity_mapping == (c.indices is None and bool(np.isfinite(c.t).all()))
    # the case's own geometry: which table, and which side of the dispatch every radius is on
    assert np.isclose(h, g.h, rtol=1e-12), (h, g.h)
    if g.sparse is not None:
        assert (cells < dense) == g.sparse and (g.sparse or cells == dense), (cells, dense)
    for r, side in g.side.items():
        far = r / h >= rc.CELL_RINGS
        assert far == (r * (1.0 / h) >= rc.CELL_RINGS)  # no case sits where the two roundings part
        assert far == (side == rc.FAR), (r, h, side)
    q = ops.cloud_to_device(ora.make_cloud(c.q), ctx.device) if c.aos48 else _dev(ctx, c.q)
    for r, max_nn in c.runs:
        got = tuple(a.cpu().numpy() for a in ops.radius(ix, q, r, max_nn))
        label = f"{name} cell={h} r={r!r} max_nn={max_nn}"
        _same(got, ref.rows(r, max_nn), label + " vs the reference")
        _same(got, rc.oracle_rows(name, r, max_nn), label + " vs the oracle")
    ix.close()


# ---------------------------------------------------------------- radius normals
# (case, forced cell size, r, row lengths that must occur)
NORMALS = [("ladder", 0.05, 0.2, (1, 2, 3, 4, 1100)),   # far; the core's rows hold all of it
           ("lattice", 0.25, 0.3, (4, 5, 6, 7)),        # near; corners, edges, faces, interior
           ("lattice", 0.25, 0.75, (23, 93))]           # far; rows of exact ties, corners to interior


@pytest.mark.parametrize("name,cell,r,lengths", NORMALS, ids=[f"{n}-r{r}" for n, _, r, _ in NORMALS])
def test_normals_radius(ctx, name, cell, r, lengths):
    """ops.normals_radius against ora_plane_h_points over the reference's rows, every row, by the
    project's plane rule (|diff| <= 1e-6 max(1, |expected|), NaN equal only to NaN)."""
    from pointcloudprocess_amd import ops
    from test_gpu_normals_paths import _parity
    c, _ = rc.case(name)
    offs, idx, _ = ref_radius(c.t, c.t, r)
    n = np.diff(offs)
    assert set(lengths) <= set(n.tolist()), sorted(set(n.tolist()))[:10]
    assert n.min() >= 1
    if name == "ladder":
        assert (n > 1024).sum() >= 1000
    lib = ora.load()
    e = np.zeros(len(c.t), dtype=ora.PLANE)
    for i in range(len(c.t)):
        nb = np.ascontiguousarray(c.t[idx[offs[i]:offs[i + 1]]])
        lib.ora_plane_h_points(nb.ctypes.data, int(n[i]), e[i:i + 1].ctypes.data)
    ix = _index(ctx, c, cell)
    assert (r / ix.cell_size >= rc.CELL_RINGS) == (r / cell >= rc.CELL_RINGS)
    g = ops.normals_radius(ix, r).cpu().numpy()
    ix.close()
    for m in sorted(set(lengths) | ({1100} if name == "ladder" else set())):
        rows = np.flatnonzero(n == m)
        _parity(g[rows], e[rows], f"{name} r={r} rows of {m}")
    _parity(g, e, f"{name} r={r} all {len(g)} rows")


def test_normals_lengths_cover():
    """Between them the normals cases hold rows of 1, 2, 3, 4 and more than 1024 points."""
    have = set()
    for _, _, _, lengths in NORMALS:
        have |= set(lengths)
    assert {1, 2, 3, 4} <= have and max(have) > 1024


# ---------------------------------------------------------------- pcp_scan_counts
TILE = 2048  # scan.hip: 256 threads x 8 items
SCAN_N = (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, TILE * TILE - 1, TILE * TILE, TILE * TILE + 1)


def _scan(ctx, counts):
    n = len(counts)
    cnt = _dev(ctx, counts) if n else None
    offs = torch.full((n + 1,), -7, dtype=torch.int64, device=ctx.device)
    total = C.c_int64(-7)
    ctx.check(ctx.lib.pcp_scan_counts(ctx.h, C.c_void_p(cnt.data_ptr()) if n else None, n,
                                      C.c_void_p(offs.data_ptr()), C.byref(total)))
    return offs.cpu().numpy(), total.value


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_counts(ctx, n):
    """Offsets 0..n against np.cumsum in int64: one tile, one tile +- 1, a second level
    (n > 2048) and a third (n > 2048^2).  Counts in [0, 7] with runs of zeros (empty rows)."""
    rng = np.random.default_rng(4700 + n % 1000)
    counts = rng.integers(0, 8, n).astype(np.int32)
    for s in rng.integers(0, max(n, 1), 6):
        counts[s:s + int(rng.integers(1, 3 * TILE))] = 0
    if n > TILE:
        counts[TILE - 3:TILE + 5] = 7  # something on both sides of the first tile boundary
    want = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, dtype=np.int64, out=want[1:])
    offs, total = _scan(ctx, counts)
    assert offs.dtype == np.int64 and len(offs) == n + 1
    assert np.array_equal(offs, want), np.flatnonzero(offs != want)[:5]
    assert total == want[n] == offs[n]


def test_scan_counts_past_2_32(ctx):
    """5000 counts up to 2^31 - 1: the running sum passes 2^32 within three entries."""
    rng = np.random.default_rng(4799)
    counts = rng.integers(0, 2**31, 5000).astype(np.int32)
    counts[:3] = 2**31 - 1
    want = np.zeros(5001, dtype=np.int64)
    np.cumsum(counts, dtype=np.int64, out=want[1:])
    assert want[3] > 2**32 and want[-1] > 2**40
    offs, total = _scan(ctx, counts)
    assert np.array_equal(offs, want), np.flatnonzero(offs != want)[:5]
    assert total == want[-1]
