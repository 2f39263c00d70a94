"""pcp_knn (the build's nearestKSearch) with both search passes forced (MI355X), bit for bit
against the exhaustive fp64 reference of tests/knn_ref.py -- np.array_equal on indices and on
d2, padding and non-finite rows included, no tolerance -- and against the oracle's kd-tree.
The inputs are tests/knn_grid_cases.py's, the same arrays that tests/test_knn_grid_ref.py holds
the oracle to on the CPU and proves to have teeth.

A release build cannot say which pass answered a row, so every call is followed by
pcp_knn_last_far: the number of queries the near pass (k_knn<K, false>: one lane per query,
cell rings 0..3) deferred to the far pass (k_knn_coop<K>: one wave per query) must lie between
the rows the reference says cannot be answered within the rings and the rows it says must be
(knn_grid_cases.classify).  The table the build chose (dense, or bricks: pcp_index_cells below
the dense product of the bounding box) and the cell size it kept are asserted too.  A changed
constant or cell-size rule fails those asserts instead of quietly moving a case off its path.
The library is called through _knn, which pre-fills the outputs with sentinels: an entry that
no pass wrote is seen as such.

Which branch of the far pass each case forces (numbers: 1 the K = 1 .. 64 instantiations,
2 the brick phase over a dense table (row masks), 3 the brick phase over a brick table (all 16
rows, slot-relative cell starts), 4 queries outside the grid (farb > 0, negative cells, the
saturated cell coordinate), 5 the merge of exact ties across lanes, 6 the write-out: padding
[kk, k), no d2 buffer, the mapping, 7 the far kernel's grid-stride loop, 8 near and far rows
in one launch):

  thin_dense        1, 2, 4.  ~1e-4 points per cell: >= 90 % of the rows are sure-far at every k on
                    both sides of every pick_k bucket; queries 0.5 .. 100 cells outside the box
                    along every face, edge and corner direction, at 1e3, 1e6 and 1e12 m; bit
                    copies of cloud points (d2 == 0 found by the far pass); NaN / +-inf rows.
  thin_sparse       1, 3, 4.  The same on a brick table whose 0.4 m cells stand (asserted), with
                    queries between the clusters: hundreds of empty brick shells.
  mixed             8.  Half the rows sure-near, half sure-far, interleaved.
  tie_lattice_far   5, 2 / 3.  Runs of 8, 6, 2 + 8 exactly tied neighbours 8 cells (dense table)
                    and 64 cells (brick table) away, cut by k = 4, 6, 7, 9: the tied points sit in
                    different lanes' lists and coop_merge's (d2, j) order decides the row.
  duplicates_far    5.  200 bit-identical points in one cell, dealt over all lanes by flat_visit:
                    rows of k equal d2 that must hold the k smallest indices, ascending.
  mapped            6, 5.  NaN rows and a shuffled `indices` subset: ties rank by the position in
                    `indices`, the row holds caller indices.  ix.identity_mapping is asserted False.
  small_index_big_k 6.  40 points, k = 40 .. 200: every row deferred, entries [40, k) padding,
                    past the wave's 64 lanes for k > 64.
  many_far          7.  8,257 queries, all deferred: more than the far launch's 8,192 waves.
  layouts, no d2    6.  48-byte query strides (a (nq, 6) tensor's rows, an AoS48 cloud); NULL d2
                    with a guard buffer behind the indices.
  nearest_query     pcp_nearest_query over 300,001 queries (k_argmin_d2's grid-stride loop runs
                    twice, ~98 % of the 1-NN rows deferred): an exact tie between query 10 and
                    query 299,999 (the first wins), init_bound equal to the winning d2 (strict)
                    and an ulp above it, NaN rows, an all-NaN set.

Checked once against builds of knn.hip (the far pass is now knn_coop.hpp) with one change each (wrong rows only, nothing out of
bounds); the tests that failed, of 55:

  coop_merge comparing d2 alone              every k of tie_lattice_far on both tables, of
                                             duplicates_far and of mapped (20)
  the brick phase not skipping the cell-ring thin_dense from k = 2, thin_sparse and mixed from k = 8,
  window (yzin false: points visited twice)  tie_lattice_far and mapped from k = 4, every k of
                                             small_index_big_k, many_far, indices only, the
                                             layouts, the rerun after k = 65 (43; at k = 1 a
                                             point seen twice still gives the right row)
  k_knn_coop writing j without mapping[]     mapped at k = 1, 7, 9 (3)
  k_knn_coop's write-out as it was, one      small_index_big_k at k = 65, 100, 200 and indices
  entry per lane (`if (lane < k)`)           only at k = 100 (4): entries 64 .. k-1 of all 220
                                             rows still held the sentinel
"""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_grid_cases as gc
import oracle_ctypes as ora

pytestmark = pytest.mark.gpu

IDX_SENTINEL = 0x5A5A5A5A
D2_SENTINEL = -7.0
PCP_ERR_ARG, PCP_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)  # a copy: the cases are read-only


def _knn_raw(ctx, ix, qptr, qstride, nq, k, with_d2=True):
    """pcp_knn on sentinel-filled outputs: (return code, idx, d2 or None, guard), all on the
    host.  The indices and, behind them, a guard of nq * k sentinel doubles share one buffer;
    d2 is a buffer of its own, or NULL."""
    rows, cols = max(nq, 0), max(k, 1)
    words = (rows * cols + 1) // 2 * 2  # the guard stays 8-byte aligned
    buf = torch.empty(words + 2 * rows * cols + 2, dtype=torch.int32, device=ctx.device)
    buf[:words] = IDX_SENTINEL
    guard = buf[words:].view(torch.float64)
    guard.fill_(D2_SENTINEL)
    d2 = torch.full((rows, cols), D2_SENTINEL, dtype=torch.float64, device=ctx.device) if with_d2 else None
    rc = ctx.lib.pcp_knn(ctx.h, ix.h, qptr, qstride, nq, int(k), C.c_void_p(buf.data_ptr()),
                         C.c_void_p(d2.data_ptr()) if with_d2 else None)
    torch.cuda.synchronize(ctx.device)
    host = buf.cpu().numpy()
    return (rc, host[:rows * cols].reshape(rows, cols), d2.cpu().numpy() if with_d2 else None,
            host[words:].view(np.float64))


def _knn(ctx, ix, q, k, with_d2=True):
    qd = _dev(ctx, q)
    rc, idx, d2, guard = _knn_raw(ctx, ix, C.c_void_p(qd.data_ptr()), 24, len(q), k, with_d2)
    ctx.check(rc)
    assert (guard == D2_SENTINEL).all(), "pcp_knn wrote behind the index rows"
    return idx, d2


def _index(ctx, name):
    """The case's index with its geometry asserted: the cell size kept as given, and the dense
    table or the brick table as the case intends."""
    from pointcloudprocess_amd import ops
    t, _, cell, _, indices, ref = gc.case(name)
    ix = ops.GridIndex(ctx, _dev(ctx, t), cell_size=cell,
                       indices=None if indices is None else torch.from_numpy(np.array(indices)))
    cells, dense = int(ctx.lib.pcp_index_cells(ix.h)), gc.dense_cells(t, cell, indices)
    print(f"{name}: cell_size {cell} -> {ix.cell_size}, {ix.size} points, cells {cells}, dense product {dense}")
    assert ix.cell_size == cell
    if gc.CASES[name][1] == gc.BRICK:
        assert cells < dense, (cells, dense)
    else:
        assert cells == dense, (cells, dense)
    assert ix.size == int(np.isfinite(t if indices is None else t[indices]).all(1).sum())
    return ix


def _same(got, want, label):
    for name, g, w in (("indices", got[0], want[0]), ("d2", got[1], want[1])):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (label, name, g.shape, w.shape, g.dtype)
        if not np.array_equal(g, w):
            rows = np.flatnonzero((g != w).any(1))
            r = int(rows[0])
            c = int(np.flatnonzero(g[r] != w[r])[0])
            unwritten = int((g == (IDX_SENTINEL if name == "indices" else D2_SENTINEL)).sum())
            raise AssertionError(f"{label}: {name} differ in {len(rows)} rows, first rows {rows[:5].tolist()}; "
                                 f"row {r} column {c}: got {g[r, c]!r}, expected {w[r, c]!r}; "
                                 f"{unwritten} entries never written")


def _far_bounds(ctx, name, k, label):
    """pcp_knn_last_far of the call just made against the reference's classification."""
    from pointcloudprocess_amd import ops
    t, q, h, _, indices, ref = gc.case(name)
    n, far, near = gc.classify(t, q, ref[1], k, h, indices)
    got = ops.knn_last_far(ctx)
    print(f"{label}: deferred {got} of {n} finite rows (sure-far {far}, sure-near {near})")
    assert far <= got <= n - near, (label, far, got, n - near)
    return got


_trees = {}


def _oracle(name):
    if name not in _trees:
        t, _, _, _, indices, _ = gc.case(name)
        _trees[name] = ora.KdTree(t, indices=indices)
    return _trees[name]


@pytest.fixture(scope="module")
def indexes(ctx):
    """One index per case, built on first use and shared by the case's k values."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = _index(ctx, name)
        return built[name]
    yield get
    for ix in built.values():
        ix.close()


@pytest.mark.parametrize("name,k", gc.PARAMS, ids=[f"{n}-k{k}" for n, k in gc.PARAMS])
def test_knn_paths(ctx, indexes, name, k):
    t, q, _, _, indices, ref = gc.case(name)
    ix = indexes(name)
    assert ix.identity_mapping == (indices is None and bool(np.isfinite(t).all()))
    got = _knn(ctx, ix, q, k)
    deferred = _far_bounds(ctx, name, k, f"{name} k={k}")
    want = gc.prefix_k(ref, k)
    _same(got, want, f"{name} k={k} vs the reference")
    fin = np.isfinite(q).all(1)
    ei, ed = _oracle(name).knn(q, k)
    _same((got[0][fin], got[1][fin]), (ei[fin], ed[fin]), f"{name} k={k} vs the oracle")
    if name == "many_far":
        assert deferred > gc.H_WAVES
    if name == "small_index_big_k":  # nothing past the 40 points, on any row
        assert (got[0][:, gc.G_N:] == -1).all() and np.isposinf(got[1][:, gc.G_N:]).all()


@pytest.mark.parametrize("name,k", [("thin_dense", 8), ("thin_dense", 64), ("small_index_big_k", 40),
                                    ("small_index_big_k", 100)])
def test_indices_only(ctx, indexes, name, k):
    """out_d2 == NULL: the same indices, and the guard where a d2 row would follow is untouched
    (asserted in _knn)."""
    _, q, _, _, _, ref = gc.case(name)
    idx, d2 = _knn(ctx, indexes(name), q, k, with_d2=False)
    assert d2 is None
    _far_bounds(ctx, name, k, f"{name} k={k} indices only")
    _same((idx, None), gc.prefix_k(ref, k), f"{name} k={k} indices only")


def test_query_layouts(ctx, indexes):
    """Case A at k = 8 through 48-byte strides: rows of a (nq, 6) float64 tensor whose other
    three columns are NaN, and an AoS48 cloud."""
    from pointcloudprocess_amd import ops
    _, q, _, _, _, ref = gc.case("thin_dense")
    ix, want = indexes("thin_dense"), gc.prefix_k(ref, 8)
    wide = np.full((len(q), 6), np.nan)
    wide[:, :3] = q
    wd = _dev(ctx, wide)
    assert wd.stride(0) * wd.element_size() == 48
    cloud = ops.cloud_to_device(ora.make_cloud(q), ctx.device)
    for label, buf in (("(nq, 6) rows", wd), ("AoS48", cloud)):
        rc, idx, d2, guard = _knn_raw(ctx, ix, C.c_void_p(buf.data_ptr()), 48, len(q), 8)
        ctx.check(rc)
        _far_bounds(ctx, "thin_dense", 8, f"thin_dense k=8 {label}")
        assert (guard == D2_SENTINEL).all()
        _same((idx, d2), want, f"thin_dense k=8 {label}")


def test_unsupported_k_and_empty_calls(ctx, indexes):
    """k = 65 over 3,000 points: PCP_ERR_UNSUPPORTED, nothing written, nothing counted, and the
    context and the index still usable; nq == 0 is PCP_OK and k <= 0 or nq < 0 PCP_ERR_ARG, as
    pcp_knn's first lines say, with the counter at 0."""
    from pointcloudprocess_amd import ops
    _, q, _, _, _, ref = gc.case("thin_dense")
    ix = indexes("thin_dense")
    qd = _dev(ctx, q)
    qp = C.c_void_p(qd.data_ptr())
    _knn(ctx, ix, q, 8)
    assert ops.knn_last_far(ctx) > 0  # the counter has something to lose
    rc, idx, d2, guard = _knn_raw(ctx, ix, qp, 24, len(q), 65)
    assert rc == PCP_ERR_UNSUPPORTED
    assert (idx == IDX_SENTINEL).all() and (d2 == D2_SENTINEL).all() and (guard == D2_SENTINEL).all()
    assert ops.knn_last_far(ctx) == 0
    _same(_knn(ctx, ix, q, 64), gc.prefix_k(ref, 64), "thin_dense k=64 after the error")
    _far_bounds(ctx, "thin_dense", 64, "thin_dense k=64 after the error")
    for nq, k, want in ((0, 8, 0), (len(q), 0, PCP_ERR_ARG), (len(q), -3, PCP_ERR_ARG), (-1, 8, PCP_ERR_ARG)):
        _knn(ctx, ix, q, 8)
        assert ops.knn_last_far(ctx) > 0
        rc, idx, d2, guard = _knn_raw(ctx, ix, qp, 24, nq, k)
        assert rc == want, (nq, k, rc)
        assert (idx == IDX_SENTINEL).all() and (d2 == D2_SENTINEL).all() and (guard == D2_SENTINEL).all()
        assert ops.knn_last_far(ctx) == 0, (nq, k)


# ---------------------------------------------------------------- pcp_nearest_query
@pytest.fixture(scope="module")
def nearest(ctx):
    from pointcloudprocess_amd import ops
    t, q, d2, want = gc.nearest_query_case()
    ix = ops.GridIndex(ctx, _dev(ctx, t), cell_size=gc.A_CELL)
    assert ix.cell_size == gc.A_CELL
    yield ix, _dev(ctx, q), q, d2, want
    ix.close()


def test_nearest_query_tie_across_the_stride(ctx, nearest):
    """300,001 queries: queries 10 and 299,999 are exactly tied for the smallest 1-NN d2, in
    different trips of k_argmin_d2's loop; the sequential strict-'<' scan keeps the first."""
    from pointcloudprocess_amd import ops
    ix, qd, q, d2, want = nearest
    assert len(q) == 300_001 > 1024 * 256
    assert d2[10] == d2[299_999] == want and np.isnan(q[3]).all() and np.isnan(q[77]).all()
    assert gc.sequential_winner(d2, 9999.0) == (10, want)
    assert ops.nearest_query(ix, qd) == (10, want)
    far = ops.knn_last_far(ctx)  # pcp_nearest_query's pcp_knn counts too
    sure_far = int((np.sqrt(d2[np.isfinite(d2)]) / gc.A_CELL >= gc.SURE_FAR).sum())
    sure_near = int((np.sqrt(d2[np.isfinite(d2)]) / gc.A_CELL < gc.SURE_NEAR).sum())
    print(f"nearest_query: deferred {far} of {len(q) - 2} finite rows (sure-far {sure_far}, sure-near {sure_near})")
    assert sure_far > gc.H_WAVES and sure_far <= far <= len(q) - 2 - sure_near


def test_nearest_query_init_bound_is_strict(ctx, nearest):
    from pointcloudprocess_amd import ops
    ix, qd, q, d2, want = nearest
    assert gc.sequential_winner(d2, want) == (-1, want)
    assert ops.nearest_query(ix, qd, init_bound=want) == (-1, want)
    above = float(np.nextafter(want, np.inf))
    assert gc.sequential_winner(d2, above) == (10, want)
    assert ops.nearest_query(ix, qd, init_bound=above) == (10, want)


def test_nearest_query_nan_rows(ctx, nearest):
    """NaN rows among finite ones never win -- a set whose only finite row is its last -- and an
    all-NaN set has no winner."""
    from pointcloudprocess_amd import ops
    ix, qd, q, d2, want = nearest
    some = np.full((300, 3), np.nan)
    some[299] = q[10]
    assert ops.nearest_query(ix, _dev(ctx, some)) == gc.sequential_winner(gc.nearest_d2(gc.case("thin_dense")[0], some), 9999.0) == (299, want)
    none = np.full((300, 3), np.nan)
    assert ops.nearest_query(ix, _dev(ctx, none)) == (-1, 9999.0)
    assert ops.nearest_query(ix, _dev(ctx, none), init_bound=np.inf) == (-1, np.inf)
