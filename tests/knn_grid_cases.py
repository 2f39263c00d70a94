"""Input builders of the grid kNN path tests, shared by tests/test_knn_grid_ref.py (CPU) and
tests/test_gpu_knn_paths.py (GPU) so that both see identical arrays.

TEST INFRASTRUCTURE ONLY.  Fixed seeds, read-only arrays.  Every builder returns
(t, q, cell_size, ks[, indices]): the cloud, the queries, the cell size the index is built
with, the k values the case runs at and, for the mapped case, the `indices` subset in the
order the build receives it.  Coordinates are true float64 (an fp32 round trip changes more
than 90 % of them, asserted) unless the docstring says otherwise, so cell coordinates depend
on the low bits.

pcp_knn answers a query in its near pass (cell rings 0..3 of the query's cell) unless the
k-th neighbour may lie beyond them; then the query is deferred to the wave-per-query pass.
classify() says from the exhaustive reference alone which rows MUST be deferred and which
MUST NOT, whatever the rounding of the cell coordinates: with h the index's cell size,
kk = min(k, finite targets) and rho = sqrt(d2_ref[kk-1]) / h,
  sure-far   rho >= 4 (1 + 1e-6): the near pass returns only when (3 + dmin - mc)^2 h^2 exceeds
             the k-th d2, and dmin <= 0.5;
  sure-near  rho < 2.999: the rings hold every neighbour and the same test passes.
"""
import numpy as np

from knn_cases import _cube, _true_f64

KREF = 64  # columns of the cached exhaustive reference (pcp_knn's largest k after clamping)
SURE_FAR = 4.0 * (1.0 + 1e-6)
SURE_NEAR = 2.999


def classify(t, q, ref_d2, k, h, indices=None):
    """(finite query rows, sure-far rows, sure-near rows) of a case at k on cells of size h."""
    sel = t if indices is None else t[indices]
    kk = min(int(k), int(np.isfinite(sel).all(1).sum()))
    fin = np.isfinite(q).all(1)
    assert 0 < kk <= ref_d2.shape[1]
    rho = np.sqrt(ref_d2[fin, kk - 1]) / h
    return int(fin.sum()), int((rho >= SURE_FAR).sum()), int((rho < SURE_NEAR).sum())


def prefix_k(ref, k):
    """The (nq, k) rows of a case from its top-64: the first k columns, or for k > 64 (an index
    of fewer than 64 points: column 63 is padding on every row) those 64 and more padding."""
    idx, d2 = ref
    if k <= idx.shape[1]:
        return idx[:, :k], d2[:, :k]
    assert (idx[:, -1] == -1).all() and np.isinf(d2[:, -1]).all()
    oi = np.full((len(idx), k), -1, dtype=np.int32)
    od = np.full((len(idx), k), np.inf, dtype=np.float64)
    oi[:, :idx.shape[1]], od[:, :idx.shape[1]] = idx, d2
    return oi, od


def _outside(rng, mn, mx, h, cells):
    """One query per face, edge and corner direction of the box [mn, mx] and per entry of
    `cells`: that many cells beyond the box along the direction's axes, uniform inside it along
    the others."""
    out = []
    for c in cells:
        for d in np.ndindex(3, 3, 3):
            d = np.array(d) - 1
            if not d.any():
                continue
            p = rng.uniform(mn, mx)
            p = np.where(d > 0, mx + c * h, np.where(d < 0, mn - c * h, p))
            out.append(p)
    return np.array(out)


def _directions():
    """The 6 axis and 8 diagonal unit directions' sign patterns (14 rows)."""
    ax = [s * np.eye(3)[a] for a in range(3) for s in (1.0, -1.0)]
    di = [np.array([sx, sy, sz]) for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    return np.array(ax + di)


# ---------------------------------------------------------------- A. thin cloud, dense table
A_CELL = 0.125
A_KS = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64)  # both sides of every pick_k bucket


def _thin_cloud():
    return _cube(np.random.default_rng(5101), 3000, 20.0)


def thin_dense():
    """3,000 uniform points in +-20 m on 0.125 m cells (322^3 cells: a dense table), ~1e-4
    points per cell: the nearest neighbour is ~12 cells away.  Queries: 1,000 uniform in the box,
    100 bit copies of cloud points, 104 outside the box by 0.5, 2, 10 and 100 cells along each
    of the 26 face, edge and corner directions, 20 at 1e3 m and 4 at 1e6 m, 12 at 1e12 m (the
    cell coordinate saturates) along axes and diagonals, and 8 non-finite rows."""
    rng = np.random.default_rng(5102)
    t = _thin_cloud()
    mn, mx = t.min(0), t.max(0)
    dirs = _directions()
    jit = lambda n: rng.uniform(-1.0, 1.0, (n, 3))  # keeps the far rows true float64
    q = np.concatenate([
        _cube(rng, 1000, 20.0),
        t[rng.choice(len(t), 100, replace=False)],
        _outside(rng, mn, mx, A_CELL, (0.5, 2.0, 10.0, 100.0)),
        1e3 * dirs[np.arange(20) % 14] + jit(20),
        1e6 * dirs[[0, 3, 6, 13]] + jit(4),
        1e12 * dirs[[0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 12, 13]] + 1e3 * jit(12),
        _cube(rng, 8, 20.0)])
    bad = len(q) - 8
    q[bad + 0] = np.nan
    q[bad + 1, 0] = np.nan
    q[bad + 2, 1] = np.inf
    q[bad + 3, 2] = -np.inf
    q[bad + 4, 0] = np.inf
    q[bad + 5, 1] = -np.inf
    q[bad + 6, 2] = np.nan
    q[bad + 7] = [np.inf, -np.inf, np.nan]
    _true_f64(t, q)
    return t, q, A_CELL, A_KS


# ---------------------------------------------------------------- B. thin cloud, brick table
B_CELL = 0.4
B_HALF, B_SHIFT = 40.0, 300.0


def thin_sparse():
    """Two clusters of 1,500 uniform points 300 m apart on 0.4 m cells: 952^3 cells are too many
    for a dense table and 238^3 bricks are under the brick cap, so the cell size stands and the
    table is the brick table.  The clusters are +-40 m wide: at +-10 m the nearest neighbour of
    a query inside a cluster is ~2.7 cells away and k = 1 would mostly stay in the near pass.
    Queries: 200 inside each cluster, 40 on the line between them (hundreds of empty brick
    shells apart), 40 outside the box, 4 at 1e6 m."""
    rng = np.random.default_rng(5201)
    t = np.concatenate([_cube(rng, 1500, B_HALF), _cube(rng, 1500, B_HALF) + B_SHIFT])
    mn, mx = t.min(0), t.max(0)
    line = np.linspace(0.1, 0.9, 40)[:, None] * B_SHIFT + rng.uniform(-0.5, 0.5, (40, 3))
    out = _outside(rng, mn, mx, B_CELL, (0.5, 30.0))
    q = np.concatenate([_cube(rng, 200, B_HALF), _cube(rng, 200, B_HALF) + B_SHIFT, line,
                        out[rng.choice(len(out), 40, replace=False)],
                        1e6 * _directions()[[0, 5, 6, 13]] + rng.uniform(-1.0, 1.0, (4, 3))])
    _true_f64(t, q)
    return t, q, B_CELL, (1, 8, 20, 64)


# ---------------------------------------------------------------- C. near and far rows mixed
def mixed():
    """20,000 points in +-1 m plus 2,000 in +-20 m, shuffled, on 0.15 m cells; 400 queries in
    +-1 m and 400 in +-20 m, interleaved: near and far rows share waves of the near kernel and
    about half of them are deferred."""
    rng = np.random.default_rng(5301)
    t = np.concatenate([_cube(rng, 20_000, 1.0), _cube(rng, 2000, 20.0)])
    t = t[rng.permutation(len(t))]
    q = np.empty((800, 3))
    q[0::2] = _cube(rng, 400, 1.0)
    q[1::2] = _cube(rng, 400, 20.0)
    _true_f64(t, q)
    return t, q, 0.15, (1, 8, 32, 64)


# ---------------------------------------------------------------- D. exact ties, far pass
D_KS = (1, 4, 6, 7, 8, 9, 27)
D_GROUPS = (300, 200, 100)  # cube centres, lattice points, edge midpoints


def _lattice():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), -1)
    t = g.reshape(-1, 3).astype(np.float64)
    return t[np.random.default_rng(5401).permutation(len(t))]  # ties must break on index, not position


def tie_lattice_far(cell=0.125):
    """A 12 x 12 x 6 integer lattice of pitch 1 m, shuffled.  NOT true float64: every d2 is
    exact, so rows are runs of exact ties that only the index order decides.  Queries, all
    taken in index order from the points for which the run is complete (no lattice face cuts
    it): the first 300 points + 0.5 (8 neighbours at d2 = 0.75), 200 lattice points themselves
    (self, then 6 at d2 = 1), 100 edge midpoints (2 at 0.25, then 8 at 1.25).  On 0.125 m cells
    (dense; points on cell faces) the neighbours are 8 cells away, on 1/64 m cells (706 x 706 x
    322: a brick table) 64: every tie is merged from different lanes' lists."""
    t = _lattice()
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    inner = (x >= 1) & (x <= 10) & (y >= 1) & (y <= 10) & (z >= 1) & (z <= 4)
    centre = np.flatnonzero((x <= 10) & (y <= 10) & (z <= 4))[:D_GROUPS[0]]
    self_ = np.flatnonzero(inner)[:D_GROUPS[1]]
    edge = np.flatnonzero(inner & (x <= 9))[-D_GROUPS[2]:]
    q = np.concatenate([t[centre] + 0.5, t[self_], t[edge] + np.array([0.5, 0.0, 0.0])])
    assert len(q) == sum(D_GROUPS)
    return t, q, cell, D_KS


# ---------------------------------------------------------------- E. duplicates, far pass
E_SITES, E_COPIES = 10, 200
E_CELL = 0.125


def duplicates_far():
    """10 sites x 200 bit-identical copies plus 500 uniform points in +-20 m, shuffled, on
    0.125 m cells.  Queries: every site displaced by 5 cells along +x and along the diagonal
    (rows that start with a run of 200 equal d2, all from one cell that the far pass deals over
    every lane), then 100 uniform points."""
    rng = np.random.default_rng(5501)
    sites = _cube(rng, E_SITES, 19.0)
    t = np.concatenate([np.repeat(sites, E_COPIES, 0), _cube(rng, 500, 20.0)])
    t = t[rng.permutation(len(t))]
    s = 5 * E_CELL
    q = np.concatenate([sites + np.array([s, 0.0, 0.0]), sites + s, _cube(rng, 100, 20.0)])
    _true_f64(t, q)
    return t, q, E_CELL, (8, 64, 33)


# ---------------------------------------------------------------- F. non-identity mapping
def mapped():
    """Case D's cloud with every 7th row NaN, indexed through `indices` = every 2nd index in a
    SHUFFLED order, on 0.125 m cells.  Internal j is the position in `indices` once the
    non-finite rows are dropped, so ties rank by that position and the far pass's write-out
    has to map j back to the caller's index."""
    t, q, cell, _ = tie_lattice_far()
    t = t.copy()
    t[::7] = np.nan
    sub = np.arange(0, len(t), 2, dtype=np.int32)
    sub = sub[np.random.default_rng(5601).permutation(len(sub))]
    return t, q, cell, (1, 7, 9), sub


# ---------------------------------------------------------------- G. k beyond a small index
G_N = 40


def small_index_big_k():
    """40 points in +-10 m on 0.5 m cells, 200 uniform queries plus 20 outside the box: k >= 40
    clamps to the 40 points (the K = 64 kernels), the 40th neighbour is never within 4 cells,
    and entries [40, k) of every row are padding -- past the wave's 64 lanes when k > 64."""
    rng = np.random.default_rng(5701)
    t = _cube(rng, G_N, 10.0)
    out = _outside(rng, t.min(0), t.max(0), 0.5, (3.0,))
    q = np.concatenate([_cube(rng, 200, 10.0), out[rng.choice(len(out), 20, replace=False)]])
    _true_f64(t, q)
    return t, q, 0.5, (40, 41, 64, 65, 100, 200)


# ---------------------------------------------------------------- H. more far rows than waves
H_WAVES = 2048 * 4  # the far launch: kFarBlocks blocks of 4 waves


def many_far():
    """Case A's cloud with 8,192 + 65 uniform queries at k = 8: more deferred rows than the far
    launch has waves, so the wave-per-query kernel's own grid-stride loop runs twice."""
    q = _cube(np.random.default_rng(5801), H_WAVES + 65, 20.0)
    t = _thin_cloud()
    _true_f64(t, q)
    return t, q, A_CELL, (8,)


# ---------------------------------------------------------------- pcp_nearest_query
NQ_N = 1024 * 256 + 37_857  # 300,001: past k_argmin_d2's 1024 blocks x 256 threads
NQ_OFFSET = np.array([0.375, 0.0, 0.0])  # dyadic: the planted d2 is exactly 0.140625
NQ_CLEAR = 0.5  # no other query lies within this distance of a cloud point


def nearest_d2(t, q, chunk=128):
    """Exhaustive 1-NN d2 of every query (FLANN's summation order), +inf for non-finite rows."""
    out = np.full(len(q), np.inf)
    fin = np.isfinite(q).all(1)
    tx, ty, tz = (np.ascontiguousarray(t[:, a])[None, :] for a in range(3))
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        d = qq[:, 0:1] - tx
        r = d * d
        np.subtract(qq[:, 1:2], ty, out=d)
        np.multiply(d, d, out=d)
        r += d
        np.subtract(qq[:, 2:3], tz, out=d)
        np.multiply(d, d, out=d)
        r += d
        out[s:s + chunk] = r.min(1)
    out[~fin] = np.inf
    return out


_nq = None


def nearest_query_case():
    """(t, q, 1-NN d2 of every query, planted d2): case A's cloud and 300,001 queries uniform in
    +-20 m, redrawn while within 0.5 m of a cloud point; then query 299,999 and query 10 are
    moved to cloud points + (0.375, 0, 0) -- two different points for which the sum is exact
    and nothing else is nearer -- so both have the smallest d2 of all, exactly equal, and the
    earlier query wins.  Rows 3 and 77 are NaN."""
    global _nq
    if _nq is None:
        rng = np.random.default_rng(5901)
        t = _thin_cloud()
        q = _cube(rng, NQ_N, 20.0)
        d = nearest_d2(t, q)
        while True:
            near = np.flatnonzero(d < NQ_CLEAR ** 2)
            if len(near) == 0:
                break
            q[near] = _cube(rng, len(near), 20.0)
            d[near] = nearest_d2(t, q[near])
        want = float(NQ_OFFSET[0] ** 2)
        p = t + NQ_OFFSET
        exact = nearest_d2(t, p) == want  # the sum is exact and the point itself is the nearest
        a, b = np.flatnonzero(exact)[[0, -1]]
        assert a != b
        q[NQ_N - 2], q[10] = p[a], p[b]
        q[3] = q[77] = np.nan
        moved = np.array([3, 10, 77, NQ_N - 2])
        d[moved] = nearest_d2(t, q[moved])
        assert d[10] == d[NQ_N - 2] == want and (np.delete(d, [10, NQ_N - 2]) >= NQ_CLEAR ** 2).all()
        for arr in (t, q, d):
            arr.setflags(write=False)
        _nq = (t, q, d, want)
    return _nq


def sequential_winner(d2, init_bound):
    """main_blend.cpp:314-320: strict '<' from init_bound, so the first query wins ties."""
    best, mix = -1, init_bound
    for j in range(len(d2)):
        if d2[j] < mix:
            mix, best = d2[j], j
    return best, mix


# ---------------------------------------------------------------- registry
# name -> (builder, the table the build must choose at the case's cell size, the case's k values)
DENSE, BRICK = "dense", "brick"
CASES = {
    "thin_dense": (thin_dense, DENSE, A_KS),
    "thin_sparse": (thin_sparse, BRICK, (1, 8, 20, 64)),
    "mixed": (mixed, DENSE, (1, 8, 32, 64)),
    "tie_lattice_far": (tie_lattice_far, DENSE, D_KS),
    "tie_lattice_far_brick": (lambda: tie_lattice_far(cell=1.0 / 64), BRICK, D_KS),
    "duplicates_far": (duplicates_far, DENSE, (8, 64, 33)),
    "mapped": (mapped, DENSE, (1, 7, 9)),
    "small_index_big_k": (small_index_big_k, DENSE, (40, 41, 64, 65, 100, 200)),
    "many_far": (many_far, DENSE, (8,)),
}
PARAMS = [(n, k) for n, c in CASES.items() for k in c[2]]  # the (case, k) pairs, nothing built

_cache = {}


def case(name):
    """(t, q, cell_size, ks, indices or None, top-64 exhaustive reference) of a case: built once
    per process, read-only."""
    if name not in _cache:
        from knn_ref import ref_knn
        t, q, cell, ks, *rest = CASES[name][0]()
        indices = rest[0] if rest else None
        assert tuple(ks) == CASES[name][2]
        ref = ref_knn(t, q, KREF, order=indices)
        for a in (t, q, *ref) + (() if indices is None else (indices,)):
            a.setflags(write=False)
        _cache[name] = (t, q, cell, tuple(ks), indices, ref)
    return _cache[name]


def dense_cells(t, h, indices=None):
    """Cells of a dense table over the bounding box of the indexed finite points (grid.hip:
    floor(extent / h) + 2 per axis)."""
    p = t if indices is None else t[indices]
    p = p[np.isfinite(p).all(1)]
    return int(np.prod(np.floor((p.max(0) - p.min(0)) / h) + 2))
