"""Input builders of the radius-search path tests, shared by tests/test_radius_ref.py (CPU) and
tests/test_gpu_radius_paths.py (GPU) so that both see identical arrays.

TEST INFRASTRUCTURE ONLY.  Fixed seeds.  A Case is one target cloud (optionally with an `indices`
subset), one query array, the (r, max_nn) searches run on it and the forced cell sizes it is
indexed at; every (cell size, r) names the side of the near/far dispatch it is meant to land on
(radius_needs_far: r / h >= 3 cells goes straight to the two-level brick search, anything below
runs the cell-ring pass and defers what that cannot certify).  The GPU test asserts that side
from the built index's own cell size, and the sparse flag from its cell count.
"""
from dataclasses import dataclass, field

import numpy as np

NEAR, FAR = "near", "far"
CELL_RINGS = 3  # the dispatch threshold in cells, as the tests understand it


@dataclass
class Grid:
    cell: float           # the forced cell_size
    side: dict            # r -> NEAR / FAR
    sparse: object = None  # True: the build must fall back to the brick table; None: not asserted
    built: object = None   # the cell size the build ends up with, where it is not `cell`

    @property
    def h(self):
        return self.cell if self.built is None else self.built


@dataclass
class Case:
    name: str
    t: np.ndarray
    q: np.ndarray
    runs: tuple                 # (r, max_nn) pairs
    grids: tuple
    indices: object = None      # ascending int32 subset of t's rows, or None
    aos48: bool = False         # hand the queries over as PointXYZRGBA records (48-byte stride)
    extra: dict = field(default_factory=dict)


def _cube(rng, n, half):
    return rng.uniform(-half, half, (n, 3))


def _with_nan(t):
    """Every 7th point a NaN row: the index compacts, so internal j != caller index."""
    t = t.copy()
    t[::7] = np.nan
    return t


def _every_third(t):
    return np.arange(0, len(t), 3, dtype=np.int32)


# ---------------------------------------------------------------- a. dyadic lattice
LATTICE_R = (0.25, 0.5, 0.75, 1.25)
LATTICE_PITCH = 0.25


def _lattice_cloud():
    rng = np.random.default_rng(4101)
    i, j, l = (a.ravel() for a in np.meshgrid(np.arange(24), np.arange(24), np.arange(12), indexing="ij"))
    t = LATTICE_PITCH * np.stack([i, j, l], 1).astype(np.float64)
    t = t[rng.permutation(len(t))]  # ties must break on index, not position
    on = t[rng.choice(len(t), 200, replace=False)]
    off = t[rng.choice(len(t), 200, replace=False)] + 0.125
    return t, np.concatenate([on, off])


def lattice():
    """24 x 24 x 12 points at pitch 0.25, shuffled; 200 queries on lattice points (every
    neighbour shell is a set of exact d2 ties, and the shell at r lies exactly on the sphere) and
    200 at cell centres.  Every coordinate, d2 and r*r is exact.  Cell 0.25 puts every point and
    the first 200 queries exactly on cell faces."""
    t, q = _lattice_cloud()
    return Case("lattice", t, q, tuple((r, 0) for r in LATTICE_R),
                (Grid(0.25, {0.25: NEAR, 0.5: NEAR, 0.75: FAR, 1.25: FAR}, sparse=False),
                 Grid(0.1, {0.25: NEAR, 0.5: FAR, 0.75: FAR, 1.25: FAR}, sparse=False)))


def lattice_mapped():
    """The lattice with every 7th point NaN and then an `indices` subset of every 3rd: tied rows
    whose internal j is neither the caller index nor a fixed multiple of it."""
    t, q = _lattice_cloud()
    t = _with_nan(t)
    return Case("lattice_mapped", t, q, ((0.5, 0), (0.75, 0), (1.25, 0), (1.25, 40)),
                (Grid(0.25, {0.5: NEAR, 0.75: FAR, 1.25: FAR}, sparse=False),),
                indices=_every_third(t))


# ---------------------------------------------------------------- b. row-length ladder
LADDER_M = (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1100)
LADDER_CORE = 1100
# rows the max_nn sweep cuts: a bitonic row of exactly one wave's width, and the shortest row of
# the in-place insertion sort (kSortMax + 1)
LADDER_SWEEP_M = (64, 1025)
# the two forced cell sizes: 0.05 m keeps every radius inside the core (< 0.0867 m) under 3
# cells -- only the whole-core row's radius, the midpoint to the first background point beyond
# the cleared 0.2 m, is ~0.24 m and goes far; 0.01 m (a sparse grid: the background spans 600
# cells per axis) sends every radius >= 0.03 m straight to the far pass, which on the full cloud
# is every row of LADDER_FAR_FROM entries or more
LADDER_FAR_FROM = 129


def _ladder_cloud():
    rng = np.random.default_rng(4201)
    core = _cube(rng, LADDER_CORE, 0.05)
    bg = _cube(rng, 4010, 3.0)
    bg = bg[np.abs(bg).max(1) > 0.2]
    t = np.concatenate([core, bg])
    return t[rng.permutation(len(t))]


def ladder_radii(t, indices=None):
    """The radius of each LADDER_M row of the query at the origin: the square root of the
    midpoint between the m-th and the (m+1)-th smallest d2 of the finite (subset) targets."""
    sel = np.arange(len(t)) if indices is None else np.asarray(indices)
    p = t[sel]
    p = p[np.isfinite(p).all(1)]
    d = p[:, 0] * p[:, 0]
    d = d + p[:, 1] * p[:, 1]
    d = d + p[:, 2] * p[:, 2]
    d.sort()
    return {m: float(np.sqrt(0.5 * (d[m - 1] + d[m]))) for m in LADDER_M if m < len(d)}


def _ladder(name, t, indices, ms):
    radii = ladder_radii(t, indices)
    assert set(ms) <= set(radii)
    size = int(np.isfinite(t if indices is None else t[indices]).all(1).sum())
    runs = [(radii[m], 0) for m in ms]
    for m in LADDER_SWEEP_M:
        if m in ms:
            runs += [(radii[m], mx) for mx in (1, m - 1, m, m + 1)]
    runs += [(radii[ms[-1]], mx) for mx in (size - 1, size, size + 1)]
    return Case(name, t, np.zeros((1, 3)), tuple(runs),
                tuple(Grid(h, {radii[m]: (FAR if radii[m] >= CELL_RINGS * h else NEAR) for m in ms}, sparse=sp)
                      for h, sp in ((0.05, False), (0.01, True))),
                indices=indices, extra={"radii": radii, "ms": tuple(ms), "size": size})


def ladder():
    """1100 points uniform in a +-0.05 box, ~4000 background points in +-3 with everything within
    Chebyshev 0.2 of the origin removed, shuffled; one query at the origin per radius, the radii
    chosen so that the row lengths are exactly LADDER_M: 1, 2, both sides of a wave (64), of the
    bitonic pad sizes 128 / 512 and of kSortMax (1024), and the whole core."""
    return _ladder("ladder", _ladder_cloud(), None, LADDER_M)


def ladder_nan():
    """The ladder cloud with every 7th point NaN (radii recomputed from the finite points): a
    mapped row in each branch of k_sort_rows."""
    t = _with_nan(_ladder_cloud())
    ms = tuple(m for m in LADDER_M if m in ladder_radii(t))
    return _ladder("ladder_nan", t, None, ms)


def ladder_subset():
    """The ladder cloud through an `indices` subset of every 3rd point (radii recomputed); only
    the rows that stay inside the core (a third of it is left: up to 129 entries)."""
    t = _ladder_cloud()
    idx = _every_third(t)
    ms = tuple(m for m, r in ladder_radii(t, idx).items() if r < 0.05)
    return _ladder("ladder_subset", t, idx, ms)


# ---------------------------------------------------------------- c. duplicates
DUP_SITES, DUP_COPIES, DUP_R = 40, 200, 0.3


def duplicates():
    """40 sites of 200 bit-identical points inside 3000 background points (+-2 m), shuffled.
    Queries: the sites (rows that start with 200 entries at d2 == 0) and the sites moved by up to
    1 mm (200 entries tied at a non-zero d2).  max_nn = 100 cuts inside the tie, 200 at its end."""
    rng = np.random.default_rng(4301)
    sites = _cube(rng, DUP_SITES, 1.8)
    t = np.concatenate([_cube(rng, 3000, 2.0), np.repeat(sites, DUP_COPIES, 0)])
    t = t[rng.permutation(len(t))]
    q = np.concatenate([sites, sites + _cube(rng, DUP_SITES, 1e-3)])
    return Case("duplicates", t, q, ((DUP_R, 0), (DUP_R, 100), (DUP_R, 200)),
                (Grid(0.15, {DUP_R: NEAR}, sparse=False), Grid(0.05, {DUP_R: FAR})))


# ---------------------------------------------------------------- d. two clusters (sparse grid)
CLUSTER_GAP = 100.0
CLUSTER_R = (0.05, 0.3, 0.5)


def two_clusters():
    """5000 points each in two +-0.5 m boxes 100 m apart on every axis, indexed with
    cell_size = 0.02: the dense table would need ~1e11 cells, so the build coarsens the cells
    until the brick table fits (0.16 m) and stays sparse (2.5e8 cells against the 2^26 cap).
    Queries: inside each cluster, up to 0.25 m outside each cluster's box, and around the midpoint
    (empty bricks on every side, empty rows).  r = 0.05 and 0.3 stay under 3 coarsened cells;
    r = 0.5 is 3.125 of them, the only way to run the brick search over a sparse table.
    No radius above 0.5: a larger one would walk the empty bricks between the clusters."""
    rng = np.random.default_rng(4401)
    a, b = _cube(rng, 5000, 0.5), _cube(rng, 5000, 0.5) + CLUSTER_GAP
    t = np.concatenate([a, b])
    t = t[rng.permutation(len(t))]
    outside = _cube(rng, 40, 0.5)
    outside[np.arange(40), rng.integers(0, 3, 40)] = rng.choice([-1.0, 1.0], 40) * rng.uniform(0.5, 0.75, 40)
    q = np.concatenate([a[:40] + 0.01, b[:40] - 0.01, outside[:20], outside[20:] + CLUSTER_GAP,
                        np.full((1, 3), 0.5 * CLUSTER_GAP), 0.5 * CLUSTER_GAP + _cube(rng, 9, 5.0)])
    assert max(CLUSTER_R) <= 0.5
    return Case("two_clusters", t, q, tuple((r, 0) for r in CLUSTER_R) + ((0.3, 50),),
                (Grid(0.02, {0.05: NEAR, 0.3: NEAR, 0.5: FAR}, sparse=True, built=0.16),))


# ---------------------------------------------------------------- e. odd queries
ODD_CELL = 0.2


def _odd_cloud():
    return _cube(np.random.default_rng(4501), 4000, 1.0)


def _odd_queries(t, far_away):
    rng = np.random.default_rng(4502)
    lo, hi = t.min(0), t.max(0)
    q = [_cube(rng, 30, 1.0)]
    for cells in (0.5, 2.0, 10.0):  # outside the bounding box by that many cells
        d = cells * ODD_CELL
        q.append(np.array([[hi[0] + d, 0.1, -0.2], [0.3, lo[1] - d, 0.4], [-0.5, 0.2, hi[2] + d],
                           [lo[0] - d, lo[1] - d, lo[2] - d], [hi[0] + d, hi[1] + d, lo[2] - d]]))
    q = np.concatenate(q)
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan],
                    [np.inf, -np.inf, 0.0]])
    q = np.insert(q, [3, 3, 17, 40, 45], bad, axis=0)  # non-finite rows among the finite ones
    if far_away:  # cell_f saturates at +-2^30 cells
        q = np.concatenate([q, [[1e12, 0.0, 0.0], [-1e12, 1e12, -1e12], [0.1, 0.2, 1e12]]])
    return q


def odd():
    """4000 points in +-1 m on 0.2 m cells (dense).  Queries: inside, 0.5 / 2 / 10 cells outside
    the box on a face, an edge and a corner, NaN / +inf / -inf rows among them, and three 1e12 m
    away.  r = 0.5 (2.5 cells), r = 1.0 (5 cells) and r = 0."""
    t = _odd_cloud()
    return Case("odd", t, _odd_queries(t, True), ((0.5, 0), (1.0, 0), (0.0, 0), (0.5, 7)),
                (Grid(ODD_CELL, {0.5: NEAR, 1.0: FAR, 0.0: NEAR}, sparse=False),))


def odd_aos48():
    """The same search with the queries handed over as 48-byte PointXYZRGBA records."""
    c = odd()
    return Case("odd_aos48", c.t, c.q, ((0.5, 0), (1.0, 0)),
                (Grid(ODD_CELL, {0.5: NEAR, 1.0: FAR}, sparse=False),), aos48=True)


def odd_everything():
    """r = 1e200: r*r is +inf and every finite query's row holds every point (the queries 1e12 m
    away are left out: their search is a walk over 2^28 empty shells, not a test).  Dense only."""
    t = _odd_cloud()
    q = _odd_queries(t, False)
    q = np.concatenate([q[:8], q[30:]])  # few rows: each is 4000 entries long
    return Case("odd_everything", t, q, ((1e200, 0), (1e200, 5)),
                (Grid(ODD_CELL, {1e200: FAR}, sparse=False),))


def _few_finite(name, finite):
    t = np.full((50, 3), np.nan)
    t[5, 1] = np.inf
    if finite:
        t[7] = [1.0, 2.0, 3.0]
    q = np.array([[1.0, 2.0, 3.0], [1.1, 2.0, 3.0], [0.0, 0.0, 0.0], [np.nan, 2.0, 3.0], [1.0, 2.0, 3.25]])
    return Case(name, t, q, ((0.25, 0), (0.75, 0), (0.25, 1), (0.0, 0)),
                (Grid(ODD_CELL, {0.25: NEAR, 0.75: FAR, 0.0: NEAR}),))


def none_finite():
    """50 points, none finite: an empty index, every row empty."""
    return _few_finite("none_finite", False)


def one_finite():
    """50 points, exactly one finite; a query on it, beside it, exactly 0.25 from it, far from it."""
    return _few_finite("one_finite", True)


# ---------------------------------------------------------------- f. the three-cell switch
def _switch_r(h):
    return (float(np.nextafter(3 * h, 0.0)), float(3 * h), float(np.nextafter(3 * h, np.inf)))


def switch_lattice():
    """The lattice on 0.25 m cells with r an ulp below, at and an ulp above 3 cells (both cell and
    r / cell are exact).  Below: the near pass runs, and the 200 queries on cell faces are the only
    ones a radius search ever defers (3 + dmin - margin cells <= r needs dmin ~ 0); the far pass
    then rebuilds their rows from scratch.  The deferral is conservative -- with r < 3 cells the
    rings already hold every hit -- so what the case pins is that the rebuilt rows are the same
    rows.  At and above: straight to the far pass; above, the thousands of pairs exactly on the
    0.75 sphere join."""
    t, q = _lattice_cloud()
    lo, at, up = _switch_r(0.25)
    return Case("switch_lattice", t, q, ((lo, 0), (at, 0), (up, 0)),
                (Grid(0.25, {lo: NEAR, at: FAR, up: FAR}, sparse=False),))


def switch_uniform():
    """The same three radii around 3 cells of 0.125 m on the uniform cloud of case e: queries in
    general position, which the near pass below the switch answers without deferring."""
    t = _odd_cloud()
    q = _cube(np.random.default_rng(4601), 100, 1.1)
    lo, at, up = _switch_r(0.125)
    return Case("switch_uniform", t, q, ((lo, 0), (at, 0), (up, 0)),
                (Grid(0.125, {lo: NEAR, at: FAR, up: FAR}, sparse=False),))


# ---------------------------------------------------------------- registry
BUILDERS = {f.__name__: f for f in (
    lattice, lattice_mapped, ladder, ladder_nan, ladder_subset, duplicates, two_clusters, odd, odd_aos48,
    odd_everything, none_finite, one_finite, switch_lattice, switch_uniform)}
# (case, grid number) of every GPU search test
GRID_PARAMS = [(n, g) for n, f in BUILDERS.items() for g in range(len(f().grids))]

_cache = {}
_oracle = {}


def case(name):
    """(Case, RadiusRef) of a case: built once per process, read-only."""
    if name not in _cache:
        from radius_ref import RadiusRef
        c = BUILDERS[name]()
        assert c.name == name
        ref = RadiusRef(c.t, c.q, c.indices)
        for a in (c.t, c.q, ref.idx, ref.d2):
            a.setflags(write=False)
        _cache[name] = (c, ref)
    return _cache[name]


def oracle_rows(name, r, max_nn):
    """CSR rows of the oracle's KdTree.radius, one call per query; once per process."""
    key = (name, r, max_nn)
    if key not in _oracle:
        import oracle_ctypes as ora
        c, _ = case(name)
        tkey = (name, "tree")
        if tkey not in _oracle:
            _oracle[tkey] = ora.KdTree(c.t, indices=c.indices)
        tree = _oracle[tkey]
        idx, d2, offs = [np.zeros(0, np.int32)], [np.zeros(0)], [0]
        for p in c.q:
            i, d = tree.radius(p, r, max_nn)
            idx.append(i.copy())
            d2.append(d.copy())
            offs.append(offs[-1] + len(i))
        _oracle[key] = (np.array(offs, dtype=np.int64), np.concatenate(idx), np.concatenate(d2))
    return _oracle[key]
