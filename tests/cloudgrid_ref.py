"""CloudGrid (cloud_grid.cpp) restated line by line in plain Python, and the hand-built edge
inputs that both the CPU tests (oracle vs this restatement, tests/test_cloudgrid.py) and the GPU
tests (libpcp vs both, tests/test_gpu_cloudgrid_edges.py) run.  Not a test module.

Every edge case carries its expected counts as literals worked out by hand from the reference's
source, so a misreading shared by the C and the Python restatement cannot hide."""
import numpy as np

import oracle_ctypes as ora

DUP_X = 0.04           # MAX_DIS_2POINT_X (cloud_grid.cpp:12)
DUP_2 = DUP_X * DUP_X  # MAX_DIS_2POINT (:13), a double
SUB = 0.045            # the GPU's hash sub-cell (cloudgrid.hip kSub)
Z_ALIAS = 184.32       # 4096 sub-cells: the period of the sub-cell key's 12-bit z field
INT_MIN = -2**31


def trunc_x86(v):
    """`int irow = x` as the x86-64 reference binary computes it (cvttsd2si): toward zero for
    |v| < 2^31, INT_MIN for NaN, +-inf and everything out of int's range."""
    v = float(v)
    if v != v or not (-2147483649.0 < v < 2147483648.0):
        return INT_MIN
    return int(v)


def occupied_subcells(points, sub=SUB):
    """Distinct floor(xyz / sub) triples: the hash slots one cell's kept points occupy on the GPU
    (ignoring the key's wrap-around).  Only for the pre-conditions of the path tests."""
    xyz = np.stack([points["x"], points["y"], points["z"]], axis=1)
    return len(np.unique(np.floor(xyz / sub).astype(np.int64), axis=0))


def _subcells(points, sub=SUB):
    xyz = np.stack([points["x"], points["y"], points["z"]], axis=1)
    return {tuple(t) for t in np.floor(xyz / sub).astype(np.int64)}


def brute_arrivals(old_kept, cloud, limit=1536):
    """What pcp_grid_last_dedupe must report for ONE cell holding `old_kept` (mutually no
    duplicates) when `cloud` arrives: (1 if the kept points come to occupy more than `limit`
    sub-cells else 0, the arrivals after that moment).  Kept / dropped comes from the oracle."""
    g = ora.Grid()
    g.add_cloud(old_kept)
    assert g.size == len(old_kept)
    occ = _subcells(old_kept) if len(old_kept) else set()
    tested = 0
    for i in range(len(cloud)):
        brute = len(occ) > limit
        tested += brute
        before = g.size
        g.add_cloud(cloud[i:i + 1])
        if g.size > before:
            occ |= _subcells(cloud[i:i + 1])
    return int(len(occ) > limit), tested


def sq_dist(a, b):
    """dis_two_point's double expression (cloud_grid.h:73-77) before its float return."""
    return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])


class PyGrid:
    """cloud_grid.cpp restated line by line in Python (small inputs only)."""

    def __init__(self):
        self.cells = {}

    def add(self, cloud):
        with np.errstate(invalid="ignore"):  # inf - inf is a quiet NaN, as in C
            self._add(cloud)

    def match(self, src, dis):
        with np.errstate(invalid="ignore"):
            return self._match(src, dis)

    def _add(self, cloud):
        for p in cloud:
            key = (trunc_x86(p["x"]), trunc_x86(p["y"]))
            if key not in self.cells:
                self.cells[key] = [p]
                continue
            keep = True
            for q in self.cells[key]:
                if abs(q["x"] - p["x"]) > 0.04 or abs(q["y"] - p["y"]) > 0.04 or abs(q["z"] - p["z"]) > 0.04:
                    continue
                d = np.float32((q["x"] - p["x"]) * (q["x"] - p["x"]) + (q["y"] - p["y"]) * (q["y"] - p["y"])
                               + (q["z"] - p["z"]) * (q["z"] - p["z"]))
                if float(d) < 0.04 * 0.04:
                    keep = False
                    break
            if keep:
                self.cells[key].append(p)

    @property
    def size(self):
        return sum(len(v) for v in self.cells.values())

    def points(self):
        """every kept point, cells ascending by (ix, iy) (the order libpcp and the oracle use)"""
        return [p for key in sorted(self.cells) for p in self.cells[key]]

    def box(self, i0, i1, j0, j1):
        return [p for i in range(i0, i1) for j in range(j0, j1) for p in self.cells.get((i, j), [])]

    def _match(self, src, dis):
        dis = float(np.float32(dis))  # float dis_threshold widened to double (cloud_grid.h:79)
        used, so, dst = {}, [], []
        for p in src:
            key = (trunc_x86(p["x"]), trunc_x86(p["y"]))
            cell = self.cells.get(key)
            if cell is None:
                continue
            # std::min(a, b) = (b < a) ? b : a, std::max(a, b) = (a < b) ? b : a; max_z starts at
            # numeric_limits<double>::min(), the smallest positive normal (:184-189)
            mn, mx = np.finfo(float).max, np.finfo(float).tiny
            for q in cell:
                z = q["z"]
                mn = z if z < mn else mn
                mx = z if mx < z else mx
            if mx - mn < 1.5:
                continue
            found = False
            for k, q in enumerate(cell):
                if abs(q["x"] - p["x"]) > dis or abs(q["y"] - p["y"]) > dis or abs(q["z"] - p["z"]) > dis:
                    continue
                found = True
                if k in used.setdefault(key, set()):
                    continue
                used[key].add(k)
                dst.append(q)
            if found:
                so.append(p)
        return so, dst


# ---------------------------------------------------------------------------- inputs
def mk(xyz, base=0):
    """records with distinct rgba / stamp_id, so a kept or emitted record is identifiable"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = len(xyz)
    return ora.make_cloud(xyz, rgba=np.arange(n, dtype=np.uint32) * 7 + 1000 + base,
                          stamp=np.arange(n, dtype=np.uint32) + base)


def column(n, seed, base=0):
    """n points in the single cell [5,6) x [7,8), z uniform in [0, 4)"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(5.0, 6.0, n), rng.uniform(7.0, 8.0, n), rng.uniform(0.0, 4.0, n)], axis=1)
    xyz[:, :2] = np.clip(xyz[:, :2], [5.0, 7.0], np.nextafter([6.0, 8.0], 0))
    return mk(xyz, base)


def echo_column(n, pairs, seed):
    """column(n), then `pairs` times a fresh point followed at once by a copy 1 cm beside it, then
    a copy 1 cm beside the very first arrival: whenever the fresh point is kept, its copy's only
    conflict is the newest kept point of the cell; the last row's is the oldest."""
    head = column(n, seed)
    rng = np.random.default_rng(seed + 1)
    fresh = np.stack([rng.uniform(5.0, 5.98, pairs), rng.uniform(7.0, 8.0, pairs), rng.uniform(0.0, 4.0, pairs)], axis=1)
    tail = np.repeat(fresh, 2, axis=0)
    tail[1::2, 0] += 0.01
    first = np.array([[head["x"][0] + (0.01 if head["x"][0] < 5.9 else -0.01), head["y"][0], head["z"][0]]])
    xyz = np.concatenate([np.stack([head["x"], head["y"], head["z"]], axis=1), tail, first])
    return mk(xyz)


def jittered(kept, n, seed, base, lo=(5.0, 7.0, 0.0), hi=(6.0, 8.0, 4.0)):
    """n points for the cell of `kept`: the first half copies of kept points moved by up to 0.03 per
    axis, the second half fresh, shuffled"""
    rng = np.random.default_rng(seed)
    h = n // 2
    pick = rng.integers(0, len(kept), h)
    a = np.stack([kept["x"][pick], kept["y"][pick], kept["z"][pick]], axis=1) + rng.uniform(-0.03, 0.03, (h, 3))
    b = rng.uniform(lo, hi, (n - h, 3))
    xyz = np.concatenate([a, b])[rng.permutation(n)]
    xyz = np.clip(xyz, lo, np.nextafter(hi, 0))
    return mk(xyz, base)


def find_float_rounded_dup():
    """A diagonal pair (origin, b) with every axis <= 0.04 whose double squared distance is above
    0.0016 while its float value is below: a duplicate only because dis_two_point returns float."""
    b = np.array([0.03, 0.02, np.sqrt(DUP_2 - 0.03 * 0.03 - 0.02 * 0.02)])
    o = np.zeros(3)
    while not sq_dist(o, b) > DUP_2:
        b[2] = np.nextafter(b[2], 1.0)
    return o, b


def dedupe_cases():
    """(name, xyz rows in arrival order, kept count): each its own grid.  One cell unless the name
    says otherwise."""
    cases = []
    # C6: the sub-cell key's z field wraps every 184.32 m; aliases are kept apart by the exact test
    cases.append(("z_alias", [(5.5, 7.5, 1.0), (5.5, 7.5, 1.0 + Z_ALIAS), (5.51, 7.5, 1.0),
                              (5.51, 7.5, 1.0 + Z_ALIAS)], 2))
    # five kept points in ONE 0.045 m sub-cell (each pair more than 0.04 apart on some axis), then a
    # duplicate of the first of them: the far end of the sub-cell's chain
    cases.append(("chain_of_five", [(0.001, 0.001, 0.001), (0.044, 0.001, 0.001), (0.001, 0.044, 0.001),
                                    (0.001, 0.001, 0.044), (0.044, 0.044, 0.044), (0.002, 0.002, 0.002)], 5))
    # C7, around the origin (cell 0 spans (-1, 1)) so that the differences are exact doubles
    up = float(np.nextafter(DUP_X, 1.0))
    for sgn, tag in ((1.0, "pos"), (-1.0, "neg")):
        for ax in range(3):
            e = np.zeros(3)
            e[ax] = sgn
            # per-axis difference == 0.04 passes the strict `>`; d2 = 0.0016 as float is below 0.0016
            cases.append((f"axis{ax}_{tag}_eq_0.04", [np.zeros(3), e * DUP_X], 1))
            cases.append((f"axis{ax}_{tag}_above_0.04", [np.zeros(3), e * up], 2))
        o, b = find_float_rounded_dup()
        cases.append((f"diag_{tag}_float_rounds_below", [o, sgn * b], 1))
        cases.append((f"diag_{tag}_clearly_above", [np.zeros(3), sgn * np.array([0.03, 0.03, 0.03])], 2))
        # a conflict across a sub-cell face: 5.49 = 122 * 0.045, 7.515 = 167 * 0.045, 0.99 = 22 * 0.045
        c = sgn * np.array([5.49, 7.515, 0.99])
        for ax in range(3):
            lo, hi = c - sgn * np.array([0.015, 0.015, 0.015]), c - sgn * np.array([0.015, 0.015, 0.015])
            lo[ax], hi[ax] = c[ax] - 0.015, c[ax] + 0.015
            cases.append((f"subcell_face{ax}_{tag}", [lo, hi], 1))
        cases.append((f"subcell_corner_{tag}", [c - 0.0085, c + 0.0085], 1))
        # 1 cm apart on either side of a 1 m cell face: two cells, both kept
        cases.append((f"cell_face_x_{tag}", [sgn * np.array([5.995, 7.5, 1.0]), sgn * np.array([6.005, 7.5, 1.0])], 2))
        cases.append((f"cell_face_y_{tag}", [sgn * np.array([5.5, 7.995, 1.0]), sgn * np.array([5.5, 8.005, 1.0])], 2))
    # truncation toward zero: (-1, 1) is one cell
    cases.append(("straddle_x0", [(-0.005, 0.5, 1.0), (0.005, 0.5, 1.0)], 1))
    cases.append(("straddle_y0", [(0.5, -0.005, 1.0), (0.5, 0.005, 1.0)], 1))
    cases.append(("straddle_xy0", [(-0.005, -0.005, 1.0), (0.005, 0.005, 1.0)], 1))
    return [(name, np.asarray(rows, dtype=np.float64), kept) for name, rows, kept in cases]


def z_alias_cloud(seed=5):
    """200 points around each of two heights 184.32 m apart (same sub-cell keys), interleaved"""
    rng = np.random.default_rng(seed)
    lo = rng.uniform([5.3, 7.3, 0.9], [5.6, 7.6, 1.2], (200, 3))
    hi = rng.uniform([5.3, 7.3, 0.9], [5.6, 7.6, 1.2], (200, 3)) + [0.0, 0.0, Z_ALIAS]
    xyz = np.empty((400, 3))
    xyz[0::2], xyz[1::2] = lo, hi
    return mk(xyz)


def _stack(k, z0, z1):
    """k grid points of cell (5, 7) rising from z0 to z1, no two of them duplicates (neighbours in z
    are 0.1 apart in x), all within 0.1 of x = 5.5, y = 7.5"""
    i = np.arange(k)
    return np.stack([5.4 + 0.1 * (i % 3), np.full(k, 7.5), np.linspace(z0, z1, k)], axis=1)


def lattice50():
    """50 grid points of cell (5, 7) in a 0.2 m box around (5.5, 7.5, 1.025), plus one far above
    that makes the cell tall"""
    g = np.array([(5.4 + 0.05 * i, 7.4 + 0.05 * j, 1.0 + 0.05 * k) for i in range(5) for j in range(5)
                  for k in range(2)])
    return np.concatenate([g, [(5.5, 7.5, 3.5)]])


def match_cases():
    """(name, grid xyz, source xyz, dis, sources out, dst): each its own grid, one add"""
    cases = []
    # max_z starts at DBL_MIN, so an all-negative cell spans to ~0: [-1.6, -0.2] counts as 1.6 m
    neg = _stack(40, -1.6, -0.2)
    cases.append(("all_negative_z_is_tall", neg, [(5.5, 7.5, -1.0)], 0.3, 1, 17))  # z_k in [-1.3, -0.7]: k = 9..25
    cases.append(("same_cell_plus_2_is_not", neg + [0, 0, 2.0], [(5.5, 7.5, 1.0)], 0.3, 0, 0))
    # `max_z - min_z < 1.5` is strict
    cases.append(("span_eq_1.5", [(5.5, 7.5, 0.25), (5.5, 7.5, 1.75)], [(5.5, 7.5, 0.25)], 0.3, 1, 1))
    cases.append(("span_below_1.5", [(5.5, 7.5, 0.25), (5.5, 7.5, float(np.nextafter(1.75, 0.0)))],
                  [(5.5, 7.5, 0.25)], 0.3, 0, 0))
    # |d| == dis, dis the float 0.3 widened: `>` is strict.  Around the origin: exact differences
    d = float(np.float32(0.3))
    tall0 = [(0.0, 0.0, 0.0), (0.0, 0.0, 2.0)]
    for ax in range(3):
        e = np.zeros(3)
        e[ax] = 1.0
        cases.append((f"axis{ax}_eq_dis", tall0, [e * d], 0.3, 1, 1))
        cases.append((f"axis{ax}_neg_eq_dis", tall0, [-e * d], 0.3, 1, 1))
        cases.append((f"axis{ax}_ulp_beyond_dis", tall0, [e * float(np.nextafter(d, 1.0))], 0.3, 0, 0))
    # the double 0.3 is below the float 0.3: a difference between them still matches
    cases.append(("between_double_and_float_dis", tall0, [(0.3 + 5e-9, 0.0, 0.0)], 0.3, 1, 1))
    # many sources, the same grid points: each emitted once, at its first source
    rng = np.random.default_rng(8)
    many = np.array([5.5, 7.5, 1.025]) + rng.uniform(-0.05, 0.05, (500, 3))
    cases.append(("500_sources_50_points", lattice50(), many, 0.3, 500, 50))
    # sources in absent cells, in a flat cell and out of reach, interleaved with matching ones
    flat = np.array([(8.2 + 0.1 * i, 7.5, 0.01 * i) for i in range(6)])
    grid = np.concatenate([lattice50(), flat])
    src = []
    for i in range(40):
        src.append((5.5 + 0.001 * i, 7.5, 1.0))        # matches
        src.append((20.5, 20.5, 1.0))                    # no such cell
        src.append((8.3, 7.5, 0.0))                      # cell (8, 7) spans 0.05 m
        src.append((5.5, 7.5, 2.0 + 0.01 * i))           # tall cell, nothing within 0.3
    cases.append(("interleaved_sources", grid, src, 0.3, 40, 50))
    # a NaN z neither poisons nor resets the z range ({0, NaN, 1, 2} spans 2) and passes the z test
    nan_z = [(5.4, 7.5, 0.0), (5.5, 7.5, np.nan), (5.6, 7.5, 1.0), (5.7, 7.5, 2.0)]
    cases.append(("nan_z_cell", nan_z, [(5.5, 7.5, 0.0)], 0.3, 1, 2))
    cases.append(("nan_z_first", [nan_z[1], nan_z[0], nan_z[3]], [(5.5, 7.5, 0.0)], 0.3, 1, 2))
    cases.append(("nan_z_last", [nan_z[0], nan_z[3], nan_z[1]], [(5.5, 7.5, 0.0)], 0.3, 1, 2))
    # a NaN-x source goes to cell (INT_MIN, 7), not to the populated, tall cell (0, 7)
    cell0 = np.array([(0.1 * (i % 8), 7.5, 0.3 * i) for i in range(12)])
    cases.append(("nan_x_source", cell0, [(np.nan, 7.5, 1.0)], 0.3, 0, 0))
    cases.append(("finite_x_source_same_cell", cell0, [(0.35, 7.5, 1.0)], 0.3, 1, 2))  # the points at z = 0.9, 1.2
    return [(name, np.asarray(g, dtype=np.float64), np.asarray(s, dtype=np.float64), dis, ns, nd)
            for name, g, s, dis, ns, nd in cases]


def nonfinite_cloud():
    """Ordinary points mixed with non-finite and out-of-range x / y.  Returns (cloud, kept,
    kept in cell (INT_MIN, 7)): of 18 rows two are duplicates; 9 go to cell (INT_MIN, 7), one of
    them a duplicate."""
    inf = np.inf
    rows = [
        (5.5, 7.5, 1.0), (np.nan, 7.5, 0.0), (5.51, 7.5, 1.0),       # the third a duplicate of the first
        (inf, 7.5, 0.5), (0.5, 7.5, 1.0), (-inf, 7.5, 1.0), (3e10, 7.5, 1.5),
        (5.5, np.nan, 1.0), (3e10 + 0.0078125, 7.5, 1.5),             # a duplicate at 3e10 (cell INT_MIN)
        (-3e10, 7.5, 2.0), (-0.5, 7.5, 3.0), (5.5, 7.5, np.nan),      # NaN z: an ordinary kept point
        (np.nan, 7.5, 0.0), (2147483648.0, 7.5, 2.5),                 # NaN again: never a duplicate; 2^31
        (-2147483648.5, 7.2, 0.0), (2147483647.5, 7.5, 0.0),          # the last two are in int's range
        (5.5, inf, 1.0), (np.nan, np.nan, np.nan),
    ]
    return mk(rows), 16, 8
