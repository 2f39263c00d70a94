"""The oracle's KdTree.radius against the exhaustive reference of tests/radius_ref.py, bit for
bit, on every case and every (r, max_nn) that tests/test_gpu_radius_paths.py runs -- and the
proof that each case has the teeth its docstring in tests/radius_cases.py claims.  CPU only.
"""
import numpy as np
import pytest

import radius_cases as rc
from radius_ref import ref_radius, row


@pytest.mark.parametrize("name", list(rc.BUILDERS))
def test_oracle_matches_reference(name):
    c, ref = rc.case(name)
    assert len(c.runs) == len(set(c.runs))
    for r, max_nn in c.runs:
        eo, ei, ed = rc.oracle_rows(name, r, max_nn)
        ro, ri, rd = ref.rows(r, max_nn)
        so, si, sd = ref_radius(c.t, c.q, r, max_nn, c.indices)  # the reference's two forms agree
        assert np.array_equal(so, ro) and np.array_equal(si, ri) and np.array_equal(sd, rd), (r, max_nn)
        assert np.array_equal(eo, ro), (r, max_nn, np.flatnonzero(np.diff(eo) != np.diff(ro))[:5])
        assert np.array_equal(ei, ri), (r, max_nn)
        assert np.array_equal(ed, rd), (r, max_nn)
        assert ri.dtype == np.int32 and rd.dtype == np.float64 and ro.dtype == np.int64
    for g in c.grids:  # every radius of the case has a side on every grid, and it is the geometric one
        assert set(g.side) == {r for r, _ in c.runs}
        for r, side in g.side.items():
            assert side == (rc.FAR if r / g.h >= rc.CELL_RINGS else rc.NEAR), (g.h, r, side)


def test_reference_on_a_hand_case():
    """The reference itself, on rows small enough to write down."""
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0, 2], [np.nan, 0, 0], [-0.5, 0, 0]], dtype=np.float64)
    q = np.array([[0, 0, 0], [np.inf, 0, 0], [0, 0, 1.5]], dtype=np.float64)
    offs, idx, d2 = ref_radius(t, q, 1.0)
    assert offs.tolist() == [0, 3, 3, 4]
    assert idx.tolist() == [0, 3, 6, 4] and d2.tolist() == [0.0, 0.25, 0.25, 0.25]  # strict; ties by index
    assert ref_radius(t, q, 1.0, max_nn=2)[1].tolist() == [0, 3, 4]
    assert ref_radius(t, q, 1.0, max_nn=5)[0].tolist() == [0, 3, 3, 4]  # 6 finite targets: 5 still cuts
    assert ref_radius(t, q, 2.0, max_nn=6)[0].tolist() == [0, 5, 5, 11]  # == size: unlimited
    assert ref_radius(t, q, 2.0, max_nn=5)[0].tolist() == [0, 5, 5, 10]
    assert ref_radius(t, q, 2.0, max_nn=4)[0].tolist() == [0, 4, 4, 8]
    sub = ref_radius(t, q, 1.0, indices=np.array([1, 3, 4, 5], dtype=np.int32))
    assert sub[0].tolist() == [0, 1, 1, 2] and sub[1].tolist() == [3, 4]
    assert ref_radius(t, q, 0.0)[0].tolist() == [0, 0, 0, 0]
    assert ref_radius(t, q, 1e200)[0].tolist() == [0, 6, 6, 12]


def _tied_pairs(csr):
    """Adjacent entries of one row with equal d2."""
    offs, _, d2 = csr
    same = d2[1:] == d2[:-1]
    same[offs[1:-1][(offs[1:-1] > 0) & (offs[1:-1] < len(d2))] - 1] = False  # pairs across two rows
    return int(same.sum())


def _rows_changed_by_descending_ties(csr):
    offs, idx, d2 = csr
    changed = 0
    for i in range(len(offs) - 1):
        ri, rd = row(csr, i)
        changed += not np.array_equal(ri[np.lexsort((-ri, rd))], ri)
    return changed


@pytest.mark.parametrize("name", ["lattice", "lattice_mapped"])
def test_lattice_teeth(name):
    c, ref = rc.case(name)
    assert np.array_equal(c.t[np.isfinite(c.t).all(1)] * 8, np.round(c.t[np.isfinite(c.t).all(1)] * 8))  # dyadic
    floor = 1000 if name == "lattice" else 100  # the mapped variant keeps 2 points in 7
    for r in sorted({r for r, _ in c.runs}):
        csr = ref.rows(r)
        sphere, tied, changed = ref.on_sphere(r), _tied_pairs(csr), _rows_changed_by_descending_ties(csr)
        print(f"{name} r={r}: on the sphere {sphere}, tied neighbours {tied}, rows a descending tie-break changes {changed}")
        assert sphere >= floor, (r, sphere)      # a `<=` in place of `<` adds that many entries
        assert tied >= floor, (r, tied)
        assert changed > 0
    if name == "lattice":
        assert len(c.t) == 24 * 24 * 12 and len(c.q) == 400
    else:
        assert not np.isfinite(c.t[::7]).any() and (np.diff(c.indices) == 3).all()
        offs, idx, _ = ref.rows(1.25, 40)
        assert np.isin(idx, c.indices).all() and (np.diff(offs) == 40).mean() > 0.9  # nearly every row is cut


@pytest.mark.parametrize("name", ["ladder", "ladder_nan", "ladder_subset"])
def test_ladder_teeth(name):
    c, ref = rc.case(name)
    radii, ms, size = c.extra["radii"], c.extra["ms"], c.extra["size"]
    assert ref.size == size and 4900 <= len(c.t) <= 5300
    if name == "ladder":
        assert ms == rc.LADDER_M
    else:  # fewer points in the core: the ladder still reaches past kSortMax or stops short of it
        print(f"{name}: finite targets {size}, row lengths {ms}")
        assert ms == (rc.LADDER_M[:9] if name == "ladder_subset" else rc.LADDER_M)
    for m in ms:
        assert ref.counts(radii[m]).tolist() == [m], (m, radii[m])
    near, far = c.grids
    # 0.05 m cells: near for every radius inside the core; the whole-core row's radius is the
    # midpoint to the first background point (>= 0.2 m away), 4.9 cells
    assert all((near.side[radii[m]] == rc.NEAR) == (m < rc.LADDER_CORE) or name != "ladder" for m in ms)
    assert all(near.side[radii[m]] == rc.NEAR for m in ms if radii[m] < 0.0867)
    assert set(far.side.values()) == {rc.NEAR, rc.FAR}
    if name == "ladder":
        assert all((far.side[radii[m]] == rc.FAR) == (m >= rc.LADDER_FAR_FROM) for m in ms)
    # the max_nn sweep: m - 1 cuts, m and m + 1 do not; size - 1 is still a finite cap
    for m in rc.LADDER_SWEEP_M:
        if m in ms:
            assert [ref.counts(radii[m], mx).tolist()[0] for mx in (1, m - 1, m, m + 1)] == [1, m - 1, m, m]
    assert all((radii[ms[-1]], mx) in c.runs for mx in (size - 1, size, size + 1))
    # a mapped row in each branch of k_sort_rows: at the cap, bitonic, and (the NaN variant) > 1024
    if name == "ladder_nan":
        assert max(ms) > 1024 and not np.isfinite(c.t[::7]).any()
    if name != "ladder":
        idx = ref.rows(radii[ms[-1]])[1]
        keep = np.flatnonzero(np.isfinite(c.t).all(1)) if c.indices is None else c.indices
        assert not np.array_equal(keep[:len(idx)], np.arange(len(idx)))  # internal j != caller index


def test_duplicates_teeth():
    c, ref = rc.case("duplicates")
    assert len(c.t) == 3000 + rc.DUP_SITES * rc.DUP_COPIES
    full, cut100, cut200 = (ref.rows(rc.DUP_R, mx) for mx in (0, 100, 200))
    for s in range(rc.DUP_SITES):
        copies = np.flatnonzero((c.t == c.q[s]).all(1))
        assert len(copies) == rc.DUP_COPIES
        ri, rd = row(full, s)
        assert len(ri) > rc.DUP_COPIES and (rd[:200] == 0).all() and rd[200] > 0
        assert np.array_equal(ri[:200], copies)                 # 200 exact ties, ascending index
        assert np.array_equal(row(cut100, s)[0], copies[:100])  # the cut falls inside the tie
        assert np.array_equal(row(cut200, s)[0], copies)        # ... and exactly at its end
        ri, rd = row(full, rc.DUP_SITES + s)                    # the moved query: a tie at d2 > 0
        at = np.flatnonzero(np.isin(ri, copies))
        assert len(at) == 200 and (np.diff(at) == 1).all() and len(set(rd[at])) == 1 and rd[at[0]] > 0


def test_two_clusters_teeth():
    c, ref = rc.case("two_clusters")
    assert len(c.t) == 10_000
    lo, hi = c.t.min(0), c.t.max(0)
    assert np.prod(np.floor((hi - lo) / 0.02) + 2) > 1e11  # the dense table the forced cell size asks for
    cnt = {r: ref.counts(r) for r in rc.CLUSTER_R}
    inside, outside, between = slice(0, 80), slice(80, 120), slice(120, 130)
    assert (cnt[0.05][inside] > 0).all() and (cnt[0.3][inside] > 100).all()
    qo = c.q[outside]
    cheb = np.minimum(np.abs(qo).max(1), np.abs(qo - rc.CLUSTER_GAP).max(1))
    assert (cheb > 0.5).all() and (cheb <= 0.75).all()  # outside both boxes, by at most 0.25 m
    assert (cnt[0.3][outside] > 0).all() and (cnt[0.05][outside] == 0).any()
    for r in rc.CLUSTER_R:
        assert (cnt[r][between] == 0).all()
    assert cnt[0.5].max() > 1024  # the far pass over the sparse table also feeds the in-place sort


def test_odd_teeth():
    c, ref = rc.case("odd")
    bad = ~np.isfinite(c.q).all(1)
    assert bad.sum() == 5 and not bad[0] and not bad[-1] and np.isnan(c.q).any() and np.isposinf(c.q).any() \
        and np.isneginf(c.q).any()
    far_away = np.abs(np.where(np.isfinite(c.q), c.q, 0)).max(1) >= 1e12
    assert far_away.sum() == 3
    lo, hi = c.t.min(0), c.t.max(0)
    with np.errstate(invalid="ignore"):
        out = np.maximum(np.maximum(lo - c.q, c.q - hi).max(1), 0) / rc.ODD_CELL  # cells outside the box
    for cells in (0.5, 2.0, 10.0):
        assert (np.abs(out - cells) < 1e-9).sum() == 5
    c05, c10 = ref.counts(0.5), ref.counts(1.0)
    assert (c05[bad] == 0).all() and (c10[far_away] == 0).all()
    assert (c05[np.abs(out - 0.5) < 1e-9] > 0).all() and (c10[np.abs(out - 2.0) < 1e-9] > 0).all()
    assert (c10[np.abs(out - 10.0) < 1e-9] == 0).all()
    assert (ref.counts(0.0) == 0).all()
    assert ref.counts(0.5, 7).max() == 7
    e, eref = rc.case("odd_everything")
    fin = np.isfinite(e.q).all(1)
    assert (~fin).sum() >= 3 and (np.abs(out) >= 10 - 1e-9).any()
    assert (eref.counts(1e200)[fin] == len(e.t)).all() and (eref.counts(1e200)[~fin] == 0).all()
    a, _ = rc.case("odd_aos48")
    assert a.aos48 and np.array_equal(a.q, c.q, equal_nan=True)


def test_few_finite_teeth():
    c, ref = rc.case("none_finite")
    assert ref.size == 0 and all((ref.counts(r, mx) == 0).all() for r, mx in c.runs)
    c, ref = rc.case("one_finite")
    assert ref.size == 1
    assert ref.counts(0.25).tolist() == [1, 1, 0, 0, 0]  # the last query is exactly 0.25 away: strict
    assert ref.counts(0.75).tolist() == [1, 1, 0, 0, 1]
    assert ref.rows(0.75)[1].tolist() == [7, 7, 7]


@pytest.mark.parametrize("name,h", [("switch_lattice", 0.25), ("switch_uniform", 0.125)])
def test_switch_teeth(name, h):
    c, ref = rc.case(name)
    (lo, _), (at, _), (up, _) = c.runs
    assert lo < at < up and at == 3 * h and np.nextafter(lo, 1.0) == at and np.nextafter(at, 1.0) == up
    assert lo / h < 3 and lo * (1.0 / h) < 3 and at / h == 3 and up / h > 3  # exact: h is a power of two
    assert (ref.counts(lo) > 0).all()
    if name == "switch_lattice":
        assert ref.on_sphere(at) >= 1000
        assert ref.counts(up).sum() - ref.counts(at).sum() == ref.on_sphere(at)
        assert np.array_equal(ref.counts(lo), ref.counts(at))
        on_face = (c.q[:200] / h == np.round(c.q[:200] / h)).all()
        assert on_face  # dmin = 0: the only queries the near pass has to defer
