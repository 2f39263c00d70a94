"""The grid kNN path inputs (tests/knn_grid_cases.py) on the CPU: the oracle's kd-tree search
against the exhaustive reference (tests/knn_ref.py), bit for bit on every finite row, and each
case's teeth -- the property of the input that sends it down the path it was built for, taken
from the reference alone (knn_grid_cases.classify), so tests/test_gpu_knn_paths.py can hold
pcp_knn_last_far to it.
"""
import numpy as np
import pytest

import knn_cases as kc
import knn_grid_cases as gc
import oracle_ctypes as ora
from knn_ref import ref_knn

# (case, smallest share of the finite rows that must be sure-far, sure-near), at every k of the case
SHARES = {"thin_dense": (0.9, 0.0), "thin_sparse": (0.9, 0.0), "mixed": (0.4, 0.4),
          "small_index_big_k": (1.0, 0.0), "many_far": (0.99, 0.0)}


@pytest.mark.parametrize("name", list(gc.CASES))
def test_oracle_equals_exhaustive(name):
    """mapped: the oracle numbers its points by their position in `indices` (ora_kdtree_build, as
    convertCloudToArray kd_tree.h:928-997 does) and so does the reference through order=; were
    the two to differ, kd_tree.h decides which is right."""
    t, q, _, ks, indices, ref = gc.case(name)
    tree = ora.KdTree(t, indices=indices)
    rows = np.isfinite(q).all(1)
    assert (ref[0][~rows] == -1).all() and np.isinf(ref[1][~rows]).all()  # all padding
    for k in ks:
        ri, rd = gc.prefix_k(ref, k)
        ei, ed = tree.knn(q, k)
        assert np.array_equal(ei[rows], ri[rows]), f"{name} k={k}: {(ei[rows] != ri[rows]).any(1).sum()} rows differ"
        assert np.array_equal(ed[rows], rd[rows]), f"{name} k={k}: d2 differs"


@pytest.mark.parametrize("name", list(SHARES))
def test_shares(name):
    t, q, cell, ks, indices, ref = gc.case(name)
    far_min, near_min = SHARES[name]
    for k in ks:
        n, far, near = gc.classify(t, q, ref[1], k, cell, indices)
        print(f"{name} k={k}: {n} finite rows, sure-far {far / n:.3f}, sure-near {near / n:.3f}")
        assert far >= far_min * n and near >= near_min * n, (name, k, far / n, near / n)


def test_true_f64():
    for name in ("thin_dense", "thin_sparse", "mixed", "duplicates_far", "small_index_big_k", "many_far"):
        t, q = gc.case(name)[:2]
        assert kc.true_f64_share(t) > 0.9 and kc.true_f64_share(q) > 0.9, name


def test_table_choice_is_forced():
    """The dense product of every case's bounding box against the build's 2^26-cell dense cap
    and, for the brick cases, the brick product against its 2^24 cap (else the build coarsens
    the cells)."""
    for name, (_, table, _) in gc.CASES.items():
        t, _, cell, _, indices, _ = gc.case(name)
        cells = gc.dense_cells(t, cell, indices)
        assert (cells <= 2 ** 26) == (table == gc.DENSE), (name, cells)
        if table == gc.BRICK:
            p = t[np.isfinite(t).all(1)]
            bricks = np.prod((np.floor((p.max(0) - p.min(0)) / cell) + 2 + 3) // 4)
            assert bricks <= 2 ** 24, (name, bricks)


def test_thin_dense_queries():
    t, q, cell, ks, _, ref = gc.case("thin_dense")
    assert ks == (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64)
    fin = np.isfinite(q).all(1)
    assert (~fin).sum() == 8 and np.isnan(q[~fin]).any() and np.isposinf(q[~fin]).any() and np.isneginf(q[~fin]).any()
    mn, mx = t.min(0), t.max(0)
    cells_out = np.maximum(np.maximum(mn - q[fin], q[fin] - mx).max(1), 0.0) / cell
    assert (ref[1][fin, 0] == 0).sum() == 100  # the bit copies
    for lo, hi, n in ((0.49, 0.51, 26), (1.99, 2.01, 26), (9.99, 10.01, 26), (99.9, 100.1, 26)):
        assert ((cells_out > lo) & (cells_out < hi)).sum() == n, (lo, n)
    far = np.abs(q[fin]).max(1)
    assert ((far > 5e5) & (far < 2e6)).sum() == 4 and (far > 5e11).sum() == 12  # 16 walk every shell
    assert ((far > 500) & (far < 2e3)).sum() == 20
    assert ((q[fin] - mn) / cell > 2.0 ** 30).any() and ((q[fin] - mn) / cell < -(2.0 ** 30)).any()  # saturates


def test_tie_lattice_teeth():
    """k = 4 and 6 cut a run of exact ties in at least 90 % of the rows (here: all), k = 7 in
    every row of the cube centres and the edge midpoints -- a lattice point's own run, itself
    and 6 at d2 = 1, ends at 7 -- and on every such row the reference under the reversed index
    order, mapped back, differs: a merge that compares d2 alone cannot pass."""
    for name in ("tie_lattice_far", "tie_lattice_far_brick"):
        t, q, _, ks, _, ref = gc.case(name)
        assert ks == (1, 4, 6, 7, 8, 9, 27)
        rev = ref_knn(t, q, gc.KREF, order=np.arange(len(t))[::-1])
        assert np.array_equal(rev[1], ref[1])
        g0, g1, g2 = np.split(np.arange(len(q)), np.cumsum(gc.D_GROUPS)[:2])
        assert (ref[1][g0, :8] == 0.75).all() and (ref[1][g0, 8] > 0.75).all()
        assert (ref[1][g1, 0] == 0).all() and (ref[1][g1, 1:7] == 1).all() and (ref[1][g1, 7] == 2).all()
        assert (ref[1][g2, :2] == 0.25).all() and (ref[1][g2, 2:10] == 1.25).all()
        for k in (4, 6, 7):
            tied = ref[1][:, k - 1] == ref[1][:, k]
            rows = np.arange(len(q)) if k != 7 else np.concatenate([g0, g2])
            print(f"{name} k={k}: rows tied across the cut {tied.mean():.3f}")
            assert tied[rows].mean() >= 0.9, (k, tied[rows].mean())
            assert (rev[0][tied, :k] != ref[0][tied, :k]).any(1).all(), k


def test_duplicates_teeth():
    """Every site query's row starts with a run of equal d2 longer than k, all copies of one
    site, and holds the k smallest of that site's 200 indices in ascending order."""
    t, q, _, ks, _, ref = gc.case("duplicates_far")
    assert ks == (8, 64, 33)
    seen = set()
    for r in range(2 * gc.E_SITES):
        same = np.flatnonzero((t == t[ref[0][r, 0]]).all(1))
        assert len(same) == gc.E_COPIES, r
        seen.add(int(same[0]))
        for k in ks:
            idx, d2 = gc.prefix_k(ref, k)
            assert d2[r, 0] == d2[r, k - 1] and np.array_equal(idx[r], same[:k]), (r, k)
    assert len(seen) == gc.E_SITES


def test_mapped_teeth():
    t, q, _, ks, sub, ref = gc.case("mapped")
    assert ks == (1, 7, 9)
    kept = sub[np.isfinite(t[sub]).all(1)]
    assert len(kept) < len(sub) and not np.array_equal(sub, np.sort(sub))  # rows dropped, order shuffled
    assert np.isin(ref[0][ref[0] >= 0], kept).all()
    # ranking ties by caller index instead of the position in `indices` gives other rows
    by_index = ref_knn(t, q, gc.KREF, order=np.sort(sub))
    assert np.array_equal(by_index[1], ref[1])
    for k in (7, 9):
        assert (by_index[0][:, :k] != ref[0][:, :k]).any(1).mean() > 0.5, k


def test_small_index_padding():
    t, q, _, ks, _, ref = gc.case("small_index_big_k")
    assert ks == (40, 41, 64, 65, 100, 200) and len(t) == gc.G_N
    for k in ks:
        idx, d2 = gc.prefix_k(ref, k)
        assert idx.shape == (len(q), k) and (idx[:, :gc.G_N] >= 0).all()
        assert (idx[:, gc.G_N:] == -1).all() and np.isinf(d2[:, gc.G_N:]).all()


def test_ref_order_default():
    """order=None is ascending original index; an order with non-finite rows drops them."""
    t, q = gc.case("mapped")[:2]
    a = ref_knn(t, q[:50], 9)
    b = ref_knn(t, q[:50], 9, order=np.arange(len(t)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.isfinite(t[a[0][a[0] >= 0]]).all()
