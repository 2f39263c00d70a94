"""The CPU oracle's RPCA records (ora_rpca) pinned to an independent reference
(tests/rpca_ref.py).  GPU records are checked bit for bit against the oracle, which restates
the kernel's Jacobi, summation order and structure; this test is what keeps that pair from
misreading the contract together, and it proves that the caps of rpca_ref.compare hold for
the oracle alone on the inputs the GPU tests use.

Measured over all cases here: no disagreeing row (excused share 0, cap 0.5 %), angle at most
4.2e-8 rad (gate 2e-7), curvature 1.5e-8 (1e-7), distance 5.9e-8 relative (2^-23).
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import oracle_ctypes as ora
import rpca_ref


def _knn(xyz, k):
    idx, _ = ora.KdTree(xyz).knn(xyz, k)
    return idx


@pytest.fixture(scope="module")
def scene():
    xyz = rpca_ref.scene(1500, 11)
    return xyz, _knn(xyz, 20)


def test_draws_equal_the_oracles():
    lib = ora.load()
    js = [0, 2 ** 31 + 3]
    for seed in (0, 7, 2 ** 63 + 5):
        vec = rpca_ref.draws(seed, js, 201)
        for a, j in enumerate(js):
            for it in (0, 33, 200):
                for slot in range(3):
                    e = lib.ora_rpca_draw(seed, j, it, slot)
                    assert rpca_ref.draw(seed, j, it, slot) == e, (seed, j, it, slot)
                    assert int(vec[a, it, slot]) == e, (seed, j, it, slot)


def test_iteration_counts():
    got = [rpca_ref.iterations(*pe) for pe in ((0.99, 0.5), (0.9999, 0.5), (0.99, 0.7), (0.5, 0.5), (0.1, 0.5))]
    assert got == [34, 68, 168, 5, 0]
    for pe in ((1.0, 0.5), (0.99, 1.0)):
        with pytest.raises(ValueError):
            rpca_ref.iterations(*pe)


def test_point_plane_distance_is_the_float_contract():
    """A hand-computed value: the float32 products, not the exact ones, are summed."""
    F = np.array([[3000.1, 7000.2, 100.3]], np.float32)
    a, b, c, d = (np.array([v], np.float32) for v in (0.6, 0.0, 0.8, -1880.0))
    f1 = float(np.float32(a[0] * F[0, 0])) + 0.0 + float(np.float32(c[0] * F[0, 2])) + float(d[0])
    g = float(np.sqrt(np.float32(np.float32(a[0] * a[0]) + np.float32(c[0] * c[0]))))
    assert rpca_ref.point_plane_distance(F, a, b, c, d)[0] == np.float32(abs(f1) / g)


@pytest.mark.parametrize("pr,epi", [(0.99, 0.5), (0.9999, 0.5), (0.99, 0.7), (0.5, 0.5), (0.1, 0.5)])
def test_oracle_vs_reference_iteration_counts(scene, pr, epi):
    xyz, idx = scene
    e = ora.rpca(xyz, idx, pr=pr, epi=epi, seed=3)
    ref = rpca_ref.rpca_ref(xyz, idx, pr=pr, epi=epi, seed=3)
    m = rpca_ref.compare(e, ref, f"oracle pr={pr} epi={epi}", expect_gated=rpca_ref.iterations(pr, epi) > 0)
    if rpca_ref.iterations(pr, epi) == 0:
        assert m["default"] == len(xyz) and ref["default"].all()


@pytest.mark.parametrize("k", [6, 9, 13])
def test_oracle_vs_reference_narrow_k(scene, k):
    xyz, _ = scene
    idx = _knn(xyz, k)
    rpca_ref.compare(ora.rpca(xyz, idx, seed=5), rpca_ref.rpca_ref(xyz, idx, seed=5), f"oracle k={k}")


def test_oracle_vs_reference_mixed_n(scene):
    xyz, idx = scene
    rows, length = rpca_ref.mixed_rows(idx)
    assert np.bincount(length, minlength=21).min() >= 40
    assert (rpca_ref.leading_run(rows) == length).all()
    e = ora.rpca(xyz, rows, seed=9)
    rpca_ref.compare(e, rpca_ref.rpca_ref(xyz, rows, seed=9), "oracle mixed N")
    s = rpca_ref.check_small(e, xyz, rows, "oracle mixed N")
    # the cnt <= 3 outcome is reached both ways (the best plane passes through hf points
    # exactly, so the MAD is rounding noise)
    _, _, _, rdef = rpca_ref.record_fields(e)
    assert rdef[length == 5].any() and (~rdef[length == 4]).any(), s


@pytest.mark.parametrize("offset", [(300.0, -200.0, 40.0), (3000.0, 7000.0, 100.0), (5e5, 4e6, 100.0)])
def test_oracle_vs_reference_coordinates(scene, offset):
    xyz, idx = scene
    big = xyz * 20.0 + np.array(offset)
    rpca_ref.compare(ora.rpca(big, idx, seed=2), rpca_ref.rpca_ref(big, idx, seed=2), f"oracle offset {offset}")


def test_oracle_vs_reference_lattice_mad_zero():
    xyz = rpca_ref.lattice()
    idx = _knn(xyz, 20)
    e = ora.rpca(xyz, idx, seed=4)
    ref = rpca_ref.rpca_ref(xyz, idx, seed=4)
    rpca_ref.compare(e, ref, "oracle lattice")
    assert (e["normal_z"] == 1.0).any()
    tilted = (e["curvature"] != 1.0) & (e["normal_z"] < 0.999)
    assert tilted.any()  # MAD == 0 kept an outlier


def test_reference_rows_subset_and_holes(scene):
    """rows= selects points without changing their records (the draws are keyed by j), and N
    is the leading run: indices after a -1 do not count."""
    xyz, idx = scene
    full = rpca_ref.rpca_ref(xyz, idx, seed=1)
    rows = np.array([3, 700, 1499])
    part = rpca_ref.rpca_ref(xyz, idx, seed=1, rows=rows)
    for k in full:
        assert np.array_equal(part[k], full[k][rows], equal_nan=True), k
    holed = idx.copy()
    holed[:, 7] = -1
    cut = idx.copy()
    cut[:, 7:] = -1
    a, b = rpca_ref.rpca_ref(xyz, holed, seed=1), rpca_ref.rpca_ref(xyz, cut, seed=1)
    assert (a["N"] == 7).all()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_reference_is_robust_on_a_noisy_plane():
    """The noisy plane with 10 % outliers of test_oracle.py: the reference's normals are
    within 0.05 rad of +z on at least 95 % of the inlier rows."""
    rng = np.random.default_rng(5)
    n = 3000
    xyz = np.c_[rng.uniform(-1, 1, (n, 2)), rng.normal(0, 1e-3, n)]
    out_i = rng.choice(n, n // 10, replace=False)
    xyz[out_i, 2] += rng.uniform(0.05, 0.2, len(out_i))
    _, idx = cKDTree(xyz).query(xyz, k=20)
    ref = rpca_ref.rpca_ref(xyz, idx.astype(np.int32), seed=7)
    inl = np.setdiff1d(np.arange(n), out_i)
    ang = rpca_ref.plane_ref.angle(ref["normal"][inl], np.broadcast_to([0.0, 0.0, 1.0], (len(inl), 3)))
    share = float(((ang < 0.05) & ~ref["default"][inl]).mean())
    print(f"reference on the noisy plane: {share:.4f} of the inlier rows within 0.05 rad of +z")
    assert share >= 0.95
