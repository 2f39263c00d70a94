"""GPU parity of the fp64 neighbour queries (MI355X) against the oracle.

K3 nearestKSearch / K4 radiusSearch (kd_tree.h:814-845, 863-903): indices AND d2 are
compared BIT-EXACT (FLANN L2_Simple<double>, ties by internal index), including the
reference KAT (tests/golden/kat_kd_tree.json, main_test.cpp:156-188).
F1 per-point normals (calculate_feature.cpp:119-206): same neighbourhoods, same fp64
arithmetic order -> compared within 1e-6 (the float outputs are expected bit-identical;
the eigen solver is the build's Jacobi, OpenCV's sign/order is "parity unpinned").
K6 kd_tree_lod (kd_tree_lod/kd_tree.cpp:29-117): indices and d2 bit-exact.
"""
import json
import os

import numpy as np
import pytest
import torch

import oracle_ctypes as ora

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _cloud(n, seed, half=10.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-half, half, (n, 3)).astype(np.float32)).astype(np.float64)


def test_kat_kd_tree(ctx):
    from pointcloudprocess_amd import ops
    g = json.load(open(os.path.join(GOLDEN, "kat_kd_tree.json")))
    xyz = np.array(g["cloud_xyz"], dtype=np.float64)
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    idx, d2 = ops.knn(ix, _dev(ctx, np.array(g["query"], dtype=np.float64).reshape(1, 3)), g["k"])
    assert idx.cpu().numpy()[0].tolist() == g["expected_indices"]
    assert d2.cpu().numpy()[0].tolist() == g["expected_sqr_distances"]


@pytest.mark.parametrize("k", [1, 3, 8, 20, 32, 50])
def test_knn_bit_exact(ctx, k):
    from pointcloudprocess_amd import ops
    xyz = _cloud(100_000, 7)
    rng = np.random.default_rng(8)
    q = np.concatenate([_cloud(15_000, 9, half=11.0), xyz[rng.integers(0, len(xyz), 5000)]])
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    gi, gd = ops.knn(ix, _dev(ctx, q), k)
    ei, ed = ora.KdTree(xyz).knn(q, k)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    assert np.array_equal(gi, ei), f"{(gi != ei).any(1).sum()} rows differ"
    assert np.array_equal(gd, ed)


@pytest.mark.parametrize("cell", [0.0, 0.05, 2.0])
def test_knn_cell_sizes_and_surface(ctx, cell):
    """Street-scene surfaces (facades/poles) and forced cell sizes (tiny and huge)."""
    from pointcloudprocess_amd import ops, synth
    xyz = synth.street_scene(80_000, 21, extent=(60.0, 60.0)).double().numpy()
    q = xyz[::7] + 0.01
    ix = ops.GridIndex(ctx, _dev(ctx, xyz), cell_size=cell)
    gi, gd = ops.knn(ix, _dev(ctx, q), 16)
    ei, ed = ora.KdTree(xyz).knn(q, 16)
    assert np.array_equal(gi.cpu().numpy(), ei)
    assert np.array_equal(gd.cpu().numpy(), ed)


def test_knn_ties_lattice(ctx):
    from pointcloudprocess_amd import ops
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), -1)
    xyz = g.reshape(-1, 3).astype(np.float64)
    rng = np.random.default_rng(3)
    xyz = xyz[rng.permutation(len(xyz))]          # ties must break on index, not position
    q = xyz[:300] + 0.5
    ix = ops.GridIndex(ctx, _dev(ctx, xyz), cell_size=1.0)
    for k in (1, 8, 27):
        gi, gd = ops.knn(ix, _dev(ctx, q), k)
        ei, ed = ora.KdTree(xyz).knn(q, k)
        assert np.array_equal(gi.cpu().numpy(), ei)
        assert np.array_equal(gd.cpu().numpy(), ed)


def test_knn_nonfinite_and_indices(ctx):
    from pointcloudprocess_amd import ops
    xyz = _cloud(20_000, 11)
    xyz[::97] = np.nan                               # dropped by convertCloudToArray
    xyz[5::101, 1] = np.inf
    q = _cloud(3000, 12)
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    t = ora.KdTree(xyz)
    assert ix.size == t.size and not ix.identity_mapping
    gi, gd = ops.knn(ix, _dev(ctx, q), 10)
    ei, ed = t.knn(q, 10)
    assert np.array_equal(gi.cpu().numpy(), ei) and np.array_equal(gd.cpu().numpy(), ed)
    sub = np.arange(0, 20_000, 3, dtype=np.int32)
    ix2 = ops.GridIndex(ctx, _dev(ctx, xyz), indices=torch.from_numpy(sub))
    t2 = ora.KdTree(xyz, indices=sub)
    assert ix2.size == t2.size
    gi, gd = ops.knn(ix2, _dev(ctx, q), 10)
    ei, ed = t2.knn(q, 10)
    assert np.array_equal(gi.cpu().numpy(), ei) and np.array_equal(gd.cpu().numpy(), ed)


@pytest.mark.parametrize("finite", [0, 1])
def test_knn_all_or_all_but_one_nonfinite(ctx, finite):
    """The build's bbox + non-finite pass with no finite point (an empty index) or exactly one:
    rows padded with -1 / inf like the oracle's."""
    from pointcloudprocess_amd import ops
    xyz = np.full((50, 3), np.nan)
    if finite:
        xyz[7] = [1.0, 2.0, 3.0]
    q = np.zeros((2, 3))
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    t = ora.KdTree(xyz)
    assert ix.size == t.size == finite
    gi, gd = ops.knn(ix, _dev(ctx, q), 4)
    ei, ed = t.knn(q, 4)
    assert np.array_equal(gi.cpu().numpy(), ei) and np.array_equal(gd.cpu().numpy(), ed)


def test_knn_aos48_and_small(ctx):
    from pointcloudprocess_amd import ops
    xyz = _cloud(5, 13)
    cloud = ora.make_cloud(xyz)
    ix = ops.GridIndex(ctx, ops.cloud_to_device(cloud, ctx.device))
    q = _cloud(4, 14)
    gi, gd = ops.knn(ix, _dev(ctx, q), 8)           # k > size: clamped, padded with -1/inf
    ei, ed = ora.KdTree(xyz).knn(q, 8)
    assert np.array_equal(gi.cpu().numpy(), ei)
    assert np.array_equal(gd.cpu().numpy(), ed)
    assert (gi.cpu().numpy()[:, 5:] == -1).all()


def test_knn_bucket_edges(ctx):
    """Every k at which pcp_knn changes its compile-time list size (1, 4, 8, 16, 32, 64), and the
    k just above each: the list that serves k must hold at least k entries.  More than 64 points,
    so k = 65 is not clamped and is PCP_ERR_UNSUPPORTED."""
    import knn_ref
    from pointcloudprocess_amd import _lib, ops
    xyz = _cloud(300, 101)
    q = _cloud(64, 102)
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    ref = knn_ref.ref_knn(xyz, q, 64)
    for k in (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64):
        gi, gd = ops.knn(ix, _dev(ctx, q), k)
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        ei, ed = ref[0][:, :k], ref[1][:, :k]  # (d2, index) is a total order: a prefix of the longer row
        assert np.array_equal(gi, ei), f"k={k}: {(gi != ei).any(1).sum()} rows differ"
        assert np.array_equal(gd, ed), f"k={k}"
    with pytest.raises(_lib.PcpError) as err:
        ops.knn(ix, _dev(ctx, q), 65)
    assert err.value.code == -5  # PCP_ERR_UNSUPPORTED


def test_knn_sparse_grid(ctx):
    """Two clusters 5 km apart: the bounding grid is too large for a dense table."""
    from pointcloudprocess_amd import ops
    a = _cloud(20_000, 15, half=5.0)
    b = _cloud(20_000, 16, half=5.0) + 5000.0
    xyz = np.concatenate([a, b])
    q = np.concatenate([a[:2000] + 0.05, b[:2000] - 0.05])
    ix = ops.GridIndex(ctx, _dev(ctx, xyz), cell_size=0.02)
    gi, gd = ops.knn(ix, _dev(ctx, q), 8)
    ei, ed = ora.KdTree(xyz).knn(q, 8)
    assert np.array_equal(gi.cpu().numpy(), ei) and np.array_equal(gd.cpu().numpy(), ed)


@pytest.mark.parametrize("r,max_nn", [(0.3, 0), (0.6, 0), (0.6, 10), (0.0, 0)])
def test_radius_bit_exact(ctx, r, max_nn):
    from pointcloudprocess_amd import ops
    xyz = _cloud(60_000, 17, half=6.0)
    q = np.concatenate([_cloud(2000, 18, half=6.5), xyz[:500]])
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    offs, gi, gd = ops.radius(ix, _dev(ctx, q), r, max_nn)
    offs, gi, gd = offs.cpu().numpy(), gi.cpu().numpy(), gd.cpu().numpy()
    t = ora.KdTree(xyz)
    for i in range(len(q)):
        ei, ed = t.radius(q[i], r, max_nn)
        s, e = offs[i], offs[i + 1]
        assert np.array_equal(gi[s:e], ei), f"query {i}"
        assert np.array_equal(gd[s:e], ed), f"query {i}"


def test_radius_boundary_strict(ctx):
    """Points exactly at distance r are excluded (d2 < r*r, FLANN RadiusResultSet)."""
    from pointcloudprocess_amd import ops
    xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0, 2]], dtype=np.float64)
    q = np.zeros((1, 3))
    ix = ops.GridIndex(ctx, _dev(ctx, xyz), cell_size=0.3)
    offs, gi, gd = ops.radius(ix, _dev(ctx, q), 1.0)
    assert gi.cpu().numpy().tolist() == [0, 3]
    ei, _ = ora.KdTree(xyz).radius(q[0], 1.0)
    assert ei.tolist() == [0, 3]


@pytest.mark.parametrize("k", [8, 20, 32])
def test_normals_vs_oracle(ctx, k):
    from pointcloudprocess_amd import ops, synth
    xyz = synth.street_scene(60_000, 31, extent=(50.0, 50.0)).double().numpy()
    xyz[::501] = np.nan
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    g = ops.normals_knn(ix, k).cpu().numpy()
    e = ora.normals_knn(xyz, k)
    ev = np.stack([e[f] for f in ("normal_x", "normal_y", "normal_z", "min_value", "curvature", "distance")], 1)
    diff = np.abs(g - ev)
    exact = (g == ev).all(1).mean()
    print(f"k={k}: bit-identical rows {exact:.6f}, max |diff| {diff.max():.3e}")
    assert np.all(diff <= 1e-6 * np.maximum(1.0, np.abs(ev)))


def test_normals_tiny_cloud(ctx):
    from pointcloudprocess_amd import ops
    xyz = _cloud(3, 41)
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    g = ops.normals_knn(ix, 20).cpu().numpy()
    assert (g[:, :4] == 0).all() and (g[:, 4] == 1).all()  # N <= 3 guard


@pytest.mark.parametrize("offset", [(1234.3, -845.7, 12.1), (1.0e5, 2.0e5, 10.0)])
def test_knn_lod(ctx, offset):
    """offset 1e3: every neighbour is re-found (dis2 <= FLT_EPSILON); offset 1e5: the float
    round trip loses more than sqrt(FLT_EPSILON), so the index is -1 and d2 is the
    residual to the last cloud point (kd_tree.cpp:100 quirk)."""
    from pointcloudprocess_amd import ops
    rng = np.random.default_rng(51)
    off = np.array(offset)
    xyz = rng.uniform(0, 30, (20_000, 3)) + off
    xyz = xyz.astype(np.float32).astype(np.float64)
    cloud = ora.make_cloud(xyz)
    qx = np.concatenate([xyz[:40] + 0.003, rng.uniform(0, 30, (40, 3)) + off])
    qc = ora.make_cloud(qx)
    k = 6
    gi, gd = ops.knn_lod(ctx, ops.cloud_to_device(cloud, ctx.device), ops.cloud_to_device(qc, ctx.device), k)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    for i in range(len(qc)):
        ei, ed = ora.knn_lod(cloud, qc[i:i + 1], k)
        assert np.array_equal(gi[i], ei), f"query {i}"
        assert np.array_equal(gd[i], ed), f"query {i}"


def test_knn_lod_bucket_edges(ctx):
    """test_knn_lod's cloud at its smaller offset, at every k where pcp_knn_lod changes its
    compile-time list size (1, 4, 8, 16, 32) and the k just above each; k = 33 has no list."""
    from pointcloudprocess_amd import _lib, ops
    rng = np.random.default_rng(51)
    off = np.array((1234.3, -845.7, 12.1))
    xyz = rng.uniform(0, 30, (20_000, 3)) + off
    xyz = xyz.astype(np.float32).astype(np.float64)
    cloud = ora.make_cloud(xyz)
    qx = np.concatenate([xyz[:40] + 0.003, rng.uniform(0, 30, (40, 3)) + off])
    qc = ora.make_cloud(qx)
    dc, dq = ops.cloud_to_device(cloud, ctx.device), ops.cloud_to_device(qc, ctx.device)
    for k in (1, 4, 5, 8, 9, 16, 17, 32):
        gi, gd = ops.knn_lod(ctx, dc, dq, k)
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        for i in range(len(qc)):
            ei, ed = ora.knn_lod(cloud, qc[i:i + 1], k)
            assert np.array_equal(gi[i], ei), f"k={k} query {i}"
            assert np.array_equal(gd[i], ed), f"k={k} query {i}"
    with pytest.raises(_lib.PcpError) as err:
        ops.knn_lod(ctx, dc, dq, 33)
    assert err.value.code == -5  # PCP_ERR_UNSUPPORTED


def test_nearest_query(ctx):
    """K7: argmin over queries of the 1-NN d2, strict '<' from 9999, first query wins ties."""
    from pointcloudprocess_amd import ops
    xyz = _cloud(20_000, 61)
    q = _cloud(5000, 62)
    q[4000] = xyz[17]            # exact hit (d2 = 0) ...
    q[4500] = xyz[17]            # ... and a later tie: the first one wins
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    bq, bd = ops.nearest_query(ix, _dev(ctx, q))
    _, ed = ora.KdTree(xyz).knn(q, 1)
    best, mix = -1, 9999.0
    for j in range(len(q)):     # main_blend.cpp:314-320
        if ed[j, 0] < mix:
            mix, best = ed[j, 0], j
    assert (bq, bd) == (best, mix) == (4000, 0.0)
    bq, bd = ops.nearest_query(ix, _dev(ctx, q + 1e6))     # nothing under the bound
    assert bq == -1 and bd == 9999.0


def test_plane_fit_segments_and_radius_normals(ctx):
    from pointcloudprocess_amd import ops, synth
    xyz = synth.street_scene(30_000, 71, extent=(30.0, 30.0)).double().numpy()
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    g = ops.normals_radius(ix, 0.3).cpu().numpy()
    t = ora.KdTree(xyz)
    lib = ora.load()
    for i in range(0, len(xyz), 97):
        ei, _ = t.radius(xyz[i], 0.3)
        e = np.zeros(1, dtype=ora.PLANE)
        if len(ei) == 0:
            continue
        nb = np.ascontiguousarray(xyz[ei])
        lib.ora_plane_h_points(nb.ctypes.data, len(ei), e.ctypes.data)
        ev = np.array([e[f][0] for f in ("normal_x", "normal_y", "normal_z", "min_value", "curvature", "distance")])
        assert np.array_equal(g[i], ev.astype(np.float32), equal_nan=True), f"point {i}"


def test_radius_long_rows(ctx):
    """Rows longer than the LDS bitonic limit (1024) take the in-place path; max_nn keeps
    the insertion path; both stay bit-exact."""
    from pointcloudprocess_amd import ops
    xyz = _cloud(3000, 91, half=0.5)
    q = _cloud(40, 92, half=0.5)
    ix = ops.GridIndex(ctx, _dev(ctx, xyz))
    t = ora.KdTree(xyz)
    for r, mx in ((2.0, 0), (0.3, 0), (2.0, 2999), (2.0, 100)):
        offs, gi, gd = ops.radius(ix, _dev(ctx, q), r, mx)
        offs, gi, gd = offs.cpu().numpy(), gi.cpu().numpy(), gd.cpu().numpy()
        for i in range(len(q)):
            ei, ed = t.radius(q[i], r, mx)
            s, e = offs[i], offs[i + 1]
            assert np.array_equal(gi[s:e], ei) and np.array_equal(gd[s:e], ed), (r, mx, i)
