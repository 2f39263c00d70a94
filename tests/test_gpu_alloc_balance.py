"""Every entry point gives back the device temporaries it took: the number of blocks the
context's allocator has handed out (pcp_ctx_alloc_stats, out[0]) is the same before a call and
after it, once the handles the call made are destroyed -- on success, and after each rejection
that plain arguments can reach once buffers were allocated.  Nothing is made to fail here: the
HIP error paths are correct by construction (the per-call guard of common.hpp)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_ctypes as ora

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = -1, -5, -7


def _xyz(n, seed, finite=False):
    """n points in a 8 m box; unless `finite`, every 7th row is NaN and one more is +inf (so the
    index build compacts), starting with row 0."""
    xyz = np.random.default_rng(seed).uniform(-4.0, 4.0, (n, 3)).astype(np.float32).astype(np.float64)
    if not finite:
        xyz[::7] = np.nan
        if n > 4:
            xyz[4, 1] = np.inf
    return xyz


# 9 points: 6 finite (k clamps to the cloud); 130: not a multiple of any block; 500: several blocks
# of the 256-thread passes; the all-finite cloud takes the build's direct branch
CLOUDS = {"n9": _xyz(9, 1), "n130": _xyz(130, 2), "n500": _xyz(500, 3), "finite300": _xyz(300, 4, finite=True)}


@pytest.fixture(params=list(CLOUDS))
def cloud(request):
    xyz = CLOUDS[request.param]
    return xyz, bool(np.isfinite(xyz).all())


@pytest.fixture
def ctx():
    from pointcloudprocess_amd import ops
    c = ops.Context(0)
    yield c
    c.close()


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _cloud48(ctx, xyz):
    from pointcloudprocess_amd import ops
    return ops.cloud_to_device(ora.make_cloud(xyz), ctx.device)


@contextlib.contextmanager
def balanced(ctx, what):
    before = ctx.alloc_stats()[0]
    yield
    ctx.sync()
    after = ctx.alloc_stats()[0]
    assert after == before, f"{what}: {after - before} block(s) still handed out ({before} -> {after})"


@contextlib.contextmanager
def rejected(ctx, what, code):
    from pointcloudprocess_amd import PcpError
    with balanced(ctx, what), pytest.raises(PcpError) as e:
        yield
    assert e.value.code == code, (what, e.value.code)


def test_getter(ctx):
    from pointcloudprocess_amd import ops
    assert ctx.alloc_stats() == (0, 0, 0, 0)
    ix = ops.GridIndex(ctx, _dev(ctx, CLOUDS["n130"]))
    blocks, nbytes, peak, mallocs = ctx.alloc_stats()
    assert blocks > 0 and nbytes >= 4096 * blocks and peak >= nbytes and mallocs >= blocks
    ix.close()
    assert ctx.alloc_stats()[:2] == (0, 0) and ctx.alloc_stats()[2:] == (peak, mallocs)
    assert ctx.lib.pcp_ctx_alloc_stats(None, (C.c_int64 * 4)()) == ERR_ARG


def test_index_builds(ctx, cloud):
    from pointcloudprocess_amd import ops
    xyz, _ = cloud
    d64, d32 = _dev(ctx, xyz), _dev(ctx, xyz.astype(np.float32))
    sub = torch.arange(0, len(xyz), 2, dtype=torch.int32)
    for what, make in [("f64", lambda: ops.GridIndex(ctx, d64)),
                       ("f64 given cell", lambda: ops.GridIndex(ctx, d64, cell_size=0.5)),
                       ("f64 indices", lambda: ops.GridIndex(ctx, d64, indices=sub)),
                       ("f64 aos48", lambda: ops.GridIndex(ctx, _cloud48(ctx, xyz))),
                       ("f32", lambda: ops.GridIndex(ctx, d32)),
                       ("f32 given cell", lambda: ops.GridIndex(ctx, d32, cell_size=0.5)),
                       ("h16", lambda: ops.H16Index(ctx, d32, 0.5))]:
        with balanced(ctx, "build " + what):
            make().close()


def test_searches(ctx, cloud):
    from pointcloudprocess_amd import ops
    xyz, _ = cloud
    d = _dev(ctx, xyz)
    with balanced(ctx, "index + searches"):
        ix = ops.GridIndex(ctx, d, cell_size=0.5)
        for what, call in [("knn", lambda: ops.knn(ix, d, 5)),
                           ("radius near", lambda: ops.radius(ix, d, 0.4)),      # < 3 cell rings
                           ("radius far", lambda: ops.radius(ix, d, 6.0)),       # straight to the far pass
                           ("nearest_query", lambda: ops.nearest_query(ix, d)),
                           ("normals dense", lambda: ops.normals_knn(ix, 8))]:
            with balanced(ctx, what):
                call()
        ix.close()


def test_normals_sparse_grid(ctx, cloud):
    """Two copies of the cloud 300 m apart at 0.4 m cells: too many cells for a dense table."""
    from pointcloudprocess_amd import ops
    xyz, _ = cloud
    d = _dev(ctx, np.concatenate([xyz, xyz + 300.0]))
    with balanced(ctx, "sparse index + normals"):
        ix = ops.GridIndex(ctx, d, cell_size=0.4)
        with balanced(ctx, "normals sparse"):
            ops.normals_knn(ix, 8)
        assert ops.normals_knn_last_deferred(ctx)[0] == -1  # no tile: the sparse path ran
        with balanced(ctx, "knn sparse"):
            ops.knn(ix, d, 5)
        ix.close()


def test_knn_lod(ctx):
    """pcp_knn_lod takes a dense cloud by contract (its centroid is a plain fold)."""
    from pointcloudprocess_amd import ops
    c = _cloud48(ctx, CLOUDS["finite300"])
    with balanced(ctx, "knn_lod"):
        ops.knn_lod(ctx, c, c[:50].contiguous(), 4)


def test_bruteforce(ctx, cloud):
    from pointcloudprocess_amd import ops
    xyz, _ = cloud
    d = _dev(ctx, xyz)
    with balanced(ctx, "bruteforce nt > 0"):
        ops.knn_bruteforce(ctx, d, d, 4)
    with balanced(ctx, "bruteforce nt == 0"):
        ops.knn_bruteforce(ctx, d[:0], d, 4)


def test_cloud_passes(ctx, cloud):
    from pointcloudprocess_amd import ops
    xyz, dense = cloud
    c = _cloud48(ctx, xyz)
    for what, call in [("voxel filter", lambda: ops.voxel_filter(ctx, c, 0.5, is_dense=dense)),
                       ("voxel filter + idx", lambda: ops.voxel_filter(ctx, c, 0.5, dense, False, True)),
                       ("remove_duplicate", lambda: ops.remove_duplicate(ctx, c, 0.5, is_dense=dense)),
                       ("minmax", lambda: ops.minmax(ctx, c, dense)),
                       ("centroid", lambda: ops.centroid(ctx, c, dense)),
                       ("centroid_concat", lambda: ops.centroid_concat(ctx, c, c, dense)),
                       ("get_rot_icp", lambda: ops.get_rot_icp(ctx, c, c, 0.5, 3, src_dense=dense, temp_dense=dense))]:
        with balanced(ctx, what):
            call()


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("gid", [False, True])
def test_h16_radius_fill(ctx, cloud, normals, gid):
    from pointcloudprocess_amd import ops
    xyz, _ = cloud
    d = _dev(ctx, xyz.astype(np.float32))
    ids = torch.arange(1000, 1000 + len(xyz), dtype=torch.int32, device=ctx.device) if gid else None
    with balanced(ctx, "h16 index + fill"):
        ix = ops.H16Index(ctx, d, 0.5)
        with balanced(ctx, f"h16 fill normals={normals} gid={gid}"):
            ix.radius_normals(0.5, global_id=ids, normals=normals)
        ix.close()


def test_region_growing(ctx, cloud):
    from pointcloudprocess_amd import ops, segments
    xyz, _ = cloud
    d = _dev(ctx, xyz)
    p = np.zeros(len(xyz), ops.POINT_PROPERTY)
    p["normal_z"] = 1.0
    p["point_id"] = np.arange(len(xyz))
    dp = _dev(ctx, p.view(np.uint8).reshape(len(p), 48))
    with balanced(ctx, "index + region growing"):
        ix = ops.GridIndex(ctx, d)
        with balanced(ctx, "region growing"):
            segments.region_growing(ix, d, dp, 0.5, 0.9)
        ix.close()


def test_cloudgrid(ctx, cloud):
    from pointcloudprocess_amd.cloudgrid import CloudGrid
    xyz, _ = cloud
    fin = np.nan_to_num(xyz, nan=1.5, posinf=2.5)  # the map cache takes finite points
    a, b = _cloud48(ctx, fin), _cloud48(ctx, fin + 0.25)
    with balanced(ctx, "cloudgrid"):
        g = CloudGrid(ctx)
        g.add_cloud_internal(a)
        held = ctx.alloc_stats()[0]
        g.add_cloud_internal(b)  # the merge swaps the grid's three blocks for three new ones
        assert ctx.alloc_stats()[0] == held
        for what, call in [("box", lambda: g.box(-5, 5, -5, 5)), ("points", g.get_grid_cloud),
                           ("match", lambda: g.get_grid_cloud_match(a, 0.3))]:
            with balanced(ctx, what):
                call()
        # outputs too small for the result: rejected after the temporaries were taken
        n, n2 = C.c_int64(), C.c_int64()
        out = torch.empty((1, 48), dtype=torch.uint8, device=ctx.device)
        with rejected(ctx, "box cap", ERR_CAPACITY):
            ctx.check(ctx.lib.pcp_grid_box(ctx.h, g.h, -5, 5, -5, 5, C.c_void_p(out.data_ptr()), 1, C.byref(n)))
        src_out = torch.empty_like(a)
        with rejected(ctx, "match cap", ERR_CAPACITY):
            ctx.check(ctx.lib.pcp_grid_match(ctx.h, g.h, C.c_void_p(a.data_ptr()), a.shape[0], 0.3,
                                             C.c_void_p(src_out.data_ptr()), C.byref(n),
                                             C.c_void_p(out.data_ptr()), 1, C.byref(n2)))
        g.close()


def test_icp(ctx, cloud):
    from pointcloudprocess_amd import ops, synth
    xyz, _ = cloud
    tgt = _dev(ctx, xyz.astype(np.float32))
    T = synth.rigid(0.05, 0.02, 0.0, (0.01, 0.0, 0.0))
    with np.errstate(invalid="ignore"):  # (inf * 0 in the non-finite rows)
        q = _dev(ctx, (xyz @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
    with balanced(ctx, "icp_create"):
        ix = ops.GridIndex(ctx, tgt, cell_size=0.5)
        icp = ops.ICP(ix, q)
        with balanced(ctx, "set_options(WIDE_CACHE)"):
            icp.set_options(wide_cache=True)
        T_dev, stats = icp.new_pose()
        with balanced(ctx, "run_dev, 3 launches"):
            icp.run_dev(T_dev, stats, 0.5, 3)
        with balanced(ctx, "step + run"):
            icp.step(np.eye(4), 0.5, corr=True)
            icp.run(np.eye(4), 0.5, 2)
        with balanced(ctx, "keys + owned accumulators"):
            keys = icp.keys_dev(T_dev, 0.5)
            icp.accumulate_keys(np.eye(4), icp.keys(np.eye(4), 0.5), 0, len(xyz), tgt)
            bounds = torch.tensor([0, len(xyz)], dtype=torch.int64, device=ctx.device)
            owner = ops.keys_owner(ctx, keys, bounds)
            ops.accumulate_owned(ctx, T_dev, q, keys, owner, 0, 0, len(xyz), tgt)
        icp.close()
        ix.close()
    with balanced(ctx, "pilot forced on + captured graph"):
        ix = ops.GridIndex(ctx, tgt, cell_size=0.5)
        icp = ops.ICP(ix, q)
        icp.set_options(pilot=True)  # the pilot's accumulators are a block of the handle's
        T_dev, stats = icp.new_pose()
        icp.run_dev(T_dev, stats, 0.5, 3)
        icp.close()
        icp = ops.ICP(ix, q)
        icp.set_options(graph=True)  # captured at launch 2, replayed at launch 3, torn down by close
        T_dev, stats = icp.new_pose()
        icp.run_dev(T_dev, stats, 0.5, 4)
        icp.close()
        ix.close()
    with balanced(ctx, "icp_create_with_target"):
        icp = ops.ICP.with_target(ctx, tgt, q, 0.5)
        icp.run(np.eye(4), 0.5, 2)
        index = icp.index
        icp.close()
        index.close()
    with balanced(ctx, "icp_create_with_target, automatic cell"):
        icp = ops.ICP.with_target(ctx, tgt, q, 0.0)
        index = icp.index
        icp.close()
        index.close()


def test_late_rejections(ctx):
    from pointcloudprocess_amd import ops
    # three points 500 m apart at 0.5 m cells: 1002^3 cells > 2^26, so the fp32 index is built in
    # full with the sparse layout and only then refused
    far = _dev(ctx, np.array([[0, 0, 0], [500, 0, 0], [0, 500, 500]], dtype=np.float32))
    with rejected(ctx, "h16 on a sparse layout", ERR_UNSUPPORTED):
        ops.H16Index(ctx, far, 0.5)
    d = _dev(ctx, CLOUDS["n130"])
    ix = ops.GridIndex(ctx, d, cell_size=0.5)
    out = torch.empty((8, 6), dtype=torch.float32, device=ctx.device)
    with rejected(ctx, "normals n_out too small", ERR_CAPACITY):
        ctx.check(ctx.lib.pcp_normals_knn(ctx.h, ix.h, 8, C.c_void_p(out.data_ptr()), 8))
    with rejected(ctx, "icp_create on an fp64 index", ERR_ARG):
        ops.ICP(ix, _dev(ctx, CLOUDS["n130"].astype(np.float32)))
    with rejected(ctx, "knn k > 64", ERR_UNSUPPORTED):
        ops.knn(ix, d, 65)
    ix.close()
    assert ctx.alloc_stats()[0] == 0
