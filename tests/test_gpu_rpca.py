"""F3 calculate_plan_parameter_rpca (calculate_feature.cpp:208-368) on the GPU (rpca.hip)
against the oracle's restatement (ora_rpca) of the same deterministic contract: every field
of every LAS_POINT_PROPERTY record identical (normals, Distance, curvature as the floats and
doubles the reference stores).  kNN(20) rows come from pcp_knn (bit-exact vs the oracle's
kd-tree, tests/test_gpu_knn.py).  Parity vs the reference itself is unpinned: it seeds rand()
with time(NULL) and takes OpenCV's eigenvector sign.  The edge-shape tests below also hold
the records to an independent reference (tests/rpca_ref.py), which shares neither the Jacobi
nor the summation order nor the structure of the oracle."""
import numpy as np
import pytest
import torch

import oracle_ctypes as ora

pytestmark = pytest.mark.gpu
FIELDS = ("normal_x", "normal_y", "normal_z", "distance", "curvature", "point_id")


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _rows(ctx, xyz):
    from pointcloudprocess_amd import ops
    d = torch.from_numpy(xyz).to(ctx.device)
    index = ops.GridIndex(ctx, d)  # fp64 (KdTreeFLANN contract) for float64 clouds
    idx, _ = ops.knn(index, d, 20)
    return d, idx, index


@pytest.mark.parametrize("seed", [0, 12345])
def test_rpca_matches_oracle_street_scene(ctx, seed):
    from pointcloudprocess_amd import ops, synth
    xyz = synth.street_scene(60_000, 3101, extent=(40.0, 40.0), noise=0.01).double().numpy()
    rng = np.random.default_rng(3)
    out = rng.choice(len(xyz), 600, replace=False)  # 1 % outliers
    xyz[out] += rng.normal(0, 0.3, (len(out), 3))
    d, idx, index = _rows(ctx, xyz)
    g = ops.normals_rpca(ctx, d, idx, seed=seed).cpu().numpy().view(ops.POINT_PROPERTY).reshape(-1)
    e = ora.rpca(xyz, idx.cpu().numpy(), seed=seed)
    for f in FIELDS:
        assert _bits(g[f]) == _bits(e[f]), (f, int((g[f] != e[f]).sum()))
    assert (g["segment_id"] == 0).all()
    assert (np.abs(g["normal_z"]) > 0.99).mean() > 0.3  # the ground is a large part of the scene


def test_rpca_short_rows_and_unsupported(ctx):
    from pointcloudprocess_amd import ops
    xyz = np.random.default_rng(1).uniform(-1, 1, (500, 3))
    d, idx, index = _rows(ctx, xyz)
    idx[:7, 2:] = -1  # N <= 3: {0, 0, 0, curvature 1}
    g = ops.normals_rpca(ctx, d, idx).cpu().numpy().view(ops.POINT_PROPERTY).reshape(-1)
    e = ora.rpca(xyz, idx.cpu().numpy())
    for f in FIELDS:
        assert _bits(g[f]) == _bits(e[f]), (f, int((g[f] != e[f]).sum()))
    assert (g["curvature"][:7] == 1.0).all() and (g["normal_x"][:7] == 0).all()
    wide = torch.cat([idx, idx[:, :1]], dim=1)  # k = 21 > the reference's 20
    with pytest.raises(Exception):
        ops.normals_rpca(ctx, d, wide)


# ---------------------------------------------------------------------------------------
# Edge shapes.  Each case checks (A) every field bit-identical to the oracle and, where it
# says so, (B) the records against the independent reference (tests/rpca_ref.py: gates of
# plane_ref.py on rows with N >= 6, disagreement only at a decision margin <= 1e-6 and on at
# most 0.5 % of the rows) and (S) the structural property of the N = 4 / 5 rows
# (rpca_ref.check_small).  tests/test_rpca_ref.py shows that the oracle alone stays inside
# the same caps on the same inputs.

def _records(ctx, d, idx, **kw):
    from pointcloudprocess_amd import ops
    n = d.shape[0]
    assert idx.shape[0] == n and idx.dtype == torch.int32
    assert n == 0 or (int(idx.min()) >= -1 and int(idx.max()) < n)  # every index inside the cloud
    return ops.normals_rpca(ctx, d, idx, **kw).cpu().numpy().view(ops.POINT_PROPERTY).reshape(-1)


def _assert_same(g, e):
    for f in FIELDS + ("segment_id", "dis_from_point_plane"):
        assert _bits(g[f]) == _bits(e[f]), (f, int((g[f] != e[f]).sum()), np.flatnonzero(g[f] != e[f])[:8])


def _check(ctx, xyz, idx_host, label, ref=False, small=False, d=None, expect_gated=True, **kw):
    """Run the cloud (host xyz, host rows) on the GPU; A always, B / S on request."""
    import rpca_ref
    d = torch.from_numpy(xyz).to(ctx.device) if d is None else d
    g = _records(ctx, d, torch.from_numpy(idx_host).to(ctx.device), **kw)
    _assert_same(g, ora.rpca(xyz, idx_host, **kw))
    if ref:
        rpca_ref.compare(g, rpca_ref.rpca_ref(xyz, idx_host, **kw), label, expect_gated=expect_gated)
    if small:
        rpca_ref.check_small(g, xyz, idx_host, label)
    return g


def _knn_host(ctx, xyz, k):
    from pointcloudprocess_amd import ops
    d = torch.from_numpy(xyz).to(ctx.device)
    idx, _ = ops.knn(ops.GridIndex(ctx, d), d, k)
    return idx.cpu().numpy()


def _raw_call(ctx, d, stride, idx, pr, epi, out):
    return ctx.lib.pcp_normals_rpca(ctx.h, d.data_ptr(), stride, d.shape[0], idx.data_ptr(), idx.shape[1],
                                    pr, epi, 0, out.data_ptr())


@pytest.fixture(scope="module")
def scene(ctx):
    import rpca_ref
    xyz = rpca_ref.scene(1500, 11)
    return xyz, _knn_host(ctx, xyz, 20)


@pytest.mark.parametrize("pr,epi,iters", [(0.9999, 0.5, 68), (0.99, 0.7, 168), (0.5, 0.5, 5), (0.1, 0.5, 0)])
def test_rpca_iteration_counts(ctx, scene, pr, epi, iters):
    """68 and 168 iterations run the `it += 64` lane loop, where lane vi & 63 holds the winner of
    a later trip; 5 leaves most lanes idle; at 0 every record is the default."""
    import rpca_ref
    assert rpca_ref.iterations(pr, epi) == iters
    xyz, idx = scene
    g = _check(ctx, xyz, idx, f"gpu pr={pr} epi={epi}", ref=True, expect_gated=iters > 0, pr=pr, epi=epi, seed=3)
    if iters == 0:
        assert rpca_ref.record_fields(g)[3].all()


@pytest.mark.parametrize("pr,epi", [(1.0, 0.5), (0.99, 1.0)])
def test_rpca_refuses_pr_epi_and_leaves_the_output(ctx, scene, pr, epi):
    from pointcloudprocess_amd import ops
    xyz, idx = scene
    d, di = torch.from_numpy(xyz).to(ctx.device), torch.from_numpy(idx).to(ctx.device)
    with pytest.raises(Exception):
        ops.normals_rpca(ctx, d, di, pr=pr, epi=epi)
    out = torch.full((len(xyz), 48), 0xA5, dtype=torch.uint8, device=ctx.device)
    assert _raw_call(ctx, d, 24, di, pr, epi, out) != 0
    ctx.sync()
    assert bool((out == 0xA5).all())


@pytest.mark.parametrize("k", [4, 5, 6, 9, 13])
def test_rpca_narrow_k(ctx, scene, k):
    """hf = floor(2k/3) from 2 to 8, the sorting network's other lanes padded at +inf."""
    xyz, _ = scene
    idx = _knn_host(ctx, xyz, k)
    assert idx.shape == (len(xyz), k) and (idx >= 0).all()
    _check(ctx, xyz, idx, f"gpu k={k}", ref=k >= 6, small=k < 6, seed=5)


def test_rpca_mixed_row_lengths(ctx, scene):
    """Every N from 0 to 20 on at least 40 rows of one launch; the cnt <= 3 default outcome is
    reached both ways on the N = 4 / 5 rows (the best plane passes through hf points exactly,
    so the MAD is rounding noise)."""
    import rpca_ref
    xyz, idx = scene
    rows, length = rpca_ref.mixed_rows(idx)
    assert np.bincount(length, minlength=21).min() >= 40
    g = _check(ctx, xyz, rows, "gpu mixed N", ref=True, small=True, seed=9)
    rdef = rpca_ref.record_fields(g)[3]
    assert rdef[length <= 3].all()
    assert rdef[length == 5].any() and (~rdef[length == 4]).any()


def test_rpca_lattice_mad_zero(ctx):
    """An exact lattice plane: MAD == 0 where more than half the neighbours lie on it, and then
    the lifted outliers are kept too (tilted rows)."""
    import rpca_ref
    xyz = rpca_ref.lattice()
    g = _check(ctx, xyz, _knn_host(ctx, xyz, 20), "gpu lattice", ref=True, seed=4)
    assert (g["normal_z"] == 1.0).any()
    assert ((g["curvature"] != 1.0) & (g["normal_z"] < 0.999)).any()


def test_rpca_duplicate_points(ctx):
    """Zero-area draws and all-equal distances: the stable sort and the earliest-iteration rule
    decide.  Oracle only (the reference is excused on nearly every row here)."""
    import rpca_ref
    xyz = np.repeat(rpca_ref.scene(300, 12), 5, axis=0)
    idx = _knn_host(ctx, xyz, 20)
    g = _check(ctx, xyz, idx, "gpu duplicates", seed=6)
    e = ora.rpca(xyz, idx, seed=6)
    for f in FIELDS:
        assert not (np.isnan(g[f].astype(np.float64)) & ~np.isnan(e[f].astype(np.float64))).any(), f
    assert (~rpca_ref.record_fields(g)[3]).mean() > 0.5


@pytest.mark.parametrize("offset", [(300.0, -200.0, 40.0), (3000.0, 7000.0, 100.0), (5e5, 4e6, 100.0)])
def test_rpca_large_coordinates(ctx, scene, offset):
    """The contract's float32 products quantise the distances at these coordinates."""
    xyz = scene[0] * 20.0 + np.array(offset)
    _check(ctx, xyz, _knn_host(ctx, xyz, 20), f"gpu offset {offset}", ref=True, seed=2)


def test_rpca_row_stride(ctx, scene):
    """Strides of 48 (the C++ shim's sizeof(CloudItem)) and 32 bytes against the packed run; a
    stride that is not whole doubles is refused."""
    xyz, idx = scene
    di = torch.from_numpy(idx).to(ctx.device)
    base = _records(ctx, torch.from_numpy(xyz).to(ctx.device), di, seed=8)
    _assert_same(base, ora.rpca(xyz, idx, seed=8))
    for cols in (6, 4):
        wide = torch.full((len(xyz), cols), 1e30, dtype=torch.float64, device=ctx.device)
        wide[:, :3] = torch.from_numpy(xyz).to(ctx.device)
        view = wide[:, :3]
        assert view.stride(0) * view.element_size() == 8 * cols
        assert _records(ctx, view, di, seed=8).tobytes() == base.tobytes(), cols
    out = torch.full((len(xyz), 48), 0xA5, dtype=torch.uint8, device=ctx.device)
    with pytest.raises(Exception):
        ctx.check(_raw_call(ctx, wide, 28, di, 0.99, 0.5, out))
    ctx.sync()
    assert bool((out == 0xA5).all())


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_rpca_tiny_clouds(ctx, n):
    """pcp_knn gives rows shorter than k: all default at n <= 3, N = 5 at n = 5."""
    import rpca_ref
    xyz = rpca_ref.scene(1500, 13)[:n].copy()
    idx = _knn_host(ctx, xyz, 20)
    assert idx.shape == (n, 20) and (rpca_ref.leading_run(idx) == n).all()
    g = _check(ctx, xyz, idx, f"gpu n={n}", small=True, seed=1)
    assert len(g) == n
    if n <= 3:
        assert rpca_ref.record_fields(g)[3].all()


def test_rpca_ragged_launch_is_row_local(ctx):
    """n = 1501 (the last block holds one live wave) against the same cloud's first 1000 rows
    run alone: the record of row j depends on (seed, j, row contents) only."""
    import rpca_ref
    xyz = rpca_ref.scene(1501, 14)
    head = np.ascontiguousarray(xyz[:1000])
    idx_head = _knn_host(ctx, head, 20)
    idx = _knn_host(ctx, xyz, 20)
    idx[:1000] = idx_head
    a = _check(ctx, head, idx_head, "gpu n=1000", seed=10)
    b = _check(ctx, xyz, idx, "gpu n=1501", ref=True, seed=10)
    assert b[:1000].tobytes() == a.tobytes()


def test_rpca_storage_permutation(ctx, scene):
    """Permuting the cloud's storage order (indices remapped, row j kept at position j) changes
    no bit: nothing depends on where a neighbour is stored."""
    xyz, idx = scene
    rng = np.random.default_rng(15)
    p = rng.permutation(len(xyz))
    inv = np.empty_like(p)
    inv[p] = np.arange(len(p))
    idx2 = np.where(idx >= 0, inv[np.maximum(idx, 0)], -1).astype(np.int32)
    a = _check(ctx, xyz, idx, "gpu storage order", seed=11)
    b = _check(ctx, np.ascontiguousarray(xyz[p]), idx2, "gpu permuted storage", seed=11)
    assert a.tobytes() == b.tobytes()


def test_rpca_wide_seeds(ctx, scene):
    """All 64 seed bits reach the draws."""
    xyz, idx = scene
    lo = _check(ctx, xyz, idx, "gpu seed 1", seed=1)
    hi = _check(ctx, xyz, idx, "gpu seed 2^32+1", seed=2 ** 32 + 1)
    assert (lo["normal_x"] != hi["normal_x"]).any()
    _check(ctx, xyz, idx, "gpu seed 2^63+5", ref=True, seed=2 ** 63 + 5)


def test_rpca_second_grid_stride_trip(ctx, scene):
    """n = 4 * 2^20 + 2048: the launch is capped at 2^20 blocks of four waves, so waves 0..2047
    take a second point (`j += nwaves`, the barrier that protects the LDS rows).  They handle a
    full row (N = 8) first and a shorter one (N = 6) second; every other row is -1.  No smaller
    n reaches that loop."""
    import rpca_ref
    base, _ = scene
    m, k, live = len(base), 8, 2048
    first = 4 << 20
    n = first + live
    knn8 = _knn_host(ctx, base, k)
    xyz = np.ascontiguousarray(np.tile(base, (n // m + 1, 1))[:n])  # xyz[i] = base[i % m]
    idx = np.full((n, k), -1, np.int32)
    idx[:live] = knn8[np.arange(live) % m]
    shift = (n // m - 1) * m                                        # the same points, stored near the end
    j2 = np.arange(first, n)
    idx[j2] = knn8[j2 % m] + shift
    idx[j2, 6:] = -1
    assert idx.max() < n
    rows = np.r_[np.arange(live), j2]
    g = _check(ctx, xyz, idx, "gpu second trip", seed=12)
    ref = rpca_ref.rpca_ref(xyz, idx, seed=12, rows=rows)
    assert (ref["N"][:live] == 8).all() and (ref["N"][live:] == 6).all()
    rpca_ref.compare(g[rows], ref, "gpu second trip")
    assert rpca_ref.record_fields(g)[3][live:first].all()


def test_rpca_holed_rows_stop_at_the_first_gap(ctx, scene):
    """N is the leading run (pcp.h, the oracle): a row with a -1 at position 3, 7 or 12 followed
    by valid indices is the row cut there.  The cloud is a view eight rows into a larger tensor."""
    import rpca_ref
    xyz, idx = scene
    holed = idx.copy()
    pos = np.array([3, 7, 12])[np.arange(len(idx)) % 3]
    holed[np.arange(len(idx)), pos] = -1
    assert (rpca_ref.leading_run(holed) == pos).all() and (holed[:, 13:] >= 0).all()
    big = torch.full((len(xyz) + 8, 3), 1e30, dtype=torch.float64, device=ctx.device)
    big[8:] = torch.from_numpy(xyz).to(ctx.device)
    g = _check(ctx, xyz, holed, "gpu holed rows", ref=True, d=big[8:], seed=13)
    cut = holed.copy()
    cut[np.arange(idx.shape[1])[None, :] >= pos[:, None]] = -1
    assert g.tobytes() == _records(ctx, big[8:], torch.from_numpy(cut).to(ctx.device), seed=13).tobytes()
    assert rpca_ref.record_fields(g)[3][pos == 3].all()
