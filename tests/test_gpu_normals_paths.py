"""pcp_normals_knn (C3) with every search path forced (MI355X): the tile pass's tie handling,
the template buckets and clamps, oversize groups, the brick-run split, the far pass, the
sparse grid (no tile), an indices subset and degenerate neighbourhoods.

Every case compares all six plane fields with the oracle by the project's rule,
|diff| <= 1e-6 max(1, |expected|), NaN equal only to NaN, and prints the share of bit-identical
rows.  Where stated the planes are also held to the independent fp64+ reference of
tests/plane_ref.py at its gates.  A release build cannot tell which pass answered a row, so the
cases that exist to force a pass assert pcp_normals_knn_last_deferred's counts as well: a
constant that changes cannot quietly stop them from reaching their path.
"""
import numpy as np
import pytest
import torch

import oracle_ctypes as ora
import plane_ref

pytestmark = pytest.mark.gpu

DEFAULT_PLANE = np.array([0, 0, 0, 0, 1, 0], dtype=np.float32)  # rpca's N <= 3 branch


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def _uniform(n, seed, half):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-half, half, (n, 3)).astype(np.float32)).astype(np.float64)


def _parity(g, e, label):
    """The project's plane rule on all six fields, NaN-aware; prints the bit-identical share."""
    ev = np.stack([e[f] for f in plane_ref.FIELDS], 1) if e.dtype.names else np.asarray(e, dtype=np.float32)
    assert g.shape == ev.shape, (g.shape, ev.shape)
    both_nan = np.isnan(g) & np.isnan(ev)
    with np.errstate(invalid="ignore"):
        diff = np.abs(g.astype(np.float64) - ev.astype(np.float64))
        ok = both_nan | (diff <= 1e-6 * np.maximum(1.0, np.abs(ev)))
    exact = (both_nan | (g == ev)).all(1).mean()
    print(f"{label}: bit-identical rows {exact:.6f}, max |diff| {np.nanmax(diff):.3e}, "
          f"rows outside the rule {int((~ok).any(1).sum())}")
    assert ok.all(), f"{label}: {int((~ok).any(1).sum())} rows outside the 1e-6 rule, first {np.argwhere(~ok)[:5].tolist()}"


def _normals(ctx, xyz, k, cell_size=0.0, indices=None):
    """GPU planes (n, 6) float32 and (tile_deferred, far_queries) of the call."""
    from pointcloudprocess_amd import ops
    ix = ops.GridIndex(ctx, _dev(ctx, xyz), cell_size=cell_size, indices=indices)
    g = ops.normals_knn(ix, k)
    deferred = ops.normals_knn_last_deferred(ctx)
    g = g.cpu().numpy()
    ix.close()
    return g, deferred


# ---------------------------------------------------------------- a. tie lattice
LATTICE_K = (5, 8, 9, 16, 17, 20, 32)


def _lattice():
    i, j, s = (a.ravel() for a in np.meshgrid(np.arange(56), np.arange(56), np.arange(2), indexing="ij"))
    xyz = np.stack([0.25 * i, 0.25 * j, 0.0625 * (i % 2) + 0.03125 * ((j // 2) % 2) + 1.5 * s], 1)
    return xyz[np.random.default_rng(3).permutation(len(xyz))]  # ties must break on index, not position


@pytest.fixture(scope="module")
def lattice():
    """Two ridged sheets on a dyadic lattice (every d2 exact), shuffled; per k the oracle's planes,
    the reference's planes of the oracle's neighbour sets, and the proof that the case has teeth."""
    xyz = _lattice()
    assert len(xyz) == 6272
    t = ora.KdTree(xyz)
    per_k = {}
    for k in LATTICE_K:
        idx, d2 = t.knn(xyz, k + 1)
        tied = d2[:, k - 1] == d2[:, k]
        if k in (8, 16, 20, 32):
            assert tied.mean() >= 0.8, (k, tied.mean())  # measured 0.96, 0.92, 0.87, 0.98
        e = ora.normals_knn(xyz, k)
        # ties broken in the opposite index order (the reversed cloud's oracle): every tied row's
        # plane moves by more than the rule, so a wrong tie-break in the tile cannot pass
        er = plane_ref.as_rows(ora.normals_knn(xyz[::-1].copy(), k))[::-1]
        ev = plane_ref.as_rows(e)
        moved = (np.abs(ev - er) > 1e-6 * np.maximum(1.0, np.abs(ev))).any(1)
        assert moved[tied].all(), (k, int((tied & ~moved).sum()))
        ref = plane_ref.plane_ref(xyz[idx[:, :k]])
        assert ref["gap"].min() >= 0.14, (k, ref["gap"].min())  # well-conditioned everywhere
        plane_ref.check(e, ref, f"lattice oracle k={k}", max_excluded=0.0)
        per_k[k] = (e, ref, float(tied.mean()))
    return xyz, per_k


@pytest.mark.parametrize("cell", [0.0, 0.25])  # 0.25: the points lie exactly on cell faces
@pytest.mark.parametrize("k", LATTICE_K)
def test_tie_lattice(ctx, lattice, k, cell):
    xyz, per_k = lattice
    e, ref, share = per_k[k]
    g, deferred = _normals(ctx, xyz, k, cell_size=cell)
    print(f"k={k} cell={cell}: tied rows {share:.3f}, (tile_deferred, far_queries) = {deferred}")
    assert deferred[0] >= 0  # a dense grid: the tile ran
    _parity(g, e, f"lattice k={k} cell={cell}")
    plane_ref.check(g, ref, f"lattice gpu k={k} cell={cell}", max_excluded=0.0)


# ---------------------------------------------------------------- b. buckets and clamps
@pytest.fixture(scope="module")
def street():
    from pointcloudprocess_amd import synth
    return synth.street_scene(30_000, 33, extent=(30.0, 30.0)).double().numpy()


@pytest.mark.parametrize("k", [4, 5, 7, 9, 16, 17])
def test_buckets(ctx, street, k):
    g, deferred = _normals(ctx, street, k)
    print(f"k={k}: (tile_deferred, far_queries) = {deferred}")
    assert deferred[0] >= 0
    _parity(g, ora.normals_knn(street, k), f"street k={k}")


def test_k_above_32_unsupported(ctx, street):
    from pointcloudprocess_amd import _lib, ops
    ix = ops.GridIndex(ctx, _dev(ctx, street))
    with pytest.raises(_lib.PcpError) as err:
        ops.normals_knn(ix, 33)
    assert err.value.code == -5  # PCP_ERR_UNSUPPORTED
    assert ops.normals_knn_last_deferred(ctx) == (0, 0)  # nothing was searched
    g = ops.normals_knn(ix, 32).cpu().numpy()  # the context and the index are still usable
    _parity(g, ora.normals_knn(street, 32), "street k=32 after the error")


@pytest.mark.parametrize("n,k", [(6, 8), (4, 20)])  # clamped to 6 (K = 8) and to 4 (K = 4)
def test_k_clamped_to_cloud(ctx, n, k):
    xyz = _uniform(n, 43, 1.0)
    g, deferred = _normals(ctx, xyz, k)
    e = ora.normals_knn(xyz, k)
    assert not (plane_ref.as_rows(e) == DEFAULT_PLANE).all(1).any()  # n > 3: a real plane per row
    _parity(g, e, f"{n} points k={k}")
    ref = plane_ref.plane_ref(np.broadcast_to(xyz, (n, n, 3)))  # every row's neighbourhood is the cloud
    plane_ref.check(g, ref, f"{n} points k={k} vs reference", max_excluded=0.0)


# ---------------------------------------------------------------- c. oversize clump
@pytest.mark.parametrize("k", [8, 32])
def test_oversize_clump(ctx, k):
    """3,000 points inside a 0.05 m ball on a 0.25 m grid: every box holding the clump's cell
    (or cells) exceeds the tile's LDS list, so those groups take the exact search."""
    rng = np.random.default_rng(47)
    d = rng.normal(size=(3000, 3))
    d *= (0.05 * rng.uniform(0, 1, (3000, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    xyz = np.concatenate([_uniform(20_000, 45, 5.0), np.array([1.1, -2.3, 0.7]) + d])
    xyz = xyz.astype(np.float32).astype(np.float64)[rng.permutation(len(xyz))]
    g, (tile_deferred, far_queries) = _normals(ctx, xyz, k, cell_size=0.25)
    print(f"k={k}: tile_deferred {tile_deferred}, far_queries {far_queries}")
    _parity(g, ora.normals_knn(xyz, k), f"clump k={k}")
    assert tile_deferred >= 3000


# ---------------------------------------------------------------- d. wide waves, far pass
@pytest.mark.parametrize("k", [8, 20])
def test_wide_waves_and_far_pass(ctx, k):
    """~0.003 points per cell of a dense table: a wave's 64 queries span many bricks (the
    brick-run split) and the neighbours lie beyond the tile window and the near pass's rings."""
    xyz = _uniform(3000, 49, 20.0)
    n = len(xyz)
    g, (tile_deferred, far_queries) = _normals(ctx, xyz, k, cell_size=0.4)
    print(f"k={k}: tile_deferred {tile_deferred}, far_queries {far_queries} of {n}")
    _parity(g, ora.normals_knn(xyz, k), f"thin cloud k={k}")
    assert tile_deferred >= 0.9 * n
    assert far_queries >= 0.9 * n


# ---------------------------------------------------------------- e. sparse grid
@pytest.fixture(scope="module")
def two_clusters():
    """test_knn_sparse_grid's cloud: the bounding grid at 0.02 m is too large for a dense table."""
    a = _uniform(20_000, 15, 5.0)
    b = _uniform(20_000, 16, 5.0) + 5000.0
    return np.concatenate([a, b])


@pytest.mark.parametrize("k", [8, 20])
def test_sparse_grid(ctx, two_clusters, k):
    xyz = two_clusters
    g, (tile_deferred, far_queries) = _normals(ctx, xyz, k, cell_size=0.02)
    print(f"k={k}: tile_deferred {tile_deferred}, far_queries {far_queries}")
    assert tile_deferred == -1  # no tile on a sparse grid
    _parity(g, ora.normals_knn(xyz, k), f"sparse k={k}")
    idx, _ = ora.KdTree(xyz).knn(xyz, k)
    # measured on the reference alone: 0.005 % of rows at or under the gap threshold
    plane_ref.check(g, plane_ref.plane_ref(xyz[idx]), f"sparse gpu k={k} vs reference", max_excluded=1e-3)


@pytest.mark.parametrize("k", [8, 20])
def test_sparse_grid_far_pass(ctx, k):
    """The two-cluster grid above is coarsened to ~5 m cells by the brick-table cap, so its near
    pass answers every row.  Here the 0.4 m cells stand (802^3 cells: too many for a dense table,
    201^3 bricks: under the cap) and hold ~0.01 points each, so the rows reach past the near
    pass's rings and the wave-per-query pass answers them without a tile before it."""
    xyz = np.concatenate([_uniform(1500, 51, 10.0), _uniform(1500, 52, 10.0) + 300.0])
    n = len(xyz)
    g, (tile_deferred, far_queries) = _normals(ctx, xyz, k, cell_size=0.4)
    print(f"k={k}: tile_deferred {tile_deferred}, far_queries {far_queries} of {n}")
    assert tile_deferred == -1
    _parity(g, ora.normals_knn(xyz, k), f"sparse thin k={k}")
    assert far_queries >= 0.9 * n


def test_sparse_grid_radius(ctx, two_clusters):
    from pointcloudprocess_amd import ops
    xyz = two_clusters
    q = np.concatenate([xyz[:1000] + 0.05, xyz[20_000:21_000] - 0.05])
    ix = ops.GridIndex(ctx, _dev(ctx, xyz), cell_size=0.02)
    offs, gi, gd = ops.radius(ix, _dev(ctx, q), 0.3)
    offs, gi, gd = offs.cpu().numpy(), gi.cpu().numpy(), gd.cpu().numpy()
    t = ora.KdTree(xyz)
    rows = 0
    for i in range(len(q)):
        ei, ed = t.radius(q[i], 0.3)
        s, e = offs[i], offs[i + 1]
        assert np.array_equal(gi[s:e], ei), f"query {i}"
        assert np.array_equal(gd[s:e], ed), f"query {i}"
        rows += len(ei) > 0
    assert rows >= 0.5 * len(q)  # the search has something to find


# ---------------------------------------------------------------- f. indices subset, NaN rows
@pytest.mark.parametrize("k", [8, 20])
def test_indices_subset_and_nonfinite(ctx, k):
    from pointcloudprocess_amd import synth
    xyz = synth.street_scene(20_000, 35, extent=(30.0, 30.0)).double().numpy()
    xyz[::97] = np.nan
    xyz[5::101, 1] = np.inf
    n = len(xyz)
    sub = np.arange(0, n, 3, dtype=np.int32)
    g, deferred = _normals(ctx, xyz, k, indices=torch.from_numpy(sub))
    print(f"k={k}: (tile_deferred, far_queries) = {deferred}")
    finite = np.isfinite(xyz).all(1)
    sel = np.zeros(n, bool)
    sel[sub] = True
    sel &= finite
    assert (sel[sub] == 0).sum() > 20 and sel.sum() > 6000
    # rows outside the subset and non-finite rows keep the default plane, exactly
    assert np.array_equal(g[~sel], np.broadcast_to(DEFAULT_PLANE, (int((~sel).sum()), 6)))
    t = ora.KdTree(xyz, indices=sub)
    rows = np.flatnonzero(sel)
    idx, _ = t.knn(xyz[rows], k)
    assert (idx >= 0).all() and sel[idx].all()
    lib = ora.load()
    e = np.zeros(len(rows), dtype=ora.PLANE)
    for r in range(len(rows)):
        nb = np.ascontiguousarray(xyz[idx[r]])
        lib.ora_plane_h_points(nb.ctypes.data, k, e[r:r + 1].ctypes.data)
    _parity(g[rows], e, f"subset k={k}")


# ---------------------------------------------------------------- g. degenerate neighbourhoods
def _degenerate(ctx, xyz, k, label):
    g, deferred = _normals(ctx, xyz, k)  # raises unless the call returned PCP_OK
    e = ora.normals_knn(xyz, k)
    ev = plane_ref.as_rows(e)
    both_nan = np.isnan(g) & np.isnan(ev.astype(np.float32))
    print(f"{label}: bit-identical rows {(both_nan | (g == ev.astype(np.float32))).all(1).mean():.6f}, "
          f"oracle NaN curvatures {int(np.isnan(ev[:, 4]).sum())}, gpu {int(np.isnan(g[:, 4]).sum())}, "
          f"(tile_deferred, far_queries) = {deferred}")
    # curvature and direction are rounding noise on both sides: only min_value and |n| are gated
    assert np.all(np.abs(g[:, 3].astype(np.float64) - ev[:, 3]) <= 1e-6 * np.maximum(1.0, np.abs(ev[:, 3])))
    en = np.linalg.norm(ev[:, :3], axis=1)
    nz = np.isfinite(en) & (en > 0)
    assert nz.any()
    assert np.all(np.abs(np.linalg.norm(g[nz, :3].astype(np.float64), axis=1) - 1.0) <= 1e-6)


def test_degenerate_coincident(ctx):
    """50 distinct points, 40 copies of each: every 20-neighbourhood is one point, zero scatter."""
    rng = np.random.default_rng(7)
    xyz = np.repeat(rng.uniform(-5, 5, (50, 3)), 40, 0)[rng.permutation(2000)]
    _degenerate(ctx, xyz, 20, "coincident k=20")


def test_degenerate_collinear(ctx):
    """200 exactly collinear points (dyadic steps): two zero eigenvalues."""
    xyz = np.outer(np.arange(200) * 0.125, [1.0, 2.0, -0.5]) + [3.0, 1.0, 2.0]
    _degenerate(ctx, xyz, 8, "collinear k=8")
