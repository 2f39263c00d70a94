"""CPU checks of the point-to-plane ICP solve (pcp_icp_solve_plane, host only; libpcp.so loads
without a GPU) against tests/icp_plane_ref.py: a well-posed system, the numerically singular
systems the solve must refuse, the thin but determined systems its pivot threshold must NOT
refuse, and null arguments."""
import ctypes as C

import numpy as np
import pytest

import icp_plane_ref as ref

PCP_ERR_ARG, PCP_ERR_ICP = -1, -6


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _on_plane(rng, n, normal, offset, half=25.0):
    """n points of the plane normal . x = offset, spread over +-half metres."""
    normal = _unit(normal)
    a = _unit(np.cross(normal, [0.3, -0.5, 0.8]))
    b = np.cross(normal, a)
    uv = rng.uniform(-half, half, size=(n, 2))
    return uv[:, :1] * a + uv[:, 1:] * b + offset * normal


def _moved(p, w, t):
    """q' with p = exp([w]x) q' + t: the motion the solve should (to first order) find."""
    return (p - np.asarray(t)) @ ref.rodrigues(np.asarray(w, dtype=np.float64))


def _solve(acc):
    from pointcloudprocess_amd import ops
    return ops.icp_solve_plane(acc)


def _three_planes(rng, per_plane):
    normals = [_unit([0.0, 0.0, 1.0]), _unit([1.0, 0.1, 0.0]), _unit([0.6, 0.8, 0.1])]
    p = np.concatenate([_on_plane(rng, per_plane, nn, off) for nn, off in zip(normals, (0.0, 12.0, -7.0))])
    n = np.concatenate([np.tile(nn, (per_plane, 1)) for nn in normals])
    return p, n


def test_well_posed_solve_matches_reference():
    rng = np.random.default_rng(1)
    p, n = _three_planes(rng, 1667)
    p, n = p[:5000], n[:5000]
    w, t = np.radians([0.05, -0.03, 0.08]), np.array([0.04, -0.03, 0.02])
    acc = ref.acc_from_pairs(_moved(p, w, t), p, n)
    rc, dT = _solve(acc)
    assert rc == 0
    assert np.abs(dT - ref.solve(acc)).max() < 1e-9
    R = dT[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    assert np.array_equal(dT[3], [0.0, 0.0, 0.0, 1.0])
    # and it is the motion that was applied, to the linearisation's second order
    assert np.abs(dT[:3, :3] - ref.rodrigues(w)).max() < 1e-5 and np.abs(dT[:3, 3] - t).max() < 1e-3


def test_large_rotation_is_rigid():
    """Rodrigues away from the small-angle series: a solution of ~0.3 rad is still orthonormal."""
    rng = np.random.default_rng(2)
    p, n = _three_planes(rng, 400)
    acc = ref.acc_from_pairs(_moved(p, [0.2, -0.15, 0.1], [0.5, 0.2, -0.3]), p, n)
    rc, dT = _solve(acc)
    assert rc == 0
    assert np.abs(dT - ref.solve(acc)).max() < 1e-9
    assert np.abs(dT[:3, :3] @ dT[:3, :3].T - np.eye(3)).max() < 1e-14
    assert abs(np.linalg.det(dT[:3, :3]) - 1.0) < 1e-14


def _singular_cases():
    rng = np.random.default_rng(3)
    cases = {}
    # five pairs of a perfectly good geometry: fewer than the six unknowns
    p, n = _three_planes(rng, 2)
    cases["n=5"] = ref.acc_from_pairs(_moved(p[:5], [0.001, 0.0, 0.0], [0.01, 0.0, 0.0]), p[:5], n[:5])
    # an exact plane z = 0: in-plane translations and the rotation about z are free
    p = _on_plane(rng, 2000, [0, 0, 1], 0.0)
    nz = np.tile([0.0, 0.0, 1.0], (len(p), 1))
    cases["plane z=0"] = ref.acc_from_pairs(p + [0.01, 0.02, 0.03], p, nz)
    # a tilted plane whose normal went through fp32: the free motions stay free
    nt = _unit([0.3, 0.2, 0.93]).astype(np.float32).astype(np.float64)
    p = _on_plane(rng, 2000, nt, 3.0)
    cases["tilted plane, fp32 normal"] = ref.acc_from_pairs(p + 0.02 * nt, p, np.tile(nt, (len(p), 1)))
    # two orthogonal planes: the translation along their common line is free
    pa, pb = _on_plane(rng, 1000, [0, 0, 1], 0.0), _on_plane(rng, 1000, [1, 0, 0], 0.0)
    n2 = np.concatenate([np.tile([0.0, 0.0, 1.0], (1000, 1)), np.tile([1.0, 0.0, 0.0], (1000, 1))])
    p = np.concatenate([pa, pb])
    cases["two orthogonal planes"] = ref.acc_from_pairs(p + [0.01, 0.0, 0.02], p, n2)
    return cases


@pytest.mark.parametrize("name", ["n=5", "plane z=0", "tilted plane, fp32 normal", "two orthogonal planes"])
def test_singular_systems_fail(name):
    acc = _singular_cases()[name]
    if name != "n=5":
        assert ref.min_pivot(acc) < 1e-10  # the reference agrees that this one is singular
    rc, dT = _solve(acc)
    assert rc == PCP_ERR_ICP
    assert np.array_equal(dT, np.eye(4))


def _six_points():
    """Two points on each of three orthogonal planes: exactly as many pairs as unknowns."""
    p = np.array([[1.0, 2.0, 0.0], [-2.0, 1.0, 0.0], [0.0, 1.0, 2.0], [0.0, -2.0, 1.0], [2.0, 0.0, 1.0],
                  [1.0, 0.0, -2.0]])
    n = np.array([[0.0, 0.0, 1.0]] * 2 + [[1.0, 0.0, 0.0]] * 2 + [[0.0, 1.0, 0.0]] * 2)
    return p, n


def _noisy_ground(rng, m=3000, k=16):
    """Ground z = N(0, 1 cm) over 50 m x 50 m with PCA normals over the k nearest neighbours
    (fp32, as the table stores them): only the noise in the normals determines the in-plane
    motions, so this system is thin -- and must still be solved."""
    p = np.column_stack([rng.uniform(-25, 25, m), rng.uniform(-25, 25, m), rng.normal(0, 0.01, m)])
    d2 = ((p[:, None, :2] - p[None, :, :2]) ** 2).sum(-1) + (p[:, None, 2] - p[None, :, 2]) ** 2
    nb = np.argpartition(d2, k, axis=1)[:, :k]
    nbr = p[nb]
    cov = np.einsum("mki,mkj->mij", nbr - nbr.mean(1, keepdims=True), nbr - nbr.mean(1, keepdims=True))
    n = np.linalg.eigh(cov)[1][:, :, 0]
    return p, n.astype(np.float32).astype(np.float64)


def test_thin_systems_are_solved():
    rng = np.random.default_rng(4)
    p, n = _six_points()
    acc = ref.acc_from_pairs(_moved(p, [0.002, -0.001, 0.003], [0.01, -0.02, 0.015]), p, n)
    assert ref.min_pivot(acc) > 1e-3
    rc, dT = _solve(acc)
    assert rc == 0
    assert np.abs(dT - ref.solve(acc)).max() < 1e-9
    p, n = _noisy_ground(rng)
    acc = ref.acc_from_pairs(_moved(p, [0.0005, -0.0004, 0.001], [0.03, -0.02, 0.01]), p, n)
    mp = ref.min_pivot(acc)
    assert 1e-8 < mp < 1e-2, mp  # thin, yet four orders of magnitude above the threshold
    rc, dT = _solve(acc)
    assert rc == 0
    # both solvers are backward stable: they differ by ~eps * cond <= 2e-16 * 6 / min pivot
    # relative to |x| <= 1 (the in-plane motions of a thin system are large but bounded here)
    assert np.abs(dT - ref.solve(acc)).max() < 1e3 * 2.2e-16 * 6.0 / mp


def test_null_arguments():
    from pointcloudprocess_amd import _lib
    lib = _lib.load()
    acc = (C.c_double * 30)()
    dT = (C.c_double * 16)()
    assert lib.pcp_icp_solve_plane(None, dT) == PCP_ERR_ARG
    assert lib.pcp_icp_solve_plane(acc, None) == PCP_ERR_ARG
    assert lib.pcp_icp_planes_destroy(None) == PCP_ERR_ARG
    assert lib.pcp_icp_planes_size(None) == -1
    assert lib.pcp_icp_planes_valid(None) == -1
    h = C.c_void_p()
    assert lib.pcp_icp_planes_create(None, None, 12, None, 12, 0, C.byref(h)) == PCP_ERR_ARG
    assert lib.pcp_icp_accumulate_plane(None, None, None, 12, 0, None, None, None) == PCP_ERR_ARG
    assert lib.pcp_icp_solve_plane_dev(None, None, None, None) == PCP_ERR_ARG
    assert lib.pcp_icp_run_plane_dev(None, None, None, None, 12, 0, None, 0.5, 1, None) == PCP_ERR_ARG
    M = (C.c_double * 16)()
    err = C.c_float()
    assert lib.pcp_get_rot_icp_plane(None, None, 0, 1, None, 0, 1, M, 0.5, 1, 16, 0.0, C.byref(err)) == PCP_ERR_ARG


def test_all_zero_accumulators_fail():
    rc, dT = _solve(np.zeros(30))
    assert rc == PCP_ERR_ICP and np.array_equal(dT, np.eye(4))
