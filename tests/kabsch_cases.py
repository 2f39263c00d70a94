"""The case list and the assertions of the Kabsch / Umeyama solve tests, shared by the host solve
(test_icp_solve.py) and the device solve (test_gpu_icp_solve_dev.py).  Every expectation comes from
kabsch_ref.solve on the pairs; the accumulators a solver reads are kabsch_ref's exact sums.

Tolerances.  The fixed host build (g++ -O2 through hipcc) measured, over the cases below:
  orthonormality  max |R^T R - I|, |det R - 1|                      8.3e-16  (3.7 eps)
  tol_c           (cost - cost_ref) / (var_q + var_p)               4.3e-17  (0.2 eps)
  tol_u           |dT - dT_ref| (s1 + det s2) / (eps max|acc[7:16]|)   26.4
  tol_s           |sc / sc_ref - 1| (s0 + s1 + det s2) / (eps max|acc[7:22]|)  3.0
and each bound below is 16 times its figure, the margin for compiler and FMA differences between
builds (host and device compilers, sqrt and division sequences).
"""
import numpy as np

import kabsch_ref as kr

EPS = 2.0 ** -52
MARGIN = 16.0
TOL_ORTHO = MARGIN * 8.3e-16
TOL_C = MARGIN * 4.3e-17
TOL_U = MARGIN * 26.4
TOL_S = MARGIN * 3.0

PCP_OK, PCP_ERR_ICP = 0, -6

# the cases whose minimiser is not unique, so (c) has nothing to compare: rank <= 1, and a
# reflection with s1 == s2
NON_UNIQUE = ["collinear", "mirror_octahedron", "rank0_one_target", "rank0_one_query", "rank0_noise"]
RANK0_EXACT = ["rank0_one_target", "rank0_one_query"]
RANK0_NOISE = ["rank0_noise"]


def rot(axis, angle):
    """Rodrigues; exactly 2 a a^T - I at pi."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    if angle == np.pi:
        return 2.0 * np.outer(a, a) - np.eye(3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


ROT90Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
OCTA = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def cases():
    """[(name, q, p, do_scale)]"""
    rng = np.random.default_rng(2024)
    cloud = rng.normal(size=(200, 3)) * [3.0, 2.0, 1.0] + [1.0, -2.0, 0.5]
    t = np.array([0.3, -0.2, 0.1])
    out = []

    def moved(q, R, t=t, sc=1.0):
        return sc * q @ R.T + t

    for aname, axis in (("z", (0, 0, 1)), ("123", (1, 2, 3))):
        for rname, ang in (("0.05rad", 0.05), ("90deg", np.pi / 2), ("179deg", np.deg2rad(179.0)), ("180deg", np.pi)):
            R = ROT90Z if (aname, rname) == ("z", "90deg") else rot(axis, ang)
            out.append((f"rot_{rname}_{aname}", cloud, moved(cloud, R), False))
    Rs = rot((1, 2, 3), 0.05)
    plane = np.concatenate([rng.uniform(-5, 5, (100, 2)), np.zeros((100, 1))], 1)
    out.append(("planar", plane, moved(plane, Rs), False))
    off = plane + [100.0, 200.0, 5.0]
    out.append(("planar_offset", off, moved(off, Rs), False))
    line = rng.uniform(-5, 5, (50, 1)) * (np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))
    out.append(("collinear", line, moved(line, Rs), False))
    tri = np.array([[0.0, 0.0, 0.0], [2.0, 0.5, 0.0], [-0.5, 1.5, 1.0]])
    out.append(("three_pairs", tri, moved(tri, Rs), False))
    out.append(("octahedron", OCTA, moved(OCTA, rot((1, 2, 3), 0.7)), False))
    M = np.diag([1.0, 1.0, -1.0])
    mir = moved(cloud @ M, Rs)
    out.append(("mirror", cloud, mir, False))
    out.append(("mirror_noise", cloud, mir + rng.normal(scale=0.01, size=mir.shape), False))
    out.append(("mirror_octahedron", OCTA, moved(OCTA @ M, rot((1, 2, 3), 0.7)), False))
    out.append(("scale_0.5", cloud, moved(cloud, Rs, sc=0.5), True))
    out.append(("scale_2", cloud, moved(cloud, Rs, sc=2.0), True))
    out.append(("scale_1", cloud, moved(cloud, Rs), True))
    out.append(("mirror_scale", cloud, mir, True))
    out.append(("mirror_noise_scale", cloud, mir + rng.normal(scale=0.01, size=mir.shape), True))
    # rank 0: every pair at one target point / every query at one point (sums exact), and 500
    # random queries against one target point (S is the accumulators' rounding noise)
    four = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 1.0]])
    out.append(("rank0_one_target", four, np.zeros((4, 3)), False))
    out.append(("rank0_one_query", np.tile([2.0, -1.0, 0.5], (4, 1)), four, False))
    out.append(("rank0_noise", rng.normal(size=(500, 3)), np.tile([0.3, -1.7, 2.9], (500, 1)), False))
    return out


def bad_accumulators():
    """[(name, acc24)]: every one must be refused with PCP_ERR_ICP."""
    rng = np.random.default_rng(5)
    q = rng.normal(size=(50, 3))
    good = kr.acc24(q, q @ rot((1, 2, 3), 0.05).T + 0.1)
    out = [("n0", np.zeros(24)), ("n2", kr.acc24(q[:2], q[:2] + 0.1))]
    a = good.copy()
    a[0] = 2.999
    out.append(("n2.999", a))
    for k in range(23):  # n, A, B, AB, AA, D: every accumulator of every group
        for vname, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
            a = good.copy()
            a[k] = v
            out.append((f"acc{k}_{vname}", a))
    return out


def scale_of(dT):
    return float(np.sqrt(np.trace(dT[:3, :3].T @ dT[:3, :3]) / 3.0))


def check_solution(name, q, p, do_scale, dT, measured=None):
    """Assertions (a), (b), (c) of one solved case against kabsch_ref.solve; returns True when (c)
    ran.  `measured` (a dict of lists) collects the figures behind the tolerances."""
    ref = kr.solve(q, p, do_scale)
    acc = kr.acc24(q, p)
    dT = np.asarray(dT, dtype=np.float64).reshape(4, 4)
    assert np.array_equal(dT[3], [0.0, 0.0, 0.0, 1.0]), name
    # (a) a proper rotation times the reference's scale
    sc = scale_of(dT)
    assert sc > 0, f"{name}: singular dT {dT}"
    R = dT[:3, :3] / sc
    ortho = max(np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0))
    s, det = ref["s"], ref["det"]
    kappa_s = np.abs(acc[7:22]).max() / (s[0] + s[1] + det * s[2]) if do_scale else 0.0
    sc_err = abs(sc / ref["sc"] - 1.0)
    # (b) as good a fit as the reference's
    excess = (kr.cost(q, p, dT) - ref["cost"]) / (ref["var_q"] + ref["var_p"])
    # (c) the same motion, where there is one
    unique = name not in NON_UNIQUE
    du = np.abs(dT - ref["dT"]).max() * (s[1] + det * s[2]) / (EPS * np.abs(acc[7:16]).max()) if unique else 0.0
    if measured is not None:
        measured.setdefault("ortho", []).append((ortho, name))
        measured.setdefault("tol_c", []).append((excess, name))
        measured.setdefault("tol_u", []).append((du, name))
        if do_scale:
            measured.setdefault("tol_s", []).append((sc_err / (EPS * kappa_s), name))
    assert ortho <= TOL_ORTHO, f"{name}: R^T R - I or det R - 1 = {ortho:.3g}"
    if do_scale:
        assert sc_err <= TOL_S * EPS * kappa_s, f"{name}: scale {sc} vs {ref['sc']}"
    else:
        assert abs(sc - 1.0) <= TOL_ORTHO, f"{name}: scale {sc} without do_scale"
    assert excess <= TOL_C, f"{name}: cost above the reference's by {excess:.3g} of the variances"
    if unique:
        assert s[1] + det * s[2] > 0, name
        assert du <= TOL_U, f"{name}: |dT - dT_ref| = {np.abs(dT - ref['dT']).max():.3g} ({du:.3g} units)"
    return unique


def check_rank0(name, q, p, dT):
    """Rank 0: the identity rotation (exactly for exact sums), the centroids aligned."""
    dT = np.asarray(dT, dtype=np.float64).reshape(4, 4)
    q = np.asarray(q, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    if name in RANK0_EXACT:
        assert np.array_equal(dT[:3, :3], np.eye(3)), f"{name}: {dT}"
    else:
        assert np.abs(dT[:3, :3] - np.eye(3)).max() <= 1e-12, f"{name}: {dT}"
    qm, pm = kr.centre(q)[0], kr.centre(p)[0]  # the exact means, rounded once
    assert np.abs(dT[:3, 3] - (pm - qm)).max() <= 4 * EPS * max(np.abs(qm).max(), np.abs(pm).max()), f"{name}: {dT}"
