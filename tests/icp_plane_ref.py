"""Independent numpy fp64 reference of the point-to-plane ICP contract (include/pcp.h, I2),
written from the contract text, not from the kernel:

  * q' = R q + t with the pose cast to fp32 and the fp32 fmaf chain
    x = fma(R02, qz, fma(R01, qy, fma(R00, qx, t0))) (likewise y, z).  Each fma is emulated as
    the float64 multiply-add cast to float32; the float64 sum is first rounded to odd (TwoSum),
    so that the cast cannot round twice and the emulation is exact, not merely almost always;
  * a query counts when its key is not INT64_MAX, its index j = key & 0xffffffff is inside the
    table and record j is valid (fp32 |n|^2 >= 0.25, finite point and normal);
  * c = q' x n, r = n . (q' - p), J = (c, n) in float64, and the 30 sums;
  * the solve through numpy.linalg.solve on the normal equations and Rodrigues' formula.
"""
import numpy as np

NO_KEY = np.iinfo(np.int64).max
NACC = 30


def _fma32(a, b, c):
    """float32 fma(a, b, c), exactly: a * b is exact in float64; the sum is rounded to odd."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # TwoSum: p + c = s + e exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def transform_f32(T, q):
    """(n, 3) float32 q' under the 4x4 float64 pose T, by the contract's fmaf chain."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    R = T[:3, :3].astype(np.float32)
    t = T[:3, 3].astype(np.float32)
    q = np.asarray(q, dtype=np.float32)
    out = np.empty((q.shape[0], 3), dtype=np.float32)
    for r in range(3):
        full = lambda v: np.full(q.shape[0], v, dtype=np.float32)
        acc = _fma32(full(R[r, 0]), q[:, 0], full(t[r]))
        acc = _fma32(full(R[r, 1]), q[:, 1], acc)
        out[:, r] = _fma32(full(R[r, 2]), q[:, 2], acc)
    return out


def valid_records(points, normals):
    """Per record: usable normal (fp32 |n|^2 >= 0.25; a NaN fails) and finite point / normal."""
    p = np.asarray(points, dtype=np.float32)
    n = np.asarray(normals, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = n2 >= np.float32(0.25)
    return ok & np.isfinite(p).all(1) & np.isfinite(n).all(1)


def accumulate(T, q, keys, points, normals):
    """The 30 accumulators and the boolean mask of the queries used.  keys: int64/uint64 (nq);
    points / normals: (n, 3) float32 of the table (normals: the first 3 columns are read)."""
    keys = np.asarray(keys).astype(np.uint64)
    points = np.asarray(points, dtype=np.float32)[:, :3]
    normals = np.asarray(normals, dtype=np.float32)[:, :3]
    nrec = points.shape[0]
    j = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    used = (keys != np.uint64(NO_KEY)) & (j < nrec)
    ok = valid_records(points, normals)
    used[used] = ok[j[used]]
    acc = np.zeros(NACC)
    if not used.any():
        return acc, used
    qt = transform_f32(T, np.asarray(q, dtype=np.float32)[:, :3])[used].astype(np.float64)
    ju = j[used]
    p = points[ju].astype(np.float64)
    n = normals[ju].astype(np.float64)
    c = np.cross(qt, n)
    r = (n * (qt - p)).sum(1)
    J = np.concatenate([c, n], axis=1)
    acc[0] = used.sum()
    k = 1
    for a in range(6):
        for b in range(a, 6):
            acc[k] = (J[:, a] * J[:, b]).sum()
            k += 1
    acc[22:28] = (r[:, None] * J).sum(0)
    acc[28] = (r * r).sum()
    d2 = (keys[used] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    acc[29] = d2.astype(np.float64).sum()
    return acc, used


def system(acc):
    """(A 6x6, b 6) of the accumulators."""
    A = np.zeros((6, 6))
    k = 1
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = acc[k]
            k += 1
    return A, np.asarray(acc[22:28], dtype=np.float64)


def rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / th ** 2) * (K @ K)


def solve(acc):
    """dT (4x4) minimising sum (r + J . x)^2: A x = -b, R = exp([w]x), t."""
    A, b = system(acc)
    x = np.linalg.solve(A, -b)
    dT = np.eye(4)
    dT[:3, :3] = rodrigues(x[:3])
    dT[:3, 3] = x[3:]
    return dT


def min_pivot(acc):
    """Smallest LDL^T pivot of the contract's scaled system, as ratios of leading principal
    minors (d_k = det A_k / det A_{k-1}): rotation unknowns scaled by the RMS lever arm, the
    matrix divided by its largest diagonal entry."""
    A, _ = system(acc)
    s = np.sqrt(np.trace(A[:3, :3]) / np.trace(A[3:, 3:]))
    D = np.diag([1 / s] * 3 + [1.0] * 3)
    A = D @ A @ D
    A = A / A.diagonal().max()
    piv, prev = [], 1.0
    for k in range(1, 7):
        d = np.linalg.det(A[:k, :k])
        piv.append(d / prev)
        if not piv[-1] > 0.0:  # the factorisation stops at the first pivot that is not positive
            break
        prev = d
    return min(piv)


def acc_from_pairs(q, p, n, d2=None):
    """Accumulators of explicit float64 pairs (q' already transformed) -- the CPU solve tests."""
    q, p, n = (np.asarray(v, dtype=np.float64) for v in (q, p, n))
    c = np.cross(q, n)
    r = (n * (q - p)).sum(1)
    J = np.concatenate([c, n], axis=1)
    acc = np.zeros(NACC)
    acc[0] = len(q)
    k = 1
    for a in range(6):
        for b in range(a, 6):
            acc[k] = (J[:, a] * J[:, b]).sum()
            k += 1
    acc[22:28] = (r[:, None] * J).sum(0)
    acc[28] = (r * r).sum()
    acc[29] = ((q - p) ** 2).sum() if d2 is None else np.sum(d2)
    return acc


def pose_error(T, T_true):
    """(rotation error in degrees, translation error in metres) of T against T_true."""
    dR = T[:3, :3] @ T_true[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return ang, float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
