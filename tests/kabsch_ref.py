"""A plain reference for the point-to-point ICP step (numpy and the standard library only).

It works from the pairs (query image q, target point p), never from the accumulators:

  exact_acc   the 23 Kabsch sums n, A = sum q, B = sum p, AB = sum q p^T (9, row-major),
              AA = sum q q^T (upper triangle 00 01 02 11 12 22), D = sum d2, computed exactly
              (Python integers over a common power-of-two denominator, or fractions.Fraction) and
              rounded once to float64; plus the bounds under which fp32 centred partial sums of
              the same pairs are exact in any order.
  correspond  the contract's correspondences by brute force: fp32 d2 =
              fmaf(dz, dz, fmaf(dy, dy, dx * dx)), the lexicographic (d2, index) winner, accepted
              iff d2 <= r2 with r2 = rmax * rmax in fp32 (icp_search.hpp, pcp.h).
  solve       the Kabsch / Umeyama minimiser from exactly centred pairs through numpy's SVD, its
              singular values and its cost.
"""
import math
from fractions import Fraction

import numpy as np

_TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _lattice_exponent(values):
    """Smallest k >= 0 with v * 2^k an integer for every v (finite floats)."""
    k = 0
    for v in values:
        den = float(v).as_integer_ratio()[1]
        k = max(k, den.bit_length() - 1)
    return k


def _sums(q, p, d):
    """The 23 sums of rows q[i], p[i] (3 numbers each) and d[i], in the numbers' own arithmetic."""
    zero = 0 * d[0] if len(d) else 0
    acc = [zero] * 23
    for qi, pi, di in zip(q, p, d):
        acc[0] += 1
        for c in range(3):
            acc[1 + c] += qi[c]
            acc[4 + c] += pi[c]
        for r in range(3):
            for c in range(3):
                acc[7 + 3 * r + c] += qi[r] * pi[c]
        for m, (r, c) in enumerate(_TRI):
            acc[16 + m] += qi[r] * qi[c]
        acc[22] += di
    return acc


def exact_acc(q_img, p, d2, centres=None, group=2048, method="int"):
    """(acc, info): the 23 sums of the pairs (q_img[i], p[i], d2[i]) as float64, each the exact sum
    rounded once, and the conditions under which a fp32 implementation is exact.

    method "int": every coordinate times 2^k (k = info["k"]), sums in Python integers; "fraction":
    fractions.Fraction of every value.  Both are exact, so they agree bit for bit.

    info (lengths in lattice steps h = 2^-k, products in h^2):
      k          the lattice exponent of the coordinates
      bound      an upper bound on |any partial sum| of the 23 values over any `group` pairs (or
                 all, when fewer) centred on any row of `centres` (default: the query images
                 themselves; pass every finite query image when unpaired queries can be a centre):
                 group * max(Dq * Dp, Dq^2, max d2, 1), Dq / Dp the largest |coordinate| of a
                 centred query / target.  Below 2^24 every such fp32 sum, product and fmaf is exact.
      bound64    n * (largest |coordinate|)^2: below 2^53 every un-centred fp64 term and every
                 partial sum of such terms is exact
      fp32       every coordinate and d2 is a fp32 value
      exact64    the 23 exact sums are float64 values (the rounding above did nothing)
    """
    q = np.asarray(q_img, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d2, dtype=np.float64).reshape(-1)
    n = q.shape[0]
    assert p.shape[0] == n and d.shape[0] == n
    assert np.isfinite(q).all() and np.isfinite(p).all() and np.isfinite(d).all()
    c = q if centres is None else np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    k = _lattice_exponent(np.concatenate([q.ravel(), p.ravel(), c.ravel()]).tolist())
    kd = max(2 * k, _lattice_exponent(d.tolist()))
    if method == "int":
        sh = 1 << k
        qi = [[int(Fraction(v) * sh) for v in row] for row in q.tolist()]  # v * 2^k is an integer
        pi = [[int(Fraction(v) * sh) for v in row] for row in p.tolist()]
        di = [int(Fraction(v) * (1 << kd)) for v in d.tolist()]
        s = _sums(qi, pi, di)
        den = [1] + [sh] * 6 + [sh * sh] * 15 + [1 << kd]
        exact = [Fraction(v, dn) for v, dn in zip(s, den)]
    elif method == "fraction":
        exact = _sums([[Fraction(v) for v in row] for row in q.tolist()],
                      [[Fraction(v) for v in row] for row in p.tolist()], [Fraction(v) for v in d.tolist()])
        exact = [Fraction(v) for v in exact]
    else:
        raise ValueError(method)
    acc = np.array([float(v) for v in exact], dtype=np.float64)  # Fraction -> float rounds correctly
    info = {"k": k, "fp32": bool((q == q.astype(np.float32)).all() and (p == p.astype(np.float32)).all() and
                                 (d == d.astype(np.float32)).all() and (c == c.astype(np.float32)).all()),
            "exact64": all(Fraction(float(v)) == v for v in exact)}
    if n:
        h = 2.0 ** -k
        allq = np.concatenate([q, c])
        dq = float((allq.max(0) - allq.min(0)).max()) / h
        dp = float(max((p.max(0) - c.min(0)).max(), (c.max(0) - p.min(0)).max())) / h
        g = min(group, n)
        info["bound"] = g * max(dq * max(dp, 0.0), dq * dq, float(d.max()) / (h * h), max(dp, 0.0), 1.0)
        info["bound64"] = n * (float(max(np.abs(allq).max(), np.abs(p).max())) / h) ** 2
    else:
        info["bound"] = info["bound64"] = 0.0
    return acc, info


def acc24(q_img, p, d2=None, method="int"):
    """The 24 accumulators a solve reads ([23], the fallback count, is 0); d2 defaults to the pairs'
    squared distances in float64 (a solve never reads it, the rms does)."""
    q = np.asarray(q_img, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    d = ((q - p) ** 2).sum(1) if d2 is None else d2
    out = np.zeros(24)
    out[:23] = exact_acc(q, p, d, method=method)[0]
    return out


def xform32(T, q):
    """The contract's image of q (n x 3 fp32) under the fp32 cast of T:
    x' = fmaf(R02, z, fmaf(R01, y, fmaf(R00, x, t0))).  (img, exact): the chain in float64 rounded
    to fp32 after every fmaf, and whether no rounding happened anywhere."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3].astype(np.float32).astype(np.float64)
    t = T[:3, 3].astype(np.float32).astype(np.float64)
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    acc = np.broadcast_to(t, q.shape).copy()
    exact = True
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            wide = R[:, c][None, :] * q[:, c][:, None] + acc  # the product of two fp32 is exact in fp64
            acc = wide.astype(np.float32).astype(np.float64)
            fin = np.isfinite(wide)
            exact = exact and bool((acc[fin] == wide[fin]).all())
    return acc.astype(np.float32), exact


def correspond(tgt, q_img, rmax, chunk=256):
    """(idx int32, d2 fp32, exact): per query image the lexicographic (d2, target index) minimum
    over every finite target point, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32; accepted iff
    d2 <= r2, r2 = rmax * rmax in fp32 (equality accepts); -1 / +inf for a rejected or non-finite
    query.  The fp32 operations are done in float64 and rounded to fp32 after each one; `exact`
    says that no such rounding changed a value (true on lattice inputs), so that the single
    rounding of a hardware fmaf and this emulation cannot differ."""
    tgt = np.asarray(tgt, dtype=np.float32)
    qi = np.asarray(q_img, dtype=np.float32)
    r2 = np.float32(rmax) * np.float32(rmax)
    n = qi.shape[0]
    idx = np.full(n, -1, np.int32)
    d2o = np.full(n, np.inf, np.float32)
    tfin = np.isfinite(tgt).all(1)
    t64 = tgt.astype(np.float64)
    exact = True

    def f32(x):
        nonlocal exact
        y = x.astype(np.float32).astype(np.float64)
        exact = exact and bool((y == x).all())
        return y

    if tgt.shape[0] == 0:
        return idx, d2o, exact
    for s in range(0, n, chunk):
        qq = qi[s:s + chunk]
        fin = np.isfinite(qq).all(1)
        if not fin.any():
            continue
        q64 = qq[fin].astype(np.float64)
        dx = f32(q64[:, None, 0] - t64[None, tfin, 0])
        dy = f32(q64[:, None, 1] - t64[None, tfin, 1])
        dz = f32(q64[:, None, 2] - t64[None, tfin, 2])
        d = f32(dz * dz + f32(dy * dy + f32(dx * dx)))
        full = np.full((q64.shape[0], tgt.shape[0]), np.inf)
        full[:, tfin] = d
        j = full.argmin(1)  # the first minimum: the lowest index among equal d2
        dj = full[np.arange(len(j)), j].astype(np.float32)
        ok = dj <= r2
        rows = np.flatnonzero(fin) + s
        idx[rows[ok]] = j[ok].astype(np.int32)
        d2o[rows[ok]] = dj[ok]
    return idx, d2o, exact


def centre(x):
    """(mean, x - mean): the exact mean and the exactly centred rows, each rounded once."""
    cols = [[Fraction(v) for v in x[:, c].tolist()] for c in range(3)]
    means = [sum(col, Fraction(0)) / len(col) for col in cols]
    xc = np.array([[float(v - m) for v in col] for col, m in zip(cols, means)]).T
    return np.array([float(m) for m in means]), xc


def cost(q, p, dT):
    """sum |M q + t - p|^2 for dT = [M t; 0 1], from exactly centred pairs (no cancellation of
    the coordinates' offset)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    dT = np.asarray(dT, dtype=np.float64).reshape(4, 4)
    qm, qc = centre(q)
    pm, pc = centre(p)
    M, t = dT[:3, :3], dT[:3, 3]
    r = qc @ M.T - pc + (M @ qm + t - pm)
    return math.fsum((r * r).ravel().tolist())


def solve(q, p, do_scale=False):
    """The least-squares similarity / rigid motion of the pairs: minimise sum |sc R q + t - p|^2.
    S = sum (q - qm)(p - pm)^T = U diag(s) V^T (numpy SVD), R = V diag(1, 1, det) U^T with
    det = det(V U^T), sc = (s0 + s1 + det s2) / sum |q - qm|^2 (1 without do_scale),
    t = pm - sc R qm.  Returns a dict: dT (4x4), R, t, sc, s (singular values, descending), det,
    cost, var_q = sum |q - qm|^2, var_p, qm, pm."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    qm, qc = centre(q)
    pm, pc = centre(p)
    S = np.array([[math.fsum((qc[:, a] * pc[:, b]).tolist()) for b in range(3)] for a in range(3)])
    U, s, Vt = np.linalg.svd(S)
    V = Vt.T
    det = 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0
    R = V @ np.diag([1.0, 1.0, det]) @ U.T
    var_q = math.fsum((qc * qc).ravel().tolist())
    var_p = math.fsum((pc * pc).ravel().tolist())
    sc = (s[0] + s[1] + det * s[2]) / var_q if do_scale and var_q > 0 else 1.0
    t = pm - sc * R @ qm
    dT = np.eye(4)
    dT[:3, :3] = sc * R
    dT[:3, 3] = t
    return {"dT": dT, "R": R, "t": t, "sc": sc, "s": s, "det": det, "cost": cost(q, p, dT),
            "var_q": var_q, "var_p": var_p, "qm": qm, "pm": pm}
