"""Independent numpy reference of batched registration (include/pcp.h, I5), written from the
contract text, not from the kernels.

Keys, per segment s with its own pose T_s:
  * q' = R q + t by icp_plane_ref.transform_f32 (the pose cast to fp32, the fp32 fmaf chain);
  * d2(j) = fma(dz, dz, fma(dy, dy, dx * dx)) in fp32 with d = q' - p_j, through
    icp_plane_ref._fma32, against EVERY finite target point;
  * the winner is the lexicographic minimum of (d2, j); it is accepted iff d2 <= r2 with
    r2 = fp32(rmax) * fp32(rmax) rounded to fp32;
  * key = bits(d2) << 32 | j, or INT64_MAX for a non-finite query, a non-finite image, or nothing
    within rmax.

The minimum is exhaustive.  To keep it quick, each block of queries is first ranked against the
whole target by a plain fp32 d2a = dx*dx + dy*dy + dz*dz (three roundings more than the contract's
d2; both are within 4 ulp = 2.4e-7 relative of the exact real value).  With m the row minimum of
d2a, every target whose contract d2 equals the contract minimum d2* has
d2a <= d2* (1 + e) <= m (1 + e) / (1 - e), e = 2.4e-7, so the candidates d2a <= m * (1 + 1e-5) + 1e-30
contain every minimiser; the contract d2 is then evaluated on the candidates only and the
lexicographic minimum taken among them.  No grid, no pruning by distance to cells.

Accumulators and solve: icp_plane_ref.accumulate and icp_plane_ref.solve per segment.
"""
import numpy as np

import icp_plane_ref as ref

NO_KEY = ref.NO_KEY
MIN_PIVOT = 1e-10  # pcp.h I2: a pivot <= 1e-10 fails the solve


def r2_of(rmax):
    return np.float32(rmax) * np.float32(rmax)


def d2_f32(qt, p):
    """The contract's fp32 d2 of paired rows qt[i], p[i] ((n, 3) float32 each)."""
    d = qt.astype(np.float32) - p.astype(np.float32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return ref._fma32(dz, dz, ref._fma32(dy, dy, dx * dx))


def keys(T, q, target, rmax, block=512):
    """int64 keys of the queries q ((n, 3) float32) under the 4x4 pose T against target ((m, 3)
    float32, indexed by its row = caller index)."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    target = np.asarray(target, dtype=np.float32)[:, :3]
    out = np.full(q.shape[0], NO_KEY, dtype=np.int64)
    idx = np.nonzero(np.isfinite(target).all(1))[0]
    tp = np.ascontiguousarray(target[idx])
    if q.shape[0] == 0 or tp.shape[0] == 0:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        qt = ref.transform_f32(T, q)
    ok = np.isfinite(q).all(1) & np.isfinite(qt).all(1)
    rows = np.nonzero(ok)[0]
    r2 = r2_of(rmax)
    tx, ty, tz = (np.ascontiguousarray(tp[:, a]) for a in range(3))
    for b0 in range(0, len(rows), block):
        rb = rows[b0:b0 + block]
        qb = qt[rb]
        with np.errstate(over="ignore"):
            d = qb[:, 0:1] - tx[None, :]
            a = d * d
            d = qb[:, 1:2] - ty[None, :]
            a += d * d
            d = qb[:, 2:3] - tz[None, :]
            a += d * d
        m = a.min(axis=1)
        thr = (m.astype(np.float64) * (1.0 + 1e-5) + 1e-30)
        ri, ci = np.nonzero(a.astype(np.float64) <= thr[:, None])
        with np.errstate(over="ignore"):
            d2 = d2_f32(qb[ri], tp[ci])
        j = idx[ci]
        order = np.lexsort((j, d2, ri))  # by row, then d2, then caller index
        ri, d2, j = ri[order], d2[order], j[order]
        first = np.ones(len(ri), dtype=bool)
        first[1:] = ri[1:] != ri[:-1]
        ri, d2, j = ri[first], d2[first], j[first]
        acc = d2 <= r2
        k = (d2[acc].view(np.uint32).astype(np.uint64) << np.uint64(32)) | j[acc].astype(np.uint64)
        out[rb[ri[acc]]] = k.view(np.int64)
    return out


def batch_keys(Ts, q, seg_offsets, target, rmax):
    """Keys of every query in q's order: segment s = q[seg_offsets[s]:seg_offsets[s + 1]] under
    Ts[s]."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    Ts = np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4)
    out = np.full(q.shape[0], NO_KEY, dtype=np.int64)
    for s in range(len(seg_offsets) - 1):
        a, b = int(seg_offsets[s]), int(seg_offsets[s + 1])
        out[a:b] = keys(Ts[s], q[a:b], target, rmax)
    return out


def solvable(acc):
    """The contract's decision: fewer than 6 pairs, a zero trace or a pivot <= 1e-10 fails."""
    if not acc[0] >= 6:
        return False
    A, _ = ref.system(acc)
    if not (np.trace(A[:3, :3]) > 0 and np.trace(A[3:, 3:]) > 0):
        return False
    return bool(ref.min_pivot(acc) > MIN_PIVOT)


def batch_step(Ts, stats, q, seg_offsets, keys_, points, normals):
    """One iteration from the given keys: (acc (B, 30), new Ts (B, 4, 4), new stats (B, 4)).  A
    segment whose solve fails (or has failed: stats[s, 0] < 0) keeps its pose; a failure latches
    stats[s, 0] = -1 and leaves stats[s, 1:] as they were."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    Ts = np.array(Ts, dtype=np.float64).reshape(-1, 4, 4)
    stats = np.array(stats, dtype=np.float64).reshape(-1, 4)
    B = len(seg_offsets) - 1
    acc = np.zeros((B, ref.NACC))
    for s in range(B):
        a, b = int(seg_offsets[s]), int(seg_offsets[s + 1])
        acc[s], _ = ref.accumulate(Ts[s], q[a:b], keys_[a:b], points, normals)
        if stats[s, 0] < 0:
            continue
        if not solvable(acc[s]):
            stats[s, 0] = -1.0
            continue
        Ts[s] = ref.solve(acc[s]) @ Ts[s]
        stats[s, 1] = np.sqrt(acc[s, 29] / acc[s, 0])
        stats[s, 2] = np.sqrt(acc[s, 28] / acc[s, 0])
        stats[s, 3] += 1.0
    return acc, Ts, stats
