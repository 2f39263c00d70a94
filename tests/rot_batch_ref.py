"""Numpy reference of the staging around a batched get_rot_icp (include/pcp.h, V pcp_minmax_segments_aos48
and I5d), written from the contract text, not from the kernels:

  * the fp64 transform in the stated order ((r0 x + r1 y) + r2 z) + t -- numpy rounds every product and
    sum once and never contracts -- with a non-finite point of a non-dense cloud left as it is;
  * the float32 cast of the centred point, (float)(moved - c) per coordinate;
  * the un-centring t'_r = (t_r - rcv) + c_r with rcv = R_r0 c0; rcv += R_r1 c1; rcv += R_r2 c2;
  * the min / max rows of a moved segment (DBL_MAX / DBL_MIN starts, data[3] untransformed).

It also builds the scene of tests/test_gpu_rot_icp_batch.py (shared, read-only).
"""
import functools

import numpy as np

DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny
EPS = np.finfo(np.float64).eps
OFF = np.array([3512.25, -1801.5, 40.0])
SIZES = [0, 1, 2, 63, 64, 65, 1000, 3000]


def xform(T, xyz, dense=True):
    """transformPointCloud on (n, 3) fp64 rows."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(p)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            acc = T[r, 0] * p[:, 0]
            acc = acc + T[r, 1] * p[:, 1]
            acc = acc + T[r, 2] * p[:, 2]
            out[:, r] = acc + T[r, 3]
    if not dense:
        keep = ~np.isfinite(p).all(axis=1)
        out[keep] = p[keep]
    return out


def stage(T, xyz, c, dense=True):
    """(n, 3) float32: the centred fp32 image of a frame's points moved by T."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (xform(T, xyz, dense) - np.asarray(c, dtype=np.float64)[:3]).astype(np.float32)


def centre(xyz, c):
    """k_centre_f32 on the target: (float)(p - c)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(xyz, dtype=np.float64).reshape(-1, 3) - np.asarray(c, dtype=np.float64)[:3]).astype(np.float32)


def uncentre(T, c):
    """The 4x4 with t' = (t - R c) + c in pcp_get_rot_icp's operation order."""
    M = np.array(T, dtype=np.float64).reshape(4, 4)
    for r in range(3):
        rcv = M[r, 0] * c[0]
        rcv = rcv + M[r, 1] * c[1]
        rcv = rcv + M[r, 2] * c[2]
        M[r, 3] = (M[r, 3] - rcv) + c[r]
    return M


def uncentre_bound(T, c):
    """Per row 4 eps (|t| + sum |R_rk c_k| + |c_r|): four roundings of terms no larger than that sum."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    return np.array([4 * EPS * (abs(T[r, 3]) + sum(abs(T[r, k] * c[k]) for k in range(3)) + abs(c[r]))
                     for r in range(3)])


def minmax_rows(xyzw, T, dense=True):
    """(mn (4), mx (4)) of getMinMax3D(transformPointCloud(segment, T)); xyzw: (n, 4) fp64."""
    a = np.asarray(xyzw, dtype=np.float64).reshape(-1, 4)
    v = np.concatenate([xform(T, a[:, :3], dense), a[:, 3:]], axis=1)
    if not dense:
        v = v[np.isfinite(v[:, :3]).all(axis=1)]
    mn, mx = np.full(4, DBL_MAX), np.full(4, DBL_MIN)
    for k in range(4):
        col = v[:, k][~np.isnan(v[:, k])]
        if len(col):
            mn[k], mx[k] = min(mn[k], col.min()), max(mx[k], col.max())
    return mn, mx


def conj(T, off=OFF):
    """T about `off` instead of the origin: Tr(off) T Tr(-off)."""
    M = np.array(T, dtype=np.float64)
    M[:3, 3] = M[:3, 3] + off - M[:3, :3] @ off
    return M


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class Scene:
    pass


@functools.lru_cache(maxsize=None)
def scene():
    """The street scene (extent 50 m, 30 000 target points) at map coordinates OFF; eight frames of
    SIZES points, each its own street scene moved by the inverse of its own T_true (about OFF), and a
    different small start pose T0 per frame (about OFF): T0 undoes most of T_true, the registration
    finds the rest.  xyz are fp64 map coordinates."""
    from pointcloudprocess_amd import synth
    s = Scene()
    s.tgt = synth.street_scene(30000, 11, extent=(50.0, 50.0)).double().numpy() + OFF
    s.T_true, s.T0, segs = [], [], []
    for k, n in enumerate(SIZES):
        Tt = synth.rigid(0.8 - 0.2 * k, 0.3, -0.25 + 0.05 * k, t=(0.12, -0.09 + 0.02 * k, 0.04))
        T0 = synth.rigid(0.5 - 0.15 * k, 0.2, -0.1, t=(0.05, -0.04 + 0.01 * k, 0.02))
        own = synth.street_scene(n, 100 + k, extent=(50.0, 50.0)) if n else None
        segs.append(synth.apply_inverse(own, Tt).double().numpy() + OFF if n else np.zeros((0, 3)))
        s.T_true.append(conj(Tt))
        s.T0.append(conj(T0))
    s.T_true, s.T0 = np.stack(s.T_true), np.stack(s.T0)
    s.segs = segs
    s.off = offsets(SIZES)
    s.frames = np.concatenate(segs)
    for a in (s.tgt, s.T_true, s.T0, s.off, s.frames):
        a.setflags(write=False)
    return s


def rms_to_truth(final, T_true, xyz):
    """RMS over the points of |final p - T_true p|."""
    p = np.concatenate([np.asarray(xyz, dtype=np.float64), np.ones((len(xyz), 1))], axis=1)
    d = (p @ np.asarray(final).T - p @ np.asarray(T_true).T)[:, :3]
    return float(np.sqrt((d * d).sum(axis=1).mean()))
