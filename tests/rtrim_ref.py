"""Numpy reference of pcp_icp_trim_keys_plane (include/pcp.h, I3b), written from the contract text,
not from the kernels:

  * key i is usable when it is not INT64_MAX, its index j = key & 0xffffffff is inside the table,
    record j is valid (icp_plane_ref.valid_records) and its statistic rho_i is not NaN; m = number
    of usable keys;
  * q' = R q + t by the fp32 fmaf chain of the accumulation (icp_plane_ref.transform_f32); p, n and
    q' widened to float64; r = (nx (q'x - px) + ny (q'y - py)) + nz (q'z - pz) in float64 in that
    order (numpy rounds each operation and never contracts); rho = float32(r * r), b = its bits;
  * selection, cut and keep are trim_ref's (pcp_icp_trim_keys's rules) over the keys
    (b << 32 | low word) of the usable pairs;
  * a kept key is the INPUT key unchanged (its high word stays the point d2), every other key is
    INT64_MAX; stats = [m, kept, sel, bits of cut].
"""
import numpy as np

import icp_plane_ref as ref
import trim_ref

NO_KEY = trim_ref.NO_KEY
_ERR = dict(invalid="ignore", over="ignore", under="ignore")

# Figures printed by tools/rtrim_reference.py (fp64 CPU: exact neighbours, fp64 normals) for the
# cluttered street scene of the GPU tests -- 30000 / 8000 points, 25 % clutter, rmax 0.5, motion
# 1.0/0.4/-0.3 deg and (0.15, -0.10, 0.05) m -- after SCENE_ITERS iterations from the identity:
# the translation error of the residual trim with SCENE_RTRIM and of the point trim with
# SCENE_PTRIM (frac, mult, d_floor).  test_rtrim_ref.py re-derives them from the tool's output.
SCENE_ITERS = 6
SCENE_RTRIM = (0.5, 3.0, 0.0)
SCENE_PTRIM = (0.6, 1.0, 0.02)
REF_RTRIMMED_M = 1.21e-3
REF_POINT_TRIMMED_M = 6.87e-3


def residual_keys(T, q, keys, points, normals):
    """int64 (n): (bits of rho << 32) | low word of the key for a usable pair, else INT64_MAX."""
    keys = np.ascontiguousarray(np.asarray(keys).view(np.int64))
    points = np.asarray(points, dtype=np.float32)[:, :3]
    normals = np.asarray(normals, dtype=np.float32)[:, :3]
    q = np.asarray(q, dtype=np.float32)[:, :3]
    out = np.full(keys.shape[0], NO_KEY, dtype=np.int64)
    if keys.shape[0] == 0:
        return out
    low = keys.view(np.uint64) & np.uint64(0xFFFFFFFF)
    j = low.astype(np.int64)
    cand = (keys != NO_KEY) & (j < points.shape[0])
    ok = ref.valid_records(points, normals)
    cand[cand] = ok[j[cand]]
    if not cand.any():
        return out
    jc = j[cand]
    qt = ref.transform_f32(T, q)[cand].astype(np.float64)
    p = points[jc].astype(np.float64)
    n = normals[jc].astype(np.float64)
    with np.errstate(**_ERR):
        r = (n[:, 0] * (qt[:, 0] - p[:, 0]) + n[:, 1] * (qt[:, 1] - p[:, 1])) + n[:, 2] * (qt[:, 2] - p[:, 2])
        rho = (r * r).astype(np.float32)
    rk = trim_ref.make_keys(rho.view(np.uint32), low[cand])
    rk[np.isnan(rho)] = NO_KEY
    out[cand] = rk
    return out


def rtrim(T, q, keys, points, normals, frac, mult=1.0, d_floor=0.0):
    """(keys_out int64, stats uint64[4]) of the contract."""
    keys = np.ascontiguousarray(np.asarray(keys).view(np.int64))
    rk, stats = trim_ref.trim(residual_keys(T, q, keys, points, normals), frac, mult, d_floor)
    return np.where(rk != NO_KEY, keys, np.int64(NO_KEY)), stats
