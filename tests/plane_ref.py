"""Independent plane reference for the PCA normals (TEST INFRASTRUCTURE ONLY, CPU).

No oracle import and none of its arithmetic: the mean and the centred scatter matrix are
accumulated in extended precision (np.longdouble), the eigen-decomposition is LAPACK's
(np.linalg.eigh), where the oracle and the kernels share one Jacobi and one summation
order.  The contract restated here is calculate_plan_parameter_h_points
(calculate_feature.cpp:119-206): normal = eigenvector of the smallest eigenvalue l3 of
sum (x - mean)(x - mean)^T, min_value = l3, curvature = l3 / (l1 + l2 + l3),
distance = -(float32(normal) . mean), sign: largest-|.| component positive, first wins.
"""
import numpy as np

FIELDS = ("normal_x", "normal_y", "normal_z", "min_value", "curvature", "distance")

# Gates of a float32 plane record against this reference, on rows with gap > GAP_MIN:
ANGLE_MAX = 2e-7        # rad; float32 rounding of a unit normal bounds it at sqrt(3) 2^-24 = 1.03e-7
CURV_MAX = 1e-7         # absolute; float32 rounding of a curvature <= 1/3 is <= 1.5e-8
L3_MAX = 1e-7           # relative to l1
DIST_MAX = 2.0 ** -23   # relative to max(1, |ref distance|)
GAP_MIN = 1e-3          # (l2 - l3) / l1 at or under this: the normal's direction is ill-conditioned


def plane_ref(nb):
    """Planes of an (m, k, 3) float64 array of neighbourhoods.  Returns a dict of per-row
    float64 arrays: normal (m, 3) unit, l1 >= l2 >= l3, curvature, distance, gap."""
    nb = np.asarray(nb, dtype=np.float64)
    assert nb.ndim == 3 and nb.shape[2] == 3
    x = nb.astype(np.longdouble)
    mean = x.sum(1) / np.longdouble(nb.shape[1])
    c = x - mean[:, None, :]
    S = np.empty((len(nb), 3, 3), np.longdouble)
    for a in range(3):
        for b in range(a, 3):
            S[:, a, b] = S[:, b, a] = (c[:, :, a] * c[:, :, b]).sum(1)
    w, v = np.linalg.eigh(S.astype(np.float64))  # ascending
    l3, l2, l1 = w[:, 0], w[:, 1], w[:, 2]
    n = v[:, :, 0].copy()
    big = np.argmax(np.abs(n), 1)  # first maximum wins
    flip = n[np.arange(len(n)), big] < 0
    n[flip] = -n[flip]
    n32 = n.astype(np.float32).astype(np.longdouble)
    dist = -(n32 * mean).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = l3 / (l1 + l2 + l3)
        gap = (l2 - l3) / l1
    return {"normal": n, "l1": l1, "l2": l2, "l3": l3, "curvature": curv,
            "distance": dist.astype(np.float64), "gap": gap}


def angle(a, b):
    """Unsigned angle between the lines spanned by a and b, (m, 3) each: atan2(|a x b|, |a . b|).
    (arccos of a float32 unit normal's dot product resolves nothing below ~3e-4 rad.)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


def as_rows(planes):
    """(m, 6) float64 view of plane records: a structured PLANE array or an (m, 6) array."""
    if getattr(planes.dtype, "names", None):
        return np.stack([planes[f] for f in FIELDS], 1).astype(np.float64)
    return np.asarray(planes, dtype=np.float64)


def measure(planes, ref):
    """Maxima of the four gated figures over the well-conditioned rows, plus the excluded share."""
    p = as_rows(planes)
    ok = ref["gap"] > GAP_MIN  # NaN gaps (zero scatter) compare false
    assert ok.any(), "no well-conditioned row"
    r = {k: v[ok] for k, v in ref.items()}
    p = p[ok]
    return {
        "rows": int(ok.sum()),
        "excluded": float(1.0 - ok.mean()),
        "angle": float(angle(p[:, :3], r["normal"]).max()),
        "curvature": float(np.abs(p[:, 4] - r["curvature"]).max()),
        "l3": float((np.abs(p[:, 3] - r["l3"]) / r["l1"]).max()),
        "distance": float((np.abs(p[:, 5] - r["distance"]) / np.maximum(1.0, np.abs(r["distance"]))).max()),
    }


def check(planes, ref, label, max_excluded):
    """Print the measured maxima, then assert the gates and the cap on excluded rows."""
    m = measure(planes, ref)
    print(f"{label}: rows {m['rows']} excluded {m['excluded']:.5f} angle {m['angle']:.3e} rad, "
          f"curvature {m['curvature']:.3e}, l3/l1 {m['l3']:.3e}, distance {m['distance']:.3e}")
    assert m["excluded"] <= max_excluded, (label, m)
    assert m["angle"] <= ANGLE_MAX, (label, m)
    assert m["curvature"] <= CURV_MAX, (label, m)
    assert m["l3"] <= L3_MAX, (label, m)
    assert m["distance"] <= DIST_MAX, (label, m)
    return m
