"""Independent reference for the robust RPCA normals, F3 (TEST INFRASTRUCTURE ONLY, CPU).

No oracle import and none of its arithmetic beyond what the contract itself fixes.  The
contract is the header comment of rpca.hip, restating calculate_plan_parameter_rpca
(calculate_feature.cpp:208-368) and compute_distance_from_point_to_plane
(extraction_tree.cpp:47-64):

* draws: the SplitMix64 finaliser of (seed, j, iteration, slot), modulo N;
* iteration count: float32 log10(1 - Pr) over float64 log10(1 - (1 - epi)^3), truncated;
* 3-point plane: here the normalised cross product in np.longdouble (the oracle and the
  kernel run their 3-point PCA); sign: largest-|.| component positive; the distance term
  is taken from the float32 normal;
* point-to-plane distance: float32 coordinates, coefficients and products, float64 sums
  ((f1 + f2) + f3) + f4, float32 sqrt of the float32 sum of squares, float32 result.  This
  part is restated float-exactly: at map-frame coordinates the float32 products carry
  decimetres of noise and that noise is what the contract ranks;
* h-subset: the hf = floor(2N/3) smallest distances in a stable order, their float32
  coordinates, plane_ref (extended-precision scatter, LAPACK eigh);
* winner: the smallest l3 over distinct subsets;
* median / MAD / Rz: index N/2 of the sorted values, MAD = float32(1.4826 x), Rz a float32
  quotient compared with 2.5, MAD == 0 keeps every neighbour;
* final plane: plane_ref over the kept neighbours' float64 coordinates when more than 3
  remain, else {0, 0, 0, 0, curvature 1}.

A row's outcome hangs on discrete decisions (which h points, which subset wins, which
neighbours are kept).  Each row therefore carries a decision margin, the smallest of
  1. d[hf] - d[hf-1] over the largest distance, in every iteration with three distinct draws,
  2. second-smallest minus smallest l3 over l1, among distinct subsets,
  3. min |Rz - 2.5| / 2.5,
  4. the winning plane's gap (l2 - l3) / l1,
and 0 when a drawn triple has zero area.  compare() lets a record disagree with this
reference only on rows whose margin is <= MARGIN_MAX, and only on EXCUSED_MAX of the rows.
Rows with N of 4 or 5 have 2- or 3-point subsets (l3 is rounding noise, the winner is not
predictable); check_small() checks what can be said about them.
"""
import itertools

import numpy as np

import plane_ref
from plane_ref import ANGLE_MAX, CURV_MAX, DIST_MAX, GAP_MIN

MARGIN_MAX = 1e-6     # a disagreeing row must have a decision margin at or under this
EXCUSED_MAX = 0.005   # share of the rows with N >= 6 that may disagree at all
N_MIN = 6             # rows below this are outside compare(), see check_small()

_M64 = (1 << 64) - 1
_F32, _F64, _LD = np.float32, np.float64, np.longdouble


def draw(seed, j, it, slot):
    """One draw, in Python integers masked to 64 bits."""
    ctr = ((j & 0xFFFFFFFF) << 32) | ((it & 0xFFFFFFFF) << 2) | slot
    z = ((seed & _M64) + 0x9E3779B97F4A7C15 * ctr + 0x632BE59BD9B4E019) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z >> 32


def draws(seed, j, iters):
    """(len(j), iters, 3) array of draw(seed, j, it, slot): the same integers in wrapping uint64."""
    u = np.uint64
    jj = (np.asarray(j, dtype=np.int64).astype(u) & u(0xFFFFFFFF))[:, None, None]
    it = np.arange(iters, dtype=u)[None, :, None]
    slot = np.arange(3, dtype=u)[None, None, :]
    ctr = (jj << u(32)) | (it << u(2)) | slot
    z = u(seed & _M64) + u(0x9E3779B97F4A7C15) * ctr + u(0x632BE59BD9B4E019)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    z = z ^ (z >> u(31))
    return z >> u(32)


def iterations(pr, epi):
    """compute_iteration_number; ValueError where the host entry refuses Pr / epi."""
    one = _F32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        num = _F64(np.log10(one - _F32(pr)))
        den = np.log10(_F64(1) - _F64(one - _F32(epi)) ** 3)
        itf = num / den
    if not (itf >= 0.0 and itf < 65536.0):
        raise ValueError(f"Pr {pr} / epi {epi} out of range")
    return int(itf)


def leading_run(knn):
    """N of each row: the length of its leading run of non-negative indices."""
    neg = np.asarray(knn) < 0
    return np.where(neg.any(1), neg.argmax(1), neg.shape[1])


def point_plane_distance(F, a, b, c, d):
    """extraction_tree.cpp:47-64 on float32 arrays: F (..., 3) against coefficients that
    broadcast over F[..., 0]."""
    assert F.dtype == _F32 and all(t.dtype == _F32 for t in (a, b, c, d))
    g = np.sqrt((a * a + b * b) + c * c)
    f1, f2, f3 = (a * F[..., 0]).astype(_F64), (b * F[..., 1]).astype(_F64), (c * F[..., 2]).astype(_F64)
    f = np.abs(((f1 + f2) + f3) + d.astype(_F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (f / g.astype(_F64)).astype(_F32)


def _canonical(n):
    """Largest-|.| component positive, first maximum wins; n is (..., 3)."""
    big = np.argmax(np.abs(n), -1)
    flip = np.take_along_axis(n, big[..., None], -1)[..., 0] < 0
    return np.where(flip[..., None], -n, n)


def _nan0(x):
    return np.where(np.isnan(x), 0.0, x)


def _group(P, j, iters, seed):
    """Rows of one N: P (R, N, 3) float64 neighbourhoods of points j."""
    R, N, _ = P.shape
    hf = int(2.0 / 3 * N)
    F = P.astype(_F32)
    ar = np.arange(R)
    res = {"default": np.ones(R, bool), "normal": np.zeros((R, 3)), "curvature": np.ones(R),
           "distance": np.zeros(R), "gap": np.full(R, np.nan), "margin": np.full(R, np.inf),
           "kept": np.zeros(R, np.int64)}
    if iters == 0:
        return res
    num = (draws(seed, j, iters) % np.uint64(N)).astype(np.intp)               # (R, iters, 3)
    ok = (num[..., 0] != num[..., 1]) & (num[..., 0] != num[..., 2]) & (num[..., 1] != num[..., 2])
    # ---- 3-point planes
    x = P[ar[:, None, None], num].astype(_LD)                                  # (R, iters, 3, 3)
    cr = np.cross(x[:, :, 1] - x[:, :, 0], x[:, :, 2] - x[:, :, 0])
    nrm = np.sqrt((cr * cr).sum(-1))
    flat = ok & (nrm == 0)
    ok &= ~flat
    with np.errstate(divide="ignore", invalid="ignore"):
        n3 = _canonical(np.where(ok[..., None], cr / nrm[..., None], _LD(0)))
    n3f = n3.astype(_F32)
    d3f = (-(n3f.astype(_LD) * (x.sum(2) / _LD(3))).sum(-1)).astype(_F32)
    # ---- distances, stable order, h-subsets
    D = point_plane_distance(F[:, None, :, :], n3f[..., 0:1], n3f[..., 1:2], n3f[..., 2:3], d3f[..., None])
    D = np.where(ok[..., None], D, _F32(0))                                    # (R, iters, N)
    order = np.argsort(D, axis=-1, kind="stable")
    ds = np.take_along_axis(D, order, -1).astype(_F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = _nan0((ds[..., hf] - ds[..., hf - 1]) / ds[..., -1])
    m1 = np.where(ok, m1, np.inf).min(1)
    sub = order[..., :hf]
    key = (np.int64(1) << sub.astype(np.int64)).sum(-1)
    pl = plane_ref.plane_ref(F[ar[:, None, None], sub].reshape(R * iters, hf, 3).astype(_F64))
    pl = {k: v.reshape((R, iters) + v.shape[1:]) for k, v in pl.items()}
    # ---- winner
    l3 = np.where(ok, pl["l3"], np.inf)
    win = np.argmin(l3, 1)
    has = ok.any(1)
    w = {k: v[ar, win] for k, v in pl.items()}
    others = np.where(ok & (key != key[ar, win][:, None]), l3, np.inf).min(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        m2 = _nan0((others - w["l3"]) / w["l1"])
    m4 = _nan0(w["gap"])
    wn = w["normal"].astype(_F32)
    wd = w["distance"].astype(_F32)
    # ---- median, MAD, Rz
    d = point_plane_distance(F, wn[:, None, 0], wn[:, None, 1], wn[:, None, 2], wd[:, None])   # (R, N)
    med = np.sort(d, 1)[:, N // 2]
    tm = np.abs(d - med[:, None])
    mad = (1.4826 * np.sort(tm, 1)[:, N // 2].astype(_F64)).astype(_F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rz = tm / mad[:, None]
        keep = (mad == 0)[:, None] | (rz < _F32(2.5))
        m3 = np.where(mad == 0, np.inf, _nan0(np.abs(rz.astype(_F64) - 2.5) / 2.5).min(1))
    cnt = np.where(has, keep.sum(1), 0)
    res["kept"] = cnt
    res["margin"] = np.where(has, np.minimum(np.minimum(m1, m2), np.minimum(m3, m4)), np.inf)
    res["margin"] = np.where(flat.any(1), 0.0, res["margin"])
    # ---- final plane over the kept neighbours, in neighbour order
    first = np.argsort(~keep, axis=1, kind="stable")
    for c in np.unique(cnt[cnt > 3]):
        r = np.flatnonzero(cnt == c)
        f = plane_ref.plane_ref(P[r[:, None], first[r, :c]])
        res["default"][r] = False
        for k in ("normal", "curvature", "distance", "gap"):
            res[k][r] = f[k]
    return res


def rpca_ref(xyz, knn, pr=0.99, epi=0.5, seed=0, rows=None, chunk=256):
    """Reference records of the points `rows` (all by default) of an (n, 3) float64 cloud with
    (n, k) kNN rows.  Returns a dict of per-row arrays: N, default (bool), normal (m, 3),
    curvature, distance, gap (of the final plane, NaN on default rows), margin, kept."""
    xyz = np.asarray(xyz, dtype=_F64)
    knn = np.asarray(knn)
    rows = np.arange(len(knn)) if rows is None else np.asarray(rows, dtype=np.int64)
    iters = iterations(pr, epi)
    m = len(rows)
    sub = knn[rows]
    N = leading_run(sub)
    out = {"N": N, "default": np.ones(m, bool), "normal": np.zeros((m, 3)), "curvature": np.ones(m),
           "distance": np.zeros(m), "gap": np.full(m, np.nan), "margin": np.full(m, np.inf),
           "kept": np.zeros(m, np.int64)}
    for n in np.unique(N[N > 3]):
        sel = np.flatnonzero(N == n)
        for lo in range(0, len(sel), chunk):
            s = sel[lo:lo + chunk]
            g = _group(xyz[sub[s, :n]], rows[s], iters, int(seed))
            for k, v in g.items():
                out[k][s] = v
    return out


# ---------------------------------------------------------------- comparing records

def record_fields(rec):
    """(normal (m, 3), distance, curvature, default) of LAS_POINT_PROPERTY records, float64."""
    nrm = np.stack([rec["normal_x"], rec["normal_y"], rec["normal_z"]], 1).astype(_F64)
    dist = rec["distance"].astype(_F64)
    curv = rec["curvature"].astype(_F64)
    default = (nrm == 0).all(1) & (dist == 0) & (curv == 1.0)
    return nrm, dist, curv, default


def _gates(nrm, dist, curv, ref):
    with np.errstate(invalid="ignore"):
        ang = plane_ref.angle(nrm, ref["normal"])
        dc = np.abs(curv - ref["curvature"])
        dd = np.abs(dist - ref["distance"]) / np.maximum(1.0, np.abs(ref["distance"]))
    return ang, dc, dd


def compare(rec, ref, label, expect_gated=True):
    """Records (of the same rows as ref) against the reference on rows with N >= N_MIN: agreement
    on default versus non-default, and plane_ref's gates where the final gap > GAP_MIN.  Prints
    the measured maxima and the excused share, then asserts: a disagreeing row has margin <=
    MARGIN_MAX, and such rows are at most EXCUSED_MAX of the rows compared."""
    nrm, dist, curv, rdef = record_fields(rec)
    assert len(rdef) == len(ref["N"])
    sel = ref["N"] >= N_MIN
    with np.errstate(invalid="ignore"):
        gated = sel & ~rdef & ~ref["default"] & (ref["gap"] > GAP_MIN)
    ang, dc, dd = _gates(nrm, dist, curv, ref)
    bad = gated & ~((ang <= ANGLE_MAX) & (dc <= CURV_MAX) & (dd <= DIST_MAX))
    disagree = sel & ((rdef != ref["default"]) | bad)
    unexcused = disagree & ~(ref["margin"] <= MARGIN_MAX)
    good = gated & ~disagree
    nsel = int(sel.sum())
    m = {"rows": nsel, "gated": int(gated.sum()), "default": int((sel & rdef).sum()),
         "excused": float(disagree.sum() / max(nsel, 1)), "unexcused": int(unexcused.sum()),
         "angle": float(ang[good].max()) if good.any() else 0.0,
         "curvature": float(dc[good].max()) if good.any() else 0.0,
         "distance": float(dd[good].max()) if good.any() else 0.0}
    print(f"{label}: rows {m['rows']} gated {m['gated']} default {m['default']} excused {m['excused']:.5f} "
          f"unexcused {m['unexcused']} angle {m['angle']:.3e} rad, curvature {m['curvature']:.3e}, "
          f"distance {m['distance']:.3e}")
    assert nsel > 0, (label, "no row with N >= 6")
    assert not expect_gated or m["gated"] > 0.5 * nsel, (label, m)
    assert m["unexcused"] == 0, (label, m, np.flatnonzero(unexcused)[:10], ref["margin"][unexcused][:10])
    assert m["excused"] <= EXCUSED_MAX, (label, m)
    return m


def check_small(rec, xyz, knn, label):
    """Rows with N of 4 or 5: a non-default record is, within the gates, plane_ref of one of the
    neighbour sets that can survive the Rz filter: all four points (N = 4); all five or one of
    the five 4-subsets (N = 5).  Rows where a candidate is ill-conditioned (gap <= GAP_MIN) and
    no well-conditioned one matches are counted, not judged.  Returns the counts."""
    xyz = np.asarray(xyz, dtype=_F64)
    nrm, dist, curv, rdef = record_fields(rec)
    N = leading_run(knn)
    out = {}
    for n in (4, 5):
        r = np.flatnonzero((N == n) & ~rdef)
        out[n] = {"rows": int((N == n).sum()), "non_default": len(r)}
        if not len(r):
            continue
        P = xyz[np.asarray(knn)[r, :n]]
        sets = [list(range(n))] + ([list(c) for c in itertools.combinations(range(5), 4)] if n == 5 else [])
        match = np.zeros(len(r), bool)
        ill = np.zeros(len(r), bool)
        best = np.full(len(r), np.inf)
        for s in sets:
            ref = plane_ref.plane_ref(P[:, s])
            ang, dc, dd = _gates(nrm[r], dist[r], curv[r], ref)
            with np.errstate(invalid="ignore"):
                well = ref["gap"] > GAP_MIN
            hit = well & (ang <= ANGLE_MAX) & (dc <= CURV_MAX) & (dd <= DIST_MAX)
            best = np.where(hit, np.minimum(best, ang), best)
            match |= hit
            ill |= ~well
        out[n].update(matched=int(match.sum()), unjudged=int((~match & ill).sum()),
                      angle=float(best[match].max()) if match.any() else 0.0)
        print(f"{label} N={n}: {out[n]}")
        assert (match | ill).all(), (label, n, r[~(match | ill)][:10])
        assert out[n]["unjudged"] <= 0.01 * len(r) + 1, (label, n, out[n])
    return out


# ---------------------------------------------------------------- inputs shared by the tests

def scene(n=1500, seed=0, outliers=0.05):
    """A small scene in a 2 x 2 x 1 box: a tilted noisy ground plane (60 %), a wall (25 %),
    clutter (15 %), and `outliers` of all points displaced by 5 cm-scale noise."""
    rng = np.random.default_rng(seed)
    ng, nw = n * 6 // 10, n // 4
    nc = n - ng - nw
    g = rng.uniform(-1, 1, (ng, 2))
    ground = np.c_[g, 0.05 * g[:, 0] - 0.03 * g[:, 1] + rng.normal(0, 2e-3, ng)]
    wall = np.c_[0.4 + rng.normal(0, 2e-3, nw), rng.uniform(-1, 1, nw), rng.uniform(0, 0.8, nw)]
    clutter = np.c_[rng.uniform(-1, 1, (nc, 2)), rng.uniform(0, 0.5, nc)]
    xyz = np.concatenate([ground, wall, clutter])[rng.permutation(n)]
    out = rng.choice(n, int(n * outliers), replace=False)
    xyz[out] += rng.normal(0, 0.05, (len(out), 3))
    return np.ascontiguousarray(xyz)


def lattice(side=30, lifted=60, seed=0):
    """side x side integer lattice at z = 0 with `lifted` points raised to z = 3: distances to a
    lattice plane are exact, so MAD == 0 wherever more than half a neighbourhood lies on it."""
    rng = np.random.default_rng(seed)
    a = np.arange(side, dtype=_F64)
    xyz = np.stack([np.repeat(a, side), np.tile(a, side), np.zeros(side * side)], 1)
    xyz[rng.choice(len(xyz), lifted, replace=False), 2] = 3.0
    return xyz


def mixed_rows(idx, seed=21):
    """Row j of (n, 20) kNN rows truncated to a random length in 0..20, -1 padded."""
    rng = np.random.default_rng(seed)
    length = rng.permutation(np.arange(len(idx)) % 21)  # every length on >= len // 21 rows
    out = idx.copy()
    out[np.arange(idx.shape[1])[None, :] >= length[:, None]] = -1
    return out, length
