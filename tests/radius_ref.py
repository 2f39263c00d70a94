"""Exhaustive fp64 radius-search reference (plain numpy, no tree, no GPU).

TEST INFRASTRUCTURE ONLY.  The contract of pcp_radius_count / pcp_scan_counts / pcp_radius_fill
and of the oracle's KdTree.radius (KdTreeFLANN::radiusSearch, kd_tree.h:863-903), restated with
nothing to prune: every finite target's FLANN L2_Simple<double> distance (r = d0*d0; r += d1*d1;
r += d2*d2, each a separate rounded numpy operation, so no FMA); a target is a hit iff
d2 < r2 with r2 the single fp64 product r*r; rows ascending by (d2, original target index),
truncated to max_nn unless max_nn == 0 or max_nn >= the number of finite targets; a non-finite
query's row is empty.  With an `indices` subset the targets outside it do not exist; the subset
must ascend, so that FLANN's tie order (the position in the subset) is the original index order.
"""
import numpy as np

CHUNK = 256  # queries per distance matrix


class RadiusRef:
    """All distances of one (targets, queries) pair, each row sorted once by (d2, index): a row
    of any radius is a prefix of it, so every radius and max_nn of a case shares one sort."""

    def __init__(self, t, q, indices=None):
        t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
        q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
        if indices is None:
            cand = np.arange(len(t), dtype=np.int32)
        else:
            cand = np.asarray(indices, dtype=np.int32).reshape(-1)
            assert (np.diff(cand) > 0).all(), "indices must ascend"
        keep = cand[np.isfinite(t[cand]).all(1)]  # original indices, ascending
        tf = t[keep]
        self.size = len(keep)  # total_nr_points_
        self.nq = len(q)
        self.qfin = np.isfinite(q).all(1)
        self.idx = np.zeros((len(q), len(keep)), dtype=np.int32)
        self.d2 = np.full((len(q), len(keep)), np.inf, dtype=np.float64)
        for s in range(0, len(q), CHUNK):
            rows = s + np.flatnonzero(self.qfin[s:s + CHUNK])
            if len(rows) == 0 or len(keep) == 0:
                continue
            qq = q[rows]
            with np.errstate(over="ignore"):
                d0 = qq[:, 0:1] - tf[None, :, 0]
                d1 = qq[:, 1:2] - tf[None, :, 1]
                dz = qq[:, 2:3] - tf[None, :, 2]
                r = d0 * d0
                r = r + d1 * d1
                r = r + dz * dz
            order = np.argsort(r, axis=1, kind="stable")  # ties: ascending index
            self.idx[rows] = keep[order]
            self.d2[rows] = np.take_along_axis(r, order, 1)

    def r2(self, r):
        with np.errstate(over="ignore"):
            return np.float64(r) * np.float64(r)

    def counts(self, r, max_nn=0):
        """Row lengths (nq,) int64."""
        cnt = (self.d2 < self.r2(r)).sum(1).astype(np.int64)
        cnt[~self.qfin] = 0
        if max_nn != 0 and max_nn < self.size:
            cnt = np.minimum(cnt, max_nn)
        return cnt

    def rows(self, r, max_nn=0):
        """CSR (offsets int64 (nq+1), idx int32, d2 float64)."""
        cnt = self.counts(r, max_nn)
        offs = np.zeros(self.nq + 1, dtype=np.int64)
        np.cumsum(cnt, out=offs[1:])
        take = np.arange(self.d2.shape[1])[None, :] < cnt[:, None]
        return offs, self.idx[take], self.d2[take]

    def on_sphere(self, r):
        """(query, target) pairs with d2 == r*r exactly: the pairs a `<=` would add."""
        return int((self.d2[self.qfin] == self.r2(r)).sum())


def ref_radius(t, q, r, max_nn=0, indices=None):
    """CSR (offsets int64, idx int32, d2 float64) of one search, without keeping the distance
    matrix: for query sets as large as the cloud itself (the radius normals)."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    if indices is None:
        cand = np.arange(len(t), dtype=np.int32)
    else:
        cand = np.asarray(indices, dtype=np.int32).reshape(-1)
        assert (np.diff(cand) > 0).all(), "indices must ascend"
    keep = cand[np.isfinite(t[cand]).all(1)]
    tf = t[keep]
    with np.errstate(over="ignore"):
        r2 = np.float64(r) * np.float64(r)
    cap = len(keep) if (max_nn == 0 or max_nn >= len(keep)) else int(max_nn)
    qfin = np.isfinite(q).all(1)
    cnt = np.zeros(len(q), dtype=np.int64)
    idx, d2 = [np.zeros(0, np.int32)], [np.zeros(0)]
    for s in range(0, len(q), CHUNK):
        rows = s + np.flatnonzero(qfin[s:s + CHUNK])
        if len(rows) == 0 or len(keep) == 0:
            continue
        qq = q[rows]
        with np.errstate(over="ignore"):
            d0 = qq[:, 0:1] - tf[None, :, 0]
            d1 = qq[:, 1:2] - tf[None, :, 1]
            dz = qq[:, 2:3] - tf[None, :, 2]
            d = d0 * d0
            d = d + d1 * d1
            d = d + dz * dz
        hr, hc = np.nonzero(d < r2)
        hd = d[hr, hc]
        order = np.lexsort((hc, hd, hr))  # by row, then d2, then index
        hr, hc, hd = hr[order], hc[order], hd[order]
        start = np.searchsorted(hr, np.arange(len(rows)))
        take = np.arange(len(hr)) - start[hr] < cap
        cnt[rows] = np.bincount(hr[take], minlength=len(rows))
        idx.append(keep[hc[take]])
        d2.append(hd[take])
    offs = np.zeros(len(q) + 1, dtype=np.int64)
    np.cumsum(cnt, out=offs[1:])
    return offs, np.concatenate(idx).astype(np.int32), np.concatenate(d2)


def row(csr, i):
    offs, idx, d2 = csr
    return idx[offs[i]:offs[i + 1]], d2[offs[i]:offs[i + 1]]
