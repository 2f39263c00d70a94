"""Exhaustive fp64 k-nearest-neighbour reference (plain numpy, no tree, no GPU).

TEST INFRASTRUCTURE ONLY.  The contract of pcp_knn / pcp_knn_bruteforce and of the oracle's
KdTree.knn, restated with nothing to prune and nothing to certify: every finite target's
FLANN L2_Simple<double> distance (r = d0*d0; r += d1*d1; r += d2*d2, each a separate rounded
numpy operation, so no FMA), rows ascending by (d2, original target index) -- or (d2, position in `order`) --, min(k, finite
targets) entries and -1 / +inf after them; a non-finite query's row is all -1 / +inf.
"""
import numpy as np

CHUNK = 256  # queries per distance matrix
KMAX = 32


def ref_knn(t, q, k, order=None):
    """(nq, k) int32 indices into t and (nq, k) float64 squared distances.

    order: the internal order of the targets, as original indices (an index built over an
    `indices` subset numbers its points by their position in it, non-finite rows dropped:
    kd_tree.h:928-997); ties then rank by that position.  Default: every row, ascending."""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    order = np.arange(len(t)) if order is None else np.asarray(order).reshape(-1)
    keep = order[np.isfinite(t[order]).all(1)].astype(np.int32)  # original indices, internal order
    tf = t[keep]
    kk = min(int(k), len(tf))
    idx = np.full((len(q), k), -1, dtype=np.int32)
    d2 = np.full((len(q), k), np.inf, dtype=np.float64)
    if kk == 0:
        return idx, d2
    qfin = np.isfinite(q).all(1)
    for s in range(0, len(q), CHUNK):
        rows = s + np.flatnonzero(qfin[s:s + CHUNK])
        if len(rows) == 0:
            continue
        qq = q[rows]
        d0 = qq[:, 0:1] - tf[None, :, 0]
        d1 = qq[:, 1:2] - tf[None, :, 1]
        dz = qq[:, 2:3] - tf[None, :, 2]
        r = d0 * d0
        r = r + d1 * d1
        r = r + dz * dz
        rank = np.argsort(r, axis=1, kind="stable")[:, :kk]  # ties: ascending internal position
        idx[rows, :kk] = keep[rank]
        d2[rows, :kk] = np.take_along_axis(r, rank, 1)
    return idx, d2


def prefix(ref, k):
    """The top-k of a case from its top-KMAX: (d2, index) is a total order, so the first k
    columns of a longer row are the shorter row, padding included."""
    idx, d2 = ref
    assert k <= idx.shape[1]
    return idx[:, :k], d2[:, :k]
