#!/usr/bin/env python3
"""CPU fp64 reference of the trimmed point-to-plane ICP on the cluttered street scene (the numbers
quoted in tests/test_gpu_icp_trim.py and DESIGN.md).  No GPU: exact nearest neighbours from scipy,
fp64 PCA normals over 16 neighbours, tests/icp_plane_ref.py for the accumulators and the solve,
tests/trim_ref.py for the trim.

    python tools/trim_reference.py [share lo hi]
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_plane_ref as ref  # noqa: E402
import trim_ref  # noqa: E402
from pointcloudprocess_amd import synth  # noqa: E402

RMAX, ITERS, FRAC, MULT, FLOOR = 0.5, 4, 0.6, 1.0, 0.02


def run(tree, tgt, nrm, q, T_true, trim):
    T = np.eye(4)
    kept = 0
    for _ in range(ITERS):
        d, j = tree.query(ref.transform_f32(T, q).astype(np.float64))
        d2 = (d * d).astype(np.float32)
        keys = trim_ref.make_keys(d2.view(np.uint32), j)
        keys[d2 > np.float32(RMAX * RMAX)] = trim_ref.NO_KEY
        if trim:
            keys, stats = trim_ref.trim(keys, FRAC, MULT, FLOOR)
            kept = int(stats[1])
        acc, used = ref.accumulate(T, q, keys, tgt, nrm)
        T = ref.solve(acc) @ T
    ang, tr = ref.pose_error(T, T_true)
    return ang, tr, int(used.sum()), kept


def main():
    share, lo, hi = (float(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (0.25, 0.15, 0.45)
    T_true = synth.rigid(1.0, 0.4, -0.3, t=(0.15, -0.10, 0.05))
    tgt, q = synth.icp_pair(30000, 8000, 11, 12, T_true, extent=(50.0, 50.0))
    tgt = tgt.numpy()
    q = trim_ref.cluttered_queries(q.numpy(), T_true, share, (lo, hi))
    tree = cKDTree(tgt.astype(np.float64))
    _, nn = tree.query(tgt.astype(np.float64), k=16)
    P = tgt[nn].astype(np.float64)
    Cc = P - P.mean(1, keepdims=True)
    nrm = np.linalg.eigh(np.einsum("nki,nkj->nij", Cc, Cc))[1][:, :, 0].astype(np.float32)
    print(f"clutter share {share}, z in [{lo}, {hi}]; rmax {RMAX}, {ITERS} iterations from the identity")
    a0, t0, u0, _ = run(tree, tgt, nrm, q, T_true, False)
    print(f"  every pair within rmax : {t0 * 1e3:.2f} mm  {a0:.4f} deg  ({u0} pairs in the last iteration)")
    a1, t1, u1, k1 = run(tree, tgt, nrm, q, T_true, True)
    print(f"  frac {FRAC} mult {MULT} floor {FLOOR}: {t1 * 1e3:.2f} mm  {a1:.4f} deg  ({k1} kept, {u1} used)")
    print(f"  ratio {t0 / t1:.2f}")


if __name__ == "__main__":
    main()
