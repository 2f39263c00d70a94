#!/usr/bin/env python3
"""CPU fp64 comparison of the two trims of the point-to-plane ICP on the cluttered street scene (the
table of DESIGN.md 5.1c and the figure tests/test_gpu_icp_rtrim.py holds the GPU to): the point trim
(pcp_icp_trim_keys, ranks the pairs by their squared point distance) against the residual trim
(pcp_icp_trim_keys_plane, ranks them by their squared plane residual), at two clutter shares and two
motions, with the translation error after every iteration.  No GPU: exact nearest neighbours from
scipy, fp64 PCA normals over 16 neighbours, tests/icp_plane_ref.py for the accumulators and the
solve, tests/trim_ref.py and tests/rtrim_ref.py for the trims.

    python tools/rtrim_reference.py
"""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_plane_ref as ref  # noqa: E402
import rtrim_ref  # noqa: E402
import trim_ref  # noqa: E402
from pointcloudprocess_amd import synth  # noqa: E402

RMAX, ITERS = 0.5, 8
SHOWN = (1, 2, 3, 4, 6, 8)
MOTIONS = {
    "1.0/0.4/-0.3 deg, (0.15, -0.10, 0.05) m": ((1.0, 0.4, -0.3), (0.15, -0.10, 0.05)),
    "2.0/0.8/-0.6 deg, (0.30, -0.20, 0.10) m": ((2.0, 0.8, -0.6), (0.30, -0.20, 0.10)),
}
# (name, kind, frac, mult, d_floor)
RULES = (
    ("every pair", None, 0, 0, 0),
    ("point trim    frac 0.6 mult 1   floor 0.02", "point", 0.6, 1.0, 0.02),
    ("residual trim frac 0.5 mult 3   floor 0", "plane", 0.5, 3.0, 0.0),
    ("residual trim frac 0.5 mult 2.5 floor 0.01", "plane", 0.5, 2.5, 0.01),
)


def run(tree, tgt, nrm, q, T_true, rule, iters=ITERS):
    """Per iteration (translation error m, rotation error deg, pairs used, pairs kept by the trim)."""
    _, kind, frac, mult, d_floor = rule
    T = np.eye(4)
    rows = []
    for _ in range(iters):
        d, j = tree.query(ref.transform_f32(T, q).astype(np.float64))
        d2 = (d * d).astype(np.float32)
        keys = trim_ref.make_keys(d2.view(np.uint32), j)
        keys[d2 > np.float32(RMAX * RMAX)] = trim_ref.NO_KEY
        kept = 0
        if kind == "point":
            keys, stats = trim_ref.trim(keys, frac, mult, d_floor)
            kept = int(stats[1])
        elif kind == "plane":
            keys, stats = rtrim_ref.rtrim(T, q, keys, tgt, nrm, frac, mult, d_floor)
            kept = int(stats[1])
        acc, used = ref.accumulate(T, q, keys, tgt, nrm)
        T = ref.solve(acc) @ T
        ang, tr = ref.pose_error(T, T_true)
        rows.append((tr, ang, int(used.sum()), kept))
    return rows


def scene(motion, share, band=(0.15, 0.45)):
    """(target, fp64 normals, kd-tree, queries, T_true) of one table row group."""
    (dz, dx, dy), t = motion
    T_true = synth.rigid(dz, dx, dy, t=t)
    tgt, q = synth.icp_pair(30000, 8000, 11, 12, T_true, extent=(50.0, 50.0))
    tgt, q = tgt.numpy(), q.numpy()
    if share > 0:
        q = trim_ref.cluttered_queries(q, T_true, share, band)
    tree = cKDTree(tgt.astype(np.float64))
    _, nn = tree.query(tgt.astype(np.float64), k=16)
    P = tgt[nn].astype(np.float64)
    Cc = P - P.mean(1, keepdims=True)
    nrm = np.linalg.eigh(np.einsum("nki,nkj->nij", Cc, Cc))[1][:, :, 0].astype(np.float32)
    return tgt, nrm, tree, q, T_true


def main():
    names = list(MOTIONS)
    cases = ((0.25, names[0], RULES), (0.40, names[0], (RULES[1], RULES[3])), (0.25, names[1], (RULES[1], RULES[2])),
             (0.0, names[0], RULES[:1]))
    print(f"translation error in mm after iteration {', '.join(str(i) for i in SHOWN)}; rmax {RMAX}, from the identity")
    for share, mname, rules in cases:
        tgt, nrm, tree, q, T_true = scene(MOTIONS[mname], share)
        print(f"clutter {int(round(100 * share))} %, motion {mname}")
        for rule in rules:
            rows = run(tree, tgt, nrm, q, T_true, rule)
            errs = "  ".join(f"{rows[i - 1][0] * 1e3:7.2f}" for i in SHOWN)
            last = rows[-1]
            print(f"  {rule[0]:<44s} {errs}   ({last[1]:.4f} deg, {last[2]} used, {last[3]} kept)")


if __name__ == "__main__":
    main()
