#!/usr/bin/env python3
"""CPU model of the look-ahead at an ICP handle's FIRST launch, on the setup of
tools/sim_icp_lookahead.py: a tile of the C4 bench scene (or the GPU tests' window), the oracle's
own registration poses, the octant block, K = 3.

Launch 0 is searched around c = T_c q with T_c = T_0 + beta_0 (T_1 - T_0),
beta_0 = min(a_0, cap_0 / s_1), s_1 the largest displacement of the step T_0 -> T_1 over the corners
of the target's box grown by rmax.  T_1 is either the hindsight second pose of the registration or
the pilot's estimate: one Kabsch step over every S-th 64-query chunk of the cell-sorted queries
(S = max(1, chunks / 8192)), over the pairs the octant certifies only (the first design) or over every
pair within rmax (what the engine does: the certified pairs alone give a step ~20 % short on the 50M
registration, measured).  Launch 1 is plain; launches 2.. follow
k_pose_set's rule (alpha 0.5, cap 20 mm).

Block rule: "c" places the 2x2x2 block from c (floor(cell(c) - 1/2)), "q" from the query at the
launch's pose q_t.  Either way the cache ranks at c with D = min(d_4(c), c's distance to the faces
of the block scanned), which can be <= 0 (the record then settles nothing), and the launch's own
result is certified by q_t's distance to the same faces; what that cannot certify goes to the ring.

  python tools/sim_icp_pilot.py [n_points | window=W] [sweep]
"""
import sys

import numpy as np
from scipy.spatial import cKDTree

import sim_icp_lookahead as S0
from sim_icp_lookahead import H, K, MC, RMAX, ora

ALPHA, CAP = 0.5, 0.02  # kLookAlpha, kLookCap


def step_size(Ta, Tb, lo, hi):
    """Largest displacement over the box corners of the step from pose Ta to pose Tb."""
    corners = np.array([[(hi if c >> a & 1 else lo)[a] for a in range(3)] for c in range(8)], np.float64)
    M = Ta @ np.linalg.inv(Tb)
    return np.linalg.norm(corners - (corners @ M[:3, :3].T + M[:3, 3]), axis=1).max()


def pilot_pose(tgt, q, T0, certified):
    """The pilot's estimate of the second pose and (stride, chunks, pairs)."""
    o = tgt.min(0).astype(np.float64)
    n = (np.floor((tgt.max(0).astype(np.float64) - o) / H) + 2).astype(np.int64)
    cell = np.clip(np.floor((q.astype(np.float64) - o) / H - 0.5).astype(np.int64), 0, n - 1)
    nbk = (n + 7) // 8
    b = ((cell[:, 2] // 8) * nbk[1] + cell[:, 1] // 8) * nbk[0] + cell[:, 0] // 8
    key = b * 512 + ((cell[:, 2] % 8) * 8 + cell[:, 1] % 8) * 8 + cell[:, 0] % 8
    order = np.argsort(key, kind="stable")
    nch = (len(q) + 63) // 64
    s = max(1, nch // 8192)
    take = np.concatenate([order[c * 64:(c + 1) * 64] for c in range(0, nch, s)])
    qs = np.ascontiguousarray(q[take])
    R, t = T0[:3, :3].astype(np.float32), T0[:3, 3].astype(np.float32)
    ei, ed = ora.F32Index(tgt).correspond(qs, R, t, RMAX)
    # only winners the octant certifies: within the query's distance to its block's faces
    f = ((qs.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]) - o) / H
    bb = np.floor(f - 0.5)
    m = (np.minimum(f - bb, bb + 2 - f).min(1) - MC) * H
    if certified:
        ei = np.where((ei >= 0) & (np.sqrt(np.maximum(ed, 0)) <= m), ei, -1).astype(ei.dtype)
    rc, dT = ora.icp_solve(ora.icp_accumulate(tgt, qs, R, t, ei, ed))
    return (dT @ T0 if rc == 0 else T0), (s, (nch + s - 1) // s, int((ei >= 0).sum()))


def model(tgt, q, poses, a0=0.0, cap0=0.0, T1=None, block0="q", block="c", alpha=ALPHA, cap=CAP):
    """Searched and ring fractions per launch.  a0 = 0: today's first launch."""
    n = len(q)
    tree = cKDTree(tgt.astype(np.float64))
    o = tgt.min(0).astype(np.float64)
    lo, hi = o - RMAX, tgt.max(0).astype(np.float64) + RMAX
    q64 = q.astype(np.float64)
    beta, _ = S0.betas(poses, lo, hi, alpha, cap)
    cs, D, cache = np.zeros((n, 3)), np.zeros(n), np.zeros((n, K), np.int64)
    searched, ring = [], []
    beta0 = 0.0
    for it, T in enumerate(poses):
        qt = q64 @ T[:3, :3].T + T[:3, 3]
        if it == 0:
            need = np.ones(n, bool)
        else:
            dc = np.linalg.norm(tgt[cache].astype(np.float64) - qt[:, None, :], axis=2).min(1)
            need = ~(dc < D - np.linalg.norm(qt - cs, axis=1))
        idx = np.nonzero(need)[0]
        if it == 0:
            Tc, rule = T, block0
            if a0 > 0 and T1 is not None:
                s1 = step_size(T, T1, lo, hi)
                if s1 > 0:
                    beta0 = min(a0, cap0 / s1)
                    Tc = T + beta0 * (T1 - T)
        else:
            Tc, rule = T + beta[it] * (T - poses[it - 1]), block
        c = q64[idx] @ Tc[:3, :3].T + Tc[:3, 3]
        dd, ii = tree.query(c, k=K + 1, workers=8)
        f, ft = (c - o) / H, (qt[idx] - o) / H
        b = np.floor((f if rule == "c" else ft) - 0.5)
        mcen = (np.minimum(f - b, b + 2 - f).min(1) - MC) * H    # c's distance to the block's faces
        mt = (np.minimum(ft - b, b + 2 - ft).min(1) - MC) * H    # q_t's, same block
        dnow = tree.query(qt[idx], k=1, workers=8)[0]
        ok = np.minimum(dnow, RMAX) <= mt
        cache[idx] = ii[:, :K]
        D[idx] = np.where(ok, np.minimum(dd[:, K], np.maximum(mcen, 0.0)), 0.0)
        cs[idx] = c
        searched.append(len(idx) / n)
        ring.append((~ok).sum() / n)
    return searched, ring, beta0


def row(name, s, r, beta0):
    print(f"{name:58s} beta0 {beta0:5.3f} | searched 1..5 " + " ".join(f"{x:.3f}" for x in s[1:6]) +
          f" | later {sum(s[1:]):.3f} n | 1+2 {s[1] + s[2]:.3f} | ring l0 {r[0]:.3f} ring 2..5 {sum(r[2:6]):.4f}"
          f" ring 1.. {sum(r[1:]):.3f}")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 2_000_000
    win = [float(a[7:]) for a in sys.argv[1:] if a.startswith("window=")]
    tgt, q, side = S0.window_scene(win[0]) if win else S0.scene(n)
    poses = S0.oracle_poses(tgt, q)
    print(f"{len(tgt)} targets, {len(q)} queries, {'window' if win else 'tile'} {side:.1f} m, cell {H} m, "
          f"rmax {RMAX} m, {S0.ITERS} launches")
    T1 = poses[1]
    Tp, info = pilot_pose(tgt, q, poses[0], True)
    Ta, info_a = pilot_pose(tgt, q, poses[0], False)
    o = tgt.min(0).astype(np.float64)
    lo, hi = o - RMAX, tgt.max(0).astype(np.float64) + RMAX
    print(f"pilot: stride {info[0]}, {info[1]} chunks, {info[2]} pairs; first step {step_size(poses[0], T1, lo, hi) * 1e3:.1f} mm, "
          f"pilot's error {step_size(T1, Tp, lo, hi) * 1e3:.2f} mm (largest corner distance between its T_1 and the real one); "
          f"with every pair within rmax {info_a[2]} pairs, error {step_size(T1, Ta, lo, hi) * 1e3:.2f} mm")
    row("today (alpha 0.5, cap 20 mm)", *model(tgt, q, poses))
    row("launch-0 look-ahead a0 1.5 cap0 30, block around c", *model(tgt, q, poses, 1.5, 0.03, T1, "c", "c"))
    row("same, block around q_t at launch 0", *model(tgt, q, poses, 1.5, 0.03, T1, "q", "c"))
    row("block around q_t at every look-ahead launch", *model(tgt, q, poses, 1.5, 0.03, T1, "q", "q"))
    row("today's beta rule, block around q_t at every launch", *model(tgt, q, poses, block="q"))
    row("PILOT's T_1, a0 1.5 cap0 30, block around q_t everywhere", *model(tgt, q, poses, 1.5, 0.03, Tp, "q", "q"))
    row("ENGINE: all-pairs pilot, a0 1.5 cap0 45, block q_t everywhere", *model(tgt, q, poses, 1.5, 0.045, Ta, "q", "q"))
    row("beta = 0 at every launch", *model(tgt, q, poses, alpha=0.0))
    if "sweep" in sys.argv:
        for a0 in (1.0, 1.5, 2.0):
            for cap0 in (0.02, 0.025, 0.03, 0.04, 0.045, 0.06):
                row(f"all-pairs pilot, a0 {a0:g} cap0 {cap0 * 1e3:g} mm, block q_t", *model(tgt, q, poses, a0, cap0, Ta, "q", "q"))


if __name__ == "__main__":
    main()
