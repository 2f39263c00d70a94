#!/usr/bin/env python3
"""One batched get_rot_icp over a span of AoS48 frames (pcp.h I5d) beside the per-frame path it
replaces, on the workload of callers.do_mul_frame_icp with is_do_sep_icp.  A measurement, not a test.

Workload: the street-scene target of tools/icp_batch_ab.py (2 M points, extent 200 m, cell 0.25 m)
and its windows (--segs frames of --per points along the street, each moved by the inverse of its own
rigid of at most 1 degree about the window's centre and 0.15 m), everything shifted to map
coordinates (3512.25, -1801.5, 40) and stored as AoS48 fp64 records; one shared start pose `rot` (a
rigid of 0.02 degrees about the map offset); rmax 0.5, --iters point-to-point iterations.

Timed with device events on the context's stream, in one process, --reps interleaved repetitions
(a b a b ..) after one dropped warm-up round, medians with the range:
  (a) batch   one ops.minmax_segments + one ops.get_rot_icp_batch over all frames and the whole target
  (b) loop    segs x (ops.transform, ops.minmax, ops.get_rot_icp): the parent's path.  Its target is
              the part of the map inside the frame's own box +- 3 m in x and y, cut before the clock
              starts (the CloudGrid cut is outside both legs); with --loop-full-target every frame
              registers against the whole target instead.
and (a) with iters = 0 (centroid, staging, index build, create, copies; no loop), whose share of (a)
is the time spent outside the loop.

    python tools/rot_batch_ab.py [--segs 64 --per 20000 --window 20] [--reps 5] [--iters 20] [--loop-full-target]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pointcloudprocess_amd import ops, synth  # noqa: E402
from icp_batch_ab import make_segments, summary, timed  # noqa: E402

RMAX = 0.5
OFF = np.array([3512.25, -1801.5, 40.0])


def aos48(xyz, off):
    """(n, 48) uint8 device records from (n, 3) device points, shifted by off in fp64."""
    rec = torch.zeros((xyz.shape[0], 6), dtype=torch.float64, device=xyz.device)
    rec[:, :3] = xyz.double() + torch.as_tensor(off, dtype=torch.float64, device=xyz.device)
    rec[:, 3] = 1.0
    return rec.view(torch.uint8).reshape(-1, 48).contiguous()


def conj(T, off):
    M = np.array(T, dtype=np.float64)
    M[:3, 3] = M[:3, 3] + off - M[:3, :3] @ off
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=2_000_000)
    ap.add_argument("--scene", type=int, default=6_000_000)
    ap.add_argument("--segs", type=int, default=64)
    ap.add_argument("--per", type=int, default=20_000)
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loop-full-target", action="store_true")
    args = ap.parse_args()
    ctx = ops.Context(0)
    dev = ctx.device
    tgt_xyz = synth.street_scene(args.target, 4101, device=dev)
    q, off, T_true = make_segments(args.scene, args.segs, args.per, args.window, dev)
    B = args.segs
    target = aos48(tgt_xyz, OFF)
    frames = aos48(q, OFF)
    rot = conj(synth.rigid(0.02, 0.01, -0.01, (0.01, -0.01, 0.005)), OFF)
    segs = [frames[int(off[s]):int(off[s + 1])] for s in range(B)]
    # (b)'s targets: the map inside each frame's own box +- 3 m (x, y), cut outside the clock
    if args.loop_full_target:
        cuts = [target] * B
    else:
        txy = target.view(torch.float64).reshape(-1, 6)[:, :2]
        cuts = []
        for s in range(B):
            mn, mx = ops.minmax(ctx, ops.transform(ctx, segs[s], rot))
            m = ((txy[:, 0] >= mn[0] - 3.0) & (txy[:, 0] <= mx[0] + 3.0) &
                 (txy[:, 1] >= mn[1] - 3.0) & (txy[:, 1] <= mx[1] + 3.0))
            cuts.append(target[m].contiguous())
    ctx.sync()

    def batch(iters=args.iters):
        box = ops.minmax_segments(ctx, frames, off, T=rot)
        return box, ops.get_rot_icp_batch(ctx, target, frames, off, RMAX, T0=rot, iters=iters, cell_size=0.25)

    def loop():
        out = []
        for s in range(B):
            moved = ops.transform(ctx, segs[s], rot)
            box = ops.minmax(ctx, moved)
            out.append((box, ops.get_rot_icp(ctx, cuts[s], moved, RMAX, iters=args.iters, cell_size=0.25)))
        return out

    sides = {"batch": batch, "loop": loop, "batch_iters0": lambda: batch(0)}
    ms = {k: [] for k in sides}
    keep = {}
    for r in range(args.reps + 1):
        for k, fn in sides.items():
            t, keep[k] = timed(fn)
            if r:
                ms[k].append(t)
    res = {"segs": B, "per": args.per, "window_m": args.window, "target": args.target, "iters": args.iters,
           "rmax": RMAX, "reps": args.reps, "loop_target": "full" if args.loop_full_target else "box +- 3 m",
           "loop_target_points": [int(np.min([c.shape[0] for c in cuts])), int(np.max([c.shape[0] for c in cuts]))],
           "build": ctx.lib.pcp_build_id().decode(), "ms": {k: summary(v) for k, v in ms.items()},
           "raw_ms": {k: [round(v, 4) for v in vs] for k, vs in ms.items()}}
    a, b = res["ms"]["batch"], res["ms"]["loop"]
    res["accept_median_a_not_above_b"] = bool(a["median"] <= b["median"])
    res["speedup_median"] = b["median"] / a["median"]
    res["share_outside_loop"] = res["ms"]["batch_iters0"]["median"] / a["median"]
    # both legs registered the same thing: where each window's centre lands against the truth
    (bmn, bmx), (err, mats, steps, _) = keep["batch"]
    half = args.window / 2.0
    xs = np.linspace(-100.0 + half + 2.0, 100.0 - half - 2.0, B)
    cerr_a, cerr_b, box_equal = [], [], True
    for s in range(B):
        cen = np.array([xs[s] + OFF[0], 25.0 + OFF[1], OFF[2], 1.0])
        truth = conj(T_true[s], OFF) @ cen
        (lmn, lmx), (_, M) = keep["loop"][s]
        cerr_a.append(float(np.linalg.norm((mats[s] @ rot @ cen - truth)[:3])))
        cerr_b.append(float(np.linalg.norm((M @ rot @ cen - truth)[:3])))
        box_equal = box_equal and np.array_equal(lmn, bmn[s]) and np.array_equal(lmx, bmx[s])
    res["max_centre_err_m"] = {"batch": max(cerr_a), "loop": max(cerr_b)}
    res["max_centre_diff_batch_vs_loop_m"] = float(np.max(np.abs(np.array(cerr_a) - np.array(cerr_b))))
    res["boxes_equal"] = bool(box_equal)
    res["solved_segments"] = int((err > 0).sum())
    res["steps"] = [int(steps.min()), int(steps.max())]
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
