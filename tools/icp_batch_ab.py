#!/usr/bin/env python3
"""Batched registration (pcp.h I5) beside a host loop over single-pair handles, on the workload
the batch is meant for: many frame-sized query sets against one map.  A measurement, not a test.

Workload: a street-scene target (2 M points, extent 200 m, cell 0.25 m) with its GPU normals
(k = 16) and plane table; --segs segments of --per queries, each a square window of a second scene
along a straight path (the street y = 25 m, window edge --window m), moved by the inverse of its own
rigid of at most 1 degree about the window's centre and 0.15 m; rmax 0.5, 4 point-to-plane
iterations from the identity.

Timed with device events on the context's stream, in one process, --reps interleaved repetitions
(a b a b ..) after one dropped warm-up round, medians with the range:
  (a) batch_total   ICPBatch create + run_plane_dev
  (b) loop_total    segs x (ICP create + run_plane_dev), the handles closed after the window
      batch_run / loop_run   the run alone, on handles created outside the window (fresh ones every
                             repetition, so the single-pair handle's caches start cold as in (b))
and the batch's entries alone (keys_dev = the search kernel; accumulate_plane = the chunk sums and
the segment sums; solve_plane_dev; one iteration of run_plane_dev).  With --no-loop only the batch
side runs.  With --trace two batched create + run rounds and nothing else, for a kernel trace.  The
8 x 160000 shape of DESIGN.md 5.1d is --segs 8 --per 160000 --window 50.

With --trimmed the windows overlap the map only in part: the last quarter of every window's queries
is replaced by clutter 0.15 .. 0.45 m above the ground of its own window (trim_ref.cluttered_queries
of the tests), and both legs run the loop that trims by the plane residual (pcp.h I3b / I5b) at
rtrim_ref.SCENE_RTRIM: (a) ICPBatch create + run_plane_rtrimmed_dev, (b) segs x (ICP create +
run_plane_rtrimmed_dev).  The entries then also time the batch's trim alone and the untrimmed
run_plane_dev on the same batch, and every window's error is listed.

With --p2p both legs minimise the point-to-point objective of get_rot_icp (pcp.h I5c): (a) ICPBatch
create + run_dev, (b) segs x (ICP create + run_dev), --iters iterations each (4, or 20 = the
get_rot_icp default); no normals and no plane table are built, and the entries are keys_dev,
accumulate, solve_dev and one iteration of run_dev.

    python tools/icp_batch_ab.py [--segs 64 --per 20000 --window 20] [--reps 5] [--no-loop] [--trace]
                                 [--trimmed | --p2p] [--iters 4]
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
from pointcloudprocess_amd import ops, synth  # noqa: E402
import rtrim_ref  # noqa: E402
import trim_ref  # noqa: E402

RMAX = 0.5
ITERS = 4
STREET_Y = 25.0  # a street's centreline: a window holds ground, both facades (y = 16, 34) and poles


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    keep = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), keep


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def make_segments(n_scene, segs, per, window, device, seed=4102, clutter=0.0):
    """(q (segs * per, 3) fp32 on the device, offsets, T_true (segs, 4, 4)).  clutter: the share of
    every window's queries replaced by points that have no counterpart in the target."""
    scene = synth.street_scene(n_scene, seed, device=device)
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    half = window / 2.0
    xs = np.linspace(-100.0 + half + 2.0, 100.0 - half - 2.0, segs)
    out, Ts = [], []
    for s in range(segs):
        m = ((scene[:, 0] - float(xs[s])).abs() <= half) & ((scene[:, 1] - STREET_Y).abs() <= half)
        pts = scene[m]
        if pts.shape[0] < per:
            raise SystemExit(f"window {s} holds {pts.shape[0]} < {per} points: raise --scene or --window")
        pick = torch.randperm(pts.shape[0], generator=g)[:per].to(device)
        ang = rng.uniform(-0.5, 0.5, 3)
        # the rotation turns about the window's centre c (about the origin, half a degree would move
        # a window 90 m out by 0.8 m, beyond rmax): T = Tr(c) R Tr(-c) + t
        T = synth.rigid(ang[0], ang[1], ang[2], t=tuple(rng.uniform(-0.08, 0.08, 3)))
        c = np.array([float(xs[s]), STREET_Y, 0.0])
        T[:3, 3] += c - T[:3, :3] @ c
        seg = synth.apply_inverse(pts[pick], T)
        if clutter > 0:
            Tc = T.copy()  # cluttered_queries scatters about the origin: move the window's centre there
            Tc[:3, 3] -= c
            seg = torch.from_numpy(trim_ref.cluttered_queries(seg.cpu().numpy(), Tc, share=clutter, half=half,
                                                              seed=seed + s)).to(device)
        out.append(seg)
        Ts.append(T)
    off = np.arange(segs + 1, dtype=np.int64) * per
    return torch.cat(out).contiguous(), off, np.stack(Ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=2_000_000)
    ap.add_argument("--scene", type=int, default=6_000_000, help="points of the scene the windows are cut from")
    ap.add_argument("--segs", type=int, default=64)
    ap.add_argument("--per", type=int, default=20_000)
    ap.add_argument("--window", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trimmed", action="store_true", help="25 %% clutter per window, residual-trimmed loops")
    ap.add_argument("--p2p", action="store_true", help="the point-to-point loops (run_dev) on both legs")
    ap.add_argument("--iters", type=int, default=ITERS)
    args = ap.parse_args()
    if args.p2p and args.trimmed:
        raise SystemExit("--p2p and --trimmed exclude each other")
    iters_all = args.iters
    ctx = ops.Context(0)
    dev = ctx.device
    tgt = synth.street_scene(args.target, 4101, device=dev)
    index = ops.GridIndex(ctx, tgt, cell_size=0.25)
    planes = None
    if not args.p2p:
        ix64 = ops.GridIndex(ctx, tgt.double())
        rows = ops.normals_knn(ix64, 16)
        ix64.close()
        planes = ops.IcpPlanes(ctx, tgt, rows)
    q, off, T_true = make_segments(args.scene, args.segs, args.per, args.window, dev,
                                   clutter=0.25 if args.trimmed else 0.0)
    B = args.segs
    segq = [q[int(off[s]):int(off[s + 1])] for s in range(B)]
    eye = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).repeat(B, 1).contiguous()
    T_b, st_b = eye.clone(), torch.zeros((B, 4), dtype=torch.float64, device=dev)
    T_l, st_l = eye.clone(), torch.zeros((B, 4), dtype=torch.float64, device=dev)

    tr_b = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    tr_l = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    RT = rtrim_ref.SCENE_RTRIM

    def reset():
        T_b.copy_(eye); st_b.zero_(); T_l.copy_(eye); st_l.zero_()

    def run_batch(b, iters=iters_all):
        if args.p2p:
            b.run_dev(tgt, T_b, st_b, RMAX, iters)
        elif args.trimmed:
            b.run_plane_rtrimmed_dev(planes, T_b, st_b, RMAX, *RT, iters=iters, trim=tr_b)
        else:
            b.run_plane_dev(planes, T_b, st_b, RMAX, iters)

    def run_single(h, s):
        if args.p2p:
            h.run_dev(T_l[s], st_l[s], RMAX, iters_all)
        elif args.trimmed:
            h.run_plane_rtrimmed_dev(planes, segq[s], T_l[s], st_l[s], RMAX, *RT, iters=iters_all, trim=tr_l[s])
        else:
            h.run_plane_dev(planes, segq[s], T_l[s], st_l[s], RMAX, iters_all)

    def batch_total():
        b = ops.ICPBatch(index, q, off)
        run_batch(b)
        return [b]

    def loop_total():
        hs = []
        for s in range(B):
            h = ops.ICP(index, segq[s])
            run_single(h, s)
            hs.append(h)
        return hs

    res = {"segs": B, "per": args.per, "window_m": args.window, "target": args.target, "iters": iters_all, "rmax": RMAX,
           "reps": args.reps, "p2p": bool(args.p2p), "trimmed": list(RT) if args.trimmed else None, "build": ctx.lib.pcp_build_id().decode()}
    if args.trace:
        for _ in range(2):
            reset()
            for h in batch_total():
                h.close()
        ctx.sync()
        print(json.dumps(res))
        return

    sides = {"batch_total": batch_total}
    if not args.no_loop:
        sides["loop_total"] = loop_total
    ms = {k: [] for k in list(sides) + ["batch_run"] + ([] if args.no_loop else ["loop_run"])}
    for r in range(args.reps + 1):
        for k, fn in sides.items():
            reset()
            t, hs = timed(fn)
            for h in hs:
                h.close()
            if r:
                ms[k].append(t)
        # the runs alone, on fresh handles
        reset()
        b = ops.ICPBatch(index, q, off)
        ctx.sync()
        t, _ = timed(lambda: run_batch(b))
        b.close()
        if r:
            ms["batch_run"].append(t)
        if not args.no_loop:
            hs = [ops.ICP(index, segq[s]) for s in range(B)]
            ctx.sync()

            def loop_run():
                for s in range(B):
                    run_single(hs[s], s)
            t, _ = timed(loop_run)
            for h in hs:
                h.close()
            if r:
                ms["loop_run"].append(t)
    res["ms"] = {k: summary(v) for k, v in ms.items()}

    # both sides registered the same thing
    Tb = T_b.cpu().numpy().reshape(B, 4, 4)
    res["status_ok_batch"] = int((st_b[:, 0] == 0).sum().item())
    # pose error per segment: where the window's centre lands, and the rotation angle left
    xs = np.linspace(-100.0 + args.window / 2 + 2.0, 100.0 - args.window / 2 - 2.0, B)
    cen = [np.array([x, STREET_Y, 0.0, 1.0]) for x in xs]
    cerr = [float(np.linalg.norm((Tb[s] - T_true[s]) @ cen[s])) for s in range(B)]
    res["max_centre_err_m"] = max(cerr)
    if args.trimmed:
        res["centre_err_mm_per_window"] = [round(1e3 * e, 3) for e in cerr]
        res["kept_per_window_last_iteration"] = tr_b[:, 1].cpu().tolist()
    dR = [Tb[s][:3, :3] @ T_true[s][:3, :3].T for s in range(B)]
    res["max_angle_err_deg"] = float(max(np.degrees(np.arccos(np.clip((np.trace(r) - 1) / 2, -1, 1))) for r in dR))
    if not args.no_loop:
        res["max_pose_diff_batch_vs_loop"] = float((T_b - T_l).abs().max().item())
        a, b_ = res["ms"]["batch_total"], res["ms"]["loop_total"]
        res["accept_median_a_not_above_b"] = bool(a["median"] <= b_["median"])

    # the batch's entries alone, from the identity (the first iteration's work)
    b = ops.ICPBatch(index, q, off)
    keys = torch.empty(q.shape[0], dtype=torch.int64, device=dev)
    acc = torch.zeros((B, 24 if args.p2p else 30), dtype=torch.float64, device=dev)
    entry = {"keys_dev": lambda: b.keys_dev(eye, RMAX, out=keys)}
    if args.p2p:
        entry["accumulate"] = lambda: b.accumulate(eye, keys, tgt, acc=acc)
        entry["solve_dev"] = lambda: b.solve_dev(acc, T_b, st_b)
    else:
        entry["accumulate_plane"] = lambda: b.accumulate_plane(eye, keys, planes, acc=acc)
        entry["solve_plane_dev"] = lambda: b.solve_plane_dev(acc, T_b, st_b)
    entry["run_1_iteration"] = lambda: run_batch(b, 1)
    if args.trimmed:
        tkeys = torch.empty_like(keys)
        entry["trim_keys_plane"] = lambda: b.trim_keys_plane(eye, keys, planes, *RT, out=tkeys)
        entry["run_rtrimmed"] = lambda: run_batch(b)
        entry["run_untrimmed_same_batch"] = lambda: b.run_plane_dev(planes, T_b, st_b, RMAX, iters_all)
    ems = {k: [] for k in entry}
    for r in range(args.reps + 1):
        for k, fn in entry.items():
            reset()
            t, _ = timed(fn)
            if r:
                ems[k].append(t)
    res["entry_ms"] = {k: summary(v) for k, v in ems.items()}
    res["keyed_fraction_first_iteration"] = float((keys != np.iinfo(np.int64).max).float().mean().item())
    b.close()
    print(json.dumps(res))
    if planes is not None:
        planes.close()
    index.close()


if __name__ == "__main__":
    main()
