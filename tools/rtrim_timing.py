#!/usr/bin/env python3
"""Device time of pcp_icp_trim_keys_plane (the trim by plane residual, pcp.h I3b) beside
pcp_icp_trim_keys (the point trim, I3), at the C4 shape (bench_configs.py: N queries against an
N-point street scene, cell 0.12 m, rmax 0.25; N = 50 M by default), with hipEvents on the context's
stream.  A measurement, not a test.

What is timed, every figure as the median of --reps repetitions after one dropped warm-up, with the
range, and the two sides of a comparison interleaved (A B A B ..) so that clock drift hits both:
  * the residual trim and the point trim alone, out of place and in place, on the same keys;
  * one of those four calls alone (--only), to be run under a kernel trace: the entry's kernels
    cannot be separated by events from outside the library, and the trace's per-kernel means then
    belong to that one call;
  * one warm iteration (keys, trim in place, accumulate, solve) of the residual-trimmed loop beside
    one of the point-trimmed loop, from the same pose on a handle whose candidate caches are warm.

The plane table gets the normal (0, 0, 1) everywhere: the gather's cost does not depend on the
normals' values, and the residual is then the height difference, centimetres on the ground and
anything up to the pair's distance on a facade.

With PCP_AB=1 and PCP_LIB naming a build that lacks the residual trim (the parent commit's), only the
point-trimmed figures are measured: the comparison point for the new loop, taken in the same session.

    python tools/rtrim_timing.py [--n 50000000] [--reps 7] [--only residual_in_place]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudprocess_amd import ops, synth  # noqa: E402

RMAX = 0.25
PTRIM = (0.6, 1.0, 0.02)
RTRIM = (0.5, 3.0, 0.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, reps, before=None):
    """{name: [ms] * reps}: one dropped warm-up round, then reps rounds of every fn in turn."""
    out = {k: [] for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            if before:
                before()
            ms = timed(fn)
            if r:
                out[k].append(ms)
    return out


def summary(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["point_out_of_place", "point_in_place", "residual_out_of_place",
                                       "residual_in_place"], help="time this one call alone, then stop")
    args = ap.parse_args()
    n = args.n
    ctx = ops.Context(0)
    have_rtrim = hasattr(ctx.lib, "pcp_icp_trim_keys_plane")
    T_true = synth.rigid()
    tgt, q = synth.icp_pair(n, n, 4001, 4002, T_true, device=ctx.device)
    index = ops.GridIndex(ctx, tgt, cell_size=0.12)
    icp = ops.ICP(index, q)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device=ctx.device)
    nrm[:, 2] = 1.0
    planes = ops.IcpPlanes(ctx, tgt, nrm)
    del nrm
    T_dev, stats = icp.new_pose()
    T0, stats0 = T_dev.clone(), stats.clone()
    raw = torch.empty(n, dtype=torch.int64, device=ctx.device)
    for _ in range(3):  # the handle's first launches search in full; from here its caches are warm
        icp.keys_dev(T_dev, RMAX, out=raw)
    keys, out = raw.clone(), torch.empty_like(raw)
    res = {"n": n, "reps": args.reps, "rtrim": have_rtrim, "build": ctx.lib.pcp_build_id().decode()}

    def reset_keys():
        keys.copy_(raw)

    # ---- the trims alone
    fns = {
        "point_out_of_place": lambda: ops.icp_trim_keys(ctx, raw, *PTRIM, out=out),
        "point_in_place": lambda: ops.icp_trim_keys(ctx, keys, *PTRIM, out=keys),
    }
    if have_rtrim:
        fns["residual_out_of_place"] = lambda: ops.icp_trim_keys_plane(ctx, T_dev, q, raw, planes, *RTRIM, out=out)
        fns["residual_in_place"] = lambda: ops.icp_trim_keys_plane(ctx, T_dev, q, keys, planes, *RTRIM, out=keys)
    if args.only:  # one call alone, for a kernel trace whose per-kernel means then belong to it
        fns = {args.only: fns[args.only]}
    alone = interleaved(fns, args.reps, before=reset_keys)
    res["trim_ms"] = {k: summary(v) for k, v in alone.items()}
    if args.only:
        print(json.dumps(res))
        return
    _, st = ops.icp_trim_keys(ctx, raw, *PTRIM, out=out)
    res["point_stats"] = st.cpu().numpy().view(np.uint64).tolist()

    if have_rtrim:
        _, st = ops.icp_trim_keys_plane(ctx, T_dev, q, raw, planes, *RTRIM, out=out)
        res["residual_stats"] = st.cpu().numpy().view(np.uint64).tolist()

    # ---- one warm iteration of each loop from the same pose
    def reset_pose():
        T_dev.copy_(T0)
        stats.copy_(stats0)

    trim = torch.zeros(4, dtype=torch.int64, device=ctx.device)
    fns = {"point_trimmed_iteration": lambda: icp.run_plane_trimmed_dev(planes, q, T_dev, stats, RMAX, *PTRIM, iters=1,
                                                                        trim=trim),
           "plain_iteration": lambda: icp.run_plane_dev(planes, q, T_dev, stats, RMAX, 1)}
    if have_rtrim:
        fns["residual_trimmed_iteration"] = lambda: icp.run_plane_rtrimmed_dev(planes, q, T_dev, stats, RMAX, *RTRIM,
                                                                               iters=1, trim=trim)
    res["iteration_ms"] = {k: summary(v) for k, v in interleaved(fns, args.reps, before=reset_pose).items()}
    print(json.dumps(res))
    planes.close()
    icp.close()
    index.close()


if __name__ == "__main__":
    main()
