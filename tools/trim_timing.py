#!/usr/bin/env python3
"""Device time of pcp_icp_trim_keys against one keys + plane-accumulate pair of the plain loop, at
the C4 shape (bench_configs.py: N queries against an N-point street scene, cell 0.12 m, rmax 0.25;
N = 50 M by default), with hipEvents on the context's stream.  A measurement, not a test.

The plane table gets the normal (0, 0, 1) everywhere: the accumulation's cost is its 32-byte gather
per pair and does not depend on the normals' values.  The keys + accumulate pair is timed at the
handle's first launches (a full search) and once its candidate caches are warm (the loop's steady
state, where the pose moves little).  For per-kernel times run this script under a kernel trace.

    python tools/trim_timing.py [--n 50000000] [--reps 5]
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frac", type=float, default=0.6)
    args = ap.parse_args()
    n = args.n
    ctx = ops.Context(0)
    T_true = synth.rigid()
    tgt, q = synth.icp_pair(n, n, 4001, 4002, T_true, device=ctx.device)
    index = ops.GridIndex(ctx, tgt, cell_size=0.12)
    icp = ops.ICP(index, q)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device=ctx.device)
    nrm[:, 2] = 1.0
    planes = ops.IcpPlanes(ctx, tgt, nrm)
    del nrm
    T_dev, _ = icp.new_pose()
    keys = torch.empty(n, dtype=torch.int64, device=ctx.device)
    acc = torch.zeros(30, dtype=torch.float64, device=ctx.device)

    def pair():
        icp.keys_dev(T_dev, 0.25, out=keys)
        ops.icp_accumulate_plane(ctx, T_dev, q, keys, planes, acc=acc)

    pair_ms = [timed(pair)[0] for _ in range(4)]
    keys_ms = timed(lambda: icp.keys_dev(T_dev, 0.25, out=keys))[0]
    acc_ms = timed(lambda: ops.icp_accumulate_plane(ctx, T_dev, q, keys, planes, acc=acc))[0]
    out = torch.empty_like(keys)
    trim_ms, stats = [], None
    for _ in range(args.reps):
        ms, (_, trim) = timed(lambda: ops.icp_trim_keys(ctx, keys, args.frac, 1.0, 0.02, out=out))
        trim_ms.append(ms)
        stats = trim.cpu().numpy().view(np.uint64).tolist()
    inplace_ms = timed(lambda: ops.icp_trim_keys(ctx, keys, args.frac, 1.0, 0.02, out=keys))[0]
    t = float(np.median(trim_ms))
    res = {
        "n": n, "frac": args.frac, "valid": stats[0], "kept": stats[1],
        "cut_m": float(np.sqrt(np.array([stats[3]], dtype=np.uint32).view(np.float32)[0])),
        "trim_ms_median": t, "trim_ms_all": trim_ms, "trim_in_place_ms": inplace_ms,
        "trim_read_GBps": 4 * 8 * n / (t * 1e-3) / 1e9,
        "pair_first_ms": pair_ms[0], "pair_warm_ms": float(np.median(pair_ms[2:])),
        "keys_warm_ms": keys_ms, "accumulate_ms": acc_ms,
        "trim_share_of_first_pair": t / pair_ms[0], "trim_share_of_warm_pair": t / float(np.median(pair_ms[2:])),
    }
    print(json.dumps(res))
    planes.close()
    icp.close()
    index.close()


if __name__ == "__main__":
    main()
