#!/usr/bin/env python3
"""Benchmark of the hot path on MI355X (contract: one JSON line from rank 0).

Workload (BASELINE.json metric "Mcorrespondences/s + ICP iter/s, 50M-vs-50M fp32 @ 1/2/4/8
MI355X"): config C4 -- a point_cloud_closure / get_rot_icp registration of a 50M-point query
cloud against a 50M-point target: build the fp32 grid index of the target, sort the queries,
then 20 ICP iterations (fused transform + exact 1-NN within rmax + 24 accumulators per
iteration, Kabsch solve on the device; the pose never leaves HBM during the 20 iterations).
One "step" = one such full registration; inputs (fp32 xyz) are resident in HBM before the
timed region.

N GPUs (one process per GPU; `--gpus N` without torchrun re-launches itself under
torch.distributed.run from a parent that never touches the GPU):
  --mode slab     (headline, STRONG scaling) the SAME 50M-vs-50M registration split into N
                  x-slabs: a rank owns the queries of its slab and indexes the targets of the
                  slab widened by a halo; a device guard certifies each iteration that the pose
                  keeps the owned queries inside the halo.  Collective per iteration:
                  all_reduce(SUM) of the 24 accumulators (RCCL over xGMI).
  --mode sharded  the north_star layout: the target sharded by x-slab (a rank holds only its
                  shard), queries replicated; per iteration ReduceScatter(MIN) of 8-byte (d2,
                  index) keys per query, AllGather of the 1-byte owning shard of each winner,
                  each rank accumulates the winners it owns from its own shard, then
                  all_reduce(SUM) of the 24 accumulators.
  --mode weak     WEAK scaling: each rank registers its own 50M-vs-50M tile.
At N > 1 a --full line also carries the two other modes under "alt_modes" (--no-alt skips them).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--mode slab|sharded|weak] [--n|--points 50000000]
                  [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: set up, warm up, time the K steps, print the
line.  --full adds the legs that take runs of their own: the CPU baseline (cpu_baseline; --no-cpu
skips it) and, at N > 1, the two other modes (alt_modes; --no-alt skips them).  --dump-outputs DIR
writes what the last timed step returned to its caller as DIR/<name>.npy (dump_outputs below).

The other BASELINE.json configs print the same JSON contract with --config (one step = one
pass of that config's hot path over one batch; every rank runs its own batch, so N > 1 is weak
scaling with no collective):
  --config C1   voxel_grid leaf 0.1 of a 105k-pt cloud + index + 1-NN of 100k queries
  --config C2   1M-vs-1M brute-force kNN k=8 (fp32 MFMA ranking, certified fp64 re-rank)
  --config C3   10M-pt street scene: VoxelGrid leaf 0.05, then the fp64 index of the centroids
                and calculate_feature normals k=32
  --config C5   radius r=0.2 + normals over the fp16 cell-relative index: the 200M-pt scene per
                GPU (--c5-points)
"""
import argparse
import glob
import hashlib
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
BYTES_PER_CORR = 32         # 12 query + 12 target + 8 (idx, d2)
METRIC = "Mcorrespondences/s + ICP iter/s, 50M-vs-50M fp32 @ 1/2/4/8 MI355X"
ICP_KERNELS = ("k_icp_verify", "k_icp_octant", "k_icp_ring")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("slab", "sharded", "weak"), default="slab")
    ap.add_argument("--n", "--points", dest="n", type=int, default=50_000_000,
                    help="points per cloud (per GPU in weak mode); spell it --points under "
                         "torch.distributed.run, whose parser rejects the ambiguous prefix --n")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rmax", type=float, default=0.25)
    ap.add_argument("--cell", type=float, default=0.12, help="ICP target grid cell (m); swept 0.1-0.16, 0.12 best")
    ap.add_argument("--halo", type=float, default=2.0, help="slab mode: target halo (m), >= rmax + motion")
    ap.add_argument("--cpu-n", type=int, default=2_000_000, help="CPU baseline sample (all threads)")
    ap.add_argument("--cpu-iters1", type=int, default=3, help="CPU baseline iterations on 1 thread")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline: the CPU baseline and, at N > 1, the alt_modes")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs as DIR/<name>.npy")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-alt", action="store_true", help="--full at N > 1: skip the alt_modes runs")
    ap.add_argument("--c5-points", type=int, default=200_000_000,
                    help="--config C5: points per GPU (the 200M-pt scene fits one GPU)")
    ap.add_argument("--c5-check", type=int, default=0,
                    help="--config C5 at N > 1: after timing, compare this many sampled rows per rank with the "
                         "single-process rows (rehearsal check)")
    ap.add_argument("--c5-order", choices=("native", "tiles", "cells"), default="native",
                    help="--config C5 diagnostic: 'tiles' feeds the scene in 1 m tile order (a scan-coherent "
                         "caller order), 'cells' in the index's own cell order, instead of the generator's random "
                         "order; the headline is 'native'")
    ap.add_argument("--config", choices=("C1", "C2", "C3", "C4", "C5"), default="C4")
    ap.add_argument("--icp-graph", action="store_true",
                    help="replay one captured HIP graph per ICP launch (PCP_ICP_OPT_GRAPH; identical results)")
    ap.add_argument("--icp-lanes", type=str, default="",
                    help="profiling: 'first,list,ring' lanes per query of the ICP passes (0 = the library's choice)")
    return ap.parse_args()


def launch(args):
    """Parent of an N-GPU run: start N ranks under torch.distributed.run and exit with their
    status.  Nothing here initialises the GPU (no HIP call before the children exist)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)]
    # torch.distributed.run's parser rejects "--n" (ambiguous prefix of its own options)
    cmd += ["--points" if a == "--n" else "--points=" + a[4:] if a.startswith("--n=") else a for a in sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def pmc_traffic(workload):
    """HBM bytes per ICP iteration (k_icp_verify + k_icp_octant + k_icp_ring, FETCH_SIZE x2 +
    WRITE_SIZE, summed over the profiled launches / iterations) from the newest
    profiles/*/pmc_traffic.json measured on THIS icp.hip (sha1 match) AND on this run's workload
    (its "workload" record equals `workload`: points per cloud, world size, mode), else None --
    counters of another size or rank count say nothing about this line's kernels.
    Made by: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate runs) of
    `bench.py --steps 1 --warmup 0 --no-cpu`, summarised by tools/pmc_summary.py --key=n=...
    --key=world=... --key=mode=..."""
    src = os.path.join(ROOT, "pointcloudprocess_amd", "csrc", "icp.hip")
    sha = hashlib.sha1(open(src, "rb").read()).hexdigest()
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*", "pmc_traffic.json")), key=os.path.getmtime,
                    reverse=True):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        if d.get("icp_hip_sha1") != sha or d.get("workload") != workload:
            continue
        ks = d["kernels"]
        if "k_icp_octant" not in ks:
            return None
        iters = ks["k_icp_octant"]["launches"]
        tot = 0.0
        for k in ICP_KERNELS:
            e = ks.get(k)
            if e is not None:
                tot += e["launches"] * (e["fetch_bytes_avg"] + (e["write_bytes_avg"] or 0.0))
        return tot / iters, os.path.relpath(f, ROOT)
    return None


DUMP_BYTES = 60_000_000    # --dump-outputs: budget of all the arrays together (under 64 MB with the headers)


def dump_outputs(path, arrays):
    """--dump-outputs: write each of `arrays` (name -> tensor, ndarray or scalar) as
    <path>/<name>.npy, floating types wider than fp32 and integers as float64 (exact below 2^53),
    the rest as float32.  The files share DUMP_BYTES equally; an array over its share is written
    as a fixed sample of its leading-axis rows (seeded by the array's length only, ascending, the
    same rows in every run and every build), so two runs compare file for file."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES // max(len(arrays), 1)
    for name, a in arrays.items():
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
        t = t.detach().reshape(1) if t.dim() == 0 else t.detach()
        wide = (not t.dtype.is_floating_point) or t.element_size() > 4
        row_bytes = max(1, t[0].numel()) * (8 if wide else 4) if t.shape[0] else 1
        keep = share // row_bytes
        if t.shape[0] > keep:
            g = torch.Generator(device="cpu")
            g.manual_seed(t.shape[0])
            rows = torch.sort(torch.randint(0, t.shape[0], (keep,), generator=g)).values
            t = t[rows.to(t.device)]
        t = t.to(torch.float64 if wide else torch.float32).cpu().contiguous()
        np.save(os.path.join(path, name + ".npy"), t.numpy())


def cpu_info():
    """(model, nproc, affinity CPUs, cgroup CPU quota or None)."""
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        out = subprocess.check_output(["lscpu"], text=True, timeout=10)
        for line in out.splitlines():
            if line.startswith("Model name:"):
                model = line.split(":", 1)[1].strip()
    except (OSError, subprocess.SubprocessError):
        pass
    quota = None
    try:  # cgroup v2 cpu.max: "<quota> <period>" or "max <period>"
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = round(int(q) / int(per), 2)
    except (OSError, ValueError):
        pass
    return model, os.cpu_count(), len(os.sched_getaffinity(0)), quota


def native_oracle():
    """The CPU baseline's oracle: built on THIS host -O3 -march=native -fopenmp (oracle/Makefile
    `native`); falls back to the portable -O2 parity build if the host compiler fails."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ctypes as ora  # test infrastructure: the checker / baseline only
    try:
        path, march = ora.use_native()
        build = f"gcc -O3 -march=native ({march}) -fopenmp -ffp-contract=off: {os.path.relpath(path, ROOT)}"
    except (OSError, subprocess.SubprocessError) as e:
        ora.load()
        build = f"portable -O2 parity build (native build failed: {e})"
    return ora, build


def cpu_baseline(args, T_true, synth):
    """The oracle's ICP (C restatement: kd-tree + OpenMP correspondences, per-thread
    accumulators), built -O3 -march=native on this host, on a bounded sample of the same
    workload.  The kd-tree build and the iterations are timed separately.  It runs with ALL the
    process's CPUs (affinity count, value_all) and with the thread count the harness allots one
    GPU (OMP_NUM_THREADS, value_share), and on one core; `value` is the faster of the first two
    (under a cgroup CPU quota smaller than the affinity set, the all-thread run oversubscribes
    the quota and is the slower one)."""
    import numpy as np
    ora, build = native_oracle()
    model, ncpu, naff, quota = cpu_info()
    share = int(os.environ.get("OMP_NUM_THREADS", "0")) or naff

    n = args.cpu_n
    side = 200.0 * math.sqrt(n / float(args.n))  # same point density as the GPU cloud
    tgt, q = synth.icp_pair(n, n, 4001, 4002, T_true, extent=(side, side), device="cpu")
    tgt, q = tgt.numpy(), q.numpy()

    def run(nthreads, iters):
        err, T, bs, its = ora.icp_timed(tgt, q, np.eye(4), args.rmax, iters, nthreads=nthreads)
        return n * iters / its / 1e6, bs, its

    v_all, b_all, i_all = run(naff, args.iters)
    v_sh, b_sh, i_sh = run(share, args.iters) if share != naff else (v_all, b_all, i_all)
    v_1, b_1, i_1 = run(1, args.cpu_iters1)
    best_all = v_all >= v_sh
    v_best, c_best, i_best, b_best = (v_all, naff, i_all, b_all) if best_all else (v_sh, share, i_sh, b_sh)
    return {
        "value": round(v_best, 3),
        "unit": "Mcorrespondences/s",
        "cores": c_best,
        "kind": "port",
        "sample": f"{n}-vs-{n} pts (same density, {side:.0f}x{side:.0f} m tile), {args.iters} ICP iters of "
                  f"oracle/pcp_oracle.c ora_icp_timed on {c_best} threads (the faster of {naff} and {share}): "
                  f"iterations {i_best:.2f} s (timed, = value), kd-tree build {b_best:.2f} s (not in value)",
        "build": build,
        "value_all": round(v_all, 3),
        "cores_all": naff,
        "value_share": round(v_sh, 3),
        "cores_share": share,
        "sample_share": f"the same sample on OMP_NUM_THREADS = {share} threads (the CPU share the harness allots one "
                        f"GPU on this box): iterations {i_sh:.2f} s, build {b_sh:.2f} s",
        "value_1core": round(v_1, 3),
        "sample_1core": f"the same {n}-vs-{n} pts, first {args.cpu_iters1} ICP iters on 1 thread: iterations "
                        f"{i_1:.2f} s, build {b_1:.2f} s",
        "nproc": ncpu,
        "affinity_cpus": naff,
        "cgroup_cpu_quota": quota,
        "cpu_model": model,
    }


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch(args)

    import faulthandler

    import numpy as np
    import torch
    import torch.distributed as dist

    from pointcloudprocess_amd import _lib
    from pointcloudprocess_amd import distributed as D
    from pointcloudprocess_amd import ops, synth
    if args.icp_lanes:  # profiling: fixed lanes per query (results are identical for every choice)
        D.GpuEngine.lane_options = tuple(int(v) for v in args.icp_lanes.split(","))
    D.GpuEngine.graph = bool(args.icp_graph)

    # a fatal signal prints the Python stack (faulthandler) and, first, the faulting native
    # library and frames (libpcp's dladdr report, which then chains to faulthandler)
    faulthandler.enable()
    _lib.load().pcp_fault_report_install()

    if args.config != "C4":
        import bench_configs  # the other BASELINE.json configs (same JSON contract)
        return bench_configs.main(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; reporting n_gpus={world}", file=sys.stderr)
    # rehearsal knobs (multi-rank logic on a one-GPU box): PCP_BENCH_DEVICE pins every rank to
    # one device, PCP_BENCH_BACKEND=gloo replaces RCCL.  The driver's runs use neither.
    local = int(os.environ.get("PCP_BENCH_DEVICE", local))
    backend = os.environ.get("PCP_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    ctx = ops.Context(local)
    T_true = synth.rigid()
    n = args.n

    def barrier():
        if world > 1:
            dist.barrier()

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def sum_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return float(t.item())

    def run_mode(mode, steps, warmup):
        """Timed registrations of one mode; returns the per-mode record (rank-uniform)."""
        kernel = {"ms": 0.0, "launches": 0, "fallback": 0.0}
        exch = []
        info = {"guard_ok": True}
        if mode == "weak":  # each rank its own tile (same density, own seeds, shifted along x)
            tgt, q = synth.icp_pair(n, n, 4001 + 1000 * rank, 4002 + 1000 * rank, T_true, device=dev)
            if rank:
                shift = torch.tensor([200.0 * rank, 0.0, 0.0], device=dev, dtype=torch.float32)
                tgt = tgt + shift
                q = synth.apply_inverse(synth.apply_inverse(q, np.linalg.inv(T_true)) + shift, T_true)
            tile_t, tile_q = tgt.contiguous(), q.contiguous()
            units = n * world
            del tgt, q
        else:  # one 50M-vs-50M registration, split across the ranks
            tgt, q = synth.icp_pair(n, n, 4001, 4002, T_true, device=dev)
            units = n
            if mode == "slab":
                xs = torch.sort(q[:, 0]).values
                b = [-math.inf] + [float(xs[(n * r) // world].item()) for r in range(1, world)] + [math.inf]
                del xs
                lo, hi = b[rank], b[rank + 1]
                qm = (q[:, 0] >= lo) & (q[:, 0] < hi)
                tm = (tgt[:, 0] >= lo - args.halo) & (tgt[:, 0] < hi + args.halo)
                tile_q, tile_t = q[qm].contiguous(), tgt[tm].contiguous()
                mn, mx = tile_q.min(0).values.double().cpu().numpy(), tile_q.max(0).values.double().cpu().numpy()
                guard = ([mn[0], mx[0], mn[1], mx[1], mn[2], mx[2]], lo - args.halo + args.rmax,
                         hi + args.halo - args.rmax)
                info["halo_m"] = args.halo
                del tgt, q
            else:  # sharded: x-sorted target, equal-count contiguous shards; queries replicated.
                # The rank keeps ONLY its shard (the full cloud is synthetic set-up, freed here).
                tgt = tgt[torch.argsort(tgt[:, 0])]
                bounds = [D.shard_range(n, world, r)[0] for r in range(world)] + [n]
                tile_t, tile_q = tgt[bounds[rank]:bounds[rank + 1]].contiguous(), q.contiguous()
                info["target_points_per_rank"] = int(tile_t.shape[0])
                del tgt, q
        torch.cuda.synchronize()
        result = {}

        spans = []  # (before build, after build + query sort, after the iterations) per timed step

        def one_step(timed):
            st = {}
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
            if timed:
                ev[0].record()
            eng = D.GpuEngine(ctx, tile_t, tile_q, cell_size=args.cell)
            if timed:
                ev[1].record()
            if mode == "sharded":
                err, T = D.run_target_sharded_dev(eng, np.eye(4), args.rmax, args.iters, bounds,
                                                  exchange=exch if timed else None)
                ok = True
            else:
                err, T, ok = D.run_slab_dev(eng, np.eye(4), args.rmax, args.iters,
                                            guard=guard if mode == "slab" else None,
                                            exchange=exch if timed else None, out_stats=st)
            ms, nl = eng.icp.kernel_ms()
            if timed:
                ev[2].record()
                spans.append(ev)
                kernel["ms"] += ms
                kernel["launches"] += nl
                kernel["fallback"] += st.get("fallback", 0.0)
                info["guard_ok"] = info["guard_ok"] and ok
            result["T"], result["err"], result["ok"], result["nq"] = T, err, ok, eng.icp.q.shape[0]
            eng.close()

        for _ in range(warmup):
            one_step(False)
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one_step(True)
        torch.cuda.synchronize()
        barrier()
        dt = max_over_ranks(time.perf_counter() - t0)
        exch_ms = (sum(a.elapsed_time(b) for a, b in exch) / len(exch)) if exch else 0.0
        # where a rank's step goes (the strong-scaling model: the pre-iteration span is the part
        # that does not shrink with the slab): every rank's averages, gathered by a SUM of slots
        pre = sum(e[0].elapsed_time(e[1]) for e in spans) / max(len(spans), 1)
        its = sum(e[1].elapsed_time(e[2]) for e in spans) / max(len(spans), 1)
        slots = torch.zeros(2 * world, dtype=torch.float64, device=dev)
        slots[2 * rank], slots[2 * rank + 1] = pre, its
        if world > 1:
            dist.all_reduce(slots, op=dist.ReduceOp.SUM)
        slots = slots.cpu().tolist()
        rec = {
            "value": units * args.iters * steps / dt / 1e6,
            "ms_per_step": dt / steps * 1e3,
            "icp_iter_per_s": args.iters * steps / dt,
            "exchange_ms_per_iter": max_over_ranks(exch_ms),
            "guard_ok": bool(max_over_ranks(0.0 if info["guard_ok"] else 1.0) == 0.0),
            "T": result["T"], "err": result["err"], "last_guard_ok": result["ok"],
            "kernel_avg_ms": kernel["ms"] / max(kernel["launches"], 1),
            "units_per_launch": result["nq"],
            "queries_all_ranks": sum_over_ranks(float(result["nq"])),
            "fallback_frac": kernel["fallback"] / max(1.0, result["nq"] * kernel["launches"]),
            "per_rank": [{"rank": r, "pre_iteration_ms": round(slots[2 * r], 3),
                          "iterations_ms": round(slots[2 * r + 1], 3)} for r in range(world)],
        }
        rec.update({k: v for k, v in info.items() if k != "guard_ok"})
        del tile_t, tile_q
        torch.cuda.empty_cache()
        return rec

    main_rec = run_mode(args.mode, args.steps, args.warmup)
    alt = {}
    if args.full and world > 1 and not args.no_alt:
        for m in ("slab", "sharded", "weak"):
            if m != args.mode:
                r = run_mode(m, max(1, args.steps), 1)
                alt[m] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()
                          if k not in ("T", "last_guard_ok")}
                alt[m]["T_err_vs_truth"] = float(np.abs(r["T"] - T_true).max())

    if rank == 0 and args.dump_outputs:
        # what run_slab_dev / run_target_sharded_dev returned to rank 0 in the last timed step
        # (err, T, guard_ok); slab and sharded modes return the same on every rank
        dump_outputs(args.dump_outputs, {"T": main_rec["T"], "err": main_rec["err"],
                                         "guard_ok": float(main_rec["last_guard_ok"])})
    if rank == 0:
        r = main_rec
        traffic = pmc_traffic({"n": n, "world": world, "mode": args.mode})
        k_avg_ms = r["kernel_avg_ms"]
        achieved = BYTES_PER_CORR * r["units_per_launch"] / (k_avg_ms * 1e-3) / 1e9  # algorithmic GB/s per launch
        par = {"slab": f"x-slabs x{world}: owned queries + targets of the slab +- {args.halo} m halo per rank; "
                       "RCCL all_reduce(SUM) of 24 fp64 accumulators per iteration",
               "sharded": f"target sharded x{world} (x-slabs; a rank holds only its shard), queries replicated; RCCL "
                          "ReduceScatter(MIN) of 8-B (d2, index) keys + AllGather of the 1-B owning shard per query + "
                          "all_reduce(SUM) of 24 fp64 per iteration",
               "weak": f"co-partitioned tiles x{world} (each rank its own 50M-vs-50M); all_reduce(SUM) of 24 fp64"}
        line = {
            "metric": METRIC,
            "value": round(r["value"], 3),
            "unit": "Mcorrespondences/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(r["ms_per_step"], 3),
            "higher_is_better": True,
            "scaling": "weak" if args.mode == "weak" else "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic street scene (ground+facades+poles, seeded); query = independent "
                    "resample moved by a known rigid motion",
            "config": {"workload": f"C4: {n / 1e6:g}M-vs-{n / 1e6:g}M get_rot_icp/point_cloud_closure ICP, "
                                   f"{args.iters} iters (index build + query sort + iterations per step)"
                                   + (" per rank" if args.mode == "weak" else ""),
                       "points_per_cloud": n, "iters": args.iters, "rmax_m": args.rmax,
                       "cell_m": args.cell, "mode": args.mode, "parallelism": par[args.mode]},
            "icp_iter_per_s": round(r["icp_iter_per_s"], 3),
            "icp_final_rms_m": round(r["err"], 6),
            "icp_max_abs_T_err_vs_truth": float(np.abs(r["T"] - T_true).max()),
            "halo_guard_ok": r["guard_ok"],
            "exchange_ms_per_iter": round(r["exchange_ms_per_iter"], 4),
            "per_rank": r["per_rank"],
            "roofline": {
                "bound": "hbm",
                "kernel": "+".join(ICP_KERNELS) + " (one ICP iteration; aggregate of the three passes and "
                                                  "their list compactions)",
                "achieved": round(achieved, 2),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": round(traffic[0] / (k_avg_ms * 1e-3) / 1e9, 2) if traffic else None,
                "traffic_bytes_per_launch": round(traffic[0]) if traffic else None,
                "traffic_source": traffic[1] if traffic else "none: no sha-matched PMC record of this workload "
                                                             f"(n {n}, world {world}, mode {args.mode})",
                "kernel_avg_ms": round(k_avg_ms, 4),
                "bytes_per_unit": BYTES_PER_CORR,
                "units_per_launch": r["units_per_launch"],
                "launch_includes": "per iteration on rank 0: k_icp_verify (candidate caches) + k_icp_octant "
                                   "(search list) + k_icp_ring (fallback) with their list compactions",
                "fallback_frac": round(r["fallback_frac"], 5),
            },
            "alt_modes": alt or None,
            "build_id": _lib.load().pcp_build_id().decode(),  # SHA-1 of the libpcp sources (provenance)
            "cpu_baseline": cpu_baseline(args, T_true, synth) if (args.full and not args.no_cpu and world == 1)
            else None,
        }
        print(json.dumps(line), flush=True)
    ctx.close()
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
