"""Numpy reference of point-to-point registration over a batch (include/pcp.h, I5c), written from
the contract text, not from the kernels, out of the pieces the single-pair tests already trust:

  * per-segment pairs: icp_batch_ref.batch_keys (the exhaustive fp32 nearest neighbour under each
    segment's own pose), then "the key is not INT64_MAX and its index is inside the target";
  * images: kabsch_ref.xform32 (the pose cast to fp32, the fp32 fmaf chain);
  * the 24 accumulators: kabsch_ref.exact_acc of (image, target point, the key's fp32 d2), each sum
    exact and rounded once; [23] = 0;
  * the step: kabsch_ref.solve on the pairs (numpy's SVD of exactly centred pairs), T <- dT T, and
    the stats of pcp_icp_solve_dev: refused below three pairs (status -1, everything else of the
    segment kept), else rms = sqrt(D / n) and one more solved step.

It also builds the two scenes of tests/test_gpu_icp_batch_p2p.py, so that tests/test_icp_batch_p2p_ref.py
can assert the conditions those tests rely on without a GPU.
"""
import functools

import numpy as np

import icp_batch_ref as bref
import kabsch_ref as kr

NO_KEY = bref.NO_KEY
NACC = 24


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def pairs(T, q, keys, target):
    """(q' (m, 3) fp32, p (m, 3) fp32, d2 (m) fp32, used mask) of one segment at pose T: the queries
    whose key is not INT64_MAX and whose index is inside target."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    target = np.asarray(target, dtype=np.float32)[:, :3]
    k = np.asarray(keys).astype(np.int64)
    j = (k.view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    used = (k != NO_KEY) & (j < target.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        img, _ = kr.xform32(T, q)
    d2 = (k.view(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return img[used], target[j[used]], d2[used], used


def accumulate(T, q, keys, target):
    """(acc (24), info): kabsch_ref.exact_acc of the segment's pairs; [23] = 0."""
    qi, p, d2, _ = pairs(T, q, keys, target)
    acc = np.zeros(NACC)
    a, info = kr.exact_acc(qi, p, d2)
    acc[:23] = a
    return acc, info


def batch_accumulate(Ts, q, off, keys, target):
    Ts = np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4)
    return np.stack([accumulate(Ts[s], q[off[s]:off[s + 1]], keys[off[s]:off[s + 1]], target)[0]
                     for s in range(len(off) - 1)]) if len(off) > 1 else np.zeros((0, NACC))


def batch_step(Ts, stats, q, off, keys, target, do_scale=False):
    """One iteration from the given keys: (acc (B, 24), new Ts (B, 4, 4), new stats (B, 4), sols).
    sols[s] is kabsch_ref.solve's dict of a segment that solved, None for a frozen or refused one
    (fewer than three pairs; the scenes have no non-finite sum)."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 3)
    Ts = np.array(Ts, dtype=np.float64).reshape(-1, 4, 4)
    stats = np.array(stats, dtype=np.float64).reshape(-1, 4)
    B = len(off) - 1
    acc = np.zeros((B, NACC))
    sols = [None] * B
    for s in range(B):
        a, b = int(off[s]), int(off[s + 1])
        qi, p, d2, _ = pairs(Ts[s], q[a:b], keys[a:b], target)
        acc[s, :23] = kr.exact_acc(qi, p, d2)[0]
        if stats[s, 0] < 0:
            continue
        stats[s, 2] += acc[s, 23]
        if len(qi) < 3:
            stats[s, 0] = -1.0
            continue
        sols[s] = kr.solve(qi, p, do_scale)
        Ts[s] = sols[s]["dT"] @ Ts[s]
        stats[s, 1] = np.sqrt(acc[s, 22] / acc[s, 0])
        stats[s, 3] += 1.0
    return acc, Ts, stats, sols


def run(T0, q, off, target, rmax, iters, do_scale=False):
    """iters reference iterations from T0: a list of dicts T_prev, st_prev, keys, acc, T, stats, sols."""
    Ts = np.array(T0, dtype=np.float64).reshape(-1, 4, 4)
    stats = np.zeros((len(off) - 1, 4))
    steps = []
    for _ in range(iters):
        keys = bref.batch_keys(Ts, q, off, target, rmax)
        acc, Tn, st, sols = batch_step(Ts, stats, q, off, keys, target, do_scale)
        steps.append(dict(T_prev=Ts, st_prev=stats, keys=keys, acc=acc, T=Tn, stats=st, sols=sols))
        Ts, stats = Tn, st
    return steps


def conditioning(acc, sol):
    """max|AB| / (s1 + det s2): how many times its own rounding a solve may amplify the sums'."""
    s, det = sol["s"], sol["det"]
    return float(np.abs(acc[7:16]).max() / (s[1] + det * s[2]))


def unkeyed(keys, off):
    """Per segment the share of queries without a key (0 for an empty segment)."""
    return [float((keys[off[s]:off[s + 1]] == NO_KEY).mean()) if off[s + 1] > off[s] else 0.0
            for s in range(len(off) - 1)]


# ------------------------------------------------------------------ the lattice scene
H = 2.0 ** -5
OFF = np.array([1024.0, -512.0, 256.0])
ROT90Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
LATTICE_SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2049, 4500]
LATTICE_BAD = (6, 11)  # the segments with three non-finite rows mixed in
LATTICE_RUNS = [(0.1, 0.25), (0.3, 0.5)]  # (cell, rmax)


def lattice_pose(steps, R=None):
    """test_gpu_icp_exact_acc.pose: R (identity or the quarter turn) about the box's corner, then
    `steps` lattice steps."""
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
        T[:3, 3] = OFF - R @ OFF + [63 * H, 0.0, 0.0]  # the turned box lands on the box
    T[:3, 3] += np.asarray(steps, dtype=np.float64) * H
    return T


class Scene:
    pass


@functools.lru_cache(maxsize=None)
def lattice_scene():
    """Every coordinate a multiple of h = 2^-5 m: queries in the 64-step box at OFF, 3000 distinct
    targets of the box grown by 8 steps with none beyond step 40 in x, one lattice pose per segment
    (translations of 0..3 steps; segments 5 and 10 turn a quarter about z first)."""
    s = Scene()
    sites = np.random.default_rng(7).choice(49 * 80 * 80, 3000, replace=False)
    s.tgt = (np.stack([sites // 6400 - 8, (sites // 80) % 80 - 8, sites % 80 - 8], 1).astype(np.float64) * H
             + OFF).astype(np.float32)
    bad = np.array([[np.nan, OFF[1], OFF[2]], [OFF[0], np.inf, OFF[2]], [np.nan, np.nan, np.nan]])
    segs, Ts = [], []
    for k, n in enumerate(LATTICE_SIZES):
        rng = np.random.default_rng(100 + k)
        q = rng.integers(0, 64, (n, 3)).astype(np.float64) * H + OFF
        if k in LATTICE_BAD:
            at = rng.permutation(n + 3)[:3]
            full = np.empty((n + 3, 3))
            mask = np.ones(n + 3, bool)
            mask[at] = False
            full[mask], full[~mask] = q, bad
            q = full
        segs.append(q.astype(np.float32))
        Ts.append(lattice_pose((k % 4, (k // 4) % 4, -(k % 3)), ROT90Z if k in (5, 10) else None))
    s.segs, s.Ts = segs, np.stack(Ts)
    s.sizes = [len(g) for g in segs]
    s.off = offsets(s.sizes)
    s.q = np.concatenate(segs)
    for a in (s.tgt, s.Ts, s.off, s.q):
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def lattice_expected(rmax):
    """Per segment (keys int64, acc (24), info, exact_pose, exact_d2) from kabsch_ref.correspond on
    kabsch_ref.xform32's images: the reference of the exact test."""
    s = lattice_scene()
    out = []
    for k in range(len(s.sizes)):
        q = s.q[s.off[k]:s.off[k + 1]]
        with np.errstate(invalid="ignore", over="ignore"):
            img, exact_pose = kr.xform32(s.Ts[k], q)
        fin = np.isfinite(q).all(1)
        ei, ed, exact_d2 = kr.correspond(s.tgt, img, rmax)
        ok = ei >= 0
        keys = np.full(len(q), NO_KEY, dtype=np.int64)
        keys[ok] = ((ed[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) |
                    ei[ok].astype(np.uint64)).view(np.int64)
        acc = np.zeros(NACC)
        a, info = kr.exact_acc(img[ok], s.tgt[ei[ok]], ed[ok], centres=img[fin] if fin.any() else None)
        acc[:23] = a
        out.append((keys, acc, info, exact_pose and bool(np.isfinite(img[fin]).all()), exact_d2))
    return out


# ------------------------------------------------------------------ the street scene
STREET_SIZES = [0, 1, 63, 64, 65, 1000, 8000, 3000]
STREET_RMAX = 0.5
STREET_ITERS = 4


@functools.lru_cache(maxsize=None)
def street_scene():
    """test_gpu_icp_batch.py's scene: a 30000-point street scene (extent 50 m) with 200 of its own
    points appended again, eight segments that are their own street scenes moved by the inverse of
    their own T_true; segment 7 is turned by 90.5 degrees and starts at 90."""
    from pointcloudprocess_amd import synth
    s = Scene()
    base = synth.street_scene(30000, 11, extent=(50.0, 50.0)).numpy()
    s.tgt = np.concatenate([base, base[::150]])  # 200 duplicates at higher indices
    s.T_true = [synth.rigid(1.0, 0.4, -0.3, t=(0.15, -0.10, 0.05)) for _ in STREET_SIZES]
    s.T_true[5] = synth.rigid(-0.8, 0.2, 0.5, t=(-0.1, 0.12, 0.03))
    s.T_true[7] = synth.rigid(90.5, 0.3, -0.2, t=(0.1, 0.1, -0.05))
    s.T0 = np.stack([np.eye(4)] * len(STREET_SIZES))
    s.T0[7] = synth.rigid(90.0, 0.0, 0.0, t=(0.0, 0.0, 0.0))
    s.segs = [synth.apply_inverse(synth.street_scene(n, 100 + k, extent=(50.0, 50.0)), s.T_true[k]).numpy()
              if n else np.zeros((0, 3), dtype=np.float32) for k, n in enumerate(STREET_SIZES)]
    s.off = offsets(STREET_SIZES)
    s.q = np.concatenate(s.segs)
    for a in (s.tgt, s.T0, s.off, s.q):
        a.setflags(write=False)
    return s


def check_street_step(step, it):
    """The conditions the stepwise GPU test relies on, for one reference step: segments 0 and 1
    refuse, every other segment solves with at most a quarter of its queries unkeyed and a
    conditioning of at most 4.  Returns (largest unkeyed share, largest conditioning)."""
    off = street_scene().off
    un = unkeyed(step["keys"], off)
    worst_u, worst_c = 0.0, 0.0
    for s in range(len(STREET_SIZES)):
        if s < 2:
            assert step["stats"][s, 0] == -1 and step["sols"][s] is None, (it, s)
            continue
        assert step["stats"][s, 0] == 0 and step["sols"][s] is not None, (it, s)
        c = conditioning(step["acc"][s], step["sols"][s])
        assert un[s] <= 0.25, (it, s, un[s])
        assert c <= 4.0, (it, s, c)
        worst_u, worst_c = max(worst_u, un[s]), max(worst_c, c)
    return worst_u, worst_c
