"""GPU checks of point-to-point registration over a batch (include/pcp.h, I5c) against the numpy
reference tests/icp_batch_p2p_ref.py and against the single-pair path on each segment's slice.

1. Lattice scene (test_gpu_icp_exact_acc.py's): every fp32 and fp64 intermediate is exact, so the
   accumulators must equal kabsch_ref.exact_acc with np.array_equal, whatever the order of the sum.
2. The solve: kabsch_cases' list through pcp_icp_batch_solve_dev, one segment per case, held to
   check_solution / check_rank0 with their tolerances unchanged (the code test_gpu_icp_solve_dev.py
   holds to them); refusals latch per segment.
3. Street scene (test_gpu_icp_batch.py's), ONE stepwise run per do_scale, shared.  The brute-force
   keys of every step are computed once at the step's own start poses.  Sums to rtol 1e-12 / atol
   1e-12 max|acc| (reordered sums of exact products; the tree is ~30 levels deep for 8000 queries,
   worst case near 3e-14).  Poses in the units of kabsch_cases' tol_u,
     u = max|T_next - dT_ref T_prev| (s1 + det s2) / (eps max|acc[7:16]| max(1, max|T_prev|)),
   against the same figure of the single path on the slice (ICP.keys_dev -> keys_owner ->
   accumulate_owned -> pcp_icp_solve_dev): u_batch <= 16 max(26.4, u_single), kabsch_cases' measured
   figure and its margin.  Measured on an MI355X: u_batch <= 8.6 and u_single
   <= 10.3 over the four steps, 14.1 and 19.3 on the first step with do_scale.
4. The loops equal the entries in turn, bit for bit (plain: the street scene; trimmed: the cluttered
   segments of test_gpu_icp_batch_trim.py).
5. Independence of the segments, repeatability, empty batches, the allocator's balance, arguments.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_trim_cases as cases
import batch_trim_ref as bt
import icp_batch_p2p_ref as pr
import icp_batch_ref as bref
import kabsch_cases as kc
import kabsch_ref as kr
import trim_ref as tr

pytestmark = pytest.mark.gpu

NO_KEY = pr.NO_KEY
RMAX, ITERS = pr.STREET_RMAX, pr.STREET_ITERS
CASES = kc.cases()


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)  # a copy: the shared scenes are read-only


def _close(g, e):
    return np.allclose(g, e, rtol=1e-12, atol=1e-12 * max(np.abs(e).max(), 1e-300))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


class Bag:
    pass


# ------------------------------------------------------------------ 1: exact accumulators
@pytest.mark.parametrize("cell,rmax", pr.LATTICE_RUNS)
def test_exact_accumulators_on_a_lattice(ctx, cell, rmax):
    from pointcloudprocess_amd import ops
    s = pr.lattice_scene()
    exp = pr.lattice_expected(rmax)
    for k, (_, eacc, info, exact_pose, exact_d2) in enumerate(exp):  # before any GPU number
        assert exact_pose and exact_d2 and info["exact64"] and info["bound64"] < 2 ** 53, (k, info)
    pairs = [int(e[1][0]) for e in exp]
    print(f"cell {cell} rmax {rmax}: pairs per segment {pairs}")
    assert pairs[0] == 0 and all(p > 0 for p in pairs[1:])
    dtgt = _dev(ctx, s.tgt)
    index = ops.GridIndex(ctx, dtgt, cell_size=cell)
    b = ops.ICPBatch(index, _dev(ctx, s.q), s.off)
    T_dev, _ = b.new_poses(s.Ts)
    keys = b.keys_dev(T_dev, rmax)
    ekeys = np.concatenate([e[0] for e in exp])
    assert np.array_equal(keys.cpu().numpy(), ekeys), int((keys.cpu().numpy() != ekeys).sum())
    acc = torch.full((len(s.sizes), 24), 5.0, dtype=torch.float64, device=ctx.device)
    got = b.accumulate(T_dev, keys, dtgt, acc=acc).cpu().numpy()
    for k, (_, eacc, _, _, _) in enumerate(exp):
        assert np.array_equal(got[k], eacc), f"segment {k}: accumulators {np.flatnonzero(got[k] != eacc)} differ"
        assert got[k, 23] == 0
    b.close()
    index.close()


# ------------------------------------------------------------------ 2: the batched solve
def _solve(ctx, acc, do_scale, T, stats):
    ctx.check(ctx.lib.pcp_icp_batch_solve_dev(ctx.h, C.c_void_p(acc.data_ptr()), acc.shape[0], int(do_scale),
                                              C.c_void_p(T.data_ptr()), C.c_void_p(stats.data_ptr())))
    ctx.sync()
    return T.cpu().numpy().reshape(-1, 4, 4).copy(), stats.cpu().numpy().copy()


def _identity(ctx, n):
    return (torch.eye(4, dtype=torch.float64).reshape(1, 16).repeat(n, 1).to(ctx.device).contiguous(),
            torch.zeros((n, 4), dtype=torch.float64, device=ctx.device))


@pytest.mark.parametrize("do_scale", [False, True])
def test_batched_solve_on_the_case_list(ctx, do_scale):
    """One segment per case of its do_scale group; with do_scale the rank-0 cases ride along (their
    scale stays 1).  T = dT * identity: dT itself."""
    group = [c for c in CASES if c[3] == do_scale]
    rank0 = [c for c in CASES if c[0] in kc.RANK0_EXACT + kc.RANK0_NOISE]
    rows = group + (rank0 if do_scale else [])
    acc = np.stack([kr.acc24(q, p) for _, q, p, _ in rows])
    acc[:, 23] = 7.0
    T, st = _solve(ctx, _dev(ctx, acc), do_scale, *_identity(ctx, len(rows)))
    for s, (name, q, p, _) in enumerate(rows):
        assert st[s].tolist() == [0.0, np.sqrt(acc[s, 22] / acc[s, 0]), 7.0, 1.0], name
        if s < len(group):
            ran_c = kc.check_solution(name, q, p, do_scale, T[s])
            assert ran_c == (name not in kc.NON_UNIQUE)
        if name in kc.RANK0_EXACT + kc.RANK0_NOISE:
            kc.check_rank0(name, q, p, T[s])


def test_batched_solve_refuses_and_latches_per_segment(ctx):
    """kabsch_cases.bad_accumulators() at the odd rows among good ones: only those segments latch -1
    and keep T, rms and count; a later call leaves them untouched while the good ones advance."""
    _, q, p, _ = CASES[0]
    good = kr.acc24(q, p)
    good[23] = 2.0
    bad = kc.bad_accumulators()
    n = 2 * len(bad)
    odd = np.arange(n) % 2 == 1
    all_good = np.tile(good, (n, 1))
    mixed = all_good.copy()
    mixed[odd] = np.stack([a for _, a in bad])
    T_dev, stats = _identity(ctx, n)
    T1, st1 = _solve(ctx, _dev(ctx, all_good), False, T_dev, stats)
    assert (st1[:, 0] == 0).all() and (st1[:, 3] == 1).all() and (st1[:, 2] == 2.0).all()
    T2, st2 = _solve(ctx, _dev(ctx, mixed), False, T_dev, stats)
    assert (st2[odd, 0] == -1).all(), [bad[i][0] for i in np.flatnonzero(st2[odd, 0] != -1)]
    assert np.array_equal(T2[odd], T1[odd]) and np.array_equal(st2[odd, 1], st1[odd, 1]) and (st2[odd, 3] == 1).all()
    assert (st2[~odd, 0] == 0).all() and (st2[~odd, 3] == 2).all() and (st2[~odd, 2] == 4.0).all()
    assert np.array_equal(_bits(T2[~odd]), _bits(np.tile(T2[0], (n // 2, 1, 1))))  # every good row alike
    assert not np.array_equal(T2[0], T1[0])
    T3, st3 = _solve(ctx, _dev(ctx, all_good), False, T_dev, stats)
    assert np.array_equal(T3[odd], T1[odd]) and np.array_equal(st3[odd], st2[odd], equal_nan=True)
    assert (st3[~odd, 0] == 0).all() and (st3[~odd, 3] == 3).all() and not np.array_equal(T3[0], T2[0])


# ------------------------------------------------------------------ 3: stepwise on the street scene
def _stepwise(g, do_scale, iters=ITERS):
    """iters x (keys_dev, accumulate, solve_dev), everything read back."""
    T_dev, stats = g.batch.new_poses(g.s.T0)
    steps = []
    for _ in range(iters):
        T_prev = T_dev.cpu().numpy().reshape(-1, 4, 4).copy()
        st_prev = stats.cpu().numpy().copy()
        keys = g.batch.keys_dev(T_dev, RMAX)
        acc = g.batch.accumulate(T_dev, keys, g.dtgt)
        g.batch.solve_dev(acc, T_dev, stats, do_scale)
        steps.append(dict(T_prev=T_prev, st_prev=st_prev, keys=keys.cpu().numpy().copy(),
                          acc=acc.cpu().numpy().copy(), T=T_dev.cpu().numpy().reshape(-1, 4, 4).copy(),
                          stats=stats.cpu().numpy().copy()))
    return steps


def _single_step(g, k, T_prev, do_scale):
    """The parent's path on segment k's slice: its own handle's keys at T_prev, every pair owned by
    shard 0 = the whole target, accumulate_owned, pcp_icp_solve_dev.  Returns (T_next, stats)."""
    from pointcloudprocess_amd import ops
    ctx, s = g.ctx, g.s
    a, b = int(s.off[k]), int(s.off[k + 1])
    icp = g.single[k]
    T_dev, stats = icp.new_pose(T_prev)
    keys = icp.keys_dev(T_dev, RMAX)
    owner = ops.keys_owner(ctx, keys, g.bounds)
    acc = ops.accumulate_owned(ctx, T_dev, g.dq[a:b], keys, owner, 0, 0, len(s.tgt), g.dtgt)
    icp.solve_dev(acc, T_dev, stats, do_scale)
    return T_dev.cpu().numpy().reshape(4, 4).copy(), stats.cpu().numpy().copy()


def _units(T_next, T_prev, sol, eacc):
    sv, det = sol["s"], sol["det"]
    return float(np.abs(T_next - sol["dT"] @ T_prev).max() * (sv[1] + det * sv[2]) /
                 (kc.EPS * np.abs(eacc[7:16]).max() * max(1.0, np.abs(T_prev).max())))


@pytest.fixture(scope="module")
def street(ctx):
    from pointcloudprocess_amd import ops
    g = Bag()
    g.ctx, g.s = ctx, pr.street_scene()
    s = g.s
    B = len(pr.STREET_SIZES)
    g.dtgt, g.dq = _dev(ctx, s.tgt), _dev(ctx, s.q)
    g.index = ops.GridIndex(ctx, g.dtgt, cell_size=0.25)
    g.batch = ops.ICPBatch(g.index, g.dq, s.off)
    g.bounds = torch.tensor([0, len(s.tgt)], dtype=torch.int64, device=ctx.device)
    g.single = {k: ops.ICP(g.index, g.dq[int(s.off[k]):int(s.off[k + 1])]) for k in range(B) if pr.STREET_SIZES[k]}
    g.steps = _stepwise(g, False)
    g.steps_scale = _stepwise(g, True)
    # the reference of every step at the step's own start poses, and the scene's conditions
    for it, st in enumerate(g.steps):
        st["ref_keys"] = bref.batch_keys(st["T_prev"], s.q, s.off, s.tgt, RMAX)
        eacc, eT, est, sols = pr.batch_step(st["T_prev"], st["st_prev"], s.q, s.off, st["ref_keys"], s.tgt, False)
        st.update(eacc=eacc, eT=eT, est=est, sols=sols)
        pr.check_street_step(dict(keys=st["ref_keys"], acc=eacc, stats=est, sols=sols), it)
    first = g.steps[0]
    eacc, eT, est, sols = pr.batch_step(first["T_prev"], first["st_prev"], s.q, s.off, first["ref_keys"], s.tgt, True)
    g.scale_ref = dict(eacc=eacc, eT=eT, est=est, sols=sols)
    pr.check_street_step(dict(keys=first["ref_keys"], acc=eacc, stats=est, sols=sols), 0)
    yield g
    for icp in g.single.values():
        icp.close()
    g.batch.close()
    g.index.close()


def _check_step(g, it, st, exp, do_scale):
    """(a) .. (d) of one step against the reference exp; returns the largest (u_batch, u_single)."""
    s = g.s
    worst = (0.0, 0.0)
    assert np.array_equal(st["keys"], g.steps[it]["ref_keys"]), int((st["keys"] != g.steps[it]["ref_keys"]).sum())
    for k in range(len(pr.STREET_SIZES)):
        eacc, sol = exp["eacc"][k], exp["sols"][k]
        assert st["acc"][k, 0] == eacc[0] and st["acc"][k, 23] == 0, (it, k)
        assert _close(st["acc"][k], eacc), (it, k, np.abs(st["acc"][k] - eacc).max())
        assert st["stats"][k, 0] == exp["est"][k, 0], (it, k)
        if sol is None:  # refused: pose and the rest of the stats as they were
            assert st["stats"][k, 0] == -1 and np.array_equal(st["T"][k], st["T_prev"][k]), (it, k)
            assert np.array_equal(st["stats"][k, 1:], st["st_prev"][k, 1:]), (it, k)
            continue
        rms = np.sqrt(eacc[22] / eacc[0])
        assert abs(st["stats"][k, 1] - rms) <= 1e-12 * rms, (it, k)
        assert st["stats"][k, 2] == 0 and st["stats"][k, 3] == st["st_prev"][k, 3] + 1, (it, k)
        T1, st1 = _single_step(g, k, st["T_prev"][k], do_scale)
        assert st1[0] == 0 and st1[3] == 1, (it, k)
        ub = _units(st["T"][k], st["T_prev"][k], sol, eacc)
        us = _units(T1, st["T_prev"][k], sol, eacc)
        print(f"do_scale={int(do_scale)} it={it} seg={k} pairs={int(eacc[0])} u_batch={ub:.2f} u_single={us:.2f} "
              f"|T-T_ref|={np.abs(st['T'][k] - exp['eT'][k]).max():.2e}")
        assert ub <= kc.MARGIN * max(26.4, us), (it, k, ub, us)
        worst = (max(worst[0], ub), max(worst[1], us))
    return worst


def test_stepwise_run_matches_reference_and_single_path(street):
    worst = [_check_step(street, it, st, st, False) for it, st in enumerate(street.steps)]
    print("largest u_batch %.2f, largest u_single %.2f" % (max(w[0] for w in worst), max(w[1] for w in worst)))
    final = street.steps[-1]
    assert (final["stats"][:2, 0] == -1).all() and (final["stats"][:2, 3] == 0).all()
    assert np.array_equal(final["T"][:2], street.s.T0[:2])
    assert (final["stats"][2:, 0] == 0).all() and (final["stats"][2:, 3] == ITERS).all()
    assert np.array_equal(final["acc"][0], np.zeros(24))  # the empty segment


def test_first_step_with_do_scale(street):
    """The same start poses, so the same keys and accumulators; the step finds the reference's scale."""
    first, plain = street.steps_scale[0], street.steps[0]
    assert np.array_equal(first["keys"], plain["keys"]) and np.array_equal(_bits(first["acc"]), _bits(plain["acc"]))
    ub, us = _check_step(street, 0, first, street.scale_ref, True)
    print("do_scale: largest u_batch %.2f, largest u_single %.2f" % (ub, us))
    for k in range(2, len(pr.STREET_SIZES)):
        sc = kc.scale_of(first["T"][k] @ np.linalg.inv(first["T_prev"][k]))
        assert abs(sc / street.scale_ref["sols"][k]["sc"] - 1.0) < 1e-12 and sc != 1.0, (k, sc)


# ------------------------------------------------------------------ 4: the loops equal the entries
@pytest.mark.parametrize("do_scale", [False, True])
def test_run_dev_equals_stepwise_and_repeats(ctx, street, do_scale):
    steps = street.steps_scale if do_scale else street.steps
    before = ctx.alloc_stats()[0]
    runs = []
    for _ in range(2):
        T_dev, stats = street.batch.new_poses(street.s.T0)
        street.batch.run_dev(street.dtgt, T_dev, stats, RMAX, ITERS, do_scale)
        runs.append((T_dev.cpu().numpy().reshape(-1, 4, 4).copy(), stats.cpu().numpy().copy()))
    assert ctx.alloc_stats()[0] == before
    assert np.array_equal(_bits(runs[0][0]), _bits(steps[-1]["T"]))  # bit for bit
    assert np.array_equal(_bits(runs[0][1]), _bits(steps[-1]["stats"]))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    # iters == 0 leaves everything as it is
    T_dev, stats = street.batch.new_poses(street.s.T0)
    stats.fill_(3.0)
    street.batch.run_dev(street.dtgt, T_dev, stats, RMAX, 0, do_scale)
    assert np.array_equal(T_dev.cpu().numpy().reshape(-1, 4, 4), street.s.T0) and (stats.cpu().numpy() == 3.0).all()


@pytest.fixture(scope="module")
def cluttered(ctx):
    """test_gpu_icp_batch_trim.py's cluttered street scene: eight segments with 25 % clutter each and
    their own motion, from the identity."""
    from pointcloudprocess_amd import ops, synth
    g = Bag()
    sizes = [0, 1, 63, 64, 65, 1000, 8000, 3000]
    T_true = [synth.rigid(1.0, 0.4, -0.3, t=(0.15, -0.10, 0.05)) for _ in sizes]
    T_true[5] = synth.rigid(-0.8, 0.2, 0.5, t=(-0.1, 0.12, 0.03))
    T_true[7] = synth.rigid(0.6, -0.3, 0.4, t=(-0.12, 0.08, 0.04))
    tgt, q6 = synth.icp_pair(30000, 8000, 11, 12, T_true[6], extent=(50.0, 50.0))
    segs = []
    for k, n in enumerate(sizes):
        if k == 6:
            segs.append(tr.cluttered_queries(q6.numpy(), T_true[6]))
        elif n == 0:
            segs.append(np.zeros((0, 3), dtype=np.float32))
        else:
            own = synth.apply_inverse(synth.street_scene(n, 100 + k, extent=(50.0, 50.0)), T_true[k]).numpy()
            segs.append(tr.cluttered_queries(own, T_true[k], seed=5 + k))
    g.sizes, g.off = sizes, cases.offsets(sizes)
    g.dtgt = tgt.to(ctx.device)
    g.index = ops.GridIndex(ctx, g.dtgt, cell_size=0.25)
    g.batch = ops.ICPBatch(g.index, _dev(ctx, np.concatenate(segs)), g.off)
    yield g
    g.batch.close()
    g.index.close()


@pytest.mark.parametrize("params,do_scale", [(cases.POINT_PARAMS[0], False), (cases.POINT_PARAMS[1], True)],
                         ids=["f0.9-m1", "f0.5-m1.5-scale"])
def test_run_trimmed_dev_equals_the_four_entries(ctx, cluttered, params, do_scale):
    g, b = cluttered, cluttered.batch
    B = len(g.sizes)
    T_dev, stats = b.new_poses()
    for it in range(ITERS):
        keys = b.keys_dev(T_dev, RMAX)
        raw = keys.cpu().numpy().copy()
        _, trim = b.trim_keys(keys, *params, out=keys)
        acc = b.accumulate(T_dev, keys, g.dtgt)
        b.solve_dev(acc, T_dev, stats, do_scale)
        # the trim is I5b's on these keys, it rejected pairs, and the sums are over the kept ones
        eo, es = bt.trim(raw, g.off, *params)
        assert np.array_equal(_u64(trim), es) and np.array_equal(keys.cpu().numpy(), eo), it
        assert np.array_equal(acc.cpu().numpy()[:, 0], es[:, 1].astype(np.float64)), it
        assert all(3 <= es[k, 1] <= es[k, 0] for k in range(2, B)), (it, es[:, :2].tolist())
        assert es[5:, 1].sum() < es[5:, 0].sum(), (it, es[:, :2].tolist())
    eT, est, etrim = T_dev.cpu().numpy().copy(), stats.cpu().numpy().copy(), _u64(trim).copy()
    assert (est[:2, 0] == -1).all() and (est[2:, 0] == 0).all() and (est[2:, 3] == ITERS).all()
    before = ctx.alloc_stats()[0]
    runs = []
    for _ in range(2):
        T_dev, stats = b.new_poses()
        trim = b.run_trimmed_dev(g.dtgt, T_dev, stats, RMAX, *params, iters=ITERS, do_scale=do_scale)
        runs.append((T_dev.cpu().numpy().copy(), stats.cpu().numpy().copy(), _u64(trim).copy()))
    assert ctx.alloc_stats()[0] == before
    assert np.array_equal(_bits(runs[0][0]), _bits(eT)) and np.array_equal(_bits(runs[0][1]), _bits(est))
    assert np.array_equal(runs[0][2], etrim)
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(_bits(x), _bits(y))
    # iters == 0: poses, stats and trim_dev untouched
    T_dev, stats = b.new_poses()
    stats.fill_(3.0)
    trim = torch.full((B, 4), 77, dtype=torch.int64, device=ctx.device)
    b.run_trimmed_dev(g.dtgt, T_dev, stats, RMAX, *params, iters=0, do_scale=do_scale, trim=trim)
    assert (trim.cpu().numpy() == 77).all() and (stats.cpu().numpy() == 3.0).all()
    assert np.array_equal(T_dev.cpu().numpy(), np.tile(np.eye(4).reshape(16), (B, 1)))


# ------------------------------------------------------------------ 5: independence, determinism, edges
def test_segments_are_independent_and_runs_repeat(ctx, street):
    from pointcloudprocess_amd import ops
    s = street.s
    B = len(pr.STREET_SIZES)
    perm = list(range(B))[::-1]
    off = pr.offsets([pr.STREET_SIZES[p] for p in perm])
    q = np.concatenate([s.q[s.off[p]:s.off[p + 1]] for p in perm])
    b = ops.ICPBatch(street.index, _dev(ctx, q), off)
    T_dev, stats = b.new_poses(s.T0[perm])
    keys = b.keys_dev(T_dev, RMAX)
    acc = b.accumulate(T_dev, keys, street.dtgt).cpu().numpy()
    b.run_dev(street.dtgt, T_dev, stats, RMAX, ITERS)
    T, st = T_dev.cpu().numpy().reshape(-1, 4, 4), stats.cpu().numpy()
    b.close()
    first, final = street.steps[0], street.steps[-1]
    assert np.array_equal(_bits(acc), _bits(first["acc"][perm]))
    assert np.array_equal(_bits(T), _bits(final["T"][perm])) and np.array_equal(_bits(st), _bits(final["stats"][perm]))
    # a second accumulation of the same keys: the same bits
    T0_dev, _ = street.batch.new_poses(s.T0)
    k0 = _dev(ctx, first["keys"])
    for _ in range(2):
        again = street.batch.accumulate(T0_dev, k0, street.dtgt).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(first["acc"]))
    # a batch of one segment gives that segment's row
    for p in (4, 6):
        b1 = ops.ICPBatch(street.index, street.dq[int(s.off[p]):int(s.off[p + 1])], [0, pr.STREET_SIZES[p]])
        T1, _ = b1.new_poses(s.T0[p])
        a1 = b1.accumulate(T1, b1.keys_dev(T1, RMAX), street.dtgt).cpu().numpy()
        b1.close()
        assert np.array_equal(_bits(a1[0]), _bits(first["acc"][p])), p


def test_skipped_keys_and_target_strides(ctx, street):
    """NO_KEY and an index at or past n_target are skipped; a wide target stride reads the same points."""
    s = street.s
    first = street.steps[0]
    T0_dev, _ = street.batch.new_poses(s.T0)
    keys = first["keys"].copy()
    keys[int(s.off[6]) + 5::7] = NO_KEY
    half = 15000
    exp = pr.batch_accumulate(s.T0, s.q, s.off, keys, s.tgt[:half])
    j = keys.view(np.uint64) & np.uint64(0xFFFFFFFF)
    assert ((keys != NO_KEY) & (j >= half)).sum() > 1000 and exp[:, 0].sum() > 1000
    got = street.batch.accumulate(T0_dev, _dev(ctx, keys), street.dtgt[:half]).cpu().numpy()
    for k in range(len(pr.STREET_SIZES)):
        assert got[k, 0] == exp[k, 0] and _close(got[k], exp[k]), k
    wide = torch.full((len(s.tgt), 5), 7.5, dtype=torch.float32, device=ctx.device)
    wide[:, :3] = street.dtgt
    got_w = street.batch.accumulate(T0_dev, _dev(ctx, first["keys"]), wide[:, :3]).cpu().numpy()
    assert np.array_equal(_bits(got_w), _bits(first["acc"]))
    T_dev, stats = street.batch.new_poses(s.T0)
    street.batch.run_dev(wide[:, :3], T_dev, stats, RMAX, ITERS)
    assert np.array_equal(_bits(T_dev.cpu().numpy().reshape(-1, 4, 4)), _bits(street.steps[-1]["T"]))


def test_argument_checks_empty_batches_and_balance(ctx, street):
    from pointcloudprocess_amd import ops
    lib, b, s = ctx.lib, street.batch, street.s
    p = lambda t: C.c_void_p(t.data_ptr())
    B, nq, nt = len(pr.STREET_SIZES), len(s.q), len(s.tgt)
    T_dev, stats = b.new_poses(s.T0)
    keys = torch.full((nq,), NO_KEY, dtype=torch.int64, device=ctx.device)
    acc = torch.full((B, 24), 55.0, dtype=torch.float64, device=ctx.device)
    trim = torch.full((B, 4), 77, dtype=torch.int64, device=ctx.device)
    nan, inf = float("nan"), float("inf")
    before = ctx.alloc_stats()[0]

    def reject(fn, good, bads):
        for pos, bad in bads:
            args = list(good)
            args[pos] = bad
            assert fn(*args) == -1, (fn.__name__, pos, bad)
            assert ctx.alloc_stats()[0] == before

    tgt = [(2, None), (3, 10), (3, 8), (3, 14), (4, -1)]  # positions in the loops' argument lists
    reject(lib.pcp_icp_batch_accumulate, [ctx.h, b.h, p(T_dev), p(keys), p(street.dtgt), 12, nt, p(acc)],
           [(0, None), (1, None), (2, None), (3, None), (4, None), (5, 10), (5, 8), (5, 14), (6, -1), (7, None)])
    reject(lib.pcp_icp_batch_solve_dev, [ctx.h, p(acc), B, 0, p(T_dev), p(stats)],
           [(0, None), (1, None), (2, -1), (2, 65536), (4, None), (5, None)])
    reject(lib.pcp_icp_batch_run_dev, [ctx.h, b.h, p(street.dtgt), 12, nt, p(T_dev), RMAX, 1, 0, p(stats)],
           [(0, None), (1, None), (5, None), (9, None), (6, -1.0), (6, nan), (7, -1)] + tgt
           + [(4, nt - 1), (4, nt + 1)])  # last: a target that is not the index's size
    assert b"target points" in lib.pcp_last_error(ctx.h)
    scalars = [(7, -0.01), (7, 1.5), (7, nan), (8, -1.0), (8, inf), (8, nan), (9, -0.1), (9, inf), (9, nan)]
    reject(lib.pcp_icp_batch_run_trimmed_dev,
           [ctx.h, b.h, p(street.dtgt), 12, nt, p(T_dev), RMAX, 0.5, 1.0, 0.0, 1, 0, p(stats), p(trim)],
           [(0, None), (1, None), (5, None), (12, None), (13, None), (6, -1.0), (6, nan), (10, -1), (4, nt - 1)]
           + tgt + scalars)
    ctx.sync()
    # a rejected call writes nothing
    assert (acc.cpu().numpy() == 55.0).all() and (trim.cpu().numpy() == 77).all() and stats.cpu().numpy().max() == 0
    assert np.array_equal(T_dev.cpu().numpy().reshape(-1, 4, 4), s.T0)
    # stride 0 = 12
    k0 = _dev(ctx, street.steps[0]["keys"])
    assert lib.pcp_icp_batch_accumulate(ctx.h, b.h, p(T_dev), p(k0), p(street.dtgt), 0, nt, p(acc)) == 0
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(street.steps[0]["acc"]))
    assert ctx.alloc_stats()[0] == before

    # nseg == 0 returns PCP_OK and writes nothing; null pointers are legal there
    e3 = torch.zeros((0, 3), dtype=torch.float32, device=ctx.device)
    b0 = ops.ICPBatch(street.index, e3, [0])
    mid = ctx.alloc_stats()[0]
    assert lib.pcp_icp_batch_accumulate(ctx.h, b0.h, None, None, p(street.dtgt), 12, nt, None) == 0
    assert lib.pcp_icp_batch_solve_dev(ctx.h, None, 0, 0, None, None) == 0
    assert lib.pcp_icp_batch_run_dev(ctx.h, b0.h, p(street.dtgt), 12, nt, None, RMAX, 2, 0, None) == 0
    assert lib.pcp_icp_batch_run_trimmed_dev(ctx.h, b0.h, p(street.dtgt), 12, nt, None, RMAX, 0.5, 1.0, 0.0, 2, 1,
                                             None, None) == 0
    T0, s0 = b0.new_poses()
    assert b0.accumulate(T0, b0.keys_dev(T0, RMAX), street.dtgt).shape == (0, 24)
    assert b0.run_trimmed_dev(street.dtgt, T0, s0, RMAX, 0.5, iters=2).numel() == 0
    assert ctx.alloc_stats()[0] == mid
    b0.close()
    # three empty segments: zero rows, every solve refused, the trim's rows of an empty segment
    be = ops.ICPBatch(street.index, e3, [0, 0, 0, 0])
    Te, se = be.new_poses()
    acc_e = torch.full((3, 24), 5.0, dtype=torch.float64, device=ctx.device)
    be.accumulate(Te, be.keys_dev(Te, RMAX), street.dtgt, acc=acc_e)
    assert np.array_equal(acc_e.cpu().numpy(), np.zeros((3, 24)))
    be.run_dev(street.dtgt, Te, se, RMAX, 2)
    assert np.array_equal(se.cpu().numpy(), np.tile([-1.0, 0, 0, 0], (3, 1)))
    assert np.array_equal(Te.cpu().numpy(), np.tile(np.eye(4).reshape(16), (3, 1)))
    Te, se = be.new_poses()
    rows = be.run_trimmed_dev(street.dtgt, Te, se, RMAX, 0.5, 2.0, 0.5, iters=2, do_scale=True)
    f2 = int(np.array([np.float32(0.5) * np.float32(0.5)], dtype=np.float32).view(np.uint32)[0])
    assert rows.cpu().numpy().tolist() == [[0, 0, 0, f2]] * 3
    assert np.array_equal(se.cpu().numpy(), np.tile([-1.0, 0, 0, 0], (3, 1)))
    be.close()
    ctx.sync()
    assert ctx.alloc_stats()[0] == before
