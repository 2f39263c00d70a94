"""The pilot step and the look-ahead of an ICP handle's first launch.

Before the first launch a Kabsch step over a strided sample of the sorted queries (the pilot), or
the caller's own prediction (pcp_icp_predict_first), gives the second pose T_1; the first launch
then caches around c = T_c q, T_c = T_0 + beta_0 (T_1 - T_0), while its own result stays the exact
winner at q_0.  Every launch must return exactly what the oracle returns whatever the prediction
is; only the number of later searches may change.  Every look-ahead search places its block from
q_t, so it sends no more queries to the fallback than beta = 0 does.

Scene and helpers: tests/test_gpu_icp_lookahead.py (a 4 m window of a 30 m tile, ~70k points a
side).  tools/sim_icp_pilot.py window=4 is the CPU model of the same scene
(profiles/pilot_sim/window4.txt).  The sampling tests use a line of cells with exactly 64 queries
per cell, so that chunk k of the sorted queries is cell k.
"""
import numpy as np
import pytest
import torch

import test_gpu_icp_lookahead as L

pytestmark = pytest.mark.gpu

RMAX, ITERS = L.RMAX, L.ITERS
A0, CAP0 = 1.5, 0.045  # kPilotAlpha, kPilotCap (icp.hip)


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


@pytest.fixture(scope="module")
def ref():
    return L.Ref()


def _first(ref):
    """The oracle's first step as a pose: poses[1] (poses[0] is the identity)."""
    return ref.poses[1]


def _run(ctx, ref, mode, q=None, poses=None, pred=None, **opts):
    """Host-pose launches at `poses` (the oracle's 20 by default), each checked against the oracle.
    mode: "pilot" (PCP_ICP_OPT_PILOT_ALWAYS), "off" (PCP_ICP_OPT_NO_PILOT), "predict"
    (pcp_icp_predict_first(pred), default the oracle's own second pose), "beta0" (no look-ahead at
    all).  Returns per-launch (beta, offset), searched, fallback and the pilot's info."""
    kw = dict(opts)
    if mode == "beta0":
        kw["lookahead"] = False
    else:
        kw["pilot"] = mode == "pilot"
    index, icp = L._engine(ctx, ref, q=q, **kw)
    if mode == "predict":
        icp.predict_first(_first(ref) if pred is None else pred)
    poses = ref.poses if poses is None else poses
    look, searched, fb = [], [], []
    for it, T in enumerate(poses):
        if q is None and poses is ref.poses:
            ei, ed, eacc = ref.corr[it][0], ref.corr[it][1], ref.acc[it]
        else:
            ei, ed, eacc = ref.at(T, q=q)
        L._check_launch(icp, T, ei, ed, eacc, f"{mode} {opts} launch {it}")
        look.append(icp.last_lookahead())
        searched.append(icp.last_searched())
        fb.append(icp.last_fallback())
    info = icp.pilot_info()
    icp.close()
    index.close()
    return look, searched, fb, info


def _check_beta0(mode, look, info, nq):
    b0, off0 = look[0]
    if mode == "pilot":
        nch = (nq + 63) // 64
        s = max(1, nch // 8192)
        assert info[0] == s and info[1] == (nch + s - 1) // s and info[2] > 0, info
    else:
        assert info == (0, 0, -1), info
    if mode in ("pilot", "predict"):
        assert 0.0 < b0 <= A0 and 0.0 < off0 <= CAP0 * 1.001, (b0, off0)
    else:
        assert b0 == 0.0 and off0 == 0.0, (b0, off0)
    assert look[1] == (0.0, 0.0), look[1]  # launch 1 has no ratio yet: plain


CASES = [("pilot", {}), ("off", {}), ("predict", {}),
         ("pilot", dict(wide_cache=True)), ("predict", dict(wide_cache=True)), ("off", dict(wide_cache=True)),
         ("pilot", dict(oct_lanes_first=2, oct_lanes_list=1)), ("pilot", dict(oct_lanes_first=4, oct_lanes_list=2)),
         ("pilot", dict(oct_lanes_first=1, oct_lanes_list=4)), ("predict", dict(oct_lanes_first=2, oct_lanes_list=4)),
         ("predict", dict(oct_lanes_first=4, oct_lanes_list=1)), ("off", dict(oct_lanes_first=4, oct_lanes_list=2))]


@pytest.mark.parametrize("mode,opts", CASES, ids=[f"{m}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'default'}"
                                                  for m, o in CASES])
def test_exact_every_launch(ctx, ref, mode, opts):
    """20 host-pose launches at the oracle's poses: indices and d2 bit-equal, accumulators within
    the existing tests' tolerance; beta_0 > 0 within the cap with the pilot or a prediction, 0
    without; both cache forms, 1, 2 and 4 lanes at the first launch and on the lists."""
    look, searched, _, info = _run(ctx, ref, mode, **opts)
    assert searched[0] == len(ref.q)
    _check_beta0(mode, look, info, len(ref.q))


def test_device_loop(ctx, ref):
    """step_dev + solve_dev from the identity, the pilot on: the accumulators equal the oracle's at
    every pose the loop visits, the poses are the oracle's own registration, beta_0 > 0.  The pilot's
    predicted second pose is close to the real one: the offset is the whole cap or a_0 steps.
    keys_dev launches (the loops that minimise something else) run no pilot, but take a prediction."""
    index, icp = L._engine(ctx, ref, pilot=True)
    T_dev, stats = icp.new_pose()
    look = []
    for it in range(ITERS):
        T = T_dev.cpu().numpy().reshape(4, 4).copy()
        gacc = icp.step_dev(T_dev, RMAX).cpu().numpy().copy()
        look.append(icp.last_lookahead())
        _, _, eacc = ref.at(T)
        assert gacc[0] == eacc[0], f"iteration {it}"
        assert np.allclose(gacc[:23], eacc[:23], rtol=1e-7, atol=1e-8 * np.abs(eacc[:23]).max()), f"iteration {it}"
        assert np.abs(T - ref.poses[it]).max() < 1e-5, f"iteration {it}"
        icp.solve_dev(icp.acc, T_dev, stats)
    _check_beta0("pilot", look, icp.pilot_info(), len(ref.q))
    assert max(b for b, _ in look[2:]) > 0.0, look
    icp.close()
    index.close()
    none = np.int64(0x7fffffffffffffff)
    for predict in (False, True):
        index, icp = L._engine(ctx, ref, pilot=True)
        if predict:
            icp.predict_first(_first(ref))
        T_dev, _ = icp.new_pose()
        for it, T in enumerate(ref.poses[:6]):
            T_dev.copy_(torch.from_numpy(T.reshape(16)))
            keys = icp.keys_dev(T_dev, RMAX).cpu().numpy()
            ei, ed = ref.corr[it]
            ek = np.where(ei >= 0, (ed.view(np.uint32).astype(np.int64) << 32) | ei.astype(np.int64), none)
            assert np.array_equal(keys, ek), f"keys_dev predict={predict} iteration {it}"
            if it == 0:
                assert (icp.last_lookahead()[0] > 0.0) == predict
                assert icp.pilot_info() == (0, 0, -1)
        icp.close()
        index.close()


def _wrong(name, ref):
    T1 = _first(ref)
    if name == "reversed":   # the first step taken backwards
        return np.linalg.inv(T1)
    if name == "jump":       # half a metre sideways
        return L._shift((0.5, 0, 0))
    if name == "far_axis":   # a rotation about an axis 9 m away
        return L._rot_about((9.0, 0.0, 0.0), 0.3)
    if name == "identity":   # no motion predicted: s_1 = 0
        return np.eye(4)
    if name == "nan":
        T = T1.copy()
        T[1, 3] = np.nan
        return T
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["reversed", "jump", "far_axis", "identity", "nan"])
def test_wrong_predictions_stay_exact(ctx, ref, name):
    """pcp_icp_predict_first with predictions that mislead the first launch: 8 launches bit-equal
    to the oracle.  No motion and a NaN give beta_0 = 0 (the plain first launch); the others look
    ahead, the wrong way, within the cap."""
    look, _, _, info = _run(ctx, ref, "predict", poses=ref.poses[:8], pred=_wrong(name, ref))
    assert info == (0, 0, -1)
    b0, off0 = look[0]
    if name in ("identity", "nan"):
        assert b0 == 0.0 and off0 == 0.0, look[0]
    else:
        assert 0.0 < b0 <= A0 and 0.0 < off0 <= CAP0 * 1.001, look[0]
        if name != "reversed":  # steps far above the cap: cut to it
            assert off0 > CAP0 * 0.999, look[0]


def test_predict_first_only_before_the_first_launch(ctx, ref):
    index, icp = L._engine(ctx, ref)
    icp.step(ref.poses[0], RMAX)
    with pytest.raises(Exception):
        icp.predict_first(_first(ref))
    icp.close()
    index.close()


def test_degenerate_pilots(ctx, ref):
    """Pilots that cannot predict: fewer than 64 queries; no query within rmax of the target (no
    pairs); 2 pairs on a target of 2 points (the solve is refused); every query non-finite.
    beta_0 = 0 wherever the solve is refused, and every launch equals the oracle."""
    # (40 neighbours, like a chunk of sorted queries: the accumulators' tolerance is for compact chunks)
    few = np.ascontiguousarray(ref.q[np.argsort(np.linalg.norm(ref.q - ref.q[0], axis=1))[:40]])
    look, _, _, info = _run(ctx, ref, "pilot", q=few, poses=ref.poses[:5])
    assert info[:2] == (1, 1) and 0 <= info[2] <= 40, info
    far = np.ascontiguousarray(ref.q[:5000] + np.float32([0, 0, 30.0]))
    look, _, _, info = _run(ctx, ref, "pilot", q=far, poses=ref.poses[:4])
    assert info == (1, (5000 + 63) // 64, 0) and look[0] == (0.0, 0.0), (info, look[0])

    class Two:  # a target of 2 points, 2 queries beside them and the rest out of reach
        tgt = np.ascontiguousarray(ref.tgt[[10, 20000]])
        oi = L.ora.F32Index(tgt)
    two = Two()
    q2 = np.concatenate([two.tgt + np.float32(0.01), ref.q[:200] + np.float32([0, 0, 30.0])]).astype(np.float32)
    index, icp = L._engine(ctx, two, q=np.ascontiguousarray(q2), pilot=True)
    for it, T in enumerate([np.eye(4), L._shift((0.004, 0, 0)), L._shift((0.006, 0, 0))]):
        ei, ed = two.oi.correspond(q2, T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32), RMAX)
        L._check_launch(icp, T, ei, ed, None, f"two-point target launch {it}")
        if it == 0:
            assert (ei >= 0).sum() == 2
            assert icp.pilot_info() == (1, 4, 2) and icp.last_lookahead() == (0.0, 0.0)
    icp.close()
    index.close()

    qn = np.full((300, 3), np.nan, np.float32)
    index, icp = L._engine(ctx, ref, q=qn, pilot=True)
    _, ci, _ = icp.step(np.eye(4), RMAX, corr=True)
    assert (ci.cpu().numpy() == -1).all()
    assert icp.pilot_info() == (0, 0, -1) and icp.last_lookahead() == (0.0, 0.0)
    icp.close()
    index.close()


# ---- sampling: a line of cells along x, exactly 64 queries per cell, so chunk k = cell k
H, R_LINE = 0.12, 0.05


def _line(ncells, nq, targets):
    """Targets: one per cell of `targets` (a boolean per cell) 1 cm above that cell's queries, plus
    the two end points that fix the grid's box; nq queries, 64 per cell from cell 0 on."""
    k = np.arange(ncells)
    x = ((k + 0.75) * H).astype(np.float32)
    keep = np.asarray(targets, bool)
    tgt = np.stack([x[keep], np.full(keep.sum(), 0.01, np.float32), np.zeros(keep.sum(), np.float32)], 1)
    ends = np.float32([[0, 0, 0], [(ncells + 1) * H, 0.02, 0.02]])
    q = np.zeros((nq, 3), np.float32)
    q[:, 0] = x[np.arange(nq) // 64]
    return np.ascontiguousarray(np.concatenate([ends, tgt]).astype(np.float32)), q


def _pilot_pairs(ctx, tgt, q):
    from pointcloudprocess_amd import ops
    index = ops.GridIndex(ctx, torch.from_numpy(tgt).to(ctx.device), cell_size=H)
    icp = ops.ICP(index, torch.from_numpy(q).to(ctx.device))
    icp.set_options(pilot=True)
    acc = icp.step(np.eye(4), R_LINE).cpu().numpy()
    info, look = icp.pilot_info(), icp.last_lookahead()
    icp.close()
    index.close()
    return info, look, acc[0]


@pytest.mark.parametrize("nq", [64, 64 * 8191, 64 * 8192, 64 * 8193 - 5, 64 * 16383, 64 * 16384, 64 * 16385,
                                64 * 16384 + 17, 64 * 24577 - 1])
def test_sampling_visits_the_chunks_of_the_rule(ctx, nq):
    """Chunk counts 1, 8191, 8192, 8193 (a partial last chunk), 16383 (stride 1), 16384, 16385
    (stride 2), 16385 with 17 queries in the last, 24577 (stride 3, partial): with a target beside
    every query the pilot's pair count is the number of queries in chunks 0, S, 2S, ...; with
    targets beside the sampled cells only it is the same, and beside the other cells only it is 0
    (then beta_0 = 0), so exactly those chunks were visited."""
    nch = (nq + 63) // 64
    s = max(1, nch // 8192)
    sampled = np.arange(0, nch, s)
    want = int(np.minimum(64, nq - 64 * sampled).sum())
    on_rule = np.zeros(nch, bool)
    on_rule[sampled] = True
    for name, targets, pairs in (("every cell", np.ones(nch, bool), want), ("sampled cells", on_rule, want),
                                 ("other cells", ~on_rule, 0)):
        if not targets.any():
            continue
        tgt, q = _line(nch, nq, targets)
        info, look, n_acc = _pilot_pairs(ctx, tgt, q)
        assert info == (s, len(sampled), pairs), (name, info, (s, len(sampled), pairs))
        assert n_acc == targets[np.arange(nq) // 64].sum(), name  # the launch itself pairs every query it can
        if pairs == 0:
            assert look == (0.0, 0.0), (name, look)


def test_unsampled_targets_register_like_no_pilot(ctx):
    """Stride 2 with targets beside the odd cells only: the pilot finds no pair, beta_0 = 0, and a
    short registration is the one of a handle without the pilot, bit for bit."""
    from pointcloudprocess_amd import ops
    nch = 16384
    tgt, q = _line(nch, 64 * nch, np.arange(nch) % 2 == 1)
    q = q + np.float32([0.004, 0.002, 0])
    out = []
    for pilot in (True, False):
        index = ops.GridIndex(ctx, torch.from_numpy(tgt).to(ctx.device), cell_size=H)
        icp = ops.ICP(index, torch.from_numpy(q).to(ctx.device))
        icp.set_options(pilot=pilot)
        err, T = icp.run(np.eye(4), R_LINE, 4)
        out.append((err, T, icp.pilot_info()))
        icp.close()
        index.close()
    assert out[0][2] == (2, 8192, 0) and out[1][2] == (0, 0, -1)
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


def test_fewer_searches_and_no_extra_fallback(ctx, ref):
    """On the window scene the queries searched at launches 1 and 2 with the pilot are below 0.7 x
    those without (the model: 0.54 x at cap_0 30 mm, 0.32 x at the engine's 45 mm, profiles/pilot_sim/window4.txt; measured 0.55 x at 30 mm), and the look-ahead launches
    2..5 send no more than 1.1 x the queries to the fallback that a beta = 0 registration sends
    (the model: equal, since the block is placed from q_t)."""
    n = len(ref.q)
    on = _run(ctx, ref, "pilot", poses=ref.poses[:8])
    off = _run(ctx, ref, "off", poses=ref.poses[:8])
    b0 = _run(ctx, ref, "beta0", poses=ref.poses[:8])
    for name, r in (("pilot", on), ("no pilot", off), ("beta = 0", b0)):
        print(f"{name:9s} searched " + " ".join(f"{s / n:.3f}" for s in r[1]) +
              "  fallback " + " ".join(f"{f / n:.4f}" for f in r[2]))
    s_on, s_off = sum(on[1][1:3]), sum(off[1][1:3])
    assert s_on < 0.7 * s_off, (s_on / n, s_off / n)
    for r in (on, off):
        assert max(b for b, _ in r[0][2:6]) > 0.0  # the launches compared do look ahead
        assert sum(r[2][2:6]) <= 1.1 * sum(b0[2][2:6]), (r[2][2:6], b0[2][2:6])
