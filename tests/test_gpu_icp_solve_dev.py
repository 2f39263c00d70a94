"""The device build of the Kabsch / Umeyama solve (pcp_icp_solve_dev: one GPU thread running the
host solve's code) and the loops around it (MI355X): the case list and assertions of
test_icp_solve.py against kabsch_ref.solve, the stats contract, and the degenerate loops -- a
one-point target (rank 0 at every iteration), a planar and a collinear lattice scene -- whose
pose must stay a rigid motion."""
import numpy as np
import pytest
import torch

import kabsch_cases as kc
import kabsch_ref as kr

pytestmark = pytest.mark.gpu

CASES = kc.cases()


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


class Dev:
    """A device pose (identity) and zeroed stats; solve(acc) runs pcp_icp_solve_dev on them."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.T = torch.eye(4, dtype=torch.float64).reshape(16).to(ctx.device).contiguous()
        self.stats = torch.zeros(4, dtype=torch.float64, device=ctx.device)

    def solve(self, acc, do_scale=False):
        a = torch.from_numpy(np.ascontiguousarray(acc, dtype=np.float64)).to(self.ctx.device)
        self.ctx.check(self.ctx.lib.pcp_icp_solve_dev(self.ctx.h, a.data_ptr(), int(do_scale), self.T.data_ptr(),
                                                      self.stats.data_ptr()))
        self.ctx.sync()
        return self.T.cpu().numpy().reshape(4, 4).copy(), self.stats.cpu().numpy().copy()


@pytest.mark.parametrize("name,q,p,do_scale", CASES, ids=[c[0] for c in CASES])
def test_solve_dev_case(ctx, name, q, p, do_scale):
    acc = kr.acc24(q, p)
    acc[23] = 7.0
    dT, st = Dev(ctx).solve(acc, do_scale)  # T = dT * identity: dT itself
    assert st.tolist() == [0.0, np.sqrt(acc[22] / acc[0]), 7.0, 1.0]
    ran_c = kc.check_solution(name, q, p, do_scale, dT)
    assert ran_c == (name not in kc.NON_UNIQUE)
    if name in kc.RANK0_EXACT + kc.RANK0_NOISE:
        kc.check_rank0(name, q, p, dT)
        dT, _ = Dev(ctx).solve(acc, True)  # the scale of a rank-0 problem stays 1
        kc.check_rank0(name, q, p, dT)


def test_solve_dev_refuses_and_latches(ctx):
    """n < 3 or a non-finite accumulator: stats[0] = -1, T frozen, and every later call a no-op."""
    name, q, p, _ = CASES[0]
    good = kr.acc24(q, p)
    good[23] = 2.0
    for bname, bad in kc.bad_accumulators():
        d = Dev(ctx)
        T1, st1 = d.solve(good)
        assert st1[0] == 0 and st1[3] == 1 and st1[2] == 2.0
        T2, st2 = d.solve(bad)
        assert st2[0] == -1.0, bname
        assert np.array_equal(T2, T1) and st2[1] == st1[1] and st2[3] == 1.0, bname
        T3, st3 = d.solve(good)
        assert np.array_equal(T3, T1) and np.array_equal(st3, st2, equal_nan=True), bname


def test_stats_contract(ctx):
    """stats[1] = sqrt(acc[22] / acc[0]) of the last solved step, stats[2] the running sum of
    acc[23], stats[3] the solved steps; T <- dT * T."""
    d = Dev(ctx)
    T = np.eye(4)
    fb = 0.0
    for k, (name, q, p, do_scale) in enumerate(CASES[:4]):
        acc = kr.acc24(q, p)
        acc[23] = 3.0 + k
        fb += acc[23]
        Tn, st = d.solve(acc, do_scale)
        assert st.tolist() == [0.0, np.sqrt(acc[22] / acc[0]), fb, k + 1.0]
        dT = kr.solve(q, p, do_scale)["dT"]
        T = dT @ T
        assert np.abs(Tn - T).max() <= 4 * (k + 1) * kc.TOL_U * kc.EPS * np.abs(T).max()


def _rigid_error(T):
    R = T[:3, :3]
    return max(np.abs(R.T @ R - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0))


def test_one_point_target_loops_stay_rigid(ctx):
    """Every query within rmax of the only target point: S is zero (or the sums' rounding) at every
    iteration.  The pose keeps R = I, moves the queries' centroid onto the point, and the loops
    report success: run_dev (device solve) and run (host solve)."""
    from pointcloudprocess_amd import ops
    tgt = np.array([[1.5, -0.75, 0.25]], np.float32)
    rng = np.random.default_rng(3)
    q = (tgt + rng.integers(-3, 4, (5, 3)) / 32.0 + [0.125, 0.0, -0.0625]).astype(np.float32)
    index = ops.GridIndex(ctx, torch.from_numpy(tgt).to(ctx.device), cell_size=0.1)
    icp = ops.ICP(index, torch.from_numpy(q).to(ctx.device))
    T_dev, stats = icp.new_pose()
    icp.run_dev(T_dev, stats, 0.5, 3)
    st = stats.cpu().numpy()
    T = T_dev.cpu().numpy().reshape(4, 4)
    err, Th = icp.run(np.eye(4), 0.5, 3)
    for M in (T, Th):
        assert np.array_equal(M[:3, :3], np.eye(3)) and np.array_equal(M[3], [0, 0, 0, 1.0]), M
        assert np.abs(q.astype(np.float64).mean(0) + M[:3, 3] - tgt[0]).max() < 1e-6, M
    assert st[0] == 0 and st[3] == 3 and err >= 0
    icp.close()
    index.close()


@pytest.mark.parametrize("shape", ["planar", "collinear"])
def test_thin_scenes_stay_rigid_every_iteration(ctx, shape):
    """A planar and a collinear lattice scene (rank 2 and rank 1): the pose stays orthonormal with
    det +1 at every iteration of the device loop, and through the host loop."""
    from pointcloudprocess_amd import ops
    n = 20 if shape == "planar" else 1
    g = np.stack(np.meshgrid(np.arange(40), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    tgt = np.concatenate([g * 0.125, np.zeros((len(g), 1))], 1).astype(np.float32)
    c, s = np.cos(0.02), np.sin(0.02)
    q = (tgt.astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + [0.03, 0.02, 0.01]).astype(np.float32)
    index = ops.GridIndex(ctx, torch.from_numpy(tgt).to(ctx.device), cell_size=0.1)
    icp = ops.ICP(index, torch.from_numpy(q).to(ctx.device))
    T_dev, stats = icp.new_pose()
    for it in range(4):
        icp.solve_dev(icp.step_dev(T_dev, 0.25), T_dev, stats)
        T = T_dev.cpu().numpy().reshape(4, 4)
        assert _rigid_error(T) <= (it + 1) * kc.TOL_ORTHO, (it, T)
    st = stats.cpu().numpy()
    assert st[0] == 0 and st[3] == 4
    err, Th = icp.run(np.eye(4), 0.25, 4)
    assert err >= 0 and _rigid_error(Th) <= 4 * kc.TOL_ORTHO, Th
    icp.close()
    index.close()
