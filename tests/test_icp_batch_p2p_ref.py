"""CPU checks of the point-to-point batch reference (tests/icp_batch_p2p_ref.py) and of the two
scenes tests/test_gpu_icp_batch_p2p.py uses: what those tests take for granted -- exact lattice
arithmetic, which segments solve, how well conditioned their solves are -- is asserted here, from
the numpy reference alone, before a GPU is involved."""
import numpy as np
import pytest

import icp_batch_p2p_ref as pr
import icp_plane_ref as ref
import kabsch_ref as kr

NO_KEY = pr.NO_KEY


def _key(d2, j):
    return int((np.uint64(np.float32(d2).view(np.uint32)) << np.uint64(32)) | np.uint64(j))


def test_accumulate_skips_no_key_and_indices_past_the_target():
    tgt = np.float32([[1, 0, 0], [0, 2, 0], [0, 0, 4]])
    q = np.float32([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]])
    keys = np.array([_key(0.25, 2), NO_KEY, _key(0.5, 3), _key(1.0, 0)], dtype=np.int64)  # index 3: past the end
    T = np.eye(4)
    T[:3, 3] = [0.5, 0.0, -1.0]
    acc, info = pr.accumulate(T, q, keys, tgt)
    qi = np.array([[1.5, 1.0, 0.0], [4.5, 4.0, 3.0]])
    p = np.array([[0.0, 0.0, 4.0], [1.0, 0.0, 0.0]])
    assert acc[0] == 2 and acc[23] == 0 and acc[22] == 1.25 and info["exact64"]
    assert np.array_equal(acc[1:4], qi.sum(0)) and np.array_equal(acc[4:7], p.sum(0))
    assert np.array_equal(acc[7:16].reshape(3, 3), qi.T @ p)
    assert np.array_equal(acc[16:22], [(qi[:, a] * qi[:, b]).sum() for a, b in kr._TRI])
    assert np.array_equal(pr.accumulate(T, q[:0], keys[:0], tgt)[0], np.zeros(24))  # an empty segment


def test_step_solves_per_segment_and_latches_refusals():
    """Segment 0: 200 pairs of a known motion; segment 1: empty; segment 2: two pairs.  Only segment
    0 moves; a latched segment stays frozen when its pairs become solvable."""
    from pointcloudprocess_amd import synth
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-5, 5, (300, 3)).astype(np.float32)
    Tt = synth.rigid(3.0, 1.0, -2.0, t=(0.3, -0.2, 0.1))
    q0 = ((tgt[:200].astype(np.float64) - Tt[:3, 3]) @ Tt[:3, :3]).astype(np.float32)
    q = np.concatenate([q0, tgt[200:202]])
    off = [0, 200, 200, 202]
    keys = np.arange(202, dtype=np.int64)  # pair i <-> target i, d2 bits 0
    acc, Tn, st, sols = pr.batch_step(np.stack([np.eye(4)] * 3), np.zeros((3, 4)), q, off, keys, tgt)
    assert acc[:, 0].tolist() == [200, 0, 2] and np.array_equal(acc[1], np.zeros(24))
    assert st[:, 0].tolist() == [0, -1, -1] and st[:, 3].tolist() == [1, 0, 0]
    assert np.array_equal(Tn[1], np.eye(4)) and np.array_equal(Tn[2], np.eye(4))
    assert np.abs(Tn[0] - Tt).max() < 1e-5 and sols[1] is None and sols[2] is None
    for do_scale in (False, True):  # the library's host solve agrees on the same sums
        from pointcloudprocess_amd import ops
        rc, dT = ops.icp_solve(acc[0], do_scale)
        assert rc == 0 and np.abs(dT - pr.batch_step(np.stack([np.eye(4)] * 3), np.zeros((3, 4)), q, off, keys, tgt,
                                                     do_scale)[1][0]).max() < 1e-9
    _, Tn2, st2, _ = pr.batch_step(Tn, [[-1, 0, 0, 0]] * 3, q, off, keys, tgt)
    assert np.array_equal(Tn2, Tn) and (st2[:, 0] == -1).all() and (st2[:, 3] == 0).all()


@pytest.mark.parametrize("cell,rmax", pr.LATTICE_RUNS)
def test_lattice_scene_is_exact(cell, rmax):
    """Every fp32 step of the pose chain and of d2 is exact, every exact sum is a float64 and every
    partial sum of un-centred fp64 terms stays below 2^53: any summation order gives the same
    doubles.  Every segment but the empty one has pairs, the larger ones also queries without."""
    s = pr.lattice_scene()
    assert s.sizes == [0, 1, 2, 3, 63, 64, 68, 255, 256, 257, 2049, 4503]
    exp = pr.lattice_expected(rmax)
    pairs = []
    for k, (keys, acc, info, exact_pose, exact_d2) in enumerate(exp):
        assert exact_pose and exact_d2 and info["exact64"] and info["fp32"], k
        assert info["bound64"] < 2 ** 53 and info["k"] <= 5, (k, info)
        q = s.q[s.off[k]:s.off[k + 1]]
        assert (keys[~np.isfinite(q).all(1)] == NO_KEY).all()
        assert acc[0] == (keys != NO_KEY).sum() and acc[23] == 0
        # the batch reference (its own exhaustive search and fmaf emulation) finds the same keys
        assert np.array_equal(pr.bref.keys(s.Ts[k], q, s.tgt, rmax), keys), k
        assert np.array_equal(pr.accumulate(s.Ts[k], q, keys, s.tgt)[0], acc), k
        pairs.append(int(acc[0]))
    print("pairs per segment:", pairs)
    assert pairs[0] == 0 and pairs[1:4] == [1, 2, 3]
    assert all(0 < pairs[k] < pr.LATTICE_SIZES[k] for k in range(4, 12)), pairs
    if rmax == 0.25:
        assert pairs == [0, 1, 2, 3, 47, 49, 47, 174, 183, 180, 1436, 3078]


@pytest.mark.slow
def test_street_scene_conditions():
    """Four reference iterations on the street scene: segments 0 and 1 refuse at every step, every
    other segment solves at every step with at most a quarter of its queries unkeyed and
    max|AB| / (s1 + det s2) <= 4; the fmaf emulations of the two references agree on every image;
    do_scale finds a scale within a thousandth of 1 on the first step's pairs."""
    s = pr.street_scene()
    assert len(s.tgt) == 30200 and len(s.q) == sum(pr.STREET_SIZES)
    steps = pr.run(s.T0, s.q, s.off, s.tgt, pr.STREET_RMAX, pr.STREET_ITERS)
    worst = [pr.check_street_step(st, it) for it, st in enumerate(steps)]
    print("largest unkeyed share %.3f, largest conditioning %.2f" % (max(w[0] for w in worst),
                                                                     max(w[1] for w in worst)))
    for st in steps:
        assert np.array_equal(st["acc"][0], np.zeros(24)) and st["acc"][1, 0] <= 1
        for k in range(len(pr.STREET_SIZES)):
            q = s.q[s.off[k]:s.off[k + 1]]
            assert np.array_equal(kr.xform32(st["T_prev"][k], q)[0], ref.transform_f32(st["T_prev"][k], q)), k
    final = steps[-1]["stats"]
    assert (final[2:, 3] == pr.STREET_ITERS).all() and (final[:2, 3] == 0).all()
    assert np.array_equal(steps[-1]["T"][:2], s.T0[:2])
    rms = np.array([st["stats"][2:, 1] for st in steps])
    assert (rms[-1] < rms[0]).all()  # every solving segment's pairs got closer
    _, _, st_s, sols = pr.batch_step(s.T0, np.zeros((len(pr.STREET_SIZES), 4)), s.q, s.off, steps[0]["keys"], s.tgt,
                                     do_scale=True)
    assert st_s[:, 0].tolist() == [-1, -1, 0, 0, 0, 0, 0, 0]
    assert all(abs(sol["sc"] - 1.0) < 1e-3 for sol in sols[2:])
    assert all(pr.conditioning(steps[0]["acc"][k], sols[k]) <= 4.0 for k in range(2, len(sols)))
