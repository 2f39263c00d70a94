"""CPU checks of batched registration (include/pcp.h, I5): the numpy reference
tests/icp_batch_ref.py on hand-made cases whose answers are known without it, and the presence of
the new entry points in the library, the binding and the ops layer."""
import numpy as np

import icp_batch_ref as bref
import icp_plane_ref as ref

NO_KEY = bref.NO_KEY


def _key(d2, j):
    return int((np.uint64(np.float32(d2).view(np.uint32)) << np.uint64(32)) | np.uint64(j))


def test_duplicate_targets_tie_goes_to_the_lower_index():
    tgt = np.float32([[5, 5, 5], [1, 0, 0], [9, 9, 9], [1, 0, 0], [1, 0, 0]])
    q = np.float32([[0.75, 0, 0]])
    k = bref.keys(np.eye(4), q, tgt, 0.5)
    assert k[0] == _key(0.0625, 1)
    # the same with the duplicates first in memory but the query equidistant from two distinct points
    tgt2 = np.float32([[2, 0, 0], [0, 0, 0], [1, 7, 7]])
    k2 = bref.keys(np.eye(4), np.float32([[1, 0, 0]]), tgt2, 1.5)
    assert k2[0] == _key(1.0, 0)


def test_distance_equal_to_rmax_is_accepted():
    tgt = np.float32([[0.5, 0, 0]])
    q = np.float32([[0, 0, 0]])
    assert bref.keys(np.eye(4), q, tgt, 0.5)[0] == _key(0.25, 0)      # d2 == r2 exactly
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert bref.keys(np.eye(4), q, tgt, below)[0] == NO_KEY            # one ulp less: rejected
    assert bref.keys(np.eye(4), np.float32([[0.5, 0, 0]]), tgt, 0.0)[0] == _key(0.0, 0)  # rmax = 0


def test_non_finite_queries_images_and_targets_have_no_key():
    tgt = np.float32([[0, 0, 0], [np.nan, 0, 0], [0.1, 0, 0]])
    q = np.float32([[np.nan, 0, 0], [0.09, 0, 0], [np.inf, 0, 0], [0, 0, 0]])
    k = bref.keys(np.eye(4), q, tgt, 0.5)
    assert k[0] == NO_KEY and k[2] == NO_KEY
    dx = np.float32(0.09) - np.float32(0.1)
    assert k[1] == _key(dx * dx, 2) and k[3] == _key(0.0, 0)  # never the NaN target
    T = np.eye(4)
    T[0, 3] = 3e38  # 3e38 + 3e38 overflows fp32: the image is not finite
    assert bref.keys(T, np.float32([[3e38, 0, 0]]), tgt, 0.5)[0] == NO_KEY


def test_pose_is_cast_to_fp32_and_chained_by_fma():
    T = np.eye(4)
    T[0, 0] = 1.0 + 2.0 ** -30           # rounds to 1.0f
    T[0, 3] = 0.1                          # rounds to fp32(0.1)
    q = np.float32([[3.0, 0, 0]])
    tgt = np.float32([[3.1, 0, 0]])
    qt = ref.transform_f32(T, q)
    assert qt[0, 0] == np.float32(np.float64(np.float32(0.1)) + 3.0)
    dx = qt[0, 0] - tgt[0, 0]
    assert bref.keys(T, q, tgt, 0.5)[0] == _key(dx * dx, 0)


def test_segment_boundaries_and_poses_are_respected():
    """Two segments of identical queries with different poses, an empty one between them: each
    query is matched under its own segment's pose only."""
    tgt = np.float32([[0, 0, 0], [10, 0, 0]])
    q = np.float32([[0.1, 0, 0], [0.2, 0, 0], [0.1, 0, 0], [0.2, 0, 0]])
    off = [0, 2, 2, 4]
    Ts = np.stack([np.eye(4)] * 3)
    Ts[2, 0, 3] = 10.0
    k = bref.batch_keys(Ts, q, off, tgt, 0.5)
    assert [int(v) & 0xFFFFFFFF for v in k] == [0, 0, 1, 1]
    Ts[2, 0, 3] = 5.0  # segment 2 now lands between the targets: no key, segment 0 unchanged
    k2 = bref.batch_keys(Ts, q, off, tgt, 0.5)
    assert list(k2[:2]) == list(k[:2]) and list(k2[2:]) == [NO_KEY, NO_KEY]


def test_step_solves_per_segment_and_latches_failures():
    """Segment 0: a well-posed set of pairs; segment 1: empty; segment 2: five pairs (< 6).  Only
    segment 0 moves; the others latch -1 and keep pose and stats."""
    rng = np.random.default_rng(3)
    pts = rng.uniform(-5, 5, (400, 3)).astype(np.float32)
    nrm = rng.normal(size=(400, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    from pointcloudprocess_amd import synth
    Tt = synth.rigid(0.3, 0.1, -0.2, t=(0.01, -0.02, 0.015))
    q0 = ((pts[:300].astype(np.float64) - Tt[:3, 3]) @ Tt[:3, :3]).astype(np.float32)
    q = np.concatenate([q0, pts[300:305]])
    off = [0, 300, 300, 305]
    keys = np.arange(305, dtype=np.int64)  # pair i <-> record i, d2 bits 0
    Ts = np.stack([np.eye(4)] * 3)
    stats = np.zeros((3, 4))
    acc, Tn, st = bref.batch_step(Ts, stats, q, off, keys, pts, nrm)
    assert acc[0, 0] == 300 and acc[1, 0] == 0 and acc[2, 0] == 5
    assert np.array_equal(acc[1], np.zeros(30))
    assert st[0, 0] == 0 and st[0, 3] == 1 and st[1, 0] == -1 and st[2, 0] == -1
    assert np.array_equal(Tn[1], np.eye(4)) and np.array_equal(Tn[2], np.eye(4))
    assert st[1, 3] == 0 and st[2, 3] == 0
    assert np.abs(Tn[0] - Tt).max() < 1e-4  # one linearised step from 0.3 deg away
    e0, _ = ref.accumulate(np.eye(4), q[:300], keys[:300], pts, nrm)
    assert np.array_equal(acc[0], e0)
    # a latched segment stays frozen even when its pairs become solvable
    acc2, Tn2, st2 = bref.batch_step(Tn, [[-1, 0, 0, 0]] * 3, q, off, keys, pts, nrm)
    assert np.array_equal(Tn2, Tn) and (st2[:, 0] == -1).all() and (st2[:, 3] == 0).all()


def test_batch_entry_points_are_exported():
    import re
    import subprocess
    from pointcloudprocess_amd import _lib, ops
    names = ["pcp_icp_batch_create", "pcp_icp_batch_destroy", "pcp_icp_batch_queries", "pcp_icp_batch_segments",
             "pcp_icp_batch_keys_dev", "pcp_icp_batch_accumulate_plane", "pcp_icp_batch_solve_plane_dev",
             "pcp_icp_batch_run_plane_dev"]
    lib = _lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pcp_[a-z0-9_]+)$", out, flags=re.M))
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for n in names:
        assert n in exported and n in bound and hasattr(lib, n), n
    for m in ("new_poses", "keys_dev", "accumulate_plane", "solve_plane_dev", "run_plane_dev", "close"):
        assert callable(getattr(ops.ICPBatch, m))
    # the null-handle rules need no device
    assert lib.pcp_icp_batch_destroy(None) == -1
    assert lib.pcp_icp_batch_queries(None) == -1 and lib.pcp_icp_batch_segments(None) == -1
