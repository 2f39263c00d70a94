"""callers.do_mul_frame_icp(..., is_do_sep_icp=True, sep_batch=True): the per-frame registrations
through ops.minmax_segments and ops.get_rot_icp_batch (include/pcp.h, I5d) against the default
per-frame path, on the scene of test_callers.test_gpu_do_mul_frame_icp (sep=True, mul_seg=False).

  * the same stamps get a pose;
  * the joint (dis, rot) is the same code on the same input: identical;
  * per frame, e = RMS over the frame's points of |final p - T_true p| (T_true about the map offset)
    of the two paths agree within max(0.05 e_default, 2e-4 m), the bound of test_gpu_rot_icp_batch.py's
    recovery test.
"""
import numpy as np
import pytest

import oracle_ctypes as ora
import rot_batch_ref as rb

pytestmark = pytest.mark.gpu


def test_sep_batch_against_the_per_frame_path(tmp_path):
    from pointcloudprocess_amd import callers, cloudgrid, ops, pcd, synth
    ctx = ops.Context(0)
    T_true = synth.rigid(0.3, 0.1, -0.1, (0.06, -0.04, 0.02))
    tgt, q = synth.icp_pair(60_000, 60_000, 81, 82, T_true, extent=(40.0, 40.0))
    off = np.array([3512.25, -1801.5, 40.0])
    map_cloud = ora.make_cloud(tgt.double().numpy() + off)
    qx = q.double().numpy() + off
    order = np.argsort(qx[:, 0], kind="stable")  # frames = consecutive strips along x
    nfr = 10
    frames_xyz, stamp_file = {}, {}
    for i in range(nfr):
        st = 5000 + 10 * i
        frames_xyz[st] = qx[order[i::nfr][: len(order) // nfr]]
        path = tmp_path / f"{st}.pcd"
        pcd.save_pcd(str(path), ora.make_cloud(frames_xyz[st]))
        stamp_file[st] = str(path)
    errs = [0.05, 0.2, 0.05, 0.05, 0.0, 0.05, 0.3, 0.05, 0.05, 0.05]
    grid = cloudgrid.CloudGrid(ctx)
    grid.add_cloud_internal(ops.cloud_to_device(map_cloud, ctx.device))
    out = {}
    for batch in (False, True):
        line = [{"stamp": 5000 + 10 * i, "icperr": errs[i], "matrix": np.eye(4)} for i in range(nfr)]
        dis, rot = callers.do_mul_frame_icp(ctx, line, stamp_file, 4, 6, grid, 2, 0.1, is_do_sep_icp=True,
                                            is_mul_seg=False, sep_batch=batch)
        out[batch] = (dis, rot, {e["stamp"]: e["matrix"] for e in line if not np.array_equal(e["matrix"], np.eye(4))})
    (dis_a, rot_a, fin_a), (dis_b, rot_b, fin_b) = out[False], out[True]
    assert dis_a == dis_b and np.array_equal(rot_a, rot_b)
    assert sorted(fin_a) == sorted(fin_b) and len(fin_a) >= 5
    T_c = rb.conj(T_true, off)
    for st in sorted(fin_a):
        e_def = rb.rms_to_truth(fin_a[st], T_c, frames_xyz[st])
        e_bat = rb.rms_to_truth(fin_b[st], T_c, frames_xyz[st])
        print(f"stamp {st}: e_default {e_def:.6e} m  e_batch {e_bat:.6e} m  diff {abs(e_def - e_bat):.3e}")
        assert not np.array_equal(fin_b[st], rot_b), st  # the frame was registered, not just given the joint pose
        assert abs(e_bat - e_def) <= max(0.05 * e_def, 2e-4), (st, e_bat, e_def)
    grid.close()
    ctx.close()
