"""CPU checks around the batched get_rot_icp (include/pcp.h, V pcp_minmax_segments_aos48 and I5d): the
numpy reference tests/rot_batch_ref.py against plain matrix algebra, the conditions the GPU tests rely
on in its scene, the presence of the two entries in the header, the library and the binding (libpcp.so
loads without a GPU), and the C++ shim's new method through a compiler's syntax pass."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rot_batch_ref as rb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pcp_minmax_segments_aos48", "pcp_get_rot_icp_batch"]


def test_new_entries_declared_exported_bound():
    from pointcloudprocess_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "pcp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/pcp.h"
        assert re.search(r" T %s$" % name, nm, flags=re.M), f"{name} is not exported"
        assert name in bound and getattr(lib, name).argtypes is not None
    assert callable(ops.minmax_segments) and callable(ops.get_rot_icp_batch)
    # a null context is rejected before anything else is read
    off = (C.c_int64 * 1)(0)
    assert lib.pcp_minmax_segments_aos48(None, None, 0, off, 0, 1, None, None, None) == -1
    assert lib.pcp_get_rot_icp_batch(None, None, 0, 1, None, 0, 1, off, 0, None, 0.5, 1, 0, None, 0.0, None, None,
                                     None, None) == -1


def test_reference_arithmetic():
    from pointcloudprocess_amd import synth
    rng = np.random.default_rng(3)
    T = rb.conj(synth.rigid(0.7, -0.2, 0.3, (0.1, -0.2, 0.05)))
    p = rng.uniform(-25, 25, (500, 3)) + rb.OFF
    hom = np.concatenate([p, np.ones((500, 1))], axis=1) @ T.T
    got = rb.xform(T, p)
    # three products and three sums of terms up to |R p| + |t|: a few ulps of 1e4
    assert np.abs(got - hom[:, :3]).max() <= 8 * rb.EPS * 1e4
    # the identity leaves finite points as they are, and a non-dense cloud's non-finite points too
    assert np.array_equal(rb.xform(np.eye(4), p), p)
    q = p.copy()
    q[7] = [np.nan, 1.0, 2.0]
    q[9] = [1.0, np.inf, 2.0]
    nd = rb.xform(T, q, dense=False)
    assert np.array_equal(nd[[7, 9]], q[[7, 9]], equal_nan=True) and np.array_equal(np.delete(nd, [7, 9], 0),
                                                                                   np.delete(got, [7, 9], 0))
    assert not np.isfinite(rb.xform(T, q, dense=True)[[7, 9]]).all(axis=1).any()
    # staging: float32 of the centred point; the un-centring undoes the centring of a pose
    c = np.append(p.mean(axis=0), 0.0)
    st = rb.stage(T, p, c)
    assert st.dtype == np.float32 and np.abs(st - (got - c[:3])).max() <= 2.0 ** -24 * 64
    M = synth.rigid(0.2, 0.1, -0.1, (0.03, 0.02, -0.01))
    U = rb.uncentre(M, c)
    want = np.eye(4)
    want[:3, :3] = M[:3, :3]
    want[:3, 3] = M[:3, 3] - M[:3, :3] @ c[:3] + c[:3]
    assert np.array_equal(U[:, :3], M[:, :3]) and (np.abs(U[:3, 3] - want[:3, 3]) <= rb.uncentre_bound(M, c)).all()
    assert np.array_equal(rb.uncentre(np.eye(4), c), np.eye(4))
    # min / max rows: the DBL_MAX / DBL_MIN starts survive an empty and an all-negative segment
    mn, mx = rb.minmax_rows(np.zeros((0, 4)), T)
    assert (mn == rb.DBL_MAX).all() and (mx == rb.DBL_MIN).all()
    neg = -rng.uniform(1, 2, (10, 4))
    mn, mx = rb.minmax_rows(neg, np.eye(4))
    assert (mx == rb.DBL_MIN).all() and np.array_equal(mn, neg.min(axis=0))
    xyzw = np.concatenate([q, rng.uniform(-1, 1, (500, 1))], axis=1)
    mn, mx = rb.minmax_rows(xyzw, T, dense=False)
    keep = np.delete(np.arange(500), [7, 9])
    assert np.array_equal(mn[:3], got[keep].min(axis=0)) and np.array_equal(mx[3], xyzw[keep, 3].max())


def test_scene_conditions():
    """What tests/test_gpu_rot_icp_batch.py relies on: the frames moved by their start poses lie
    inside the target's box grown by rmax, at most rmax-ish from where the truth puts them, and the
    start poses differ from frame to frame and from the truth."""
    s = rb.scene()
    assert [len(g) for g in s.segs] == rb.SIZES and s.off[-1] == len(s.frames)
    lo, hi = s.tgt.min(axis=0), s.tgt.max(axis=0)
    for k, seg in enumerate(s.segs):
        if not len(seg):
            continue
        moved = rb.xform(s.T0[k], seg)
        truth = rb.xform(s.T_true[k], seg)
        gap = np.linalg.norm(moved - truth, axis=1)
        assert gap.max() < 0.45 and (len(seg) < 1000 or gap.max() > 0.02), (k, gap.max())
        assert (truth >= lo - 0.5).all() and (truth <= hi + 0.5).all(), k
    assert len({s.T0[k].tobytes() for k in range(len(rb.SIZES))}) == len(rb.SIZES)
    c = s.tgt.mean(axis=0)
    assert np.abs(c - rb.OFF).max() < 5.0  # the centroid is inside the scene: fp32 spacing there is <= 2^-19 m


SHIM_TU = r"""
#include <vector>
#include "pcp_pcl.hpp"
struct Mat4 {
    double v[16];
    double& operator()(int r, int c) { return v[4 * r + c]; }
    double operator()(int r, int c) const { return v[4 * r + c]; }
};
bool use(cloud_blend_double::CloudPtr cache, const std::vector<cloud_blend_double::CloudPtr>& frames,
         const std::vector<Mat4>& T0s, std::vector<Mat4>& rots, std::vector<float>& errs) {
    return cloud_blend_double::PointCloudHelper::get_rot_icp_batch(cache, frames, T0s, rots, errs, 20, 0.25f);
}
"""


def test_shim_method_instantiates(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler found for the shim's syntax pass")
    tu = tmp_path / "shim_rot_batch.cpp"
    tu.write_text(SHIM_TU)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
