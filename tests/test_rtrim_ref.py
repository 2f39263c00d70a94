"""CPU checks around the trim by plane residual (include/pcp.h, I3b): the numpy reference
tests/rtrim_ref.py against a brute-force restatement (per pair, python floats, sort the usable rho
and pick the rank), its composition with the accumulation's reference, its invariance under negated
normals, the frac 0 / frac 1 / nothing-usable cases, the presence of the three entries in the
header, the library and the binding, the argument errors that return before any device call, and
the comparison tool tools/rtrim_reference.py (needs scipy)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import icp_plane_ref as ref
import rtrim_ref as rr
import trim_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCP_ERR_ARG = -1
NO_KEY = tr.NO_KEY
NEW = ["pcp_icp_trim_keys_plane", "pcp_icp_run_plane_rtrimmed_dev", "pcp_get_rot_icp_plane_rtrimmed"]


def _bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def _pose(rng):
    a = rng.uniform(-0.05, 0.05, 3)
    T = np.eye(4)
    T[:3, :3] = ref.rodrigues(a)
    T[:3, 3] = rng.uniform(-0.2, 0.2, 3)
    return T


def _random_case(rng, n, ntab=200):
    """A table with a zero, a NaN and a {0,0,0,1,..}-style record and a non-finite point, queries near
    their records' planes (residuals of centimetres to decimetres), keys with every kind of unusable
    pair: no key, index past the table (0xffffffff included), an invalid record, a NaN query."""
    pts = rng.uniform(-20, 20, (ntab, 3)).astype(np.float32)
    v = rng.normal(size=(ntab, 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    nrm[1] = 0
    nrm[2] = np.nan
    nrm[3] = [0.3, 0.2, 0.1]  # |n|^2 < 0.25
    pts[4, 1] = np.inf
    T = _pose(rng)
    j = rng.integers(0, ntab, n)
    off = rng.normal(size=(n, 3)) * rng.choice([0.01, 0.3], (n, 1))
    target = pts[j].astype(np.float64)
    target[~np.isfinite(target)] = 0.0
    q = ((target + off - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    d2 = (off ** 2).sum(1).astype(np.float32)
    keys = tr.make_keys(d2.view(np.uint32), j)
    kind = rng.random(n)
    keys[kind < 0.1] = NO_KEY
    past = (kind >= 0.1) & (kind < 0.15)
    keys[past] = tr.make_keys(d2[past].view(np.uint32), rng.choice([ntab, ntab + 7, 0xFFFFFFFF], int(past.sum())))
    q[(kind >= 0.15) & (kind < 0.18), rng.integers(0, 3)] = np.nan
    if rng.random() < 0.3:  # heavy ties: copies of one pair
        c = rng.integers(0, n)
        dup = rng.random(n) < 0.4
        q[dup], keys[dup] = q[c], keys[c]
    return T, q, keys, pts, nrm


def _brute(T, q, keys, pts, nrm, frac, mult, d_floor):
    """The contract restated pair by pair."""
    qt = ref.transform_f32(T, q)
    n = len(keys)
    rho = [None] * n
    for i in range(n):
        k = int(keys[i])
        if k == NO_KEY:
            continue
        j = k & 0xFFFFFFFF
        if j >= len(pts):
            continue
        nx, ny, nz = (np.float32(c) for c in nrm[j])
        with np.errstate(invalid="ignore", over="ignore"):
            n2 = (nx * nx + ny * ny) + nz * nz
        if not n2 >= np.float32(0.25) or not np.isfinite(pts[j]).all() or not np.isfinite(nrm[j]).all():
            continue
        p = [float(c) for c in pts[j]]
        x = [float(c) for c in qt[i]]
        r = (float(nx) * (x[0] - p[0]) + float(ny) * (x[1] - p[1])) + float(nz) * (x[2] - p[2])
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.float32(np.float64(r) * np.float64(r))
        if not math.isnan(v):
            rho[i] = v
    usable = sorted(_bits(v) for v in rho if v is not None)
    m = len(usable)
    sel = usable[int(math.floor(float(np.float32(frac)) * (m - 1)))] if m else 0
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        c = (np.float32(mult) * np.float32(mult)) * np.array([sel], dtype=np.uint32).view(np.float32)[0]
        f2 = np.float32(d_floor) * np.float32(d_floor)
    cut = f2 if (np.isnan(c) or not c > f2) else c
    out = np.full(n, NO_KEY, dtype=np.int64)
    kept = 0
    for i in range(n):
        if rho[i] is not None and rho[i] <= cut:
            out[i] = keys[i]
            kept += 1
    return out, [m, kept, sel, _bits(cut)]


def test_matches_brute_force():
    rng = np.random.default_rng(1)
    rejected = 0
    for it in range(60):
        n = int(rng.integers(1, 400))
        T, q, keys, pts, nrm = _random_case(rng, n)
        frac = [0.0, 1.0, float(rng.random())][rng.integers(0, 3)]
        mult = [1.0, float(rng.uniform(0, 3))][rng.integers(0, 2)]
        d_floor = [0.0, float(rng.uniform(0, 0.2))][rng.integers(0, 2)]
        out, stats = rr.rtrim(T, q, keys, pts, nrm, frac, mult, d_floor)
        eo, es = _brute(T, q, keys, pts, nrm, frac, mult, d_floor)
        assert stats.tolist() == es, (it, n, frac, mult, d_floor)
        assert np.array_equal(out, eo), (it, n, frac, mult, d_floor)
        rejected += int(es[1] < es[0])
    assert rejected > 20  # the cases do trim


def test_kept_equals_accumulated_pairs_and_keys_unchanged():
    rng = np.random.default_rng(2)
    for _ in range(20):
        T, q, keys, pts, nrm = _random_case(rng, 500)
        out, stats = rr.rtrim(T, q, keys, pts, nrm, 0.5, 1.5)
        acc, used = ref.accumulate(T, q, out, pts, nrm)
        assert acc[0] == int(stats[1]) == int((out != NO_KEY).sum())
        kept = out != NO_KEY
        assert np.array_equal(out[kept], keys[kept]) and np.array_equal(used, kept)
        # m counts what the accumulation would use, less the pairs with a NaN statistic
        acc_in, used_in = ref.accumulate(T, q, keys, pts, nrm)
        nan_q = np.isnan(q).any(1)
        assert int(stats[0]) == int((used_in & ~nan_q).sum())


def test_negated_normals_change_nothing():
    rng = np.random.default_rng(3)
    for _ in range(10):
        T, q, keys, pts, nrm = _random_case(rng, 500)
        a = rr.rtrim(T, q, keys, pts, nrm, 0.5, 2.0, 0.01)
        b = rr.rtrim(T, q, keys, pts, -nrm, 0.5, 2.0, 0.01)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(rr.residual_keys(T, q, keys, pts, nrm), rr.residual_keys(T, q, keys, pts, -nrm))


def test_frac_zero_and_one():
    rng = np.random.default_rng(4)
    T, q, keys, pts, nrm = _random_case(rng, 500)
    rk = rr.residual_keys(T, q, keys, pts, nrm)
    b = tr.high_words(rk[rk != NO_KEY])
    out, stats = rr.rtrim(T, q, keys, pts, nrm, 0.0)
    assert stats[0] == b.size and stats[2] == b.min() and stats[3] == b.min() and stats[1] == (b == b.min()).sum()
    out, stats = rr.rtrim(T, q, keys, pts, nrm, 1.0)
    assert stats[2] == b.max() and stats[1] == stats[0] == b.size
    assert np.array_equal(out != NO_KEY, rk != NO_KEY)  # every usable pair, and only those


def test_nothing_usable():
    rng = np.random.default_rng(5)
    T, q, keys, pts, nrm = _random_case(rng, 300)
    f2 = _bits(np.float32(0.5) * np.float32(0.5))
    cases = {
        "no keys": np.full(300, NO_KEY, dtype=np.int64),
        "indices past the table": tr.make_keys(tr.high_words(keys), np.full(300, len(pts))),
        "invalid records": tr.make_keys(tr.high_words(keys), rng.integers(1, 5, 300)),
    }
    for name, k in cases.items():
        out, stats = rr.rtrim(T, q, k, pts, nrm, 0.5, 2.0, 0.5)
        assert stats.tolist() == [0, 0, 0, f2] and (out == NO_KEY).all(), name
    out, stats = rr.rtrim(T, np.full_like(q, np.nan), keys, pts, nrm, 0.5, 2.0, 0.5)
    assert stats.tolist() == [0, 0, 0, f2] and (out == NO_KEY).all()
    out, stats = rr.rtrim(T, q[:0], keys[:0], pts, nrm, 0.5, 2.0, 0.5)
    assert out.size == 0 and stats.tolist() == [0, 0, 0, f2]


def test_infinite_statistic_is_an_ordinary_value():
    pts = np.zeros((1, 3), dtype=np.float32)
    nrm = np.float32([[0, 0, 1]])
    q = np.float32([[0, 0, 0.1], [0, 0, 3e38], [0, 0, 0.2]])  # r * r overflows fp32 for the second
    keys = tr.make_keys(np.float32([0.01, 0.02, 0.04]).view(np.uint32), [0, 0, 0])
    out, stats = rr.rtrim(np.eye(4), q, keys, pts, nrm, 1.0)
    assert stats.tolist() == [3, 3, 0x7F800000, 0x7F800000] and np.array_equal(out, keys)
    out, stats = rr.rtrim(np.eye(4), q, keys, pts, nrm, 0.5)
    assert stats[:2].tolist() == [3, 2] and out.tolist() == [keys[0], NO_KEY, keys[2]]


def test_new_entries_declared_exported_bound():
    from pointcloudprocess_amd import _lib
    src = open(os.path.join(ROOT, "include", "pcp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    bound = {name for name, _, _ in _lib.SIGNATURES}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/pcp.h"
        assert re.search(r" T %s$" % name, nm, flags=re.M), f"{name} is not exported"
        assert name in bound and getattr(lib, name).argtypes is not None


def test_argument_errors_before_any_device_call():
    """These checks read nothing through the context (pcp.h), so an opaque non-null block of memory
    stands in for one, and for the plane table; every call returns before any device call."""
    from pointcloudprocess_amd import _lib
    lib = _lib.load()
    fake_ctx = C.create_string_buffer(4096)
    ctx = C.cast(fake_ctx, C.c_void_p)
    fake_planes = C.create_string_buffer(256)
    pl = C.cast(fake_planes, C.c_void_p)
    keys, out = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(*([55] * 8))
    q = (C.c_float * 24)()
    T = (C.c_double * 16)()
    trim = (C.c_uint64 * 4)(*([77] * 4))
    nan, inf = float("nan"), float("inf")
    good = [ctx, T, q, 12, 8, keys, pl, 0.5, 1.0, 0.0, out, trim]
    bad = {"null ctx": (0, None), "null T": (1, None), "null q": (2, None), "n < 0": (4, -1), "n = 2^31": (4, 1 << 31),
           "null keys": (5, None), "null planes": (6, None), "frac < 0": (7, -0.01), "frac > 1": (7, 1.01),
           "frac NaN": (7, nan), "mult < 0": (8, -1.0), "mult inf": (8, inf), "mult NaN": (8, nan),
           "d_floor < 0": (9, -0.1), "d_floor inf": (9, inf), "d_floor NaN": (9, nan), "null out": (10, None),
           "null trim": (11, None)}
    for name, (pos, val) in bad.items():
        args = list(good)
        args[pos] = val
        assert lib.pcp_icp_trim_keys_plane(*args) == PCP_ERR_ARG, name
    assert list(trim) == [77] * 4 and list(out) == [55] * 8 and bytes(fake_ctx) == bytes(4096)
    assert lib.pcp_icp_run_plane_rtrimmed_dev(None, None, None, None, 12, 0, None, 0.5, 0.5, 1.0, 0.0, 1, None,
                                              None) == PCP_ERR_ARG
    assert lib.pcp_icp_run_plane_rtrimmed_dev(ctx, None, None, None, 12, 0, T, 0.5, 1.5, 1.0, 0.0, 1, T,
                                              trim) == PCP_ERR_ARG
    assert lib.pcp_icp_run_plane_rtrimmed_dev(ctx, None, None, None, 12, 0, T, 0.5, 0.5, 1.0, 0.0, 1, T,
                                              None) == PCP_ERR_ARG
    assert lib.pcp_get_rot_icp_plane_rtrimmed(None, None, 0, 1, None, 0, 1, T, 0.5, 0.5, 1.0, 0.0, 1, 16, 0.0, None,
                                              None) == PCP_ERR_ARG
    assert list(trim) == [77] * 4


def test_reference_tool_prints_the_table():
    pytest.importorskip("scipy")
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "rtrim_reference.py")],
                                  stderr=subprocess.STDOUT).decode()
    rows = [ln for ln in out.splitlines() if re.search(r"(every pair|point trim|residual trim)", ln)]
    assert len(rows) == 9, out
    # a row: name, six errors in mm (after iteration 1, 2, 3, 4, 6, 8), a bracket of other figures
    err = lambda ln: [float(v) for v in ln.split("(")[0].split()[-6:]]
    assert "point trim" in rows[1] and "frac 0.6 mult 1 " in rows[1]
    assert "residual trim" in rows[2] and "frac 0.5 mult 3 " in rows[2]
    point, plane = err(rows[1]), err(rows[2])
    # the figures the GPU scene test is held to: after 6 iterations, 25 % clutter, the smaller motion
    assert abs(plane[4] - rr.REF_RTRIMMED_M * 1e3) < 0.006 and abs(point[4] - rr.REF_POINT_TRIMMED_M * 1e3) < 0.006
    assert point[4] / plane[4] > 5.0
