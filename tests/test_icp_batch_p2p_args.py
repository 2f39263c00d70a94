"""CPU checks of the point-to-point batch entries (include/pcp.h, I5c) that need no device: the four
symbols are declared, exported, bound and wrapped, and every argument rule that can be reached
without a context or without a batch rejects the call with PCP_ERR_ARG (-1).  The rules that need a
live handle (null poses, keys, target, strides, sizes, the trim's scalars) are in
tests/test_gpu_icp_batch_p2p.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pcp_icp_batch_accumulate", "pcp_icp_batch_solve_dev", "pcp_icp_batch_run_dev",
         "pcp_icp_batch_run_trimmed_dev"]
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from pointcloudprocess_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_bound_and_wrapped(lib):
    from pointcloudprocess_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "pcp.h")).read()
    assert re.search(r"^#define PCP_ICP_ACC 24$", header, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (pcp_[a-z0-9_]+)$", out, flags=re.M))
    bound = {n for n, _, _ in _lib.SIGNATURES}
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in exported and n in bound and hasattr(lib, n), n
    for m in ("accumulate", "solve_dev", "run_dev", "run_trimmed_dev"):
        assert callable(getattr(ops.ICPBatch, m))


# a pointer that is never dereferenced: every call below must be rejected before it is looked at
P = C.c_void_p(64)


def _accumulate(lib, ctx=None, b=P, T=P, keys=P, tgt=P, stride=12, nt=10, acc=P):
    return lib.pcp_icp_batch_accumulate(ctx, b, T, keys, tgt, stride, nt, acc)


def _solve(lib, ctx=None, acc=P, nseg=3, do_scale=0, T=P, stats=P):
    return lib.pcp_icp_batch_solve_dev(ctx, acc, nseg, do_scale, T, stats)


def _run(lib, ctx=None, b=P, tgt=P, stride=12, nt=10, T=P, rmax=0.5, iters=2, do_scale=0, stats=P):
    return lib.pcp_icp_batch_run_dev(ctx, b, tgt, stride, nt, T, rmax, iters, do_scale, stats)


def _run_trimmed(lib, ctx=None, b=P, tgt=P, stride=12, nt=10, T=P, rmax=0.5, frac=0.5, mult=1.0, d_floor=0.0,
                 iters=2, do_scale=0, stats=P, trim=P):
    return lib.pcp_icp_batch_run_trimmed_dev(ctx, b, tgt, stride, nt, T, rmax, frac, mult, d_floor, iters, do_scale,
                                             stats, trim)


def test_null_context_rejects_every_entry(lib):
    for fn in (_accumulate, _solve, _run, _run_trimmed):
        assert fn(lib) == -1, fn.__name__
    # ... whatever else is wrong with the call, and with nothing else wrong but a null batch too
    assert _accumulate(lib, b=None) == -1 and _run(lib, b=None) == -1 and _run_trimmed(lib, b=None) == -1
    assert _accumulate(lib, T=None, keys=None, tgt=None, acc=None) == -1
    assert _accumulate(lib, stride=10) == -1 and _accumulate(lib, stride=8) == -1 and _accumulate(lib, nt=-1) == -1
    assert _accumulate(lib, stride=0, nt=0, tgt=None) == -1
    assert _solve(lib, acc=None) == -1 and _solve(lib, T=None) == -1 and _solve(lib, stats=None) == -1
    assert _solve(lib, nseg=-1) == -1 and _solve(lib, nseg=65536) == -1 and _solve(lib, nseg=0) == -1
    assert _solve(lib, do_scale=1) == -1
    for fn in (_run, _run_trimmed):
        assert fn(lib, iters=-1) == -1 and fn(lib, iters=0) == -1, fn.__name__
        assert fn(lib, rmax=-1.0) == -1 and fn(lib, rmax=NAN) == -1, fn.__name__
        assert fn(lib, T=None) == -1 and fn(lib, stats=None) == -1 and fn(lib, tgt=None) == -1, fn.__name__
        assert fn(lib, stride=14) == -1 and fn(lib, nt=-5) == -1 and fn(lib, do_scale=1) == -1, fn.__name__
    assert _run_trimmed(lib, trim=None) == -1
    for bad in (dict(frac=-0.01), dict(frac=1.5), dict(frac=NAN), dict(mult=-1.0), dict(mult=float("inf")),
                dict(mult=NAN), dict(d_floor=-0.1), dict(d_floor=float("inf")), dict(d_floor=NAN)):
        assert _run_trimmed(lib, **bad) == -1, bad
