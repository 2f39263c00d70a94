"""pcp_knn_bruteforce (C2) against inputs built to defeat its certification (MI355X).

The kernel ranks in fp32, keeps L scores per (row, target index & 15), re-ranks in fp64 and
certifies each row against an error bound; rows that do not certify are redone by an exact scan.
A wrong bound, filter, list or tile would still give plausible rows, so every case here compares
indices and d2 with np.array_equal against BOTH the exhaustive fp64 reference (tests/knn_ref.py)
and the oracle's kd-tree, on the inputs of tests/knn_cases.py: true fp64 coordinates, a cloud
kilometres from the origin, neighbours that all share one class, points fp32 cannot tell apart,
exact duplicates, every k and shape at which the code switches path, every layout, non-finite
rows and scales at which fp32 squares underflow or overflow.  A release build cannot tell which
pass answered a row, so the cases built to force the exact scan assert
pcp_knn_bruteforce_last_fallback as well; every case prints it.  tests/test_knn_ref.py holds the
CPU half: the oracle against the reference and each case's teeth.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_cases as kc
import oracle_ctypes as ora
from knn_ref import KMAX, prefix, ref_knn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _dev(ctx, a):
    return torch.from_numpy(np.array(a, order="C")).to(ctx.device)  # a copy: the cases are read-only


_trees = {}


def _oracle(name, t, q, k):
    if name not in _trees:
        _trees[name] = ora.KdTree(t)
    return _trees[name].knn(q, k)


def _bf(ctx, t_dev, q_dev, k):
    """GPU rows and the call's fallback count."""
    from pointcloudprocess_amd import ops
    gi, gd = ops.knn_bruteforce(ctx, t_dev, q_dev, k)
    fb = ops.knn_bruteforce_last_fallback(ctx)
    return gi.cpu().numpy(), gd.cpu().numpy(), fb


def _exact(gi, gd, ei, ed, label, rows=slice(None)):
    bad = (gi[rows] != ei[rows]).any(1) | (gd[rows] != ed[rows]).any(1)
    assert np.array_equal(gi[rows], ei[rows]), f"{label}: {int(bad.sum())} rows differ, first {np.flatnonzero(bad)[:5]}"
    assert np.array_equal(gd[rows], ed[rows]), f"{label}: d2 of {int(bad.sum())} rows differ"


def _run_case(ctx, name, k, t_dev=None, q_dev=None):
    """One brute-force call of a registered case at k against the reference and the oracle;
    returns the fallback count.  A non-finite query's row must be all -1 / +inf (the reference's
    row); the oracle is compared on the finite queries."""
    t, q, _, ref = kc.case(name)
    gi, gd, fb = _bf(ctx, _dev(ctx, t) if t_dev is None else t_dev, _dev(ctx, q) if q_dev is None else q_dev, k)
    print(f"{name} k={k}: fallback queries {fb} of {len(q)}")
    ri, rd = prefix(ref, k)
    _exact(gi, gd, ri, rd, f"{name} k={k} vs reference")
    if len(t):
        ei, ed = _oracle(name, t, q, k)
        _exact(gi, gd, ei, ed, f"{name} k={k} vs oracle", rows=np.isfinite(q).all(1))
    return fb


# ---------------------------------------------------------------- a. off-origin, true fp64
@pytest.mark.parametrize("k", kc.K_SWEEP)
@pytest.mark.parametrize("name", ["off_origin", "centred"])
def test_true_fp64_cloud(ctx, name, k):
    """Exactness only: by E = 40 2^-24 (pmax + |q|)^2 every off-origin row is expected to fall
    back today; a build that centres the coordinates may bring that to 0."""
    _run_case(ctx, name, k)


# ---------------------------------------------------------------- b. class collision
@pytest.mark.parametrize("k", kc.K_SWEEP)
@pytest.mark.parametrize("cls", [3, 0, 15])  # 0 and 15: first and last lane of the group shuffle
def test_class_collision(ctx, cls, k):
    fb = _run_case(ctx, f"collision_{cls}", k)
    if k > kc.LIST_LEN[k]:  # the class's list cannot hold the k neighbours: certification must refuse
        assert fb >= kc.COLLISION_NQ


# ---------------------------------------------------------------- c. fp32-identical clusters
@pytest.mark.parametrize("k", [8, 16, 32])
def test_micro_clusters(ctx, k):
    _run_case(ctx, "micro_clusters", k)


# ---------------------------------------------------------------- d. exact duplicates
@pytest.mark.parametrize("k", [8, 32])
def test_duplicates(ctx, k):
    _run_case(ctx, "duplicates", k)  # the reference rows are the lowest indices, ascending, d2 = 0


@pytest.mark.parametrize("k", [8, 9, 16])
def test_tie_lattice(ctx, k):
    """Exact ties among the k nearest in rows that certify: the order comes from the fp64
    re-rank's (d2, index) sort, not from the exact scan (which answers every duplicate row)."""
    fb = _run_case(ctx, "tie_lattice", k)
    if k == 8:
        t, q, _, ref = kc.case("tie_lattice")
        assert fb <= len(q) - int(kc.tie_lattice_must_certify(t, q, ref).sum())


# ---------------------------------------------------------------- e. k boundaries and errors
def test_few_finite_targets(ctx):
    _run_case(ctx, "few_finite", 8)


@pytest.mark.parametrize("k,code", [(33, -5), (0, -1)])  # PCP_ERR_UNSUPPORTED, PCP_ERR_ARG
def test_rejected_k(ctx, k, code):
    from pointcloudprocess_amd import _lib, ops
    t, q, _, _ = kc.case("collision_3")
    td, qd = _dev(ctx, t), _dev(ctx, q)
    assert _run_case(ctx, "collision_3", 8, td, qd) >= kc.COLLISION_NQ  # leaves a non-zero count behind
    with pytest.raises(_lib.PcpError) as err:
        ops.knn_bruteforce(ctx, td, qd, k)
    assert err.value.code == code
    assert ops.knn_bruteforce_last_fallback(ctx) == 0  # nothing was searched
    _run_case(ctx, "collision_3", 8, td, qd)  # the context still answers exactly


# ---------------------------------------------------------------- f. shape sweep
IDX_SENTINEL, D2_SENTINEL = -77, -1234.5


def test_shape_sweep(ctx):
    """Every nt around the tile (1024) and sub-tile (16) sizes times every nq around the block
    (64) and MFMA row (16) sizes, k = 8 and 32 (k > nt occurs).  The outputs are 64 rows longer
    than nq and pre-filled: a partial wave writing past the end would show."""
    t, q = kc.shape_cloud()
    td, qd = _dev(ctx, t), _dev(ctx, q)
    for nt in kc.SHAPE_NT:
        ref = ref_knn(t[:nt], q, KMAX)
        tree = ora.KdTree(t[:nt])
        counts = []
        for k in (8, 32):
            ei, ed = tree.knn(q, k)
            ri, rd = prefix(ref, k)
            for nq in kc.SHAPE_NQ:
                oi = torch.full((nq + 64, k), IDX_SENTINEL, dtype=torch.int32, device=ctx.device)
                od = torch.full((nq + 64, k), D2_SENTINEL, dtype=torch.float64, device=ctx.device)
                ctx.check(ctx.lib.pcp_knn_bruteforce(ctx.h, C.c_void_p(td.data_ptr()), 24, nt, C.c_void_p(qd.data_ptr()),
                                                     24, nq, k, C.c_void_p(oi.data_ptr()), C.c_void_p(od.data_ptr())))
                gi, gd = oi.cpu().numpy(), od.cpu().numpy()
                label = f"nt={nt} nq={nq} k={k}"
                assert (gi[nq:] == IDX_SENTINEL).all() and (gd[nq:] == D2_SENTINEL).all(), f"{label}: wrote past nq"
                _exact(gi[:nq], gd[:nq], ri[:nq], rd[:nq], f"{label} vs reference")
                _exact(gi[:nq], gd[:nq], ei[:nq], ed[:nq], f"{label} vs oracle")
                n = C.c_int64()
                ctx.check(ctx.lib.pcp_knn_bruteforce_last_fallback(ctx.h, C.byref(n)))
                counts.append(n.value)
        print(f"nt={nt}: fallback queries per (k, nq) {counts}")


# ---------------------------------------------------------------- g. layouts, non-finite rows
def _strided4(ctx, a):
    """(n, 4) float64 with NaN in the 4th column, viewed as [:, :3]: 32-byte stride."""
    w = np.full((len(a), 4), np.nan)
    w[:, :3] = a
    v = _dev(ctx, w)[:, :3]
    assert v.stride(0) == 4 and not v.is_contiguous()
    return v


@pytest.mark.parametrize("layout", ["packed", "aos48", "strided32"])
@pytest.mark.parametrize("k", [8, 32])
def test_layouts_and_nonfinite(ctx, layout, k):
    from pointcloudprocess_amd import ops
    t, q, _, _ = kc.case("nonfinite_mix")
    if layout == "aos48":
        td, qd = (ops.cloud_to_device(ora.make_cloud(a), ctx.device) for a in (t, q))
    elif layout == "strided32":
        td, qd = _strided4(ctx, t), _strided4(ctx, q)
    else:
        td, qd = _dev(ctx, t), _dev(ctx, q)
    fb = _run_case(ctx, "nonfinite_mix", k, td, qd)
    assert fb <= int(np.isfinite(q).all(1).sum())  # a non-finite query is answered, not redone


def test_nonfinite_queries_not_counted(ctx):
    """Off-origin every finite row falls back; with NaN rows mixed in the count must be exactly
    the finite rows -- whatever share falls back, it is the same with and without the NaN rows."""
    t, q, _, ref = kc.case("off_origin")
    q = q[:300].copy()
    td = _dev(ctx, t)
    _, _, fb_all = _bf(ctx, td, _dev(ctx, q), 8)
    q[::7] = np.nan
    gi, gd, fb = _bf(ctx, td, _dev(ctx, q), 8)
    bad = ~np.isfinite(q).all(1)
    ri, rd = (a[:300].copy() for a in prefix(ref, 8))
    ri[bad], rd[bad] = -1, np.inf
    _exact(gi, gd, ri, rd, "off-origin with NaN queries")
    _, _, fb_fin = _bf(ctx, td, _dev(ctx, q[~bad]), 8)
    print(f"fallback queries: all rows {fb_all}, with NaN rows {fb}, finite rows alone {fb_fin}")
    assert fb == fb_fin <= int((~bad).sum())


# ---------------------------------------------------------------- h. scale
@pytest.mark.parametrize("e", kc.SCALE_EXP)
def test_scale(ctx, e):
    """Metamorphic: scaling by 2^e is exact in fp64, so the indices are the base run's and the
    d2 its d2 * 2^(2e).  2^60: fp32 squares overflow, every row must take the exact scan.
    2^-100: fp32 squares underflow, every score is 0 and a purely relative bound would certify
    whatever the lists happen to hold."""
    t, q, _, _ = kc.case("scale_base")
    bi, bd, _ = _bf(ctx, _dev(ctx, t), _dev(ctx, q), 8)
    _run_case(ctx, "scale_base", 8)
    ts, qs, _, _ = kc.case(f"scale_2^{e}")
    gi, gd, fb = _bf(ctx, _dev(ctx, ts), _dev(ctx, qs), 8)
    print(f"2^{e}: fallback queries {fb} of {len(q)}")
    _exact(gi, gd, bi, np.ldexp(bd, 2 * e), f"2^{e} vs the base run")
    _run_case(ctx, f"scale_2^{e}", 8)
    if e == 60:
        assert fb == len(q)


def test_scale_mixed(ctx):
    _run_case(ctx, "scale_mixed", 8)


# ---------------------------------------------------------------- i. no targets
@pytest.mark.parametrize("name", ["no_targets", "no_finite_targets"])
def test_no_targets(ctx, name):
    """Nothing to rank: every row is -1 / +inf and nothing is redone."""
    assert _run_case(ctx, name, 8) == 0


# ---------------------------------------------------------------- the same inputs through pcp_knn
@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("name", ["off_origin", "duplicates"])
def test_grid_knn_same_inputs(ctx, name, k):
    """The fp64 grid search on true-fp64, off-origin and duplicated targets."""
    from pointcloudprocess_amd import ops
    t, q, _, ref = kc.case(name)
    ix = ops.GridIndex(ctx, _dev(ctx, t))
    gi, gd = ops.knn(ix, _dev(ctx, q), k)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    ix.close()
    _exact(gi, gd, *prefix(ref, k), f"pcp_knn {name} k={k} vs reference")
    _exact(gi, gd, *_oracle(name, t, q, k), f"pcp_knn {name} k={k} vs oracle")
