"""The host Kabsch / Umeyama solve (pcp_icp_solve through ops.icp_solve) against kabsch_ref.solve on
the pairs: well-posed motions up to exactly 180 degrees, planar / collinear / three-point clouds,
the isotropic octahedron, reflections (with noise, with do_scale), scaled copies, the rank-0
collapse and the refusals (n < 3, non-finite accumulators).  No GPU needed.

Per case (kabsch_cases.check_solution): (a) dT[:3,:3] / sc is a proper rotation and sc the
reference's; (b) the cost is the reference's minimum to rounding; (c) where the minimiser is
unique, dT is the reference's within the cancellation of forming S from the accumulators,
eps * max|acc[7:16]| / (s1 + det s2).  Measured on the fixed host build over these cases:
orthonormality 8.3e-16, cost excess 4.3e-17 of the variances, (c) 26.4 units (planar at offset
(100, 200, 5); 4.1 elsewhere), scale 3.0 units; each bound is 16 times its figure
(kabsch_cases.py).
"""
import numpy as np
import pytest

import kabsch_cases as kc
import kabsch_ref as kr

CASES = kc.cases()
BAD = kc.bad_accumulators()


def _solve(q, p, do_scale):
    from pointcloudprocess_amd import ops
    return ops.icp_solve(kr.acc24(q, p), do_scale)


@pytest.mark.parametrize("name,q,p,do_scale", CASES, ids=[c[0] for c in CASES])
def test_solve_case(name, q, p, do_scale):
    rc, dT = _solve(q, p, do_scale)
    assert rc == kc.PCP_OK
    ran_c = kc.check_solution(name, q, p, do_scale, dT)
    assert ran_c == (name not in kc.NON_UNIQUE)
    if name in kc.RANK0_EXACT + kc.RANK0_NOISE:
        kc.check_rank0(name, q, p, dT)


def test_uniqueness_check_runs_on_every_other_case():
    """(c) is skipped on the named non-unique cases only, and those really are non-unique: rank
    <= 1 (s1 at the rounding level of s0, or s0 itself at the accumulators') or a reflection with
    s1 == s2."""
    names = [c[0] for c in CASES]
    assert set(kc.NON_UNIQUE) <= set(names)
    assert len(names) == len(set(names))
    for name, q, p, do_scale in CASES:
        ref = kr.solve(q, p, do_scale)
        s, det = ref["s"], ref["det"]
        noise = 64 * kc.EPS * max(s[0], np.abs(kr.acc24(q, p)[7:16]).max())
        degenerate = s[1] <= noise or (det < 0 and s[1] - s[2] <= noise)
        assert degenerate == (name in kc.NON_UNIQUE), (name, s, det)


def test_rank0_with_scale_stays_rigid():
    """The Umeyama scale of a rank-0 problem is 0, a collapse: the solve keeps scale 1."""
    for name, q, p, _ in CASES:
        if name in kc.RANK0_EXACT + kc.RANK0_NOISE:
            rc, dT = _solve(q, p, True)
            assert rc == kc.PCP_OK
            kc.check_rank0(name, q, p, dT)


@pytest.mark.parametrize("name,acc", BAD, ids=[b[0] for b in BAD])
def test_refused(name, acc):
    from pointcloudprocess_amd import ops
    for do_scale in (False, True):
        rc, _ = ops.icp_solve(acc, do_scale)
        assert rc == kc.PCP_ERR_ICP, name


def test_thin_inputs_stay_on_the_normal_path():
    """The rank-0 decision is relative to the accumulators' rounding level, so thin but
    well-defined problems still get their rotation: a millimetre-scale cloud, and a 30 m cloud at
    UTM-scale coordinates (un-centred accumulators)."""
    rng = np.random.default_rng(9)
    R = kc.rot((1, 2, 3), 0.05)
    for name, q in (("mm", rng.normal(size=(300, 3)) * 1e-3),
                    ("utm", rng.normal(size=(300, 3)) * [30.0, 30.0, 3.0] + [5.1e5, 4.2e6, 40.0])):
        p = q @ R.T + [0.3, -0.2, 0.1]
        rc, dT = _solve(q, p, False)
        assert rc == kc.PCP_OK
        ref = kr.solve(q, p)
        s = ref["s"]
        bound = kc.TOL_U * kc.EPS * np.abs(kr.acc24(q, p)[7:16]).max() / (s[1] + s[2])
        assert np.abs(dT[:3, :3] - ref["R"]).max() <= bound, name
        assert np.abs(dT[:3, :3] - R).max() <= bound + 1e-12, name
