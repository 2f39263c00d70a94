"""kabsch_ref pinned against itself: the two exact summation paths agree, the exactness bounds are
what a hand count gives, the brute-force correspondences follow the contract's order and radius
rule, the solve recovers planted motions and its cost is a minimum.  No GPU, no library."""
from fractions import Fraction

import numpy as np

import kabsch_cases as kc
import kabsch_ref as kr


def test_integer_and_fraction_paths_agree():
    rng = np.random.default_rng(1)
    for q, p in ((rng.normal(size=(300, 3)) * 50, rng.normal(size=(300, 3)) * 50 + 1e3),          # any doubles
                 (rng.integers(-2000, 2000, (300, 3)) / 32.0, rng.integers(-2000, 2000, (300, 3)) / 32.0),
                 (rng.normal(size=(40, 3)).astype(np.float32), rng.normal(size=(40, 3)).astype(np.float32))):
        d = ((q - p) ** 2).sum(1).astype(np.float32)
        a, ia = kr.exact_acc(q, p, d, method="int")
        b, ib = kr.exact_acc(q, p, d, method="fraction")
        assert np.array_equal(a, b)
        assert ia == ib


def test_exact_acc_on_a_lattice_is_the_plain_sum():
    """On a 2^-5 lattice every product and sum is a float64 value, so numpy's sums are exact too."""
    rng = np.random.default_rng(2)
    q = (rng.integers(0, 64, (500, 3)) + [32768, -16384, 8192]) / 32.0
    p = q + rng.integers(-16, 17, (500, 3)) / 32.0
    d = ((q - p) ** 2).sum(1)
    acc, info = kr.exact_acc(q, p, d)
    assert info["k"] <= 5 and info["fp32"] and info["exact64"]
    assert acc[0] == 500
    assert np.array_equal(acc[1:4], q.sum(0)) and np.array_equal(acc[4:7], p.sum(0))
    assert np.array_equal(acc[7:16], (q[:, :, None] * p[:, None, :]).sum(0).ravel())
    qq = (q[:, :, None] * q[:, None, :]).sum(0)
    assert np.array_equal(acc[16:22], [qq[0, 0], qq[0, 1], qq[0, 2], qq[1, 1], qq[1, 2], qq[2, 2]])
    assert acc[22] == d.sum()
    # 500 pairs, queries within 63 steps of each other, targets within 63 + 16 of any query
    assert info["bound"] <= 500 * 63 * 79 < 2 ** 24
    assert info["bound64"] <= 500 * (32768 + 63 + 16) ** 2 < 2 ** 53


def test_bounds_by_hand():
    q = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, 0.0]])
    p = np.array([[0.25, 0.0, 0.0], [0.5, 0.25, 1.0]])
    d = np.array([0.0625, 1.0])
    acc, info = kr.exact_acc(q, p, d)
    assert info["k"] == 2  # quarters
    # in quarters: queries span 2, a target is at most 4 from a query, d2 <= 16 quarter^2
    assert info["bound"] == 2 * max(2 * 4, 2 * 2, 16)
    assert info["bound64"] == 2 * 4 ** 2
    # an unpaired far centre widens the spans
    _, wide = kr.exact_acc(q, p, d, centres=np.array([[8.0, 0.0, 0.0]]))
    assert wide["bound"] == 2 * 32 * 32
    assert not kr.exact_acc(q + 1e-9, p, d)[1]["fp32"]
    # beyond 2^53 the sums stop being float64 values
    big = np.array([[2.0 ** 30 + 1, 1.0, 1.0]] * 3)
    assert not kr.exact_acc(big, big, np.zeros(3))[1]["exact64"]


def test_correspond_order_radius_and_non_finite():
    tgt = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [np.nan, 0, 0], [0, 1.0, 0]], np.float32)
    q = np.array([[0, 0, 0], [0, 0.75, 0], [0, 3.0, 0], [0, 2.0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    idx, d2, exact = kr.correspond(tgt, q, 1.0)
    assert exact
    # a four-way tie goes to the lowest index; a duplicate point to its first copy; d2 == r2 is
    # accepted; beyond it, and non-finite queries, are rejected; the NaN target never wins
    assert idx.tolist() == [0, 2, -1, 2, -1, -1]
    assert d2[:2].tolist() == [1.0, 0.0625] and d2[3] == 1.0
    assert np.isinf(d2[[2, 4, 5]]).all()
    assert (kr.correspond(np.zeros((0, 3), np.float32), q, 1.0)[0] == -1).all()
    # r2 is the fp32 product: 0.1f * 0.1f < 0.01 in double, and a pair at exactly that fp32 d2 is in
    r = np.float32(0.1)
    d = np.sqrt(np.float64(r * r))
    one = np.array([[0, 0, 0]], np.float32)
    qq = np.array([[d, 0, 0]], np.float32)
    got = kr.correspond(one, qq, 0.1)
    assert (got[1][0] <= r * r) == (got[0][0] == 0)


def test_correspond_matches_float64_on_a_lattice():
    rng = np.random.default_rng(3)
    tgt = (rng.integers(0, 64, (700, 3)) / 32.0 + 100.0).astype(np.float32)
    q = (rng.integers(0, 64, (300, 3)) / 32.0 + 100.0).astype(np.float32)
    idx, d2, exact = kr.correspond(tgt, q, 0.25)
    assert exact
    dd = ((q[:, None, :].astype(np.float64) - tgt[None].astype(np.float64)) ** 2).sum(2)
    j = dd.argmin(1)
    ok = dd[np.arange(300), j] <= 0.0625
    assert ok.any() and not ok.all()
    assert np.array_equal(idx, np.where(ok, j, -1))
    assert np.array_equal(d2[ok].astype(np.float64), dd[np.arange(300), j][ok])


def test_xform32_exact_on_lattice_poses():
    q = (np.random.default_rng(4).integers(0, 64, (50, 3)) / 32.0).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = kc.ROT90Z
    T[:3, 3] = [1024.0, -512.0, 256.03125]
    img, exact = kr.xform32(T, q)
    assert exact
    assert np.array_equal(img.astype(np.float64), q.astype(np.float64) @ kc.ROT90Z.T + T[:3, 3])
    T[:3, :3] = kc.rot((1, 2, 3), 0.3)  # a general rotation rounds
    assert not kr.xform32(T, q)[1]


def test_solve_recovers_planted_motion():
    rng = np.random.default_rng(5)
    q = rng.normal(size=(400, 3)) * [3.0, 2.0, 1.0] + [10.0, -4.0, 2.0]
    for ang in (0.05, 1.0, np.pi / 2, 3.0, np.pi):
        for sc in (1.0, 0.5, 2.0):
            R = kc.rot((1, 2, 3), ang)
            t = np.array([0.3, -2.0, 7.0])
            p = sc * q @ R.T + t
            ref = kr.solve(q, p, do_scale=sc != 1.0)
            assert np.abs(ref["R"] - R).max() < 1e-13 and ref["det"] == 1.0
            assert abs(ref["sc"] - sc) < 1e-13 and np.abs(ref["t"] - t).max() < 1e-12
            assert ref["cost"] < 1e-24 * ref["var_p"]
    # a mirrored copy: det = -1, and the best proper rotation leaves the mirrored axis's spread
    p = (q * [1.0, 1.0, -1.0]) @ kc.rot((1, 2, 3), 0.4).T
    ref = kr.solve(q, p)
    assert ref["det"] == -1.0 and abs(np.linalg.det(ref["R"]) - 1.0) < 1e-14
    assert ref["cost"] > 0.1 * ref["var_q"] * (1.0 / 14.0)


def test_cost_is_minimal_under_small_rotations():
    rng = np.random.default_rng(6)
    for name, q, p, do_scale in kc.cases():
        ref = kr.solve(q, p, do_scale)
        assert abs(kr.cost(q, p, ref["dT"]) - ref["cost"]) == 0.0
        for _ in range(6):
            for ang in (1e-3, 1e-6):
                dR = kc.rot(rng.normal(size=3), ang)
                T2 = ref["dT"].copy()
                T2[:3, :3] = dR @ T2[:3, :3]
                T2[:3, 3] = ref["pm"] - T2[:3, :3] @ ref["qm"]  # the best translation of that rotation
                more = kr.cost(q, p, T2) - ref["cost"]
                assert more >= -8 * kc.EPS * (ref["var_q"] + ref["var_p"]), (name, ang, more)


def test_centre_is_exact():
    x = np.array([[1e16, 1.0, 3.0], [1.0, 1.0, 3.0], [-1e16, 1.0, 3.5]])
    m, xc = kr.centre(x)
    assert m.tolist() == [float(Fraction(1, 3)), 1.0, float(Fraction(19, 6))]
    assert xc[:, 1].tolist() == [0.0, 0.0, 0.0] and xc[1, 0] == float(1 - Fraction(1, 3))
