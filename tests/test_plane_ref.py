"""The CPU oracle's planes pinned to an independent, higher-precision reference
(tests/plane_ref.py) on realistic kNN neighbourhoods, near the origin and at map-frame
coordinates, where a centring mistake would show.  GPU planes are checked against the oracle,
which restates the kernels' Jacobi and summation order; this test is what keeps that pair from
being wrong together.

Measured maxima over all cases (gates in plane_ref.py): angle 4.6e-8 rad (gate 2e-7),
curvature 1.5e-8 (1e-7), |min_value - l3| / l1 2.9e-8 (1e-7), distance 5.9e-8 relative
(2^-23); at most 0.04 % of rows at or under the gap threshold (cap 0.1 %).
"""
import numpy as np
import pytest

import oracle_ctypes as ora
import plane_ref

SHIFT = np.array([4.5e5, 5.4e6, 120.0])


@pytest.fixture(scope="module")
def scenes():
    from pointcloudprocess_amd import synth
    xyz = synth.street_scene(20_000, 31, extent=(30.0, 30.0)).double().numpy()
    return {"origin": xyz, "map": xyz + SHIFT}


def test_helper_on_known_planes():
    """The reference itself: an exactly known tilted plane at a map-frame offset."""
    rng = np.random.default_rng(5)
    n = np.array([0.48, -0.64, 0.6])           # unit, |n_y| largest -> canonical sign flips it
    u = np.cross(n, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    ab = rng.uniform(-1, 1, (50, 12, 2))
    nb = SHIFT + ab[..., :1] * u + ab[..., 1:] * v
    r = plane_ref.plane_ref(nb)
    assert plane_ref.angle(r["normal"], np.broadcast_to(n, (50, 3))).max() < 1e-8  # inputs round at 1e-9 m
    assert (r["normal"][:, 1] > 0).all()
    assert np.abs(r["l3"]).max() < 1e-15 * r["l1"].max() + 1e-16
    assert np.allclose(r["distance"], -(r["normal"].astype(np.float32).astype(np.float64) * nb.mean(1)).sum(1),
                       rtol=0, atol=1e-6)
    # angle(): resolves far below arccos' float32 floor and ignores sign
    a = np.array([[1.0, 0.0, 0.0]])
    assert abs(plane_ref.angle(a, [[-1.0, -3e-9, 0.0]])[0] - 3e-9) < 1e-15


@pytest.mark.parametrize("frame", ["origin", "map"])
@pytest.mark.parametrize("k", [5, 8, 20, 32])
def test_oracle_planes_vs_reference(scenes, frame, k):
    xyz = scenes[frame]
    idx, _ = ora.KdTree(xyz).knn(xyz, k)
    assert (idx >= 0).all()
    ref = plane_ref.plane_ref(xyz[idx])
    planes = ora.normals_knn(xyz, k)
    plane_ref.check(planes, ref, f"oracle {frame} k={k}", max_excluded=1e-3)
