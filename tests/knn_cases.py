"""Input builders of the kNN certification tests, shared by tests/test_knn_ref.py (CPU) and
tests/test_gpu_bruteforce_adversarial.py (GPU) so that both see identical arrays.

TEST INFRASTRUCTURE ONLY.  Fixed seeds.  Every builder returns true float64 arrays: most of
their coordinates are NOT representable in fp32 (asserted), so the brute-force kernel's casts
to fp32 lose bits and only its fp64 re-rank can give the exact row.  A builder whose docstring
says otherwise is the exception.
"""
import numpy as np

K_SWEEP = (1, 5, 6, 8, 9, 10, 11, 16, 17, 32)  # both sides of every template / list-length switch
# per-(row, class) list length of k_bf_mfma for a given k
LIST_LEN = {k: (5 if k <= 8 else 10 if k <= 16 else 16) for k in range(1, 33)}


def true_f64_share(a):
    """Share of the finite coordinates that an fp32 round trip changes."""
    a = np.asarray(a, dtype=np.float64)
    fin = np.isfinite(a)
    with np.errstate(over="ignore"):
        back = a.astype(np.float32).astype(np.float64)
    return float((back[fin] != a[fin]).mean()) if fin.any() else 0.0


def _true_f64(*arrays):
    for a in arrays:
        assert a.dtype == np.float64
        assert true_f64_share(a) > 0.9, true_f64_share(a)


def _cube(rng, n, half):
    return rng.uniform(-half, half, (n, 3))


# ---------------------------------------------------------------- a. off-origin
OFFSET = np.array([5000.0, -3000.0, 40.0])


def off_origin(centred=False):
    """20,000 targets in a +-50 m cube, 1,500 queries in +-55 m plus 500 of the targets, all
    translated by OFFSET (a cloud a few km from the origin); centred=True: the same draws
    without the translation."""
    rng = np.random.default_rng(3101)
    t = _cube(rng, 20_000, 50.0)
    q = np.concatenate([_cube(rng, 1500, 55.0), t[rng.choice(len(t), 500, replace=False)]])
    if not centred:
        t, q = t + OFFSET, q + OFFSET
    _true_f64(t, q)
    return t, q


# ---------------------------------------------------------------- b. class collision
COLLISION_C = np.array([10.0, -7.0, 3.0])
COLLISION_NQ = 600


def class_collision(cls):
    """19,200 targets in +-50 m; every target with index % 16 == cls lies in a +-1 m box around
    COLLISION_C and every other target within 6 m (Chebyshev) of it is pushed away by +20 m on
    each axis; 600 queries at COLLISION_C +- 0.5 m.  All k neighbours of every query share one
    class of the kernel's 16, so its per-class lists cannot hold them when k > L."""
    rng = np.random.default_rng(3200 + cls)
    nt = 19_200
    t = _cube(rng, nt, 50.0)
    near = np.arange(nt) % 16 == cls
    t[near] = COLLISION_C + _cube(rng, int(near.sum()), 1.0)
    close = ~near & (np.abs(t - COLLISION_C).max(1) <= 6.0)
    t[close] += 20.0
    q = COLLISION_C + _cube(rng, COLLISION_NQ, 0.5)
    _true_f64(t, q)
    return t, q


# ---------------------------------------------------------------- c. fp32-identical clusters
CLUSTERS, CLUSTER_SIZE = 40, 200


def micro_clusters():
    """8,000 uniform targets plus 40 clusters of 200 points, each an fp32-representable centre
    plus +-1e-7 noise that fp32 mostly cannot see, shuffled.  Queries: the centres (these 40
    rows ARE fp32-representable), the centres +- 1e-3 and 300 uniform points.
    Returns (t, q, member) with member[i] = cluster of target i or -1."""
    rng = np.random.default_rng(3301)
    centres = _cube(rng, CLUSTERS, 50.0).astype(np.float32).astype(np.float64)
    noise = rng.uniform(-1e-7, 1e-7, (CLUSTERS, CLUSTER_SIZE, 3))
    t = np.concatenate([_cube(rng, 8000, 50.0), (centres[:, None, :] + noise).reshape(-1, 3)])
    member = np.concatenate([np.full(8000, -1), np.repeat(np.arange(CLUSTERS), CLUSTER_SIZE)])
    perm = rng.permutation(len(t))
    t, member = t[perm], member[perm]
    q = np.concatenate([centres, centres + 1e-3, centres - 1e-3, _cube(rng, 300, 50.0)])
    _true_f64(t, q[CLUSTERS:])
    return t, q, member


# ---------------------------------------------------------------- d. exact duplicates
DUP_POINTS, DUP_COPIES = 10, 300


def duplicates():
    """3,000 uniform targets plus 10 points repeated 300 times each, shuffled.  Queries: the 10
    duplicated points, then 300 uniform points."""
    rng = np.random.default_rng(3401)
    pts = _cube(rng, DUP_POINTS, 50.0)
    t = np.concatenate([_cube(rng, 3000, 50.0), np.repeat(pts, DUP_COPIES, 0)])
    t = t[rng.permutation(len(t))]
    q = np.concatenate([pts, _cube(rng, 300, 50.0)])
    _true_f64(t, q)
    return t, q


def tie_lattice():
    """A 16^3 lattice of odd integers, pitch 64 m, 4 km from the origin, shuffled; 600 queries at
    cell centres, so the 8 nearest targets are exactly tied in fp64 (inner rows).  NOT true
    fp64: every coordinate is an integer fp32 holds -- but |p|^2 and q.p exceed 2^24, so the
    fp32 scores of tied targets round apart and a class list's score order need not be its
    index order.  The duplicates above cannot test the index tie-break of the fp64 re-rank:
    300 copies never certify.  Here the tied 8 sit well inside the lists and the row does."""
    rng = np.random.default_rng(3451)
    i, j, l = (a.ravel() for a in np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"))
    t = np.stack([4001.0 + 64 * i, 64.0 * j - 511, 64.0 * l - 513], 1)
    t = t[rng.permutation(len(t))]
    q = t[:600] + 32.0
    return t, q


def tie_lattice_must_certify(t, q, ref):
    """Rows of tie_lattice that a correct k = 8 certification cannot refuse: 8 tied neighbours,
    no class (index & 15) holding 5 = L of them -- so every class's L-th best score belongs to the
    9th neighbour or beyond and tau >= d2[8] - |q|^2 - E -- and d2[8] - d2[7] > 2 E, which puts
    the bound |q|^2 + tau - E above the k-th distance."""
    idx, d2 = ref
    pmax = np.sqrt((t * t).sum(1).max())
    e = 40.0 * 2.0 ** -24 * (pmax + np.sqrt((q * q).sum(1))) ** 2
    per_class = np.stack([(idx[:, :8] % 16 == c).sum(1) for c in range(16)], 1)
    return (d2[:, 0] == d2[:, 7]) & (per_class.max(1) < 5) & (d2[:, 8] - d2[:, 7] > 2 * e)


# ---------------------------------------------------------------- e. few finite targets
def few_finite():
    """20 targets of which 14 are NaN rows (6 finite: kk = 6 < k = 8), 100 queries."""
    rng = np.random.default_rng(3501)
    t = _cube(rng, 20, 50.0)
    t[rng.choice(20, 14, replace=False)] = np.nan
    q = _cube(rng, 100, 50.0)
    assert int(np.isfinite(t).all(1).sum()) == 6
    _true_f64(t, q)
    return t, q


# ---------------------------------------------------------------- f. shape sweep
SHAPE_NT = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
SHAPE_NQ = (1, 15, 16, 17, 63, 64, 65, 257)


def shape_cloud():
    """One +-50 m cloud; the sweep takes t[:nt] and q[:nq]."""
    rng = np.random.default_rng(3601)
    t, q = _cube(rng, max(SHAPE_NT), 50.0), _cube(rng, max(SHAPE_NQ), 50.0)
    _true_f64(t, q)
    return t, q


# ---------------------------------------------------------------- g. layouts, non-finite
def nonfinite_mix():
    """3,000 targets with every 13th a NaN row and one -inf component; 500 queries with every
    7th a NaN row and one +inf component."""
    rng = np.random.default_rng(3701)
    t, q = _cube(rng, 3000, 50.0), _cube(rng, 500, 50.0)
    t[::13] = np.nan
    t[5, 2] = -np.inf
    q[::7] = np.nan
    q[3, 1] = np.inf
    _true_f64(t, q)
    return t, q


# ---------------------------------------------------------------- h. scale
SCALE_EXP = (-100, -10, 10, 60)


def scale_base():
    """+-50 m, 5,000 targets, 400 queries; the scale tests multiply both by 2**e (exact)."""
    rng = np.random.default_rng(3801)
    t, q = _cube(rng, 5000, 50.0), _cube(rng, 400, 50.0)
    _true_f64(t, q)
    return t, q


def scale_mixed():
    """scale_base with every 50th target replaced by a uniform +-3e19 point, and 30 more queries
    placed 1.0 from such points whose fp32 |p|^2 overflows: their nearest target is one the
    kernel never ranks.  Returns (t, q, far) with far = those 30 targets' indices."""
    rng = np.random.default_rng(3802)
    t, q = scale_base()
    t = t.copy()
    t[::50] = _cube(rng, len(t[::50]), 3e19)
    with np.errstate(over="ignore"):
        p2 = (t.astype(np.float32) ** 2).sum(1, dtype=np.float32)
    far = np.flatnonzero(np.isinf(p2))[:30]
    assert len(far) == 30 and (far % 50 == 0).all()
    q = np.concatenate([q, t[far] + np.array([1.0, 0.0, 0.0])])
    _true_f64(t, q)
    return t, q, far


# ---------------------------------------------------------------- registry
def _scaled(e):
    t, q = scale_base()
    return np.ldexp(t, e), np.ldexp(q, e)


# name -> (builder of (t, q, ...), the k values the case is run at)
CASES = {
    "off_origin": (off_origin, K_SWEEP),
    "centred": (lambda: off_origin(centred=True), K_SWEEP),
    "collision_3": (lambda: class_collision(3), K_SWEEP),
    "collision_0": (lambda: class_collision(0), K_SWEEP),
    "collision_15": (lambda: class_collision(15), K_SWEEP),
    "micro_clusters": (micro_clusters, (8, 16, 32)),
    "duplicates": (duplicates, (8, 32)),
    "tie_lattice": (tie_lattice, (8, 9, 16)),
    "few_finite": (few_finite, (8,)),
    "nonfinite_mix": (nonfinite_mix, (8, 32)),
    "scale_base": (scale_base, (8,)),
    **{f"scale_2^{e}": ((lambda e=e: _scaled(e)), (8,)) for e in SCALE_EXP},
    "scale_mixed": (scale_mixed, (8,)),
    "no_targets": (lambda: (np.empty((0, 3)), scale_base()[1][:5]), (8,)),
    "no_finite_targets": (lambda: (np.full((40, 3), np.nan), scale_base()[1][:70]), (8,)),
}

_cache = {}


def case(name):
    """(t, q, extras, top-32 exhaustive reference) of a case: built once per process, read-only."""
    if name not in _cache:
        from knn_ref import KMAX, ref_knn
        t, q, *extra = CASES[name][0]()
        ref = ref_knn(t, q, KMAX)
        for a in (t, q, *ref):
            a.setflags(write=False)
        _cache[name] = (t, q, tuple(extra), ref)
    return _cache[name]
