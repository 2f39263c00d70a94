"""The kNN certification inputs (tests/knn_cases.py) on the CPU: the oracle's kd-tree search
against the exhaustive reference (tests/knn_ref.py), bit for bit, and each case's teeth -- the
property of the input that makes it reach the path it was built for.

The exhaustive reference has no tree, so this also pins the oracle's pruning rule
(bound <= kth) at ties, duplicates and off-origin coordinates.
"""
import numpy as np
import pytest

import knn_cases as kc
import oracle_ctypes as ora
from knn_ref import KMAX, prefix, ref_knn


def _oracle_equals_ref(t, q, ref, ks, label):
    tree = ora.KdTree(t)
    rows = np.isfinite(q).all(1)
    for k in ks:
        ri, rd = prefix(ref, k)
        ei, ed = tree.knn(q, k)
        assert np.array_equal(ei[rows], ri[rows]), f"{label} k={k}: {(ei[rows] != ri[rows]).any(1).sum()} rows differ"
        assert np.array_equal(ed[rows], rd[rows]), f"{label} k={k}: d2 differs"
        # a non-finite query's reference row is all padding
        assert (ri[~rows] == -1).all() and np.isinf(rd[~rows]).all()


@pytest.mark.parametrize("name", list(kc.CASES))
def test_oracle_equals_exhaustive(name):
    t, q, _, ref = kc.case(name)
    _oracle_equals_ref(t, q, ref, kc.CASES[name][1], name)


def test_shape_sweep_oracle_equals_exhaustive():
    t, q = kc.shape_cloud()
    for nt in kc.SHAPE_NT:
        ref = ref_knn(t[:nt], q, KMAX)
        _oracle_equals_ref(t[:nt], q, ref, (8, 32), f"nt={nt}")
        kk = min(nt, KMAX)
        assert (ref[0][:, :kk] >= 0).all() and (ref[0][:, kk:] == -1).all() and np.isinf(ref[1][:, kk:]).all()


def test_ref_prefix_is_topk():
    """The slicing the other tests rely on: ref_knn(k) is the first k columns of ref_knn(32)."""
    t, q, _, ref = kc.case("duplicates")
    for k in (1, 8, 17):
        i, d = ref_knn(t, q, k)
        assert np.array_equal(i, ref[0][:, :k]) and np.array_equal(d, ref[1][:, :k])


def test_ref_padding_and_nonfinite():
    t, q, _, ref = kc.case("few_finite")
    idx, d2 = prefix(ref, 8)
    fin = np.flatnonzero(np.isfinite(t).all(1))
    assert np.array_equal(np.sort(idx[:, :6], 1), np.broadcast_to(fin, (len(q), 6)))  # original indices
    assert (idx[:, 6:] == -1).all() and np.isinf(d2[:, 6:]).all()
    assert (np.diff(d2[:, :6], axis=1) >= 0).all()
    t, q, _, ref = kc.case("nonfinite_mix")
    bad = ~np.isfinite(q).all(1)
    assert bad.sum() > 70 and bad[3] and (ref[0][bad] == -1).all() and np.isinf(ref[1][bad]).all()
    assert (ref[0][~bad] >= 0).all() and np.isfinite(t[ref[0][~bad]]).all()
    for name, nq in (("no_targets", 5), ("no_finite_targets", 70)):
        t, q, _, ref = kc.case(name)
        assert ref[0].shape == (nq, KMAX) and (ref[0] == -1).all() and np.isinf(ref[1]).all()


# ---------------------------------------------------------------- teeth
def test_teeth_true_f64():
    """Every case's coordinates change under an fp32 round trip (the builders assert > 90 %),
    and the off-origin cloud is where the certification bound E = 40 2^-24 (pmax + |q|)^2
    exceeds the squared distance to the 8th neighbour, while at the origin it is a small
    fraction of it."""
    for name in kc.CASES:
        t, q, _, _ = kc.case(name)
        if np.isfinite(t).any() and name != "tie_lattice":  # integers by design, see its docstring
            assert kc.true_f64_share(t) > 0.9, name
    share = {}
    for name in ("off_origin", "centred"):
        t, q, _, ref = kc.case(name)
        pmax = np.sqrt((t * t).sum(1).max())
        e = 40.0 * 2.0 ** -24 * (pmax + np.sqrt((q * q).sum(1))) ** 2
        share[name] = float((e > ref[1][:, 7]).mean())
    print(f"rows with E above the 8th neighbour's d2: {share}")
    assert share["off_origin"] > 0.99 and share["centred"] < 0.01


@pytest.mark.parametrize("cls", [3, 0, 15])
def test_teeth_class_collision(cls):
    t, q, _, ref = kc.case(f"collision_{cls}")
    assert len(t) == 19_200 and len(q) == kc.COLLISION_NQ
    for k in kc.K_SWEEP:
        idx, _ = prefix(ref, k)
        assert (idx % 16 == cls).all(), (k, int((idx % 16 != cls).any(1).sum()))


def test_teeth_micro_clusters():
    """Most clusters collapse to one fp32 point of more than 16 L = 160 copies (L = 10), and
    every collapsed cluster's copies outnumber the L = 5 and L = 10 lists of some class."""
    t, q, (member,), ref = kc.case("micro_clusters")
    t32 = t.astype(np.float32)
    distinct = len(np.unique(t32, axis=0))
    collapsed = 0
    for c in range(kc.CLUSTERS):
        pts = t32[member == c]
        assert len(pts) == kc.CLUSTER_SIZE
        _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
        big = int(cnt.argmax())
        if cnt[big] > 160:
            collapsed += 1
            per_class = np.bincount(np.flatnonzero(member == c)[inv.ravel() == big] % 16, minlength=16)
            assert per_class.max() > 10
    print(f"distinct fp32 points {distinct} of {len(t)}, clusters with > 160 identical casts {collapsed}")
    assert collapsed >= 20
    assert distinct <= 8000 + kc.CLUSTERS * kc.CLUSTER_SIZE // 4
    # fp64 tells the copies apart: the centre rows' 32 neighbours are 32 distinct distances
    d2 = ref[1][:kc.CLUSTERS]
    assert (np.diff(d2, axis=1) > 0).mean() > 0.99 and (d2 < 1e-12).all()


def test_teeth_duplicates():
    t, q, _, ref = kc.case("duplicates")
    for k in (8, 32):
        idx, d2 = prefix(ref, k)
        for r in range(kc.DUP_POINTS):
            same = np.flatnonzero((t == q[r]).all(1))
            assert len(same) == kc.DUP_COPIES
            assert np.array_equal(idx[r], same[:k]) and (d2[r] == 0).all()  # lowest indices, ascending


def test_teeth_tie_lattice():
    """Most rows have 8 exactly tied neighbours with two or more in one class of the kernel, in
    rows that a correct bound must certify: the fp64 re-rank's index tie-break decides them."""
    t, q, _, ref = kc.case("tie_lattice")
    idx, d2 = ref
    must = kc.tie_lattice_must_certify(t, q, ref)
    shared = np.array([len(set(r % 16)) < 8 for r in idx[:, :8]])
    t32 = t.astype(np.float32)
    p2 = (t32 * t32).sum(1, dtype=np.float32).astype(np.float64)
    inexact = float((p2 != (t * t).sum(1)).mean())
    print(f"rows that must certify {int(must.sum())}, of them with a shared class {int((must & shared).sum())}, "
          f"targets whose fp32 |p|^2 is rounded {inexact:.3f}")
    assert must.sum() >= 400 and (must & shared).sum() >= 300 and inexact > 0.5


def test_teeth_scale():
    t, q, _, base = kc.case("scale_base")
    for e in kc.SCALE_EXP:
        ts, qs, _, ref = kc.case(f"scale_2^{e}")
        assert np.array_equal(ref[0], base[0])
        assert np.array_equal(ref[1], np.ldexp(base[1], 2 * e))  # exact in fp64
    with np.errstate(over="ignore", under="ignore"):
        lo = kc.case("scale_2^-100")[0].astype(np.float32)
        hi = kc.case("scale_2^60")[0].astype(np.float32)
        assert ((lo * lo).sum(1) == 0).all()      # fp32 squares underflow: every score is 0
        over = np.isinf((hi * hi).sum(1))         # fp32 squares overflow: never ranked, yet finite
        assert 0.9 < over.mean() < 1.0            # all but the targets within 16 m of the origin
    t, q, (far,), ref = kc.case("scale_mixed")
    assert np.array_equal(ref[0][-30:, 0], far)   # the nearest target is a never-ranked one
