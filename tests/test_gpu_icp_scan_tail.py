"""The tail of the ICP octant scan (Top3P::scan4, DESIGN.md §5.1 "Round 7", MI355X).

The packed-key scan loads its candidates in batches of 4 per lane over a wave-uniform trip count
Lg = ceil(Lw / G) (Lw the longest list of the chunk, G lanes per query), two batches in flight, and
issues no batch at or past Lg.  What can go wrong sits at the batch edges and at the ends of the
lanes' lists, so the scene fixes the length of every query's list:

* cell 0.125 m, target origin (0, 0, 0); site k is the grid vertex ((4k + 2) h, 2h, 2h), with L_k
  targets in the 8 cells around it and one query next to it, whose octant block is those 8 cells.
  The queries sort by the x cell of their block, so query k is the k-th of the first launch and
  64 / G consecutive sites make a chunk;
* sites come in runs of 64: special runs (one 40- or 255-candidate list at the first lane, the last
  lane or in a middle group with every other list empty; a run of empty lists, Lw = 0), then one
  run per length L in 0-9, 11-13, 15-17, 31-33, 63-65, 255 (and 24, 28, 48, 56) whose longest list
  is L.  For G = 1, 2, 4, 8 these give Lg = 0, 1, 4, 5, 8, 9 and every residue of ceil(L / G)
  modulo 4 and 8, and lists shorter than G (lanes with no entry at all);
* 9 launches along x: shrinking steps (the look-ahead engages from the third launch), a jump of one
  site spacing (every query is searched again, now with the lists of the next site, by the
  look-ahead form of the scan), shrinking steps again.  Half of the queries sit 0.05 cell from a
  face of their block: their certificate fails at every launch, so their lists, short ones too, are
  scanned at every launch, and the fallback pass consumes what the scan recorded; the verify pass
  consumes the records of the others.

Every launch must equal the oracle: index and d2 bit for bit, accumulators within the tolerance of
test_gpu_icp_lookahead.py.
"""
import numpy as np
import pytest
import torch

import oracle_ctypes as ora

pytestmark = pytest.mark.gpu

H, RMAX, SPACING = 0.125, 0.09, 4
REQUIRED = list(range(0, 10)) + [11, 12, 13, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255]
# ceil(L / G) = 6 and 7 modulo 8 for G = 4 and G = 8, which the lengths above do not give
EXTRA = [24, 28, 48, 56]
# (site of the run, its list length): every other list of the run is empty
SPECIAL = [(0, 40), (63, 40), (29, 40), (None, 0), (37, 255)]
SHIFT_MM = [0.0, 6.0, 10.0, 12.5, 14.0, 514.0, 517.0, 519.0, 520.0]  # launch 5: + one site spacing
JUMP = 5


@pytest.fixture(scope="module")
def ctx():
    from pointcloudprocess_amd import ops
    return ops.Context(0)


def _pose(x_mm):
    T = np.eye(4)
    T[0, 3] = float(np.float32(x_mm * 1e-3))
    return T


class Scene:
    """Targets, queries, the host's count of every query's block at every pose, and the oracle's
    correspondences and accumulators at every pose (computed once, shared, never changed)."""

    def __init__(self):
        rng = np.random.default_rng(7001)
        lens = []
        for pos, L in SPECIAL:
            run = np.zeros(64, np.int64)
            if pos is not None:
                run[pos] = L
            lens.append(run)
        for L in REQUIRED + EXTRA:
            run = rng.integers(0, min(L, 40) + 1, 64)
            run[(7 * L) % 64] = L
            lens.append(run)
        self.lens = np.concatenate(lens)
        n = len(self.lens)
        vx = (SPACING * np.arange(n) + 2) * H  # the sites' vertices ((4k + 2) h, 2h, 2h)
        # targets: 0.05 to 0.3 cell from the vertex on every axis (no point near a cell boundary)
        site = np.repeat(np.arange(n), self.lens)
        off = rng.uniform(0.05, 0.3, (len(site), 3)) * rng.choice([-1.0, 1.0], (len(site), 3))
        tgt = np.stack([vx[site], np.full(len(site), 2 * H), np.full(len(site), 2 * H)], 1) + off * H
        anchors = np.array([[0.0, 0.0, 0.0], [0.0, 3.5 * H, 3.5 * H]])  # origin and y / z extent
        self.tgt = np.ascontiguousarray(np.concatenate([anchors, tgt]).astype(np.float32))
        # queries: one per site; x within 0.05 cell of the vertex (the path and the look-ahead
        # offset stay inside the half cell that keeps the block), half of them 0.45 cell off in y
        qo = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n)], 1)
        edge = rng.random(n) < 0.5
        edge[:64 * len(SPECIAL)] = False
        qo[edge, 1] = 0.45
        self.q = np.ascontiguousarray((np.stack([vx, np.full(n, 2 * H), np.full(n, 2 * H)], 1) + qo * H)
                                      .astype(np.float32))
        self.poses = [_pose(x) for x in SHIFT_MM]
        self.blocks = [self.block_counts(T) for T in self.poses]
        oi = ora.F32Index(self.tgt)
        self.corr, self.acc = [], []
        for T in self.poses:
            R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
            ei, ed = oi.correspond(self.q, R, t, RMAX)
            self.corr.append((ei, ed))
            self.acc.append(ora.icp_accumulate(self.tgt, self.q, R, t, ei, ed))

    def block_counts(self, T):
        """Targets in each query's octant block, the cells [b, b + 1]^3 with b = floor(f - 1/2) of
        its cell coordinate f at pose T.  Also checks that no query is near a plane where b flips
        (0.03 cell in y and z; 0.17 cell in x, where the look-ahead centre may lie 20 mm ahead)."""
        o = self.tgt.min(0).astype(np.float64)
        assert (o == 0.0).all()
        f = (self.q.astype(np.float64) + T[:3, 3]) / H
        frac = np.abs(f - 0.5 - np.round(f - 0.5))  # distance to the nearest flip plane, cells
        assert (frac[:, 0] > 0.17).all() and (frac[:, 1:] > 0.03).all()
        b = np.floor(f - 0.5).astype(np.int64)
        tc = np.floor(self.tgt.astype(np.float64) / H).astype(np.int64)
        shape = tc.max(0) + 3
        cnt = np.zeros(shape, np.int64)
        np.add.at(cnt, tuple(tc.T), 1)
        out = np.zeros(len(f), np.int64)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    c = b + (dx, dy, dz)
                    ok = ((c >= 0) & (c < shape)).all(1)
                    out[ok] += cnt[tuple(c[ok].T)]
        return out


@pytest.fixture(scope="module")
def scene():
    return Scene()


def test_scene_has_every_list_length(scene):
    """The precondition: the block contents counted on the host hold every listed length, at the
    first launch and at the jump (when every list is scanned again), and the special chunks are
    what they are meant to be."""
    assert len(scene.tgt) <= 20_000 and len(scene.q) <= 20_000
    assert np.array_equal(scene.blocks[0], scene.lens)
    for it in range(JUMP):
        assert np.array_equal(scene.blocks[it], scene.lens), it
    for it in range(JUMP, len(scene.poses)):  # one site further along x
        assert np.array_equal(scene.blocks[it][:-1], scene.lens[1:]), it
    for blocks in (scene.blocks[0], scene.blocks[JUMP]):
        assert set(REQUIRED) <= set(blocks.tolist())
    runs = scene.lens.reshape(-1, 64)
    for r, (pos, L) in enumerate(SPECIAL):
        if pos is None:
            assert (runs[r] == 0).all()
        else:
            assert runs[r][pos] == L and runs[r].sum() == L
    for r, L in enumerate(REQUIRED + EXTRA, len(SPECIAL)):
        assert runs[r].max() == L
    for G in (1, 2, 4, 8):
        lg = {-(-int(L) // G) for L in scene.lens.reshape(-1, 64 // G).max(1)}
        assert {0, 1, 4, 5, 8, 9} <= lg, (G, sorted(lg))
        assert {x % 8 for x in lg} == set(range(8)), (G, sorted(lg))
    assert (scene.lens[scene.lens > 0] < 8).any()  # lists shorter than a group


def _run(ctx, scene, **opts):
    from pointcloudprocess_amd import ops
    index = ops.GridIndex(ctx, torch.from_numpy(scene.tgt).to(ctx.device), cell_size=H)
    icp = ops.ICP(index, torch.from_numpy(scene.q).to(ctx.device))
    icp.set_options(**opts)
    beta, searched = [], []
    try:
        for it, T in enumerate(scene.poses):
            tag = f"{opts} launch {it}"
            acc, ci, cd = icp.step(T, RMAX, corr=True)
            gi, gd = ci.cpu().numpy(), cd.cpu().numpy()
            ei, ed = scene.corr[it]
            bad = np.flatnonzero(gi != ei)
            assert len(bad) == 0, (f"{tag}: {len(bad)} mismatching correspondences, list lengths "
                                   f"{sorted(set(scene.blocks[it][bad].tolist()))[:20]}")
            assert np.array_equal(gd[ei >= 0], ed[ei >= 0]), f"{tag}: d2 differs"
            gacc, eacc = acc.cpu().numpy(), scene.acc[it]
            assert gacc[0] == eacc[0], f"{tag}: {gacc[0]} pairs, oracle {eacc[0]}"
            scale = np.abs(eacc[:23]).max()
            assert np.allclose(gacc[:23], eacc[:23], rtol=1e-7, atol=1e-8 * scale), tag
            beta.append(icp.last_lookahead()[0])
            searched.append(icp.last_searched())
    finally:
        icp.close()
        index.close()
    return beta, searched


@pytest.mark.parametrize("wide", [False, True], ids=["cache12", "cache16"])
@pytest.mark.parametrize("lanes_list", [1, 2, 4, 8])
@pytest.mark.parametrize("lanes_first", [1, 2, 4, 8])
def test_every_tail_equals_oracle(ctx, scene, lanes_first, lanes_list, wide):
    """Both forms of the scan at every lanes-per-query count and both cache record forms: the plain
    form at launches 0 and 1, the look-ahead form from launch 2 on (beta > 0 on some launch; the
    jump launch scans every list again)."""
    beta, searched = _run(ctx, scene, oct_lanes_first=lanes_first, oct_lanes_list=lanes_list, wide_cache=wide)
    n = len(scene.q)
    print("searched:", searched, "beta:", " ".join(f"{b:.3f}" for b in beta))
    assert beta[0] == 0.0 and beta[1] == 0.0 and max(beta[2:JUMP]) > 0.0, beta
    assert searched[0] == n and searched[JUMP] == n, searched
    assert all(s > 0 for s in searched), searched  # every launch scanned some lists


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_plain_form_on_every_launch(ctx, scene, lanes):
    """Without the look-ahead the plain form of the scan serves every launch."""
    beta, searched = _run(ctx, scene, oct_lanes_first=lanes, oct_lanes_list=lanes, lookahead=False)
    assert all(b == 0.0 for b in beta), beta
    assert searched[0] == len(scene.q) and searched[JUMP] == len(scene.q), searched
