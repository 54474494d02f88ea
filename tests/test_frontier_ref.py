"""The three restatements of include/tsdf_hip_frontier.h in tests/frontierref.py agree with each other
on seeded random fields and give the known answers of one free 8^3 block in an unknown field;
`FrontierSet.clusters` against a brute-force flood fill.  No library involved — CPU suite."""
import numpy as np
import pytest

import frontierref as fr

F = np.float32
# n_unknown of a face / edge / corner voxel of a free block, per connectivity
KNOWN = {6: (1, 2, 3), 18: (5, 9, 12), 26: (9, 15, 19)}


def surface_class(coords, corner, size=8):
    """How many axes a voxel of the block touches the block's surface on: 0 interior, 1 face,
    2 edge, 3 corner."""
    r = np.asarray(coords, np.int64) - np.asarray(corner, np.int64)
    return ((r == 0) | (r == size - 1)).sum(axis=1)


def random_field(seed, nbz=2, nby=2, nbx=3, lo=(-8, 8, -16)):
    """A dense 8-aligned field with missing bricks, W in {0, 1, 3} and S uniform in [-1, 1]."""
    rng = np.random.default_rng(seed)
    shape = (8 * nbz, 8 * nby, 8 * nbx)
    S = rng.uniform(-1.0, 1.0, shape).astype(F)
    W = rng.choice(np.array([0, 1, 3], F), shape, p=[0.3, 0.4, 0.3])
    for z in range(nbz):
        for y in range(nby):
            for x in range(nbx):
                if rng.random() < 0.33:
                    W[8 * z:8 * z + 8, 8 * y:8 * y + 8, 8 * x:8 * x + 8] = 0
    S[W == 0] = 0.25  # what an unobserved voxel holds does not matter
    return S, W, np.asarray(lo, np.int64)


def grown(S, W, flo, lo, hi, bg=0.0):
    """The field's voxels lo - 1 .. hi as query_dense would read them (background outside)."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    n = hi - lo + 2
    gs, gw = np.full(tuple(n[::-1]), bg, F), np.zeros(tuple(n[::-1]), F)
    fhi = flo + np.array(S.shape[::-1])
    a, b = np.maximum(lo - 1, flo), np.minimum(hi + 1, fhi)
    if np.all(b > a):
        src = tuple(slice(int(a[k] - flo[k]), int(b[k] - flo[k])) for k in (2, 1, 0))
        dst = tuple(slice(int(a[k] - lo[k] + 1), int(b[k] - lo[k] + 1)) for k in (2, 1, 0))
        gs[dst], gw[dst] = S[src], W[src]
    return gs, gw


def same(a, b):
    fr.assert_same((a.coords, a.n_unknown, a.dir), b)
    for k in ("n_frontier_bricks", "n_voxels", "n_free"):
        assert a.counts[k] == b.counts[k]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_three_restatements_agree(seed):
    S, W, flo = random_field(seed)
    fhi = flo + np.array(S.shape[::-1])
    bricks = fr.bricks_of(S, W, flo)
    boxes = [(flo, fhi), (flo + [3, -2, 5], fhi - [9, 3, -4]), (flo + [9, 9, 9], flo + [10, 10, 10])]
    n = 0
    for lo, hi in boxes:
        for conn in (6, 18, 26):
            for mu in (1, 3, conn):
                for band, mw in ((0.0, 0.0), (0.3, 2.0)):
                    gs, gw = grown(S, W, flo, lo, hi)
                    d = fr.dense(gs, gw, lo, hi, band, mw, conn, mu)
                    s = fr.sparse(*bricks, band, mw, conn, mu, lo, hi, chunk=3)
                    same(s, d)
                    if conn != 18 and mu != 3:
                        same(fr.scalar(gs, gw, lo, hi, band, mw, conn, mu), d)
                    n += d.counts["n_voxels"]
    assert n > 1000  # the fields have frontiers
    # the whole map: no box
    d = fr.dense(*grown(S, W, flo, flo, fhi), flo, fhi, 0.0)
    same(fr.sparse(*bricks, 0.0), d)


@pytest.mark.parametrize("conn", [6, 18, 26])
def test_one_free_block_known_answers(conn):
    corner = np.array([8, -8, 16])
    S, W, flo, fhi = fr.block_field(corner, [8, 8, 8], [(corner, 8)])
    r = fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, conn, 1)
    k = surface_class(r.coords, corner)
    assert r.counts["n_voxels"] == 296 and r.counts["n_free"] == 512
    assert [(k == j).sum() for j in (1, 2, 3)] == [216, 72, 8]
    for j in (1, 2, 3):
        assert set(r.n_unknown[k == j].tolist()) == {KNOWN[conn][j - 1]}
    same(fr.scalar(S, W, flo + 1, fhi - 1, 0.5, 0.0, conn, 1), r)
    same(fr.sparse(*fr.bricks_of(S[2:-2, 2:-2, 2:-2], W[2:-2, 2:-2, 2:-2], corner), 0.5, 0.0,
                   conn, 1), r)
    # the direction points out of the block: at connectivity 6 a face voxel's is its unit offset
    rel = r.coords.astype(np.int64) - corner
    out = (rel == 7).astype(np.int64) - (rel == 0).astype(np.int64)
    if conn == 6:
        assert np.array_equal(r.dir, out)
    else:
        assert np.all(np.sign(r.dir) == out)


def test_min_unknown_keeps_the_edges_and_corners():
    corner = np.array([0, 0, 0])
    S, W, flo, fhi = fr.block_field(corner, [8, 8, 8], [(corner, 8)])
    r = fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, 26, 10)
    assert r.counts["n_voxels"] == 80 and r.counts["n_free"] == 512
    assert np.all(surface_class(r.coords, corner) >= 2)
    # free_band above the block's S: nothing is free
    r = fr.dense(S, W, flo + 1, fhi - 1, 1.5, 0.0, 26, 1)
    assert r.counts["n_voxels"] == 0 and r.counts["n_free"] == 0
    # min_weight above its W: nothing is observed
    assert fr.dense(S, W, flo + 1, fhi - 1, 0.5, 2.0, 26, 1).counts["n_free"] == 0


def test_a_box_cutting_the_block_keeps_the_voxels_inside_it():
    corner = np.array([-8, 0, 8])
    S, W, flo, fhi = fr.block_field(corner, [8, 8, 8], [(corner, 8)])
    full = fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, 18, 1)
    lo, hi = corner + [3, -1, 0], corner + [9, 5, 6]
    gs, gw = grown(S, W, flo, lo, hi)
    cut = fr.dense(gs, gw, lo, hi, 0.5, 0.0, 18, 1)
    inside = np.all((full.coords >= lo) & (full.coords < hi), axis=1)
    assert 0 < inside.sum() < 296
    assert np.array_equal(cut.coords, full.coords[inside])
    assert np.array_equal(cut.n_unknown, full.n_unknown[inside])  # neighbours are read outside it
    assert np.array_equal(cut.dir, full.dir[inside])
    assert cut.counts["n_free"] == 5 * 5 * 6


def flood_fill(coords):
    """Connected components under 26-connectivity, brute force: a list of sorted index lists."""
    cells = {tuple(c): i for i, c in enumerate(np.asarray(coords).tolist())}
    seen, comps = set(), []
    for start in cells:
        if start in seen:
            continue
        seen.add(start)
        stack, comp = [start], []
        while stack:
            c = stack.pop()
            comp.append(cells[c])
            for dx, dy, dz in fr.OFFSETS:
                q = (c[0] + dx, c[1] + dy, c[2] + dz)
                if q in cells and q not in seen:
                    seen.add(q)
                    stack.append(q)
        comps.append(sorted(comp))
    return comps


def set_of(ref, vs=0.1):
    from tsdf_map import FrontierSet
    return FrontierSet(ref.coords, ref.n_unknown, ref.dir, ref.counts, vs)


def check_clusters(ref, min_voxels=1):
    s = set_of(ref)
    got = s.clusters(min_voxels)
    want = [c for c in flood_fill(ref.coords) if len(c) >= min_voxels]

    def first(idx):  # the smallest voxel in (z, y, x)
        return min(tuple(ref.coords[i][::-1].tolist()) for i in idx)

    want.sort(key=lambda c: (-len(c), first(c)))
    assert [c.indices.tolist() for c in got] == want
    for c in got:
        pts = ref.coords[c.indices].astype(np.float64)
        assert c.size == len(c.indices)
        assert np.allclose(c.centroid, (pts.mean(axis=0) + 0.5) * 0.1)
        assert c.lo.tolist() == pts.min(axis=0).tolist()
        assert c.hi.tolist() == (pts.max(axis=0) + 1).tolist()
        d = ref.dir[c.indices].astype(np.float64).sum(axis=0)
        n = np.linalg.norm(d)
        assert np.allclose(c.mean_direction, d / n if n > 0 else 0.0)
    return got


def test_clusters_against_a_flood_fill():
    corner = np.array([8, -8, 16])
    S, W, flo, fhi = fr.block_field(corner, [8, 8, 8], [(corner, 8)])
    one = fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, 26, 1)
    got = check_clusters(one)
    assert len(got) == 1 and got[0].size == 296
    assert np.allclose(got[0].mean_direction, 0.0)  # a closed shell: the directions cancel
    # with min_unknown 10 at 26 the 12 edges stay connected through the corners
    assert len(check_clusters(fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, 26, 10))) == 1
    # two separated blocks, one of them smaller, and a third that touches the first by a corner
    lo = np.array([0, 0, 0])
    S, W, flo, fhi = fr.block_field(lo, [40, 16, 16], [([0, 0, 0], 8), ([20, 3, 2], 5),
                                                       ([8, 8, 8], 3)])
    two = fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, 6, 1)
    got = check_clusters(two)
    assert [c.size for c in got] == [296 + 26, 98]
    assert [c.size for c in check_clusters(two, min_voxels=99)] == [296 + 26]
    for seed in (4, 5):
        S, W, flo = random_field(seed)
        fhi = flo + np.array(S.shape[::-1])
        r = fr.dense(*grown(S, W, flo, flo, fhi), flo, fhi, 0.0, 0.0, 6, 2)
        assert len(check_clusters(r)) > 3
    assert set_of(fr.Ref(np.zeros((0, 3)), [], np.zeros((0, 3)), 0)).clusters() == []


def test_the_set_helpers():
    corner = np.array([-8, 0, 8])
    S, W, flo, fhi = fr.block_field(corner, [16, 8, 8], [(corner, 8), (corner + [8, 0, 0], 8)])
    r = fr.dense(S, W, flo + 1, fhi - 1, 0.5, 0.0, 6, 1)
    s = set_of(r, vs=0.05)
    assert len(s) == r.counts["n_voxels"] and s.counts == r.counts
    assert np.array_equal(s.points, (r.coords.astype(np.float64) + 0.5) * 0.05)
    d = s.directions
    nz = np.any(r.dir != 0, axis=1)
    assert np.allclose(np.linalg.norm(d[nz], axis=1), 1.0) and np.all(d[~nz] == 0)
    bricks, start, length = s.brick_runs()
    assert bricks.tolist() == [[-1, 0, 1], [0, 0, 1]] and start.tolist() == [0, length[0]]
    assert length.sum() == len(s)
    for b, a, n in zip(bricks, start, length):
        assert np.all(r.coords[a:a + n] >> 3 == b)
    with pytest.raises(ValueError):
        from tsdf_map import FrontierSet
        FrontierSet(r.coords, r.n_unknown[:-1], r.dir, r.counts, 0.05)
