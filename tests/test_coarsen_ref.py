"""tests/coarsenref.py, the numpy restatement of include/tsdf_hip_coarsen.h that the GPU tests
compare against, held to answers known beforehand: single voxels and octets by hand, the order of
the children, negative and odd coordinates, both thresholds, and two analytic fields with bounds
derived here from the arithmetic.  CPU suite."""
import numpy as np
import pytest

import coarsenref as cr

F = np.float32
U = 2.0 ** -24  # fp32 unit roundoff
BG = F(0.3)
EMPTY = cr.empty_bricks()


def octet(V, values, weights):
    """The bricks holding the eight children of coarse voxel V: child k = a + 2 b + 4 c."""
    V = np.asarray(V, np.int64)
    vox = [2 * V + np.array([k & 1, (k >> 1) & 1, k >> 2]) for k in range(8)]
    return cr.bricks_of(vox, values, weights, BG)


def coarse_value(exp, V):
    V = np.asarray(V, np.int64)
    row = np.nonzero(np.all(exp.coords == (V >> 3), axis=1))[0]
    assert row.size == 1
    x, y, z = V & 7
    return exp.sdf[row[0], z, y, x], exp.weight[row[0], z, y, x]


def test_one_voxel():
    src = cr.bricks_of([[5, -3, 9]], [0.07], [4.0], BG)
    exp = cr.coarsen(EMPTY, src, BG)
    assert exp.counts == dict(src_bricks=1, parent_bricks=1, touched_bricks=1, new_bricks=1,
                              coarse_voxels=1, overlap_voxels=0, child_voxels=1)
    assert exp.coords.tolist() == [[0, -1, 0]] and exp.voxels.tolist() == [[2, -2, 4]]
    s, w = coarse_value(exp, (2, -2, 4))
    # s = fl(fl(0.07 * 4) / 4), w = 4 / 1
    assert s == F(F(F(0.07) * F(4.0)) / F(4.0)) and w == F(4.0)
    assert (exp.weight > 0).sum() == 1
    assert np.all(exp.sdf[exp.weight == 0] == BG)


def test_a_full_octet_of_equal_voxels_keeps_its_value():
    for s0, w0 in ((0.125, 2.0), (-0.2, 1.0), (0.07, 3.0)):
        exp = cr.coarsen(EMPTY, octet((3, 1, -2), [s0] * 8, [w0] * 8), BG)
        s, w = coarse_value(exp, (3, 1, -2))
        assert w == F(w0) and exp.counts["child_voxels"] == 8 and exp.counts["coarse_voxels"] == 1
        if s0 == 0.125:  # every partial sum is exact
            assert s == F(s0)
        else:
            assert abs(float(s) - float(F(s0))) <= 10 * U * abs(s0)


def test_the_children_are_summed_in_the_order_of_k():
    """Unit weights, one child of 2^24 among seven of 1: fp32 drops every 1 added after the large
    child (ties to even) and keeps those added before it."""
    big = 2.0 ** 24
    for k_big, want in ((0, big / 8), (7, (big + 8) / 8),
                        # k = 1 is the child (a, b, c) = (1, 0, 0): 1 + 2^24 -> 2^24, and stays
                        (1, big / 8),
                        # k = 4 is (0, 0, 1): 1 + 1 + 1 + 1 + 2^24 exact, then 3 dropped ones
                        (4, (big + 4) / 8)):
        vals = [1.0] * 8
        vals[k_big] = big
        exp = cr.coarsen(EMPTY, octet((0, 0, 0), vals, [1.0] * 8), BG)
        s, w = coarse_value(exp, (0, 0, 0))
        assert float(s) == want and w == F(1.0), (k_big, float(s), want)
    # and the voxel that k = 1 names is x + 1, not z + 1
    src = cr.bricks_of([[0, 0, 0], [1, 0, 0], [0, 0, 1]], [1.0, big, 1.0], [1.0, 1.0, 1.0], BG)
    s, _ = coarse_value(cr.coarsen(EMPTY, src, BG), (0, 0, 0))
    # (1 + 2^24 -> 2^24) + 1 -> 2^24; the x neighbour last would give 1 + 1 + 2^24 = 2^24 + 2
    assert s == F(F(big) / F(3)) and s != F(F(big + 2) / F(3))


def test_negative_and_odd_coordinates():
    # fine voxels -2 and -1 are the children of coarse voxel -1 on every axis
    exp = cr.coarsen(EMPTY, octet((-1, -1, -1), np.arange(8) * 0.01, [1.0] * 8), BG)
    assert exp.coords.tolist() == [[-1, -1, -1]] and exp.voxels.tolist() == [[-1, -1, -1]]
    assert exp.counts["child_voxels"] == 8
    # fine voxel -1 alone, and fine voxel -3 (coarse -2), per axis
    for fine, coarse in ((-1, -1), (-2, -1), (-3, -2), (-16, -8), (-17, -9), (15, 7), (16, 8)):
        for axis in range(3):
            v = [4, 4, 4]
            v[axis] = fine
            exp = cr.coarsen(EMPTY, cr.bricks_of([v], [0.1], [1.0], BG), BG)
            want = [2, 2, 2]
            want[axis] = coarse
            assert exp.voxels.tolist() == [want]
            assert exp.coords.tolist() == [[c >> 3 for c in want]]
    # bricks: the parent of an odd negative brick is the floor
    for B, D in ((-1, -1), (-2, -1), (-3, -2), (1, 0), (3, 1), (-(1 << 20), -(1 << 19)),
                 ((1 << 20) - 1, (1 << 19) - 1)):
        exp = cr.coarsen(EMPTY, cr.bricks_of([[8 * B + 3, 0, 8 * B + 7]], [0.1], [1.0], BG), BG)
        assert exp.coords.tolist() == [[D, 0, D]]


def test_min_children_on_an_octet_of_five():
    w = [1.0, 0.0, 2.0, 0.0, 3.0, 1.0, 0.0, 1.0]
    src = octet((10, -7, 3), [0.1] * 8, w)
    for mc in range(1, 9):
        exp = cr.coarsen(EMPTY, src, BG, min_children=mc)
        if mc <= 5:
            s, wc = coarse_value(exp, (10, -7, 3))
            assert wc == F(F(8.0) / F(5.0)) and exp.counts["child_voxels"] == 5
            assert exp.counts["touched_bricks"] == exp.counts["new_bricks"] == 1
        else:  # nothing valid: no brick
            assert exp.coords.shape[0] == 0 and exp.counts["coarse_voxels"] == 0
            assert exp.counts["touched_bricks"] == 0 and exp.counts["child_voxels"] == 0
        assert exp.counts["src_bricks"] == exp.counts["parent_bricks"] == 1


def test_min_weight_drops_children():
    w = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    s = [0.01 * k for k in range(8)]
    src = octet((0, 0, 0), s, w)
    exp = cr.coarsen(EMPTY, src, BG, min_weight=6.0)
    sc, wc = coarse_value(exp, (0, 0, 0))
    ssw = F(0)
    for k in (5, 6, 7):
        ssw = F(ssw + F(F(s[k]) * F(w[k])))
    assert wc == F(F(21.0) / F(3.0)) and sc == F(ssw / F(21.0))
    assert exp.counts["child_voxels"] == 3
    assert cr.coarsen(EMPTY, src, BG, min_weight=6.0, min_children=4).counts["coarse_voxels"] == 0
    assert cr.coarsen(EMPTY, src, BG, min_weight=8.5).coords.shape[0] == 0
    assert cr.child_histogram(src) == [0] * 7 + [1]
    assert cr.child_histogram(src, 6.0) == [0, 0, 1, 0, 0, 0, 0, 0]


def test_selection_and_fusing_into_a_held_voxel():
    a = cr.bricks_of([[0, 0, 0], [16, 0, 0]], [0.1, 0.2], [2.0, 4.0], BG)  # bricks 0 and 2 in x
    box = ((0, 0, 0), (1, 1, 1))
    ins = cr.coarsen(EMPTY, a, BG, box=box, side="inside")
    out = cr.coarsen(EMPTY, a, BG, box=box, side="outside")
    assert ins.voxels.tolist() == [[0, 0, 0]] and out.voxels.tolist() == [[8, 0, 0]]
    assert ins.counts["src_bricks"] == out.counts["src_bricks"] == 1
    both = cr.coarsen(ins[:3], a, BG, box=box, side="outside")
    cr.assert_same_bricks(both, cr.coarsen(EMPTY, a, BG))
    # an empty box selects nothing inside and everything outside
    assert cr.coarsen(EMPTY, a, BG, box=((0, 0, 0), (0, 5, 5))).counts["src_bricks"] == 0
    assert cr.coarsen(EMPTY, a, BG, box=((0, 0, 0), (0, 5, 5)), side="outside").counts["src_bricks"] == 2
    # rule 6 into a held voxel: (S W + s w) / (W + w), and the cap
    dst = cr.bricks_of([[0, 0, 0]], [0.3], [1.0], BG)
    exp = cr.coarsen(dst, a, BG, box=box)
    s, w = coarse_value(exp, (0, 0, 0))
    sv = F(F(F(0.1) * F(2.0)) / F(2.0))
    assert w == F(3.0) and s == F(F(F(F(0.3) * F(1.0)) + F(sv * F(2.0))) / F(3.0))
    assert exp.counts["overlap_voxels"] == 1 and exp.counts["new_bricks"] == 0
    _, w = coarse_value(cr.coarsen(dst, a, BG, box=box, max_weight=2.5), (0, 0, 0))
    assert w == F(2.5)


def test_a_linear_field_is_reproduced_at_the_coarse_centre():
    """S = g . c + d at the fine centres, equal weights 3 (every partial weight sum k * 3 is
    exact), full octets: in real arithmetic the mean of the eight children is the field at their
    centroid, the coarse centre.  In fp32, with M = max |S_c| of the octet: the rounding of each
    child's value (1), of its product with W (1), of the seven additions to partial sums of at
    most 8 M W (7 of 8 u M W each, an eighth after the division), and of the division (1): ten
    roundings of at most u M each, plus their second-order terms."""
    vs = 0.1
    g, d = np.array([0.31, -0.17, 0.23]), 0.05
    r = np.arange(-8, 8)
    fine = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    vals = ((fine + 0.5) * vs) @ g + d
    exp = cr.coarsen(EMPTY, cr.bricks_of(fine, vals, np.full(len(fine), 3.0), BG), BG,
                     min_children=8)
    assert exp.counts["coarse_voxels"] == 8 ** 3 and exp.counts["child_voxels"] == 8 ** 4
    V = exp.voxels
    want = ((V + 0.5) * (2 * vs)) @ g + d
    got = np.array([coarse_value(exp, v)[0] for v in V], np.float64)
    M = np.abs(vals).max()
    bound = 10 * U * M * (1 + 1e-5) + 1e-13
    assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
    assert np.abs(got - want).max() > 0  # fp32 is at work
    assert all(coarse_value(exp, v)[1] == F(3.0) for v in V[::37])


def test_a_spheres_distance_field_within_the_curvature_bound():
    """S = |c - c0| - R, untruncated, unit weights, full octets.  The mean over the eight centres
    at (+-vs/2)^3 around p is S(p) + (vs/2)^2 / 2 * trace(Hessian) + O(vs^4) = S(p) + vs^2 / (4 r):
    |s - S(centre)| <= vs^2 / (2 r_min), the factor 2 covering the higher orders (and fp32)."""
    vs, R = 0.1, 2.0
    c0 = np.array([0.13, -0.21, 0.37])
    r = np.arange(10, 42)  # x from 1 m to 4.2 m: every centre at least 1 m from c0 ...
    o = np.arange(-8, 8)
    fine = np.stack(np.meshgrid(r, o, o, indexing="ij"), -1).reshape(-1, 3)
    dist = np.linalg.norm((fine + 0.5) * vs - c0, axis=1)
    exp = cr.coarsen(EMPTY, cr.bricks_of(fine, dist - R, np.ones(len(fine)), BG), BG,
                     min_children=8)
    V = exp.voxels
    assert V.shape[0] == 16 * 8 * 8
    rc = np.linalg.norm((V + 0.5) * (2 * vs) - c0, axis=1)
    r_min = rc.min()
    assert 0.8 <= r_min <= 1.2
    got = np.array([coarse_value(exp, v)[0] for v in V], np.float64)
    err = np.abs(got - (rc - R))
    assert err.max() <= vs * vs / (2 * r_min), (err.max(), vs * vs / (2 * r_min))
    # the leading term is there: near r_min the error is about vs^2 / (4 r)
    near = np.argmin(rc)
    assert 0.5 * vs * vs / (4 * r_min) <= err[near]


def test_the_counts_add_up_over_a_partition():
    rng = np.random.default_rng(7)
    vox = rng.integers(-12, 12, (6000, 3))
    vox = np.unique(vox, axis=0)
    src = cr.bricks_of(vox, rng.uniform(-0.3, 0.3, len(vox)), rng.integers(1, 6, len(vox)), BG)
    dv = np.unique(rng.integers(-6, 6, (500, 3)), axis=0)
    dst = cr.bricks_of(dv, np.full(len(dv), 0.1), np.ones(len(dv)), BG)
    box = ((-2, -1, -3), (3, 2, 1))
    whole = cr.coarsen(dst, src, BG, min_children=2, min_weight=2.0)
    a = cr.coarsen(dst, src, BG, 2, 2.0, box, "inside")
    b = cr.coarsen(a[:3], src, BG, 2, 2.0, box, "outside")
    cr.assert_same_bricks(b, whole)
    for k in ("src_bricks", "coarse_voxels", "child_voxels", "overlap_voxels"):
        assert a.counts[k] + b.counts[k] == whole.counts[k] > 0, k
    assert whole.counts["parent_bricks"] <= a.counts["parent_bricks"] + b.counts["parent_bricks"]


def test_expected_is_not_changed_by_a_later_call():
    src = cr.bricks_of([[1, 1, 1]], [0.1], [1.0], BG)
    dst = cr.bricks_of([[0, 0, 0]], [0.2], [1.0], BG)
    keep = [a.copy() for a in dst]
    cr.coarsen(dst, src, BG)
    for a, b in zip(dst, keep):
        assert np.array_equal(a, b)
    with pytest.raises(AssertionError):
        cr.assert_same_bricks(cr.coarsen(dst, src, BG), dst)
