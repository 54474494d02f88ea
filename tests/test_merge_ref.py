"""tests/mergeref.py, the numpy restatement of include/tsdf_hip_merge.h the GPU tests compare with,
held to what the rules say on fields small enough to reason about -- on the CPU, on oracle volumes
(import_bricks builds the fields, export_bricks / export_voxels read them)."""
import numpy as np
import pytest

import mergeref as mr
import oracle
import sampleref as sr

F = np.float32
VS, TAU = sr.VOXEL_SIZE, sr.SDF_TRUNC
U = 2.0 ** -24  # fp32 unit roundoff
GENERAL = mr.rigid((10.0, -20.0, 30.0), (1.234, -2.345, 0.456))
EMPTY = (np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), F), np.zeros((0, 8, 8, 8), F))


def volume(sem="vdbfusion_f64", **kw):
    return oracle.OracleTSDFVolume(VS, TAU, semantics=sem, **kw)


def bricks_of(voxels, sdf, weight, bg):
    """(coords, sdf, weight) bricks holding the given voxels, the rest (bg, 0)."""
    v = np.asarray(voxels, np.int64).reshape(-1, 3)
    b, inv = np.unique(v >> 3, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    S = np.full((b.shape[0], 8, 8, 8), F(bg), F)
    W = np.zeros((b.shape[0], 8, 8, 8), F)
    S[inv, v[:, 2] & 7, v[:, 1] & 7, v[:, 0] & 7] = np.asarray(sdf, F)
    W[inv, v[:, 2] & 7, v[:, 1] & 7, v[:, 0] & 7] = np.asarray(weight, F)
    return b.astype(np.int32), S, W


def filled(vol, voxels, sdf, weight):
    vol.import_bricks(*bricks_of(voxels, sdf, weight, mr.background(vol)))
    return vol


def observed(exp):
    """export_voxels of an Expected: (ijk, S, W) sorted (z, y, x)."""
    from tsdf_map import bricks_to_voxels
    return bricks_to_voxels(exp.coords, exp.sdf, exp.weight)


@pytest.fixture(scope="module")
def scan_map(scan0):
    """One scan, cropped to a few bricks: a field with ragged borders and varied weights."""
    pts, org = scan0
    v = volume()
    v.integrate(np.ascontiguousarray(pts[::2]), org)
    c, s, w = v.export_bricks()
    keep = np.all((c >= (6, -11, -7)) & (c < (15, -2, 2)), axis=1)
    v.close()
    out = volume()
    out.import_bricks(c[keep], s[keep], w[keep])
    assert out.num_bricks() >= 10
    yield out
    out.close()


def test_rule_1_inverse_pose_arithmetic():
    m = mr.inverse_pose(GENERAL)
    R, t = GENERAL[:, :3], GENERAL[:, 3]
    assert m.dtype == F and m.shape == (3, 4)
    assert np.array_equal(m[:, :3], R.T.astype(F))
    for r in range(3):
        want = -((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2])
        assert m[r, 3] == F(want)
    # a 4x4 pose is its first three rows; the exact quarter turn has an exact inverse
    T4 = np.vstack([mr.rot_z90((1.0, 2.0, 0.5)), [0, 0, 0, 1]])
    assert np.array_equal(mr.inverse_pose(T4),
                          np.array([[0, 1, 0, -2], [-1, 0, 0, 1], [0, 0, 1, -0.5]], F))
    # rule 2: the centre and the preimage in the stated order
    v = np.array([[3, -7, 100], [-(1 << 23) + 1, (1 << 23) - 1, 0]])
    c = mr.centres(v, VS)
    assert np.array_equal(c[0], np.array([F(3.5) * F(VS), F(-6.5) * F(VS), F(100.5) * F(VS)], F))
    q = mr.preimage(m, v, VS)
    x, y, z = c[0]
    assert q[0, 1] == F(F(F(m[1, 0] * x + m[1, 1] * y) + m[1, 2] * z) + m[1, 3])


def test_nearest_identity_reproduces_the_source(scan_map):
    src = scan_map.export_voxels()
    exp = mr.merge(EMPTY, src, mr.rigid(), VS, F(TAU), sr.NEAREST)
    mr.assert_same_bricks(scan_map.export_bricks(), exp)
    n = src[0].shape[0]
    assert n >= 1000
    assert exp.counts == dict(touched_bricks=scan_map.num_bricks(), new_bricks=scan_map.num_bricks(),
                              merged_voxels=n, overlap_voxels=0)


def test_nearest_whole_voxel_shift_reproduces_the_source_shifted(scan_map):
    ijk, s, w = scan_map.export_voxels()
    shift = np.array([3, -5, 1])
    T = mr.rigid(t=shift * float(F(VS)))
    # (the header's condition: no q rounds across a voxel face)
    q = mr.preimage(mr.inverse_pose(T), ijk.astype(np.int64) + shift, VS)
    assert np.array_equal(np.floor((q * (F(1) / F(VS))).astype(F)).astype(np.int64), ijk)
    exp = mr.merge(EMPTY, (ijk, s, w), T, VS, F(TAU), sr.NEAREST)
    gi, gs, gw = observed(exp)
    assert np.array_equal(gi, ijk + shift)
    assert np.array_equal(gs.view(np.uint32), s.view(np.uint32))
    assert np.array_equal(gw.view(np.uint32), w.view(np.uint32))
    assert exp.counts["merged_voxels"] == ijk.shape[0]


def test_trilinear_identity_keeps_only_the_fully_observed_cubes(scan_map):
    """Rule 7 on a real scan: under the identity q is the voxel's own centre up to rounding, the
    cube is the voxel's own or a neighbour's, and only a share of the voxels survives."""
    src = scan_map.export_voxels()
    exp = mr.merge(EMPTY, src, mr.rigid(), VS, F(TAU), sr.TRILINEAR)
    n, m = src[0].shape[0], exp.counts["merged_voxels"]
    assert 0 < m < n // 2, (m, n)
    have = {tuple(v) for v in src[0]}
    assert all(tuple(v) in have for v in exp.voxels)
    assert exp.counts["touched_bricks"] == exp.coords.shape[0] <= scan_map.num_bricks()


def linear_field(n, d, bricks=(-2, 2)):
    """Voxels of the bricks [lo, hi)^3 whose S = n . x - d lies inside the truncation band."""
    r = np.arange(bricks[0] * 8, bricks[1] * 8)
    v = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    x = (v + 0.5) * float(F(VS))
    s = x @ n - d
    keep = np.abs(s) < 0.95 * TAU
    return v[keep], s[keep].astype(F)


def test_a_linear_field_stays_linear_under_a_general_pose():
    """S = n . x - d moved by (R, t) is n' . c - d' with n' = R n, d' = d + n' . t; the trilinear
    interpolant of a linear field is exact in exact arithmetic, so what is left is rounding.

    The bound, from the fp32 unit roundoff u = 2^-24 and the operation count.  M = the largest
    coordinate magnitude in play (metres).  Position: c carries one rounding, each product of rule
    2 two more, the three additions three, so |dq| <= 6 u (sqrt(3) M + M) per axis; the index
    coordinate q * inv - 0.5 three more roundings on a number of magnitude <= M / vs, i.e.
    3 u M in metres.  A position error e per axis moves a unit-gradient linear field by at most
    sqrt(3) e.  Values: the stored S is rounded once (u tau); a lerp is three operations on
    numbers bounded by 2 tau, and three levels of lerps follow one another (convex combinations do
    not amplify what they are given): 9 * 2 u tau.  Measured maximum: see DESIGN.md §15."""
    n = np.array([0.48, -0.6, 0.64])
    assert abs(np.linalg.norm(n) - 1.0) < 1e-12
    d = 0.123
    v, s = linear_field(n, d)
    src = filled(volume(), v, s, np.ones(len(v), F))
    R, t = GENERAL[:, :3], GENERAL[:, 3]
    n2 = R @ n
    d2 = d + n2 @ t
    worst = {}
    for name, T in (("general", GENERAL), ("identity", mr.rigid())):
        exp = mr.merge(EMPTY, src.export_voxels(), T, VS, F(TAU), sr.TRILINEAR)
        gi, gs, gw = observed(exp)
        assert gi.shape[0] >= 2000 and np.all(gw == 1.0)
        c = (gi + 0.5) * float(F(VS))
        want = c @ (n2 if name == "general" else n) - (d2 if name == "general" else d)
        M = max(np.abs(c).max(), np.abs(t).max(), 16 * VS)
        e_pos = 6 * U * (np.sqrt(3) + 1) * M + 3 * U * M
        bound = np.sqrt(3) * e_pos + 19 * U * TAU
        err = np.abs(gs.astype(np.float64) - want).max()
        worst[name] = (err, bound)
        assert err <= bound, (name, err, bound)
        assert bound < 1e-3 * VS  # the bound means something: a thousandth of a voxel
    print("linear field: max |error| / bound:", worst)
    src.close()


def test_one_observed_voxel():
    """Nearest moves it; trilinear merges nothing and allocates nothing."""
    src = ([[5, -3, 9]], F([0.07]), F([4.0]))
    T = mr.rigid(t=(2 * float(F(VS)), 0.0, -float(F(VS))))
    exp = mr.merge(EMPTY, src, T, VS, F(TAU), sr.NEAREST)
    gi, gs, gw = observed(exp)
    assert gi.tolist() == [[7, -3, 8]] and gs[0] == F(0.07) and gw[0] == F(4.0)
    assert exp.counts == dict(touched_bricks=1, new_bricks=1, merged_voxels=1, overlap_voxels=0)
    assert exp.coords.tolist() == [[0, -1, 1]]
    assert np.all(exp.sdf.reshape(-1)[exp.weight.reshape(-1) == 0] == F(TAU))  # a new brick's rest
    for pose in (T, mr.rigid(), GENERAL):
        exp = mr.merge(EMPTY, src, pose, VS, F(TAU), sr.TRILINEAR)
        assert exp.coords.shape[0] == 0 and not any(exp.counts.values())
    # under a rotation the voxel's image may cover one, two or no destination centres
    exp = mr.merge(EMPTY, src, GENERAL, VS, F(TAU), sr.NEAREST)
    assert 0 <= exp.counts["merged_voxels"] <= 3


def cube_voxels():
    """A fully observed 2 x 2 x 2 cube straddling the brick corner at (8, 8, 8): 8 bricks."""
    v = np.array([[7 + dx, 7 + dy, 7 + dz] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    return v, F(np.linspace(-0.2, 0.2, 8)), F(np.arange(1, 9))


def test_the_cube_across_a_brick_corner():
    v, s, w = cube_voxels()
    assert np.unique(v >> 3, axis=0).shape[0] == 8
    # identity: q is a voxel's own centre up to rounding; the cube based at (7, 7, 7) covers index
    # coordinates [7.5, 8.5)^3, so only the centre of (8, 8, 8) -- 8.5 exactly in real arithmetic,
    # and whatever fp32 makes of it -- can fall inside.  Assert what the rules give:
    exp = mr.merge(EMPTY, (v, s, w), mr.rigid(), VS, F(TAU), sr.TRILINEAR)
    q = mr.preimage(mr.inverse_pose(mr.rigid()), v, VS)
    u = ((q * (F(1) / F(VS))).astype(F) - F(0.5)).astype(F)
    inside = np.all(np.floor(u) == 7, axis=1)
    assert exp.counts["merged_voxels"] == int(inside.sum()) <= 8
    assert np.array_equal(exp.voxels, v[inside])
    # a shift of half a voxel along every axis puts the preimage of (8, 8, 8)'s centre at the
    # cube's centre: exactly one voxel, the interpolant at f ~ 0.5 is the mean of the 8 corners,
    # the weight the cube's minimum
    h = 0.5 * float(F(VS))
    exp = mr.merge(EMPTY, (v, s, w), mr.rigid(t=(h, h, h)), VS, F(TAU), sr.TRILINEAR)
    gi, gs, gw = observed(exp)
    assert gi.tolist() == [[8, 8, 8]] and gw[0] == 1.0
    assert abs(float(gs[0]) - float(s.astype(np.float64).mean())) < 1e-6
    assert exp.counts == dict(touched_bricks=1, new_bricks=1, merged_voxels=1, overlap_voxels=0)
    # nearest + identity: all 8 voxels, all 8 bricks
    exp = mr.merge(EMPTY, (v, s, w), mr.rigid(), VS, F(TAU), sr.NEAREST)
    assert exp.counts["merged_voxels"] == 8 and exp.counts["new_bricks"] == 8


def test_min_weight():
    v, s, w = cube_voxels()
    for mw, n in ((0.0, 8), (1.0, 8), (4.5, 4), (8.0, 1), (8.5, 0)):
        exp = mr.merge(EMPTY, (v, s, w), mr.rigid(), VS, F(TAU), sr.NEAREST, min_weight=mw)
        assert exp.counts["merged_voxels"] == n
        assert exp.coords.shape[0] == n  # one brick each, none left empty
    h = 0.5 * float(F(VS))
    for mw, n in ((1.0, 1), (1.5, 0)):  # trilinear: every corner must pass
        exp = mr.merge(EMPTY, (v, s, w), mr.rigid(t=(h, h, h)), VS, F(TAU), sr.TRILINEAR,
                       min_weight=mw)
        assert exp.counts["merged_voxels"] == n and exp.coords.shape[0] == n


@pytest.mark.parametrize("sem", ["vdbfusion_f64", "voxblox"])
def test_the_fuse_branches_and_the_weight_cap(sem):
    """The copy where W == 0 against the weighted mean, on a destination that holds one of the two
    voxels; Voxblox caps the fused weight at max_weight, the copy is not capped."""
    dst = filled(volume(sem, max_weight=5.0), [[1, 2, 3], [6, 6, 6]], F([0.1, -0.05]), F([3.0, 0.0]))
    bg = mr.background(dst)
    src = ([[1, 2, 3], [2, 2, 3]], F([-0.2, 0.25]), F([4.0, 7.0]))
    exp = mr.merge(dst.export_bricks(), src, mr.rigid(), VS, bg, sr.NEAREST,
                   max_weight=mr.weight_cap(dst))
    assert exp.counts == dict(touched_bricks=1, new_bricks=0, merged_voxels=2, overlap_voxels=1)
    S, W = exp.sdf[0], exp.weight[0]
    want = F(F(F(F(0.1) * F(3.0)) + F(F(-0.2) * F(4.0))) / F(7.0))
    assert S[3, 2, 1] == want
    assert W[3, 2, 1] == (F(5.0) if sem == "voxblox" else F(7.0))
    assert S[3, 2, 2] == F(0.25) and W[3, 2, 2] == F(7.0)  # the copy: as it is, above the cap
    assert S[6, 6, 6] == F(bg) and W[6, 6, 6] == 0.0  # (an import takes no unobserved voxel)
    # the same through the library's own import: merging the source's bricks where they sit
    dst.import_bricks(*bricks_of(src[0], src[1], src[2], bg))
    mr.assert_same_bricks(dst.export_bricks(), exp)
    dst.close()


def test_voxels_outside_the_index_domain_are_dropped():
    lim = 1 << 23
    v = np.array([[lim - 2, 0, 0], [lim - 1, 0, 0], [-lim + 1, 5, 5]])
    src = (v, F([0.1, 0.2, -0.1]), F([1.0, 2.0, 3.0]))
    exp = mr.merge(EMPTY, src, mr.rigid(), VS, F(TAU), sr.NEAREST, reach=3)
    cand = mr.candidate_voxels(v, mr.rigid(), VS, reach=3)
    assert np.all(np.abs(cand) < lim) and cand.shape[0] > 0
    assert np.all(np.abs(exp.voxels) < lim)
    assert np.all((exp.coords >= mr.BRICK_MIN) & (exp.coords < mr.BRICK_MAX))
